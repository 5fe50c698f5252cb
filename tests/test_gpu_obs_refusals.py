"""GPU: every call the seven observation entry points refuse -- fl_step_obs, fl_obs_cutils, fl_obs_cutils_policy, fl_obs_cutils_handles,
fl_obs_cutils_tree, fl_obs_tree, fl_obs_tree_handles -- and the handle lists the two *_handles functions accept.

The calls go through hip_backend.lib() (the Python wrapper would stop some of them first).  A refused call returns its FL_ERR_* code with a
message that starts with the called function's name, launches nothing (state(), state_aux() as before: for fl_step_obs the envs have not
advanced) and leaves the handle's record of its last observation launch (last_obs_launch()) as it was.  One env of cfg1_uniform; one env of
threeway_cfg2 (a cell with three transitions in one direction) for depth 4."""
import ctypes as C

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

FL_ERR_ARG = 1
CUTILS_OUT = ("attr", "forest", "adjacency", "node_order", "edge_order", "valid", "props")
NAMES = ("fl_step_obs", "fl_obs_cutils", "fl_obs_cutils_policy", "fl_obs_cutils_handles", "fl_obs_cutils_tree", "fl_obs_tree", "fl_obs_tree_handles")
WITH_CUTILS = NAMES[:5]
SWAP = (1, 0)              # the shortest list that is a permutation of 0 .. n-1 and not all the agents in order


class _Handle:
    """a batch of one env with output buffers for the LARGEST request any case names (65 nodes, depth 5): a call that a broken check lets
    through still writes inside them"""

    def __init__(self, fixture):
        import torch
        from flatland_marl_amd.hip_backend import BatchedRailEnv
        self.env = env = BatchedRailEnv([util.static_of(util.load(fixture))])
        assert env.A >= 3
        for t in range(3):
            env.step_synth(1, 0, 0, auto_reset=False)
        env.obs_cutils()                                     # the record of a real launch: "unchanged" below is not "still empty"
        assert env.last_obs_launch()["mode"] >= 0
        A, N, dev = env.A, 65, env.device
        z = lambda shape, dt: torch.zeros((1, A) + shape, dtype=dt, device=dev)     # noqa: E731
        self.buf = dict(attr=z((83,), torch.float32), forest=z((N, 12), torch.float32), adjacency=z((N - 1, 3), torch.int64),
                        node_order=z((N,), torch.int64), edge_order=z((N - 1,), torch.int64), valid=z((5,), torch.uint8),
                        props=z((3,), torch.float64), tree_out=z((1365, 12), torch.float64))
        self.defaults = dict(max_nodes=31, pred_depth=500, depth=2, tree_pred=30, handles=SWAP, n_handles=None, kind=0,
                             rewards=env.rewards.data_ptr(), dones=env.dones.data_ptr(), done_all=env.done_all.data_ptr(),
                             **{k: v.data_ptr() for k, v in self.buf.items()})

    def call(self, name, **over):
        """(return code, message) of entry point `name` with this handle's valid arguments, `over` replacing some of them"""
        from flatland_marl_amd import hip_backend
        L = hip_backend.lib()
        a = dict(self.defaults, **over)
        cut = [a[k] for k in CUTILS_OUT]
        hs = np.ascontiguousarray(a["handles"], dtype=np.int32) if a["handles"] is not None else None
        hp = hs.ctypes.data_as(C.c_void_p) if hs is not None else None
        n = len(hs) if a["n_handles"] is None else a["n_handles"]
        h, mn, pd = self.env.h, a["max_nodes"], a["pred_depth"]
        if name == "fl_step_obs":
            args = [h, None, 1, 0, a["kind"], a["rewards"], a["dones"], a["done_all"], 0, mn, pd] + cut + [a["depth"], a["tree_pred"], a["tree_out"]]
        elif name in ("fl_obs_cutils", "fl_obs_cutils_policy"):
            args = [h, mn, pd] + cut
        elif name == "fl_obs_cutils_handles":
            args = [h, mn, pd, hp, n] + cut
        elif name == "fl_obs_cutils_tree":
            args = [h, mn, pd] + cut + [a["depth"], a["tree_pred"], a["tree_out"]]
        elif name == "fl_obs_tree":
            args = [h, a["depth"], a["tree_pred"], a["tree_out"]]
        else:
            args = [h, a["depth"], a["tree_pred"], hp, n, a["tree_out"]]
        rc = getattr(L, name)(*args)
        return rc, L.fl_last_error().decode()

    def snapshot(self):
        st, el = self.env.state()
        return st, el, self.env.state_aux(), self.env.last_obs_launch()


@pytest.fixture(scope="module")
def flat():
    return _Handle("cfg1_uniform")


@pytest.fixture(scope="module")
def threeway():
    return _Handle("threeway_cfg2")


def _refused(hd, name, says, **over):
    before = hd.snapshot()
    rc, msg = hd.call(name, **over)
    assert rc == FL_ERR_ARG, (name, over, rc, msg)
    assert msg.startswith(name + ":"), (name, over, msg)
    for s in says:
        assert s in msg, (name, over, msg)
    after = hd.snapshot()
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x, y, err_msg=f"{name} {over}: a refused call changed the envs")
    assert after[3] == before[3], (name, over, "a refused call changed the handle's launch record")
    return msg


def _cases():
    """(entry point, substrings of the message, the arguments that differ from a valid call)"""
    out = []
    for name in WITH_CUTILS:
        out += [(name, ("max_nodes",), dict(max_nodes=3)), (name, ("max_nodes",), dict(max_nodes=65)),
                (name, ("pred_depth",), dict(pred_depth=0)), (name, ("pred_depth",), dict(pred_depth=501))]
        out += [(name, ("null output buffer",), {k: None}) for k in CUTILS_OUT[:6]]
        out += [(name, ("max_nodes",), dict(max_nodes=3, attr=None))]             # sizes before pointers
    for name in ("fl_step_obs", "fl_obs_cutils_tree"):
        out += [(name, ("in [%d,4]" % (name == "fl_obs_cutils_tree"),), dict(depth=5)), (name, ("tree_pred_depth <= pred_depth",), dict(pred_depth=100, tree_pred=101)),
                (name, ("tree_pred_depth <= pred_depth",), dict(tree_pred=-1)), (name, (), dict(tree_out=None)),
                (name, ("in [%d,4]" % (name == "fl_obs_cutils_tree"),), dict(depth=5, attr=None))]      # sizes before pointers
    out += [("fl_step_obs", ("in [0,4]",), dict(depth=-1)), ("fl_obs_cutils_tree", ("in [1,4]",), dict(depth=0))]
    out += [("fl_step_obs", ("bad step argument",), {k: None}) for k in ("rewards", "dones", "done_all")]
    out += [("fl_step_obs", ("bad step argument",), dict(kind=3)), ("fl_step_obs", ("bad step argument",), dict(kind=-1)),
            ("fl_step_obs", ("bad step argument",), dict(kind=3, max_nodes=3))]
    for name in ("fl_obs_tree", "fl_obs_tree_handles"):
        out += [(name, ("max_depth must be in [1,4]",), dict(depth=0)), (name, ("max_depth must be in [1,4]",), dict(depth=5)),
                (name, ("pred_depth <= 500",), dict(tree_pred=501)), (name, (), dict(tree_out=None))]
    return out


def _handle_list_cases(A):
    return [(("n_handles",), dict(handles=(), n_handles=0)), (("n_handles",), dict(handles=tuple(range(A)) + (0,))),
            (("n_handles",), dict(handles=None, n_handles=2)),
            (("permutation",), dict(handles=(0, 0))), (("permutation",), dict(handles=(1, 1, 0))),
            (("permutation",), dict(handles=(0, 2))), (("permutation",), dict(handles=(0, A))),
            (("permutation",), dict(handles=(-1, 0))), (("permutation",), dict(handles=(0, 1, -2)))]


def _id(case):
    return case[0] + "-" + ",".join("%s=%s" % kv for kv in case[2].items())


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_bad_sizes_and_null_buffers_are_refused_before_anything_runs(flat, case):
    name, says, over = case
    _refused(flat, name, says, **over)


@pytest.mark.parametrize("name", ("fl_obs_cutils_handles", "fl_obs_tree_handles"))
def test_bad_handle_lists_are_refused_and_reported_before_bad_sizes(flat, name):
    A = flat.env.A
    for says, over in _handle_list_cases(A):
        _refused(flat, name, says, **over)
        # a bad list wins over bad sizes and null buffers
        bad = dict(max_nodes=3, attr=None) if name == "fl_obs_cutils_handles" else dict(depth=5, tree_out=None)
        msg = _refused(flat, name, says, **dict(over, **bad))
        assert "max_nodes" not in msg and "max_depth" not in msg and "null" not in msg, msg


@pytest.mark.parametrize("name", ("fl_step_obs", "fl_obs_cutils_tree", "fl_obs_tree", "fl_obs_tree_handles"))
def test_depth_4_on_a_grid_with_a_three_way_cell_is_refused_before_anything_runs(threeway, name):
    _refused(threeway, name, ("more than two transitions",), depth=4)
    if name in WITH_CUTILS:          # the other argument errors go first
        _refused(threeway, name, ("null output buffer",), depth=4, forest=None)
        _refused(threeway, name, ("max_nodes",), depth=4, max_nodes=65)
    rc, msg = threeway.call(name, depth=3)             # depth 3 runs on this grid
    assert rc == 0, msg
    if name == "fl_step_obs":
        assert threeway.env.state()[1][0] == 4         # three steps of the fixture + this one: no refused call advanced the env
    threeway.env.check()


@pytest.mark.parametrize("name", ("fl_obs_cutils_handles", "fl_obs_tree_handles"))
def test_accepted_handle_lists_and_what_the_record_says_of_them(flat, name):
    env, A = flat.env, flat.env.A
    for handles, label in ((tuple(range(A)), 0), (SWAP, 1), (tuple(range(A)), 0), (tuple(reversed(range(A))), 1), ((0,), 1)):
        rc, msg = flat.call(name, handles=handles)
        assert rc == 0, (handles, msg)
        rec = env.last_obs_launch()
        assert rec["mode"] >= 0 and rec["label"] == label, (handles, rec)
    if name == "fl_obs_cutils_handles":
        rc, msg = flat.call(name, handles=SWAP, props=None)        # props may be NULL (include/flatland_hip.h)
        assert rc == 0, msg
    else:
        rc, msg = flat.call(name, handles=SWAP, tree_pred=-1)      # no predictor: no conflict test, the list does not matter
        assert rc == 0 and env.last_obs_launch()["label"] == 0, msg
    env.check()
