"""What the GPU tests of the observation kernels on constructed states share (tests/test_gpu_cf_dirs.py, test_gpu_obs_flat_fill.py,
test_gpu_obs_tail_fill.py, test_gpu_passb_slices.py: "this switch changes no byte"; test_gpu_prefix_scans.py; the launchers of
test_gpu_obs_states.py, test_gpu_obs_kernel_cases.py and test_gpu_handmaps.py).  Data and helpers, no test; nothing of the GPU is imported
before a function that needs it is called.

A case: ((row, col, direction, target row, target col) per agent, speeds, the agents' states as tests/obs_state_cases.py constructs them).
A batch: (name, grid, {case name: case}) -- the cases are the envs of one BatchedRailEnv.  A test gives run_batches, the body of its child
process, its batches and an `oracle(batch, name)` that returns (flatland_cutils tensors, upstream depth-2 tree, ...) computed once; the
parent starts one child per switch set with run_switch_sets and compares what they saved with assert_same_bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import handmaps, util
from tests import obs_state_cases as oc

N, E, S, W = 0, 1, 2, 3
M, DONE, WAITING = oc.MOVING, oc.DONE, oc.WAITING
CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"), ("edge_order", "edge_order"),
          ("valid_actions", "valid"), ("props", "props"))
MAX_NODES = 31
GONE3 = (4, 1, E, 6, 1)      # a third agent of the yard, DONE on the stub nobody reaches
WAIT = oc.off(WAITING)


# ---- the shared cases (what each exists for: the docstrings of the tests that assert it on the oracle's output)
def crowd(pairs):
    """the yard's crowd with `pairs` pairs of agents waiting on the two start cells (4, 1) and (4, 6), four travelling: 2 * pairs + 4 agents"""
    spec = [(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(4, 1, E, 4, 0), (4, 6, W, 4, 7)] * pairs + [(4, 5, W, 4, 0), (3, 3, N, 1, 6)]
    speed = [1.0, 1 / 3] + [1.0] * (2 * pairs) + [1.0, 1 / 3]
    agents = [oc.on(M, 1, 4, W), oc.on(M, 4, 1, E)] + [WAIT] * (2 * pairs) + [oc.on(M, 4, 5, W), oc.on(M, 3, 3, N)]
    return spec, speed, agents


def dense(pairs):
    """two travelling agents and `pairs` pairs waiting on the two start cells of the yard from which ONE agent's two trees visit the most cells (80 from
    (1, 3) heading north for (4, 7), 75 from (4, 3) heading east for (1, 6), counted once on the GPU over every rail state of the yard as a start and the
    five targets of the cases; only the unreachable target on the stub gives more, 87): about the densest round these rails allow"""
    spec = [(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(1, 3, N, 4, 7), (4, 3, E, 1, 6)] * pairs
    return spec, [1.0] * len(spec), [oc.on(M, 1, 4, W), oc.on(M, 4, 2, E)] + [WAIT] * (2 * pairs)


Y1 = {
    "dead_end": ([(4, 5, E, 1, 6)], [1.0], [oc.on(M, 4, 5, E)]),
    "done": ([(4, 1, E, 4, 4)], [1.0], [oc.off(DONE, d=W)]),
    "waiting": ([(4, 1, E, 4, 7)], [0.5], [WAIT]),
    "stub": ([(6, 1, E, 6, 0)], [1.0], [oc.on(M, 6, 1, E)]),
}
Y3 = {
    "follower": ([(4, 6, W, 4, 0), (4, 5, W, 4, 0), GONE3], [1.0, 0.5, 1.0], [oc.on(M, 4, 6, W), oc.on(M, 4, 5, W), oc.GONE]),
    "head_on": ([(4, 6, W, 4, 0), (4, 2, E, 4, 7), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 4, 6, W), oc.on(M, 4, 2, E), oc.GONE]),
    "bend": ([(3, 3, N, 1, 6), (2, 3, N, 1, 0), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 2, 3, N), oc.GONE]),
    "done": ([(4, 6, W, 4, 0), (4, 1, E, 4, 4), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 4, 6, W), oc.off(DONE, d=W), oc.GONE]),
    "own": ([(3, 3, N, 1, 0), (1, 2, E, 4, 0), GONE3], [1 / 7, 1 / 12, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 1, 2, E), oc.GONE]),
    "own_ctl": ([(3, 3, N, 1, 0), (1, 2, E, 4, 0), GONE3], [1 / 7, 1 / 12, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 4, 1, W), oc.GONE]),
    "dead_end": ([(4, 5, E, 1, 6), (4, 6, E, 1, 6), GONE3], [1.0, 0.5, 1.0], [oc.on(M, 4, 5, E), oc.on(M, 4, 6, E), oc.GONE]),
}
X3 = {
    "cross": ([(4, 1, E, 7, 6), (1, 4, S, 8, 4), (4, 7, W, 4, 0)], [1.0, 1.0, 0.5], [oc.on(M, 4, 1, E), oc.on(M, 1, 4, S), oc.on(M, 4, 7, W)]),
    "spur": ([(4, 5, E, 7, 6), (6, 6, N, 4, 0), (7, 4, N, 0, 4)], [1.0, 1.0, 1.0], [oc.on(M, 4, 5, E), oc.on(M, 6, 6, N), WAIT]),
}
Y32 = {
    "crowd": crowd(14),
    "moving": (crowd(14)[0], [1.0] * 32, [oc.on(M, 1, 5, W), oc.on(M, 4, 2, E)] + [WAIT, oc.GONE] * 14 + [oc.on(M, 4, 4, W), oc.on(M, 2, 3, N)]),
}


# ---- builders
def grid_of(map_name):
    return handmaps.STEP_MAPS[map_name]()["grid"]


def rows(grid, spec, agents):
    """(rows i32[A, 12] in util.STATE_NAMES order, aux i32[A, 4]) of agents in the given states; a train on the map faces a way its cell
    allows.  No malfunction has been counted and none is signalled, whatever the counter says (tests/obs_state_cases.py's own _rows sets
    both from the counter, as the reference's env does: its fixtures were captured that way)"""
    st, aux = np.zeros((len(spec), 12), dtype=np.int32), np.zeros((len(spec), 4), dtype=np.int32)
    for i, a in enumerate(agents):
        d = spec[i][2] if a["d"] is None else a["d"]
        if a["r"] >= 0:
            assert handmaps.nibble(grid[a["r"], a["c"]], d) != 0, (i, a)
        st[i] = (a["r"], a["c"], d, a["state"], a["malf"], 0, 0, 0, 1 if a["state"] == DONE else -1, a["r"], a["c"], d if a["r"] >= 0 else -1)
        aux[i] = (-1, 0, 0, int(a["state"] == DONE))
    return st, aux


def policy_form(cu, b, A, max_nodes=MAX_NODES):
    """the three index tensors of one env as the policy takes them: int64, parent / child offset by tree * max_nodes, every negative entry -2"""
    adj = cu["adjacency"].astype(np.int64)
    neg = adj < 0
    adj[:, :, 0:2] += ((b * A + np.arange(A, dtype=np.int64)) * max_nodes)[:, None, None]
    adj[neg] = -2
    no, eo = cu["node_order"].astype(np.int64), cu["edge_order"].astype(np.int64)
    no[no < 0] = -2
    eo[eo < 0] = -2
    return adj, no, eo


def shape_of(cu, i):
    """(real nodes, absent nodes among them) of agent i's tree: a real node has an order, an absent one the padding row's features"""
    real = cu["node_order"][i] >= 0
    pad_row = np.array([-1.0] * 12, dtype=np.float32)
    absent = real & (cu["forest"][i] == pad_row).all(axis=1)
    return int(real.sum()), int(absent.sum())


def oracle_obs(static, st, aux, max_nodes=MAX_NODES, cu_pred=500, tree_depth=2, py_pred=30):
    """(flatland_cutils tensors, upstream tree) of the CPU oracle set to a state"""
    from oracle import orc
    o = orc.OracleEnv(static)
    o.set_state(st, aux, 0, False)
    tree = o.obs_pytree(tree_depth, py_pred)
    o.set_state(st, aux, 0, False)      # (a flatland_cutils call leaves its deadlock flags in the env)
    return o.obs_cutils(max_nodes, cu_pred), tree


def oracle_case(grid, case, **kw):
    spec, speed, agents = case
    return oracle_obs(util.plain_static(grid, spec, speed), *rows(grid, spec, agents), **kw)


# ---- the child
def run_batches(batches, calls, out_path, *, oracle, max_nodes=MAX_NODES, cu_pred=500, py_pred=30):
    """child: the launches `calls` -- among "both" (obs_both(2, py_pred)), "alone" (obs_cutils()) and "policy" (obs_policy()) -- on every
    batch against oracle(batch, name)[0:2], values and dtypes; what the launcher says it ran goes to stdout as RECORD lines, every tensor
    to out_path for the parent's byte comparison"""
    keep = {}
    for batch, grid, cases in batches:
        names = list(cases)
        env = util.batched([util.plain_static(grid, cases[k][0], cases[k][1]) for k in names])
        assert env.max_nodes == max_nodes and env.pred_depth == cu_pred
        pairs = [rows(grid, cases[k][0], cases[k][2]) for k in names]
        states, aux = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        B, A = len(names), env.A
        for call in calls:
            env.set_state(states, aux, np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8))
            tree = None
            if call == "both":
                got, tree = env.obs_both(2, py_pred)
                tree = tree.cpu().numpy()
            elif call == "alone":
                got = env.obs_cutils()
            else:
                assert call == "policy", call
                pol = env.obs_policy()
                got = dict(env.obs_outputs(), agent_attr=pol[0], forest=pol[1], adjacency=pol[2], node_order=pol[3], edge_order=pol[4])
            print("RECORD", batch, call, json.dumps(env.last_obs_launch()), flush=True)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            for b, k in enumerate(names):
                exp_cu, exp_tree = oracle(batch, k)[0:2]
                exp_cu = dict(exp_cu)
                if call == "policy":
                    exp_cu["adjacency"], exp_cu["node_order"], exp_cu["edge_order"] = policy_form(exp_cu, b, A, max_nodes)
                for g, e in CUTILS:
                    util.same(got[g][b], exp_cu[e], f"{batch}/{k} {call} {g}", dtype=True)
                if tree is not None:
                    util.same(tree[b], exp_tree, f"{batch}/{k} {call} depth-2 tree", dtype=True)
            for g, _ in CUTILS:
                keep[f"{batch}/{call}/{g}"] = got[g]
            if tree is not None:
                keep[f"{batch}/{call}/tree"] = tree
        env.check()
        env.close()
    np.savez(out_path, **keep)
    print("DONE", len(keep), "tensors")


# ---- the parent
def fresh_child(script, args, switches, timeout, tag=None, lost=None):
    """`script args` in ONE fresh python process (the launcher reads its switches once per process) whose environment holds `switches` and no
    other FL_OBS_* variable, under a time limit.  Returns the lines of its stdout.  A child that ends at its limit or with another status
    than 0 fails the calling test with the end of its output -- an exception, so a caller's loop starts nothing more on the card; one
    that ended at its limit or on a signal is also appended to `lost`, for a caller that is entered again (a parametrised test).
    An FL_OBS_* key of `switches` that the library's table (csrc/fl_obs_switches.h) does not have is refused before any child starts: the
    launcher would ignore it, and the child would run the default."""
    from flatland_marl_amd.hip_backend import obs_switches
    tag = " ".join(args) if tag is None else tag
    unknown = sorted(k for k in switches if k.startswith("FL_OBS_") and k not in obs_switches())
    assert not unknown, "%s: no such switch of the launcher: %s" % (tag, ", ".join(unknown))
    env = {k: v for k, v in os.environ.items() if not k.startswith("FL_OBS_")}
    try:
        child = subprocess.run([sys.executable, os.path.abspath(script)] + list(args), env=dict(env, PYTHONPATH=util.ROOT, **switches),
                               capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        if lost is not None:
            lost.append((tag, "at its time limit of %d s" % timeout))
        err = e.stderr or ""
        pytest.fail("%s: no end after %d s\n%s" % (tag, timeout, (err if isinstance(err, str) else err.decode(errors="replace"))[-3000:]))
    if lost is not None and (child.returncode < 0 or child.returncode in (134, 139)):      # a signal: the card may be in a bad state
        lost.append((tag, "with exit status %d" % child.returncode))
    assert child.returncode == 0, "%s: exit status %d\n%s\n%s" % (tag, child.returncode, child.stdout[-1500:], child.stderr[-3000:])
    return child.stdout.splitlines()


def run_switch_sets(script, switch_sets, tmp_path, timeout):
    """one fresh child `script <tmp_path>/<tag>.npz` per (tag, switches), one after the other: ({tag: the saved tensors},
    {tag: {(batch, call): the launch record}})"""
    outs, records = {}, {}
    for tag, switches in switch_sets:
        path = str(tmp_path / (tag + ".npz"))
        lines = fresh_child(script, [path], switches, timeout, tag=tag)
        assert any(ln.startswith("DONE ") for ln in lines), tag
        records[tag] = {tuple(ln.split()[1:3]): json.loads(ln.split(None, 3)[3]) for ln in lines if ln.startswith("RECORD ")}
        outs[tag] = np.load(path)
    return outs, records


def assert_same_bytes(outs, n_files):
    """every child saved the same n_files tensors, byte for byte, as the "default" one (the first, where no tag is "default")"""
    a = outs["default"] if "default" in outs else next(iter(outs.values()))
    assert len(a.files) == n_files, (len(a.files), n_files)
    for tag, b in outs.items():
        assert sorted(a.files) == sorted(b.files), tag
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
