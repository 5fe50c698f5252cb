"""GPU: the one-round observation kernels (k_obs MODE 3 / 6: csrc/fl_obs_body.h, fl_obs_trees.h) fill the prediction index with a leaner body
(the direction masks through cf_dirs_swar, the second index's masks as two 64-bit ORs) and hand the topology piece of every flatland_cutils
tree -- adjacency, padding rows, rows of absent nodes, both evaluation orders -- to the late queue of pass B's work-list step, where ANY
wavefront takes it before pass B is over.  Neither changes a byte: every output equals the oracle's (oracle.orc), and the same bytes come out with
FL_OBS_NO_CF_DIRS=1 (no masks: every query filed), FL_OBS_NO_EARLY_TOPO=1 (the topology piece behind pass B's last barrier) and FL_OBS_NO_FIX=1
(the runtime carving of the same kernels).

Batches (a batch holds envs of one agent count; tests/handmaps.py rails, tests/obs_state_cases.py constructors):

  y1    one agent on the yard: fewer trees than wavefronts, every topology job is taken by a wavefront that does not own the tree.  dead_end: the
        walker runs into the buffer and comes back, the tree fills all 31 nodes; done / waiting: an agent off the map (the reference walks
        from its virtual position: a full tree too); stub: the three-cell component nobody leaves, whose queue runs dry (padding rows)
  y3    three agents on the yard: the cases of the direction filter rebuilt -- follower, head_on, bend (the leader turns on the symmetric switch:
        its item's next direction differs from its direction, so the first index's mask has a bit the second's lacks), done (a DONE agent's
        item), own / own_ctl (the walker's own item satisfies the condition through its next direction), dead_end
  x3    three agents on the crossing: trees that fill all 31 nodes (children beyond max_nodes are never popped) and hold absent branches
  y32   32 agents on the yard, 28 of them waiting on two start cells: every wavefront owns two trees, none is idle

What each batch exists for is asserted on the ORACLE's output before anything runs on the GPU.  Each switch set runs in ONE fresh child process
(the launcher reads its switches once per process) under a time limit; after a child that ends on a signal or at its limit no other is started.
Per batch a child runs obs_both(2, 30), obs_cutils() and obs_policy() (the int64 adjacency with the tree * max_nodes offsets and -2 for every
negative entry, the int64 orders -- written by a wavefront other than the tree's) and prints what last_obs_launch() says it ran."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import handmaps, util
from tests import obs_state_cases as oc

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M, DONE, WAITING = oc.MOVING, oc.DONE, oc.WAITING
CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"), ("edge_order", "edge_order"),
          ("valid_actions", "valid"), ("props", "props"))
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
MAX_NODES = 31
GONE3 = (4, 1, E, 6, 1)
WAIT = oc.off(WAITING)
# batch -> (map, {case: ((row, col, direction, target row, target col) per agent, speeds, the agents' states)})
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
_Y32_SPEC = [(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(4, 1, E, 4, 0), (4, 6, W, 4, 7)] * 14 + [(4, 5, W, 4, 0), (3, 3, N, 1, 6)]
Y32 = {
    "crowd": (_Y32_SPEC, [1.0, 1 / 3] + [1.0] * 28 + [1.0, 1 / 3], [oc.on(M, 1, 4, W), oc.on(M, 4, 1, E)] + [WAIT] * 28 + [oc.on(M, 4, 5, W), oc.on(M, 3, 3, N)]),
    "moving": (_Y32_SPEC, [1.0] * 32, [oc.on(M, 1, 5, W), oc.on(M, 4, 2, E)] + [WAIT, oc.GONE] * 14 + [oc.on(M, 4, 4, W), oc.on(M, 2, 3, N)]),
}
BATCHES = (("y1", "yard", Y1), ("y3", "yard", Y3), ("x3", "crossing", X3), ("y32", "yard", Y32))
SWITCH_SETS = (("default", {}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"}), ("latetopo", {"FL_OBS_NO_EARLY_TOPO": "1"}), ("nofix", {"FL_OBS_NO_FIX": "1"}))


def _grid(map_name):
    return handmaps.STEP_MAPS[map_name]()["grid"]


def _static(map_name, spec, speed):
    a = np.array(spec, dtype=np.int32)
    A = len(a)
    return dict(grid=_grid(map_name), init_pos=a[:, 0:2].copy(), init_dir=a[:, 2].copy(), target=a[:, 3:5].copy(), speed=np.array(speed, dtype=np.float64),
                earliest=np.zeros(A, dtype=np.int32), latest=np.full(A, 200, dtype=np.int32), T=400, malf_rate=0.0, malf_min=0, malf_max=0,
                mt_key=np.arange(624, dtype=np.uint32), mt_pos=624)


def _rows(map_name, spec, agents):
    grid = _grid(map_name)
    st, aux = np.zeros((len(spec), 12), dtype=np.int32), np.zeros((len(spec), 4), dtype=np.int32)
    for i, a in enumerate(agents):
        d = spec[i][2] if a["d"] is None else a["d"]
        if a["r"] >= 0:
            assert handmaps.nibble(grid[a["r"], a["c"]], d) != 0, (i, a)
        st[i] = (a["r"], a["c"], d, a["state"], a["malf"], 0, 0, 0, 1 if a["state"] == DONE else -1, a["r"], a["c"], d if a["r"] >= 0 else -1)
        aux[i] = (-1, 0, 0, int(a["state"] == DONE))
    return st, aux


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30) of the oracle set to the case's state; computed once"""
    from oracle import orc
    map_name, cases = {b: (m, c) for b, m, c in BATCHES}[batch]
    spec, speed, agents = cases[name]
    o = orc.OracleEnv(_static(map_name, spec, speed))
    st, aux = _rows(map_name, spec, agents)
    o.set_state(st, aux, 0, False)
    tree = o.obs_pytree(2, 30)
    o.set_state(st, aux, 0, False)      # (a flatland_cutils call leaves its deadlock flags in the env)
    return o.obs_cutils(MAX_NODES, 500), tree


def _policy_form(cu, b, A):
    """the three index tensors of one env as the policy takes them: int64, parent / child offset by tree * max_nodes, every negative entry -2"""
    adj = cu["adjacency"].astype(np.int64)
    neg = adj < 0
    adj[:, :, 0:2] += ((b * A + np.arange(A, dtype=np.int64)) * MAX_NODES)[:, None, None]
    adj[neg] = -2
    no, eo = cu["node_order"].astype(np.int64), cu["edge_order"].astype(np.int64)
    no[no < 0] = -2
    eo[eo < 0] = -2
    return adj, no, eo


def _shape_of(cu, i):
    """(real nodes, absent nodes among them) of agent i's tree: a real node has an order, an absent one the padding row's features"""
    real = cu["node_order"][i] >= 0
    pad_row = np.array([-1.0] * 12, dtype=np.float32)
    absent = real & (cu["forest"][i] == pad_row).all(axis=1)
    return int(real.sum()), int(absent.sum())


def _reached():
    """every batch reaches what it exists for, judged on the oracle's output"""
    y1 = {k: _oracle("y1", k)[0] for k in Y1}
    n_stub, _ = _shape_of(y1["stub"], 0)
    assert 1 < n_stub < MAX_NODES, n_stub                                    # the queue ran dry: padding rows, padding adjacency
    assert (y1["stub"]["adjacency"][0, n_stub - 1:] == -2).all() and (y1["stub"]["node_order"][0, n_stub:] == -2).all()
    assert (y1["stub"]["forest"][0, n_stub:] == -1).all()
    # (a dead end turns the train round, so a walk on the yard's lines goes on until the tree is full -- for a DONE agent and one that has not
    # departed too, which the reference walks from their virtual position: no tree of these rails is the root alone)
    assert all(_shape_of(y1[k], 0)[0] == MAX_NODES for k in ("dead_end", "done", "waiting"))
    x3 = {k: _oracle("x3", k)[0] for k in X3}
    shapes = [_shape_of(x3[k], i) for k in X3 for i in range(3)]
    assert any(n == MAX_NODES for n, _ in shapes), shapes                    # a tree that fills all 31 nodes
    assert any(ab > 0 for _, ab in shapes), shapes                           # real nodes of absent branches
    y32 = {k: _oracle("y32", k)[0] for k in Y32}
    assert all(len(Y32[k][0]) == 32 for k in Y32)
    kinds = {_shape_of(y32[k], i)[0] for k in Y32 for i in range(32)}
    assert min(kinds) <= 4 and max(kinds) == MAX_NODES and len(kinds) >= 4, kinds      # trees of four nodes beside full ones in one round
    # the direction filter's cases (tests/test_gpu_cf_dirs.py says what each is): the forward child of walker 0, columns 2 / 3 = other agent / conflict
    y3 = {k: _oracle("y3", k) for k in Y3}
    cu = {k: v[0]["forest"][0, 2] for k, v in y3.items()}
    py = {k: v[1][0, 6] for k, v in y3.items()}
    scale = cu["head_on"][3] / 2.0
    assert py["follower"][2] == 1 and np.isposinf(py["follower"][3]) and cu["follower"][2] > 0 and cu["follower"][3] == -1
    assert py["head_on"][3] == 2 and cu["head_on"][3] > 0
    assert np.isposinf(py["bend"][3]) and py["bend"][2] == 1 and cu["bend"][3] == np.float32(2 * scale)      # only through the item's NEXT direction
    assert py["done"][3] == 2 and cu["done"][3] == np.float32(2 * scale) and np.isposinf(py["done"][2]) and cu["done"][2] == -1
    assert cu["own"][3] == np.float32(2 * scale) and cu["own_ctl"][3] == -1
    assert py["dead_end"][2] == 1 and np.isposinf(py["dead_end"][3]) and cu["dead_end"][2] > 0 and cu["dead_end"][3] == -1


def _same(got, exp, msg):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{msg}: shape {got.shape} vs {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{msg}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {exp[tuple(bad[0])]}")


def _run(out_path):
    """child: the three launches on every batch against the oracle; every tensor goes to out_path for the parent's byte comparison"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    keep = {}
    for batch, map_name, cases in BATCHES:
        names = list(cases)
        env = BatchedRailEnv([_static(map_name, cases[k][0], cases[k][1]) for k in names])
        assert env.max_nodes == MAX_NODES and env.pred_depth == 500
        pairs = [_rows(map_name, cases[k][0], cases[k][2]) for k in names]
        states, aux = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        B, A = len(names), env.A

        def inject():
            env.set_state(states, aux, np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8))

        for call in ("both", "alone", "policy"):
            inject()
            tree = None
            if call == "both":
                got, tree = env.obs_both(2, 30)
                tree = tree.cpu().numpy()
            elif call == "alone":
                got = env.obs_cutils()
            else:
                pol = env.obs_policy()
                got = dict(env.obs_outputs(), agent_attr=pol[0], forest=pol[1], adjacency=pol[2], node_order=pol[3], edge_order=pol[4])
            print("RECORD", batch, call, json.dumps(env.last_obs_launch()), flush=True)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            for b, k in enumerate(names):
                exp_cu, exp_tree = _oracle(batch, k)
                exp_cu = dict(exp_cu)
                if call == "policy":
                    exp_cu["adjacency"], exp_cu["node_order"], exp_cu["edge_order"] = _policy_form(exp_cu, b, A)
                for g, e in CUTILS:
                    assert got[g][b].dtype == exp_cu[e].dtype, (g, got[g].dtype)
                    _same(got[g][b], exp_cu[e], f"{batch}/{k} {call} {g}")
                if tree is not None:
                    _same(tree[b], exp_tree, f"{batch}/{k} {call} depth-2 tree")
            for g, _ in CUTILS:
                keep[f"{batch}/{call}/{g}"] = got[g]
            if tree is not None:
                keep[f"{batch}/{call}/tree"] = tree
        env.check()
        env.close()
    np.savez(out_path, **keep)
    print("DONE", len(keep), "tensors")


def test_fill_and_early_topology_change_no_byte_and_equal_the_oracle(tmp_path):
    _reached()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FL_OBS_")}
    outs, records = {}, {}
    for tag, switches in SWITCH_SETS:
        path = str(tmp_path / (tag + ".npz"))
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(env, PYTHONPATH=util.ROOT, **switches),
                                   capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:      # nothing more is started on the card
            err = e.stderr or ""
            pytest.fail("%s: no end after %d s\n%s" % (tag, CHILD_TIMEOUT, (err if isinstance(err, str) else err.decode(errors="replace"))[-3000:]))
        assert child.returncode == 0, "%s: exit status %d\n%s" % (tag, child.returncode, child.stderr[-3000:])      # (a failed assert ends the test: no further child)
        lines = child.stdout.splitlines()
        assert any(ln.startswith("DONE ") for ln in lines), tag
        records[tag] = {tuple(ln.split()[1:3]): json.loads(ln.split(None, 3)[3]) for ln in lines if ln.startswith("RECORD ")}
        outs[tag] = np.load(path)
    # every batch runs the one-round kernels: both builders MODE 3, the builder alone (int32 and the policy's int64 form) MODE 6 -- on a launch
    # class (compile-time carving) unless FL_OBS_NO_FIX asks for the runtime carving
    for tag, rec in records.items():
        assert len(rec) == 3 * len(BATCHES)
        for (batch, call), r in rec.items():
            assert r["mode"] == (3 if call == "both" else 6) and r["nt"] == 1024 and r["tmask"] == 1 and r["split"] == 0, (tag, batch, call, r)
            assert (r["fix"] == 0) == (tag == "nofix"), (tag, batch, call, r)
            assert r["fix"] in ((0,) if tag == "nofix" else (1, 11) if call == "both" else (6,)), (tag, batch, call, r)
    for tag in ("nomasks", "latetopo"):
        assert records[tag] == records["default"], tag
    a = outs["default"]
    assert len(a.files) == len(BATCHES) * (3 * len(CUTILS) + 1)
    for tag, b in outs.items():
        assert sorted(a.files) == sorted(b.files), tag
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)


if __name__ == "__main__":
    _run(sys.argv[1])
