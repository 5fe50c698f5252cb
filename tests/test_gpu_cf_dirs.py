"""GPU: the direction filter of pass B's classify loop (csrc/fl_obs_passb.h: ObsCtx::cmask) files no conflict query whose key holds no item that
could satisfy the conflict condition for the walking direction.  Skipping such a query is exact, so the observations are the oracle's
(oracle.orc), and the same bytes with FL_OBS_NO_CF_DIRS=1 (every query filed, as before the filter).

Seven envs of three agents on the yard (tests/handmaps.py; the third agent is DONE on the stub nobody reaches) and one env on a mesh whose cells
have three ways on.  What each env exists for is asserted on the ORACLE's output before anything runs on the GPU (py: the dense upstream depth-2
tree, row 6 = the root's forward child; cu: the flatland_cutils forest, node 2; columns 2 / 3 = other agent / potential conflict):

  follower   a slower train ahead on the same track, same direction: on the cell at the queried time (other agent finite), never a conflict --
             the query the masks reject
  head_on    the same track, the second train head-on: a conflict at tot_dist 2 for both builders
  bend       the leader turns west on the symmetric switch one step ahead of the walker, which comes up the stem behind it: at the queried time
             the leader has left the switch, at the step before it is there facing north like the walker -- flatland_cutils reads its direction at the
             queried time (west: IT_DNEXT) and reports a conflict, upstream reads the direction at the step before and reports none
  done       a DONE agent's item on the walked cell
  own        walker at speed 1/7 (float32: six steps a cell, queried at t = 13): on the switch its OWN item covers t = 12 only and satisfies the
             condition through its next direction; the second agent (1/12, on the switch until t = 12, bound down the stem) supplies presence
             and no condition of its own.  own_ctl: the second agent elsewhere -- no conflict
  dead_end   the walker runs into the dead end (4, 7), whose only transition for its direction is the U-turn: the slower train on it is seen,
             no conflict
  mesh       three ways on per direction: no compact upstream trees, so the two-stage kernels without the masks run (asserted from
             last_obs_launch) -- the old loop

Each switch value runs in ONE fresh child process (the launcher reads its switches once per process)."""
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
M, DONE = oc.MOVING, oc.DONE
CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"), ("edge_order", "edge_order"),
          ("valid_actions", "valid"), ("props", "props"))
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
GONE3 = (4, 1, E, 6, 1)
# name -> ((row, col, direction, target row, target col) per agent, speeds, the agents' states)
YARD = {
    "follower": ([(4, 6, W, 4, 0), (4, 5, W, 4, 0), GONE3], [1.0, 0.5, 1.0], [oc.on(M, 4, 6, W), oc.on(M, 4, 5, W), oc.GONE]),
    "head_on": ([(4, 6, W, 4, 0), (4, 2, E, 4, 7), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 4, 6, W), oc.on(M, 4, 2, E), oc.GONE]),
    "bend": ([(3, 3, N, 1, 6), (2, 3, N, 1, 0), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 2, 3, N), oc.GONE]),
    "done": ([(4, 6, W, 4, 0), (4, 1, E, 4, 4), GONE3], [1.0, 1.0, 1.0], [oc.on(M, 4, 6, W), oc.off(DONE, d=W), oc.GONE]),
    "own": ([(3, 3, N, 1, 0), (1, 2, E, 4, 0), GONE3], [1 / 7, 1 / 12, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 1, 2, E), oc.GONE]),
    "own_ctl": ([(3, 3, N, 1, 0), (1, 2, E, 4, 0), GONE3], [1 / 7, 1 / 12, 1.0], [oc.on(M, 3, 3, N), oc.on(M, 4, 1, W), oc.GONE]),
    "dead_end": ([(4, 5, E, 1, 6), (4, 6, E, 1, 6), GONE3], [1.0, 0.5, 1.0], [oc.on(M, 4, 5, E), oc.on(M, 4, 6, E), oc.GONE]),
}
MESH = {"mesh": ([(2, 1, E, 2, 5), (2, 4, W, 2, 0), (0, 0, E, 4, 5)], [1.0, 0.5, 1.0], [oc.on(M, 2, 1, E), oc.on(M, 2, 4, W), oc.GONE])}
BATCHES = (("yard", YARD), ("mesh", MESH))


def _grid(batch):
    return handmaps.STEP_MAPS["yard"]()["grid"] if batch == "yard" else handmaps.full_grid(5, 6)


def _static(batch, spec, speed):
    a = np.array(spec, dtype=np.int32)
    A = len(a)
    return dict(grid=_grid(batch), init_pos=a[:, 0:2].copy(), init_dir=a[:, 2].copy(), target=a[:, 3:5].copy(), speed=np.array(speed, dtype=np.float64),
                earliest=np.zeros(A, dtype=np.int32), latest=np.full(A, 200, dtype=np.int32), T=400, malf_rate=0.0, malf_min=0, malf_max=0,
                mt_key=np.arange(624, dtype=np.uint32), mt_pos=624)


def _rows(batch, spec, agents):
    grid = _grid(batch)
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
    spec, speed, agents = dict(BATCHES)[batch][name]
    o = orc.OracleEnv(_static(batch, spec, speed))
    st, aux = _rows(batch, spec, agents)
    o.set_state(st, aux, 0, False)
    tree = o.obs_pytree(2, 30)
    o.set_state(st, aux, 0, False)      # (a flatland_cutils call leaves its deadlock flags in the env)
    return o.obs_cutils(31, 500), tree


def _reached():
    """every case reaches what it exists for, judged on the oracle's output"""
    g = _grid("yard")
    PY_F, CU_F, OA, PC = 6, 2, 2, 3
    res = {k: _oracle("yard", k) for k in YARD}
    py = {k: v[1][0, PY_F] for k, v in res.items()}            # walker 0, the root's forward child
    cu = {k: v[0]["forest"][0, CU_F] for k, v in res.items()}
    scale = cu["head_on"][PC] / 2.0                               # the forest holds distances divided by a per-env length: tot_dist 2 here
    assert py["follower"][OA] == 1 and np.isposinf(py["follower"][PC]) and cu["follower"][OA] > 0 and cu["follower"][PC] == -1
    for k in YARD:      # the follower env holds no conflict at all, for no agent and no builder
        if k in ("follower", "own_ctl"):
            real = ~np.isneginf(res[k][1][:, 1:, PC])
            assert np.isposinf(res[k][1][:, 1:, PC][real]).all() and (res[k][0]["forest"][:, 1:, PC] <= 0).all(), k
    assert py["head_on"][PC] == 2 and cu["head_on"][PC] > 0
    assert np.isposinf(py["bend"][PC]) and py["bend"][OA] == 1 and cu["bend"][PC] == np.float32(2 * scale)      # only through the next direction
    assert py["done"][PC] == 2 and cu["done"][PC] == np.float32(2 * scale) and np.isposinf(py["done"][OA]) and cu["done"][OA] == -1
    assert cu["own"][PC] == np.float32(2 * scale) and cu["own_ctl"][PC] == -1
    # ... flatland_cutils reads both agents' directions at the queried time, when both have left the switch: the second agent's (south, down
    # the stem) has no opposite among the transitions of a walker heading north, the walker's own (west) has -- the conflict is its own item's
    nib = handmaps.nibble(g[1, 3], N)
    assert not (nib >> (3 - (S + 2) % 4)) & 1 and (nib >> (3 - (W + 2) % 4)) & 1
    assert handmaps.nibble(g[4, 7], E) == 1 << (3 - W)          # the dead end: the U-turn is the only transition
    assert py["dead_end"][OA] == 1 and np.isposinf(py["dead_end"][PC]) and cu["dead_end"][OA] > 0 and cu["dead_end"][PC] == -1


def _same(got, exp, msg):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{msg}: shape {got.shape} vs {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{msg}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {exp[tuple(bad[0])]}")


def _run(out_path):
    """child: both launches on both batches against the oracle; every tensor goes to out_path for the parent's byte comparison"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    keep = {}
    for batch, cases in BATCHES:
        names = list(cases)
        env = BatchedRailEnv([_static(batch, cases[k][0], cases[k][1]) for k in names])
        pairs = [_rows(batch, cases[k][0], cases[k][2]) for k in names]
        states, aux = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        B = len(names)

        def inject():
            env.set_state(states, aux, np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8))

        for call in ("both", "alone"):
            inject()
            if call == "both":
                got, tree = env.obs_both(2, 30)
                tree = tree.cpu().numpy()
            else:
                got, tree = env.obs_cutils(), None
            record = env.last_obs_launch()
            print("RECORD", batch, call, json.dumps(record), flush=True)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            for b, k in enumerate(names):
                exp_cu, exp_tree = _oracle(batch, k)
                for g, e in CUTILS:
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


def test_masks_change_no_byte_and_every_case_equals_the_oracle(tmp_path):
    _reached()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FL_OBS_")}
    outs, records = [], []
    for tag, switches in (("masks", {}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"})):
        path = str(tmp_path / (tag + ".npz"))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(env, PYTHONPATH=util.ROOT, **switches),
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert child.returncode == 0, "%s: exit status %d\n%s" % (tag, child.returncode, child.stderr[-3000:])
        lines = child.stdout.splitlines()
        assert any(ln.startswith("DONE ") for ln in lines), tag
        records.append({tuple(ln.split()[1:3]): json.loads(ln.split(None, 3)[3]) for ln in lines if ln.startswith("RECORD ")})
        outs.append(np.load(path))
    # the yard runs the one-round kernels (the masks' carving) under both switch values, the mesh the two-stage kernels without them
    for rec in records:
        assert rec[("yard", "both")]["mode"] == 3 and rec[("yard", "alone")]["mode"] == 6 and rec[("yard", "both")]["tmask"] == 1, rec
        assert rec[("mesh", "both")]["mode"] == 2 and rec[("mesh", "both")]["compact_t"] == 0 and rec[("mesh", "alone")]["mode"] == 0, rec
    assert records[0] == records[1]
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 2 * (2 * len(CUTILS) + 1)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


if __name__ == "__main__":
    _run(sys.argv[1])
