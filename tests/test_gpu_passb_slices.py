"""GPU: pass B of k_obs (csrc/fl_obs_passb.h) splits the visited cells of a round of trees over the lanes in EVEN slices -- total / nt cells a
lane and one more for the first total % nt lanes (csrc/fl_obs_slices.h; tests/test_passb_slices.py carries the arithmetic) -- where it gave every
lane ceil(total / nt) cells until none were left.  The split decides which lane classifies a cell, never what is filed: every output equals the
oracle's (oracle.orc) byte for byte, and the same bytes come out with FL_OBS_PB_CEIL_SPLIT=1 (the split as it was), FL_OBS_NO_FIX=1 (the runtime
carving of the same kernels) and FL_OBS_NO_CF_DIRS=1 (no direction masks: every query filed, longer work lists).

Batches (a batch holds envs of one agent count; tests/handmaps.py rails, tests/obs_state_cases.py constructors, the cases of
tests/test_gpu_obs_tail_fill.py where they serve):

  y1    one agent on the yard: two teams with cells among 64, so total < nt -- one cell a lane, most wavefronts without any
  x3    three agents on the crossing: trees that fill all 31 nodes, slices that cross many nodes of one tree
  y20   20 agents on the yard, 16 of them waiting on two start cells: forty teams with cells, half of them the short upstream trees, and total
        just above nt -- one cell a lane and a second one for the first 53 lanes only, where the split before gave 539 lanes two cells
        dense: 18 agents waiting on the two start cells whose trees visit the most cells -- 1 515 cells, still one cell a lane and a second for 491:
        20 agents cannot reach two cells a lane on these rails (one agent's two trees visit at most 87 cells: 20 x 87 < 2 x 1 024)
  y32   32 agents on the yard, 28 waiting: every team of the round has cells
        dense: 30 agents waiting on those two start cells -- 2 445 cells, TWO cells a lane and a third for the first 397, the headline's regime
        (the split before: three cells a lane and three wavefronts without any); a lane leaves its team in 12 of the 39 wave-iterations
  y40   40 agents on the yard, 36 waiting: a ROUNDS kernel (k_obs MODE 4 / 7) -- the second round's pass B splits its own total (eight agents)

The regime of each batch's `both` launch, read once from a counting build (-DFL_OBS_TIMING -DFL_OBS_COUNTS, slots 26 / 44 / 45 / 47 / 49 of
fl_debug_obs_clocks; largest env of the batch): see REGIMES below -- the test does not depend on them, they say what the bytes were compared on.

What each batch exists for is asserted on the ORACLE's output before anything runs on the GPU.  Each switch set runs in ONE fresh child process
(the launcher reads its switches once per process) under a guard time limit; after a child that ends on a signal or at its limit no other is
started.  Per batch a child runs obs_both(2, 30), obs_cutils() and obs_policy() and prints what last_obs_launch() says it ran."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import obs_state_cases as oc
from tests import test_gpu_obs_tail_fill as tf
from tests import util

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M, WAIT = oc.MOVING, oc.off(oc.WAITING)
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
MAX_NODES = tf.MAX_NODES
# what a counting build said of the `both` launch of each batch's largest env: cells of the round(s), total / nt, total % nt, wavefronts without
# a cell (even split | ceil split), wave-iterations of the classify loop and those among them in which a lane moved to another team
REGIMES = {
    "y1": "6 .. 62 cells: total / nt 0, remainder = total, 15 of 16 wavefronts without a cell under either split, 1 wave-iteration",
    "x3": "80 .. 86 cells: total / nt 0, remainder = total, 14 wavefronts without a cell, 2 wave-iterations, no lane leaves its team",
    "y20": "1 077 cells: total / nt 1, remainder 53, no wavefront without a cell (ceil split: 2 cells a lane, 7 without), 17 wave-iterations "
           "(18), a lane moves to another team in 1 of them (9 of 18); dense 1 515 cells: total / nt 1, remainder 491, none without a cell (ceil: 4), "
           "24 wave-iterations, 6 with a move (10)",
    "y32": "crowd 1 743 cells: total / nt 1, remainder 719, none without a cell (ceil: 2), 28 wave-iterations, 10 with a move (13); moving 871 "
           "cells: total / nt 0, 2 wavefronts without a cell, 14 wave-iterations; dense 2 445 cells: total / nt 2, remainder 397, none without a "
           "cell (ceil: 3 cells a lane, 3 without), 39 wave-iterations, 12 with a move (18)",
    "y40": "two rounds, the larger 1 787 cells: total / nt 1, remainder 763; 9 wavefronts without a cell over both rounds (ceil: 11), 35 "
           "wave-iterations, 11 with a move (13)",
}


def _crowd(pairs):
    """the yard's crowd with `pairs` pairs of agents waiting on the two start cells (4, 1) and (4, 6), four travelling: 2 * pairs + 4 agents"""
    spec = [(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(4, 1, E, 4, 0), (4, 6, W, 4, 7)] * pairs + [(4, 5, W, 4, 0), (3, 3, N, 1, 6)]
    speed = [1.0, 1 / 3] + [1.0] * (2 * pairs) + [1.0, 1 / 3]
    agents = [oc.on(M, 1, 4, W), oc.on(M, 4, 1, E)] + [WAIT] * (2 * pairs) + [oc.on(M, 4, 5, W), oc.on(M, 3, 3, N)]
    return spec, speed, agents


def _dense(pairs):
    """two travelling agents and `pairs` pairs waiting on the two start cells of the yard from which ONE agent's two trees visit the most cells (80 from
    (1, 3) heading north for (4, 7), 75 from (4, 3) heading east for (1, 6), counted once on the GPU over every rail state of the yard as a start and the
    five targets of the cases; only the unreachable target on the stub gives more, 87): about the densest round these rails allow"""
    spec = [(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(1, 3, N, 4, 7), (4, 3, E, 1, 6)] * pairs
    return spec, [1.0] * len(spec), [oc.on(M, 1, 4, W), oc.on(M, 4, 2, E)] + [WAIT] * (2 * pairs)


Y20 = {"crowd": _crowd(8), "dense": _dense(9)}
Y32 = dict(tf.Y32, dense=_dense(15))
Y40 = {"crowd": _crowd(18)}
BATCHES = (("y1", "yard", tf.Y1), ("x3", "crossing", tf.X3), ("y20", "yard", Y20), ("y32", "yard", Y32), ("y40", "yard", Y40))
ONE_ROUND = ("y1", "x3", "y20", "y32")
SWITCH_SETS = (("default", {}), ("ceil", {"FL_OBS_PB_CEIL_SPLIT": "1"}), ("nofix", {"FL_OBS_NO_FIX": "1"}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"}))


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30) of the oracle set to the case's state; computed once"""
    from oracle import orc
    map_name, cases = {b: (m, c) for b, m, c in BATCHES}[batch]
    spec, speed, agents = cases[name]
    o = orc.OracleEnv(tf._static(map_name, spec, speed))
    st, aux = tf._rows(map_name, spec, agents)
    o.set_state(st, aux, 0, False)
    tree = o.obs_pytree(2, 30)
    o.set_state(st, aux, 0, False)      # (a flatland_cutils call leaves its deadlock flags in the env)
    return o.obs_cutils(MAX_NODES, 500), tree


def _reached():
    """every batch reaches what it exists for, judged on the oracle's output"""
    y1 = {k: _oracle("y1", k)[0] for k in tf.Y1}
    assert all(v["forest"].shape[0] == 1 for v in y1.values())                                   # one tree of each builder: 62 of the 64 teams are empty
    assert any(tf._shape_of(v, 0)[0] == MAX_NODES for v in y1.values())
    x3 = {k: _oracle("x3", k)[0] for k in tf.X3}
    assert any(tf._shape_of(x3[k], i)[0] == MAX_NODES for k in tf.X3 for i in range(3))          # a tree that fills all 31 nodes
    for batch, cases, n in (("y20", Y20, 20), ("y32", Y32, 32), ("y40", Y40, 40)):
        for k in cases:
            cu, tree = _oracle(batch, k)
            assert len(cases[k][0]) == n and cu["forest"].shape[0] == n and tree.shape[0] == n
            nodes = [tf._shape_of(cu, i)[0] for i in range(n)]
            assert min(nodes) > 1, (batch, k, nodes)                                             # every agent's tree has branches to walk: no team without cells
            if k == "dense":      # every waiting agent's tree is one of the two largest the yard gives: full, all of them
                assert sum(v == MAX_NODES for v in nodes) >= n - 2, (batch, k, nodes)
                continue
            # many trees, most of them the waiting agents' (the same few shapes over and over), full ones beside them
            assert max(nodes) == MAX_NODES and len(set(nodes)) >= 3, (batch, k, sorted(set(nodes)))
            # the upstream trees of the same agents: real nodes beyond the root for everyone who is not DONE (a row of -inf is an absent node)
            assert all(np.isfinite(tree[i, 1:]).any() for i in range(n) if cases[k][2][i]["state"] != oc.DONE), (batch, k)
    assert len(Y40["crowd"][0]) > 32                                                             # more than one round of trees


def _run(out_path):
    """child: the three launches on every batch against the oracle; every tensor goes to out_path for the parent's byte comparison"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    keep = {}
    for batch, map_name, cases in BATCHES:
        names = list(cases)
        env = BatchedRailEnv([tf._static(map_name, cases[k][0], cases[k][1]) for k in names])
        assert env.max_nodes == MAX_NODES and env.pred_depth == 500
        pairs = [tf._rows(map_name, cases[k][0], cases[k][2]) for k in names]
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
                    exp_cu["adjacency"], exp_cu["node_order"], exp_cu["edge_order"] = tf._policy_form(exp_cu, b, A)
                for g, e in tf.CUTILS:
                    assert got[g][b].dtype == exp_cu[e].dtype, (g, got[g].dtype)
                    tf._same(got[g][b], exp_cu[e], f"{batch}/{k} {call} {g}")
                if tree is not None:
                    tf._same(tree[b], exp_tree, f"{batch}/{k} {call} depth-2 tree")
            for g, _ in tf.CUTILS:
                keep[f"{batch}/{call}/{g}"] = got[g]
            if tree is not None:
                keep[f"{batch}/{call}/tree"] = tree
        env.check()
        env.close()
    np.savez(out_path, **keep)
    print("DONE", len(keep), "tensors")


def test_even_slices_change_no_byte_and_equal_the_oracle(tmp_path):
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
    # up to 32 agents: the one-round kernels (both builders MODE 3, the builder alone MODE 6); 40 agents: rounds of trees (MODE 4 / 5, 7 / 8) --
    # on a launch class (compile-time carving) unless FL_OBS_NO_FIX asks for the runtime carving
    for tag, rec in records.items():
        assert len(rec) == 3 * len(BATCHES)
        for (batch, call), r in rec.items():
            if batch in ONE_ROUND:
                assert r["mode"] == (3 if call == "both" else 6) and r["nt"] == 1024 and r["tmask"] == 1 and r["split"] == 0, (tag, batch, call, r)
                assert (r["fix"] == 0) == (tag == "nofix"), (tag, batch, call, r)
            else:
                assert r["mode"] in ((4, 5) if call == "both" else (7, 8)) and r["tmask"] == 1, (tag, batch, call, r)
            if tag == "nofix":
                assert r["fix"] == 0, (tag, batch, call, r)
    for tag in ("ceil", "nomasks"):
        assert records[tag] == records["default"], tag
    a = outs["default"]
    assert len(a.files) == len(BATCHES) * (3 * len(tf.CUTILS) + 1)
    for tag, b in outs.items():
        assert sorted(a.files) == sorted(b.files), tag
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)


if __name__ == "__main__":
    _run(sys.argv[1])
