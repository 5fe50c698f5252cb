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
import sys

import numpy as np
import pytest

from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
MAX_NODES = sw.MAX_NODES
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


Y20 = {"crowd": sw.crowd(8), "dense": sw.dense(9)}
Y32 = dict(sw.Y32, dense=sw.dense(15))
Y40 = {"crowd": sw.crowd(18)}
BATCHES = (("y1", "yard", sw.Y1), ("x3", "crossing", sw.X3), ("y20", "yard", Y20), ("y32", "yard", Y32), ("y40", "yard", Y40))
ONE_ROUND = ("y1", "x3", "y20", "y32")
SWITCH_SETS = (("default", {}), ("ceil", {"FL_OBS_PB_CEIL_SPLIT": "1"}), ("nofix", {"FL_OBS_NO_FIX": "1"}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"}))


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30) of the oracle set to the case's state; computed once"""
    map_name, cases = {b: (m, c) for b, m, c in BATCHES}[batch]
    return sw.oracle_case(sw.grid_of(map_name), cases[name])


def _reached():
    """every batch reaches what it exists for, judged on the oracle's output"""
    y1 = {k: _oracle("y1", k)[0] for k in sw.Y1}
    assert all(v["forest"].shape[0] == 1 for v in y1.values())                                   # one tree of each builder: 62 of the 64 teams are empty
    assert any(sw.shape_of(v, 0)[0] == MAX_NODES for v in y1.values())
    x3 = {k: _oracle("x3", k)[0] for k in sw.X3}
    assert any(sw.shape_of(x3[k], i)[0] == MAX_NODES for k in sw.X3 for i in range(3))          # a tree that fills all 31 nodes
    for batch, cases, n in (("y20", Y20, 20), ("y32", Y32, 32), ("y40", Y40, 40)):
        for k in cases:
            cu, tree = _oracle(batch, k)
            assert len(cases[k][0]) == n and cu["forest"].shape[0] == n and tree.shape[0] == n
            nodes = [sw.shape_of(cu, i)[0] for i in range(n)]
            assert min(nodes) > 1, (batch, k, nodes)                                             # every agent's tree has branches to walk: no team without cells
            if k == "dense":      # every waiting agent's tree is one of the two largest the yard gives: full, all of them
                assert sum(v == MAX_NODES for v in nodes) >= n - 2, (batch, k, nodes)
                continue
            # many trees, most of them the waiting agents' (the same few shapes over and over), full ones beside them
            assert max(nodes) == MAX_NODES and len(set(nodes)) >= 3, (batch, k, sorted(set(nodes)))
            # the upstream trees of the same agents: real nodes beyond the root for everyone who is not DONE (a row of -inf is an absent node)
            assert all(np.isfinite(tree[i, 1:]).any() for i in range(n) if cases[k][2][i]["state"] != oc.DONE), (batch, k)
    assert len(Y40["crowd"][0]) > 32                                                             # more than one round of trees


def test_even_slices_change_no_byte_and_equal_the_oracle(tmp_path):
    _reached()
    outs, records = sw.run_switch_sets(__file__, SWITCH_SETS, tmp_path, CHILD_TIMEOUT)
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
    sw.assert_same_bytes(outs, len(BATCHES) * (3 * len(sw.CUTILS) + 1))


if __name__ == "__main__":
    sw.run_batches([(b, sw.grid_of(m), c) for b, m, c in BATCHES], ("both", "alone", "policy"), sys.argv[1], oracle=_oracle)
