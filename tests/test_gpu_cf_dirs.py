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
import sys

import numpy as np
import pytest

from tests import handmaps
from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M = oc.MOVING
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
# name -> ((row, col, direction, target row, target col) per agent, speeds, the agents' states)
YARD = sw.Y3
MESH = {"mesh": ([(2, 1, E, 2, 5), (2, 4, W, 2, 0), (0, 0, E, 4, 5)], [1.0, 0.5, 1.0], [oc.on(M, 2, 1, E), oc.on(M, 2, 4, W), oc.GONE])}
BATCHES = (("yard", YARD), ("mesh", MESH))
SWITCH_SETS = (("masks", {}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"}))


def _grid(batch):
    return handmaps.STEP_MAPS["yard"]()["grid"] if batch == "yard" else handmaps.full_grid(5, 6)


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30) of the oracle set to the case's state; computed once"""
    return sw.oracle_case(_grid(batch), dict(BATCHES)[batch][name])


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


def test_masks_change_no_byte_and_every_case_equals_the_oracle(tmp_path):
    _reached()
    outs, records = sw.run_switch_sets(__file__, SWITCH_SETS, tmp_path, CHILD_TIMEOUT)
    # the yard runs the one-round kernels (the masks' carving) under both switch values, the mesh the two-stage kernels without them
    for rec in records.values():
        assert rec[("yard", "both")]["mode"] == 3 and rec[("yard", "alone")]["mode"] == 6 and rec[("yard", "both")]["tmask"] == 1, rec
        assert rec[("mesh", "both")]["mode"] == 2 and rec[("mesh", "both")]["compact_t"] == 0 and rec[("mesh", "alone")]["mode"] == 0, rec
    assert records["masks"] == records["nomasks"]
    sw.assert_same_bytes(outs, 2 * (2 * len(sw.CUTILS) + 1))


if __name__ == "__main__":
    sw.run_batches([(b, _grid(b), c) for b, c in BATCHES], ("both", "alone"), sys.argv[1], oracle=_oracle)
