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
import sys

import numpy as np
import pytest

from tests import obs_switch_runs as sw
from tests.obs_switch_runs import MAX_NODES, X3, Y1, Y3, Y32, shape_of as _shape_of

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
# batch, map, {case: ((row, col, direction, target row, target col) per agent, speeds, the agents' states)}: tests/obs_switch_runs.py
BATCHES = (("y1", "yard", Y1), ("y3", "yard", Y3), ("x3", "crossing", X3), ("y32", "yard", Y32))
SWITCH_SETS = (("default", {}), ("nomasks", {"FL_OBS_NO_CF_DIRS": "1"}), ("latetopo", {"FL_OBS_NO_EARLY_TOPO": "1"}), ("nofix", {"FL_OBS_NO_FIX": "1"}))


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30) of the oracle set to the case's state; computed once"""
    map_name, cases = {b: (m, c) for b, m, c in BATCHES}[batch]
    return sw.oracle_case(sw.grid_of(map_name), cases[name])


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


def test_fill_and_early_topology_change_no_byte_and_equal_the_oracle(tmp_path):
    _reached()
    outs, records = sw.run_switch_sets(__file__, SWITCH_SETS, tmp_path, CHILD_TIMEOUT)
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
    sw.assert_same_bytes(outs, len(BATCHES) * (3 * len(sw.CUTILS) + 1))


if __name__ == "__main__":
    sw.run_batches([(b, sw.grid_of(m), c) for b, m, c in BATCHES], ("both", "alone", "policy"), sys.argv[1], oracle=_oracle)
