"""GPU: the one-round observation kernels (k_obs MODE 3 / 6: csrc/fl_obs_body.h, FLAT_FILL) fill the prediction index from ONE item space:
the waypoints 0 .. lp of all agents laid end to end (agent a owns the items incl[a - 1] .. incl[a] - 1), item t on lane t of the workgroup's
1 024, a further pass of the same body when an env has more items than lanes.  Every wavefront finds the agents of its 64 items from the
prefix of lp + 1 (two ballots, a compare-and-count through v_readlane) and requests the three path words of an item in front of the key scan.
The mapping changes no byte: every output of obs_both(2, 30), obs_cutils() and obs_policy() equals the oracle's (oracle.orc), with the launch
classes and with FL_OBS_NO_FIX=1 (the runtime carving of the same kernels).

The cases are the smallest at which the mapping can go wrong, on a long oval (12 x 30, a loop of 72 cells that a train follows clockwise or
counter-clockwise as it is oriented: the way to a cell just behind it is the whole loop) with a stub of three cells nobody reaches:

  o3    three agents: `small` (20 + 1 + 30 items: one partial wavefront, the agents' boundaries inside it; the middle agent is DONE: its one
        item is first and last of its piece at once), `unreach` (the middle agent's target lies on the stub: one waypoint between two long
        paths), `edge64` (64 + 30 + 41 = 135 items: the first boundary IS the wavefront boundary, the total no multiple of 64), `slow`
        (speed 1 / 12: the horizon of 500 steps cuts lp to 42 of 60 waypoints and the upstream index keeps three of them, lp2 = 2 < lp;
        beside it an agent of speed 1 whose lp2 = 29 is cut by the upstream depth 30, and one whose path of 12 waypoints is not cut at all)
  o32   32 agents, 26 of them waiting: `over` (1 117 items: a second pass that ends on a partial wavefront), `exact` (1 024 items: the first
        pass is full, no second one), `mid` (503 items, 16 an agent: every fourth boundary is a wavefront boundary, the last wavefront partial)

Each case asserts its edge on the CPU before anything runs on the GPU: the per-agent lp and lp2 are worked out from the oracle's distance map
(a flatland_cutils path has distance + 1 waypoints, one when the target cannot be reached or the agent is DONE; lp = min(n - 1, 499 // tpc + 1),
lp2 = min(min(n, 30) - 1, 30 // tpc)).  Each switch set runs in ONE fresh child process under a time limit; after a child that ends on a
signal or at its limit no other is started."""
import functools
import sys

import numpy as np
import pytest

from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw
from tests import util
from tests.handmaps import CURVE_NE, CURVE_NW, CURVE_SE, CURVE_SW, DEAD_E, DEAD_W, HORZ, VERT

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M, DONE, WAITING = oc.MOVING, oc.DONE, oc.WAITING
CHILD_TIMEOUT = 90      # a guard, not a measurement (a child takes a few seconds)
MAX_NODES, CU_PRED, PY_PRED, NT = 31, 500, 30, 1024
H, WD, TOP, BOTTOM, LEFT, RIGHT = 12, 30, 1, 10, 1, 28
STUB = (5, 11)


def long_oval():
    g = np.zeros((H, WD), dtype=np.uint16)
    g[TOP, LEFT], g[TOP, RIGHT], g[BOTTOM, LEFT], g[BOTTOM, RIGHT] = CURVE_SE, CURVE_SW, CURVE_NE, CURVE_NW
    g[TOP, LEFT + 1:RIGHT] = HORZ
    g[BOTTOM, LEFT + 1:RIGHT] = HORZ
    g[TOP + 1:BOTTOM, LEFT] = VERT
    g[TOP + 1:BOTTOM, RIGHT] = VERT
    g[5, 10], g[5, 11], g[5, 12] = DEAD_E, HORZ, DEAD_W      # a component of its own
    return g


def _loop():
    """the loop's cells clockwise from the top-left curve, with the orientation a clockwise train has on each"""
    cells = [(TOP, c, E) for c in range(LEFT + 1, RIGHT + 1)] + [(r, RIGHT, S) for r in range(TOP + 1, BOTTOM + 1)]
    cells += [(BOTTOM, c, W) for c in range(RIGHT - 1, LEFT - 1, -1)] + [(r, LEFT, N) for r in range(BOTTOM - 1, TOP - 1, -1)]
    return cells


LOOP = _loop()
assert len(LOOP) == 72 and len(set((r, c) for r, c, _ in LOOP)) == 72


def cw(start, n):
    """a clockwise agent that starts on the loop's cell `start` and whose path has n waypoints: (row, col, direction, target row, target col)"""
    r, c, d = LOOP[start % 72]
    tr, tc, _ = LOOP[(start + n - 1) % 72]
    return (r, c, d, tr, tc)


def _case(spec, speeds, states):
    return (spec, speeds, states)


def _waiting(ns, first=0, step=5):
    """waiting agents with paths of ns waypoints, their start cells spread over the loop"""
    return [cw(first + step * j, n) for j, n in enumerate(ns)]


def _o32(ns):
    """32 agents with paths of ns waypoints: six on the map (moving, on cells of their own), 26 waiting"""
    spec = _waiting(ns, first=0, step=2)
    states = [oc.on(M, *spec[j][0:3]) if j % 6 == 0 else oc.off(WAITING) for j in range(32)]
    return _case(spec, [1.0 if j % 3 else 0.5 for j in range(32)], states)


def _on(spec):
    return [oc.on(M, *s[0:3]) for s in spec]


O3 = {
    "small": _case([cw(3, 20), cw(40, 5), cw(50, 30)], [1.0, 1.0, 0.5], [oc.on(M, *cw(3, 20)[0:3]), oc.off(DONE, d=S), oc.on(M, *cw(50, 30)[0:3])]),
    "unreach": _case([cw(3, 41), cw(30, 9)[0:3] + STUB, cw(50, 45)], [1.0, 1.0, 1.0], _on([cw(3, 41), cw(30, 9), cw(50, 45)])),
    "edge64": _case([cw(3, 64), cw(20, 30), cw(60, 41)], [1.0, 0.5, 1.0], _on([cw(3, 64), cw(20, 30), cw(60, 41)])),
    "slow": _case([cw(3, 60), cw(20, 45), cw(60, 12)], [1 / 12, 1.0, 1.0], _on([cw(3, 60), cw(20, 45), cw(60, 12)])),
}
O32 = {
    "over": _o32([33 + j % 5 for j in range(32)]),
    "exact": _o32([31 + 2 * (j % 2) for j in range(32)]),
    "mid": _o32([16] * 31 + [7]),
}
BATCHES = (("o3", O3), ("o32", O32))
SWITCH_SETS = (("default", {}), ("nofix", {"FL_OBS_NO_FIX": "1"}))


@functools.lru_cache(maxsize=None)
def _oracle(batch, name):
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30, per-agent (n, lp, lp2)) of the oracle set to the case's
    state; computed once"""
    from oracle import orc
    spec, speed, agents = dict(BATCHES)[batch][name]
    dm, slot = orc.OracleEnv(util.plain_static(long_oval(), spec, speed)).distance_map()      # (of the map and the targets alone)
    pieces = []
    for i, a in enumerate(agents):
        if a["state"] == DONE:
            n = 1
        else:
            r, c, d = (a["r"], a["c"], a["d"]) if a["r"] >= 0 else spec[i][0:3]
            dist = int(dm[slot[i], r, c, d])
            n = 1 if dist == 0xFFFF else dist + 1
        tpc = int(np.reciprocal(np.float64(speed[i])))
        lp = max(0, min(n - 1, (CU_PRED - 1) // tpc + 1))
        lp2 = max(0, min(min(n, PY_PRED) - 1, PY_PRED // tpc))
        pieces.append((n, lp, lp2))
    return sw.oracle_case(long_oval(), (spec, speed, agents), max_nodes=MAX_NODES, cu_pred=CU_PRED, py_pred=PY_PRED) + (tuple(pieces),)


def _items(batch, name):
    p = _oracle(batch, name)[2]
    return [lp + 1 for _, lp, _ in p], p


def _reached():
    """every case has the edge it exists for, judged on the oracle's distance map"""
    it, p = _items("o3", "small")
    assert it == [20, 1, 30] and sum(it) < 64                                        # one partial wavefront, two boundaries inside it
    assert O3["small"][2][1]["state"] == DONE and p[1] == (1, 0, 0)                     # a DONE agent: one item, first and last at once
    it, p = _items("o3", "unreach")
    assert it == [41, 1, 45] and p[1][0] == 1                                         # an unreachable target between two long paths
    it, p = _items("o3", "edge64")
    assert it[0] == 64 and 64 < sum(it) < NT and sum(it) % 64 != 0                      # a boundary on the wavefront boundary
    it, p = _items("o3", "slow")
    assert p[0] == (60, 42, 2) and p[0][1] < p[0][0] - 1                              # the horizon cuts lp below n - 1, and lp2 < lp
    assert p[1] == (45, 44, 29) and p[2] == (12, 11, 11)                              # lp2 cut by the upstream depth; nothing cut
    it, p = _items("o32", "over")
    assert len(it) == 32 and sum(it) == 1117 and sum(it) > NT and sum(it) % 64 != 0     # a second pass that ends on a partial wavefront
    it, p = _items("o32", "exact")
    assert len(it) == 32 and sum(it) == NT                                            # exactly one full pass
    it, p = _items("o32", "mid")
    assert sum(it) == 503 and all(sum(it[:4 * q]) == 64 * q for q in range(1, 8))       # boundaries on the wavefront boundaries
    for batch, cases in BATCHES:                                                      # every piece longer than one item has both ends
        for k in cases:
            assert any(lp >= 1 for _, lp, _ in _oracle(batch, k)[2])


def test_flat_item_space_changes_no_byte_and_equals_the_oracle(tmp_path):
    _reached()
    outs, records = sw.run_switch_sets(__file__, SWITCH_SETS, tmp_path, CHILD_TIMEOUT)
    # every batch runs the one-round kernels: both builders MODE 3, the builder alone (int32 and the policy's int64 form) MODE 6
    for tag, rec in records.items():
        assert len(rec) == 3 * len(BATCHES)
        for (batch, call), r in rec.items():
            assert r["mode"] == (3 if call == "both" else 6) and r["nt"] == NT and r["split"] == 0, (tag, batch, call, r)
            assert (r["fix"] == 0) == (tag == "nofix"), (tag, batch, call, r)
    sw.assert_same_bytes(outs, len(BATCHES) * (3 * len(sw.CUTILS) + 1))


if __name__ == "__main__":
    sw.run_batches([(b, long_oval(), c) for b, c in BATCHES], ("both", "alone", "policy"), sys.argv[1], oracle=_oracle,
                   max_nodes=MAX_NODES, cu_pred=CU_PRED, py_pred=PY_PRED)
