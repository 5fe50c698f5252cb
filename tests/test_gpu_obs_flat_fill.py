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
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import handmaps, util
from tests import obs_state_cases as oc
from tests.handmaps import CURVE_NE, CURVE_NW, CURVE_SE, CURVE_SW, DEAD_E, DEAD_W, HORZ, VERT

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M, DONE, WAITING = oc.MOVING, oc.DONE, oc.WAITING
CUTILS = (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"), ("node_order", "node_order"), ("edge_order", "edge_order"),
          ("valid_actions", "valid"), ("props", "props"))
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


def _static(spec, speed):
    a = np.array(spec, dtype=np.int32)
    A = len(a)
    return dict(grid=long_oval(), init_pos=a[:, 0:2].copy(), init_dir=a[:, 2].copy(), target=a[:, 3:5].copy(), speed=np.array(speed, dtype=np.float64),
                earliest=np.zeros(A, dtype=np.int32), latest=np.full(A, 200, dtype=np.int32), T=400, malf_rate=0.0, malf_min=0, malf_max=0,
                mt_key=np.arange(624, dtype=np.uint32), mt_pos=624)


def _rows(spec, agents):
    grid = long_oval()
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
    """(flatland_cutils tensors at depth 500, upstream depth-2 tree at depth 30, per-agent (n, lp, lp2)) of the oracle set to the case's
    state; computed once"""
    from oracle import orc
    spec, speed, agents = dict(BATCHES)[batch][name]
    o = orc.OracleEnv(_static(spec, speed))
    st, aux = _rows(spec, agents)
    o.set_state(st, aux, 0, False)
    dm, slot = o.distance_map()
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
    tree = o.obs_pytree(2, PY_PRED)
    o.set_state(st, aux, 0, False)      # (a flatland_cutils call leaves its deadlock flags in the env)
    return o.obs_cutils(MAX_NODES, CU_PRED), tree, tuple(pieces)


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


def _same(got, exp, msg):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{msg}: shape {got.shape} vs {exp.shape}"
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{msg}: {len(bad)} mismatches, first {bad[0].tolist()}: {got[tuple(bad[0])]} vs {exp[tuple(bad[0])]}")


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


def _run(out_path):
    """child: the three launches on every batch against the oracle; every tensor goes to out_path for the parent's byte comparison"""
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    keep = {}
    for batch, cases in BATCHES:
        names = list(cases)
        env = BatchedRailEnv([_static(cases[k][0], cases[k][1]) for k in names])
        assert env.max_nodes == MAX_NODES and env.pred_depth == CU_PRED
        pairs = [_rows(cases[k][0], cases[k][2]) for k in names]
        states, aux = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        B, A = len(names), env.A

        def inject():
            env.set_state(states, aux, np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8))

        for call in ("both", "alone", "policy"):
            inject()
            tree = None
            if call == "both":
                got, tree = env.obs_both(2, PY_PRED)
                tree = tree.cpu().numpy()
            elif call == "alone":
                got = env.obs_cutils()
            else:
                pol = env.obs_policy()
                got = dict(env.obs_outputs(), agent_attr=pol[0], forest=pol[1], adjacency=pol[2], node_order=pol[3], edge_order=pol[4])
            print("RECORD", batch, call, json.dumps(env.last_obs_launch()), flush=True)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            for b, k in enumerate(names):
                exp_cu, exp_tree, _ = _oracle(batch, k)
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


def test_flat_item_space_changes_no_byte_and_equals_the_oracle(tmp_path):
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
    # every batch runs the one-round kernels: both builders MODE 3, the builder alone (int32 and the policy's int64 form) MODE 6
    for tag, rec in records.items():
        assert len(rec) == 3 * len(BATCHES)
        for (batch, call), r in rec.items():
            assert r["mode"] == (3 if call == "both" else 6) and r["nt"] == NT and r["split"] == 0, (tag, batch, call, r)
            assert (r["fix"] == 0) == (tag == "nofix"), (tag, batch, call, r)
    a = outs["default"]
    assert len(a.files) == len(BATCHES) * (3 * len(CUTILS) + 1)
    for tag, b in outs.items():
        assert sorted(a.files) == sorted(b.files), tag
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)


if __name__ == "__main__":
    _run(sys.argv[1])
