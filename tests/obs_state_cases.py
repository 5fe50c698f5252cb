"""Constructed agent states for the two tree observations -- the per-cell feature block of a branch walk (observations.py:295-374,
treeobs.cpp:329-476), which pass B of k_obs (csrc/fl_obs_passb.h) does not transcribe but re-derives: occupant maps folded into atomics, the
if / elif / elif over three times as six flag bits, the neighbouring waypoint's direction, the own-path filter, chunked scans of long lists.
Data and small constructors only -- numpy and tests/handmaps.py (and the loader of its own fixtures), nothing of the reference.  oracle/refharness/capture_obs_states.py sets every
case's state on the REAL RailEnv, calls the reference's own two builders and writes tests/golden/obs_states_<map>_<set>_<k>.npz;
tests/test_obs_states.py (CPU) asserts that every row of TABLE is reached by a case that names it -- judged on what the reference returned,
never on the inputs -- and that the oracle set to the state equals the reference; tests/test_gpu_obs_states.py compares k_obs with the
fixture, bit for bit, under the launcher switches that reach the compiled forms of pass B.

Maps: the rails of handmaps.STEP_MAPS (every cell a transition word RailEnvTransitions.is_valid accepts, asserted by the capture script: the
flatland_cutils attribute row is defined everywhere and compared whole).  The yard's symmetric switch and facing switch turn a train, so a
waypoint's direction differs from its neighbour's there; its bottom line is a single track on which two trains meet head-on.  No new map
was needed.

Agent sets (AGENTS[map][set]): "small", 8 agents, for the focused cases; "crowd", 24 agents of which many start on a few cells, for the long
lists.  A variant (VARIANTS[map][set]) gives the speeds and may move targets.

A case: map, set, variant, rows i32[A, 12] in util.STATE_NAMES order, aux i32[A, 4] (previous state, in_malfunction signal, deadlocked,
done), py_pred / cu_pred (the predictor depths the builders are called with: upstream ShortestPathPredictorForRailEnv(depth) under trees of
depth 2 and 3; flatland_cutils.TreeObsForRailEnv(31, depth)), rows (the TABLE rows it exists for), doc (one line), pins.

A pin: (row, builder, param, agent, node, control).  builder "py": node is a row of the dense upstream depth-3 tree (85 rows: a node, then its
L, F, R, B subtrees); "cu": a node index of the flatland_cutils forest.  The feature column is the row's (TABLE[row]["col"]).  The control
is the same case with ONE field of ONE agent changed -- (agent, field, value), field one of pos, dir, state, malf -- captured beside the case
as NAME~k.  The reference's value at the pin differs between case and control and has the kind the row names (KINDS).  The node of a pin is
data of this module (_NODES), written down from what the reference returned: oracle/refharness/capture_obs_states.py --pins prints, for every
pin, the nodes at which case and control differ.

Adding a case: append it in one of the builders below with its rows and pins (node None at first), run
oracle/refharness/capture_obs_states.py --pins where the reference lies and copy the node it prints into _NODES, run the capture, then
tests/test_obs_states.py: a case that misses a row it names fails there and names the row.

Time rows: TRUNCATIONS lists the (speed, tot_dist) pairs at which int(tot * time_per_cell) differs between float32 (treeobs.cpp:304, 378) and
float64 (observations.py:278, 328) or either differs from the exact quotient, searched by truncation_pairs() over the speeds 1/2 .. 1/64,
0.3, 0.7 and the walk lengths the maps allow (tot_dist <= MAX_WALK): float32 is one lower than float64 at the eleven speeds 1/7, 1/13, 1/14, 1/15,
1/26, 1/28, 1/30, 1/52, 1/56, 1/60, 1/63, at EVERY walk length (float(1 / float(1/7)) is 6.9999995); float64 is the exact quotient at every
speed and length of the search, 0.3 and 0.7 included, so no case can tell float64 from exact arithmetic -- tests/test_obs_states.py asserts
both findings.  The third clamp the horizon could show, tot_dist >= max_prediction_depth with predicted_time below it, does not exist:
predicted_time = int(tot_dist / speed) >= tot_dist for every speed <= 1.

Long lists: the items of a cell's key are appended through an atomic counter by wavefronts that race, so WHICH chunk of the conflict scan
holds an item is not decided by the inputs.  The crowd cases fix what the inputs can: more stays on the cell than CF_DIRECT (below it pass B
never splits a list) and than either chunk size, ONE item that conflicts (the lowest handle's, then the highest's), ONE item at the queried
time that hides ten hits a step later; wherever the race puts them, the chunk that holds the item has to deliver it."""
import fractions
import os

import numpy as np

from tests import handmaps, util

WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)
N, E, S, W = 0, 1, 2, 3
FEATURES = ("own_target", "other_target", "other_agent", "conflict", "unusable_switch", "next_branch", "min_target", "same_dir", "opp_dir",
            "malf", "speed", "ready")
COL = {f: k for k, f in enumerate(FEATURES)}
PY_ROWS = {2: 21, 3: 85}
CUTILS_KEYS = ("attr", "forest", "adjacency", "node_order", "edge_order", "valid", "p_dist_target", "p_deadlocked", "p_ready")
MAPS = handmaps.STEP_MAPS
MAX_WALK = 24      # the longest tot_dist of a depth-3 tree on these rails (the yard: stem, line, dead end and back)


# ---- int(tot * time_per_cell): float32, float64, exact
def truncation_pairs(max_walk=MAX_WALK):
    """(speed, tot, float32 value, float64 value, exact value) wherever the three are not the same.  The reference's own expressions:
    treeobs.cpp:304 / 378 `float time_per_cell = 1.0 / agent.speed; int predicted_time = (int)tot_dist * time_per_cell` with agent.speed a
    float; observations.py:278 / 328 `int(tot_dist * np.reciprocal(speed))` in double"""
    speeds = [(1.0 / n, fractions.Fraction(n)) for n in range(2, 65)] + [(0.3, fractions.Fraction(10, 3)), (0.7, fractions.Fraction(10, 7))]
    out = []
    for s, exact_tpc in speeds:
        tpc32 = np.float32(np.float64(1.0) / np.float64(np.float32(s)))
        tpc64 = np.reciprocal(np.float64(s))
        for tot in range(1, max_walk + 1):
            v32, v64 = int(np.float32(tot) * tpc32), int(np.float64(tot) * tpc64)
            exact = int(tot * exact_tpc)
            if not v32 == v64 == exact:
                out.append((s, tot, v32, v64, exact))
    return out


def _variant(speed, target=None):
    return dict(speed=[float(v) for v in speed], target=target)


# (row, col, direction, target row, target col) per agent
# small: agents 4 .. 6 start on agent 0's cell; the targets of 4 .. 7 lie on the yard's stub, which nobody reaches (a DONE agent there
# is out of every walk)
YARD_SMALL = [(4, 1, E, 4, 7), (4, 6, W, 4, 0), (3, 3, N, 1, 6), (1, 5, W, 1, 0), (4, 1, E, 6, 1), (4, 1, E, 6, 0), (4, 1, E, 6, 2), (4, 5, W, 6, 1)]
CROSSING_SMALL = [(4, 1, E, 4, 8), (1, 4, S, 8, 4), (4, 7, W, 4, 0), (7, 4, N, 0, 4), (6, 6, N, 4, 0), (4, 1, E, 7, 6), (4, 1, E, 4, 8), (4, 1, E, 8, 4)]
# the crowd: handles 0, 1, 22 and 23 travel; twenty start on two cells, ten each, and their shortest paths run to the far dead end and
# back: every one of them visits the cells between TWICE, so a cell's key holds 40 items and more
YARD_CROWD = ([(1, 5, W, 1, 0), (4, 1, E, 1, 6)] + [(4, 1, E, 4, 0), (4, 6, W, 4, 7)] * 10 + [(4, 5, W, 4, 0), (3, 3, N, 1, 6)])
CROSSING_CROWD = ([(1, 4, S, 8, 4), (7, 4, N, 0, 4)] + [(4, 1, E, 4, 0), (4, 7, W, 4, 8)] * 10 + [(6, 6, N, 4, 0), (4, 1, E, 7, 6)])
AGENTS = {"yard": {"small": YARD_SMALL, "crowd": YARD_CROWD}, "crossing": {"small": CROSSING_SMALL, "crowd": CROSSING_CROWD}}
SETS = tuple((m, s) for m in AGENTS for s in AGENTS[m])

VARIANTS = {
    ("yard", "small"): {
        "fast": _variant([1.0] * 8),
        # walker 1 at 1/2 meets a fast agent 0; 7 is slower than 3; 2 is the non-reciprocal speed
        "mixed": _variant([1.0, 1 / 2, 0.3, 1 / 3, 1.0, 1 / 2, 1 / 4, 1 / 4]),
        # a fast walker 1 (or 0) against slow predicted agents
        "slow_others": _variant([1.0, 1.0, 1 / 2, 1 / 4, 1.0, 1.0, 1.0, 1 / 2], target=[(4, 7), (4, 0), (1, 6), (1, 0), (6, 1), (6, 0), (6, 2), (4, 0)]),
        # (4, 4) is 7's target and lies on 0's and 1's walks; 0's own target is also 5's
        "targets": _variant([1.0] * 8, target=[(4, 7), (4, 0), (1, 6), (1, 0), (6, 1), (4, 7), (6, 2), (4, 4)]),
        # 1 / 7 is the fastest speed of TRUNCATIONS: float32 says int(1 * tpc) = 6, float64 and the exact quotient 7
        "trunc": _variant([1 / 7, 1.0, 1 / 13, 0.3, 0.7, 1.0, 1.0, 1.0]),
    },
    ("crossing", "small"): {
        "fast": _variant([1.0] * 8),
        "mixed": _variant([1 / 2, 1.0, 1 / 3, 0.3, 1 / 4, 1.0, 1.0, 1.0]),
    },
    ("yard", "crowd"): {"single": _variant([1.0, 1 / 3] + [1.0] * 20 + [1.0, 1 / 3]), "quarter": _variant([1 / 4, 1.0] + [1.0] * 20 + [1 / 4, 1.0])},
    ("crossing", "crowd"): {"fast": _variant([1.0] * 24)},
}


def static_of(map_name, set_name, variant):
    """the static description BatchedRailEnv / OracleEnv take (no malfunctions are drawn, a long episode)"""
    v = VARIANTS[(map_name, set_name)][variant]
    grid = MAPS[map_name]()["grid"]
    static = util.plain_static(grid, AGENTS[map_name][set_name], v["speed"], target=v["target"])
    for (r, c), d, (tr, tc) in zip(static["init_pos"], static["init_dir"], static["target"]):
        assert handmaps.nibble(grid[r, c], d) != 0 and grid[tr, tc] != 0
    return static


# ---- constructors
def on(state, r, c, d, malf=0):
    assert MOVING <= state <= MALF
    return dict(state=state, r=r, c=c, d=d, malf=malf)


def off(state=WAITING, d=None, malf=0):
    assert state <= MALF_OFF or state == DONE
    return dict(state=state, r=-1, c=-1, d=d, malf=malf)


GONE = off(DONE)
CASES = []
FIELDS = ("pos", "dir", "state", "malf")


def _rows(map_name, set_name, agents):
    spec = AGENTS[map_name][set_name]
    grid = MAPS[map_name]()["grid"]
    st = np.zeros((len(spec), 12), dtype=np.int32)
    aux = np.zeros((len(spec), 4), dtype=np.int32)
    for i, a in enumerate(agents):
        d = spec[i][2] if a["d"] is None else a["d"]
        if a["r"] >= 0:      # a train stands on rail and faces a way its cell allows
            assert handmaps.nibble(grid[a["r"], a["c"]], d) != 0, (i, a)
        st[i] = (a["r"], a["c"], d, a["state"], a["malf"], int(a["malf"] > 0), 0, 0, 1 if a["state"] == DONE else -1, a["r"], a["c"], d if a["r"] >= 0 else -1)
        aux[i] = (-1, int(a["malf"] > 0), 0, int(a["state"] == DONE))
    return st, aux


def changed(agents, control):
    """the agents of a control: ONE field of ONE agent changed"""
    i, field, value = control
    assert field in FIELDS
    a = dict(agents[i])
    if field == "pos":
        assert (a["r"] >= 0) and value[0] >= 0
        a["r"], a["c"] = value
    elif field == "dir":
        a["d"] = value
    elif field == "malf":
        a["malf"] = value
    else:      # a state of the same kind: on the map, or off it (DONE and the three off-map states have no position)
        assert (a["state"] in (MOVING, STOPPED, MALF)) == (value in (MOVING, STOPPED, MALF))
        a["state"] = value
    out = list(agents)
    out[i] = a
    return out


def pin(row, builder, param, agent, control):
    assert builder in ("py", "cu")
    return dict(row=row, builder=builder, param=param, agent=agent, control=tuple(control))


def case(name, map_name, set_name, variant, agents, rows, doc, pins=(), py_pred=(30,), cu_pred=(500,), default=GONE):
    spec = AGENTS[map_name][set_name]
    agents = list(agents) + [default] * (len(spec) - len(agents))
    assert len(agents) == len(spec) and isinstance(rows, tuple) and rows and "\n" not in doc and "~" not in name
    assert name not in {c["name"] for c in CASES}, name
    st, aux = _rows(map_name, set_name, agents)
    controls = []
    for p in pins:
        assert p["row"] in rows, (name, p["row"])
        if p["control"] not in controls:
            controls.append(p["control"])
        p["control_name"] = "%s~%d" % (name, controls.index(p["control"]))
        p["node"] = _NODES.get((name, p["row"], p["builder"], p["param"], p["agent"]))
    c = dict(name=name, map=map_name, set=set_name, variant=variant, agents=agents, state=st, aux=aux, rows=rows, doc=doc, pins=list(pins),
             py_pred=tuple(py_pred), cu_pred=tuple(cu_pred), control_of=None)
    CASES.append(c)
    for k, ctl in enumerate(controls):
        cst, caux = _rows(map_name, set_name, changed(agents, ctl))
        assert int((cst != st).any(axis=1).sum()) == 1
        CASES.append(dict(c, name="%s~%d" % (name, k), state=cst, aux=caux, rows=(), pins=[], control_of=name, doc="control of %s: agent %d's %s" % (name, ctl[0], ctl[1])))


def pin_key(p):
    return "py_d3_p%d" % p["param"] if p["builder"] == "py" else "cu_p%d_forest" % p["param"]


def both(row, agent, control, py=30, cu=500, at=None):
    """the pin in both builders"""
    return [dict(pin(row, "py", py, agent, control), at=at), dict(pin(row, "cu", cu, agent, control), at=at)]


def py_pin(row, agent, control, P=30, at=None):
    return [dict(pin(row, "py", P, agent, control), at=at)]


def cu_pin(row, agent, control, P=500, at=None):
    return [dict(pin(row, "cu", P, agent, control), at=at)]


def put(**by_handle):
    """agents by handle (a8=...), DONE wherever none is given"""
    n = max(int(k[1:]) for k in by_handle) + 1
    return [by_handle.get("a%d" % i, GONE) for i in range(n)]


# ---- the kinds of a pin: (value in the case, value in the control) of the reference, raw.  A flatland_cutils forest holds the features scaled
# (treeobs.cpp:111-152): distances divided by a per-agent length with inf as -1, counts divided by the number of agents, the speed as it is
def _inf(builder, v):
    return v == -1 if builder == "cu" else np.isposinf(v)


def _count(builder, v, A):
    return v * A if builder == "cu" else v


KINDS = {
    "finite": lambda b, v, c, A, arg: not _inf(b, v) and _inf(b, c),
    "inf": lambda b, v, c, A, arg: _inf(b, v) and not _inf(b, c),
    # a distance of `arg` cells (the scaled value of flatland_cutils: finite, and smaller / larger than the control's as arg says)
    "dist": lambda b, v, c, A, arg: (v == arg if b == "py" else not _inf(b, v)) and v != c,
    "count": lambda b, v, c, A, arg: abs(_count(b, v, A) - arg) < 1e-4 and v != c,
    "speed": lambda b, v, c, A, arg: v == (np.float32(arg) if b == "cu" else arg) and v != c,
}

# ---- the table: one row per branch of the per-cell feature block.  col: the feature; kind, arg: what the reference's value at the pin is (the
# builders differ where a pair is given: (upstream, flatland_cutils)); chain (time rows, upstream): which of the three times the reference's
# if / elif / elif took on the pin's cell -- recomputed by chain_of() from the builder's own predicted_pos / predicted_dir -- whether an agent
# there satisfied the condition, and whether a LATER time of the chain held a hit that the elif hid
_R = "observations.py:%s / treeobs.cpp:%s"


def _row(ref, col, kind, arg=None, builders=("py", "cu"), chain=None):
    return dict(ref=ref, col=col, kind=kind, arg=arg, builders=builders, chain=chain)


TABLE = {
    # occupant
    "occ.same_dir": _row(_R % ("305-307", "347-349"), "same_dir", "count", 1),
    "occ.opp_dir": _row(_R % ("314-317", "358-364"), "opp_dir", "count", 1),
    "occ.malf": _row(_R % ("300-301", "336-340"), "malf", "count", (5, 1)),           # the down counter upstream, a flag for flatland_cutils (loader.cpp:38-39)
    "occ.malf_max": _row("observations.py:300-301", "malf", "count", 7, builders=("py",)),      # two on one branch: the larger counter, whichever comes first
    "occ.speed_min": _row(_R % ("310-312", "352-357"), "speed", "speed", 0.25),       # a slower and a faster one in the same direction
    "occ.speed_full": _row(_R % ("310-312", "352-357"), "speed", "speed", 1.0),       # a full-speed occupant in the same direction: nothing below 1.0
    "occ.ready_1": _row(_R % ("106-109, 303", "82-91, 342-345"), "ready", "count", (1, 0)),      # flatland_cutils starts the count at 0
    "occ.ready_2": _row(_R % ("106-109, 303", "82-91, 342-345"), "ready", "count", (2, 1)),
    "occ.ready_3": _row(_R % ("106-109, 303", "82-91, 342-345"), "ready", "count", (3, 2)),
    "occ.ready_no_occupant": _row(_R % ("295, 303", "329, 342"), "ready", "count", 0),           # counted only under `position in location_has_agent`
    "occ.stack_dir": _row(_R % ("99-100, 317", "76-77, 362"), "opp_dir", "count", 1),            # two trains on a cell: the highest handle's direction, and +1, not +2
    "occ.stack_malf": _row(_R % ("102-103", "79-80"), "malf", "count", (2, 1)),                  # ... its counter, not the larger one below it
    "occ.stack_speed": _row(_R % ("101", "78"), "speed", "speed", 0.5),                          # ... its speed, not the slower one below it
    "occ.first_of_two": _row(_R % ("296-297", "330-332"), "other_agent", "dist", 2),
    # conflict
    "cf.pt_true": _row(_R % ("337-345", "403-422"), "conflict", "dist", 2, chain=dict(branch=0, cond=True)),
    "cf.pt_false": _row(_R % ("337-345", "403-422"), "conflict", "inf", chain=dict(branch=0, cond=False)),
    "cf.elif_hides_pre": _row(_R % ("337, 348", "403, 423"), "conflict", "inf", chain=dict(branch=0, cond=False, hidden=1)),
    # (upstream; what flatland_cutils says on this cell is the row cf.cu_dir_pre)
    "cf.pre_only": _row("observations.py:348-356", "conflict", "dist", 3, builders=("py",), chain=dict(branch=1, cond=True)),
    "cf.post_only": _row(_R % ("359-367", "443-462"), "conflict", "dist", 2, chain=dict(branch=2, cond=True)),
    # flatland_cutils reads predicted_dir[predicted_time] in the pre / post branches: on a curve that is the neighbouring waypoint's direction
    "cf.cu_dir_pre": _row("treeobs.cpp:429-433", "conflict", "inf", builders=("cu",), chain=dict(branch=1, cond=True, cond_at_pt=False)),
    # (7: nothing on (3, 3) at tot_dist 3 nor on the switch at 4; the DONE agent 1 stands on (4, 0) at the end of the walk)
    "cf.cu_dir_post": _row("treeobs.cpp:449-453", "conflict", "dist", 7, builders=("cu",), chain=dict(branch=2, cond=True, cond_at_pt=False)),
    # (8: nothing on the switch at tot_dist 5; the DONE agent 1 stands on (4, 0) at the end of the walk)
    "cf.reverse_fails": _row(_R % ("340-342", "409-413"), "conflict", "dist", 8, chain=dict(branch=0, cond=False)),
    "cf.done_same": _row(_R % ("344-345", "417-420"), "conflict", "dist", 2, chain=dict(branch=0, cond=True, done=True)),
    "cf.done_opp": _row(_R % ("344-345", "417-420"), "conflict", "dist", 2, chain=dict(branch=0, cond=True, done=True)),
    "cf.own_alone": _row(_R % ("337-338", "392-406"), "conflict", "inf", chain=dict(branch=None)),
    "cf.own_with_other": _row(_R % ("337-338", "392-406"), "conflict", "dist", 2, chain=dict(branch=0, cond=True, own=True)),
    "cf.off_map_predicted": _row("predictions.py:130-131 / predictions.cpp:146-235", "conflict", "finite"),
    "cf.no_path_stands": _row("predictions.py:161-164", "conflict", "dist", 5, chain=dict(branch=0, cond=True)),
    "cf.arrives_and_stays": _row("predictions.py:161-164", "conflict", "dist", 3, chain=dict(branch=0, cond=True)),
    # time
    "time.trunc_f32": _row("treeobs.cpp:304, 378", "conflict", "finite", builders=("cu",)),
    "time.trunc_f64": _row("observations.py:278, 328", "conflict", "inf", builders=("py",), chain=dict(branch=None)),
    "time.slow_walker": _row(_R % ("328", "378"), "conflict", "dist", 2, chain=dict(branch=1, cond=True)),
    "time.fast_walker": _row(_R % ("328", "378"), "conflict", "dist", 3, chain=dict(branch=2, cond=True)),
    "time.last_step": _row(_R % ("333-334", "384-389"), "conflict", "dist", 4, chain=dict(branch=0, cond=True, pt_is_last=True)),
    "time.beyond_horizon": _row(_R % ("329-331", "379-383"), "conflict", "inf"),
    # targets
    "tg.other": _row("observations.py:369-371", "other_target", "dist", 2, builders=("py",)),
    "tg.own": _row(_R % ("373-374", "474-476"), "own_target", "dist", 6),
    "tg.own_not_other": _row("observations.py:369", "other_target", "inf", builders=("py",)),
    "tg.cutils_never": _row("treeobs.cpp:72, 467", "other_target", "never", builders=("cu",)),
    "cf.elif_hides_post": _row(_R % ("337, 359", "403, 443"), "conflict", "dist", 4, chain=dict(branch=0, cond=False, hidden=2)),
    # long lists (the crowd).  The chain is recomputed from the UPSTREAM predictor's arrays; flatland_cutils moves a slow agent at t = 1 and then
    # every int(1 / speed) steps (predictions.cpp:146-235), so its conflict falls a cell earlier (tot_dist 4, not 5, in the two single-item
    # cases): its pins hold the forest's value against the control's, on a walk whose cells all hold 40 items and more
    "ll.single_at_pt": _row(_R % ("337-345", "403-422"), "conflict", "dist", 3, chain=dict(branch=0, cond=True, long=True)),
    "ll.single_low": _row(_R % ("337-345", "403-422"), "conflict", "dist", 5, chain=dict(branch=0, cond=True, long=True)),
    "ll.single_high": _row(_R % ("337-345", "403-422"), "conflict", "dist", 5, chain=dict(branch=0, cond=True, long=True)),
    "ll.hider": _row(_R % ("337, 359", "403, 443"), "conflict", "inf", chain=dict(branch=0, cond=False, hidden=2, long=True)),
    # root
    "root.virtual_done": _row(_R % ("204-205, 219-221", "154-200"), "min_target", "dist", 0),
    "root.virtual_off_map": _row(_R % ("200-201, 219-221", "154-200"), "min_target", "dist", 6),
    "root.malf": _row(_R % ("223", "154-200"), "malf", "count", (3, 1)),
    "root.reoriented": _row("observations.py:236-237", "next_branch", "reoriented", builders=("py",)),
}


def kind_of(row, builder):
    t = TABLE[row]
    kind = t["kind"] if isinstance(t["kind"], str) else t["kind"][0 if builder == "py" else 1]
    arg = t["arg"][0 if builder == "py" else 1] if isinstance(t["arg"], tuple) else t["arg"]
    return kind, arg


def chain_of(grid, pred_pos, pred_dir, states, handle, speed, at):
    """the reference's if / elif / elif of observations.py:329-367 on ONE cell, recomputed from the builder's own predicted_pos /
    predicted_dir: at = (row, col, walking direction, tot_dist).  Returns None when no test is made (predicted_time or tot_dist beyond the
    horizon), else dict(pt, times, branch (0, 1, 2: the first time of pt, pt - 1, pt + 1 with somebody else on the cell; None: nobody),
    agents (those on the cell then, the walker included), cond (per such agent: the conflict condition with the direction at THAT time),
    cond_at_pt (... with the direction at pt, as treeobs.cpp reads it), later (time index -> a condition holds there))"""
    r, c, d, tot = at
    T, A = pred_pos.shape
    pt = int(tot * np.reciprocal(np.float64(speed)))
    if not (pt < T and tot < T):
        return None
    times = [pt, max(0, pt - 1), min(T - 1, pt + 1)]
    pos = c * grid.shape[1] + r      # (coordinate_to_position: column-major on the width)
    bits = handmaps.nibble(grid[r, c], d)

    def cond(a, t):
        cd = int(pred_dir[t, a])
        return bool((d != cd and (bits >> (3 - (cd + 2) % 4)) & 1) or states[a] == DONE)

    there = [[a for a in range(A) if pred_pos[t, a] == pos] for t in times]
    branch = next((k for k in range(3) if any(a != handle for a in there[k])), None)
    out = dict(pt=pt, times=times, branch=branch, agents=[], cond=[], cond_at_pt=[], later={}, T=T)
    if branch is not None:
        out["agents"] = there[branch]
        out["cond"] = [cond(a, times[branch]) for a in there[branch]]
        out["cond_at_pt"] = [cond(a, pt) for a in there[branch]]
        out["later"] = {k: any(cond(a, times[k]) for a in there[k] if a != handle) for k in range(branch + 1, 3)}
    return out


def visits_of(pred_pos, cell, width):
    """how many separate stays on the cell the predictions hold (the items of the cell's key)"""
    on = (pred_pos == cell[1] * width + cell[0])
    return int(on[0].sum() + (on[1:] & ~on[:-1]).sum())


# ---- the nodes of the pins, as oracle/refharness/capture_obs_states.py --pins printed them: (case, row, builder, param, agent) -> node
_NODES = {
    ('occ_same', 'occ.same_dir', 'py', 30, 1): 22,
    ('occ_same', 'occ.same_dir', 'cu', 500, 1): 2,
    ('occ_opp', 'occ.opp_dir', 'py', 30, 1): 22,
    ('occ_opp', 'occ.opp_dir', 'cu', 500, 1): 2,
    ('occ_malf', 'occ.malf', 'py', 30, 1): 22,
    ('occ_malf', 'occ.malf', 'cu', 500, 1): 2,
    ('occ_malf_max_far', 'occ.malf_max', 'py', 30, 1): 22,
    ('occ_malf_max_near', 'occ.malf_max', 'py', 30, 1): 22,
    ('occ_slower', 'occ.speed_min', 'py', 30, 1): 22,
    ('occ_slower', 'occ.speed_min', 'cu', 500, 1): 2,
    ('occ_full_speed', 'occ.speed_full', 'py', 30, 1): 22,
    ('occ_full_speed', 'occ.speed_full', 'cu', 500, 1): 2,
    ('ready_3', 'occ.ready_3', 'py', 30, 1): 22,
    ('ready_3', 'occ.ready_3', 'cu', 500, 1): 2,
    ('ready_2', 'occ.ready_2', 'py', 30, 1): 22,
    ('ready_2', 'occ.ready_2', 'cu', 500, 1): 2,
    ('ready_1', 'occ.ready_1', 'py', 30, 1): 22,
    ('ready_1', 'occ.ready_1', 'cu', 500, 1): 2,
    ('ready_no_occupant', 'occ.ready_no_occupant', 'py', 30, 1): 22,
    ('ready_no_occupant', 'occ.ready_no_occupant', 'cu', 500, 1): 2,
    ('stack_dir', 'occ.stack_dir', 'py', 30, 1): 22,
    ('stack_dir', 'occ.stack_dir', 'cu', 500, 1): 2,
    ('stack_dir', 'occ.stack_malf', 'py', 30, 1): 22,
    ('stack_dir', 'occ.stack_malf', 'cu', 500, 1): 2,
    ('stack_speed', 'occ.stack_speed', 'py', 30, 1): 22,
    ('stack_speed', 'occ.stack_speed', 'cu', 500, 1): 2,
    ('first_of_two', 'occ.first_of_two', 'py', 30, 1): 22,
    ('first_of_two', 'occ.first_of_two', 'cu', 500, 1): 2,
    ('x_ready_3', 'occ.ready_3', 'py', 30, 2): 22,
    ('x_ready_3', 'occ.ready_3', 'cu', 500, 2): 2,
    ('x_diamond_hides', 'cf.elif_hides_post', 'py', 30, 1): 22,
    ('x_diamond_hides', 'cf.elif_hides_post', 'cu', 500, 1): 2,
    ('x_spur', 'occ.opp_dir', 'py', 30, 0): 33,
    ('x_spur', 'occ.opp_dir', 'cu', 500, 0): 6,
    ('x_spur', 'occ.malf', 'py', 30, 0): 33,
    ('x_spur', 'occ.malf', 'cu', 500, 0): 6,
    ('x_root_states', 'root.virtual_done', 'py', 30, 6): 0,
    ('x_root_states', 'root.virtual_done', 'cu', 500, 6): 0,
    ('x_root_states', 'root.malf', 'py', 30, 2): 0,
    ('x_root_states', 'root.malf', 'cu', 500, 2): 0,
    ('xl_diamond', 'll.single_at_pt', 'py', 30, 0): 22,
    ('xl_diamond', 'll.single_at_pt', 'cu', 500, 0): 2,
    ('cf_pt_true', 'cf.pt_true', 'py', 30, 1): 22,
    ('cf_pt_true', 'cf.pt_true', 'cu', 500, 1): 2,
    ('cf_pt_true', 'cf.own_with_other', 'py', 30, 1): 22,
    ('cf_pt_true', 'cf.own_with_other', 'cu', 500, 1): 2,
    ('cf_pt_false', 'cf.pt_false', 'py', 30, 1): 22,
    ('cf_pt_false', 'cf.pt_false', 'cu', 500, 1): 2,
    ('cf_elif_hides', 'cf.elif_hides_pre', 'py', 30, 1): 22,
    ('cf_elif_hides', 'cf.elif_hides_pre', 'cu', 500, 1): 2,
    ('cf_pre_only', 'cf.pre_only', 'py', 30, 1): 22,
    ('cf_pre_only', 'cf.cu_dir_pre', 'cu', 500, 1): 2,
    ('cf_post_only', 'cf.post_only', 'py', 30, 1): 22,
    ('cf_post_only', 'cf.post_only', 'cu', 500, 1): 2,
    ('cf_cu_post_curve', 'cf.cu_dir_post', 'cu', 500, 3): 2,
    ('cf_reverse_fails', 'cf.reverse_fails', 'py', 30, 3): 22,
    ('cf_reverse_fails', 'cf.reverse_fails', 'cu', 500, 3): 2,
    ('cf_no_path', 'cf.no_path_stands', 'py', 30, 3): 22,
    ('cf_no_path', 'cf.no_path_stands', 'cu', 500, 3): 2,
    ('cf_done_same', 'cf.done_same', 'py', 30, 1): 22,
    ('cf_done_same', 'cf.done_same', 'cu', 500, 1): 2,
    ('cf_done_opp', 'cf.done_opp', 'py', 30, 1): 22,
    ('cf_done_opp', 'cf.done_opp', 'cu', 500, 1): 2,
    ('cf_own_alone', 'cf.own_alone', 'py', 30, 1): 22,
    ('cf_own_alone', 'cf.own_alone', 'cu', 500, 1): 2,
    ('cf_off_map', 'cf.off_map_predicted', 'py', 30, 1): 22,
    ('cf_off_map', 'cf.off_map_predicted', 'cu', 500, 1): 2,
    ('cf_arrives_stays', 'cf.arrives_and_stays', 'py', 30, 0): 28,
    ('cf_arrives_stays', 'cf.arrives_and_stays', 'cu', 500, 0): 5,
    ('time_trunc', 'time.trunc_f32', 'cu', 500, 0): 2,
    ('time_trunc', 'time.trunc_f64', 'py', 30, 0): 22,
    ('time_slow_walker', 'time.slow_walker', 'py', 30, 1): 22,
    ('time_slow_walker', 'time.slow_walker', 'cu', 500, 1): 2,
    ('time_fast_walker', 'time.fast_walker', 'py', 30, 0): 28,
    ('time_fast_walker', 'time.fast_walker', 'cu', 500, 0): 5,
    ('time_clamps', 'time.last_step', 'py', 4, 1): 22,
    ('time_clamps', 'time.last_step', 'cu', 4, 1): 2,
    ('time_clamps', 'time.beyond_horizon', 'py', 3, 1): 22,
    ('time_clamps', 'time.beyond_horizon', 'cu', 3, 1): 2,
    ('tg_other', 'tg.other', 'py', 30, 1): 22,
    ('tg_other', 'tg.own', 'py', 30, 1): 22,
    ('tg_other', 'tg.own', 'cu', 500, 1): 2,
    ('tg_other', 'tg.cutils_never', 'cu', 500, 1): 2,
    ('tg_own_not_other', 'tg.own_not_other', 'py', 30, 0): 22,
    ('root_states', 'root.virtual_done', 'py', 30, 6): 0,
    ('root_states', 'root.virtual_done', 'cu', 500, 6): 0,
    ('root_states', 'root.virtual_off_map', 'py', 30, 0): 0,
    ('root_states', 'root.virtual_off_map', 'cu', 500, 0): 0,
    ('root_states', 'root.malf', 'py', 30, 2): 0,
    ('root_states', 'root.malf', 'cu', 500, 2): 0,
    ('root_dead_end', 'root.reoriented', 'py', 30, 1): 22,
    ('ll_single_low', 'll.single_low', 'py', 30, 0): 22,
    ('ll_single_low', 'll.single_low', 'cu', 500, 0): 2,
    ('ll_single_high', 'll.single_high', 'py', 30, 0): 22,
    ('ll_single_high', 'll.single_high', 'cu', 500, 0): 2,
    ('ll_hider', 'll.hider', 'py', 30, 0): 22,
    ('ll_hider', 'll.hider', 'cu', 500, 0): 2,
}

M, ST, MF = MOVING, STOPPED, MALF


def _yard_occupant_cases():
    """walker 1 heads west along the bottom line: (4, 5) at tot_dist 1 .. its target (4, 0) at 6, one node"""
    W1 = on(M, 4, 6, W)
    case("occ_same", "yard", "small", "fast", put(a1=W1, a7=on(M, 4, 4, W)), ("occ.same_dir",), "a train ahead, facing the same way",
         both("occ.same_dir", 1, (7, "dir", E)))
    case("occ_opp", "yard", "small", "fast", put(a1=W1, a7=on(M, 4, 4, E)), ("occ.opp_dir",), "a train ahead, facing the walker",
         both("occ.opp_dir", 1, (7, "dir", W)))
    case("occ_malf", "yard", "small", "fast", put(a1=W1, a7=on(MF, 4, 4, W, malf=5)), ("occ.malf",), "a broken-down train ahead, counter 5",
         both("occ.malf", 1, (7, "malf", 0)))
    case("occ_malf_max_far", "yard", "small", "fast", put(a0=on(MF, 4, 2, E, malf=7), a1=W1, a7=on(MF, 4, 4, W, malf=3)), ("occ.malf_max",),
         "two broken-down trains on one branch, the farther one with the larger counter", py_pin("occ.malf_max", 1, (0, "malf", 2)))
    case("occ_malf_max_near", "yard", "small", "fast", put(a0=on(MF, 4, 2, E, malf=3), a1=W1, a7=on(MF, 4, 4, W, malf=7)), ("occ.malf_max",),
         "... the nearer one with the larger counter", py_pin("occ.malf_max", 1, (7, "malf", 2)))
    case("occ_slower", "yard", "small", "mixed", put(a1=W1, a3=on(M, 4, 2, W), a7=on(M, 4, 4, W)), ("occ.speed_min",),
         "speeds 1/4 and 1/3 ahead in the walker's direction: the slower one is reported", both("occ.speed_min", 1, (7, "dir", E)))
    case("occ_full_speed", "yard", "small", "mixed", put(a0=on(M, 4, 4, W), a1=W1, a3=on(M, 4, 2, E)), ("occ.speed_full",),
         "a full-speed train in the walker's direction and a slow one against it: 1.0", both("occ.speed_full", 1, (3, "dir", W)))
    S0 = on(ST, 4, 1, E)
    case("ready_3", "yard", "small", "fast", put(a0=S0, a1=W1, a4=off(WAITING), a5=off(READY), a6=off(MALF_OFF, malf=2)), ("occ.ready_3",),
         "three agents off the map, one in each off-map state, on a start cell that holds a train", both("occ.ready_3", 1, (6, "state", DONE)))
    case("ready_2", "yard", "small", "fast", put(a0=S0, a1=W1, a4=off(WAITING), a5=off(READY)), ("occ.ready_2",),
         "two agents off the map on the occupied start cell", both("occ.ready_2", 1, (5, "state", DONE)))
    case("ready_1", "yard", "small", "fast", put(a0=S0, a1=W1, a4=off(WAITING)), ("occ.ready_1",),
         "one agent off the map on the occupied start cell: upstream counts 1, flatland_cutils 0",
         py_pin("occ.ready_1", 1, (4, "state", DONE)) + cu_pin("occ.ready_1", 1, (5, "state", WAITING)))
    case("ready_no_occupant", "yard", "small", "fast", put(a0=on(ST, 4, 2, E), a1=W1, a4=off(WAITING), a5=off(READY), a6=off(MALF_OFF, malf=2)),
         ("occ.ready_no_occupant",), "the same three agents, the train one cell further: nothing is counted", both("occ.ready_no_occupant", 1, (0, "pos", (4, 1))))
    case("stack_dir", "yard", "small", "fast", put(a0=on(MF, 4, 4, W, malf=9), a1=W1, a7=on(MF, 4, 4, E, malf=2)), ("occ.stack_dir", "occ.stack_malf"),
         "two trains on one cell, the lower handle facing west with counter 9, the higher east with 2: one train against the walker, counter 2",
         both("occ.stack_dir", 1, (7, "dir", W)) + both("occ.stack_malf", 1, (7, "malf", 0)))
    case("stack_speed", "yard", "small", "mixed", put(a1=W1, a3=on(M, 4, 4, W), a5=on(M, 4, 4, W)), ("occ.stack_speed",),
         "speeds 1/3 (handle 3) and 1/2 (handle 5) on one cell: the higher handle's", both("occ.stack_speed", 1, (5, "dir", E)))
    case("first_of_two", "yard", "small", "fast", put(a0=on(M, 4, 2, E), a1=W1, a7=on(M, 4, 4, W)), ("occ.first_of_two",),
         "trains at distance 2 and 4 on one branch", both("occ.first_of_two", 1, (7, "pos", (4, 3))))


def _yard_conflict_cases():
    W1 = on(M, 4, 6, W)
    case("cf_pt_true", "yard", "small", "fast", put(a0=on(M, 4, 2, E), a1=W1), ("cf.pt_true", "cf.own_with_other"),
         "head-on at an even distance: both are predicted on (4, 4) at t = 2, the walker itself included",
         both("cf.pt_true", 1, (0, "dir", W), at=(4, 4, W, 2)) + both("cf.own_with_other", 1, (0, "dir", W), at=(4, 4, W, 2)))
    case("cf_pt_false", "yard", "small", "slow_others", put(a1=W1, a7=on(M, 4, 5, W)), ("cf.pt_false",),
         "a slower train ahead in the same direction: on the cell at the queried time, without the condition",
         both("cf.pt_false", 1, (7, "dir", E), at=(4, 5, W, 1)))
    case("cf_elif_hides", "yard", "small", "slow_others", put(a0=on(M, 4, 3, E), a1=W1, a7=on(M, 4, 5, W)), ("cf.elif_hides_pre",),
         "on (4, 4) the slow train ahead is there at pt without the condition, the oncoming one at pt - 1 with it: no conflict",
         both("cf.elif_hides_pre", 1, (7, "pos", (4, 1)), at=(4, 4, W, 2)))
    case("cf_pre_only", "yard", "small", "fast", put(a1=W1, a2=on(M, 4, 1, E)), ("cf.pre_only", "cf.cu_dir_pre"),
         "agent 2 passes the facing switch at t = 2 and turns up the stem: on (4, 3) at pt - 1 only; at pt it faces north",
         py_pin("cf.pre_only", 1, (2, "pos", (4, 2)), at=(4, 3, W, 3)) + cu_pin("cf.cu_dir_pre", 1, (1, "pos", (4, 5)), at=(4, 3, W, 3)))
    case("cf_post_only", "yard", "small", "fast", put(a0=on(M, 4, 1, E), a1=W1), ("cf.post_only",),
         "head-on at an odd distance: the other is on (4, 4) at pt + 1", both("cf.post_only", 1, (0, "dir", W), at=(4, 4, W, 2)))
    case("cf_cu_post_curve", "yard", "small", "fast", put(a2=on(M, 4, 0, W), a3=on(M, 1, 4, W)), ("cf.cu_dir_post",),
         "agent 2 turns up the stem on the facing switch: on (3, 3) at pt + 1 facing north, head-on for walker 3; at pt it is on the switch, facing east",
         cu_pin("cf.cu_dir_post", 3, (2, "pos", (4, 1)), at=(3, 3, S, 3)))
    case("cf_reverse_fails", "yard", "small", "fast", put(a3=on(M, 1, 5, W), a4=on(ST, 4, 3, W)), ("cf.reverse_fails",),
         "walker 3 comes down the stem onto the switch, where agent 4 (no path: it stands) faces west: another direction, no way back along it",
         both("cf.reverse_fails", 3, (4, "dir", E), at=(4, 3, S, 5)))
    case("cf_no_path", "yard", "small", "fast", put(a3=on(M, 1, 5, W), a4=on(ST, 4, 3, E)), ("cf.no_path_stands",),
         "agent 4's target is unreachable: predicted on its cell for the whole horizon", both("cf.no_path_stands", 3, (4, "dir", W), at=(4, 3, S, 5)))
    case("cf_done_same", "yard", "small", "targets", put(a1=W1, a7=off(DONE, d=W)), ("cf.done_same",),
         "a DONE agent on its target (4, 4), facing the walker's way", both("cf.done_same", 1, (7, "state", WAITING), at=(4, 4, W, 2)))
    case("cf_done_opp", "yard", "small", "targets", put(a1=W1, a7=off(DONE, d=E)), ("cf.done_opp",),
         "a DONE agent on its target, facing the walker", both("cf.done_opp", 1, (7, "state", READY), at=(4, 4, W, 2)))
    case("cf_own_alone", "yard", "small", "fast", put(a1=W1), ("cf.own_alone",), "nobody else: the walker's own prediction is on every cell at the queried time",
         both("cf.own_alone", 1, (0, "state", WAITING), at=(4, 4, W, 2)))
    case("cf_off_map", "yard", "small", "fast", put(a0=off(WAITING), a1=W1), ("cf.off_map_predicted",),
         "agent 0 waits off the map: predicted from its start cell", both("cf.off_map_predicted", 1, (0, "state", DONE)))
    case("cf_arrives_stays", "yard", "small", "targets", put(a0=on(M, 4, 1, E), a7=on(M, 4, 5, W)), ("cf.arrives_and_stays",),
         "agent 7 reaches its target (4, 4) at t = 1 and stays: walker 0 meets it there at t = 3", both("cf.arrives_and_stays", 0, (7, "dir", E), at=(4, 4, E, 3)))


def _yard_time_cases():
    W1 = on(M, 4, 6, W)
    case("time_trunc", "yard", "small", "trunc", put(a0=on(M, 4, 1, E), a1=on(M, 4, 7, E)), ("time.trunc_f32", "time.trunc_f64"),
         "walker 0 at speed 1/7, tot_dist 1: float32 says t = 6, float64 t = 7; agent 1 is on (4, 2) at t = 5 only",
         cu_pin("time.trunc_f32", 0, (1, "pos", (4, 4))) + py_pin("time.trunc_f64", 0, (1, "pos", (4, 4)), at=(4, 2, E, 1)))
    case("time_slow_walker", "yard", "small", "mixed", put(a0=on(M, 4, 1, E), a1=W1), ("time.slow_walker",),
         "walker 1 at speed 1/2 against a full-speed agent 0: on (4, 4) at tot_dist 2 it asks for t = 4", both("time.slow_walker", 1, (0, "pos", (4, 2)), at=(4, 4, W, 2)))
    case("time_fast_walker", "yard", "small", "mixed", put(a0=on(M, 4, 1, E), a1=W1), ("time.fast_walker",),
         "walker 0 at full speed against agent 1 at 1/2", both("time.fast_walker", 0, (1, "dir", E), at=(4, 4, E, 3)))
    case("time_clamps", "yard", "small", "fast", put(a1=W1, a4=on(ST, 4, 2, E)), ("time.last_step", "time.beyond_horizon"),
         "agent 4 stands on (4, 2), tot_dist 4: the last step of a horizon of depth 4 (pt + 1 clamped onto pt), beyond one of depth 3",
         both("time.last_step", 1, (4, "dir", W), py=4, cu=4, at=(4, 2, W, 4)) + both("time.beyond_horizon", 1, (4, "pos", (4, 3)), py=3, cu=3),
         py_pred=(30, 10, 6, 4, 3), cu_pred=(500, 4, 3))


def _yard_target_cases():
    W1 = on(M, 4, 6, W)
    case("tg_other", "yard", "small", "targets", put(a1=W1, a7=off(WAITING)), ("tg.other", "tg.own", "tg.cutils_never"),
         "agent 7's target (4, 4) on the walker's branch, the walker's own at its end",
         py_pin("tg.other", 1, (1, "pos", (4, 5))) + both("tg.own", 1, (1, "pos", (4, 5))) + cu_pin("tg.cutils_never", 1, (1, "pos", (4, 5))))
    case("tg_own_not_other", "yard", "small", "targets", put(a0=on(M, 4, 5, E)), ("tg.own_not_other",),
         "(4, 7) is walker 0's target and agent 5's: not another agent's target", py_pin("tg.own_not_other", 0, (0, "pos", (4, 3))))


def _yard_root_cases():
    case("root_states", "yard", "small", "mixed", [off(WAITING), off(READY), off(MALF_OFF, malf=3), on(M, 1, 4, W), on(ST, 4, 2, E), on(MF, 4, 4, E, malf=2), off(DONE), on(M, 4, 5, W)],
         ("root.virtual_done", "root.virtual_off_map", "root.malf"), "an agent in each of the seven states",
         both("root.virtual_done", 6, (6, "state", WAITING)) + both("root.virtual_off_map", 0, (0, "state", DONE)) + both("root.malf", 2, (2, "malf", 0)))
    case("root_dead_end", "yard", "small", "fast", put(a1=on(M, 4, 7, E)), ("root.reoriented",),
         "a root on a dead end, facing the buffer: one transition, and the tree is turned so that it is the forward branch",
         py_pin("root.reoriented", 1, (1, "pos", (4, 6))))


def _yard_crowd_cases():
    crowd = {"a%d" % i: off(WAITING) for i in range(2, 22)}
    case("ll_single_low", "yard", "crowd", "single", put(a0=on(M, 1, 4, W), a1=on(M, 4, 1, E), **crowd), ("ll.single_low",),
         "twenty agents wait on two start cells, there and back along the line; of the 40 and more items on (4, 2) ONE conflicts: agent 1's, at pt = 5",
         both("ll.single_low", 0, (1, "pos", (4, 4)), at=(4, 2, W, 5)))
    case("ll_single_high", "yard", "crowd", "single", put(a0=on(M, 1, 4, W), a23=on(M, 4, 1, E), **crowd), ("ll.single_high",),
         "... the highest handle's", both("ll.single_high", 0, (23, "pos", (4, 4)), at=(4, 2, W, 5)))
    case("ll_hider", "yard", "crowd", "quarter", put(a0=on(M, 2, 3, S), a22=on(M, 4, 5, W), **crowd), ("ll.hider",),
         "walker 0 at speed 1/4 asks (4, 3) for t = 8: agent 22 is there without the condition, ten of the crowd at t = 9 with it",
         both("ll.hider", 0, (22, "pos", (4, 6)), at=(4, 3, S, 2)))


def _crossing_cases():
    """walker 2 heads west along the horizontal line (its trailing switch, the diamond, the start cell of 5 .. 7); walker 1 south across the diamond;
    walker 0 east to the facing switch, whose right branch is the spur"""
    case("x_ready_3", "crossing", "small", "fast", put(a0=on(ST, 4, 1, E), a2=on(M, 4, 7, W), a5=off(WAITING), a6=off(READY), a7=off(MALF_OFF, malf=1)),
         ("occ.ready_3",), "three agents off the map on the occupied start cell of the crossing", both("occ.ready_3", 2, (7, "state", DONE)))
    case("x_diamond_hides", "crossing", "small", "fast", put(a0=on(M, 4, 1, E), a1=on(M, 1, 4, S), a3=on(M, 8, 4, S)), ("cf.elif_hides_post",),
         "walker 1 is on the diamond at pt = 3 with agent 0, which crosses it (no way back along its direction); agent 3, head-on, is there at pt + 1: hidden",
         both("cf.elif_hides_post", 1, (0, "dir", W), at=(4, 4, S, 3)))
    case("x_spur", "crossing", "small", "fast", put(a0=on(M, 4, 1, E), a4=on(MF, 6, 6, N, malf=5)), ("occ.opp_dir", "occ.malf"),
         "a broken-down train on the spur, in a node of depth 2 of walker 0", both("occ.opp_dir", 0, (4, "pos", (4, 4))) + both("occ.malf", 0, (4, "malf", 0)))
    case("x_root_states", "crossing", "small", "mixed", [off(WAITING), off(READY), off(MALF_OFF, malf=3), on(M, 6, 4, N), on(ST, 5, 6, N), on(MF, 4, 4, E, malf=2), off(DONE), on(M, 4, 4, S)],
         ("root.virtual_done", "root.malf"), "an agent in each of the seven states on the crossing, two of them on the diamond",
         both("root.virtual_done", 6, (6, "state", WAITING)) + both("root.malf", 2, (2, "malf", 0)))
    crowd = {"a%d" % i: off(WAITING) for i in range(2, 22)}
    case("xl_diamond", "crossing", "crowd", "fast", put(a0=on(M, 1, 4, S), a1=on(M, 7, 4, N), **crowd), ("ll.single_at_pt",),
         "twenty waiting agents cross the diamond at t = 3 and again at t = 11, none with a way back along its direction; agent 1, head-on, is the one item that conflicts",
         both("ll.single_at_pt", 0, (1, "pos", (6, 4)), at=(4, 4, S, 3)))


_yard_occupant_cases()
_crossing_cases()
_yard_conflict_cases()
_yard_time_cases()
_yard_target_cases()
_yard_root_cases()
_yard_crowd_cases()
BY_NAME = {c["name"]: c for c in CASES}
PART = 24      # cases of one fixture file (a case and its controls stay together): each file stays below the largest step fixture


def parts_of(map_name, set_name):
    """the cases of an agent set, in order, as the lists of names of its fixture files obs_states_<map>_<set>_<k>.npz"""
    parts, cur = [], []
    for c in CASES:
        if (c["map"], c["set"]) != (map_name, set_name):
            continue
        if c["control_of"] is None and len(cur) >= PART:
            parts.append(cur)
            cur = []
        cur.append(c["name"])
    return parts + [cur] if cur else parts


def fixture_files(map_name, set_name):
    return ["obs_states_%s_%s_%d" % (map_name, set_name, k) for k in range(len(parts_of(map_name, set_name)))]


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_set(map_name, set_name):
    """name -> array over the fixture files of an agent set (np.load's default: no pickle); `names`: the cases in order"""
    out, names = {}, []
    for f in fixture_files(map_name, set_name):
        fx = np.load(os.path.join(GOLD, f + ".npz"))
        names += [str(n) for n in fx["names"]]
        out.update({k: fx[k] for k in fx.files if k != "names"})
    out["names"] = names
    return out
assert {row for c in CASES for row in c["rows"]} <= set(TABLE), sorted({row for c in CASES for row in c["rows"]} - set(TABLE))
TRUNCATIONS = truncation_pairs()
