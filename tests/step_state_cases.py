"""Constructed one-agent-one-step situations of RailEnv.step() (rail_env.py:501-634): action preprocessing, the action saver, the speed counter,
the seven-state machine, placement, arrival, the end of the episode.  Data and small constructors only -- numpy and tests/handmaps.py, nothing
of the reference.  oracle/refharness/capture_step_states.py sets every case's state on the REAL RailEnv, calls its step() for the case's actions
and writes tests/golden/step_states_<map>.npz; tests/test_step_states.py (CPU) asserts that every row of TABLE is reached by a case that names
it -- judged on the log the reference left, not on the inputs -- and that the oracle started from the state equals the reference;
tests/test_gpu_step_states.py compares k_step with the fixture after every step.

A case: map (handmaps.STEP_MAPS), variant (VARIANTS[map]: speed, earliest, latest, target, T, malfunction parameters), rows i32[A, 12] in
util.STATE_NAMES order, aux i32[A, 4] (previous state, in_malfunction signal, deadlocked, done), elapsed, done_all, rng (seed, position),
actions u8[steps, A] (255 = absent from the dict), filter (eval_env.parse_actions: bit 1 of fl_step's flags), rows (the TABLE rows it exists
for), doc (one line).

Adding a case: append it in one of the builders below with the table rows it is for, run oracle/refharness/capture_step_states.py where the
reference lies, and run tests/test_step_states.py: a case that misses a row it names fails there.

Speeds: max_count = int(1 / speed) - 1 of 0, 1, 2, 3, and 0.3 (no reciprocal: int(3.33) - 1 = 2).  A speed 1 / n whose int(1 / (1 / n)) is n - 1
starts at n = 93 (max_count 91); FL_MAX_SPEED_COUNT is 63 and no n of 2 .. 64 truncates (TRUNCATING_SPEEDS below, asserted by the CPU test):
none fits."""
import numpy as np

from tests import handmaps

WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)
NOTHING, LEFT, FORWARD, RIGHT, STOP, ABSENT, ILLEGAL = 0, 1, 2, 3, 4, 255, 7
N, E, S, W = 0, 1, 2, 3
SIGNALS = ("in_malfunction", "malfunction_counter_complete", "earliest_departure_reached", "stop_action_given",
           "valid_movement_action_given", "target_reached", "movement_conflict")
TRUNCATING_SPEEDS = [n for n in range(2, 65) if int(1 / (1 / n)) != n]      # (empty)
MALF_ALL = 40.0      # 1 - exp(-40) is 1.0 in double: every draw fires
MALF_SOME = 0.2      # p = 0.18: seeds are searched for the wanted pattern (seed_for)


def _variant(speed, earliest=2, latest=20, T=40, target=None, rate=0.0, mn=0, mx=0):
    full = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * 5      # noqa: E731
    return dict(speed=[float(v) for v in full(speed)], earliest=full(earliest), latest=full(latest), T=T, target=target, malf_rate=rate,
                malf_min=mn, malf_max=mx)


SLOW = [1 / 2, 1 / 3, 1 / 4, 0.3, 1.0]
VARIANTS = {
    "yard": {
        "fast": _variant(1.0),
        "slow": _variant(SLOW),
        # the episode ends at T = 6: latest arrivals before and after it; agent 4's target is the stub nobody reaches
        "end": _variant([1.0, 1 / 2, 0.3, 1 / 3, 0.3], latest=[3, 3, 8, 4, 8], T=6),
        "end_int": _variant([1 / 3, 1.0, 1 / 4, 1 / 2, 1.0], latest=[3, 9, 8, 4, 2], T=6),
        "malf1": _variant([1.0, 1 / 2, 1.0, 1.0, 1.0], rate=MALF_ALL, mn=0, mx=0),      # every agent, one step (the shortest the generator draws)
        "malf2": _variant([1.0, 1 / 2, 1.0, 1.0, 1.0], rate=MALF_ALL, mn=1, mx=1),      # every agent, two steps
        "some1": _variant([1.0, 1 / 2, 1.0, 1.0, 1.0], rate=MALF_SOME, mn=0, mx=0),     # the agents a searched seed picks, one step
        "some12": _variant([1.0, 1 / 2, 1.0, 1.0, 1.0], rate=MALF_SOME, mn=0, mx=1),    # ... one or two steps (a randint draw)
    },
    "crossing": {
        "fast": _variant(1.0, latest=30),
        "slow": _variant(SLOW, latest=30),
        "end": _variant([1.0, 0.3, 1 / 2, 1.0, 1 / 3], latest=[3, 8, 3, 8, 5], T=5),
    },
}


def rng_of(seed, pos=624):
    key = np.random.RandomState(seed).get_state()[1].astype(np.uint32)
    return key, pos


def static_of(map_name, variant, rng=(1, 624)):
    """the static description BatchedRailEnv / OracleEnv take"""
    m = handmaps.STEP_MAPS[map_name]()
    v = VARIANTS[map_name][variant]
    key, pos = rng_of(*rng)
    return dict(grid=m["grid"], init_pos=m["init_pos"], init_dir=m["init_dir"], target=np.array(v["target"] or m["target"], dtype=np.int32),
                speed=np.array(v["speed"], dtype=np.float64), earliest=np.array(v["earliest"], dtype=np.int32),
                latest=np.array(v["latest"], dtype=np.int32), T=v["T"], malf_rate=v["malf_rate"], malf_min=v["malf_min"],
                malf_max=v["malf_max"], mt_key=key, mt_pos=pos)


def max_count(map_name, variant):
    return [int(1 / s) - 1 for s in VARIANTS[map_name][variant]["speed"]]


# (pattern, variant, position) -> seed, as seed_for found them (tests/test_step_states.py replays these)
_SEEDS = {(((0,), (), ()), 'some1', 624): 217, (((0,), (), (2,), ()), 'some12', 600): 876, (((1,), (), ()), 'some1', 624): 75,
          (((1,), (), (3,), ()), 'some12', 605): 3635, (((2,), (), ()), 'some1', 624): 86, (((2,), (), (4,), ()), 'some12', 610): 609,
          (((3,), (), ()), 'some1', 624): 39, (((3,), (), (0,), ()), 'some12', 615): 310, (((4,), (), ()), 'some1', 624): 20,
          (((4,), (), (1,), ()), 'some12', 620): 1880, (((1, 3), (1, 3), (), ()), 'some1', 624): 1335}


def fires_as(seed, pattern, variant, A=5, pos=624):
    """does the stream of `seed` make exactly the agents of pattern[k] fire in step k?  (numpy's own generator: rand() per agent in handle
    order, randint(min, max + 1) after a draw that fires)"""
    v = VARIANTS["yard"][variant]
    p = float(1 - np.exp(-v["malf_rate"]))
    rs = np.random.RandomState(seed)
    st = rs.get_state()
    rs.set_state((st[0], st[1], pos, 0, 0.0))
    for want in pattern:
        for i in range(A):
            fire = rs.rand() < p
            if fire:
                rs.randint(v["malf_min"], v["malf_max"] + 1)
            if fire != (i in want):
                return False
    return True


def seed_for(pattern, variant, pos=624):
    """(seed, position) of the first seed that fires_as the pattern, from _SEEDS; a pattern that is not there yet is searched and the
    entry to add is named in the error"""
    key = (tuple(tuple(sorted(p)) for p in pattern), variant, pos)
    if key not in _SEEDS:      # searched once, by whoever adds the pattern: the seed is data of this module
        seed = next(seed for seed in range(1, 200000) if fires_as(seed, pattern, variant, pos=pos))
        raise KeyError("seed_for: add to _SEEDS  %r: %d," % (key, seed))
    return _SEEDS[key], pos


# ---- constructors
def ag(state, r=-1, c=-1, d=None, malf=0, nmalf=None, sc=0, saved=0, arrival=-1, old=None, prev=-1, done=None):
    """one agent: old = (row, col, dir) of the last step or None; nmalf defaults to `a malfunction is running`; done to `state is DONE`"""
    if state == DONE and arrival < 0:
        arrival = 1
    return dict(state=state, r=r, c=c, d=d, malf=malf, nmalf=int(malf > 0) if nmalf is None else nmalf, sc=sc, saved=saved, arrival=arrival,
                old=old, prev=prev, done=int(state == DONE) if done is None else done)


def _valid(grid, r, c, d, action):
    """is the movement action valid for a train on (r, c) facing d?  (transition_utils.check_valid_action)"""
    bits = handmaps.nibble(grid[r, c], d)
    nd = (d + action - 2) % 4
    if bin(bits).count("1") <= 1:
        if action != FORWARD or bits == 0:      # (one way on: LEFT and RIGHT are never valid, FORWARD takes that way)
            return False
        nd = [k for k in range(4) if (bits >> (3 - k)) & 1][0]
    nr, nc = r + handmaps.DR[nd], c + handmaps.DC[nd]
    return bool((bits >> (3 - nd)) & 1) and 0 <= nr < grid.shape[0] and 0 <= nc < grid.shape[1] and grid[nr, nc] != 0


IDLE = ag(WAITING)      # never given an action: WAITING, then READY_TO_DEPART for good
GONE = ag(DONE)
CASES = []


def case(name, map_name, variant, agents, actions, rows, doc, elapsed=0, done_all=0, rng=(1, 624), filter=False):
    m = handmaps.STEP_MAPS[map_name]()
    agents = list(agents) + [IDLE] * (5 - len(agents))
    st = np.zeros((5, 12), dtype=np.int32)
    aux = np.zeros((5, 4), dtype=np.int32)
    for i, a in enumerate(agents):
        on = a["r"] >= 0
        assert on == (MOVING <= a["state"] <= MALF), (name, i)
        d = int(m["init_dir"][i]) if a["d"] is None else a["d"]
        # a train faces a way its cell allows, and a saved action is one that was valid where it was saved: this cell (the reference
        # applies it unchecked -- a stale one would take the train off the rail)
        r, c = (a["r"], a["c"]) if on else (int(v) for v in m["init_pos"][i])
        assert handmaps.nibble(m["grid"][r, c], d) != 0 and (a["saved"] == 0 or _valid(m["grid"], r, c, d, a["saved"])), (name, i)
        old = a["old"] if a["old"] is not None else ((a["r"], a["c"], d) if on else (-1, -1, -1))
        st[i] = (a["r"], a["c"] if on else -1, d, a["state"], a["malf"], a["nmalf"], a["sc"], a["saved"], a["arrival"], old[0], old[1], old[2])
        aux[i] = (a["prev"], int(a["malf"] > 0), 0, a["done"])
    acts = np.array(actions, dtype=np.uint8).reshape(-1, 5)
    assert 1 <= len(acts) <= 4 and isinstance(rows, tuple) and rows and "\n" not in doc
    assert name not in {c["name"] for c in CASES}, name
    CASES.append(dict(name=name, map=map_name, variant=variant, state=st, aux=aux, elapsed=elapsed, done_all=done_all, rng=rng, actions=acts,
                      filter=filter, rows=rows, doc=doc))


def acts(*per_agent):
    """actions of one step: the listed agents', ABSENT for the rest"""
    return list(per_agent) + [ABSENT] * (5 - len(per_agent))


ACT_NAME = {0: "nothing", 1: "left", 2: "forward", 3: "right", 4: "stop", 255: "absent", 7: "illegal"}
ST_NAME = ("waiting", "ready", "malfoff", "moving", "stopped", "malf", "done")


# ---- the state machine off the map: agents 0 .. 3 of the yard start on cells of their own (agent 4 shares agent 0's and idles)
def _off_map_cases():
    # WAITING
    case("waiting_stay", "yard", "fast", [ag(WAITING), ag(WAITING), ag(WAITING)], acts(FORWARD, STOP, LEFT), ("waiting.stay", "act.waiting_blocks"),
         "before the earliest departure a waiting agent stays, whatever it is told")
    case("waiting_ready", "yard", "fast", [ag(WAITING), ag(WAITING), ag(WAITING), ag(WAITING)], acts(FORWARD, NOTHING, STOP, ILLEGAL),
         ("waiting.ready", "act.waiting_blocks"), "t reaches earliest_departure exactly (t >= earliest): READY_TO_DEPART, nothing saved", elapsed=1)
    case("waiting_ready_late", "yard", "fast", [ag(WAITING), ag(WAITING)], [acts(FORWARD, FORWARD), acts(FORWARD, NOTHING)],
         ("waiting.ready", "ready.moving", "ready.stay"), "past the earliest departure; the step after, FORWARD departs and DO_NOTHING does not", elapsed=7)
    case("waiting_malf", "yard", "fast", [ag(WAITING, malf=3), ag(WAITING, malf=1)], [acts(FORWARD, FORWARD)] * 2,
         ("waiting.malf", "malf.counter_one_on_entry"),
         "a waiting agent breaks down before its departure; the counter of 1 is complete one step later, when the departure is due")
    case("waiting_malf_and_departure", "yard", "fast", [ag(WAITING, malf=2), ag(WAITING, malf=1)], [acts(FORWARD, FORWARD)] * 3,
         ("waiting.malf_and_departure", "malfoff.stay", "malfoff.moving"),
         "both signals at once (the reference's TODO): in malfunction wins over earliest departure reached", elapsed=1)
    # READY_TO_DEPART
    for a in (NOTHING, LEFT, FORWARD, RIGHT, STOP, ABSENT, ILLEGAL):
        moving = a in (LEFT, FORWARD, RIGHT)
        rows = ("ready.moving", "speed.not_on_entry") if moving else ("ready.stay",)
        rows += {LEFT: ("act.lr_invalid_to_forward",), RIGHT: ("act.lr_invalid_to_forward",), ABSENT: ("act.absent", "act.nothing_stays"),
                 ILLEGAL: ("act.illegal",), NOTHING: ("act.nothing_stays",)}.get(a, ())
        case("ready_" + ACT_NAME[a], "yard", "fast", [ag(READY, prev=WAITING), ag(READY, prev=WAITING), ag(READY), ag(READY)], acts(a, a, a, a), rows,
             "ready to depart, told %s: %s" % (ACT_NAME[a], "placed on the start cell, counter untouched" if moving else "stays off the map"), elapsed=3)
    case("ready_saved_nothing", "yard", "fast", [ag(READY, saved=FORWARD), ag(READY, saved=FORWARD)], acts(NOTHING, ABSENT),
         ("act.nothing_to_saved", "ready.moving"), "DO_NOTHING with a saved action becomes that action: the agent departs", elapsed=3)
    case("ready_saved_stop", "yard", "fast", [ag(READY, saved=FORWARD), ag(READY, saved=FORWARD)], [acts(STOP, STOP), acts(NOTHING, NOTHING)],
         ("saver.cleared_by_stop_off_map", "ready.stay"), "STOP off the map clears the saved action: DO_NOTHING departs nobody a step later", elapsed=3)
    case("ready_malf", "yard", "fast", [ag(READY, malf=2), ag(READY, malf=1, saved=FORWARD)], [acts(FORWARD, NOTHING)] * 3,
         ("ready.malf", "malfoff.stay", "malfoff.moving", "saver.saved", "malf.in_malf_before_decrement"),
         "READY with a running counter goes to MALFUNCTION_OFF_MAP although told to move; it departs when the counter is complete", elapsed=3)
    # MALFUNCTION_OFF_MAP, five branches
    for a in (NOTHING, FORWARD, STOP, RIGHT, ABSENT):
        rows = {FORWARD: ("malfoff.moving",), RIGHT: ("malfoff.moving", "act.lr_invalid_to_forward"), STOP: ("malfoff.stopped", "place.stopped_without_motioncheck"),
                NOTHING: ("malfoff.ready",), ABSENT: ("malfoff.ready", "act.absent")}[a]
        case("malfoff_complete_" + ACT_NAME[a], "yard", "fast", [ag(MALF_OFF, nmalf=1, prev=READY), ag(MALF_OFF, nmalf=2, prev=MALF_OFF), ag(MALF_OFF, nmalf=1)],
             [acts(a, a, a), acts(FORWARD, NOTHING, STOP)], rows,
             "counter complete and departure reached, told %s; the next step from where that led" % ACT_NAME[a], elapsed=4)
    case("malfoff_complete_early", "yard", "fast", [ag(MALF_OFF, nmalf=1), ag(MALF_OFF, nmalf=1), ag(MALF_OFF, nmalf=1)], [acts(FORWARD, STOP, NOTHING)] * 2,
         ("malfoff.waiting", "waiting.ready"), "counter complete BEFORE the earliest departure: back to WAITING whatever the action, READY a step later")
    case("malfoff_running", "yard", "fast", [ag(MALF_OFF, malf=1, prev=WAITING), ag(MALF_OFF, malf=2), ag(MALF_OFF, malf=5)], [acts(FORWARD, STOP, FORWARD)] * 2,
         ("malfoff.stay", "malf.counter_one_on_entry", "malf.in_malf_before_decrement"),
         "counters of 1, 2 and 5 on entry: in_malfunction is read before the tick, so a counter of 1 still holds the agent this step", elapsed=4)
    case("malfoff_stop_on_occupied", "yard", "fast", [ag(MOVING, 4, 1, E), IDLE, IDLE, IDLE, ag(MALF_OFF, nmalf=1)], [acts(STOP, ABSENT, ABSENT, ABSENT, STOP),
                                                                                                       acts(FORWARD, ABSENT, ABSENT, ABSENT, FORWARD)],
         ("malfoff.stopped", "place.initial_on_occupied", "place.stopped_without_motioncheck"),
         "agent 4's start cell holds train 0: told STOP at the end of its malfunction it is put there all the same (a stack of two)", elapsed=4)
    case("depart_on_occupied", "yard", "fast", [ag(STOPPED, 4, 1, E), IDLE, IDLE, IDLE, ag(READY)], [acts(STOP, ABSENT, ABSENT, ABSENT, FORWARD)] * 2,
         ("ready.stay", "stopped.stay"), "a stopped train on the start cell: MotionCheck keeps the ready agent off the map", elapsed=4)
    case("depart_two_one_cell", "yard", "fast", [ag(READY), IDLE, IDLE, IDLE, ag(READY)], [acts(FORWARD, ABSENT, ABSENT, ABSENT, FORWARD)] * 2,
         ("ready.moving", "ready.stay"), "agents 0 and 4 leave from one cell: the lower handle wins, the other follows when the cell is free", elapsed=4)
    case("done_stays", "yard", "fast", [GONE, ag(DONE, arrival=3, saved=0), ag(MOVING, 2, 3, N)], [acts(FORWARD, LEFT, FORWARD), acts(STOP, FORWARD, FORWARD)],
         ("done.stay", "saver.none_in_done"), "DONE is terminal: no action is saved, nothing moves, the arrival time stays", elapsed=9)


# ---- on the map
def _on_map_cases():
    # MOVING on plain track, every action (speed 1)
    for a in (NOTHING, LEFT, FORWARD, RIGHT, STOP, ABSENT, ILLEGAL):
        rows = {NOTHING: ("act.nothing_to_forward", "moving.stay"), ABSENT: ("act.absent", "act.nothing_to_forward", "moving.stay"),
                ILLEGAL: ("act.illegal", "act.nothing_to_forward", "moving.stay"), LEFT: ("act.lr_invalid_to_forward", "moving.stay"),
                RIGHT: ("act.lr_invalid_to_forward", "moving.stay"), FORWARD: ("moving.stay", "speed.max_count_0"), STOP: ("moving.stopped_by_stop",)}[a]
        case("moving_" + ACT_NAME[a], "yard", "fast", [ag(MOVING, 4, 1, E), ag(MOVING, 4, 6, W), ag(MOVING, 2, 3, N), ag(MOVING, 1, 5, W)],
             [acts(a, a, a, a), acts(FORWARD, FORWARD, STOP, NOTHING)], rows,
             "four moving trains on plain track told %s, then a second step" % ACT_NAME[a], elapsed=5)
    # STOPPED, every action
    for a in (NOTHING, LEFT, FORWARD, RIGHT, STOP, ABSENT, ILLEGAL):
        moving = a in (LEFT, FORWARD, RIGHT)
        rows = ("stopped.moving",) if moving else ("stopped.stay", "act.nothing_stays") if a != STOP else ("stopped.stay",)
        case("stopped_" + ACT_NAME[a], "yard", "fast", [ag(STOPPED, 4, 1, E), ag(STOPPED, 4, 6, W), ag(STOPPED, 2, 3, N, saved=0), ag(STOPPED, 1, 5, W)],
             [acts(a, a, a, a), acts(NOTHING, NOTHING, NOTHING, NOTHING)], rows,
             "four stopped trains told %s; DO_NOTHING a step later keeps a moving train moving and a stopped one stopped" % ACT_NAME[a], elapsed=5)
    case("stopped_saved_nothing", "yard", "fast", [ag(STOPPED, 4, 1, E, saved=FORWARD), ag(STOPPED, 4, 3, E, saved=LEFT)], acts(NOTHING, ABSENT),
         ("act.nothing_to_saved", "stopped.moving"), "a stopped train with a saved action and DO_NOTHING moves on", elapsed=5)
    case("stopped_malf", "yard", "fast", [ag(STOPPED, 4, 1, E, malf=2), ag(STOPPED, 4, 6, W, malf=1)], [acts(FORWARD, FORWARD)] * 3,
         ("stopped.malf", "malf.stay", "malf.moving", "place.malf_never_moves", "malf.counter_one_on_entry"),
         "a stopped train whose counter runs goes to MALFUNCTION and does not move; it moves the step after the counter is complete", elapsed=5)
    case("moving_malf", "yard", "fast", [ag(MOVING, 4, 1, E, malf=3), ag(MOVING, 4, 6, W, malf=1)], [acts(FORWARD, FORWARD)] * 4,
         ("moving.malf", "malf.stay", "malf.moving", "place.malf_never_moves"), "a moving train breaks down: it stands for as long as the counter says", elapsed=5)
    for a in (NOTHING, STOP, FORWARD, ABSENT):
        rows = ("malf.moving",) if a == FORWARD else ("malf.stopped",)
        case("malf_complete_" + ACT_NAME[a], "yard", "fast", [ag(MALF, 4, 1, E, nmalf=1, prev=MALF), ag(MALF, 4, 6, W, nmalf=3, prev=MOVING)],
             [acts(a, a), acts(NOTHING, FORWARD)], rows, "MALFUNCTION with a complete counter told %s" % ACT_NAME[a], elapsed=5)
    case("malf_complete_saved", "yard", "fast", [ag(MALF, 4, 1, E, nmalf=1, saved=FORWARD), ag(MALF, 4, 6, W, nmalf=1, saved=FORWARD)], acts(NOTHING, STOP),
         ("malf.moving", "malf.stopped", "act.nothing_to_saved"), "the action saved before the breakdown restarts the train; STOP overrides it", elapsed=5)
    case("malf_running", "yard", "fast", [ag(MALF, 4, 1, E, malf=1), ag(MALF, 4, 6, W, malf=2), ag(MALF, 2, 3, N, malf=9, nmalf=4)], [acts(FORWARD, FORWARD, FORWARD)] * 3,
         ("malf.stay", "malf.moving", "malf.in_malf_before_decrement", "place.malf_never_moves"),
         "counters of 1, 2 and 9 on entry of a broken train: the move comes the step after the counter reads 0", elapsed=5)
    # conflicts
    case("moving_conflict_head_on", "yard", "fast", [ag(MOVING, 4, 4, E), ag(MOVING, 4, 5, W)], [acts(FORWARD, FORWARD)] * 2,
         ("moving.stopped_by_conflict", "stopped.stay"), "two trains want to swap cells: both are STOPPED by movement_conflict alone, and stay so", elapsed=5)
    case("moving_conflict_same_cell", "yard", "fast", [ag(MOVING, 4, 2, E), IDLE, ag(MOVING, 3, 3, S)], [acts(FORWARD, ABSENT, FORWARD)] * 2,
         ("moving.stopped_by_conflict", "moving.stay", "stopped.moving"), "two trains want the switch cell: the lower handle gets it, the other stops and follows", elapsed=5)
    case("moving_conflict_chain", "yard", "fast", [ag(STOPPED, 4, 6, E), ag(MOVING, 4, 5, E), ag(MOVING, 4, 4, E)], [acts(STOP, FORWARD, FORWARD)] * 2,
         ("moving.stopped_by_conflict",), "a queue behind a stopped train: blocked transitively", elapsed=5)
    case("stack_moves_apart", "yard", "fast", [ag(MOVING, 4, 1, E), IDLE, IDLE, IDLE, ag(STOPPED, 4, 1, E)], [acts(FORWARD, ABSENT, ABSENT, ABSENT, FORWARD)] * 2,
         ("moving.stay", "stopped.moving"), "two trains on one cell both told FORWARD (what MALFUNCTION_OFF_MAP -> STOPPED leaves behind): one node, one edge, both move", elapsed=5)
    # switches, dead ends, the symmetric switch from its stem
    for a in (LEFT, FORWARD, RIGHT, NOTHING):
        rows = {LEFT: ("act.left_valid",), FORWARD: ("moving.stay",), RIGHT: ("act.lr_invalid_to_forward",), NOTHING: ("act.nothing_to_forward",)}[a]
        case("switch_facing_" + ACT_NAME[a], "yard", "fast", [ag(MOVING, 4, 3, E), ag(STOPPED, 4, 3, W), ag(MOVING, 4, 3, S)], acts(a, a, a), rows,
             "three trains on the simple switch (a stack), eastbound facing it, westbound and southbound trailing it, told %s" % ACT_NAME[a], elapsed=5)
    for a in (LEFT, FORWARD, RIGHT, NOTHING, STOP):
        rows = {LEFT: ("act.left_valid",), FORWARD: ("act.forward_invalid_to_stop", "moving.stopped_by_stop"), RIGHT: ("act.right_valid",),
                NOTHING: ("act.forward_invalid_to_stop", "act.nothing_to_forward"), STOP: ("moving.stopped_by_stop",)}[a]
        case("sym_stem_" + ACT_NAME[a], "yard", "fast", [ag(MOVING, 1, 3, N), IDLE, ag(STOPPED, 1, 3, E), ag(MOVING, 1, 3, W)], acts(a, ABSENT, a, a), rows,
             "on the symmetric switch: from the stem FORWARD has no transition and becomes STOP_MOVING; from a branch there is one way; told %s" % ACT_NAME[a],
             elapsed=5)
    case("sym_stem_stopped_forward", "yard", "slow", [ag(STOPPED, 1, 3, N, sc=1), ag(STOPPED, 1, 3, N, sc=2, saved=LEFT)], [acts(FORWARD, FORWARD)] * 2,
         ("act.forward_invalid_to_stop", "stopped.stay", "saver.not_overwritten"), "stopped on the symmetric switch, from the stem, told FORWARD: stays stopped", elapsed=5)
    for a in (FORWARD, LEFT, NOTHING):
        case("dead_end_" + ACT_NAME[a], "yard", "fast", [ag(MOVING, 4, 0, W), ag(MOVING, 4, 7, E), ag(MOVING, 1, 0, W), ag(STOPPED, 1, 6, E)], [acts(a, a, a, a)] * 2,
             ("act.dead_end_turn",) if a != NOTHING else ("act.dead_end_turn", "act.nothing_to_forward"),
             "on the four dead ends told %s: FORWARD is valid and turns the train round" % ACT_NAME[a], elapsed=5)
    case("crossing_diamond", "crossing", "fast", [ag(MOVING, 4, 3, E), ag(MOVING, 3, 4, S), ag(MOVING, 4, 5, W), ag(MOVING, 5, 4, N)],
         [acts(FORWARD, LEFT, RIGHT, NOTHING)] * 3, ("moving.stopped_by_conflict", "act.lr_invalid_to_forward"),
         "four trains want the diamond crossing: handle 0 gets it", elapsed=5)
    for a in (LEFT, FORWARD, RIGHT):
        case("crossing_switch_" + ACT_NAME[a], "crossing", "fast", [ag(MOVING, 4, 6, E), ag(MOVING, 6, 6, N), ag(MOVING, 4, 4, N), ag(STOPPED, 4, 8, E), ag(READY)],
             [acts(a, a, a, a, a)] * 2, ("act.right_valid",) if a == RIGHT else ("moving.stay",),
             "the crossing's facing switch, its trailing side, the diamond, a dead end and a departure told %s" % ACT_NAME[a], elapsed=31)


# ---- the action saver and the speed counter
def _speed_cases():
    mc = max_count("yard", "slow")      # 1, 2, 3, 2 (speed 0.3), 0
    assert mc == [1, 2, 3, 2, 0]
    spots = [(4, 1, E), (4, 6, W), (2, 3, N), (1, 5, W), (1, 2, W)]
    for sc in range(4):
        agents = [ag(MOVING, r, c, d, sc=min(sc, mc[i])) for i, (r, c, d) in enumerate(spots)]
        rows = ("speed.max_count_0", "speed.max_count_1", "speed.max_count_2", "speed.max_count_3", "speed.non_reciprocal", "speed.wrap", "saver.saved",
                "saver.cleared_on_entry") if sc == 0 else ("speed.wrap", "speed.advance")
        case("slow_moving_sc%d" % sc, "yard", "slow", agents, [acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD)] * 4, rows,
             "speeds 1/2, 1/3, 1/4, 0.3 and 1 from counter min(%d, max_count) through four steps: advance, wrap, move at cell exit only" % sc, elapsed=5)
        agents = [ag(STOPPED, r, c, d, sc=min(sc, mc[i])) for i, (r, c, d) in enumerate(spots)]
        case("slow_stopped_sc%d" % sc, "yard", "slow", agents, [acts(STOP, NOTHING, FORWARD, FORWARD, FORWARD), acts(FORWARD, FORWARD, NOTHING, STOP, FORWARD),
                                                             acts(NOTHING, NOTHING, NOTHING, NOTHING, NOTHING)],
             ("speed.only_moving", "place.inside_cell") if 0 < sc else ("speed.only_moving",),
             "stopped trains of every speed at counter min(%d, max_count): no advance while stopped; mid-cell, movement_inside_cell lets them start" % sc, elapsed=5)
    case("inside_cell_blocked", "yard", "slow", [ag(MOVING, 4, 5, W, sc=0), ag(STOPPED, 4, 6, W, sc=1), ag(STOPPED, 4, 4, E, sc=1)], [acts(STOP, FORWARD, FORWARD)] * 3,
         ("place.inside_cell", "stopped.moving", "moving.stopped_by_conflict"),
         "stopped mid-cell behind and in front of a standing train: MotionCheck blocks them, movement_inside_cell starts them; at cell exit they stop again", elapsed=5)
    case("stop_mid_cell", "yard", "slow", [ag(MOVING, 4, 1, E, sc=0), ag(MOVING, 4, 6, W, sc=1), ag(MOVING, 2, 3, N, sc=2), ag(MOVING, 1, 5, W, sc=1)],
         [acts(STOP, STOP, STOP, STOP), acts(FORWARD, FORWARD, FORWARD, FORWARD), acts(STOP, NOTHING, STOP, NOTHING)],
         ("speed.stopped_mid_cell", "moving.stopped_by_stop", "stopped.moving", "place.inside_cell"), "slow trains stopped in mid-cell keep their counter and go on from it", elapsed=5)
    case("malf_mid_cell", "yard", "slow", [ag(MOVING, 4, 1, E, sc=1, malf=2), ag(MOVING, 4, 6, W, sc=1, malf=1, saved=FORWARD), ag(MOVING, 2, 3, N, sc=3, malf=2, saved=FORWARD)],
         [acts(FORWARD, FORWARD, FORWARD)] * 4, ("speed.malf_mid_cell", "moving.malf", "malf.moving", "place.malf_never_moves"),
         "slow trains broken down in mid-cell and at cell exit keep their counter and saved action", elapsed=5)
    # the saver at the facing switch: speed 1/2 (agent 0), the saved action decides at cell exit
    for saved, a in ((LEFT, FORWARD), (FORWARD, LEFT), (LEFT, STOP), (FORWARD, NOTHING), (LEFT, RIGHT)):
        rows = {STOP: ("moving.stopped_by_stop",), NOTHING: ("act.nothing_to_forward",), FORWARD: ()}.get(a, ("saver.not_overwritten",))
        if a in (LEFT, FORWARD, RIGHT):
            rows += ("saver.saved_applied_at_exit", "saver.cleared_on_entry")
        case("saver_%s_then_%s" % (ACT_NAME[saved], ACT_NAME[a]), "yard", "slow", [ag(MOVING, 4, 3, E, sc=1, saved=saved), ag(MOVING, 4, 6, W, sc=1, saved=FORWARD)],
             [acts(a, a), acts(FORWARD, FORWARD)], rows,
             "at the exit of the facing switch with %s saved, told %s: the saved action is applied, and cleared on entering the next cell" % (ACT_NAME[saved], ACT_NAME[a]), elapsed=5)
    case("saver_two_steps", "yard", "slow", [ag(MOVING, 4, 3, E, sc=0), ag(MOVING, 4, 1, E, sc=0)], [acts(LEFT, FORWARD), acts(FORWARD, LEFT), acts(NOTHING, NOTHING)],
         ("saver.saved", "saver.not_overwritten", "saver.saved_applied_at_exit"),
         "entering the facing switch at speed 1/2, plain track at 1/3: the first action is saved, the second ignored, the first applied", elapsed=5)
    case("filter_required", "yard", "slow", [ag(MOVING, 4, 1, E, sc=1), ag(STOPPED, 4, 6, W, sc=0), ag(READY), ag(MOVING, 1, 5, W, sc=0), ag(MALF_OFF, nmalf=1)],
         [acts(STOP, FORWARD, FORWARD, STOP, FORWARD)] * 2, ("act.filter_required",),
         "eval_env.parse_actions: the mid-cell train's STOP and the off-map agent's FORWARD never reach the env", elapsed=5, filter=True)
    case("filter_required_waiting", "yard", "slow", [ag(MOVING, 4, 1, E, sc=1, saved=FORWARD), ag(MALF, 4, 6, W, sc=2, malf=1), ag(WAITING), ag(STOPPED, 1, 5, W, sc=1), GONE],
         [acts(STOP, STOP, FORWARD, FORWARD, FORWARD)] * 3, ("act.filter_required",),
         "eval_env.parse_actions over three steps: who is required changes with the counters", elapsed=0, filter=True)
    case("crossing_slow", "crossing", "slow", [ag(MOVING, 4, 2, E, sc=1), ag(MOVING, 2, 4, S, sc=2), ag(MOVING, 4, 7, W, sc=3), ag(MOVING, 6, 4, N, sc=2), ag(MOVING, 5, 6, N, sc=0)],
         [acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD)] * 4, ("speed.wrap", "speed.non_reciprocal"), "five speeds on the crossing's rail through four steps", elapsed=5)


# ---- arrival and the end of the episode
def _end_cases():
    case("arrive_from_moving", "yard", "fast", [ag(MOVING, 4, 5, E), ag(MOVING, 4, 1, W), ag(MOVING, 1, 5, E), ag(MOVING, 1, 1, W)], [acts(FORWARD, FORWARD, NOTHING, ABSENT)] * 2,
         ("reached.from_moving", "done.stay"), "four moving trains one cell before their targets: update_if_reached after the move, position None, arrival = t", elapsed=5)
    case("arrive_from_stopped", "yard", "fast", [ag(STOPPED, 4, 5, E), ag(STOPPED, 4, 1, W, saved=FORWARD)], acts(FORWARD, NOTHING),
         ("reached.from_stopped",), "stopped one cell before the target and told to move: MOVING and DONE in one step", elapsed=5)
    case("arrive_from_malf", "yard", "fast", [ag(MALF, 4, 5, E, nmalf=1), ag(MALF, 4, 1, W, nmalf=1, saved=FORWARD)], acts(FORWARD, NOTHING),
         ("reached.from_malf",), "a complete counter one cell before the target: MALFUNCTION -> MOVING -> DONE in one step", elapsed=5)
    case("arrive_slow", "yard", "slow", [ag(MOVING, 4, 5, E, sc=0), ag(MOVING, 4, 1, W, sc=2), ag(MOVING, 1, 5, E, sc=3), ag(MOVING, 1, 1, W, sc=1)],
         [acts(FORWARD, FORWARD, FORWARD, FORWARD)] * 3, ("reached.from_moving",), "slow trains before their targets: they arrive when the counter is at cell exit", elapsed=5)
    case("on_target_moving", "yard", "fast", [ag(MOVING, 4, 6, E), ag(MOVING, 4, 0, W), ag(MOVING, 1, 6, E), ag(MOVING, 1, 0, W)], acts(FORWARD, FORWARD, NOTHING, LEFT),
         ("moving.done_before_move", "place.done_guard"),
         "MOVING trains that already STAND on their targets (dead ends, FORWARD would turn them round): DONE before the move, direction kept", elapsed=5)
    case("on_target_other_states", "yard", "fast", [ag(STOPPED, 4, 6, E), ag(MALF, 4, 0, W, malf=1), ag(MOVING, 1, 6, E, malf=1), ag(STOPPED, 1, 0, W)],
         [acts(FORWARD, FORWARD, FORWARD, STOP)] * 2, ("stopped.moving", "moving.malf"),
         "standing on the target STOPPED or broken down: only the MOVING handler looks at target_reached", elapsed=5)
    case("on_target_slow", "yard", "slow", [ag(MOVING, 4, 6, E, sc=0), ag(MOVING, 4, 0, W, sc=1)], acts(FORWARD, FORWARD), ("moving.done_before_move",),
         "a slow train on its target in mid-cell is DONE at once", elapsed=5)
    # all done before T
    others = [GONE, ag(DONE, arrival=4), ag(DONE, arrival=30)]
    case("last_arrives", "yard", "fast", [ag(MOVING, 4, 5, E), ag(DONE, arrival=25), GONE, ag(DONE, arrival=4), ag(DONE, arrival=20)], [acts(FORWARD), acts(FORWARD)],
         ("end.all_done_before_T", "reward.done_early", "reward.done_late", "end.dones_all_set", "end.next_step_raises"),
         "the last agent arrives before T: terminal rewards of the early (0) and the late (latest - arrival), then a step on the finished env", elapsed=9)
    case("last_arrives_late", "yard", "fast", [ag(MOVING, 4, 5, E)] + others + [ag(DONE, arrival=21)], acts(NOTHING),
         ("end.all_done_before_T", "reward.done_late"), "the last agent arrives after its latest arrival, before T", elapsed=27)
    case("last_on_target", "yard", "fast", [ag(MOVING, 4, 6, E)] + others + [GONE], acts(STOP), ("end.all_done_before_T", "moving.done_before_move"),
         "the last agent is DONE because it stands on its target", elapsed=9)
    case("last_is_stopped", "yard", "fast", [ag(MOVING, 4, 5, E)] + others + [GONE], [acts(STOP), acts(FORWARD)], ("reached.from_stopped", "end.all_done_before_T"),
         "the last agent stops short, then arrives", elapsed=9)
    case("already_over", "yard", "fast", [ag(STOPPED, 4, 5, E, done=1), ag(READY, done=1), ag(DONE, arrival=3), ag(WAITING, done=1), ag(MALF_OFF, malf=4, done=1)],
         [acts(FORWARD, FORWARD), acts(STOP)], ("end.next_step_raises",),
         "an env whose episode is over (done_all set): step() counts the step and raises, twice; nothing else changes", elapsed=40, done_all=1)
    # T reached: the four branches of the terminal reward
    for v in ("end", "end_int"):
        case("T_%s_mixed" % v, "yard", v, [ag(MOVING, 4, 3, E), ag(WAITING), ag(READY), ag(DONE, arrival=2), ag(MALF_OFF, malf=3)], [acts(FORWARD, FORWARD, NOTHING), acts(FORWARD)],
             ("end.by_T", "reward.on_map", "reward.off_map", "reward.done_early", "reward.unreachable_off_map", "end.dones_all_set", "end.next_step_raises"),
             "T reached with a train on the map, agents that never departed, one that arrived and one whose target nobody reaches", elapsed=5)
        case("T_%s_on_map" % v, "yard", v, [ag(MOVING, 4, 4, E), ag(STOPPED, 4, 2, W, sc=0), ag(MALF, 2, 3, N, malf=3), ag(MOVING, 1, 2, W), ag(STOPPED, 4, 1, E)],
             acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD), ("end.by_T", "reward.on_map", "reward.unreachable_on_map"),
             "T reached with everybody on the map, moving, stopped and broken down, one of them bound for the stub", elapsed=5)
        case("T_%s_off_map" % v, "yard", v, [ag(WAITING), ag(READY), ag(MALF_OFF, malf=2), ag(DONE, arrival=5), ag(READY)], acts(NOTHING, STOP, FORWARD),
             ("end.by_T", "reward.off_map", "reward.done_late"), "T reached with nobody on the map", elapsed=5)
        case("T_%s_arrives_at_T" % v, "yard", v, [ag(MOVING, 4, 5, E, sc=max_count("yard", v)[0]), ag(MOVING, 4, 1, W, sc=max_count("yard", v)[1]), GONE, GONE, GONE], acts(FORWARD, FORWARD),
             ("end.by_T", "reward.done_late", "reached.from_moving"), "both reasons at once: the last two agents arrive in step T", elapsed=5)
        case("T_%s_not_yet" % v, "yard", v, [ag(MOVING, 4, 3, E), ag(WAITING), ag(READY)], [acts(FORWARD, FORWARD, FORWARD)] * 3, ("end.by_T", "reward.on_map"),
             "two steps before T, T - 1, T: no reward and no done flag before the ending step", elapsed=3)
    case("T_ceil_off_map", "yard", "end", [IDLE, IDLE, ag(READY), IDLE, IDLE], acts(), ("reward.ceil_fractional_off_map",),
         "agent 2 (speed 0.3) never departed, shortest path of 6 waypoints: ceil(6 / 0.3) = 20, not 6 * round(1 / 0.3) = 18", elapsed=5)
    case("T_ceil_on_map", "yard", "end", [IDLE, IDLE, ag(MOVING, 1, 4, E), IDLE, ag(STOPPED, 1, 4, E)], acts(), ("reward.ceil_fractional_on_map",),
         "agent 2 (speed 0.3) three waypoints from its target: ceil(3 / 0.3) = 10 in double, not 3 * 3 = 9", elapsed=5)
    case("crossing_T", "crossing", "end", [ag(MOVING, 4, 5, E), ag(MOVING, 2, 4, S, sc=1), ag(READY), ag(DONE, arrival=4), ag(STOPPED, 5, 6, S)], [acts(FORWARD, FORWARD, NOTHING), acts(FORWARD)],
         ("end.by_T", "reward.on_map", "reward.off_map", "reward.done_early", "end.next_step_raises"), "the crossing at T = 5: every branch of the terminal reward on another rail", elapsed=4)


# ---- fresh malfunction draws
def _malf_cases():
    mixed = [ag(WAITING), ag(MOVING, 4, 6, W, sc=1), ag(READY), ag(STOPPED, 1, 5, W), ag(MALF_OFF, malf=3)]
    for v in ("malf1", "malf2"):
        case("draw_all_%s" % v, "yard", v, mixed, [acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD)] * 4,
             ("malf.count_incremented", "malf.draw_ignored_while_positive", "waiting.malf", "ready.malf", "moving.malf", "stopped.malf")
             + (("malf.fresh_completes",) if v == "malf2" else ()),
             "every draw fires (%s steps): every state breaks down, a running counter ignores its draw, a counter drawn in step k is complete in step k + %s"
             % (("one", "1") if v == "malf1" else ("two", "2")), elapsed=5, rng=(11, 624))
        case("draw_all_%s_at_departure" % v, "yard", v, [ag(WAITING), ag(WAITING), ag(READY), ag(MALF_OFF, malf=1), ag(MALF, 4, 1, E, malf=1)],
             [acts(FORWARD, STOP, FORWARD, FORWARD, FORWARD)] * 3, ("malf.breaks_at_earliest", "waiting.malf_and_departure", "malf.in_malf_before_decrement"),
             "a breakdown drawn in the very step of earliest_departure; counters of 1 next to fresh draws", elapsed=1, rng=(12, 620))
        case("draw_all_%s_done" % v, "yard", v, [GONE, ag(MOVING, 4, 1, W, sc=1), ag(DONE, arrival=3, malf=0, nmalf=2), GONE, GONE], [acts(FORWARD, FORWARD)] * 3,
             ("malf.count_incremented", "done.stay"), "DONE agents still draw, count and tick; the last train arrives between breakdowns", elapsed=5, rng=(13, 1))
    for k in range(5):
        rows = (("malf.count_incremented", "malf.fresh_completes") if k < 4 else ()) + (("waiting.malf",), ("moving.malf",), ("ready.malf",), ("stopped.malf",),
                                                                                          ("malf.draw_ignored_while_positive",))[k]
        case("draw_one_agent%d" % k, "yard", "some1", mixed, [acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD)] * 3, rows,
             "exactly agent %d fires in the first step and nobody after: a one-step breakdown among neighbours that run on" % k, elapsed=5,
             rng=seed_for([{k}, set(), set()], "some1"))
        case("draw_one12_agent%d" % k, "yard", "some12", mixed, [acts(FORWARD, NOTHING, FORWARD, STOP, FORWARD)] * 4, ("malf.count_incremented",),
             "agent %d fires in the first step, agent %d in the third: durations of one or two steps from randint" % (k, (k + 2) % 5), elapsed=5,
             rng=seed_for([{k}, set(), {(k + 2) % 5}, set()], "some12", pos=600 + 5 * k))
    case("draw_every_step_pair", "yard", "some1", mixed, [acts(FORWARD, FORWARD, FORWARD, FORWARD, FORWARD)] * 4, ("malf.count_incremented", "malf.fresh_completes"),
         "agents 1 and 3 fire in step one, again in step two (counter just complete: a new breakdown at once), nobody after", elapsed=5,
         rng=seed_for([{1, 3}, {1, 3}, set(), set()], "some1"))
    case("draw_malfoff_stop", "yard", "some1", [IDLE, IDLE, ag(READY), IDLE, IDLE], [acts(ABSENT, ABSENT, FORWARD), acts(ABSENT, ABSENT, STOP), acts(ABSENT, ABSENT, FORWARD)],
         ("ready.malf", "malfoff.stopped", "malf.fresh_completes", "place.stopped_without_motioncheck"),
         "READY, breaks down for one step, told STOP when the counter is complete: MALFUNCTION_OFF_MAP -> STOPPED on the start cell", elapsed=5,
         rng=seed_for([{2}, set(), set()], "some1"))


# ---- the same machine on the crossing's rail (the second map of the mixed batch): start cells (4, 1) E, (1, 4) S, (4, 7) W, (7, 4) N, (6, 6) N
def _crossing_cases():
    spots = [(4, 2, E), (2, 4, S), (4, 7, W), (6, 4, N), (6, 6, N)]
    for a in (NOTHING, LEFT, FORWARD, RIGHT, STOP, ABSENT, ILLEGAL):
        moving = a in (LEFT, FORWARD, RIGHT)
        case("crossing_ready_" + ACT_NAME[a], "crossing", "fast", [ag(READY), ag(READY, saved=FORWARD), ag(READY), ag(WAITING), ag(MALF_OFF, nmalf=1)],
             [acts(a, a, a, a, a)] * 2, ("ready.moving",) if moving else ("ready.stay",),
             "the crossing's agents off the map, ready, waiting and at the end of a malfunction, told %s twice" % ACT_NAME[a], elapsed=31)
        case("crossing_moving_" + ACT_NAME[a], "crossing", "slow", [ag(MOVING, r, c, d, sc=i % 2) for i, (r, c, d) in enumerate(spots)],
             [acts(a, a, a, a, a)] * 2, ("moving.stopped_by_stop",) if a == STOP else ("moving.stay",),
             "five slow trains on the crossing's rail, counters 0 and 1, told %s twice" % ACT_NAME[a], elapsed=31)
        case("crossing_stopped_" + ACT_NAME[a], "crossing", "slow", [ag(STOPPED, r, c, d, sc=(i + 1) % 2 if i < 4 else 0, saved=(FORWARD if i == 3 else 0)) for i, (r, c, d) in enumerate(spots)],
             [acts(a, a, a, a, a)] * 2, ("stopped.moving",) if moving else ("stopped.stay",),
             "five stopped trains on the crossing's rail, the slow ones at counters 1 and 0, one with a saved action, told %s twice" % ACT_NAME[a], elapsed=31)
    for a in (NOTHING, FORWARD, STOP, LEFT):
        case("crossing_malf_" + ACT_NAME[a], "crossing", "slow", [ag(MALF, 4, 2, E, malf=1, sc=1), ag(MALF, 2, 4, S, nmalf=2, sc=2), ag(MALF_OFF, malf=1), ag(MALF_OFF, nmalf=1),
                                                                    ag(MALF, 6, 6, N, malf=2)],
             [acts(a, a, a, a, a)] * 3, ("malf.moving",) if a in (FORWARD, LEFT) else ("malf.stopped",),
             "counters of 0, 1 and 2 on and off the crossing's rail told %s for three steps" % ACT_NAME[a], elapsed=31)


_off_map_cases()
_on_map_cases()
_crossing_cases()
_speed_cases()
_end_cases()
_malf_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- the table: name -> predicate over ONE agent in ONE step of the reference's log
class Rec:
    """what the reference recorded for agent i in step k of a case: s0 / s1 state before / after, sig (SIGNALS order) and pa, mv as handed to
    generate_state_transition_signals, raw (the action given, 255 absent), dropped (by parse_actions), drawn (num_broken_steps of its
    draw), b / a (the agent's row before / after), reward, done; of the step: t0 / t (elapsed before / after), T, ended, raised, done_all, states1 (all agents' states
    after); static: mc, speed, earliest, latest, target, init; prev (the Rec of step k - 1 or None); others (the Recs of the other agents)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sig(r, name):
    return bool(r.sig[SIGNALS.index(name)])


def _moving_action(a):
    return a in (LEFT, FORWARD, RIGHT)


def _pos(row):
    return (int(row[0]), int(row[1]))


def _eff_raw(r):
    return ABSENT if r.dropped else r.raw


TABLE = {
    # state machine: every branch of every handler (22) ...
    "waiting.malf": lambda r: r.s0 == WAITING and _sig(r, "in_malfunction") and r.s1 == MALF_OFF,
    "waiting.ready": lambda r: r.s0 == WAITING and not _sig(r, "in_malfunction") and _sig(r, "earliest_departure_reached") and r.s1 == READY,
    "waiting.stay": lambda r: r.s0 == WAITING and not _sig(r, "in_malfunction") and not _sig(r, "earliest_departure_reached") and r.s1 == WAITING,
    "ready.malf": lambda r: r.s0 == READY and _sig(r, "in_malfunction") and r.s1 == MALF_OFF,
    "ready.moving": lambda r: r.s0 == READY and not _sig(r, "in_malfunction") and _sig(r, "valid_movement_action_given") and r.s1 == MOVING,
    "ready.stay": lambda r: r.s0 == READY and not _sig(r, "in_malfunction") and not _sig(r, "valid_movement_action_given") and r.s1 == READY,
    "malfoff.moving": lambda r: (r.s0 == MALF_OFF and _sig(r, "malfunction_counter_complete") and _sig(r, "earliest_departure_reached")
                                 and _sig(r, "valid_movement_action_given") and r.s1 == MOVING),
    "malfoff.stopped": lambda r: (r.s0 == MALF_OFF and _sig(r, "malfunction_counter_complete") and _sig(r, "earliest_departure_reached")
                                  and not _sig(r, "valid_movement_action_given") and _sig(r, "stop_action_given") and r.s1 == STOPPED),
    "malfoff.ready": lambda r: (r.s0 == MALF_OFF and _sig(r, "malfunction_counter_complete") and _sig(r, "earliest_departure_reached")
                                and not _sig(r, "valid_movement_action_given") and not _sig(r, "stop_action_given") and r.s1 == READY),
    "malfoff.waiting": lambda r: (r.s0 == MALF_OFF and _sig(r, "malfunction_counter_complete") and not _sig(r, "earliest_departure_reached")
                                  and r.s1 == WAITING),
    "malfoff.stay": lambda r: r.s0 == MALF_OFF and not _sig(r, "malfunction_counter_complete") and r.s1 == MALF_OFF,
    "moving.malf": lambda r: r.s0 == MOVING and _sig(r, "in_malfunction") and r.s1 == MALF,
    "moving.done_before_move": lambda r: (r.s0 == MOVING and not _sig(r, "in_malfunction") and _sig(r, "target_reached") and r.s1 == DONE
                                          and _pos(r.b) == tuple(r.target)),
    "moving.stopped_by_stop": lambda r: (r.s0 == MOVING and not _sig(r, "in_malfunction") and not _sig(r, "target_reached")
                                         and _sig(r, "stop_action_given") and r.s1 == STOPPED),
    "moving.stopped_by_conflict": lambda r: (r.s0 == MOVING and not _sig(r, "in_malfunction") and not _sig(r, "target_reached")
                                             and not _sig(r, "stop_action_given") and _sig(r, "movement_conflict") and r.s1 == STOPPED),
    "moving.stay": lambda r: (r.s0 == MOVING and not _sig(r, "in_malfunction") and not _sig(r, "target_reached") and not _sig(r, "stop_action_given")
                              and not _sig(r, "movement_conflict") and r.s1 == MOVING),
    "stopped.malf": lambda r: r.s0 == STOPPED and _sig(r, "in_malfunction") and r.s1 == MALF,
    "stopped.moving": lambda r: r.s0 == STOPPED and not _sig(r, "in_malfunction") and _sig(r, "valid_movement_action_given") and r.s1 == MOVING,
    "stopped.stay": lambda r: r.s0 == STOPPED and not _sig(r, "in_malfunction") and not _sig(r, "valid_movement_action_given") and r.s1 == STOPPED,
    "malf.moving": lambda r: r.s0 == MALF and _sig(r, "malfunction_counter_complete") and _sig(r, "valid_movement_action_given") and r.s1 == MOVING,
    "malf.stopped": lambda r: r.s0 == MALF and _sig(r, "malfunction_counter_complete") and not _sig(r, "valid_movement_action_given") and r.s1 == STOPPED,
    "malf.stay": lambda r: r.s0 == MALF and not _sig(r, "malfunction_counter_complete") and r.s1 == MALF,
    "done.stay": lambda r: r.s0 == DONE and r.s1 == DONE and tuple(r.a[[0, 1, 8]]) == tuple(r.b[[0, 1, 8]]),
    # ... update_if_reached after the handler, and both signals at once
    "reached.from_moving": lambda r: r.s0 == MOVING and r.s1 == DONE and not _sig(r, "target_reached") and r.a[8] == r.t and r.a[0] < 0,
    "reached.from_stopped": lambda r: r.s0 == STOPPED and r.s1 == DONE and not _sig(r, "target_reached") and r.a[8] == r.t,
    "reached.from_malf": lambda r: r.s0 == MALF and r.s1 == DONE and not _sig(r, "target_reached") and r.a[8] == r.t,
    "waiting.malf_and_departure": lambda r: (r.s0 == WAITING and _sig(r, "in_malfunction") and _sig(r, "earliest_departure_reached")
                                             and r.s1 == MALF_OFF),
    # placement
    "place.initial_on_occupied": lambda r: (r.s0 <= MALF_OFF and MOVING <= r.s1 <= MALF and _pos(r.a) == tuple(r.init)
                                            and any(_pos(o.a) == tuple(r.init) for o in r.others)),
    "place.stopped_without_motioncheck": lambda r: r.s0 == MALF_OFF and r.s1 == STOPPED and not r.mv and _pos(r.a) == tuple(r.init),
    "place.inside_cell": lambda r: r.s0 == STOPPED and r.b[6] != r.mc and r.mv and _pos(r.a) == _pos(r.b),
    "place.malf_never_moves": lambda r: (_sig(r, "in_malfunction") and r.b[0] >= 0 and _moving_action(r.pa) and not r.mv
                                         and tuple(r.a[0:3]) == tuple(r.b[0:3])),
    # (`movement_allowed and agent.state != DONE`, rail_env.py:596: with remove_agents_at_target the move below it is taken in on-map states
    # only, so the guard decides nothing -- dropping it from k_step changes no output; the row pins what is observable, the direction kept)
    "place.done_guard": lambda r: (r.s0 == MOVING and r.s1 == DONE and _sig(r, "target_reached") and r.mv and r.b[6] == r.mc and _moving_action(r.pa)
                                   and r.a[2] == r.b[2]),
    # actions
    "act.nothing_to_forward": lambda r: _eff_raw(r) == NOTHING and r.s0 == MOVING and r.b[7] != LEFT and r.pa in (FORWARD, STOP) and r.b[7] in (0, FORWARD),
    "act.nothing_to_saved": lambda r: _eff_raw(r) in (NOTHING, ABSENT) and r.s0 not in (MOVING, WAITING) and r.b[7] != 0 and r.pa == r.b[7],
    "act.nothing_stays": lambda r: _eff_raw(r) in (NOTHING, ABSENT) and r.s0 not in (MOVING, WAITING) and r.b[7] == 0 and r.pa == NOTHING,
    "act.waiting_blocks": lambda r: r.s0 == WAITING and 1 <= r.raw <= 4 and r.pa == NOTHING and r.a[7] == 0,
    "act.lr_invalid_to_forward": lambda r: r.raw in (LEFT, RIGHT) and not r.dropped and r.s0 != WAITING and r.b[7] == 0 and r.pa == FORWARD,
    "act.left_valid": lambda r: r.raw == LEFT and r.s0 != WAITING and r.pa == LEFT and _sig(r, "valid_movement_action_given"),
    "act.right_valid": lambda r: r.raw == RIGHT and r.s0 != WAITING and r.pa == RIGHT and _sig(r, "valid_movement_action_given"),
    "act.forward_invalid_to_stop": lambda r: (r.raw == FORWARD or (r.raw == NOTHING and r.s0 == MOVING)) and r.b[7] == 0 and r.pa == STOP,
    "act.dead_end_turn": lambda r: (r.pa == FORWARD and r.b[0] >= 0 and r.a[0] >= 0 and _pos(r.a) != _pos(r.b) and r.a[2] == (r.b[2] + 2) % 4),
    "act.absent": lambda r: r.raw == ABSENT and r.s0 != WAITING and r.pa == (FORWARD if r.s0 == MOVING else r.b[7]),
    "act.illegal": lambda r: 4 < r.raw < ABSENT and r.s0 != WAITING and r.pa == (FORWARD if r.s0 == MOVING else r.b[7]),
    "act.filter_required": lambda r: r.dropped and 1 <= r.raw <= 4 and r.s0 != WAITING and r.pa != r.raw,
    # action saver
    "saver.saved": lambda r: r.b[7] == 0 and _moving_action(r.pa) and r.a[7] == r.pa and r.s0 != DONE,
    "saver.not_overwritten": lambda r: r.b[7] != 0 and 1 <= _eff_raw(r) <= 3 and _eff_raw(r) != r.b[7] and r.a[7] == r.b[7],
    "saver.none_in_done": lambda r: r.s0 == DONE and _moving_action(r.raw) and r.a[7] == 0,
    "saver.cleared_by_stop_off_map": lambda r: r.b[0] < 0 and r.b[7] != 0 and r.pa == STOP and r.a[7] == 0 and r.a[0] < 0,
    "saver.cleared_on_entry": lambda r: (r.b[7] != 0 or _moving_action(r.pa)) and r.a[0] >= 0 and r.a[6] == 0 and r.a[7] == 0,
    "saver.saved_applied_at_exit": lambda r: (r.b[7] != 0 and _moving_action(r.raw) and r.raw != r.b[7] and r.b[6] == r.mc and r.pa == r.b[7]
                                              and _pos(r.a) != _pos(r.b)),
    # speed counter
    "speed.max_count_0": lambda r: r.mc == 0 and r.s0 == MOVING and r.s1 == MOVING and _pos(r.a) != _pos(r.b) and r.a[6] == 0,
    "speed.max_count_1": lambda r: r.mc == 1 and r.s1 == MOVING and r.b[6] == 1 and r.a[6] == 0 and _pos(r.a) != _pos(r.b),
    "speed.max_count_2": lambda r: r.mc == 2 and r.speed != 0.3 and r.s1 == MOVING and r.b[6] == 2 and r.a[6] == 0 and _pos(r.a) != _pos(r.b),
    "speed.max_count_3": lambda r: r.mc == 3 and r.s1 == MOVING and r.b[6] == 3 and r.a[6] == 0 and _pos(r.a) != _pos(r.b),
    "speed.non_reciprocal": lambda r: r.speed == 0.3 and r.mc == 2 and r.s1 == MOVING and r.b[6] == 2 and r.a[6] == 0 and _pos(r.a) != _pos(r.b),
    "speed.advance": lambda r: r.s1 == MOVING and r.b[9] >= 0 and r.b[0] >= 0 and r.b[6] < r.mc and r.a[6] == r.b[6] + 1 and _pos(r.a) == _pos(r.b),
    "speed.not_on_entry": lambda r: r.s0 <= MALF_OFF and r.s1 == MOVING and r.a[9] < 0 and r.a[6] == r.b[6],
    "speed.only_moving": lambda r: r.s1 == STOPPED and r.b[0] >= 0 and r.a[6] == r.b[6],
    "speed.wrap": lambda r: r.mc > 0 and r.b[6] == r.mc and r.a[6] == 0 and r.s1 == MOVING,
    "speed.malf_mid_cell": lambda r: _sig(r, "in_malfunction") and 0 < r.b[6] and r.b[0] >= 0 and r.a[6] == r.b[6] and r.s1 == MALF,
    "speed.stopped_mid_cell": lambda r: r.s0 == MOVING and r.s1 == STOPPED and 0 < r.b[6] < r.mc and r.a[6] == r.b[6],
    # malfunction
    "malf.in_malf_before_decrement": lambda r: r.b[4] == 1 and _sig(r, "in_malfunction") and r.a[4] == 0,
    "malf.counter_one_on_entry": lambda r: r.b[4] == 1 and r.k == 0 and _sig(r, "in_malfunction") and not _sig(r, "malfunction_counter_complete") and r.a[4] == 0,
    "malf.draw_ignored_while_positive": lambda r: r.b[4] > 0 and r.drawn > 0 and r.a[4] == r.b[4] - 1 and r.a[5] == r.b[5],
    "malf.count_incremented": lambda r: r.b[4] == 0 and r.drawn > 0 and r.a[5] == r.b[5] + 1 and r.a[4] == r.drawn - 1,
    "malf.fresh_completes": lambda r: (r.prev is not None and r.prev.b[4] == 0 and r.prev.drawn in (1, 2) and r.b[4] == r.prev.drawn - 1
                                       and (_sig(r, "malfunction_counter_complete") if r.prev.drawn == 1 else r.a[4] == 0)),
    "malf.breaks_at_earliest": lambda r: r.s0 == WAITING and r.b[4] == 0 and r.drawn > 0 and r.t == r.earliest and r.s1 == MALF_OFF,
    # the end of the episode
    "end.by_T": lambda r: r.ended and r.t >= r.T and r.done == 1,
    "end.all_done_before_T": lambda r: r.ended and r.t < r.T and all(s == DONE for s in r.states1) and r.a[8] == r.t,
    "end.dones_all_set": lambda r: r.ended and r.done == 1 and all(o.done == 1 for o in r.others) and r.done_all,
    "end.next_step_raises": lambda r: r.raised and r.t == r.t0 + 1 and tuple(r.a) == tuple(r.b) and r.reward == 0 and r.done_all,
    "reward.done_early": lambda r: r.ended and r.s1 == DONE and r.a[8] <= r.latest and r.reward == 0,
    "reward.done_late": lambda r: r.ended and r.s1 == DONE and r.a[8] > r.latest and r.reward == r.latest - r.a[8],
    "reward.off_map": lambda r: r.ended and r.s1 <= MALF_OFF and r.reward < 0,
    "reward.on_map": lambda r: r.ended and MOVING <= r.s1 <= MALF and r.reward != r.latest - r.t,
    "reward.unreachable_off_map": lambda r: r.ended and r.s1 <= MALF_OFF and r.reward == 0,
    "reward.unreachable_on_map": lambda r: r.ended and MOVING <= r.s1 <= MALF and r.reward == r.latest - r.t,
    "reward.ceil_fractional_off_map": lambda r: r.ended and r.s1 <= MALF_OFF and r.speed == 0.3 and r.reward == -20,
    "reward.ceil_fractional_on_map": lambda r: r.ended and MOVING <= r.s1 <= MALF and r.speed == 0.3 and r.reward == (r.latest - r.t) - 10,
}
assert {row for c in CASES for row in c["rows"]} <= set(TABLE), sorted({row for c in CASES for row in c["rows"]} - set(TABLE))


def recs(case, fx_case):
    """the Recs of a case: [step][agent]; fx_case: the case's arrays of the fixture (see capture_step_states.py)"""
    v = VARIANTS[case["map"]][case["variant"]]
    m = handmaps.STEP_MAPS[case["map"]]()
    target = np.array(v["target"] or m["target"])
    mc = max_count(case["map"], case["variant"])
    out = []
    for k in range(len(case["actions"])):
        before = case["state"] if k == 0 else fx_case["state"][k - 1]
        step = []
        for i in range(5):
            lg = fx_case["log"][k][i]
            step.append(Rec(k=k, i=i, s0=int(lg[0]), s1=int(lg[1]), pa=int(lg[2]), mv=bool(lg[3]), sig=tuple(int(x) for x in lg[4:11]), drawn=int(lg[11]),
                            dropped=bool(lg[12]), raw=int(case["actions"][k][i]), b=np.array(before[i]), a=np.array(fx_case["state"][k][i]),
                            reward=int(fx_case["reward"][k][i]), done=int(fx_case["done"][k][i]), t=int(fx_case["elapsed"][k]), T=v["T"],
                            t0=int(case["elapsed"] if k == 0 else fx_case["elapsed"][k - 1]),
                            raised=bool(fx_case["raised"][k]), done_all=bool(fx_case["done_all"][k]),
                            ended=bool(fx_case["done_all"][k]) and not bool(fx_case["raised"][k]), states1=[int(x) for x in fx_case["state"][k][:, 3]],
                            mc=mc[i], speed=v["speed"][i], earliest=v["earliest"][i], latest=v["latest"][i], target=target[i], init=m["init_pos"][i],
                            prev=out[k - 1][i] if k else None))
        for r in step:
            r.others = [o for o in step if o is not r]
        out.append(step)
    return out
