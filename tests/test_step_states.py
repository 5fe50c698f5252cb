"""CPU side of the constructed step states (tests/step_state_cases.py; fixtures tests/golden/step_states_<map>.npz from the real RailEnv,
oracle/refharness/capture_step_states.py): every row of the table is reached by a case that names it, judged on the reference's log; the
injected rows keep fl_set_state's rules; the oracle, started from the state (orc_set_state), equals the reference after every step."""
import numpy as np
import pytest

from oracle import orc
from tests import handmaps, step_state_cases as sc, util

MAPS = tuple(handmaps.STEP_MAPS)


@pytest.fixture(scope="module")
def fixtures():
    return {m: util.load("step_states_" + m) for m in MAPS}


def fx_case(fx, name):
    return {k: fx[name + "/" + k] for k in ("state", "aux", "reward", "done", "done_all", "raised", "elapsed", "mt_key_id", "mt_pos", "log")}


def test_the_modules_data_is_what_it_says():
    assert 150 <= len(sc.CASES) <= 250
    assert all(c["doc"] and c["rows"] for c in sc.CASES)
    for c in sc.CASES:
        H, W = handmaps.STEP_MAPS[c["map"]]()["grid"].shape
        assert H <= 12 and W <= 12 and c["state"].shape == (5, 12) and c["actions"].dtype == np.uint8
    raw = np.concatenate([c["actions"].ravel() for c in sc.CASES])
    assert {0, 1, 2, 3, 4, sc.ABSENT, sc.ILLEGAL} <= set(raw.tolist()) and 4 < sc.ILLEGAL < 255
    assert sorted({mc for m in sc.VARIANTS for v in sc.VARIANTS[m] for mc in sc.max_count(m, v)}) == [0, 1, 2, 3]
    assert int(1 / 0.3) - 1 == 2 and int(1 / (1 / 93)) == 92 and 92 - 1 > 63      # 1/93 needs max_count 91: beyond FL_MAX_SPEED_COUNT
    assert sc.TRUNCATING_SPEEDS == []                                              # ... and no 1/n that the library admits truncates
    # the seeds written down fire the agents they were searched for
    for (pattern, variant, pos), seed in sc._SEEDS.items():
        assert sc.fires_as(seed, [set(p) for p in pattern], variant, pos=pos), (pattern, variant)
    # every new map holds the cells it was drawn for
    g = handmaps.yard()["grid"]
    assert g[handmaps.YARD_SYM] == handmaps.SYM_SWITCH and handmaps.nibble(g[handmaps.YARD_SYM], handmaps.N) == 0b0101
    assert all(handmaps.known_cell_type(v) for v in g.ravel())


def test_fixtures_hold_the_cases_in_order(fixtures):
    for m in MAPS:
        assert [str(n) for n in fixtures[m]["names"]] == [c["name"] for c in sc.CASES if c["map"] == m]
        for c in sc.CASES:
            if c["map"] == m:
                f = fx_case(fixtures[m], c["name"])
                K = len(c["actions"])
                assert f["state"].shape == (K, 5, 12) and f["log"].shape == (K, 5, 13) and f["mt_key_id"].shape == (K,)
                # wherever the reference took a train there is rail, and the train faces a way the cell allows (the kernels index the
                # env's rail tables with the position)
                g = handmaps.STEP_MAPS[m]()["grid"]
                for row in f["state"].reshape(-1, 12):
                    assert row[0] < 0 or (g[row[0], row[1]] != 0 and handmaps.nibble(g[row[0], row[1]], row[2]) != 0), (c["name"], row)


def test_every_table_row_is_reached_by_a_case_that_names_it(fixtures):
    """Every row of step_state_cases.TABLE is named by at least one case and its predicate holds on the log the reference left for each
    case that names it; no row is waived.

    Of the 27 state-machine rows of the table (22 handler branches, update_if_reached after three states, both signals at once, MOVING on
    its target) the 18 recorded episodes reach 24: 22 of the 24 (state before, state after) pairs that carry them occur in their 310 000
    agent-steps; of the three pairs with two rows each, WAITING -> MALFUNCTION_OFF_MAP and MOVING -> STOPPED reach both of theirs, and
    MOVING -> DONE only update_if_reached (a train is removed when it arrives, so none ever stands MOVING on its target);
    MALFUNCTION_OFF_MAP -> STOPPED and MALFUNCTION -> DONE never occur.  The other 52 rows of the table (placement, actions,
    saver, counters, draws, the end of the episode) are not counted: they need the signals, which an episode fixture does not hold.
    test_recorded_episodes_reach_24_of_the_27_state_machine_rows recomputes the figures from the fixtures."""
    claimed = {}
    for c in sc.CASES:
        rs = [r for step in sc.recs(c, fx_case(fixtures[c["map"]], c["name"])) for r in step]
        for row in c["rows"]:
            assert any(sc.TABLE[row](r) for r in rs), "case %s does not reach %s" % (c["name"], row)
            claimed.setdefault(row, []).append(c["name"])
    assert sorted(claimed) == sorted(sc.TABLE), sorted(set(sc.TABLE) - set(claimed))


# the 27 state-machine rows by (state before, state after); three pairs carry two rows each, told apart from the episode's own arrays
ROWS_OF_PAIR = {
    (sc.WAITING, sc.MALF_OFF): ("waiting.malf", "waiting.malf_and_departure"), (sc.WAITING, sc.READY): ("waiting.ready",),
    (sc.WAITING, sc.WAITING): ("waiting.stay",), (sc.READY, sc.MALF_OFF): ("ready.malf",), (sc.READY, sc.MOVING): ("ready.moving",),
    (sc.READY, sc.READY): ("ready.stay",), (sc.MALF_OFF, sc.MOVING): ("malfoff.moving",), (sc.MALF_OFF, sc.STOPPED): ("malfoff.stopped",),
    (sc.MALF_OFF, sc.READY): ("malfoff.ready",), (sc.MALF_OFF, sc.WAITING): ("malfoff.waiting",), (sc.MALF_OFF, sc.MALF_OFF): ("malfoff.stay",),
    (sc.MOVING, sc.MALF): ("moving.malf",), (sc.MOVING, sc.DONE): ("moving.done_before_move", "reached.from_moving"),
    (sc.MOVING, sc.STOPPED): ("moving.stopped_by_stop", "moving.stopped_by_conflict"), (sc.MOVING, sc.MOVING): ("moving.stay",),
    (sc.STOPPED, sc.MALF): ("stopped.malf",), (sc.STOPPED, sc.MOVING): ("stopped.moving",), (sc.STOPPED, sc.STOPPED): ("stopped.stay",),
    (sc.MALF, sc.MOVING): ("malf.moving",), (sc.MALF, sc.STOPPED): ("malf.stopped",), (sc.MALF, sc.MALF): ("malf.stay",),
    (sc.DONE, sc.DONE): ("done.stay",), (sc.STOPPED, sc.DONE): ("reached.from_stopped",), (sc.MALF, sc.DONE): ("reached.from_malf",),
}


def _episode_rows(names):
    """(the (state before, state after) pairs, the state-machine rows of the table) that the recorded episodes reach.  A pair with one row
    reaches it; WAITING -> MALFUNCTION_OFF_MAP is also `both signals at once` when t >= earliest_departure; MOVING -> DONE is `on its
    target before the move` when the train stood on the target, else update_if_reached; MOVING -> STOPPED is `by stop` when the
    preprocessed action (action_preprocessing.py, restated for a MOVING agent) is STOP_MOVING, else `by conflict`"""
    pairs, rows = set(), set()
    for n in names:
        fx = util.load(n)
        s1 = np.asarray(fx["s_state"]).astype(np.int64)
        s0 = np.concatenate([np.zeros((1, s1.shape[1]), dtype=np.int64), s1[:-1]])      # after reset(): WAITING
        here = {(int(p) // 7, int(p) % 7) for p in np.unique(s0 * 7 + s1)}
        pairs |= here
        rows |= {ROWS_OF_PAIR[p][0] for p in here if len(ROWS_OF_PAIR[p]) == 1}
        t = np.arange(1, len(s1) + 1)[:, None]
        wm = (s0 == sc.WAITING) & (s1 == sc.MALF_OFF)
        rows |= {"waiting.malf"} if wm.any() else set()
        rows |= {"waiting.malf_and_departure"} if (wm & (t >= np.asarray(fx["earliest"])[None])).any() else set()
        row0, col0, dir0 = (np.concatenate([np.full((1, s1.shape[1]), -1), np.asarray(fx[k])[:-1]]) for k in ("s_row", "s_col", "s_dir"))
        md = (s0 == sc.MOVING) & (s1 == sc.DONE)
        on_target = (row0 == np.asarray(fx["target"])[None, :, 0]) & (col0 == np.asarray(fx["target"])[None, :, 1])
        rows |= {"moving.done_before_move"} if (md & on_target).any() else set()
        rows |= {"reached.from_moving"} if (md & ~on_target).any() else set()
        acts, grid = util.actions_of(fx), np.asarray(fx["grid"])
        for k, i in np.argwhere((s0 == sc.MOVING) & (s1 == sc.STOPPED)):
            a = int(acts[k][i])
            a = sc.FORWARD if a == 0 or a > 4 else a                                  # absent, illegal, DO_NOTHING: FORWARD when MOVING
            if a in (sc.LEFT, sc.RIGHT) and not sc._valid(grid, row0[k, i], col0[k, i], dir0[k, i], a):
                a = sc.FORWARD
            if a != sc.STOP and not sc._valid(grid, row0[k, i], col0[k, i], dir0[k, i], a):
                a = sc.STOP
            rows.add("moving.stopped_by_stop" if a == sc.STOP else "moving.stopped_by_conflict")
    return pairs, rows


def test_recorded_episodes_reach_24_of_the_27_state_machine_rows():
    """the numbers in the docstring above, recomputed from the 18 episode fixtures"""
    assert sorted(r for rs in ROWS_OF_PAIR.values() for r in rs) == sorted(list(sc.TABLE)[:27])      # (the table begins with them)
    pairs, rows = _episode_rows(util.episode_fixtures())
    assert len(ROWS_OF_PAIR) == 24 and len(pairs) == 22
    assert sorted(set(ROWS_OF_PAIR) - pairs) == [(sc.MALF_OFF, sc.STOPPED), (sc.MALF, sc.DONE)]
    missing = sorted({r for rs in ROWS_OF_PAIR.values() for r in rs} - rows)
    assert missing == ["malfoff.stopped", "moving.done_before_move", "reached.from_malf"], missing


def _consistent(case, grid):
    """fl_set_state's own rules on the injected rows"""
    H, W = grid.shape
    for row, aux in zip(case["state"], case["aux"]):
        r, c, d, st, mf, nmf, scn, sv, arr, orow, ocol, od = (int(v) for v in row)
        on = r >= 0
        assert (not on or (r < H and 0 <= c < W)) and 0 <= d <= 3 and 0 <= st <= 6 and 0 <= mf <= 0xFFFF and 0 <= nmf <= 0xFFFF
        assert 0 <= scn <= 63 and 0 <= sv <= 3 and -1 <= od <= 3 and (orow < 0 or (orow < H and 0 <= ocol < W))
        assert on == (sc.MOVING <= st <= sc.MALF)
        assert (not on or grid[r, c] != 0) and (orow < 0 or grid[orow, ocol] != 0)
        assert -1 <= aux[0] <= 6 and set(aux[1:].tolist()) <= {0, 1}
    assert case["elapsed"] >= 0


@pytest.mark.parametrize("map_name", MAPS)
def test_oracle_started_from_the_state_equals_the_reference(fixtures, map_name):
    fx = fixtures[map_name]
    keys = fx["mt_keys"]
    for c in (c for c in sc.CASES if c["map"] == map_name):
        st = sc.static_of(c["map"], c["variant"], c["rng"])
        _consistent(c, st["grid"])
        mc = sc.max_count(c["map"], c["variant"])
        assert all(row[6] <= mc[i] for i, row in enumerate(c["state"])), c["name"]
        o = orc.OracleEnv(st)
        o.set_state(c["state"], c["aux"], c["elapsed"], c["done_all"])
        assert np.array_equal(o.state(), c["state"]) and np.array_equal(o.state_aux(), c["aux"])
        f = fx_case(fx, c["name"])
        for k, acts in enumerate(c["actions"]):
            w = "%s step %d" % (c["name"], k)
            acts = acts.copy()
            acts[f["log"][k][:, 12] == 1] = sc.ABSENT      # eval_env.parse_actions dropped them
            if f["raised"][k]:
                with pytest.raises(RuntimeError, match="Episode is done"):
                    o.step(acts)
                rew, done, done_all = np.zeros(5, np.int32), f["done"][k], True      # (the env's dones stay as they were)
            else:
                rew, done, done_all = o.step(acts)
            assert np.array_equal(o.state(), f["state"][k]), w + " rows\n%s\n%s" % (o.state(), f["state"][k])
            assert np.array_equal(o.state_aux()[:, [0, 1, 3]], f["aux"][k][:, [0, 1, 3]]), w + " aux"
            assert np.array_equal(rew, f["reward"][k]), w + " rewards %s %s" % (rew, f["reward"][k])
            assert np.array_equal(done, f["done"][k]) and bool(done_all) == bool(f["done_all"][k]), w + " dones"
            assert o.elapsed() == f["elapsed"][k], w + " elapsed"
            key, pos = o.get_rng()
            assert pos == f["mt_pos"][k] and np.array_equal(key, keys[f["mt_key_id"][k]]), w + " rng"


def test_set_state_refuses_what_fl_set_state_refuses():
    c = sc.BY_NAME["moving_forward"]
    o = orc.OracleEnv(sc.static_of(c["map"], c["variant"]))
    for col, val in ((2, 4), (3, 7), (4, -1), (6, 64), (7, 4), (11, 4), (0, 8), (9, 8)):
        bad = c["state"].copy()
        bad[0, col] = val
        with pytest.raises(ValueError, match="out of range"):
            o.set_state(bad)
    bad = c["state"].copy()
    bad[0, 3] = sc.READY                      # on the map in an off-map state
    with pytest.raises(ValueError, match="does not match position"):
        o.set_state(bad)
    bad = c["state"].copy()
    bad[0, 0:2] = (0, 0)                      # no rail there
    with pytest.raises(ValueError, match="not a rail cell"):
        o.set_state(bad)
    aux = c["aux"].copy()
    aux[1, 3] = 2
    with pytest.raises(ValueError, match="aux value out of range"):
        o.set_state(c["state"], aux)
    with pytest.raises(ValueError, match="negative elapsed"):
        o.set_state(c["state"], None, -1)
    o.set_state(c["state"], None, 3)          # aux left out: fl_set_state's defaults
    assert np.array_equal(o.state_aux(), np.stack([[-1, int(r[4] > 0), 0, int(r[3] == sc.DONE)] for r in c["state"]]))
