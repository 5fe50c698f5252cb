#!/usr/bin/env python3
"""Golden vectors of the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py from the REAL reference:
possible_actions_sorted_by_distance (:14-56), find_all_cells_where_agent_can_choose (:145-176), SkipNoChoiceCellsWrapper.on_decision_cell
(:197-198), and one episode driven through SkipNoChoiceCellsWrapper(ShortestPathActionWrapper(env), True, 0.9) (:122-141, :179-258).

The sources are those of tools/capture_predictions.py, built with the helpers of oracle/refharness/ (nothing there is edited):
  hand-made maps      the `actions` of tests/golden/handmap_<name>.npz replayed, the agent state asserted against the fixture at every step;
                      up to 24 sampled steps
  constructed states  every case and control of tests/obs_state_cases.py (they hold MALFUNCTION and MALFUNCTION_OFF_MAP)
  episodes            the three recipes of capture_predictions.EPISODES replayed (one of them taller than wide); about 12 sampled steps
-> tests/golden/action_space_<source>.npz.  A file holds GROUPS (`groups`: their names); group G has
  G/grid u16[H][W], G/init_pos, G/target i32[A][2], G/init_dir i32[A], G/speed f64[A], G/dm u16[U][H][W][4] (0xFFFF = inf) and
  G/slot i32[A] (the reference's distance map per unique target, every agent's map), G/steps i32[S], G/state i32[S][A][12]
  (util.STATE_NAMES order), and
  G/sp_action u8[S][A][3], G/sp_dist f64[S][A][3], G/sp_count u8[S][A]   the list of every agent: 0 / inf behind its length
  G/on_decision u8[S][A]                                                 on_decision_cell(agent)
  G/cells u8[H][W]                                                       bit 0: in `switches`, bit 1: in `switches_neighbors`
The file of the episodes has one more group, `wrapped_episode`: the stacked wrappers on cfg1_malf20_spfollow's env (its statics are that
fixture's), driven by numpy.random.RandomState(WRAPPED_SEED).choice((0, 1, 2), A) per outer step for at most WRAPPED_STEPS outer steps:
  wrapped_episode/reduced u8[S][A], /present u8[S][A] (the keys of o), /reward f64[S][A], /done u8[S][A], /done_all u8[S],
  /action_required u8[S][A], /malfunction i32[S][A], /speed f64[S][A], /info_state i32[S][A] (the four info dicts; 0 where not present),
  /state i32[S][A][12] (after the outer step), /inner i32[S] (env.step calls of the outer step)
and the file of the hand-made maps `wrapped_lasso`, the same record on the lasso (the env of tests/golden/handmap_lasso.npz) with the
choices (0, 1, 1, 1, 2) until the episode ends: there agents are skipped while others are handed back, and the rewards are not 0.

Usage:  python tools/capture_action_space.py [--only SOURCE ...]
        python tools/capture_action_space.py --check [SOURCE ...]   re-capture into a temporary directory, compare bit for bit
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "oracle", "refharness"), REPO]
import capture_predictions as cp  # noqa: E402  (sets up the reference's import path; its groups' statics and episodes are reused)
import numpy as np  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from flatland.contrib.wrappers import flatland_wrappers as fw  # noqa: E402

from tests import handmaps, util  # noqa: E402
from tests import obs_state_cases as oc  # noqa: E402

ch, cg, cos = cp.ch, cp.cg, cp.cos
SOURCES = cp.SOURCES
HANDMAP_STEPS, EPISODE_STEPS = 24, 12
WRAPPED_ENV, WRAPPED_SEED, WRAPPED_STEPS = "cfg1_malf20_spfollow", 7, 40
WRAPPED_HANDMAP = "lasso"
SLOTS = 3


def quiet():
    """the reference prints at every call"""
    return contextlib.redirect_stdout(io.StringIO())


def cells_of(env):
    with quiet():
        switches, neighbors, decision = fw.find_all_cells_where_agent_can_choose(env)
    assert decision == switches | neighbors
    cells = np.zeros((env.height, env.width), dtype=np.uint8)
    for bit, group in ((1, switches), (2, neighbors)):
        for r, c in group:
            # (a cell a switch points at lies on the grid and has rail on every map recorded here: the byte map loses nothing)
            assert 0 <= r < env.height and 0 <= c < env.width and env.rail.grid[r, c] != 0, (r, c)
            cells[r, c] |= bit
    return cells


def lists_of(env, skip):
    A = env.get_num_agents()
    act = np.zeros((A, SLOTS), dtype=np.uint8)
    dist = np.full((A, SLOTS), np.inf, dtype=np.float64)
    cnt = np.zeros(A, dtype=np.uint8)
    dec = np.zeros(A, dtype=np.uint8)
    with quiet():
        for h in range(A):
            got = fw.possible_actions_sorted_by_distance(env, h)
            assert 2 <= len(got) <= SLOTS, (h, got)
            cnt[h] = len(got)
            for k, (a, dd) in enumerate(got):
                act[h, k] = int(a)
                dist[h, k] = float(dd)
            dec[h] = bool(skip.on_decision_cell(env.agents[h]))
    return dict(sp_action=act, sp_dist=dist, sp_count=cnt, on_decision=dec)


class Group:
    def __init__(self, name, env):
        self.name = name
        self.out = cp.static_of(env)
        self.out["cells"] = cells_of(env)
        with quiet():
            self.skip = fw.SkipNoChoiceCellsWrapper(env, False, 1.0)
        self.steps, self.state = [], []
        self.rec = {k: [] for k in ("sp_action", "sp_dist", "sp_count", "on_decision")}

    def sample(self, env, t):
        self.steps.append(t)
        self.state.append(cp.snapshot(env))
        for k, v in lists_of(env, self.skip).items():
            self.rec[k].append(v)
        assert np.array_equal(cp.snapshot(env), self.state[-1])

    def arrays(self):
        o = {self.name + "/" + k: v for k, v in self.out.items()}
        o[self.name + "/steps"] = np.array(self.steps, dtype=np.int32)
        o[self.name + "/state"] = np.stack(self.state)
        for k, v in self.rec.items():
            o[self.name + "/" + k] = np.stack(v)
        return o


def sampled(S, n):
    return sorted({int(t) for t in np.linspace(0, S, min(n, S + 1)).astype(int)})


def capture_handmaps():
    out, names = {}, []
    for name in cp.HANDMAPS:
        fx = np.load(os.path.join(util.GOLD, "handmap_%s.npz" % name))
        env, _ = ch.make_env(handmaps.MAPS[name](), 23)
        S = len(fx["actions"])
        env._max_episode_steps = max(int(env._max_episode_steps), S + 20)
        g = Group(name, env)
        assert np.array_equal(cp.snapshot(env), fx["state"][0]), name
        steps = sampled(S, HANDMAP_STEPS)
        for t in range(S + 1):
            if t:
                with quiet():
                    env.step({i: int(a) for i, a in enumerate(fx["actions"][t - 1])})
                assert np.array_equal(cp.snapshot(env), fx["state"][t]), f"{name}: the agent state after step {t} is not the fixture's"
            if t in steps:
                g.sample(env, t)
        out.update(g.arrays())
        names.append(name)
    # (agents that stay off the map keep the recorded episode's inner loop at one step and its rewards at 0: on the lasso trains run past
    # cells without a choice, rewards are skipped and summed, and the episode ends)
    env, _ = ch.make_env(handmaps.MAPS[WRAPPED_HANDMAP](), 23)
    env._max_episode_steps = int(util.load("handmap_" + WRAPPED_HANDMAP)["T"])      # (the episode length the fixture's statics carry)
    out.update(capture_wrapped("wrapped_" + WRAPPED_HANDMAP, env, WRAPPED_SEED, (0, 1, 1, 1, 2), env._max_episode_steps))
    names.append("wrapped_" + WRAPPED_HANDMAP)
    out["groups"] = np.array(names)
    return out


def capture_states(map_name, set_name):
    out, names = {}, []
    for c in oc.CASES:
        if (c["map"], c["set"]) != (map_name, set_name):
            continue
        env = cos.make_env(c)
        g = Group(c["name"], env)
        g.sample(env, 0)
        out.update(g.arrays())
        names.append(c["name"])
    out["groups"] = np.array(names)
    return out


def replayed_episode(name):
    """the env of a recorded episode with its fixture, checked against it"""
    fx = util.load(name)
    env, mp = cp.episode_env(name)
    st0 = cg.static_arrays(env, mp)
    for k in cp.STATIC_KEYS:
        assert np.array_equal(st0[k], fx[k]), f"{name}: the rebuilt env's {k} is not the fixture's"
    assert np.array_equal(cp.snapshot(env), cp.fixture_state(fx, 0))
    return env, fx


def capture_episodes():
    out, names = {}, []
    for name in cp.EPISODES:
        env, fx = replayed_episode(name)
        actions = util.actions_of(fx)
        S, A = len(actions), env.get_num_agents()
        done_first = next((t for t in range(1, S + 1) if (np.asarray(fx["s_state"])[t - 1] == 6).any()), S)
        steps = sorted({done_first} | set(sampled(S, EPISODE_STEPS)))
        g = Group(name, env)
        for t in range(max(steps) + 1):
            if t:
                a = actions[t - 1]
                env.step({i: int(a[i]) for i in range(A) if a[i] != cg.ABSENT})
                assert np.array_equal(cp.snapshot(env), cp.fixture_state(fx, t)), f"{name}: the agent state after step {t} is not the fixture's"
            if t in steps:
                g.sample(env, t)
        out.update(g.arrays())
        names.append(name)
    out.update(capture_wrapped("wrapped_episode", replayed_episode(WRAPPED_ENV)[0], WRAPPED_SEED, (0, 1, 2)))
    names.append("wrapped_episode")
    out["groups"] = np.array(names)
    return out


def capture_wrapped(name, env, seed, choices, outer_steps=WRAPPED_STEPS):
    """the reference's stacked wrappers on `env`, a reduced action drawn from `choices` per agent and outer step"""
    A = env.get_num_agents()
    calls = [0]
    inner_step = env.step

    def counted(action_dict):
        calls[0] += 1
        return inner_step(action_dict)

    env.step = counted
    with quiet():
        top = fw.SkipNoChoiceCellsWrapper(fw.ShortestPathActionWrapper(env), True, 0.9)
    rng = np.random.RandomState(seed)
    rec = {k: [] for k in ("reduced", "present", "reward", "done", "done_all", "action_required", "malfunction", "speed", "info_state",
                           "state", "inner")}
    for _ in range(outer_steps):
        row = rng.choice(np.array(choices, dtype=np.uint8), A)
        calls[0] = 0
        with quiet():
            o, r, d, i = top.step({h: int(row[h]) for h in range(A)})
        keys = sorted(o)
        assert keys == sorted(r) == sorted(k for k in d if k != "__all__") and all(sorted(i[k]) == keys for k in i)
        present = np.zeros(A, dtype=np.uint8)
        present[keys] = 1
        z = lambda dt: np.zeros(A, dtype=dt)  # noqa: E731
        rw, dn, ar, mf, sp, st = z(np.float64), z(np.uint8), z(np.uint8), z(np.int32), z(np.float64), z(np.int32)
        for h in keys:
            rw[h], dn[h] = r[h], d[h]
            ar[h], mf[h], sp[h], st[h] = i["action_required"][h], i["malfunction"][h], i["speed"][h], int(i["state"][h])
        for k, v in (("reduced", row), ("present", present), ("reward", rw), ("done", dn), ("done_all", np.uint8(d["__all__"])),
                     ("action_required", ar), ("malfunction", mf), ("speed", sp), ("info_state", st), ("state", cp.snapshot(env)),
                     ("inner", np.int32(calls[0]))):
            rec[k].append(v)
        if d["__all__"]:
            break
    return {name + "/" + k: np.stack(v) for k, v in rec.items()}


def capture(source, gold_dir):
    if source == "handmaps":
        out = capture_handmaps()
    elif source == "episodes":
        out = capture_episodes()
    else:
        m, s = source[len("states_"):].split("_")
        out = capture_states(m, s)
    path = os.path.join(gold_dir, "action_space_%s.npz" % source)
    np.savez_compressed(path, **out)
    raw = sum(v.nbytes for v in out.values())
    assert os.path.getsize(path) < 1 << 20, path
    print(f"action_space_{source}: {len(out['groups'])} groups, {len(out)} arrays, {raw / 1024:.0f} KB -> {os.path.getsize(path) / 1024:.0f} KB")
    return path


def check(sources):
    tmp = tempfile.mkdtemp(prefix="action_space_check_")
    problems, n = [], 0
    try:
        for src in sources:
            new = np.load(capture(src, tmp))
            old_path = os.path.join(util.GOLD, "action_space_%s.npz" % src)
            if not os.path.exists(old_path):
                problems.append(f"action_space_{src}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                n += 1
                if k not in new.files or k not in old.files:
                    problems.append(f"action_space_{src}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"action_space_{src}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems, n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", nargs="*", default=None, metavar="SOURCE")
    args = ap.parse_args()
    if args.check is not None:
        bad, n = check(args.check or SOURCES)
        for line in bad:
            print("MISMATCH", line)
        print("action-space golden check: %d arrays," % n, "all identical" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for src in (args.only or SOURCES):
        capture(src, util.GOLD)
