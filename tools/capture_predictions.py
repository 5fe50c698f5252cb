#!/usr/bin/env python3
"""Golden vectors of flatland.envs.predictions.ShortestPathPredictorForRailEnv.get() (predictions.py:97-180) and of
get_shortest_paths(env.distance_map, max_depth) (rail_env_shortest_paths.py:203-274) from the REAL reference.

Three kinds of sources, all built with the helpers of oracle/refharness/ (nothing there is edited):
  hand-made maps      capture_handmaps.make_env, the `actions` of tests/golden/handmap_<name>.npz replayed with the agent state asserted
                      against the fixture at every step; about 5 sampled steps, depths 1, 8, 9, 30 (mesh12: 500 too)
  constructed states  every case and control of tests/obs_state_cases.py, set as capture_obs_states.make_env sets them; depths 30, 10, 3;
                      positions and directions asserted equal to the pred_pos_pP / pred_dir_pP of tests/golden/obs_states_*.npz
  episodes            the recipes of capture_golden.JOBS replayed as tools/capture_global_obs.py does; about 6 sampled steps, depths 30, 10
-> tests/golden/predictions_<source>.npz.  A file holds GROUPS (`groups`: their names), one per map / case / episode; group G has
  G/grid u16[H][W], G/init_pos, G/target i32[A][2], G/init_dir i32[A], G/speed f64[A], G/dm u16[U][H][W][4] (0xFFFF = inf) and
  G/slot i32[A] (the reference's distance map per unique target, every agent's map), G/steps i32[S], G/state i32[S][A][12]
  (util.STATE_NAMES order), G/depths i32[n], and per depth D
  G/pred_dD f64[S][A][D + 1][5]   get() of every agent
  G/wp_dD i32[S][A][D][3], G/len_dD i32[S][A]   the waypoints (row, col, direction) of get_shortest_paths, -1 behind the length, 0 = None
  G/dev_dD i32[S][A][D][3], G/devlen_dD i32[S][A]   env.dev_pred_dict[handle] after get(), in insertion order
  G/get3 i32[n] (one state of the file's first group with more than 3 agents): the keys of get(3), with G/get0 and G/getnone.

Usage:  python tools/capture_predictions.py [--only SOURCE ...]
        python tools/capture_predictions.py --check [SOURCE ...]   re-capture into a temporary directory, compare bit for bit
        python tools/capture_predictions.py --time                 median of 20 calls of the reference's get() at depth 30, cfg2 / cfg3
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "oracle", "refharness"), REPO]
import capture_obs_states as cos  # noqa: E402  (sets up the reference's import path)
import numpy as np  # noqa: E402
from flatland.envs.observations import GlobalObsForRailEnv  # noqa: E402
from flatland.envs.predictions import ShortestPathPredictorForRailEnv  # noqa: E402
from flatland.envs.rail_env_shortest_paths import get_shortest_paths  # noqa: E402

from tests import handmaps, util  # noqa: E402
from tests import obs_state_cases as oc  # noqa: E402

ch, cg = cos.ch, cos.cg
HANDMAPS = {"oval": (1, 8, 9, 30), "lasso": (1, 8, 9, 30), "disconnected": (1, 8, 9, 30), "crossing_u1": (1, 8, 9, 30),
            "mesh12": (1, 8, 9, 30, 500)}
STATE_DEPTHS = (30, 10, 3)
# fixture -> (test_id, level, make_env keywords, speed_ratios): the recipes of capture_golden.JOBS
EPISODES = {
    "cfg1_malf20_spfollow": ("Test_0", "Level_2", dict(malfunction_interval=20), None),
    "cfg2_slow_trains": ("Test_2", "Level_4", {}, {1.0: 0.25, 1.0 / 20.0: 0.25, 1.0 / 33.0: 0.25, 1.0 / 50.0: 0.25}),
    "cfg0_tall_spfollow": ("Test_2", "Level_3", dict(dims=(26, 40), malfunction_interval=300), None),
}
EPISODE_DEPTHS = (30, 10)
SOURCES = ["handmaps"] + ["states_%s_%s" % s for s in oc.SETS] + ["episodes"]
STATIC_KEYS = ("grid", "init_pos", "init_dir", "target", "speed", "earliest", "latest", "T", "malf_min", "malf_max", "mt_key", "mt_pos")


def snapshot(env):
    s = cg.agent_snapshot(env)
    return np.stack([s[k] for k in util.STATE_NAMES], axis=1).astype(np.int32)


def static_of(env):
    d = cg.dm_unique(env)
    return dict(grid=np.asarray(env.rail.grid, dtype=np.uint16),
                init_pos=np.array([a.initial_position for a in env.agents], dtype=np.int32),
                init_dir=np.array([int(a.initial_direction) for a in env.agents], dtype=np.int32),
                target=np.array([a.target for a in env.agents], dtype=np.int32),
                speed=np.array([a.speed_counter.speed for a in env.agents], dtype=np.float64),
                dm=d["dm_u16"], slot=d["target_slot"])


def predict(env, depth):
    """the reference's own outputs for the env's current state"""
    A = env.get_num_agents()
    p = ShortestPathPredictorForRailEnv(depth)
    p.set_env(env)
    env.dev_pred_dict = {}
    with contextlib.redirect_stdout(io.StringIO()):
        got = p.get()
        paths = get_shortest_paths(env.distance_map, depth)
    assert sorted(got) == list(range(A)) and sorted(paths) == list(range(A))
    pred = np.stack([got[h] for h in range(A)])
    assert pred.dtype == np.float64 and pred.shape == (A, depth + 1, 5)
    wp = np.full((A, depth, 3), -1, dtype=np.int32)
    ln = np.zeros(A, dtype=np.int32)
    dev = np.full((A, depth, 3), -1, dtype=np.int32)
    devlen = np.zeros(A, dtype=np.int32)
    for h in range(A):
        if paths[h] is not None:
            assert 1 <= len(paths[h]) <= depth
            ln[h] = len(paths[h])
            for k, w in enumerate(paths[h]):
                wp[h, k] = (w.position[0], w.position[1], int(w.direction))
        v = list(env.dev_pred_dict[h])
        devlen[h] = len(v)
        for k, x in enumerate(v):
            dev[h, k] = [int(q) for q in x]
    return dict(pred=pred, wp=wp, len=ln, dev=dev, devlen=devlen)


def handle_keys(env, depth):
    """`if handle:` (predictions.py:122): the keys of get(3), get(0) and get(None)"""
    p = ShortestPathPredictorForRailEnv(depth)
    p.set_env(env)
    with contextlib.redirect_stdout(io.StringIO()):
        return {"get3": np.array(sorted(p.get(3)), dtype=np.int32), "get0": np.array(sorted(p.get(0)), dtype=np.int32),
                "getnone": np.array(sorted(p.get(None)), dtype=np.int32)}


class Group:
    def __init__(self, name, env, depths):
        self.name, self.depths = name, tuple(depths)
        self.out = static_of(env)
        self.steps, self.state = [], []
        self.rec = {(k, D): [] for D in self.depths for k in ("pred", "wp", "len", "dev", "devlen")}

    def sample(self, env, t):
        self.steps.append(t)
        self.state.append(snapshot(env))
        for D in self.depths:
            for k, v in predict(env, D).items():
                self.rec[(k, D)].append(v)
        assert np.array_equal(snapshot(env), self.state[-1])      # (the predictor changed nothing)
        return {D: self.rec[("pred", D)][-1] for D in self.depths}

    def arrays(self):
        o = {self.name + "/" + k: v for k, v in self.out.items()}
        o[self.name + "/steps"] = np.array(self.steps, dtype=np.int32)
        o[self.name + "/state"] = np.stack(self.state)
        o[self.name + "/depths"] = np.array(self.depths, dtype=np.int32)
        for (k, D), v in self.rec.items():
            o["%s/%s_d%d" % (self.name, k, D)] = np.stack(v)
        return o


def capture_handmaps():
    out, names = {}, []
    for name, depths in HANDMAPS.items():
        fx = np.load(os.path.join(util.GOLD, "handmap_%s.npz" % name))
        m = handmaps.MAPS[name]()
        env, _ = ch.make_env(m, 23)
        S = len(fx["actions"])
        env._max_episode_steps = max(int(env._max_episode_steps), S + 20)
        g = Group(name, env, depths)
        assert np.array_equal(snapshot(env), fx["state"][0]), name
        steps = sorted({0, S} | {int(t) for t in np.linspace(0, S, 5).astype(int)})
        A = env.get_num_agents()
        for t in range(S + 1):
            if t:
                with contextlib.redirect_stdout(io.StringIO()):
                    env.step({i: int(a) for i, a in enumerate(fx["actions"][t - 1])})
                assert np.array_equal(snapshot(env), fx["state"][t]), f"{name}: the agent state after step {t} is not the fixture's"
            if t in steps:
                g.sample(env, t)
                if not any(k.endswith("/get3") for k in out) and A > 3 and t == steps[1]:
                    for k, v in handle_keys(env, 8).items():
                        out[name + "/" + k] = v
                    out[name + "/get3_step"] = np.int32(len(g.steps) - 1)
        out.update(g.arrays())
        names.append(name)
    out["groups"] = np.array(names)
    return out


def capture_states(map_name, set_name):
    where = {n: f for f, part in zip(oc.fixture_files(map_name, set_name), oc.parts_of(map_name, set_name)) for n in part}
    stored = {f: np.load(os.path.join(util.GOLD, f + ".npz")) for f in set(where.values())}
    out, names = {}, []
    for c in oc.CASES:
        if (c["map"], c["set"]) != (map_name, set_name):
            continue
        env = cos.make_env(c)
        g = Group(c["name"], env, STATE_DEPTHS)
        preds = g.sample(env, 0)
        W = env.width
        for D, pred in preds.items():
            key = "%s/pred_pos_p%d" % (c["name"], D)
            if key in stored[where[c["name"]]].files:       # the upstream tree builder's own predicted_pos / predicted_dir
                pos, dirs = stored[where[c["name"]]][key], stored[where[c["name"]]]["%s/pred_dir_p%d" % (c["name"], D)]
                # (coordinate_to_position(width, ...) is col * width + row, core/grid/grid_utils.py)
                assert np.array_equal((pred[:, :, 2] * W + pred[:, :, 1]).T.astype(np.int64), pos), key
                assert np.array_equal(pred[:, :, 3].T.astype(np.int64), dirs), key
        out.update(g.arrays())
        names.append(c["name"])
    out["groups"] = np.array(names)
    return out


def episode_env(name):
    test_id, level, kw, speed_ratios = EPISODES[name]
    row = cg.csv_row(test_id, level)
    if speed_ratios is not None:
        row["speed_ratios"] = dict(speed_ratios)
    env, mp = cg.make_env(row, kw.get("malfunction_interval"), obs=GlobalObsForRailEnv(), dims=kw.get("dims"))
    env.reset()
    return env, mp


def fixture_state(fx, t):
    if t == 0:
        order = sorted(util.STATE_NAMES)
        return np.stack([fx["snap0"][order.index(k)] for k in util.STATE_NAMES], axis=1).astype(np.int32)
    return util.golden_state(fx, t - 1)


def capture_episodes():
    out, names = {}, []
    for name in EPISODES:
        fx = util.load(name)
        env, mp = episode_env(name)
        st0 = cg.static_arrays(env, mp)
        for k in STATIC_KEYS:
            assert np.array_equal(st0[k], fx[k]), f"{name}: the rebuilt env's {k} is not the fixture's"
        actions = util.actions_of(fx)
        S = len(actions)
        A = env.get_num_agents()
        done_first = next((t for t in range(1, S + 1) if (np.asarray(fx["s_state"])[t - 1] == 6).any()), S)
        steps = sorted({0, done_first, S} | {int(t) for t in np.linspace(0, S, 5).astype(int)})[:7]
        g = Group(name, env, EPISODE_DEPTHS)
        assert np.array_equal(snapshot(env), fixture_state(fx, 0))
        for t in range(max(steps) + 1):
            if t:
                a = actions[t - 1]
                env.step({i: int(a[i]) for i in range(A) if a[i] != cg.ABSENT})
                assert np.array_equal(snapshot(env), fixture_state(fx, t)), f"{name}: the agent state after step {t} is not the fixture's"
            if t in steps:
                g.sample(env, t)
        out.update(g.arrays())
        names.append(name)
    out["groups"] = np.array(names)
    return out


def capture(source, gold_dir):
    if source == "handmaps":
        out = capture_handmaps()
    elif source == "episodes":
        out = capture_episodes()
    else:
        m, s = source[len("states_"):].split("_")
        out = capture_states(m, s)
    path = os.path.join(gold_dir, "predictions_%s.npz" % source)
    np.savez_compressed(path, **out)
    raw = sum(v.nbytes for v in out.values())
    assert os.path.getsize(path) < 1 << 20, path
    print(f"predictions_{source}: {len(out['groups'])} groups, {len(out)} arrays, {raw / 1024:.0f} KB -> {os.path.getsize(path) / 1024:.0f} KB")
    return path


def check(sources):
    tmp = tempfile.mkdtemp(prefix="predictions_check_")
    problems, n = [], 0
    try:
        for src in sources:
            new = np.load(capture(src, tmp))
            old_path = os.path.join(util.GOLD, "predictions_%s.npz" % src)
            if not os.path.exists(old_path):
                problems.append(f"predictions_{src}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                n += 1
                if k not in new.files or k not in old.files:
                    problems.append(f"predictions_{src}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"predictions_{src}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems, n


def time_reference():
    """the host baseline: the reference's own ShortestPathPredictorForRailEnv(30).get() on one env, median of 20 calls"""
    for label, (test_id, level) in (("cfg2", ("Test_2", "Level_4")), ("cfg3", ("Test_4", "Level_0"))):
        env, _ = cg.make_env(cg.csv_row(test_id, level), obs=GlobalObsForRailEnv())
        env.reset()
        p = ShortestPathPredictorForRailEnv(30)
        p.set_env(env)
        p.get()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            p.get()
            ts.append(time.perf_counter() - t0)
        print(f"reference get() depth 30, {label}: {env.height}x{env.width}, {env.get_num_agents()} agents, ONE env: "
              f"median {np.median(ts) * 1e3:.2f} ms of 20 calls on this CPU")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", nargs="*", default=None, metavar="SOURCE")
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if args.time:
        time_reference()
        sys.exit(0)
    if args.check is not None:
        bad, n = check(args.check or SOURCES)
        for line in bad:
            print("MISMATCH", line)
        print("predictions golden check: %d arrays," % n, "all identical" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for src in (args.only or SOURCES):
        capture(src, util.GOLD)
