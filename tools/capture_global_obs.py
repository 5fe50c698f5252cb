#!/usr/bin/env python3
"""Golden vectors of flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) from the REAL reference.

For each episode fixture below, the reference env is rebuilt with oracle/refharness/capture_golden.py's own helpers (csv_row,
make_env, the CSV row's seed and the fixture's recipe of capture_golden.JOBS), its static side is checked against the fixture,
and it is driven with the fixture's recorded action stream (tests/util.actions_of), the agent state asserted equal to the
fixture's at every step.  At a few sampled steps the reference's own GlobalObsForRailEnv outputs are recorded ->
tests/golden/global_<fixture>.npz:
  steps i32[S] (0 = after reset()), state i32[S][A][12] (the agent rows, util.STATE_NAMES order), rail f64[H][W][16] (one array
  for every handle and step), agents_state f64[S][A][H][W][5], targets f64[S][A][H][W][2].

Usage:  python tools/capture_global_obs.py [--only FIXTURE ...]
        python tools/capture_global_obs.py --check [FIXTURE ...]   re-capture into a temporary directory, compare bit for bit
"""
import argparse
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "oracle", "refharness"), REPO]
import capture_golden as cg  # noqa: E402  (sets up the reference's import path)
import numpy as np  # noqa: E402
from flatland.envs.observations import GlobalObsForRailEnv  # noqa: E402

from tests import util  # noqa: E402

# fixture -> (test_id, level, make_env keywords, speed_ratios, sampled steps): the recipes of capture_golden.JOBS
RECIPES = {
    "cfg0_tall_spfollow": ("Test_2", "Level_3", dict(dims=(26, 40), malfunction_interval=300), None, 8),
    "cfg1_malf20_spfollow": ("Test_0", "Level_2", dict(malfunction_interval=20), None, 8),
    "cfg2_slow_trains": ("Test_2", "Level_4", {}, {1.0: 0.25, 1.0 / 20.0: 0.25, 1.0 / 33.0: 0.25, 1.0 / 50.0: 0.25}, 8),
    "cfg1_sparse": ("Test_0", "Level_0", {}, None, 8),
    "cfg3_spfollow_malf100": ("Test_4", "Level_0", dict(malfunction_interval=100), None, 5),
}
STATIC_KEYS = ("grid", "init_pos", "init_dir", "target", "speed", "earliest", "latest", "T", "malf_min", "malf_max", "mt_key", "mt_pos")


def fixture_state(fx, t):
    """[A, 12] agent rows after t steps (t = 0: after reset(), the fixture's snap0)"""
    if t == 0:
        order = sorted(util.STATE_NAMES)
        return np.stack([fx["snap0"][order.index(k)] for k in util.STATE_NAMES], axis=1).astype(np.int32)
    return util.golden_state(fx, t - 1)


def pick_steps(fx, n):
    """t = 0, the first step with an agent MALFUNCTION_OFF_MAP, with a DONE agent, with a DONE agent's target under another
    train, the last step, then evenly spaced ones up to n"""
    S = len(fx["actions"])
    st = np.asarray(fx["s_state"])
    pick = [0]

    def first(cond):
        for t in range(1, S + 1):
            if cond(t):
                return t
        return None

    def done_target_occupied(t):
        s = fixture_state(fx, t)
        occ = {(int(r), int(c)) for r, c, q in zip(s[:, 0], s[:, 1], s[:, 3]) if r >= 0 and 3 <= q <= 5}
        return any(q == 6 and tuple(int(v) for v in fx["target"][i]) in occ for i, q in enumerate(s[:, 3]))

    for t in (first(lambda t: (st[t - 1] == 2).any()), first(lambda t: (st[t - 1] == 6).any()), first(done_target_occupied), S):
        if t is not None and t not in pick:
            pick.append(t)
    for t in np.linspace(0, S, n + 2).astype(int)[1:-1]:
        if len(pick) >= n:
            break
        if int(t) not in pick:
            pick.append(int(t))
    return sorted(pick[:max(n, 1)])


def capture(name, gold_dir):
    test_id, level, kw, speed_ratios, n = RECIPES[name]
    fx = util.load(name)
    row = cg.csv_row(test_id, level)
    if speed_ratios is not None:
        row["speed_ratios"] = dict(speed_ratios)
    builder = GlobalObsForRailEnv()
    env, mp = cg.make_env(row, kw.get("malfunction_interval"), obs=builder, dims=kw.get("dims"))
    obs, _ = env.reset()
    st0 = cg.static_arrays(env, mp)
    for k in STATIC_KEYS:
        assert np.array_equal(st0[k], fx[k]), f"{name}: the rebuilt env's {k} is not the fixture's"
    assert builder.get_many(None) == {}      # core/env_observation_builder.py:52-55
    actions = util.actions_of(fx)
    steps = pick_steps(fx, n)
    A = env.get_num_agents()
    rec = {"state": [], "agents_state": [], "targets": []}
    rail = None

    def record(t, obs):
        nonlocal rail
        s = np.stack([cg.agent_snapshot(env)[k] for k in util.STATE_NAMES], axis=1).astype(np.int32)
        assert all(obs[h][0] is obs[0][0] for h in range(A)), "rail_obs is one array for every handle"
        if rail is None:
            rail = np.array(obs[0][0], dtype=np.float64)
        assert np.array_equal(obs[0][0], rail)
        rec["state"].append(s)
        rec["agents_state"].append(np.stack([obs[h][1] for h in range(A)]))
        rec["targets"].append(np.stack([obs[h][2] for h in range(A)]))

    assert np.array_equal(np.stack([cg.agent_snapshot(env)[k] for k in util.STATE_NAMES], axis=1), fixture_state(fx, 0))
    if 0 in steps:
        record(0, obs)
    for t in range(1, max(steps) + 1):
        a = actions[t - 1]
        obs, _, dones, _ = env.step({i: int(a[i]) for i in range(A) if a[i] != cg.ABSENT})
        s = np.stack([cg.agent_snapshot(env)[k] for k in util.STATE_NAMES], axis=1)
        assert np.array_equal(s, fixture_state(fx, t)), f"{name}: the agent state after step {t} is not the fixture's"
        if t in steps:
            record(t, obs)
    out = dict(steps=np.array(steps, dtype=np.int32), rail=rail, **{k: np.stack(v) for k, v in rec.items()})
    for k in ("agents_state", "targets"):
        assert out[k].dtype == np.float64
    path = os.path.join(gold_dir, "global_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(f"global_{name}: {env.height}x{env.width} A={A} steps {steps} -> {os.path.getsize(path) / 1024:.0f} KB")
    return path


def check(names):
    tmp = tempfile.mkdtemp(prefix="global_check_")
    problems = []
    try:
        for name in names:
            new = np.load(capture(name, tmp))
            old_path = os.path.join(util.GOLD, "global_%s.npz" % name)
            if not os.path.exists(old_path):
                problems.append(f"global_{name}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                if k not in new.files or k not in old.files:
                    problems.append(f"global_{name}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"global_{name}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", nargs="*", default=None, metavar="FIXTURE")
    args = ap.parse_args()
    if args.check is not None:
        bad = check(args.check or list(RECIPES))
        for line in bad:
            print("MISMATCH", line)
        print("global-obs golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for name in (args.only or RECIPES):
        capture(name, util.GOLD)
