#!/usr/bin/env python3
"""Golden vectors of flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) from the REAL reference on CONSTRUCTED
agent states (tests/handmaps.py, GLOBAL_STATES): trains that share a cell, such a stack on a DONE agent's target or on the start cell of
waiting agents, many off-map agents on one start cell, the corner cells -- what the recorded episodes of tools/capture_global_obs.py do not
reach.  The reference RailEnv is built on the hand-made map as capture_handmaps.py does; for every state the fields get() reads (state,
position, direction, the malfunction counter; target, initial_position and speed once) are set on its agents and get_many() is recorded ->
tests/golden/global_states_<map>.npz:
  state i32[S][A][12] (the agent rows, util.STATE_NAMES order), rail f64[H][W][16] (one array for every handle and state),
  agents_state f64[S][A][H][W][5], targets f64[S][A][H][W][2].
CPU only; data, no reference source.

Adding a state: append its rows to the map's list in tests/handmaps.py (or add a map to GLOBAL_STATES there), run this script where the
reference lies, and name what the state is for in tests/test_global_obs_states.py::test_the_fixtures_hold_the_states_they_exist_for.

Usage:  python oracle/refharness/capture_global_states.py [MAP ...]
        python oracle/refharness/capture_global_states.py --check [MAP ...]   re-capture into a temporary directory, compare bit for bit
"""
import argparse
import os
import shutil
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import capture_handmaps as ch  # noqa: E402  (sets up sys.path for the reference)
from flatland.envs.observations import GlobalObsForRailEnv  # noqa: E402
from flatland.envs.step_utils.speed_counter import SpeedCounter  # noqa: E402
from flatland.envs.step_utils.states import TrainState  # noqa: E402
from tests import handmaps  # noqa: E402

cg = ch.cg


def capture(name, gold_dir):
    m, states = handmaps.GLOBAL_STATES[name]()
    H, W = m["grid"].shape
    assert H <= 12 and W <= 12 and len(m["init_dir"]) <= 8
    env, _ = ch.make_env(m, seed=23)
    A = env.get_num_agents()
    for i, a in enumerate(env.agents):
        a.speed_counter = SpeedCounter(speed=float(m["speed"][i]))
    builder = GlobalObsForRailEnv()
    builder.set_env(env)
    builder.reset()
    rec = {"agents_state": [], "targets": []}
    rail = None
    for rows in states:
        for i, a in enumerate(env.agents):
            r, c, d, kind, malf = (int(v) for v in rows[i, 0:5])
            a.position = None if r < 0 else (r, c)
            a.direction = d
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                a.state_machine.set_state(TrainState(kind))
            a.malfunction_handler._malfunction_down_counter = malf
        obs = builder.get_many(list(range(A)))
        # the rows written are the rows the reference's agents now show
        snap = cg.agent_snapshot(env)
        for k, col in (("row", 0), ("col", 1), ("dir", 2), ("state", 3), ("malf", 4)):
            assert np.array_equal(snap[k], rows[:, col]), k
        assert all(obs[h][0] is obs[0][0] for h in range(A)), "rail_obs is one array for every handle"
        if rail is None:
            rail = np.array(obs[0][0], dtype=np.float64)
        assert np.array_equal(obs[0][0], rail)
        rec["agents_state"].append(np.stack([obs[h][1] for h in range(A)]))
        rec["targets"].append(np.stack([obs[h][2] for h in range(A)]))
    out = dict(state=np.asarray(states, dtype=np.int32), rail=rail, **{k: np.stack(v) for k, v in rec.items()})
    for k in ("agents_state", "targets"):
        assert out[k].dtype == np.float64
    path = os.path.join(gold_dir, "global_states_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(f"global_states_{name}: {H}x{W} A={A} states {len(states)} -> {os.path.getsize(path) / 1024:.1f} KB")
    return path


def check(names):
    tmp = tempfile.mkdtemp(prefix="global_states_check_")
    problems = []
    try:
        for name in names:
            new = np.load(capture(name, tmp))
            old_path = os.path.join(cg.GOLD, "global_states_%s.npz" % name)
            if not os.path.exists(old_path):
                problems.append(f"global_states_{name}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                if k not in new.files or k not in old.files:
                    problems.append(f"global_states_{name}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"global_states_{name}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("maps", nargs="*")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    names = args.maps or list(handmaps.GLOBAL_STATES)
    if args.check:
        bad = check(names)
        for line in bad:
            print("MISMATCH", line)
        print("global-states golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for name in names:
        capture(name, cg.GOLD)
