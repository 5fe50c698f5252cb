#!/usr/bin/env python3
"""Golden vectors of RailEnv.step() (rail_env.py:501-634) from the REAL reference on CONSTRUCTED states (tests/step_state_cases.py): what
one agent does in one step -- action preprocessing, the action saver, the speed counter, the state machine, placement, arrival, the end of
the episode -- at the branches the recorded episodes reach rarely or never.  The reference RailEnv is built on the hand-made map as
capture_handmaps.py does, anew for every case; every field step() reads is set on its agents (position, direction, state and previous state, the
malfunction counter and count, SpeedCounter(speed) and its counter, the saved action, old position and direction, arrival time, earliest and
latest, target) and on the env (_elapsed_steps, _max_episode_steps, dones, the malfunction generator's parameters, np_random's state); the
real step() is called for the case's actions (a case with `filter` drops the agents without action_required first, as
eval_env.parse_actions does) -> tests/golden/step_states_<map>.npz, per case NAME:
  NAME/state i32[K][A][12] (util.STATE_NAMES order, after each step), NAME/aux i32[K][A][4] (previous state, in_malfunction signal, 0, done),
  NAME/reward i32[K][A], NAME/done u8[K][A], NAME/done_all u8[K], NAME/raised u8[K], NAME/elapsed i32[K], NAME/mt_key_id i32[K] (a row of
  `mt_keys` u32[U][624], the distinct MT19937 keys of the file), NAME/mt_pos i32[K], NAME/log i32[K][A][13]: state before, state after, the preprocessed action and movement_allowed as handed to
  generate_state_transition_signals, the seven st_signals it returned, num_broken_steps of the agent's draw, dropped by parse_actions.
and `names`, the cases in order.  CPU only; data, no reference source.

Usage:  python oracle/refharness/capture_step_states.py [MAP ...]
        python oracle/refharness/capture_step_states.py --check [MAP ...]   re-capture into a temporary directory, compare bit for bit
"""
import argparse
import contextlib
import io
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
from flatland.core.env_observation_builder import DummyObservationBuilder  # noqa: E402
from flatland.core.grid.rail_env_grid import RailEnvTransitions  # noqa: E402
from flatland.envs.malfunction_generators import MalfunctionParameters, ParamMalfunctionGen  # noqa: E402
from flatland.envs.rail_env_action import RailEnvActions  # noqa: E402
from flatland.envs.step_utils.speed_counter import SpeedCounter  # noqa: E402
from flatland.envs.step_utils.states import TrainState  # noqa: E402
from tests import handmaps, step_state_cases as sc  # noqa: E402

cg = ch.cg
SNAP = ("row", "col", "dir", "state", "malf", "nmalf", "scount", "saved", "arrival", "old_row", "old_col", "old_dir")


def check_maps():
    """check_reference_maps compares the two maps the reference ships with their builders, which says nothing about a map drawn here: for the
    maps of STEP_MAPS (the yard is new) the check is per cell -- every cell is a transition word RailEnvTransitions.is_valid accepts -- and
    the size limits of a case"""
    ch.check_reference_maps()
    rt = RailEnvTransitions()
    for name, build in handmaps.STEP_MAPS.items():
        m = build()
        H, W = m["grid"].shape
        assert H <= 12 and W <= 12 and len(m["init_dir"]) <= 8, name
        for g in m["grid"].ravel():
            assert rt.is_valid(int(g)), (name, hex(int(g)))


def snapshot(env):
    s = cg.agent_snapshot(env)
    return np.stack([s[k] for k in SNAP], axis=1).astype(np.int32)


def make_env(map_name, variant):
    m = handmaps.STEP_MAPS[map_name]()
    st = sc.static_of(map_name, variant)
    env, _ = ch.make_env(dict(m, target=st["target"]), seed=23)
    env.obs_builder = DummyObservationBuilder()
    env.obs_builder.set_env(env)
    env.malfunction_generator = ParamMalfunctionGen(MalfunctionParameters(malfunction_rate=float(st["malf_rate"]), min_duration=int(st["malf_min"]),
                                                                           max_duration=int(st["malf_max"])))
    env._max_episode_steps = int(st["T"])
    for i, a in enumerate(env.agents):
        a.earliest_departure = int(st["earliest"][i])
        a.latest_arrival = int(st["latest"][i])
        assert tuple(a.target) == tuple(st["target"][i])
    return env, st


def run_case(env, st, case):
    A = env.get_num_agents()
    key, pos = sc.rng_of(*case["rng"])
    env.np_random.set_state(("MT19937", key, int(pos), 0, 0.0))
    for i, a in enumerate(env.agents):
        r, c, d, kind, malf, nmalf, scount, saved, arrival, orow, ocol, odir = (int(v) for v in case["state"][i])
        a.position = None if r < 0 else (r, c)
        a.direction = d
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a.state_machine.set_state(TrainState(kind))
        prev = int(case["aux"][i][0])
        a.state_machine.previous_state = None if prev < 0 else TrainState(prev)
        a.state_machine.st_signals.in_malfunction = bool(case["aux"][i][1])
        a.malfunction_handler._malfunction_down_counter = malf
        a.malfunction_handler.num_malfunctions = nmalf
        a.speed_counter = SpeedCounter(speed=float(st["speed"][i]))
        a.speed_counter.counter = scount
        a.action_saver.saved_action = None if saved == 0 else RailEnvActions(saved)
        a.arrival_time = None if arrival < 0 else arrival
        a.old_position = None if orow < 0 else (orow, ocol)
        a.old_direction = None if odir < 0 else odir
        env.dones[i] = bool(case["aux"][i][3])
    env.dones["__all__"] = bool(case["done_all"])
    env._elapsed_steps = int(case["elapsed"])
    assert np.array_equal(snapshot(env), case["state"]), case["name"]      # the rows written are the rows the reference's agents now show

    # what the step hands to and gets from generate_state_transition_signals, and what the generator draws: wrappers around the
    # reference's own bound methods
    seen, draws = {}, []
    signals_of = env.generate_state_transition_signals
    generate = env.malfunction_generator.generate

    def spy_signals(agent, preprocessed_action, movement_allowed):
        s = signals_of(agent, preprocessed_action, movement_allowed)
        seen[agent.handle] = (int(agent.state), int(preprocessed_action), int(bool(movement_allowed)),
                              [int(bool(getattr(s, n))) for n in sc.SIGNALS])
        return s

    def spy_generate(np_random):
        mf = generate(np_random)
        draws.append(int(mf.num_broken_steps))
        return mf

    env.generate_state_transition_signals = spy_signals
    env.malfunction_generator.generate = spy_generate
    rec = {k: [] for k in ("state", "aux", "reward", "done", "done_all", "raised", "elapsed", "mt_key", "mt_pos", "log")}
    try:
        for acts in case["actions"]:
            seen.clear()
            del draws[:]
            before = snapshot(env)
            required = [bool(env.action_required(a)) for a in env.agents]
            dropped = [int(case["filter"] and int(acts[i]) != sc.ABSENT and not required[i]) for i in range(A)]
            d = {i: int(acts[i]) for i in range(A) if int(acts[i]) != sc.ABSENT and not dropped[i]}
            raised, rew = 0, {i: 0 for i in range(A)}
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    _, rew, _, _ = env.step(d)
            except Exception as e:
                assert str(e) == "Episode is done, cannot call step()", (case["name"], repr(e))
                raised = 1
            after = snapshot(env)
            log = np.zeros((A, 13), dtype=np.int32)
            for i in range(A):
                if raised:
                    log[i, 0:2] = before[i, 3]
                else:
                    s0, pa, mv, sig = seen[i]
                    log[i] = [s0, after[i, 3], pa, mv] + sig + [draws[i], dropped[i]]
            prev = [a.state_machine.previous_state for a in env.agents]
            rec["state"].append(after)
            rec["aux"].append(np.array([[-1 if prev[i] is None else int(prev[i]), int(bool(a.state_machine.st_signals.in_malfunction)), 0,
                                         int(bool(env.dones[i]))] for i, a in enumerate(env.agents)], dtype=np.int32))
            rec["reward"].append(np.array([rew[i] for i in range(A)], dtype=np.int32))
            rec["done"].append(np.array([env.dones[i] for i in range(A)], dtype=np.uint8))
            rec["done_all"].append(np.uint8(env.dones["__all__"]))
            rec["raised"].append(np.uint8(raised))
            rec["elapsed"].append(np.int32(env._elapsed_steps))
            rs = env.np_random.get_state()
            assert rs[3] == 0
            rec["mt_key"].append(np.asarray(rs[1], dtype=np.uint32))
            rec["mt_pos"].append(np.int32(rs[2]))
            rec["log"].append(log)
    finally:
        del env.generate_state_transition_signals      # (the instance attributes: the class's methods are back)
        del env.malfunction_generator.generate
    return {k: np.stack(v) for k, v in rec.items()}


def capture(map_name, gold_dir):
    cases = [c for c in sc.CASES if c["map"] == map_name]
    out = {"names": np.array([c["name"] for c in cases])}
    variants, keys = set(), {}
    for c in cases:
        env, st = make_env(map_name, c["variant"])      # a fresh RailEnv per case: nothing step() keeps is carried from case to case
        variants.add(c["variant"])
        for k, v in run_case(env, st, c).items():
            if k == "mt_key":
                k, v = "mt_key_id", np.array([keys.setdefault(row.tobytes(), len(keys)) for row in v], dtype=np.int32)
            out[c["name"] + "/" + k] = v
    out["mt_keys"] = np.stack([np.frombuffer(b, dtype=np.uint32) for b in keys])      # (in the order of their ids)
    path = os.path.join(gold_dir, "step_states_%s.npz" % map_name)
    np.savez_compressed(path, **out)
    steps = sum(len(c["actions"]) for c in cases)
    print(f"step_states_{map_name}: {len(cases)} cases, {steps} steps, variants {sorted(variants)} -> {os.path.getsize(path) / 1024:.1f} KB")
    return path


def check(names):
    tmp = tempfile.mkdtemp(prefix="step_states_check_")
    problems = []
    try:
        for name in names:
            new = np.load(capture(name, tmp))
            old_path = os.path.join(cg.GOLD, "step_states_%s.npz" % name)
            if not os.path.exists(old_path):
                problems.append(f"step_states_{name}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                if k not in new.files or k not in old.files:
                    problems.append(f"step_states_{name}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"step_states_{name}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("maps", nargs="*")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    check_maps()
    names = args.maps or list(handmaps.STEP_MAPS)
    if args.check:
        bad = check(names)
        for line in bad:
            print("MISMATCH", line)
        print("step-states golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for name in names:
        capture(name, cg.GOLD)
