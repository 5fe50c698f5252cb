#!/usr/bin/env python3
"""Golden vectors of the two tree observation builders from the REAL reference on CONSTRUCTED agent states (tests/obs_state_cases.py): the
per-cell feature block of a branch walk (observations.py:295-374, treeobs.cpp:329-476) at the branches the recorded episodes reach with no
discriminating data.  The reference RailEnv is built on the hand-made map as capture_step_states.py does, anew for every case; every field
the builders and the predictor read is set on its agents (position, direction, state, the malfunction counter and count, SpeedCounter(speed),
old position and direction, arrival time, earliest and latest, target, initial position) and on the env (_elapsed_steps, _max_episode_steps);
then the reference's own flatland.envs.observations.TreeObsForRailEnv (depths 2 and 3, ShortestPathPredictorForRailEnv of the depths the
case names) and the unmodified flatland_cutils.TreeObsForRailEnv (31 nodes, the predictor depths the case names) are called ->
tests/golden/obs_states_<map>_<set>_<k>.npz (obs_state_cases.parts_of splits a set: every file stays below the largest step fixture), per case NAME (a control is the case NAME~k):
  NAME/state i32[A][12] (util.STATE_NAMES order), NAME/aux i32[A][4],
  NAME/py_d2_pP f64[A][21][12], NAME/py_d3_pP f64[A][85][12] (the dense trees as capture_golden.pytree_arrays flattens them),
  NAME/pred_pos_pP i32[P + 1][A], NAME/pred_dir_pP i32[P + 1][A] (the upstream builder's own predicted_pos / predicted_dir after get_many),
  NAME/cu_pP_<key> for the seven flatland_cutils tensors and the three properties (obs_state_cases.CUTILS_KEYS)
and `names`, the cases in order, `grid` u16[H][W], the reference env's rail.  CPU only; data, no reference source.

Usage:  python oracle/refharness/capture_obs_states.py [MAP_SET ...]              (yard_small, yard_crowd, crossing_small, crossing_crowd)
        python oracle/refharness/capture_obs_states.py --check [MAP_SET ...]      re-capture into a temporary directory, compare bit for bit
        python oracle/refharness/capture_obs_states.py --pins [MAP_SET ...]       for every pin, the nodes at which the reference's value of
                                                                                  the pin's column differs between case and control
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
from flatland.core.grid.rail_env_grid import RailEnvTransitions  # noqa: E402
from flatland.envs.step_utils.speed_counter import SpeedCounter  # noqa: E402
from flatland.envs.step_utils.states import TrainState  # noqa: E402
from tests import obs_state_cases as oc  # noqa: E402

cg = ch.cg
SNAP = ("row", "col", "dir", "state", "malf", "nmalf", "scount", "saved", "arrival", "old_row", "old_col", "old_dir")
LARGEST_STEP_FIXTURE = "step_states_yard.npz"


def check_maps():
    """every cell of a map used here is a transition word RailEnvTransitions.is_valid accepts (flatland_cutils then knows the road type of
    every cell: the attribute rows are defined everywhere), and the size limits of a case"""
    rt = RailEnvTransitions()
    for (name, set_name) in oc.SETS:
        grid = oc.MAPS[name]()["grid"]
        H, W = grid.shape
        assert H <= 12 and W <= 12 and len(oc.AGENTS[name][set_name]) <= 24, name
        for g in grid.ravel():
            assert rt.is_valid(int(g)), (name, hex(int(g)))


def snapshot(env):
    s = cg.agent_snapshot(env)
    return np.stack([s[k] for k in SNAP], axis=1).astype(np.int32)


def make_env(case):
    st = oc.static_of(case["map"], case["set"], case["variant"])
    m = dict(grid=st["grid"], init_pos=st["init_pos"], init_dir=st["init_dir"], target=st["target"], earliest=st["earliest"])
    env, _ = ch.make_env(m, seed=23)
    env._max_episode_steps = int(st["T"])
    env._elapsed_steps = 0
    for i, a in enumerate(env.agents):
        a.latest_arrival = int(st["latest"][i])
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
        a.action_saver.saved_action = None
        a.arrival_time = None if arrival < 0 else arrival
        a.old_position = None if orow < 0 else (orow, ocol)
        a.old_direction = None if odir < 0 else odir
        env.dones[i] = bool(case["aux"][i][3])
        assert tuple(a.target) == tuple(st["target"][i]) and tuple(a.initial_position) == tuple(st["init_pos"][i])
    env.dones["__all__"] = False
    assert np.array_equal(snapshot(env), case["state"]), case["name"]      # the rows written are the rows the reference's agents now show
    return env


def reference_obs(case):
    """what the reference's two builders return for the case's state: name -> array"""
    env = make_env(case)
    A = env.get_num_agents()
    out = {"state": case["state"], "aux": case["aux"], "grid": np.asarray(env.rail.grid, dtype=np.uint16)}
    with contextlib.redirect_stdout(io.StringIO()):
        for P in case["py_pred"]:
            for depth in (2, 3):
                b = cg.PyTreeObs(max_depth=depth, predictor=cg.ShortestPathPredictorForRailEnv(P))
                b.set_env(env)
                b.reset()
                out["py_d%d_p%d" % (depth, P)] = cg.pytree_arrays(b, env, depth)
            # the builder's own attributes after get_many: where it believes everybody is at every time of the horizon
            assert b.max_prediction_depth == P + 1 and all(len(b.predicted_pos[t]) == A for t in range(P + 1))
            out["pred_pos_p%d" % P] = np.array([b.predicted_pos[t] for t in range(P + 1)], dtype=np.int32)
            out["pred_dir_p%d" % P] = np.array([b.predicted_dir[t] for t in range(P + 1)], dtype=np.int32)
        env.distance_map.get()
        for P in case["cu_pred"]:
            cut = cg.TreeCutils(31, P)      # a fresh builder: nothing it keeps (deadlocks) is carried from case to case
            cut.set_env(env)
            cut.reset()
            env.obs_builder = cut
            obs = cut.get_many(list(range(A)))
            for k, v in cg.cutils_arrays(obs, env).items():
                out["cu_p%d_%s" % (P, k)] = v
    assert np.array_equal(snapshot(env), case["state"]), case["name"]      # (the builders changed nothing)
    return out


def capture(map_name, set_name, gold_dir):
    """one file per part of the set (obs_state_cases.parts_of): each below the size of the largest step fixture"""
    paths = []
    limit = os.path.getsize(os.path.join(cg.GOLD, LARGEST_STEP_FIXTURE))
    for name, part in zip(oc.fixture_files(map_name, set_name), oc.parts_of(map_name, set_name)):
        cases = [oc.BY_NAME[n] for n in part]
        out = {"names": np.array(part)}
        for c in cases:
            ref = reference_obs(c)
            out["grid"] = ref.pop("grid")      # (the reference env's own rail: one map per file)
            for k, v in ref.items():
                out[c["name"] + "/" + k] = v
        path = os.path.join(gold_dir, name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < limit, "%s: %d bytes, the largest step fixture has %d" % (path, os.path.getsize(path), limit)
        print(f"{name}: {len(cases)} cases ({sum(c['control_of'] is not None for c in cases)} controls), {len(out)} arrays -> {os.path.getsize(path) / 1024:.1f} KB")
        paths.append(path)
    return paths


def check(sets):
    tmp = tempfile.mkdtemp(prefix="obs_states_check_")
    problems, n = [], 0
    try:
        for (m, s) in sets:
            for path in capture(m, s, tmp):
                name = os.path.basename(path)[:-4]
                new = np.load(path)
                old_path = os.path.join(cg.GOLD, name + ".npz")
                if not os.path.exists(old_path):
                    problems.append(f"{name}: no committed fixture")
                    continue
                old = np.load(old_path)
                for k in sorted(set(new.files) | set(old.files)):
                    n += 1
                    if k not in new.files or k not in old.files:
                        problems.append(f"{name}: key {k} only on one side")
                    elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                        problems.append(f"{name}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems, n


def show_pins(sets):
    """for every pin: the nodes of the pin's agent at which the reference's value of the row's column differs between case and control"""
    by_name = {c["name"]: c for c in oc.CASES}
    for c in oc.CASES:
        if (c["map"], c["set"]) not in sets or not c["pins"]:
            continue
        ref = {c["name"]: reference_obs(c)}
        for p in c["pins"]:
            if p["control_name"] not in ref:
                ref[p["control_name"]] = reference_obs(by_name[p["control_name"]])
            key = oc.pin_key(p)
            if oc.TABLE[p["row"]]["kind"] in ("never", "reoriented"):      # (a property of the whole tree: the node is chosen by hand)
                continue
            a, b = ref[c["name"]][key][p["agent"]], ref[p["control_name"]][key][p["agent"]]
            col = oc.COL[oc.TABLE[p["row"]]["col"]]
            nodes = [int(n) for n in np.flatnonzero(a[:, col] != b[:, col])]
            print("    (%r, %r, %r, %r, %d): %s,      # %s" % (c["name"], p["row"], p["builder"], p["param"], p["agent"], nodes[0] if nodes else None,
                                                              ", ".join("node %d: %s vs %s" % (n, a[n, col], b[n, col]) for n in nodes)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sets", nargs="*")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--pins", action="store_true")
    args = ap.parse_args()
    check_maps()
    sets = [s for s in oc.SETS if not args.sets or "%s_%s" % s in args.sets]
    assert sets and len(sets) == (len(args.sets) or len(oc.SETS)), args.sets
    if args.pins:
        show_pins(sets)
        sys.exit(0)
    if args.check:
        bad, n = check(sets)
        for line in bad:
            print("MISMATCH", line)
        print("obs-states golden check: %d arrays," % n, "all identical" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for (m, s) in sets:
        capture(m, s, cg.GOLD)
