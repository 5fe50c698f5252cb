#!/usr/bin/env python3
"""Golden vectors on HAND-MADE rails (tests/handmaps.py): a ring of track, a loop entered at a trailing switch, two components, a diamond
crossing, a mesh with BFS levels wider than a wavefront -- what the sparse rail generator never draws.  Every grid goes through the REAL
reference (rail_from_grid_transition_map takes any 16-bit grid); after reset() the agents get the start cells, directions and targets of the
map's builder, the distance map and the observation builders are reset, and a forward-biased action stream is replayed.  Stored per step, as
capture_threeway.py does: the agents' state, reward and done, the upstream depth-2 / depth-3 trees (predictor depth 30), the flatland_cutils
tensors or the fact that it raised (and its first message); plus the distance map per unique target.  mesh33: static arrays and distance map.
The oval and the disconnected rail are also compared with the reference's own make_oval_rail / make_disconnected_simple_rail.
Build-container only; data, no reference source."""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import capture_golden as cg  # noqa: E402  (sets up sys.path for the reference)
from flatland.core.grid.rail_env_grid import RailEnvTransitions  # noqa: E402
from flatland.core.transition_map import GridTransitionMap  # noqa: E402
from flatland.envs.line_generators import sparse_line_generator  # noqa: E402
from flatland.envs.malfunction_generators import MalfunctionParameters, ParamMalfunctionGen  # noqa: E402
from flatland.envs.rail_env import RailEnv  # noqa: E402
from flatland.envs.rail_generators import rail_from_grid_transition_map  # noqa: E402
from flatland.utils import simple_rail  # noqa: E402
from flatland_marl_amd import synth  # noqa: E402
from tests import handmaps  # noqa: E402

PRED = 30
CUTILS_KEYS = ("attr", "forest", "adjacency", "node_order", "edge_order", "valid", "p_dist_target", "p_deadlocked", "p_ready")


def make_env(m, seed):
    grid = np.array(m["grid"], dtype=np.uint16)
    H, W = grid.shape
    A = len(m["init_dir"])
    rail = GridTransitionMap(width=W, height=H, transitions=RailEnvTransitions())
    rail.grid = grid.copy()
    # the line generator wants two "cities" with a station each: the first two agents' start cells (every agent is placed anew below)
    stations = [tuple(int(v) for v in m["init_pos"][k]) for k in (0, 1)]
    hints = {"city_positions": stations, "train_stations": [[(stations[0], 0)], [(stations[1], 0)]],
             "city_orientations": [int(m["init_dir"][0]), int(m["init_dir"][1])]}
    mp = MalfunctionParameters(malfunction_rate=0.0, min_duration=0, max_duration=0)
    env = RailEnv(width=W, height=H, rail_generator=rail_from_grid_transition_map(rail, {"agents_hints": hints}),
                  line_generator=sparse_line_generator(), number_of_agents=A, malfunction_generator=ParamMalfunctionGen(mp),
                  obs_builder_object=cg.PyTreeObs(max_depth=2, predictor=cg.ShortestPathPredictorForRailEnv(PRED)), random_seed=seed)
    with contextlib.redirect_stdout(io.StringIO()):
        env.reset()
    assert np.array_equal(np.asarray(env.rail.grid), grid)
    for i, a in enumerate(env.agents):
        a.initial_position = tuple(int(v) for v in m["init_pos"][i])
        a.initial_direction = a.direction = int(m["init_dir"][i])
        a.target = tuple(int(v) for v in m["target"][i])
        a.earliest_departure = int(m["earliest"][i])      # (the timetable was drawn for the line generator's agents)
        a.latest_arrival = int(m["earliest"][i]) + 30
        assert a.position is None
    env.distance_map.reset(env.agents, env.rail)      # the distance maps of the new targets (recomputed at the next get())
    return env, mp


def capture(name, steps, seed=23):
    m = handmaps.MAPS[name]()
    env, mp = make_env(m, seed)
    env._max_episode_steps = max(int(env._max_episode_steps), steps + 20)      # the episode survives the run
    out = cg.static_arrays(env, mp)
    out.update(cg.dm_unique(env))
    for k in ("grid", "init_pos", "init_dir", "target", "earliest"):
        assert np.array_equal(out[k], m[k]), k
    path = os.path.join(cg.GOLD, "handmap_" + name + ".npz")
    if steps == 0:
        np.savez_compressed(path, **out)
        print("handmap_" + name, "static, targets", len(out["dm_targets"]), "->", os.path.getsize(path) // 1024, "KB")
        return
    builders = {2: cg.PyTreeObs(max_depth=2, predictor=cg.ShortestPathPredictorForRailEnv(PRED)),
                3: cg.PyTreeObs(max_depth=3, predictor=cg.ShortestPathPredictorForRailEnv(PRED))}
    for b in builders.values():
        b.set_env(env)
        b.reset()
    cut = cg.TreeCutils(31, 500)
    cut.set_env(env)
    cut.reset()
    A = env.get_num_agents()
    rec = {k: [] for k in ("state", "py_d2_p%d" % PRED, "py_d3_p%d" % PRED, "cutils_raised", "actions", "reward", "done")}
    cut_rec = {k: [] for k in CUTILS_KEYS}
    msgs = []

    def observe():
        with contextlib.redirect_stdout(io.StringIO()):
            rec["py_d2_p%d" % PRED].append(cg.pytree_arrays(builders[2], env, 2))
            rec["py_d3_p%d" % PRED].append(cg.pytree_arrays(builders[3], env, 3))
        arrs = None
        try:
            attr, (nodes, adj, node_order, edge_order) = cut.get_many(list(range(A)))
            _, props, valid = cut.get_properties()
            arrs = dict(attr=np.array(attr, dtype=np.float32), forest=np.array(nodes, dtype=np.float32), adjacency=np.array(adj, dtype=np.int32),
                        node_order=np.array(node_order, dtype=np.int32), edge_order=np.array(edge_order, dtype=np.int32),
                        valid=np.array(valid, dtype=np.uint8), p_dist_target=np.array(props["dist_target"], dtype=np.float64),
                        p_deadlocked=np.array(props["deadlocked"], dtype=np.float64), p_ready=np.array(props["ready_not_depart"], dtype=np.float64))
        except ValueError as e:
            msgs.append(str(e))
        rec["cutils_raised"].append(int(arrs is None))
        for k in CUTILS_KEYS:
            cut_rec[k].append(None if arrs is None else arrs[k])
        s = cg.agent_snapshot(env)
        rec["state"].append(np.stack([s[k] for k in ("row", "col", "dir", "state", "malf", "nmalf", "scount", "saved", "arrival",
                                                      "old_row", "old_col", "old_dir")], axis=1).astype(np.int32))

    observe()
    for t in range(steps):
        acts = synth.forward_biased_actions(seed, 0, t, A)
        with contextlib.redirect_stdout(io.StringIO()):
            _, rew, dones, _ = env.step({i: int(a) for i, a in enumerate(acts)})
        rec["actions"].append(acts.astype(np.uint8))
        rec["reward"].append(np.array([rew[i] for i in range(A)], dtype=np.int32))
        rec["done"].append(np.array([dones[i] for i in range(A)], dtype=np.uint8))
        observe()
        if dones["__all__"]:
            break
    for k, v in rec.items():
        out[k] = np.stack(v)
    for k, v in cut_rec.items():      # (a step at which flatland_cutils raised would hold zeros; it raised on none of these maps)
        proto = next(x for x in v if x is not None)
        out["o_" + k] = np.stack([x if x is not None else np.zeros_like(proto) for x in v])
    out["cutils_message"] = np.array(msgs[0] if msgs else "")
    np.savez_compressed(path, **out)
    on_map = int((out["state"][:, :, 0] >= 0).any(axis=0).sum())
    print("  cells visited per agent", [len({tuple(p) for p in out["state"][:, i, 0:2].tolist()}) for i in range(A)],
          "deadlocked at the end", out["o_p_deadlocked"][-1].tolist())
    print("handmap_" + name, "steps", len(rec["actions"]), "agents on the map at some step", on_map, "of", A, "arrived", int((out["state"][-1][:, 3] == 6).sum()),
          "cutils raised at", int(np.sum(out["cutils_raised"])), "of", len(out["cutils_raised"]), "|", str(out["cutils_message"])[:80],
          "->", os.path.getsize(path) // 1024, "KB")


def check_reference_maps():
    """the two maps the reference ships are the builders' grids, cell for cell"""
    for ref, own in ((simple_rail.make_oval_rail, handmaps.oval), (simple_rail.make_disconnected_simple_rail, handmaps.disconnected)):
        _, rail_map, _ = ref()
        assert np.array_equal(np.asarray(rail_map, dtype=np.uint16), own()["grid"]), ref.__name__


if __name__ == "__main__":
    check_reference_maps()
    capture("oval", 50)
    capture("lasso", 60)
    capture("disconnected", 50)
    capture("crossing_u1", 40)
    capture("crossing_u5", 50)
    capture("mesh12", 30)
    capture("mesh33", 0)
