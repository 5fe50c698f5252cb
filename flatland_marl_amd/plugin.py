"""Observation builders that plug into ANY env object through the reference's own plugin API
(`ObservationBuilder.set_env / reset / get_many / get`, flatland/core/env_observation_builder.py:18-73):

    env = flatland.envs.rail_env.RailEnv(..., obs_builder_object=flatland_marl_amd.plugin.TreeObsForRailEnv(31, 500))

`TreeObsForRailEnv(max_nodes, max_pred_depth)` replaces the pybind11 class `flatland_cutils.TreeObsForRailEnv`
(flatland_cutils/src/main.cpp:17-22), `TreeObsUpstream(max_depth, predictor)` replaces
`flatland.envs.observations.TreeObsForRailEnv` (observations.py:34-532), `ShortestPathPredictorForRailEnv(max_depth)` replaces the predictor of
flatland/envs/predictions.py:86-180 (get() -> {handle: [max_depth + 1, 5]}, env.dev_pred_dict, get_shortest_paths(); behind
`TreeObsUpstream` or behind the reference's own TreeObsForRailEnv(predictor=...)).  Like the reference module they keep whatever object
`set_env` hands them (treeobs.cpp:17-21 -- at that time a reference RailEnv has no rail yet, rail_env.py:178-179) and read it
again on every call, duck-typed:

  reset()      static read, as AgentsLoader::reset / RailLoader::reset do (loader.cpp:207-219, 329-333): `env.rail.grid`,
               `env._max_episode_steps`, the agents' line (initial position / direction, target, speed) and timetable ->
               fl_create / fl_load_env / fl_commit (distance maps and static tables are built on the GPU from the grid); a new
               DeadlockChecker, i.e. all sticky flags cleared (loader.cpp:186-199), then one AgentsLoader::update
               (treeobs.cpp:22-28) when some agent is on the map;
  get_many()   dynamic read, as Agent::Agent does per call (loader.cpp:8-120): position, direction, state, the malfunction
               handler, the speed counter, arrival time, old position / direction, `state_machine.st_signals.in_malfunction`,
               `env._elapsed_steps` -> fl_set_state (the builder's own sticky deadlock flags of the previous call carried
               forward, deadlock_checker.cpp:11-29) -> fl_obs_cutils / fl_obs_tree -> the reference's return shapes.

Everything is computed by the HIP kernels through the C-ABI; there is no CPU path (BatchedRailEnv raises without a GPU).
The env's own `distance_map` is not read: the reference's is the BFS of `env.rail.grid` towards the agents' targets
(distance_map.py:57-160), which is what the GPU builds; `verify_distance_map=True` compares the two at reset().
`handles`: `RailEnv` always passes every handle (rail_env.py:665).  With a strict subset the flatland_cutils builder of the reference
keeps only the listed agents' predictions, indexed by list position (treeobs.cpp:50-62): reproduced (fl_obs_cutils_handles;
goldens from the reference in tests/golden/subset_cfg2.npz); lists for which the reference's behaviour is undefined -- a handle >=
len(handles), tool.h:428-434 -- raise ValueError.  The upstream builder does the same since round 6 (fl_obs_tree_handles: observations.py:72-83,
337-366; a handle >= len(handles) is the reference's IndexError).

Cost of a call (tools/plugin_latency.py, profiles/r05_plugin_latency.json): the per-call host work is the reference's own -- one
pass over the agents' attributes -- and nothing that grows with the map: the grid is read and hashed at reset() only, the per-call
check of the static side compares the agents' line / timetable arrays.  `get_many(handles, as_arrays=True)` returns the numpy
arrays themselves instead of the nested lists the pybind11 casters of the reference build.
"""
from . import rail_env as _re
from .rail_env import TreeObsForRailEnv, GlobalObsForRailEnv, ShortestPathPredictorForRailEnv, _EnvBinding  # noqa: F401

# The builders themselves are rail_env's: one class per kind, for this library's RailEnv (read in place on the device) and for any
# other env object (mirrored through _EnvBinding).  Here are the names with the reference's constructor arguments.


class TreeObsUpstream(_re.TreeObsUpstream):
    """`flatland.envs.observations.TreeObsForRailEnv(max_depth, predictor)` for any env object: {handle: Node} with nested
    `childs` dicts (observations.py:117-254, 464-494).  predictor: anything with `max_depth` (the shortest-path predictor,
    predictions.py:91-180, is part of the kernel) or None (no conflict prediction, observations.py:72)."""

    def __init__(self, max_depth, predictor=None, *, device=0, verify_distance_map=False):
        super().__init__(max_depth, -1 if predictor is None else int(predictor.max_depth), predictor, device=device,
                         verify_distance_map=verify_distance_map)
