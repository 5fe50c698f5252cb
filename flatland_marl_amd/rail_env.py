"""Dict-shaped facade over the batched HIP env for B = 1: keeps the API surface of the reference's
`flatland.envs.rail_env.RailEnv` (reset()/step(), rail_env.py:260-357, 501-634), of the
`ObservationBuilder` plugin interface (core/env_observation_builder.py:18-73), of the native module
`flatland_cutils.TreeObsForRailEnv` (flatland_cutils/src/main.cpp:17-22) and of the caller
`LocalTestEnvWrapper` (solution/eval_env.py:97-114), so solution/plfActor.py consumes it unchanged.

Everything of step() / the observations is computed by the HIP kernels through the C-ABI; this file only reshapes tensors
into the reference's dicts / lists.  reset(regenerate_rail=True, regenerate_schedule=True) runs the native host generators
(flatland_marl_amd/generators.py -> csrc/gen) on the env's MT19937 stream; an env can also be created from the static
description a reference env has after reset() (RailEnv.from_static, flatland_marl_amd.from_reference_env).
"""
import collections
import time
from enum import IntEnum

import numpy as np

from . import generators
from .hip_backend import BatchedRailEnv, EpisodeDoneError, FlatlandHipError
from .reference_bridge import static_of_env, agents_static_of_env, dynamic_state_of_env, AGENT_STATIC_KEYS

# flatland.envs.malfunction_generators.MalfunctionParameters / ParamMalfunctionGen (malfunction_generators.py:19-53)
MalfunctionParameters = collections.namedtuple("MalfunctionParameters", ["malfunction_rate", "min_duration", "max_duration"])


class ParamMalfunctionGen:
    def __init__(self, parameters):
        self.MFP = parameters


class NoMalfunctionGen(ParamMalfunctionGen):
    def __init__(self):
        super().__init__(MalfunctionParameters(0.0, 0, 0))


class TrainState(IntEnum):  # flatland/envs/step_utils/states.py:5-25
    WAITING = 0
    READY_TO_DEPART = 1
    MALFUNCTION_OFF_MAP = 2
    MOVING = 3
    STOPPED = 4
    MALFUNCTION = 5
    DONE = 6

    def is_malfunction_state(self):
        return self in (TrainState.MALFUNCTION, TrainState.MALFUNCTION_OFF_MAP)

    def is_off_map_state(self):
        return self in (TrainState.WAITING, TrainState.READY_TO_DEPART, TrainState.MALFUNCTION_OFF_MAP)

    def is_on_map_state(self):
        return self in (TrainState.MOVING, TrainState.STOPPED, TrainState.MALFUNCTION)


class RailEnvActions(IntEnum):  # flatland/envs/rail_env_action.py:5-27
    DO_NOTHING = 0
    MOVE_LEFT = 1
    MOVE_FORWARD = 2
    MOVE_RIGHT = 3
    STOP_MOVING = 4


class _SpeedCounter:  # step_utils/speed_counter.py:4-53 (read-only view)
    def __init__(self, speed):
        self.speed = float(speed)
        self.max_count = int(1 / self.speed) - 1
        self.counter = 0

    @property
    def is_cell_entry(self):
        return self.counter == 0

    @property
    def is_cell_exit(self):
        return self.counter == self.max_count


class _MalfunctionHandler:  # step_utils/malfunction_handler.py:10-67 (read-only view)
    def __init__(self):
        self.malfunction_down_counter = 0
        self.num_malfunctions = 0

    @property
    def in_malfunction(self):
        return self.malfunction_down_counter > 0

    @property
    def malfunction_counter_complete(self):
        return self.malfunction_down_counter == 0


class _ActionSaver:  # step_utils/action_saver.py:4-36 (read-only view)
    def __init__(self):
        self.saved_action = None

    @property
    def is_action_saved(self):
        return self.saved_action is not None


class EnvAgent:
    """read-only mirror of flatland.envs.agent_utils.EnvAgent (agent_utils.py:57-88), refreshed after every step."""

    def __init__(self, handle, st):
        self.handle = handle
        self.initial_position = tuple(int(v) for v in st["init_pos"][handle])
        self.initial_direction = int(st["init_dir"][handle])
        self.target = tuple(int(v) for v in st["target"][handle])
        self.earliest_departure = int(st["earliest"][handle])
        self.latest_arrival = int(st["latest"][handle])
        self.speed_counter = _SpeedCounter(st["speed"][handle])
        self.malfunction_handler = _MalfunctionHandler()
        self.action_saver = _ActionSaver()
        self.position = None
        self.direction = self.initial_direction
        self.old_position = None
        self.old_direction = None
        self.arrival_time = None
        self.state = TrainState.WAITING
        self.moving = False

    def _refresh(self, row):
        r, c, d, s, malf, nmalf, scount, saved, arrival, orow, ocol, odir = (int(v) for v in row)
        self.position = None if r < 0 else (r, c)
        self.direction = d
        self.state = TrainState(s)
        self.malfunction_handler.malfunction_down_counter = malf
        self.malfunction_handler.num_malfunctions = nmalf
        self.speed_counter.counter = scount
        self.action_saver.saved_action = None if saved == 0 else RailEnvActions(saved)
        self.arrival_time = None if arrival < 0 else arrival
        self.old_position = None if orow < 0 else (orow, ocol)
        self.old_direction = None if odir < 0 else odir


class _Rail:
    def __init__(self, grid):
        self.grid = np.array(grid, dtype=np.uint16)
        self.height, self.width = self.grid.shape


def distance_map_of(batch, b=0):
    """DistanceMap.get() (flatland/envs/distance_map.py:27-45) of env b of a batch: float64 [A, H, W, 4], inf = unreachable -- the
    device keeps one u16 map per unique target (0xFFFF = unreachable) and every agent's target slot"""
    dm, slot = batch.distance_map(b)
    full = dm[slot].astype(np.float64)
    full[dm[slot] == 0xFFFF] = np.inf
    return full


class _DistanceMap:
    """env.distance_map of this library's RailEnv: get() computed once per map"""

    def __init__(self, env):
        self._env = env
        self._cache = None

    def get(self):
        if self._cache is None:
            self._cache = distance_map_of(self._env._batch)
        return self._cache


class ObservationBuilder:
    """core/env_observation_builder.py:18-73"""

    def __init__(self):
        self.env = None

    def set_env(self, env):
        self.env = env

    def reset(self):
        pass

    def get_many(self, handles=None):
        raise NotImplementedError

    def get(self, handle=0):
        """ONE agent's observation (core/env_observation_builder.py:56-73); the builders compute whole batches, so this is
        get_many([handle]) unpacked"""
        return self.get_many([handle])[handle]


def cutils_handle_list(handles, n_agents):
    """get_many(handles) of flatland_cutils: None for "every agent in order" (the usual call, rail_env.py:665), else the list for
    fl_obs_cutils_handles -- a strict subset makes the reference's conflict test work on list POSITIONS (treeobs.cpp:50-62, 393-465),
    which is only defined when the list is a permutation of 0 .. n-1 (tool.h:428-434 erases position `handle`)."""
    h = [int(x) for x in handles]
    if h == list(range(n_agents)) or not h:     # ([]: the reference's `assert((!handles.empty(), "Input Error"))` is a comma expression that never
        return None                             # fires, treeobs.cpp:33 -- it returns every agent's attribute rows and an empty forest)
    if sorted(h) != list(range(len(h))):
        raise ValueError("get_many(handles=%r): the reference's behaviour is undefined for this list -- its conflict test erases list position "
                         "`handle` (flatland_cutils tool.h:428-434), so a strict subset has to be a permutation of 0 .. len(handles)-1" % (h,))
    return h


def upstream_handle_list(handles, n_agents, has_predictor=True):
    """get_many(handles) of the upstream builder: None for "every agent in order" (or no predictor: no conflict test, the list does not
    matter), else the list for fl_obs_tree_handles -- predicted_pos / predicted_dir hold the listed handles' predictions in list order
    (observations.py:72-83) and the conflict test deletes list position `handle` (np.delete, :337): a handle >= len(handles) is an IndexError
    in the reference, raised here too; lists with repeated handles are not reproduced (ValueError)."""
    h = [int(x) for x in handles]
    if not has_predictor or h == list(range(n_agents)):
        return None
    if h and max(h) >= len(h):
        raise IndexError("index %d is out of bounds for axis 0 with size %d (get_many(handles=%r): the reference's conflict test deletes list "
                         "position `handle`, observations.py:337)" % (max(h), len(h), h))
    if not h or sorted(h) != list(range(len(h))):
        raise ValueError("get_many(handles=%r): lists with repeated handles are not reproduced" % (h,))
    return h


# ---- where a builder's B = 1 batch comes from and how it is kept current: this library's own RailEnv (_OwnBatch) or any other env
# object (_EnvBinding).  The builders below hold everything else once.
class _Source:
    computes_at_reset = False     # True: the cutils builder's reset() runs one AgentsLoader::update itself (treeobs.cpp:22-28)
    profile = None                # a dict: seconds per stage of the calls, accumulated (tools/plugin_latency.py)
    dead = None                   # the DeadlockChecker's sticky flags as of the last call (deadlock_checker.cpp:3-9)

    def clock(self):
        return time.perf_counter() if self.profile is not None else 0.0

    def lap(self, key, t0, sync=False):
        """profiling only: seconds since t0 into stage `key` (sync: after the handle's stream has drained)"""
        if self.profile is None:
            return t0
        if sync:
            self.batch.sync()
        t1 = time.perf_counter()
        self.profile[key] = self.profile.get(key, 0.0) + (t1 - t0)
        return t1


class _OwnBatch(_Source):
    """this library's own RailEnv: the env's device-resident batch IS the state, nothing is read or pushed per call (the sticky
    deadlock flags live in it too)"""

    def __init__(self, env):
        self.env = env

    @property
    def batch(self):
        return self.env._batch        # (a new object with every map the env adopts)

    def configure(self, max_nodes, pred_depth):
        b = self.batch
        if b is not None:             # (before the env's first reset() there is nothing to configure yet: reset() binds again)
            b.max_nodes, b.pred_depth = max_nodes, pred_depth
            b._obs = None

    def load_static(self, env, max_nodes=31, pred_depth=500):
        pass

    def current(self, env, what):
        return self.batch

    def pred_depth(self, builder):
        return builder.pred_depth

    def properties(self, env):
        cfg = {"curr_step": env._elapsed_steps, "n_agents": env.get_num_agents(), "max_timesteps": env._max_episode_steps,
               "height": env.height, "width": env.width}
        return (cfg, [a.earliest_departure for a in env.agents], [a.latest_arrival for a in env.agents],
                [a.speed_counter.speed for a in env.agents])


def _agents_signature(st):
    return tuple(np.asarray(st[k]).tobytes() for k in AGENT_STATIC_KEYS)


def _static_signature(st):
    g = np.asarray(st["grid"])
    return (g.shape, g.tobytes()) + _agents_signature(st)


class _EnvBinding(_Source):
    """a caller-owned env mirrored into a B = 1 batch on the device: the static side is read at reset() (load_static), the agents'
    dynamic state before every launch (push_dynamic), duck-typed -- see flatland_marl_amd/plugin.py"""
    make_batch = BatchedRailEnv          # (tests of the host-side extraction substitute a recorder: there is no CPU compute path)
    computes_at_reset = True

    def __init__(self, device, verify_distance_map):
        self.device = device
        self.verify = verify_distance_map
        self.batch = None
        self.sig = None
        self.static = None
        self.dead = None
        self.elapsed = 0
        self.agents_sig = None    # the agents' line / timetable as of the last static read (compared on every call)
        self.profile = None

    def configure(self, max_nodes, pred_depth):
        pass                      # (set_env reads nothing, treeobs.cpp:17-21 -- a reference RailEnv has no rail yet: load_static does it)

    def load_static(self, env, max_nodes=31, pred_depth=500):
        st = static_of_env(env)
        sig = _static_signature(st)
        if sig != self.sig:
            H, W = st["grid"].shape
            b = self.batch
            if b is not None and (b.H, b.W, b.A) == (H, W, len(st["init_dir"])):
                try:
                    b.replace_env(0, st)          # same shape: into the live handle (fl_load_env + fl_commit)
                except FlatlandHipError as e:
                    if e.code != 6:               # FL_ERR_CAPACITY: more rail cells / targets than the first map -> new handle
                        raise
                    b = None
            else:
                b = None
            if b is None:
                if self.batch is not None:
                    self.batch.close()
                b = self.make_batch([st], device=self.device, max_nodes=max_nodes, pred_depth=pred_depth)
            self.batch, self.sig, self.static = b, sig, st
            if self.verify:
                self.verify_distance_map(env)
        self.agents_sig = _agents_signature(st)
        if self.batch.max_nodes != max_nodes:
            self.batch._obs = None
        self.batch.max_nodes, self.batch.pred_depth = max_nodes, pred_depth
        self.dead = np.zeros(self.batch.A, dtype=np.int32)
        return st

    def verify_distance_map(self, env):
        ours = distance_map_of(self.batch)
        theirs = np.asarray(env.distance_map.get(), dtype=np.float64)
        if theirs.shape != ours.shape or not np.array_equal(ours, theirs):
            raise ValueError("env.distance_map is not the distance map of env.rail.grid towards the agents' targets "
                             "(distance_map.py:57-160): a caller-supplied distance map is not supported")

    def push_dynamic(self, env):
        """Agent::Agent for every agent (loader.cpp:8-120); the line and timetable are re-read too, like the reference does on
        every call (loader.cpp:19-73), and a change of them reloads the static side.  The rail is the reference's RailLoader: read
        at reset() only (loader.cpp:329-333) -- nothing here is proportional to the map."""
        t0 = self.clock()
        if _agents_signature(agents_static_of_env(env)) != self.agents_sig:
            dead = self.dead
            self.load_static(env, self.batch.max_nodes, self.batch.pred_depth)
            if dead is not None and len(dead) == len(self.dead):
                self.dead = dead                 # the checker object lives until reset() (loader.cpp:186-199)
        state, aux, elapsed = dynamic_state_of_env(env)
        aux[:, 2] = self.dead
        self.elapsed = elapsed
        t0 = self.lap("extract_python", t0)
        self.batch.set_state(state[None], aux[None], np.array([elapsed], dtype=np.int32))
        self.lap("fl_set_state", t0)

    def current(self, env, what):
        if self.batch is None:
            raise RuntimeError("%s before reset()" % what)
        self.push_dynamic(env)
        return self.batch

    def pred_depth(self, builder):
        """the predictor is the caller's object too: read again at every call"""
        return builder.pred_depth if builder.predictor is None else int(builder.predictor.max_depth)

    def properties(self, env):
        st = self.static
        H, W = st["grid"].shape
        cfg = {"curr_step": int(self.elapsed), "n_agents": len(st["init_dir"]), "max_timesteps": int(st["T"]),
               "height": int(getattr(env, "height", H)), "width": int(getattr(env, "width", W))}
        return cfg, st["earliest"], st["latest"], st["speed"]


class _DeviceObs(ObservationBuilder):
    """what the three builders share: the binding for a caller-owned env, and the choice of the source when the env is set"""
    checks_errors = True          # (RailEnv.step leaves the one synchronising error check of a step to the builder)

    def __init__(self, device=0, verify_distance_map=False):
        super().__init__()
        self._bind = _EnvBinding(device, verify_distance_map)
        self._src = self._bind

    def set_env(self, env):
        self.env = env
        self._src = _OwnBatch(env) if isinstance(env, RailEnv) else self._bind


class TreeObsForRailEnv(_DeviceObs):
    """Drop-in for flatland_cutils.TreeObsForRailEnv(max_nodes, max_pred_depth) (treeobs.h:133-169), for any env object."""

    def __init__(self, max_nodes=31, max_pred_depth=500, *, device=0, verify_distance_map=False):
        super().__init__(device, verify_distance_map)
        self.max_nodes, self.max_pred_depth = int(max_nodes), int(max_pred_depth)
        self._last = None

    def set_env(self, env):                      # treeobs.cpp:17-21: keeps the object
        super().set_env(env)
        self._src.configure(self.max_nodes, self.max_pred_depth)

    def reset(self):                             # treeobs.cpp:22-28
        self._src.load_static(self.env, self.max_nodes, self.max_pred_depth)
        if self._src.computes_at_reset:
            self._compute()                      # the checker sees the state at reset, and get_properties() is valid straight after it

    def _compute(self, handles=None):
        s = self._src
        b = s.current(self.env, "TreeObsForRailEnv.get_many()")
        t0 = s.clock()
        # a strict subset: the reference's conflict test then sees the listed agents' predictions only, by list position
        # (treeobs.cpp:50-62) -- fl_obs_cutils_handles; lists the reference has no defined behaviour for raise ValueError
        o = b.obs_cutils(None if handles is None else cutils_handle_list(handles, b.A))
        b.check()                                # (synchronises: the kernel has run)
        t0 = s.lap("kernel", t0)
        self._last = {k: v[0].cpu().numpy() for k, v in o.items()}
        s.dead = self._last["props"][:, 1].astype(np.int32)
        s.lap("read_back", t0)
        return self._last

    def get_many(self, handles, as_arrays=False):
        """-> (agent_attr [A][83], (nodes [n][N][12], adjacency [n][N-1][3], node_order [n][N], edge_order [n][N-1])) as nested
        lists, what the pybind11 STL casters return (treeobs.h:160-161, treeobs.cpp:30-108); as_arrays=True: the same five as
        numpy arrays (float32 / int32), without the conversion to Python lists."""
        h = list(handles)
        L = self._compute(h)
        # the attribute rows of ALL agents (feature_parser.cpp:100-118), the trees of the listed ones in list order (treeobs.cpp:93-101)
        trees = tuple(L[k][h] for k in ("forest", "adjacency", "node_order", "edge_order"))
        if as_arrays:
            return L["agent_attr"], trees
        t0 = self._src.clock()
        out = (L["agent_attr"].tolist(), tuple(a.tolist() for a in trees))
        self._src.lap("tolist", t0)
        return out

    def get(self, handle=0):
        """ONE agent's observation as RailEnv would see it: its row of get_many(every handle) (the pybind11 class has no get();
        get_many([handle]) alone would be the reference's strict-subset semantics, see cutils_handle_list)"""
        attr, (nodes, adj, node_order, edge_order) = self.get_many(range(self.env.get_num_agents()))
        return attr[handle], (nodes[handle], adj[handle], node_order[handle], edge_order[handle])

    def get_properties(self):
        """treeobs.cpp:612-640: the values of the last get_many() / reset()"""
        L = self._last
        if L is None:
            raise RuntimeError("TreeObsForRailEnv.get_properties() before get_many()")
        cfg, earliest, latest, speed = self._src.properties(self.env)
        props = {"dist_target": L["props"][:, 0].tolist(), "deadlocked": L["props"][:, 1].tolist(),
                 "ready_not_depart": L["props"][:, 2].tolist(),
                 "earliest_departure": [float(v) for v in earliest],
                 "latest_arrival": [float(v) for v in latest],
                 "speed": [float(np.float32(v)) for v in speed]}
        return cfg, props, L["valid_actions"].astype(bool).tolist()

    def last_arrays(self):
        """the tensors of the last call, for callers that want arrays instead of nested lists"""
        return self._last


NODE_FIELDS = ("dist_own_target_encountered", "dist_other_target_encountered", "dist_other_agent_encountered",
               "dist_potential_conflict", "dist_unusable_switch", "dist_to_next_branch", "dist_min_to_target",
               "num_agents_same_direction", "num_agents_opposite_direction", "num_agents_malfunctioning",
               "speed_min_fractional", "num_agents_ready_to_depart")
# flatland.envs.observations.Node (observations.py:20-32): the 12 features + the `childs` dict
Node = collections.namedtuple("Node", NODE_FIELDS + ("childs",))


def nodes_from_dense(arr, max_depth):
    """the nested Node namedtuples TreeObsForRailEnv.get() returns (observations.py:117-254, 464-494) from one agent's dense
    [N(max_depth), 12] array in DFS pre-order (node, L, F, R, B): a missing child is -inf (:247, :489), the nodes of the last
    level have an empty `childs` dict (:491-492)."""
    sz = [(4 ** (max_depth - d + 1) - 1) // 3 for d in range(max_depth + 2)]   # rows of a subtree rooted at depth d

    def build(idx, depth):
        childs = {}
        if depth < max_depth:
            for k, ch in enumerate("LFRB"):
                c = idx + 1 + k * sz[depth + 1]
                childs[ch] = build(c, depth + 1) if arr[c, 0] != -np.inf else -np.inf
        return Node(*(float(v) for v in arr[idx]), childs)
    return build(0, 0)


def dense_from_nodes(node, max_depth):
    """inverse of nodes_from_dense (what the golden fixtures store): [N(max_depth), 12], -inf rows for missing subtrees"""
    rows = []

    def walk(n, depth):
        if not isinstance(n, tuple):
            rows.extend([[-np.inf] * 12] * ((4 ** (max_depth - depth + 1) - 1) // 3))
            return
        rows.append([getattr(n, f) for f in NODE_FIELDS])
        if depth < max_depth:
            for ch in "LFRB":
                walk(n.childs.get(ch, -np.inf), depth + 1)
    walk(node, 0)
    return np.array(rows, dtype=np.float64)


class TreeObsUpstream(_DeviceObs):
    """flatland.envs.observations.TreeObsForRailEnv(max_depth, ShortestPathPredictorForRailEnv(pred_depth))
    (observations.py:34-532), for any env object.  get_many() returns what the reference returns: {handle: Node}, nested namedtuples
    with a `childs` dict ('L', 'F', 'R', 'B' -> Node or -inf).  get_many_dense() / the batched tensor API keep the dense form the
    kernel writes: float64 [N(max_depth), 12] per agent in DFS pre-order (node, L, F, R, B), missing subtree = -inf.
    predictor: anything with `max_depth` (the shortest-path predictor, predictions.py:91-180, is part of the kernel); without one the
    conflict prediction runs pred_depth deep, pred_depth < 0: not at all (observations.py:72)."""

    FIELDS = NODE_FIELDS
    tree_explored_actions_char = ["L", "F", "R", "B"]     # observations.py:41

    def __init__(self, max_depth=2, pred_depth=30, predictor=None, *, device=0, verify_distance_map=False):
        super().__init__(device, verify_distance_map)
        self.max_depth = int(max_depth)
        self.predictor = predictor
        self.pred_depth = pred_depth if predictor is None else getattr(predictor, "max_depth", pred_depth)
        self.observation_dim = 11                         # observations.py:46

    def set_env(self, env):                      # observations.py:524-527
        super().set_env(env)
        if self.predictor is not None and hasattr(self.predictor, "set_env"):
            self.predictor.set_env(env)

    def reset(self):                             # observations.py:57-58: the targets' lookup = the static side
        self._src.load_static(self.env)

    def get_many_dense(self, handles=None):
        """{handle: float64 [N(max_depth), 12]}; the dense form is this library's own: None = every agent"""
        s = self._src
        b = s.current(self.env, "TreeObsForRailEnv.get_many()")
        pred = s.pred_depth(self)
        hs = list(range(b.A)) if handles is None else list(handles)
        # a handle list: the reference's semantics (the listed agents' predictions only, by list position: observations.py:72-83, 337-366)
        t = b.obs_tree(self.max_depth, pred, upstream_handle_list(hs, b.A, pred >= 0) if hs else None)
        b.check()
        arr = t[0].cpu().numpy()
        return {h: arr[h] for h in hs}

    def get_many(self, handles=None):
        if handles is None:
            return {}                 # observations.py:66-67: None -> no handles, no observations
        return {h: nodes_from_dense(a, self.max_depth) for h, a in self.get_many_dense(handles).items()}

    def get(self, handle=0):
        """observations.py:117-254 computes ONE agent's tree against the predictions the last get_many() prepared -- RailEnv's call with
        every handle (rail_env.py:665): the agent's node of get_many(every handle), not get_many([handle]) (a one-entry prediction list)"""
        return self.get_many(list(range(len(self.env.agents))))[handle]


class GlobalObsForRailEnv(_DeviceObs):
    """flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611), for any env object: get_many(handles) -> {handle:
    (rail_obs [H,W,16], agents_state [H,W,5], targets [H,W,2])}, float64 numpy; rail_obs is ONE array for every handle, built at
    reset() (:560-566).  Computed by the GPU (fl_obs_global) for every agent in one launch; get_many(None) is {} as in the reference."""

    def __init__(self, *, device=0, verify_distance_map=False):
        super().__init__(device, verify_distance_map)
        self.rail_obs = None

    def reset(self):
        self._src.load_static(self.env)
        b = self._src.batch
        r, _, _ = b.obs_global(rail=True)
        b.check()
        self.rail_obs = r[0].cpu().numpy()

    def get_many(self, handles=None):
        if handles is None:
            return {}                 # core/env_observation_builder.py:52-55: no handles, no observations
        b = self._src.current(self.env, "GlobalObsForRailEnv.get_many()")
        handles = list(handles)
        if not handles:
            return {}
        _, ast, tgt = b.obs_global(rail=False)
        b.check()
        ast, tgt = ast[0].cpu().numpy(), tgt[0].cpu().numpy()
        return {h: (self.rail_obs, ast[h], tgt[h]) for h in handles}


Waypoint = collections.namedtuple("Waypoint", ["position", "direction"])      # rail_trainrun_data_structures.py: ((row, col), direction)


class OrderedSet(dict):
    """what the reference keeps in env.dev_pred_dict (flatland/utils/ordered_set.py): a set that iterates in insertion order"""

    def __init__(self, items=()):
        super().__init__((x, None) for x in items)

    def add(self, x):
        self[x] = None

    def __repr__(self):
        return "OrderedSet(%r)" % (list(self),)


class ShortestPathPredictorForRailEnv:
    """flatland.envs.predictions.ShortestPathPredictorForRailEnv(max_depth) (predictions.py:86-180), for any env object: get() ->
    {handle: float64 [max_depth + 1, 5]} with the rows (time, row, col, direction, action), computed by the GPU for every agent in
    one launch (fl_predict).  Like the reference get() tests `if handle:` -- get(0) and get(None) return every agent, get(3) agent 3
    alone -- and leaves env.dev_pred_dict[handle], the ordered set of the (row, col, direction) visited (:158-177).
    get_shortest_paths(max_depth) is rail_env_shortest_paths.get_shortest_paths(env.distance_map, max_depth) (:203-274).
    The reference's TreeObsForRailEnv never calls predictor.reset() (observations.py:57-58): with a caller-owned env the static side
    is read at the first get() after set_env() (and again after a reset() of an env that counts its resets); reset() reads it again."""

    def __init__(self, max_depth=20, *, device=0, verify_distance_map=False):
        self.max_depth = max_depth
        self.env = None
        self._bind = _EnvBinding(device, verify_distance_map)
        self._src = self._bind
        self._loaded = None        # the env's num_resets when the static side was read (True: an env without that counter)

    def set_env(self, env):
        self.env = env
        self._src = _OwnBatch(env) if isinstance(env, RailEnv) else self._bind
        self._loaded = None

    def _resets(self):
        n = getattr(self.env, "num_resets", None)
        return True if n is None else n

    def reset(self):
        self._src.load_static(self.env)
        self._loaded = self._resets()

    def _batch(self, what):
        if self._loaded is None or self._loaded != self._resets():
            self.reset()
        b = self._src.current(self.env, what)
        if b is None:
            raise RuntimeError("%s before the env's reset()" % what)
        return b

    def get(self, handle=None):
        b = self._batch("ShortestPathPredictorForRailEnv.get()")
        pred = b.predictions(int(self.max_depth))
        b.check()
        arr = pred[0].cpu().numpy()
        handles = [handle] if handle else range(b.A)          # predictions.py:121-123: `if handle:`
        dev = getattr(self.env, "dev_pred_dict", None)
        if dev is None:
            try:
                self.env.dev_pred_dict = dev = {}
            except AttributeError:
                dev = None
        out = {}
        for h in handles:
            p = arr[h].copy()
            out[h] = p
            if dev is not None:
                own_dir = int(p[0, 3])                        # (a stop row is filed under agent.direction, :163)
                dev[h] = OrderedSet((int(r[1]), int(r[2]), own_dir if r[4] == RailEnvActions.STOP_MOVING else int(r[3])) for r in p[1:])
        return out

    def get_shortest_paths(self, max_depth=None):
        """{handle: [Waypoint((row, col), direction), ...] or None}: at most max_depth waypoints (default: the predictor's depth)"""
        b = self._batch("ShortestPathPredictorForRailEnv.get_shortest_paths()")
        _, wp, ln = b.predictions(int(self.max_depth if max_depth is None else max_depth), paths=True)
        b.check()
        wp, ln = wp[0].cpu().numpy(), ln[0].cpu().numpy()
        return {h: [Waypoint((int(r), int(c)), int(d)) for r, c, d in wp[h, :ln[h]]] if ln[h] else None for h in range(b.A)}


class _FromDescription:
    """what `env.rail_generator` / `env.line_generator` are on an env made from a description or a file (the reference:
    rail_from_file / line_from_file closures, rail_generators.py:116-145, line_generators.py:168-206): hands the env's own rail /
    line back"""

    def __init__(self, what):
        self.what = what

    def __repr__(self):
        return "<%s of the loaded description>" % self.what


class RailEnv:
    """B = 1 view with the reference's constructor, attribute and method surface (rail_env.py:35-777)."""

    def __init__(self, width, height, rail_generator=None, line_generator=None, number_of_agents=2, obs_builder_object=None,
                 malfunction_generator_and_process_data=None, malfunction_generator=None, remove_agents_at_target=True,
                 random_seed=None, record_steps=False, *, device=0):
        """Same arguments as flatland.envs.rail_env.RailEnv (rail_env.py:100-112).  rail_generator / line_generator:
        generators.sparse_rail_generator(...) / sparse_line_generator(...) (the Round-2 generators; others: build the env
        with the reference and use RailEnv.from_static).  Nothing is generated before reset(), like the reference."""
        if not remove_agents_at_target:
            raise NotImplementedError("remove_agents_at_target=False is unused by the solution and not supported")
        if malfunction_generator_and_process_data is not None:
            raise NotImplementedError("the deprecated malfunction closures are not supported; pass malfunction_generator")
        self.width, self.height = int(width), int(height)
        self.rail_generator = rail_generator if rail_generator is not None else generators.sparse_rail_generator()
        self.line_generator = line_generator if line_generator is not None else generators.sparse_line_generator()
        self.number_of_agents = int(number_of_agents)
        self.malfunction_generator = malfunction_generator if malfunction_generator is not None else NoMalfunctionGen()
        self.remove_agents_at_target = True
        self.record_steps = record_steps
        self._device = device
        self.obs_builder = obs_builder_object if obs_builder_object is not None else TreeObsForRailEnv()
        self.np_random = None
        self.random_seed = None
        if random_seed:
            self._seed(random_seed)
        self.num_resets = 0
        self._static, self._hints, self._batch = None, None, None
        self._from_static = self._from_file = False
        self.rail, self.agents, self.distance_map = None, [], None
        self._max_episode_steps = None
        self._elapsed_steps = 0
        self.dones = dict.fromkeys(list(range(self.number_of_agents)) + ["__all__"], False)
        self.rewards_dict = {}
        self.obs_dict = None

    @classmethod
    def from_static(cls, static, obs_builder_object=None, device=0, from_file=False):
        """an env from the static description a (reference) env has after reset(): no generators involved.
        from_file: the description comes from an env FILE (RailEnvPersister.load_new, persistence.py:105-129): reset() with
        regenerate_rail or regenerate_schedule then behaves like the reference's rail_from_file / line_from_file env -- the same
        rail and line, the timetable drawn again from the env's MT19937 stream (see generators.redraw_timetable)."""
        H, W = np.asarray(static["grid"]).shape
        mfp = MalfunctionParameters(float(static["malf_rate"]), int(static["malf_min"]), int(static["malf_max"]))
        env = cls(W, H, number_of_agents=len(static["init_dir"]), obs_builder_object=obs_builder_object,
                  malfunction_generator=ParamMalfunctionGen(mfp), device=device)
        # no generators to run: reset() re-adopts this same rail and line (solution/eval_env.py:102 calls env.reset() on such an env)
        env.rail_generator, env.line_generator = _FromDescription("rail"), _FromDescription("line")
        env._from_static = True
        env._from_file = bool(from_file)
        env._adopt(static)
        return env

    def _seed(self, seed):  # rail_env.py:210-222
        self.np_random = generators.np_random(seed)
        self.random_seed = seed
        return [seed]

    def _rng_state(self):
        """the env's MT19937 stream: on the device while a batch exists (the step's malfunction draws advance it there)"""
        if self._batch is not None:
            key, pos = self._batch.rng_state()
            return key[0], int(pos[0])
        if self.np_random is None:
            self.np_random = np.random.RandomState()     # unseeded env, like gym's seeding.np_random(None)
        st = self.np_random.get_state()
        return np.asarray(st[1], dtype=np.uint32), int(st[2])

    def _adopt(self, static):
        """(re)create the B = 1 batch for a new static description"""
        if self._batch is not None:
            self._batch.close()
        self._static = static
        self._batch = BatchedRailEnv([static], device=self._device)
        self.rail = _Rail(static["grid"])
        self.height, self.width = self.rail.height, self.rail.width
        self.number_of_agents = self._batch.A
        self._max_episode_steps = int(static["T"])
        self.agents = [EnvAgent(i, static) for i in range(self.number_of_agents)]
        self.distance_map = _DistanceMap(self)
        self.obs_builder.set_env(self)

    def get_num_agents(self):
        return len(self.agents)

    @property
    def agent_positions(self):
        """RailEnv.agent_positions (rail_env.py:341-342, 360-367): int [H, W], the handle of the agent on a cell, -1 = free"""
        return self._batch.positions_map(0)

    def get_agent_handles(self):
        return range(self.get_num_agents())

    def action_required(self, agent):  # rail_env.py:243-258
        return agent.state == TrainState.READY_TO_DEPART or \
            (agent.state.is_on_map_state() and agent.speed_counter.is_cell_entry)

    def _refresh(self):
        st, el = self._batch.state()
        for a, row in zip(self.agents, st[0]):
            a._refresh(row)
        self._elapsed_steps = int(el[0])

    def get_info_dict(self):  # rail_env.py:452-468
        return {"action_required": {i: self.action_required(a) for i, a in enumerate(self.agents)},
                "malfunction": {i: a.malfunction_handler.malfunction_down_counter for i, a in enumerate(self.agents)},
                "speed": {i: a.speed_counter.speed for i, a in enumerate(self.agents)},
                "state": {i: a.state for i, a in enumerate(self.agents)}}

    def _get_observations(self):  # rail_env.py:660-666
        self.obs_dict = self.obs_builder.get_many(list(range(self.get_num_agents())))
        return self.obs_dict

    def reset(self, regenerate_rail=True, regenerate_schedule=True, *, random_seed=None):
        """rail_env.py:260-357.  regenerate_rail: a new map, lines and timetable on the env's own MT19937 stream; neither flag:
        EnvAgent.reset() for every agent; regenerate_schedule alone fails like the reference does with the sparse generators."""
        if random_seed:
            self._seed(random_seed)
            if self._batch is not None:       # the device copy of the stream follows the re-seed
                st = self.np_random.get_state()
                self._batch.set_rng_state(np.asarray(st[1], dtype=np.uint32)[None], np.array([st[2]], dtype=np.int32))
        mfp = self.malfunction_generator.MFP
        if self._from_static and self._from_file and (regenerate_rail or regenerate_schedule):
            # an env loaded from a FILE (rail_from_file + line_from_file): the same rail and line come back, the agents are fresh
            # (EnvAgent.from_line, rail_env.py:315-317) and timetable_generator draws earliest_departure / latest_arrival /
            # max_episode_steps AGAIN from the env's stream, without agents_hints (rail_env.py:310-331)
            key, pos = self._rng_state()
            self._adopt(generators.redraw_timetable(self._static, key, pos, num_cities=2))
        elif self._from_static:
            # an env made from a description: the same map, lines and timetable again; regenerate_schedule makes fresh agents,
            # without it EnvAgent.reset() keeps arrival_time (agent_utils.py:90-105).  The MT19937 stream runs on.
            self._batch.reset(fresh=bool(regenerate_rail or regenerate_schedule))
        elif regenerate_rail or self._static is None:
            key, pos = self._rng_state()
            hints = {}
            static = generators.generate_env(self.width, self.height, self.number_of_agents, self.rail_generator, self.line_generator,
                                             key, pos, mfp.malfunction_rate, mfp.min_duration, mfp.max_duration, hints=hints)
            self._hints = hints
            self._adopt(static)
        elif regenerate_schedule:
            # the reference passes no hints to the line generator on this path and SparseLineGen fails on them
            # (rail_env.py:311-316, line_generators.py:96): same error here
            raise TypeError("'NoneType' object is not subscriptable")
        else:
            self._batch.reset(fresh=False)      # EnvAgent.reset() literally: arrival_time survives (agent_utils.py:90-105)
        self.num_resets += 1
        self.obs_builder.set_env(self)      # rail_env.py:305 (a builder assigned to env.obs_builder after construction is bound here)
        self.obs_builder.reset()
        self.dones = dict.fromkeys(list(range(self.number_of_agents)) + ["__all__"], False)
        self.rewards_dict = {i: 0 for i in range(self.number_of_agents)}
        self._refresh()
        return self._get_observations(), self.get_info_dict()

    def step(self, action_dict_):  # rail_env.py:501-634
        action_dict = action_dict_
        if self.dones["__all__"]:
            self._elapsed_steps += 1
            raise Exception("Episode is done, cannot call step()")
        acts = np.full((1, self.number_of_agents), 255, dtype=np.uint8)
        for i, a in action_dict.items():
            if 0 <= int(i) < self.number_of_agents:
                v = int(a)
                acts[0, int(i)] = v if 0 <= v <= 4 else 7   # illegal values become DO_NOTHING inside the kernel
        rew, done, done_all = self._batch.step(acts)
        try:
            if not getattr(self.obs_builder, "checks_errors", False):
                self._batch.check()
            obs = self._get_observations()      # the builders call fl_check themselves: one sync + read-back per step
        except EpisodeDoneError as e:
            raise Exception("Episode is done, cannot call step()") from e
        except FlatlandHipError as e:
            if e.code == 4:
                raise ValueError(str(e)) from e
            raise
        rew, done = rew[0].cpu().numpy(), done[0].cpu().numpy()
        self.rewards_dict = {i: int(rew[i]) for i in range(self.number_of_agents)}
        for i in range(self.number_of_agents):
            self.dones[i] = bool(done[i])
        self.dones["__all__"] = bool(done_all[0].item())
        self._refresh()
        self.obs_dict = obs
        return obs, self.rewards_dict, self.dones, self.get_info_dict()


# ---- flatland/contrib/wrappers/flatland_wrappers.py: the reduced action space most training code puts in front of RailEnv.
# The lists, the flags and the cell sets are computed on the device (fl_action_space, fl_decision_cells), one read-back per call;
# the wrappers' loops are the reference's host loops.  DeadlockWrapper is left out: see the shim module and DESIGN.md section 7.
def _batch_of(env):
    b = getattr(env, "_batch", None)      # (a wrapper hands the attribute of the env it wraps on)
    if b is None:
        raise RuntimeError("the env has no batch yet: reset() it first")
    return b


def possible_actions_sorted_by_distance(env, handle):
    """flatland_wrappers.py:14-56: the moves agent `handle` has, [(RailEnvActions, distance)] sorted by the distance map, of length 2
    (a single move is doubled) or 3; distance is a numpy float64, and the int 0 of [(DO_NOTHING, 0)] * 2 for an agent that is neither
    READY_TO_DEPART nor on the map.  The reference's prints are not reproduced."""
    b = _batch_of(env)
    act, dist, cnt = b.shortest_path_actions()
    b.check()
    row = b.torch.cat([act[0, handle].to(dist.dtype), dist[0, handle], cnt[0, handle:handle + 1].to(dist.dtype)]).cpu().numpy()
    n = int(row[6])
    state = env.agents[handle].state
    if state != TrainState.READY_TO_DEPART and not state.is_on_map_state():
        return [(RailEnvActions.DO_NOTHING, 0)] * 2
    return [(RailEnvActions(int(row[k])), np.float64(row[3 + k])) for k in range(n)]


def find_all_cells_where_agent_can_choose(env):
    """flatland_wrappers.py:145-176: (switches, switches_neighbors, decision_cells) as sets of (row, col).  Cells with rail only: the
    reference also lists the empty cell a malformed switch points at, where no agent can stand."""
    b = _batch_of(env)
    cells = b.decision_cells()[0].cpu().numpy()
    b.check()
    switches = {(int(r), int(c)) for r, c in zip(*np.nonzero(cells & 1))}
    neighbors = {(int(r), int(c)) for r, c in zip(*np.nonzero(cells & 2))}
    return switches, neighbors, switches | neighbors


class RailEnvWrapper:  # flatland_wrappers.py:59-119
    def __init__(self, env):
        self.env = env
        assert self.env is not None
        assert self.env.rail is not None, "Reset original environment first!"
        assert self.env.agents is not None, "Reset original environment first!"
        assert len(self.env.agents) > 0, "Reset original environment first!"

    def __getattr__(self, name):
        """Expose any other attributes of the underlying environment."""
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def rail(self):
        return self.env.rail

    @property
    def width(self):
        return self.env.width

    @property
    def height(self):
        return self.env.height

    @property
    def agent_positions(self):
        return self.env.agent_positions

    def get_num_agents(self):
        return self.env.get_num_agents()

    def get_agent_handles(self):
        return self.env.get_agent_handles()

    def step(self, action_dict):
        return self.env.step(action_dict)

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        return obs, info


class ShortestPathActionWrapper(RailEnvWrapper):  # flatland_wrappers.py:122-141
    def step(self, action_dict):
        """action_dict: {handle: 0 = do nothing, 1 = shortest path, 2 = second shortest path}; translated on the device
        (BatchedRailEnv.reduced_actions), one read-back.  An entry the agent's list does not have raises IndexError like the reference."""
        b = _batch_of(self.env)
        A = self.env.get_num_agents()
        reduced = np.full((1, A), 255, dtype=np.uint8)
        passed = {}      # (a handle outside the env, an action outside 0 .. 254: handed on as it came, the env deals with it)
        for h, a in action_dict.items():
            if 0 <= int(h) < A and 0 <= int(a) < 255:
                reduced[0, int(h)] = int(a)
            else:
                passed[h] = a
        acts = b.reduced_actions(reduced)
        cnt = b.shortest_path_actions()[2]
        b.check()
        both = b.torch.stack([acts[0], cnt[0]]).cpu().numpy()
        transformed = {}
        for h, a in action_dict.items():
            if h in passed:
                transformed[h] = a
            elif int(a) == 0:
                transformed[h] = a
            else:
                if int(a) - 1 >= int(both[1, int(h)]):
                    raise IndexError("list index out of range")
                transformed[h] = RailEnvActions(int(both[0, int(h)]))
        return self.env.step(transformed)


class SkipNoChoiceCellsWrapper(RailEnvWrapper):  # flatland_wrappers.py:179-258
    def __init__(self, env, accumulate_skipped_rewards, discounting):
        super().__init__(env)
        self.accumulate_skipped_rewards = accumulate_skipped_rewards
        self.discounting = discounting
        self.switches = None
        self.switches_neighbors = None
        self.decision_cells = None
        self.skipped_rewards = collections.defaultdict(list)
        self.reset_cells()

    def _flags(self):
        b = _batch_of(self.env)
        flags = b.on_decision_cell()[0].cpu().numpy()
        b.check()
        return flags

    def on_decision_cell(self, agent):
        return bool(self._flags()[agent.handle])

    def on_switch(self, agent):
        return agent.position in self.switches

    def next_to_switch(self, agent):
        return agent.position in self.switches_neighbors

    def reset_cells(self):
        self.switches, self.switches_neighbors, self.decision_cells = find_all_cells_where_agent_can_choose(self.env)

    def step(self, action_dict):
        """the reference's loop: the env is stepped -- with an EMPTY action dict from the second time on -- until an agent is done or on a
        decision cell; the skipped rewards are summed on the host in the reference's order (a reversed Horner scheme)"""
        o, r, d, i = {}, {}, {}, {}
        i["action_required"] = dict()
        i["malfunction"] = dict()
        i["speed"] = dict()
        i["state"] = dict()
        while len(o) == 0:
            obs, reward, done, info = self.env.step(action_dict)
            flags = self._flags()      # (one read-back for the agents of this step)
            for agent_id, agent_obs in obs.items():
                if done[agent_id] or flags[agent_id]:
                    o[agent_id] = agent_obs
                    r[agent_id] = reward[agent_id]
                    d[agent_id] = done[agent_id]
                    i["action_required"][agent_id] = info["action_required"][agent_id]
                    i["malfunction"][agent_id] = info["malfunction"][agent_id]
                    i["speed"][agent_id] = info["speed"][agent_id]
                    i["state"][agent_id] = info["state"][agent_id]
                    if self.accumulate_skipped_rewards:
                        discounted_skipped_reward = r[agent_id]
                        for skipped_reward in reversed(self.skipped_rewards[agent_id]):
                            discounted_skipped_reward = self.discounting * discounted_skipped_reward + skipped_reward
                        r[agent_id] = discounted_skipped_reward
                        self.skipped_rewards[agent_id] = []
                elif self.accumulate_skipped_rewards:
                    self.skipped_rewards[agent_id].append(reward[agent_id])
            d["__all__"] = done["__all__"]
            action_dict = {}
        return o, r, d, i

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        self.reset_cells()      # (the cells can change with the map)
        return obs, info


class LocalTestEnvWrapper:
    """Counterpart of solution/eval_env.py:9-114 (TestEnvWrapper / LocalTestEnvWrapper)."""

    def __init__(self, env):
        self.env = env
        self.obs_properties = {}

    def action_required(self):
        return {i: self.env.action_required(a) for i, a in enumerate(self.env.agents)}

    def parse_actions(self, actions):  # eval_env.py:33-39
        req = self.action_required()
        return {idx: act for idx, act in actions.items() if req[idx]}

    def update_obs_properties(self):  # eval_env.py:56-62
        cfg, props, valid = self.env.obs_builder.get_properties()
        self.obs_properties = {}
        self.obs_properties.update(cfg)
        self.obs_properties.update(props)
        self.obs_properties["valid_actions"] = valid

    @staticmethod
    def parse_features(feature, obs_properties):  # eval_env.py:64-79
        fl = {"agent_attr": np.array(feature[0]), "forest": np.array(feature[1][0])}
        fl["forest"][fl["forest"] == np.inf] = -1
        fl["adjacency"] = np.array(feature[1][1])
        fl["node_order"] = np.array(feature[1][2])
        fl["edge_order"] = np.array(feature[1][3])
        fl.update(obs_properties)
        return fl

    def get_valid_actions(self):
        return self.obs_properties["valid_actions"]

    def reset(self):
        feature, _ = self.env.reset()
        self.update_obs_properties()
        return [self.parse_features(feature, self.obs_properties)]

    def step(self, actions):
        actions = self.parse_actions(actions)
        feature, reward, done, info = self.env.step(actions)
        self.update_obs_properties()
        return [self.parse_features(feature, self.obs_properties)], reward, done

    def final_metric(self):  # eval_env.py:81-94 (counts every off-map, non-READY agent as "arrived")
        assert self.env.dones["__all__"]
        env = self.env
        n_arrival = sum(1 for a in env.agents if a.position is None and a.state != TrainState.READY_TO_DEPART)
        total_reward = sum(env.rewards_dict.values())
        norm_reward = 1 + total_reward / env._max_episode_steps / env.get_num_agents()
        return n_arrival / env.get_num_agents(), total_reward, norm_reward
