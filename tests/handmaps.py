"""Hand-made rail maps: the shapes the sparse rail generator never draws -- a ring of track, a loop that can only be entered at a trailing
switch, two components, a diamond crossing, and a mesh whose BFS levels are wider than a wavefront.  A helper module like
tests/tree_lstm_forests.py, not a test: own numpy code that imports nothing of the reference.  oracle/refharness/capture_handmaps.py runs the
real reference on these maps and writes tests/golden/handmap_<name>.npz; tests/test_handmaps.py (CPU) pins the builders to the fixtures'
grids and asserts that every fixture still reaches the path it exists for; tests/test_gpu_handmaps.py (GPU) replays them on the kernels.

A map is a dict: grid u16[H, W] in the repository's bit layout (bit (3 - d) * 4 + (3 - m): a train with orientation d may leave towards m;
N, E, S, W = 0 .. 3), init_pos i32[A, 2], init_dir i32[A], target i32[A, 2], earliest i32[A] (earliest departures).

  name          shape  what it is / what it reaches
  oval          6x9    a ring of 18 cells without a switch: every walk is a cycle that starts on itself (mu = 0, lam = 18), in both directions
                       of travel; the agents' own targets lie inside the loop
  lasso         8x9    the oval with one simple switch in its bottom side and a spur of three cells to a dead end.  Clockwise the ring FACES the
                       switch (SEG_SWITCH); counter-clockwise it TRAILS it: a cycle that holds an unusable switch; from the spur heading in, the
                       cycle is entered after mu > 0 steps; the dead end is unreachable from the counter-clockwise ring
  disconnected  7x10   two components: some agents' targets lie in the other one (0xFFFF at the agent's own state, next-hop 4, no predicted path)
  crossing_u1   9x9    two lines with dead ends meeting in a diamond crossing (0x8421) and a switch off the east arm; every agent has ONE target
  crossing_u5   9x9    the same rail, five targets (one more than the wavefronts of a distance-map workgroup), among them a dead end and the crossing
  mesh12        12x12  every cell allows left, forward and right wherever the neighbour is inside the grid: BFS levels of up to 90 states,
                       three ways on per direction
  mesh33        33x33  the same mesh: 4 356 states (more than the BFS ring holds), levels of up to 260 states

  yard          8x9    (STEP_MAPS, not in MAPS: no recorded episode) two lines joined by a stem that enters a symmetric switch from below and
                       leaves at a facing simple switch, four dead ends, a stub nobody reaches: the rail of tests/step_state_cases.py

full_grid(H, W) is the mesh on any H x W: rail on every cell, the border included.  GLOBAL_STATES (end of the file): constructed agent states
for GlobalObsForRailEnv on full5x7 and the crossing, captured by oracle/refharness/capture_global_states.py.

Adding a map: write a builder that returns such a dict, list it in MAPS, add its capture to oracle/refharness/capture_handmaps.py (run there,
where the reference lies), and add the condition the map exists for to tests/test_handmaps.py::test_each_fixture_reaches_the_path_it_exists_for.
"""
import numpy as np

N, E, S, W = 0, 1, 2, 3
DR, DC = (-1, 0, 1, 0), (0, 1, 0, -1)


def way(d, m):
    """the bit of: a train with orientation d may leave towards m"""
    return 1 << ((3 - d) * 4 + (3 - m))


def ways(*pairs):
    g = 0
    for d, m in pairs:
        g |= way(d, m)
    return g


def nibble(g, d):
    return (int(g) >> ((3 - d) * 4)) & 15


VERT = ways((N, N), (S, S))
HORZ = ways((E, E), (W, W))
# a dead end named by the side its track lies on: the train arrives from there and turns round
DEAD_S, DEAD_W, DEAD_N, DEAD_E = way(N, S), way(E, W), way(S, N), way(W, E)
# a curve named by the two sides it joins
CURVE_SE, CURVE_SW, CURVE_NW, CURVE_NE = ways((N, E), (W, S)), ways((E, S), (N, W)), ways((S, W), (E, N)), ways((W, N), (S, E))
DIAMOND = VERT | HORZ
assert DIAMOND == 0x8421


def _map(grid, agents, earliest=None):
    """earliest: the agents' earliest departures -- trains that would meet head-on on a single track leave one after the other"""
    a = np.array(agents, dtype=np.int32).reshape(-1, 5)
    grid = np.array(grid, dtype=np.uint16)
    for r, c, d, tr, tc in a:
        assert nibble(grid[r, c], d) != 0 and grid[tr, tc] != 0, (r, c, d, tr, tc)
    earliest = np.arange(len(a)) % 3 if earliest is None else earliest
    return dict(grid=grid, init_pos=a[:, 0:2].copy(), init_dir=a[:, 2].copy(), target=a[:, 3:5].copy(), earliest=np.array(earliest, dtype=np.int32))


def _oval_grid(H, Wd):
    g = np.zeros((H, Wd), dtype=np.uint16)
    g[1, 1], g[1, 7], g[4, 1], g[4, 7] = CURVE_SE, CURVE_SW, CURVE_NE, CURVE_NW
    g[1, 2:7] = HORZ
    g[4, 2:7] = HORZ
    g[2:4, 1] = VERT
    g[2:4, 7] = VERT
    return g


def oval():
    # clockwise = east along the top row; agents: (row, col, orientation, target row, target col)
    return _map(_oval_grid(6, 9), [(1, 3, E, 4, 4), (1, 5, W, 4, 2), (4, 5, W, 1, 4), (2, 1, S, 4, 4), (3, 7, S, 2, 1)],
                earliest=[0, 28, 0, 34, 0])      # the clockwise trains first


LASSO_SWITCH, LASSO_DEAD_END = (4, 4), (7, 4)


def lasso():
    g = _oval_grid(8, 9)
    # westbound (clockwise) trains choose west or south; eastbound ones pass; the spur joins towards the east
    g[LASSO_SWITCH] = ways((W, W), (W, S), (E, E), (N, E))
    g[5:7, 4] = VERT
    g[LASSO_DEAD_END] = DEAD_N
    return _map(g, [(1, 3, E, 7, 4),      # clockwise: reaches the dead end through the facing switch
                    (1, 5, W, 7, 4),      # counter-clockwise: never does (its own distance is 0xFFFF)
                    (6, 4, N, 2, 7),      # on the spur heading in: a cycle entered after mu > 0 steps, own target inside it
                    (5, 4, S, 3, 1),      # on the spur heading out: dead end, then the counter-clockwise ring
                    (4, 6, E, 6, 4)],     # counter-clockwise, its target on the spur: unreachable
                earliest=[0, 14, 16, 22, 14])


def disconnected():
    g = np.zeros((7, 10), dtype=np.uint16)
    g[0, 3], g[1:3, 3] = DEAD_S, VERT
    g[3, 0], g[3, 1:3] = DEAD_E, HORZ
    g[3, 3] = ways((E, E), (W, W), (W, N), (S, E))      # west of it the stem: westbound trains choose west or north
    g[3, 4], g[3, 5] = DEAD_W, DEAD_E                   # the gap: two dead ends back to back
    g[3, 6] = ways((W, W), (W, S), (E, E), (N, E))      # westbound trains choose west or south
    g[3, 7:9], g[3, 9] = HORZ, DEAD_W
    g[4:6, 6], g[6, 6] = VERT, DEAD_N
    return _map(g, [(3, 1, E, 6, 6),      # left component, target in the right one
                    (3, 8, W, 0, 3),      # right component, target in the left one
                    (1, 3, S, 3, 0),
                    (5, 6, N, 3, 9),
                    (3, 2, W, 0, 3)], earliest=[20, 10, 0, 0, 10])


CROSSING_AGENTS = [(4, 1, E), (1, 4, S), (4, 7, W), (7, 4, N), (6, 6, N)]


def _crossing_grid():
    g = np.zeros((9, 9), dtype=np.uint16)
    g[4, :], g[:, 4] = HORZ, VERT
    g[4, 0], g[4, 8], g[0, 4], g[8, 4] = DEAD_E, DEAD_W, DEAD_S, DEAD_N
    g[4, 4] = DIAMOND
    g[4, 6] = ways((E, E), (E, S), (W, W), (N, W))      # eastbound trains choose east or south
    g[5:7, 6], g[7, 6] = VERT, DEAD_N
    return g


def crossing_u1():
    return _map(_crossing_grid(), [a + (4, 3) for a in CROSSING_AGENTS], earliest=[0, 0, 0, 25, 6])      # (unreachable from the vertical line)


def crossing_u5():
    # a dead end behind the switch, the crossing itself, a plain cell, another dead end, a cell of the line the spur never reaches
    targets = [(7, 6), (4, 4), (4, 2), (0, 4), (6, 4)]
    return _map(_crossing_grid(), [a + t for a, t in zip(CROSSING_AGENTS, targets)], earliest=[8, 0, 0, 5, 30])


def full_grid(H, Wd):
    """rail on EVERY cell, the border included: left, forward and right wherever the neighbour is inside the grid"""
    g = np.zeros((H, Wd), dtype=np.uint16)
    for r in range(H):
        for c in range(Wd):
            for d in range(4):
                for m in ((d + 3) % 4, d, (d + 1) % 4):
                    if 0 <= r + DR[m] < H and 0 <= c + DC[m] < Wd:
                        g[r, c] |= way(d, m)
    return g


def mesh_grid(n):
    return full_grid(n, n)


def mesh12():
    return _map(mesh_grid(12), [(0, 0, E, 6, 6), (11, 11, W, 0, 5), (3, 8, S, 6, 6), (9, 2, N, 11, 0)])


def mesh33():
    return _map(mesh_grid(33), [(0, 0, E, 16, 16), (32, 32, W, 0, 0), (5, 20, S, 31, 7)])


MAPS = {"oval": oval, "lasso": lasso, "disconnected": disconnected, "crossing_u1": crossing_u1, "crossing_u5": crossing_u5,
        "mesh12": mesh12, "mesh33": mesh33}
SMALL = ("oval", "lasso", "disconnected", "crossing_u5")      # five agents each: they fit one batch when padded onto one canvas
EPISODES = SMALL + ("crossing_u1", "mesh12")                  # the fixtures with a recorded episode (mesh33: static arrays and distance map)


def padded(env, H, Wd):
    """the env dict `env` with its grid in the top-left corner of an empty H x W canvas (positions keep their coordinates)"""
    g = np.zeros((H, Wd), dtype=np.uint16)
    h, w = np.asarray(env["grid"]).shape
    g[:h, :w] = env["grid"]
    return dict(env, grid=g)


# Flatland's eleven cell types (the public rail specification: empty, straight, simple switch, diamond crossing, single slip, double slip,
# symmetrical switch, dead end, turn right, turn left, mirrored switch), each in its first orientation
CELL_TYPES = (0x0000, 0x8020, 0x9220, 0x8421, 0x9621, 0xCC33, 0x5202, 0x2000, 0x4002, 0x1200, 0xC022)


def rotated(g, quarter_turns):
    out = 0
    for d in range(4):
        for m in range(4):
            if int(g) & way(d, m):
                out |= way((d + quarter_turns) % 4, (m + quarter_turns) % 4)
    return out


def known_cell_type(g):
    """is the cell a rotation of one of Flatland's cell types?  On any other cell flatland_cutils leaves its agent's road type unset
    (Agent::update_transitions finds no match and the constructor sets no default): the eleven road-type columns 7 .. 17 of that agent's
    attribute row are whatever the field held -- the one part of a fixture that is no function of the env.  The project's builders say type 0."""
    return any(rotated(g, k) in CELL_TYPES for k in range(4))


ROAD_TYPE_COLS = slice(7, 18)


def defined_attr(fx, t):
    """bool[A, 83]: the elements of the flatland_cutils attribute rows of step t that the reference defines (see known_cell_type)"""
    st = fx["state"][t]
    ok = np.ones((len(st), 83), dtype=bool)
    for i, (r, c) in enumerate(st[:, 0:2]):
        if r >= 0 and not known_cell_type(fx["grid"][r, c]):
            ok[i, ROAD_TYPE_COLS] = False
    return ok


# ---- the maps of tests/step_state_cases.py (constructed states of RailEnv.step(); oracle/refharness/capture_step_states.py)
SYM_SWITCH = 0x5202                  # Flatland's symmetrical switch, stem to the south: a northbound train chooses west or east, never ahead
YARD_SYM, YARD_SWITCH = (1, 3), (4, 3)


def yard():
    """8 x 9: two lines with dead ends joined by a stem.  The stem enters a SYMMETRIC switch from below (FORWARD has no transition there and
    becomes STOP_MOVING); it leaves the bottom line at a simple switch that eastbound trains face (LEFT and FORWARD valid, RIGHT not); a
    stub of three cells in row 6 is a component of its own (a target nobody reaches: shortest path of length 0)"""
    g = np.zeros((8, 9), dtype=np.uint16)
    g[1, 0], g[1, 1:6], g[1, 6] = DEAD_E, HORZ, DEAD_W
    g[YARD_SYM] = SYM_SWITCH
    g[2:4, 3] = VERT
    g[4, 0], g[4, 1:7], g[4, 7] = DEAD_E, HORZ, DEAD_W
    g[YARD_SWITCH] = rotated(0x9220, 1)      # eastbound: east or north; southbound (off the stem): west; westbound: west
    g[6, 0], g[6, 1], g[6, 2] = DEAD_E, HORZ, DEAD_W
    assert g[YARD_SWITCH] == ways((E, E), (E, N), (S, W), (W, W))
    return _map(g, [(4, 1, E, 4, 6), (4, 5, W, 4, 0), (3, 3, N, 1, 6), (1, 5, W, 1, 0), (4, 1, E, 6, 1)], earliest=[2, 2, 2, 2, 2])


STEP_MAPS = {"yard": yard, "crossing": crossing_u5}      # five agents each: they share a batch when padded onto one canvas


# ---- plain numpy measurements of a map or a fixture (what tests/test_handmaps.py asserts the fixtures reach)
def successor(grid, state):
    """the state after (r, c, d) when it has exactly one way on, else None"""
    r, c, d = state
    bits = nibble(grid[r, c], d)
    if bin(bits).count("1") != 1:
        return None
    m = [k for k in range(4) if (bits >> (3 - k)) & 1][0]
    return (r + DR[m], c + DC[m], m)


def chain(grid, state):
    """walk the single-way states from `state`: (mu, lam) of the cycle it runs into -- the first repeated state is the one at index mu, the
    loop has lam states -- or None when the chain ends at a switch, a dead end or the edge of the rail"""
    seen, k = {}, 0
    while state is not None:
        if state in seen:
            return seen[state], k - seen[state]
        r, c, d = state
        if not (0 <= r < grid.shape[0] and 0 <= c < grid.shape[1]) or grid[r, c] == 0:
            return None
        if bin(int(grid[r, c])).count("1") == 1:      # a dead end: the branch walks stop here
            return None
        seen[state] = k
        state, k = successor(grid, state), k + 1
    return None


def level_sizes(dm_slab):
    """sizes of the BFS levels of one target's distance map u16[H, W, 4]: count of states per finite distance"""
    v = np.asarray(dm_slab).ravel()
    return np.bincount(v[v != 0xFFFF].astype(np.int64))


# ---- constructed agent states for GlobalObsForRailEnv (oracle/refharness/capture_global_states.py -> tests/golden/global_states_<map>.npz)
# What a played episode reaches only by luck: trains that SHARE a cell (an agent whose malfunction ends off the map and that is told to stop
# is put on its initial_position without MotionCheck), such a stack on a DONE agent's target or on the start cell of waiting agents, many
# agents of all three off-map states on one start cell, the two corner cells.  A state is one row per agent: (state, row, col, direction,
# malfunction_down_counter); row = col = -1 off the map and when DONE.
WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)


def state_rows(spec):
    """i32[A, 12] agent rows in the order of tests/util.STATE_NAMES from (state, row, col, direction, malfunction) per agent"""
    rows = np.full((len(spec), 12), -1, dtype=np.int32)
    for i, (kind, r, c, d, malf) in enumerate(spec):
        assert (r >= 0) == (MOVING <= kind <= MALF), spec[i]
        rows[i, 0:8] = (r, c, d, kind, malf, int(malf > 0), 0, 0)
        rows[i, 8] = 7 if kind == DONE else -1
    return rows


def _off(kind, d=0, malf=0):
    return (kind, -1, -1, d, malf)


def full5x7_states():
    """8 agents on a 5 x 7 grid with rail everywhere; agents 0 .. 4 start on ONE cell, agents 5 and 6 on the two corners"""
    m = _map(full_grid(5, 7), [(2, 3, E, 4, 6), (2, 3, S, 0, 0), (2, 3, W, 3, 1), (2, 3, N, 3, 1), (2, 3, E, 1, 2),
                               (0, 0, E, 4, 6), (4, 6, W, 0, 0), (1, 5, S, 2, 3)])
    m["speed"] = np.array([1.0, 1 / 2, 1 / 3, 1 / 4, 1 / 5, 1 / 2, 1 / 3, 1.0])
    states = [
        # a stack of two (handles 1 and 4) on the start cell of the off-map agents 0, 2 and 3: ch0 at the virtual position over a ch4 count
        [_off(WAITING, E), (STOPPED, 2, 3, E, 0), _off(READY, W), _off(MALF_OFF, N, 3), (MALF, 2, 3, W, 5), (MOVING, 1, 1, S, 0),
         _off(WAITING, W), (MOVING, 3, 4, N, 0)],
        # a stack of three (2, 5, 7), every direction, counter and speed different; trains on both corner cells
        [(MOVING, 0, 0, S, 0), _off(WAITING, S), (STOPPED, 3, 3, N, 0), _off(READY, N), _off(MALF_OFF, E, 4), (MALF, 3, 3, E, 7),
         (MOVING, 4, 6, N, 0), (MOVING, 3, 3, S, 1)],
        # five agents off the map on one start cell, in all three off-map states; off-map agents on the corners
        [_off(WAITING, E), _off(READY, S), _off(MALF_OFF, W, 2), _off(WAITING, N), _off(READY, E), _off(READY, E), _off(MALF_OFF, W, 6),
         (MOVING, 1, 5, S, 0)],
        # DONE agents: 2's target (3, 1) under the stack of 0 and 5 and also 3's target; 1's target (0, 0) under train 7
        [(MOVING, 3, 1, W, 0), _off(DONE, N), _off(DONE, W), (STOPPED, 2, 2, W, 0), (MALF, 1, 2, N, 9), (STOPPED, 3, 1, S, 2),
         (STOPPED, 4, 6, E, 0), (MOVING, 0, 0, N, 0)],
        # everybody but the last handle DONE
        [_off(DONE, E), _off(DONE, S), _off(DONE, W), _off(DONE, N), _off(DONE, E), _off(DONE, S), _off(DONE, W), (MOVING, 2, 3, S, 0)],
        # two stacks at once, on the two corners, one of them on its lower handle's own start cell
        [(MOVING, 4, 6, E, 0), _off(WAITING, S), _off(READY, W), (MOVING, 2, 3, N, 0), _off(MALF_OFF, E, 1), (STOPPED, 0, 0, W, 0),
         (MALF, 4, 6, S, 3), (MOVING, 0, 0, S, 8)],
    ]
    return m, np.stack([state_rows(s) for s in states])


def crossing_states():
    """the five agents of crossing_u5 (a sparse rail: most cells hold none)"""
    m = crossing_u5()
    m["speed"] = np.array([1.0, 1 / 2, 1 / 3, 1 / 4, 1 / 5])
    states = [
        [_off(WAITING, E), _off(WAITING, S), _off(WAITING, W), _off(WAITING, N), _off(WAITING, N)],
        # a stack of two on the diamond crossing, which is agent 1's target; agent 4 DONE with train 0 on its target
        [(MOVING, 6, 4, N, 0), (MALF, 4, 4, S, 4), _off(MALF_OFF, W, 2), (MOVING, 4, 4, E, 0), _off(DONE, N)],
        # a stack of three on the start cell of agent 2, which is ready to depart; observed from below, from inside and from the top
        [(STOPPED, 4, 7, E, 2), (MOVING, 4, 7, W, 0), _off(READY, W), _off(DONE, N), (MALF, 4, 7, N, 6)],
        # the highest handle of the stack is the only other train: the lowest one sees it, a handle elsewhere sees it too
        [(MOVING, 4, 2, W, 0), (STOPPED, 2, 4, S, 0), (STOPPED, 4, 2, E, 1), _off(WAITING, N), (MOVING, 5, 6, S, 0)],
    ]
    return m, np.stack([state_rows(s) for s in states])


GLOBAL_STATES = {"full5x7": full5x7_states, "crossing": crossing_states}


def global_static(m):
    """the static description BatchedRailEnv / tests/global_obs_np.py take, from a map dict that has speeds (no malfunctions, a long episode)"""
    A = len(m["init_dir"])
    return dict(grid=m["grid"], init_pos=m["init_pos"], init_dir=m["init_dir"], target=m["target"], speed=np.asarray(m["speed"], dtype=np.float64),
                earliest=m["earliest"], latest=np.asarray(m["earliest"]) + 200, T=400, malf_rate=0.0, malf_min=0, malf_max=0,
                mt_key=np.arange(624, dtype=np.uint32), mt_pos=624)
