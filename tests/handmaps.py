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


def mesh_grid(n):
    g = np.zeros((n, n), dtype=np.uint16)
    for r in range(n):
        for c in range(n):
            for d in range(4):
                for m in ((d + 3) % 4, d, (d + 1) % 4):
                    if 0 <= r + DR[m] < n and 0 <= c + DC[m] < n:
                        g[r, c] |= way(d, m)
    return g


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
