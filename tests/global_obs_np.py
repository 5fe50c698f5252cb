"""Numpy restatements of flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) from an env's static description
and its agent state rows (the [A, 12] int32 rows of util.golden_state / BatchedRailEnv.state()): global_obs, vectorised, and
global_obs_literal, one pass per handle.  Both hold for ANY state, trains that share a cell included (an agent whose malfunction
ends off the map and that is told to stop is put on its initial_position without MotionCheck being asked).  Pinned against the
reference-captured goldens by tests/test_global_obs_golden.py (episodes, global_*.npz) and tests/test_global_obs_states.py
(constructed states, global_states_*.npz); the GPU tests use them at sizes no fixture covers."""
import numpy as np

WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)


def rail_obs(grid):
    """[H, W, 16] float64: channel k = bit 15 - k of the cell's transitions (observations.py:560-566)"""
    g = np.asarray(grid, dtype=np.uint16).astype(np.int64)
    return ((g[..., None] >> (15 - np.arange(16))) & 1).astype(np.float64)


def global_obs_literal(static, state):
    """(rail [H,W,16], agents_state [A,H,W,5], targets [A,H,W,2]), float64 -- get(handle) for every handle, stacked.  One pass per
    handle over the agents in handle order, every write a plain assignment, so that on a cell several agents write the last one wins."""
    grid = np.asarray(static["grid"])
    H, W = grid.shape
    state = np.asarray(state)
    A = len(state)
    ast = np.empty((A, H, W, 5))
    tgt = np.zeros((A, H, W, 2))
    for h in range(A):
        mine = ast[h]
        mine[..., 0:4] = -1.0
        mine[..., 4] = 0.0
        kind = int(state[h, 3])
        if kind <= MALF_OFF:                      # the virtual position (:571-576)
            where = tuple(int(v) for v in static["init_pos"][h])
        elif kind == DONE:
            where = tuple(int(v) for v in static["target"][h])
        else:
            where = (int(state[h, 0]), int(state[h, 1]))
        mine[where][0] = float(state[h, 2])
        tgt[h][tuple(int(v) for v in static["target"][h])][0] = 1.0
        for i in range(A):
            if int(state[i, 3]) == DONE:           # not on the grid any more
                continue
            tgt[h][tuple(int(v) for v in static["target"][i])][1] = 1.0
            if state[i, 0] >= 0:
                cell = (int(state[i, 0]), int(state[i, 1]))
                if i != h:
                    mine[cell][1] = float(state[i, 2])
                mine[cell][2] = float(state[i, 4])
                mine[cell][3] = float(static["speed"][i])
            if int(state[i, 3]) <= MALF_OFF:
                mine[tuple(int(v) for v in static["init_pos"][i])][4] += 1.0
    return rail_obs(grid), ast, tgt


def global_obs(static, state):
    """the same three arrays, vectorised: one slab for every handle -- ch1 .. ch3 of a cell from the HIGHEST handle that stands on it --
    and per handle ch0 at its virtual position, the targets' ch0 at its own target, and ch1 of its own cell taken from the highest
    OTHER handle there (-1 when it stands alone)"""
    grid = np.asarray(static["grid"])
    H, W = grid.shape
    state = np.asarray(state)
    A = len(state)
    row, col, dr, st, malf = (state[:, k].astype(np.int64) for k in (0, 1, 2, 3, 4))
    ip = np.asarray(static["init_pos"], dtype=np.int64)
    tg = np.asarray(static["target"], dtype=np.int64)
    speed = np.asarray(static["speed"], dtype=np.float64)
    done = st == DONE
    off = st <= MALF_OFF
    has_pos = ~done & (row >= 0)
    on = np.flatnonzero(has_pos)                                    # ascending handles
    cell = row[on] * W + col[on]

    # the two highest handles of every occupied cell (-1: none)
    top = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(top, cell, on)
    below = on != top[cell]
    second = np.full(H * W, -1, dtype=np.int64)
    np.maximum.at(second, cell[below], on[below])

    base = np.full((H * W, 5), -1.0)
    base[:, 4] = 0.0
    occ = np.flatnonzero(top >= 0)
    base[occ, 1] = dr[top[occ]]
    base[occ, 2] = malf[top[occ]]
    base[occ, 3] = speed[top[occ]]
    np.add.at(base[:, 4], ip[off, 0] * W + ip[off, 1], 1.0)
    tbase = np.zeros((H, W, 2))
    tbase[tg[~done, 0], tg[~done, 1], 1] = 1.0

    ast = np.repeat(base.reshape(1, H, W, 5), A, axis=0)
    tgt = np.repeat(tbase[None], A, axis=0)
    h = np.arange(A)
    vr = np.where(off, ip[:, 0], np.where(done, tg[:, 0], row))     # the virtual position (:572-579)
    vc = np.where(off, ip[:, 1], np.where(done, tg[:, 1], col))
    ast[h, vr, vc, 0] = dr
    # ch1 is for the OTHER agents (:601-602): the highest handle of a cell sees the second highest there
    mine = on[~below]
    other = second[cell[~below]]
    ast[mine, row[mine], col[mine], 1] = np.where(other >= 0, dr[np.maximum(other, 0)], -1.0)
    tgt[h, tg[:, 0], tg[:, 1], 0] = 1.0
    return rail_obs(grid), ast, tgt


def shared_cells(state):
    """bool[A]: the agent is on the map, not DONE, and another such agent stands on its cell; and bool[A]: it is the highest handle there"""
    state = np.asarray(state)
    on = (state[:, 0] >= 0) & (state[:, 3] != DONE)
    key = np.where(on, state[:, 0].astype(np.int64) * 65536 + state[:, 1], -1 - np.arange(len(state)))
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    shared = on & (cnt[inv] > 1)
    top = np.zeros(len(state), dtype=bool)
    for k in np.unique(key[shared]):
        top[np.flatnonzero(key == k).max()] = True
    return shared, top
