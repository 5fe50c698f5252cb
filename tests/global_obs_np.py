"""Vectorised numpy restatement of flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) from an env's static
description and its agent state rows (the [A, 12] int32 rows of util.golden_state / BatchedRailEnv.state()).  Pinned against the
reference-captured goldens by tests/test_global_obs_golden.py; the GPU tests use it at sizes no fixture covers."""
import numpy as np

WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)


def rail_obs(grid):
    """[H, W, 16] float64: channel k = bit 15 - k of the cell's transitions (observations.py:560-566)"""
    g = np.asarray(grid, dtype=np.uint16).astype(np.int64)
    return ((g[..., None] >> (15 - np.arange(16))) & 1).astype(np.float64)


def global_obs(static, state):
    """(rail [H,W,16], agents_state [A,H,W,5], targets [A,H,W,2]), float64 -- get(handle) for every handle, stacked"""
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

    base = np.full((H, W, 5), -1.0)
    base[..., 4] = 0.0
    base[row[has_pos], col[has_pos], 1] = dr[has_pos]
    base[row[has_pos], col[has_pos], 2] = malf[has_pos]
    base[row[has_pos], col[has_pos], 3] = speed[has_pos]
    np.add.at(base[..., 4], (ip[off, 0], ip[off, 1]), 1.0)
    tbase = np.zeros((H, W, 2))
    tbase[tg[~done, 0], tg[~done, 1], 1] = 1.0

    ast = np.repeat(base[None], A, axis=0)
    tgt = np.repeat(tbase[None], A, axis=0)
    h = np.arange(A)
    vr = np.where(off, ip[:, 0], np.where(done, tg[:, 0], row))     # the virtual position (:572-579)
    vc = np.where(off, ip[:, 1], np.where(done, tg[:, 1], col))
    ast[h, vr, vc, 0] = dr
    ast[h[has_pos], row[has_pos], col[has_pos], 1] = -1.0            # ch1 is for the OTHER agents (:601-602)
    tgt[h, tg[:, 0], tg[:, 1], 0] = 1.0
    return rail_obs(grid), ast, tgt
