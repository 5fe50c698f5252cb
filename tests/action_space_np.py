"""The fixtures of tools/capture_action_space.py (tests/golden/action_space_*.npz) as a list of groups, and a loop-by-loop numpy
restatement of the reference's functions they record (flatland/contrib/wrappers/flatland_wrappers.py): possible_actions_sorted_by_distance
(:14-56), find_all_cells_where_agent_can_choose (:145-176) and SkipNoChoiceCellsWrapper.on_decision_cell (:197-198).  A helper module,
not a test: own numpy code that imports nothing of the reference and nothing of the library."""
import glob
import os

import numpy as np

from tests import util

SOURCES = ("handmaps", "states_yard_small", "states_yard_crowd", "states_crossing_small", "states_crossing_crowd", "episodes")
STATIC = ("grid", "init_pos", "init_dir", "target", "speed", "dm", "slot", "cells")
KINDS = ("sp_action", "sp_dist", "sp_count", "on_decision")
WRAPPED = {"wrapped_episode": "episodes", "wrapped_lasso": "handmaps"}      # group -> the file that holds it
WRAPPED_STATICS = {"wrapped_episode": "cfg1_malf20_spfollow", "wrapped_lasso": "handmap_lasso"}      # ... -> the fixture with its env
WRAPPED_KEYS = ("reduced", "present", "reward", "done", "done_all", "action_required", "malfunction", "speed", "info_state", "state", "inner")
WRAPPED_DISCOUNT = 0.9
DR, DC = (-1, 0, 1, 0), (0, 1, 0, -1)
WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)
NOTHING, LEFT, FORWARD, RIGHT, STOP = range(5)
SLOTS = 3
_cache = {}


def files():
    return sorted(os.path.basename(f)[len("action_space_"):-4] for f in glob.glob(os.path.join(util.GOLD, "action_space_*.npz")))


def _load(source):
    if source not in _cache:
        _cache[source] = np.load(os.path.join(util.GOLD, "action_space_%s.npz" % source))
    return _cache[source]


def groups(source):
    """[dict(source, name, grid, ..., cells [H, W], steps, state [S, A, 12], sp_action, sp_dist [S, A, 3], sp_count, on_decision [S, A])]"""
    z = _load(source)
    out = []
    for name in z["groups"]:
        name = str(name)
        if name in WRAPPED:
            continue
        g = {"source": source, "name": name}
        for k in STATIC + KINDS + ("steps", "state"):
            g[k] = z[name + "/" + k]
        out.append(g)
    return out


def all_groups():
    return [g for s in SOURCES for g in groups(s)]


def wrapped_episode(name="wrapped_episode"):
    z = _load(WRAPPED[name])
    return {k: z[name + "/" + k] for k in WRAPPED_KEYS}


def static_of(g, agents=None):
    """a static description BatchedRailEnv loads: the group's map and its agents (`agents`: a subset of them); what the action space
    does not read (timetable, malfunction parameters, the RNG) is filled in"""
    return util.group_static(g, agents)


# ---- the restatement
def transitions(grid, r, c, d):
    """rail.get_transitions(r, c, d): (N, E, S, W)"""
    nib = (int(grid[r, c]) >> ((3 - d) * 4)) & 15
    return tuple((nib >> (3 - m)) & 1 for m in range(4))


def decision_cells(grid):
    """find_all_cells_where_agent_can_choose as a byte map: bit 0 switch, bit 1 neighbour of a switch"""
    H, W = grid.shape
    cells = np.zeros((H, W), dtype=np.uint8)
    for r in range(H):
        for c in range(W):
            is_switch = False
            for o in range(4):
                if sum(transitions(grid, r, c, o)) > 1:
                    cells[r, c] |= 1
                    is_switch = True
                    break
            if is_switch:
                for o in range(4):
                    t = transitions(grid, r, c, o)
                    for m in range(4):
                        if t[m]:
                            nr, nc = r + DR[m], c + DC[m]
                            # (a cell off the grid or without rail -- no valid map points at one -- has no byte, or keeps 0)
                            if 0 <= nr < H and 0 <= nc < W and grid[nr, nc] != 0:
                                cells[nr, nc] |= 2
    return cells


def possible_actions(grid, dm, slot, init_pos, row):
    """possible_actions_sorted_by_distance for one agent: the reference's list of (action, distance)"""
    r, c, d, state = (int(v) for v in row[:4])
    H, W = grid.shape
    if state == READY:
        vr, vc = (int(v) for v in init_pos)
    elif MOVING <= state <= MALF:
        vr, vc = r, c
    else:
        return [(NOTHING, 0.0)] * 2
    t = transitions(grid, vr, vc, d)
    steps = []
    for m in range(4):
        if t[m]:
            if m == d:
                a = FORWARD
            elif m == (d + 1) % 4:
                a = RIGHT
            elif m == (d - 1) % 4:
                a = LEFT
            else:
                a = FORWARD
            nr, nc = vr + DR[m], vc + DC[m]
            dist = np.inf
            if 0 <= nr < H and 0 <= nc < W:
                v = dm[slot, nr, nc, m]
                dist = np.inf if v == 0xFFFF else float(v)
            steps.append((a, dist))
    steps = sorted(steps, key=lambda s: s[1])
    return steps * 2 if len(steps) == 1 else steps


def action_space(grid, dm, slot, init_pos, state, cells):
    """every agent of one recorded state -> (sp_action u8 [A, 3], sp_dist f64 [A, 3], sp_count u8 [A], on_decision u8 [A])"""
    A = len(slot)
    act = np.zeros((A, SLOTS), dtype=np.uint8)
    dist = np.full((A, SLOTS), np.inf, dtype=np.float64)
    cnt = np.zeros(A, dtype=np.uint8)
    dec = np.zeros(A, dtype=np.uint8)
    for h in range(A):
        got = possible_actions(grid, dm, int(slot[h]), init_pos[h], state[h])
        cnt[h] = len(got)
        for k, (a, dd) in enumerate(got):
            act[h, k], dist[h, k] = a, dd
        r, c = int(state[h][0]), int(state[h][1])
        dec[h] = r < 0 or (r, c) == tuple(int(v) for v in init_pos[h]) or cells[r, c] != 0
    return act, dist, cnt, dec


def translate(reduced, act, cnt):
    """ShortestPathActionWrapper.step's translation by indexing a recorded list; an entry the list does not have gives 0"""
    out = np.array(reduced, dtype=np.uint8).copy()
    for idx in np.ndindex(out.shape):
        a = int(out[idx])
        if a != 255 and a != 0:
            out[idx] = act[idx][a - 1] if a - 1 < int(cnt[idx]) else 0
    return out
