"""flatland.envs.predictions.ShortestPathPredictorForRailEnv.get() (predictions.py:97-180) and get_shortest_paths(distance_map,
max_depth) (rail_env_shortest_paths.py:17-71, 203-274) restated in numpy, loop by loop, on this library's arrays:

  grid      uint16 [H, W]          the rail's transitions
  dm, slot  uint16 [U, H, W, 4], int [A]: one distance map per unique target (0xFFFF = inf, BatchedRailEnv.distance_map) and every
                                   agent's map -- distance_map.get()[handle] is dm[slot[handle]]
  init_pos, target  int [A, 2];  speed float64 [A]
  state     int [A, >= 4]          rows (row, col, dir, TrainState) as BatchedRailEnv.state() / fl_set_state have them

No closed forms: what the kernel computes with them is compared against these loops."""
import math

import numpy as np

STOP_MOVING = 4
OFF_MAP = (0, 1, 2)      # WAITING, READY_TO_DEPART, MALFUNCTION_OFF_MAP
ON_MAP = (3, 4, 5)       # MOVING, STOPPED, MALFUNCTION
DONE = 6
_DELTA = ((-1, 0), (0, 1), (1, 0), (0, -1))


def _transitions(grid, pos, direction):
    """GridTransitionMap.get_transitions(row, col, direction): the four bits of the direction's nibble, N E S W"""
    nib = (int(grid[pos]) >> ((3 - direction) * 4)) & 15
    return [(nib >> 3) & 1, (nib >> 2) & 1, (nib >> 1) & 1, nib & 1]


def _is_dead_end(grid, pos):
    return bin(int(grid[pos])).count("1") == 1


def valid_move_actions(grid, direction, pos):
    """get_valid_move_actions_ (rail_env_shortest_paths.py:17-71): [(next position, next direction)] in the order the OrderedSet
    is iterated in (the action itself does not matter to the walk)"""
    out = []
    possible = _transitions(grid, pos, direction)
    if _is_dead_end(grid, pos):
        ex = (direction + 2) % 4
        if possible[ex]:
            out.append(((pos[0] + _DELTA[ex][0], pos[1] + _DELTA[ex][1]), ex))
    else:           # (one transition or several: the same directions in the same order)
        for nd in [(direction + i) % 4 for i in range(-1, 2)]:
            if possible[nd]:
                out.append(((pos[0] + _DELTA[nd][0], pos[1] + _DELTA[nd][1]), nd))
    return out


def _start(state_row, init_pos, target):
    st = int(state_row[3])
    if st in OFF_MAP:
        return (int(init_pos[0]), int(init_pos[1]))
    if st in ON_MAP:
        return (int(state_row[0]), int(state_row[1]))
    assert st == DONE
    return (int(target[0]), int(target[1]))


def shortest_path(grid, dm_a, start, direction, target, max_depth):
    """_shortest_path_for_agent (:229-266) for one agent: [((row, col), dir)] or None.  dm_a: uint16 [H, W, 4]"""
    H, W = grid.shape
    position = start
    path = []
    distance = math.inf
    depth = 0
    while position != target and depth < max_depth:
        best = None
        for npos, ndir in valid_move_actions(grid, direction, position):
            if 0 <= npos[0] < H and 0 <= npos[1] < W:
                v = int(dm_a[npos[0], npos[1], ndir])
                nd = math.inf if v == 0xFFFF else v
            else:
                nd = math.inf      # (a transition off the map: the reference's distance map has no such cell)
            if nd < distance:
                best = (npos, ndir)
                distance = nd
        path.append((position, direction))
        depth += 1
        if best is None:
            return None
        position, direction = best
    if depth < max_depth:
        path.append((position, direction))
    return path


def predict(grid, dm, slot, init_pos, target, speed, state, max_depth):
    """-> pred float64 [A, max_depth + 1, 5], waypoints int32 [A, max_depth, 3] (-1 behind the length), length int32 [A] (0 = None),
    visited: per agent the list of (row, col, dir) in insertion order (env.dev_pred_dict[handle])"""
    grid = np.asarray(grid)
    A = len(slot)
    pred = np.zeros((A, max_depth + 1, 5), dtype=np.float64)
    wps = np.full((A, max_depth, 3), -1, dtype=np.int32)
    length = np.zeros(A, dtype=np.int32)
    visited_all = []
    for a in range(A):
        tgt = (int(target[a][0]), int(target[a][1]))
        vpos = _start(state[a], init_pos[a], tgt)
        vdir = int(state[a][2])
        sp = shortest_path(grid, dm[int(slot[a])], vpos, vdir, tgt, max_depth)
        if sp is not None:
            length[a] = len(sp)
            for k, (p, d) in enumerate(sp):
                wps[a, k] = (p[0], p[1], d)
        times_per_cell = int(np.reciprocal(np.float64(speed[a])))
        pred[a, 0] = [0, vpos[0], vpos[1], vdir, 0]
        if sp:
            sp = sp[1:]
        new_direction, new_position = vdir, vpos
        visited = []
        for index in range(1, max_depth + 1):
            if new_position == tgt or not sp:
                pred[a, index] = [index, new_position[0], new_position[1], new_direction, STOP_MOVING]
                v = (new_position[0], new_position[1], vdir)
                if v not in visited:
                    visited.append(v)
                continue
            if index % times_per_cell == 0:
                new_position, new_direction = sp[0]
                sp = sp[1:]
            pred[a, index] = [index, new_position[0], new_position[1], new_direction, 0]
            v = (new_position[0], new_position[1], new_direction)
            if v not in visited:
                visited.append(v)
        visited_all.append(visited)
    return pred, wps, length, visited_all
