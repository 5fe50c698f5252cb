"""Constructed envs and agent states for the GlobalObsForRailEnv kernel (fl_obs_global), on grids with rail on EVERY cell
(tests/handmaps.full_grid: fl_set_state refuses a position without rail).  A helper module, not a test; numpy only.

sweep(H, W, A): a list of (static, rows) -- one env per state, because the start cells and the targets move with the state -- in which
every cell of the map is, in some state, a train's own position, some handle's target and the initial_position of a handle that is off the
map.  However the launcher carves the map into bands and the agents into groups, every band edge, every cell 0 and HW - 1 and every phase
of a run's first and last element against the 16-byte words of the output is then hit by a patch and by a slab value; the tests that use
it copy none of the launcher's arithmetic.

  - handles 0 .. n - 1 sweep (n = A - 1, or 1 when A = 1): in state k the handle i has the cell q = (k * n + i) mod HW; its position is q,
    its initial_position q + HW // 3 + 1 and its target q + 2 * (HW // 3) + 2 (mod HW): three cells far apart, in different bands wherever
    the map has several
  - its state is KINDS[(q + r) mod 7] in pass r = 0, 1, 2 -- off the map and on it in turn, then DONE -- so that over the three passes
    every q has been a position, a start cell of an off-map agent and a DONE agent's virtual position; S = ceil(HW / n) states a pass
  - when A >= 2 the last handle rides: it stands ON the highest sweeping handle that is on the map (a shared cell in every state that has
    a train; always when A >= 5), with another direction, counter and speed
  - in every second state of the list the handles are rotated by one, so that the rider is the LOWEST handle of its stack as often as the highest
"""
import numpy as np

from tests import handmaps, util

WAITING, READY, MALF_OFF, MOVING, STOPPED, MALF, DONE = range(7)
KINDS = (WAITING, MOVING, READY, STOPPED, MALF_OFF, MALF, DONE)
# (H, W, A): 2x3 the smallest; 3x5 and 5x5 odd phases of a run's start (HW * 5 mod 4 = 3 and 1); 27x27 more than one float64 band,
# 37x35 more than one float32 band; 257 agents: the second trip of the kernel's agent loop and a short last agent group
SWEEPS = [(H, W, A) for H, W in ((2, 3), (3, 5), (5, 5)) for A in (1, 2, 5, 27)] + [(27, 27, 5), (27, 27, 27), (27, 27, 257),
                                                                                     (37, 35, 5), (37, 35, 27)]


def _static(grid, ip, idir, tg, speed):
    W = grid.shape[1]
    return util.plain_static(grid, np.stack([ip // W, ip % W, idir, tg // W, tg % W], axis=1), speed)


def _rows(W, kind, cell, dr, malf):
    A = len(kind)
    rows = np.full((A, 12), -1, dtype=np.int32)
    on = (kind >= MOVING) & (kind <= MALF)
    rows[:, 0] = np.where(on, cell // W, -1)
    rows[:, 1] = np.where(on, cell % W, -1)
    rows[:, 2], rows[:, 3], rows[:, 4] = dr, kind, malf
    rows[:, 5] = malf > 0
    rows[:, 6] = rows[:, 7] = 0
    rows[:, 8] = np.where(kind == DONE, 7, -1)
    return rows


def sweep(H, W, A):
    grid = handmaps.full_grid(H, W)
    HW = H * W
    n = max(A - 1, 1)
    S = -(-HW // n)
    off_ip, off_tg = HW // 3 + 1, 2 * (HW // 3) + 2
    out = []
    for r in range(3):
        for k in range(S):
            q = (k * n + np.arange(n)) % HW
            kind = np.array([KINDS[(int(c) + r) % 7] for c in q])
            dr = (q + k) % 4
            malf = np.where((kind == MALF) | (kind == MALF_OFF), q % 5 + 1, 0)
            speed = 1.0 / (1 + np.arange(n) % 4)
            cell = q.copy()
            if A >= 2:
                on = np.flatnonzero((kind >= MOVING) & (kind <= MALF))
                under = int(on[-1]) if len(on) else 0
                c = int(q[under])
                cell = np.append(cell, c)
                q = np.append(q, c)
                kind = np.append(kind, (MOVING, STOPPED, MALF)[k % 3])
                dr = np.append(dr, (dr[under] + 1 + k % 3) % 4)
                malf = np.append(malf, malf[under] + 2 if k % 3 == 2 else 0)
                speed = np.append(speed, 0.2)
            ip, tg = (q + off_ip) % HW, (q + off_tg) % HW
            shift = (r * S + k) % 2 if A >= 2 else 0
            kind, cell, dr, malf, speed, ip, tg = (np.roll(v, shift) for v in (kind, cell, dr, malf, speed, ip, tg))
            out.append((_static(grid, ip, (dr + 1) % 4, tg, speed), _rows(W, kind, cell, dr, malf)))
    return out


def random_states(H, W, A, count, seed):
    """count (static, rows) on the full H x W grid with everything drawn at random: on a small map most states hold stacks"""
    rng = np.random.RandomState(seed)
    grid = handmaps.full_grid(H, W)
    HW = H * W
    out = []
    for _ in range(count):
        kind = rng.randint(0, 7, A)
        cell, ip, tg = rng.randint(0, HW, A), rng.randint(0, HW, A), rng.randint(0, HW, A)
        dr = rng.randint(0, 4, A)
        malf = np.where((kind == MALF) | (kind == MALF_OFF), rng.randint(1, 9, A), 0)
        speed = 1.0 / rng.randint(1, 5, A)
        out.append((_static(grid, ip, rng.randint(0, 4, A), tg, speed), _rows(W, kind, cell, dr, malf)))
    return out
