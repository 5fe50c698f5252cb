"""GPU: the prefix sums of the observation kernels' trees phase and index scan are data-parallel scans (csrc/fl_obs_ctx.h: wave_incl_scan, DPP row
shifts and row broadcasts over segments of 16, 32 or 64 lanes) instead of chains of shuffles: team_prepare's inclusive prefix of a tree's visit
counts (teams of 32 lanes for the flatland_cutils trees, 16 for the compact upstream trees), wg_pass_b's prefix over the cell counts of up to 64
teams, and the prefix over the workgroup's partial sums when the prediction index is built.  A wrong sum at a row boundary (lanes 15 | 16,
31 | 32, 47 | 48) would move slices, node links or item offsets, so every output tensor of both builders, the state, the rewards and the dones
are compared with the CPU oracle's (oracle.orc) on EVERY step of a short episode, byte for byte.  Also: pass B's late() has one call site and
trees_merged no second call behind it -- the rest of phase 1 and the topology piece must still be complete (attribute rows, valid actions,
adjacency, orders: all among the compared tensors).

Batches (two to four envs each, 6 - 16 steps; obs_both(depth, 30) and obs_policy() on every step):

  cfg1     7 agents on 30 x 30: 14 of the 64 teams have cells, all in rows 0 and 2 of the team prefix
  cfg2     the headline's envs (20 agents): classes 1 and 6
  y1       ONE agent on the yard (tests/test_gpu_obs_tail_fill.py): two teams with cells, lanes 0 and 32 -- the second one's prefix is the
           row_bcast:31 term alone
  y20      20 agents on the yard, 16 of them DONE or waiting in turn by handle (set with fl_set_state): teams without cells between teams with
           cells; y20over: the same beside an env with every agent DONE, observed and not stepped (that episode is over)
  y32      32 agents on the yard (tests/test_gpu_passb_slices.py: crowd, moving, dense): all 64 teams of the round, every row boundary of the
           prefix carries a sum; trees that fill all 31 nodes (team_prepare's 32-lane segments: both rows of a segment)
  cfg3     80 agents, two envs, depth 3: a ROUNDS kernel (classes 2 and 7) -- three rounds of trees, the last with 16 agents"""

import numpy as np
import pytest

from tests import obs_state_cases as oc
from tests import obs_switch_runs as sw
from tests import util

pytestmark = pytest.mark.gpu
N, E, S, W = 0, 1, 2, 3
M, WAIT = oc.MOVING, oc.off(oc.WAITING)


def _y20():
    spec, speed, _ = sw.crowd(8)
    turn = [oc.on(M, 1, 4, W), oc.on(M, 4, 1, E)] + [oc.GONE, WAIT] * 8 + [oc.on(M, 4, 5, W), oc.on(M, 3, 3, N)]
    return {"turn": (spec, speed, turn)}, {"alldone": (spec, speed, [oc.GONE] * 20), "turn": (spec, speed, turn)}


Y20, Y20_OVER = _y20()
# batch -> (map, cases, steps): the constructed states are stepped with the synthetic uniform actions like the generated envs
STATE_BATCHES = (("y1", "yard", sw.Y1, 10), ("y20", "yard", Y20, 10), ("y20over", "yard", Y20_OVER, 0), ("y32", "yard", dict(sw.Y32, dense=sw.dense(15)), 10))
GEN_BATCHES = (("cfg1", 3, 2, 16), ("cfg2", 3, 2, 12), ("cfg3", 2, 3, 6))      # workload, envs, depth of the upstream tree, steps


def _compare(env, oracles, depth, where, classes):
    """both launches on the batch's current state against every env's oracle"""
    B, A = env.B, env.A
    got, tree = env.obs_both(depth, 30)
    fix = env.last_obs_class()[0]
    got = {k: v.cpu().numpy() for k, v in got.items()}
    tree = tree.cpu().numpy()
    pol = env.obs_policy()
    fix_p = env.last_obs_class()[0]
    assert (fix, fix_p) == classes, (where, fix, fix_p)
    names = ("agent_attr", "forest", "adjacency", "node_order", "edge_order")
    pol = {n: t.cpu().numpy() for n, t in zip(names, pol)}
    for b, o in enumerate(oracles):
        exp_tree = o.obs_pytree(depth, 30)
        exp = o.obs_cutils(sw.MAX_NODES, 500)       # (every step: the deadlock flags are sticky)
        for g, e in sw.CUTILS:
            util.same(got[g][b], exp[e], f"{where} env {b} both {g}", dtype=True, bytes=True)
        util.same(tree[b], exp_tree, f"{where} env {b} depth-{depth} tree", dtype=True, bytes=True)
        adj, no, eo = sw.policy_form(exp, b, A)
        for g, e in (("agent_attr", exp["attr"]), ("forest", exp["forest"]), ("adjacency", adj), ("node_order", no), ("edge_order", eo)):
            util.same(pol[g][b], e, f"{where} env {b} policy {g}", dtype=True, bytes=True)


def _episode(env, oracles, statics, seed, steps, depth, name, classes):
    from flatland_marl_amd import synth
    from oracle import orc
    A = env.A
    tc = [0] * env.B
    _compare(env, oracles, depth, f"{name} start", classes)
    for t in range(steps):
        rew, done, done_all = (x.cpu().numpy() for x in env.step_synth(seed, 0, 0, auto_reset=True))
        st, _ = env.state()
        ended = []
        for b, o in enumerate(oracles):
            r_o, d_o, da = o.step(synth.uniform_actions(seed, b, tc[b], A))
            tc[b] += 1
            w = f"{name} env {b} step {t}"
            util.same(st[b], o.state(), w + " state", dtype=True, bytes=True)
            util.same(rew[b], np.asarray(r_o, dtype=rew.dtype), w + " rewards", dtype=True, bytes=True)
            util.same(done[b].astype(bool), np.asarray(d_o).astype(bool), w + " dones", dtype=True, bytes=True)
            assert bool(done_all[b]) == bool(da), w + " done_all"
            if da:
                ended.append(b)
        _compare(env, oracles, depth, f"{name} step {t}", classes)
        for b in ended:      # (the batch starts an ended episode over with its next step: the observation above is the ended episode's)
            key, pos = oracles[b].get_rng()
            oracles[b] = orc.OracleEnv(statics[b])
            oracles[b].set_rng(key, pos)
            tc[b] = 0
    env.check()


def _state_batch(batch):
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    from oracle import orc
    _, map_name, cases, steps = next(b for b in STATE_BATCHES if b[0] == batch)
    names = list(cases)
    grid = sw.grid_of(map_name)
    statics = [util.plain_static(grid, cases[k][0], cases[k][1]) for k in names]
    env = BatchedRailEnv(statics)
    pairs = [sw.rows(grid, cases[k][0], cases[k][2]) for k in names]
    states, aux = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    env.set_state(states, aux, np.zeros(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.uint8))
    oracles = [orc.OracleEnv(s) for s in statics]
    for o, (st, ax) in zip(oracles, pairs):
        o.set_state(st, ax, 0, False)
    _episode(env, oracles, statics, 7, steps, 2, batch, (1, 6))
    env.close()


def _generated_batch(workload):
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    from oracle import orc
    _, B, depth, steps = next(b for b in GEN_BATCHES if b[0] == workload)
    statics, seed = wl.make_envs(workload, B=B)
    env = BatchedRailEnv(statics)
    oracles = [orc.OracleEnv(s) for s in statics]
    _episode(env, oracles, statics, seed, steps, depth, workload, (2, 7) if workload == "cfg3" else (1, 6))
    env.close()


@pytest.mark.parametrize("batch", [b[0] for b in STATE_BATCHES])
def test_constructed_states_equal_the_oracle_on_every_step(batch):
    _state_batch(batch)


@pytest.mark.parametrize("workload", [b[0] for b in GEN_BATCHES])
def test_generated_envs_equal_the_oracle_on_every_step(workload):
    _generated_batch(workload)
