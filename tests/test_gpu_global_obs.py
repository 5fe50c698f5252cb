"""GPU: GlobalObsForRailEnv (flatland/envs/observations.py:535-611) through every layer -- fl_obs_global, BatchedRailEnv.obs_global /
MixedBatch.obs_global, rail_env.GlobalObsForRailEnv on this library's RailEnv and plugin.GlobalObsForRailEnv on a duck-typed env --
against the reference's own outputs (tests/golden/global_*.npz) and, at sizes no fixture covers, against the numpy restatement
that tests/test_global_obs_golden.py pins to those goldens."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import util
from tests.global_obs_np import global_obs, rail_obs

pytestmark = pytest.mark.gpu

# the episode fixtures (global_states_*.npz are constructed states: tests/test_global_obs_states.py, tests/test_gpu_global_obs_states.py)
FIXTURES = sorted(os.path.basename(f)[len("global_"):-4] for f in glob.glob(os.path.join(util.GOLD, "global_*.npz"))
                  if not os.path.basename(f).startswith("global_states_"))


def _check_env(ast, tgt, static, state, msg, rail=None):
    """one env's outputs (numpy, float64 or float32) against the restatement"""
    r, a, t = global_obs(static, state)
    dt = ast.dtype
    util.same(ast, a.astype(dt), msg + " agents_state", dtype=True)
    util.same(tgt, t.astype(dt), msg + " targets", dtype=True)
    if rail is not None:
        util.same(rail, r.astype(dt), msg + " rail", dtype=True)


@pytest.mark.parametrize("name", FIXTURES)
def test_batched_replay_equals_the_reference(name):
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    g, fx = util.load("global_" + name), util.load(name)
    env = BatchedRailEnv([util.static_of(fx)])
    steps = [int(t) for t in g["steps"]]
    actions = util.actions_of(fx)
    for t in range(0, max(steps) + 1):
        if t > 0:
            env.step(actions[t - 1][None])
        if t not in steps:
            continue
        k = steps.index(t)
        util.same(env.state()[0][0], g["state"][k], f"{name} t={t} agent state", dtype=True)
        r, ast, tgt = env.obs_global()
        assert r.dtype == torch.float64 and ast.shape == (1, env.A, env.H, env.W, 5) and tgt.shape == (1, env.A, env.H, env.W, 2)
        util.same(r[0].cpu().numpy(), g["rail"], f"{name} t={t} rail f64", dtype=True)
        util.same(ast[0].cpu().numpy(), g["agents_state"][k], f"{name} t={t} agents_state f64", dtype=True)
        util.same(tgt[0].cpu().numpy(), g["targets"][k], f"{name} t={t} targets f64", dtype=True)
        r, ast, tgt = env.obs_global(torch.float32)
        util.same(r[0].cpu().numpy(), g["rail"].astype(np.float32), f"{name} t={t} rail f32", dtype=True)
        util.same(ast[0].cpu().numpy(), g["agents_state"][k].astype(np.float32), f"{name} t={t} agents_state f32", dtype=True)
        util.same(tgt[0].cpu().numpy(), g["targets"][k].astype(np.float32), f"{name} t={t} targets f32", dtype=True)
    env.check()
    env.close()


def test_cfg2_whole_batch_with_auto_reset():
    """256 envs x 20 agents (8 maps, shared static tables), 30 steps of the on-device shortest-path stream with auto-reset, every env
    against the restatement of its state() read-back"""
    import torch
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs("cfg2")
    env = BatchedRailEnv(envs)
    for it in range(1, 31):
        env.step_synth(seed, 0, 2, auto_reset=True)
        dt = torch.float64 if it % 2 else torch.float32
        r, ast, tgt = env.obs_global(dt)
        if it % 5:
            continue
        st, _ = env.state()
        r, ast, tgt = r.cpu().numpy(), ast.cpu().numpy(), tgt.cpu().numpy()
        for b in range(env.B):
            _check_env(ast[b], tgt[b], envs[b], st[b], f"cfg2 it {it} env {b}", rail=r[b])
        assert (st[..., 3] >= 3).any()          # trains on the map
    env.check()
    env.close()


def test_cfg3_in_two_env_chunks_equals_one_call_and_the_restatement():
    import torch
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs("cfg3")
    env = BatchedRailEnv(envs)
    for _ in range(24):
        env.step_synth(seed, 0, 2, auto_reset=True)
    f32 = torch.float32
    r0, a0, t0 = env.obs_global(f32, envs=range(0, 384))
    r1, a1, t1 = env.obs_global(f32, envs=(384, 1024))
    r, a, t = env.obs_global(f32)
    torch.cuda.synchronize()
    assert a0.shape[0] == 384 and a1.shape[0] == 640
    assert torch.equal(torch.cat([r0, r1]), r) and torch.equal(torch.cat([a0, a1]), a) and torch.equal(torch.cat([t0, t1]), t)
    st, _ = env.state()
    assert (st[..., 3] >= 3).any() and (st[..., 3] <= 2).any()
    r, a, t = r.cpu().numpy(), a.cpu().numpy(), t.cpu().numpy()
    for b in range(env.B):
        _check_env(a[b], t[b], envs[b], st[b], f"cfg3 env {b}", rail=r[b])
    # float64: the slab of a 35 x 30 map is more than one LDS band at 80 agents
    rd, ad, td = env.obs_global(torch.float64, envs=slice(1000, 1024))
    for k, b in enumerate(range(1000, 1024)):
        _check_env(ad[k].cpu().numpy(), td[k].cpu().numpy(), envs[b], st[b], f"cfg3 f64 env {b}", rail=rd[k].cpu().numpy())
    env.check()
    env.close()


def test_cfg5_map_larger_than_one_band():
    """150 x 150 / 400 agents: 22 500 cells, far more than one LDS band; the fixture's 40 recorded steps"""
    import torch
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    fx = util.load("cfg5_fwd_head")
    static = util.static_of(fx)
    env = BatchedRailEnv([static])
    actions = util.actions_of(fx)
    for t, row in enumerate(actions):
        env.step(row[None])
        if t + 1 not in (1, len(actions)):
            continue
        st = env.state()[0][0]
        util.same(st, util.golden_state(fx, t), f"cfg5 state t={t + 1}", dtype=True)
        for dt in (torch.float64, torch.float32):
            r, a, g = env.obs_global(dt)
            _check_env(a[0].cpu().numpy(), g[0].cpu().numpy(), static, st, f"cfg5 t={t + 1} {dt}", rail=r[0].cpu().numpy())
    env.check()
    env.close()


def test_rail_channels_follow_a_replaced_map():
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    bases = [util.load("base_cfg2_L%d" % k) for k in range(1, 8)]
    U = max(len(fx["dm_targets"]) for fx in bases)
    R = max(int((fx["grid"] != 0).sum()) for fx in bases)
    envs = [util.static_of(bases[k], *wl.replica_rng(500 + b)) for b, k in enumerate((0, 0, 1))]   # envs 0 and 1 share one map's tables
    env = BatchedRailEnv(envs, reserve=(U, R))
    for _ in range(5):
        env.step_synth(7, 0, 2)
    r, _, _ = env.obs_global()
    util.same(r[1].cpu().numpy(), rail_obs(bases[0]["grid"]), "rail before the replacement", dtype=True)
    envs[1] = util.static_of(bases[4], *wl.replica_rng(900))
    env.replace_env(1, envs[1])
    for _ in range(3):
        env.step_synth(7, 0, 2)
    r, a, t = env.obs_global()
    st, _ = env.state()
    for b in range(3):
        _check_env(a[b].cpu().numpy(), t[b].cpu().numpy(), envs[b], st[b], f"after replacement env {b}", rail=r[b].cpu().numpy())
    assert not np.array_equal(bases[0]["grid"], bases[4]["grid"])
    env.check()
    env.close()


def test_mixed_batch_per_shape_group():
    from flatland_marl_amd.hip_backend import MixedBatch
    names = ("cfg1_sparse", "cfg0_tall_spfollow", "cfg1_malf20_spfollow")
    statics = [util.static_of(util.load(n)) for n in names]
    mb = MixedBatch(statics)
    assert len(mb.groups) == 2
    for _ in range(12):
        mb.step_synth(3, kind=2, auto_reset=True)
    out = mb.obs_global()
    assert len(out) == 2
    for i, s in enumerate(statics):
        r, a, t = mb.pick(i, out)
        st, _ = mb.state(i)
        _check_env(a.cpu().numpy(), t.cpu().numpy(), s, st, f"mixed env {i}", rail=r.cpu().numpy())
    out = mb.obs_global(rail=False)
    assert all(o[0] is None for o in out)
    mb.check()
    mb.close()


@pytest.mark.parametrize("name", ["cfg1_malf20_spfollow", "cfg0_tall_spfollow"])
def test_rail_env_builder_reset_and_step_dicts(name):
    from flatland_marl_amd.rail_env import RailEnv, GlobalObsForRailEnv
    g, fx = util.load("global_" + name), util.load(name)
    builder = GlobalObsForRailEnv()
    env = RailEnv.from_static(util.static_of(fx), obs_builder_object=builder)
    obs, _ = env.reset(regenerate_rail=False, regenerate_schedule=False)
    steps = [int(t) for t in g["steps"]]
    A = env.get_num_agents()
    assert builder.get_many(None) == {}

    def compare(t, obs):
        k = steps.index(t)
        assert sorted(obs) == list(range(A))
        assert all(obs[h][0] is obs[0][0] for h in range(A)), "rail_obs is one array for every handle"
        util.same(obs[0][0], g["rail"], f"{name} t={t} rail", dtype=True)
        for h in range(A):
            util.same(obs[h][1], g["agents_state"][k][h], f"{name} t={t} handle {h} agents_state", dtype=True)
            util.same(obs[h][2], g["targets"][k][h], f"{name} t={t} handle {h} targets", dtype=True)

    compare(0, obs)
    for t, row in enumerate(util.actions_of(fx)[:max(steps)], start=1):
        obs, _, dones, _ = env.step({i: int(a) for i, a in enumerate(row) if a != 255})
        if t in steps:
            compare(t, obs)
    one = builder.get(3)
    util.same(one[1], obs[3][1], "get(handle)", dtype=True)


@pytest.mark.parametrize("name,string_states", [("cfg3_spfollow_malf100", False), ("cfg2_slow_trains", True)])
def test_plugin_on_a_duck_typed_env_replaying_a_reference_episode(name, string_states):
    from flatland_marl_amd.plugin import GlobalObsForRailEnv
    g, fx = util.load("global_" + name), util.load(name)
    env = util.DuckEnv(fx, string_states)
    b = GlobalObsForRailEnv()
    b.set_env(env)
    b.reset()
    A = env.get_num_agents()
    for k, t in enumerate(g["steps"]):
        env.goto(int(t))
        out = b.get_many(list(range(A)))
        assert all(out[h][0] is out[0][0] for h in range(A))
        util.same(out[0][0], g["rail"], f"{name} t={t} rail", dtype=True)
        util.same(np.stack([out[h][1] for h in range(A)]), g["agents_state"][k], f"{name} t={t} agents_state", dtype=True)
        util.same(np.stack([out[h][2] for h in range(A)]), g["targets"][k], f"{name} t={t} targets", dtype=True)
    assert b.get_many(None) == {}


def test_bad_arguments_are_refused_before_anything_is_written():
    import torch
    from flatland_marl_amd import hip_backend as hb
    fx = util.load("cfg1_sparse")
    env = hb.BatchedRailEnv([util.static_of(fx), util.static_of(fx)])
    L = hb.lib()
    H, W, A = env.H, env.W, env.A
    bufs = [torch.full((2 * H * W * 16 + 8,), 7.0, dtype=torch.float64, device=env.device),
            torch.full((2 * A * H * W * 5 + 8,), 7.0, dtype=torch.float64, device=env.device),
            torch.full((2 * A * H * W * 2 + 8,), 7.0, dtype=torch.float64, device=env.device)]
    p = [x.data_ptr() for x in bufs]
    cases = [(-1, 1, 8, p), (0, 0, 8, p), (1, 2, 8, p), (2, 1, 8, p), (0, 1, 2, p), (0, 1, 16, p), (0, 2, 8, [None] * 3),
             (0, 1, 8, [p[0] + 8, p[1], p[2]]), (0, 1, 8, [None, p[1] + 4, None]), (0, 1, 4, [None, None, p[2] + 4])]
    for b0, nb, eb, ptrs in cases:
        rc = L.fl_obs_global(env.h, b0, nb, eb, *[None if q is None else C.c_void_p(q) for q in ptrs])
        assert rc == 1, (b0, nb, eb, rc)          # FL_ERR_ARG
    torch.cuda.synchronize()
    for x in bufs:
        assert bool((x == 7.0).all())
    with pytest.raises(ValueError):
        env.obs_global(envs=(1, 3))
    with pytest.raises(ValueError):
        env.obs_global(torch.int32)
    env.check()
    env.close()
