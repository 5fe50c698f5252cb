"""GPU parity through the C-ABI's state-injection and MotionCheck entry points:

* fl_motion_check: the 3002 known-answer cases captured from the reference's MotionCheck (its own scenario builders,
  agent_chains.py:302-415, plus a fuzz with agents sharing a cell) run through the conflict resolution of the step kernel;
* fl_set_state: every observation snapshot of the reference goldens is reproduced by INJECTING the agent state of that
  step (no replay of the episode), the way flatland_cutils' AgentsLoader reads a caller-owned env (loader.cpp:221-327);
* fl_get_state / fl_get_state_aux / fl_get_rng -> fl_set_state / fl_set_rng: a mid-episode hand-over to a fresh batch
  continues bit for bit (RailEnvPersister.set_full_state, persistence.py:182-222)."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

CUTILS_KEYS = (("agent_attr", "o_attr"), ("forest", "o_forest"), ("adjacency", "o_adjacency"),
               ("node_order", "o_node_order"), ("edge_order", "o_edge_order"), ("valid_actions", "o_valid"))


def test_motion_check_known_answers_through_the_step_kernel():
    from flatland_marl_amd import hip_backend as hb
    z = util.load("motioncheck")
    off = z["offsets"]
    cur, nxt = z["cur"].astype(np.int64), z["nxt"].astype(np.int64)
    # the capture script numbers the private virtual node of agent i of a case 100000 + i; the C-ABI takes -1 for it
    for k in range(len(off) - 1):
        i = np.arange(off[k + 1] - off[k])
        for arr in (cur, nxt):
            seg = arr[off[k]:off[k + 1]]
            virt = seg >= 100000
            assert (seg[virt] == 100000 + i[virt]).all()
    cur[cur >= 100000] = -1
    nxt[nxt >= 100000] = -1
    got = hb.motion_check(off, cur, nxt)
    bad = np.nonzero(got != z["can_move"].astype(bool))[0]
    assert len(bad) == 0, f"{len(bad)} agents differ, first in case {np.searchsorted(off, bad[0], side='right') - 1}"
    assert len(off) - 1 == 3002


def test_motion_check_wide_case_matches_oracle():
    """1000 agents on a ring / chains with contention and stacked cells: beyond what the fuzz covers in size."""
    from oracle import orc
    from flatland_marl_amd import hip_backend as hb
    rng = np.random.default_rng(3)
    n = 1000
    cells = rng.permutation(4000)[:n].astype(np.int64)
    cur = cells.copy()
    cur[rng.random(n) < 0.15] = -1
    stacked = rng.random(n) < 0.05
    cur[stacked] = cur[rng.integers(0, n, stacked.sum())]
    nxt = np.where(rng.random(n) < 0.2, cur, np.where(rng.random(n) < 0.5, np.roll(cells, 1), rng.integers(0, 4000, n)))
    nxt[(cur < 0) & (rng.random(n) < 0.5)] = -1
    o_cur = np.where(cur < 0, 100000 + np.arange(n), cur)
    o_nxt = np.where(nxt < 0, 100000 + np.arange(n), nxt)
    exp = orc.motion_check(o_cur, o_nxt)
    got = hb.motion_check(np.array([0, n]), cur, nxt)
    util.same(got, exp, "wide case")


def _aux_of(fx, T, k_obs=None):
    """aux columns of the state after T steps of a golden episode (see fl_get_state_aux)."""
    A = len(fx["init_dir"])
    aux = np.zeros((A, 4), dtype=np.int32)
    aux[:, 0] = -1
    malf_now = fx["s_malf"][T - 1]
    malf_before = fx["s_malf"][T - 2] if T >= 2 else np.zeros(A, dtype=np.int32)
    # in_malfunction was evaluated before the counter ticked down: it held if the counter is still positive, or just expired
    # (malfunction durations of the fixtures are >= 21 steps, so a counter at 0 was 1 a step ago or idle)
    assert int(fx["malf_min"]) >= 1
    aux[:, 1] = (malf_now > 0) | (malf_before == 1)
    if k_obs is not None:
        aux[:, 2] = fx["o_p_deadlocked"][k_obs].astype(np.int32)   # sticky flags: re-deriving them from themselves is idempotent
    aux[:, 3] = fx["s_done"][T - 1]
    return aux


@pytest.mark.parametrize("name", ["cfg3_uniform", "cfg3_spfollow_malf100", "cfg2_spfollow", "cfg1_malf20_spfollow", "cfg0_tall_spfollow"])
def test_injected_reference_states_reproduce_the_observation_snapshots(name):
    fx = util.load(name)
    env = util.batched([util.static_of(fx)])
    obs_steps = [int(t) for t in fx["obs_steps"]]
    py_steps = {int(t): k for k, t in enumerate(fx["py_steps"])} if "py_steps" in fx.files else {}
    pykeys = [k for k in fx.files if k.startswith("py_d")]
    n = 0
    for k, T in enumerate(obs_steps):
        if T == 0:
            continue
        env.set_state(util.golden_state(fx, T - 1)[None], _aux_of(fx, T, k)[None], np.array([T], dtype=np.int32),
                      np.array([fx["done_all"][T - 1]], dtype=np.uint8))
        o = env.obs_cutils()
        for got, key in CUTILS_KEYS:
            util.same(o[got].cpu().numpy()[0], fx[key][k], f"{name} T={T} {got}")
        pr = o["props"].cpu().numpy()[0]
        util.same(pr[:, 0], fx["o_p_dist_target"][k], f"{name} T={T} dist_target")
        util.same(pr[:, 1], fx["o_p_deadlocked"][k], f"{name} T={T} deadlocked")
        util.same(pr[:, 2], fx["o_p_ready"][k], f"{name} T={T} ready")
        n += 1
    for T, k in py_steps.items():
        if T == 0:
            continue
        env.set_state(util.golden_state(fx, T - 1)[None], _aux_of(fx, T)[None], np.array([T], dtype=np.int32))
        for pk in pykeys:
            depth, pdepth = int(pk.split("_")[1][1:]), int(pk.split("_")[2][1:])
            util.same(env.obs_tree(depth, pdepth).cpu().numpy()[0], fx[pk][k], f"{name} T={T} {pk}")
    env.check()
    assert n >= 3


def test_mid_episode_hand_over_to_a_fresh_batch_continues_bit_for_bit():
    """state + aux + RNG read from a running batch and injected into a new one: both continue identically (step outputs,
    observations with their sticky deadlock flags, RNG), through an auto-reset."""
    fxs = [util.load(n) for n in ("base_cfg3_L1", "base_cfg3_L2")]
    envs = []
    for b in range(4):
        st = util.static_of(fxs[b % 2])
        st["malf_rate"] = 1 / 80.0
        st["mt_key"], st["mt_pos"] = (lambda s: (np.array(s[1], dtype=np.uint32), int(s[2])))(np.random.RandomState([40 + b]).get_state())
        envs.append(st)
    e1 = util.batched(envs)
    for t in range(230):
        e1.step_synth(17, 5, 1, auto_reset=True)
        e1.obs_cutils()
    st, el = e1.state()
    aux = e1.state_aux()
    key, pos = e1.rng_state()
    assert (st[:, :, 0] >= 0).sum() > 20 and aux[:, :, 2].sum() >= 0
    e2 = util.batched(envs)
    e2.set_state(st, aux, el, e1.done_all.cpu().numpy())
    e2.set_rng_state(key, pos)
    np.testing.assert_array_equal(e2.state()[0], st)
    np.testing.assert_array_equal(e2.state_aux(), aux)
    T = int(max(e["T"] for e in envs))
    for t in range(T - 150):
        r1, d1, a1 = (x.clone() for x in e1.step_synth(17, 5, 0, auto_reset=True))
        r2, d2, a2 = e2.step_synth(17, 5, 0, auto_reset=True)
        # the synthetic stream is indexed by the env's own step counter, which the injection carried over
        util.same(r2.cpu().numpy(), r1.cpu().numpy(), f"t={t} rewards")
        util.same(d2.cpu().numpy(), d1.cpu().numpy(), f"t={t} dones")
        util.same(a2.cpu().numpy(), a1.cpu().numpy(), f"t={t} done_all")
        o1 = {k: v.clone() for k, v in e1.obs_cutils().items()}
        o2 = e2.obs_cutils()
        if t % 5 == 0:
            util.same(e2.state()[0], e1.state()[0], f"t={t} state")
            for k in o1:
                util.same(o2[k].cpu().numpy(), o1[k].cpu().numpy(), f"t={t} {k}")
    assert int(e1.metrics().cpu().numpy()[3]) >= 4          # every env finished an episode on the way
    k1, p1 = e1.rng_state()
    k2, p2 = e2.rng_state()
    util.same(k2, k1, "mt key")
    util.same(p2, p1, "mt pos")
    e1.check(); e2.check()


def test_set_state_refuses_a_state_position_mismatch():
    from flatland_marl_amd.hip_backend import FlatlandHipError
    fx = util.load("cfg1_uniform")
    env = util.batched([util.static_of(fx)])
    st, _ = env.state()
    st[0, 0, 3] = 3          # MOVING without a position (env_utils.py:45-52)
    with pytest.raises(FlatlandHipError, match="FL_ERR_STATE_SYNC"):
        env.set_state(st)
    st[0, 0, 3] = 9
    with pytest.raises(FlatlandHipError, match="FL_ERR_ARG"):
        env.set_state(st)


def test_finished_env_inside_a_batch_reports_zero_rewards_and_done():
    """an env whose episode is over (no auto-reset) must not leave its terminal rewards in the output tensors
    while the rest of the batch advances; _elapsed_steps still counts the refused step (rail_env.py:505-509)."""
    import torch
    from flatland_marl_amd.hip_backend import EpisodeDoneError
    fx = util.load("cfg1_spfollow")
    st = util.static_of(fx)
    long = dict(st)
    long["T"] = np.int32(int(st["T"]) + 50)
    env = util.batched([st, long])
    acts = util.actions_of(fx)
    idle = np.zeros_like(acts[0])            # env 1 never departs, so it outlives env 0
    for a in acts:
        rew, done, done_all = env.step(torch.from_numpy(np.stack([a, idle])).cuda())
    assert done_all.cpu().numpy().tolist() == [1, 0]
    assert (rew.cpu().numpy()[0] != 0).any()                 # env 0's terminal rewards are in the tensors now
    env.check()
    rew, done, done_all = env.step(torch.from_numpy(np.stack([acts[-1], idle])).cuda())
    assert (rew.cpu().numpy()[0] == 0).all() and (done.cpu().numpy()[0] == 1).all()
    assert done_all.cpu().numpy().tolist() == [1, 0]
    assert env.state()[1].tolist() == [len(acts) + 1, len(acts) + 1]
    with pytest.raises(EpisodeDoneError):
        env.check()
