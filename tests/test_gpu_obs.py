"""GPU parity (through the C-ABI): HIP observation kernels vs golden tensors captured from the reference's
flatland_cutils module / upstream TreeObsForRailEnv, and vs the CPU oracle on batched seeded runs.
Bit-exact: integer outputs and float32/float64 features alike."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

CUTILS_KEYS = (("agent_attr", "o_attr"), ("forest", "o_forest"), ("adjacency", "o_adjacency"),
               ("node_order", "o_node_order"), ("edge_order", "o_edge_order"), ("valid_actions", "o_valid"))


@pytest.mark.parametrize("name", util.episode_fixtures())
def test_obs_match_reference_golden(name):
    import torch
    fx = util.load(name)
    env = util.batched([util.static_of(fx)])
    obs_steps = {int(t): k for k, t in enumerate(fx["obs_steps"])}
    py_steps = {int(t): k for k, t in enumerate(fx["py_steps"])} if "py_steps" in fx.files else {}
    pykeys = [k for k in fx.files if k.startswith("py_d")]

    def check(t):
        o = env.obs_cutils()     # every step: the deadlock flags are sticky and advance once per get_many()
        if t in obs_steps:
            k = obs_steps[t]
            for got, key in CUTILS_KEYS:
                util.same(o[got].cpu().numpy()[0], fx[key][k], f"{name} t={t} {got}")
            pr = o["props"].cpu().numpy()[0]
            util.same(pr[:, 0], fx["o_p_dist_target"][k], f"{name} t={t} dist_target")
            util.same(pr[:, 1], fx["o_p_deadlocked"][k], f"{name} t={t} deadlocked")
            util.same(pr[:, 2], fx["o_p_ready"][k], f"{name} t={t} ready")
        if t in py_steps:
            k = py_steps[t]
            for pk in pykeys:
                depth, pdepth = int(pk.split("_")[1][1:]), int(pk.split("_")[2][1:])
                got = env.obs_tree(depth, pdepth).cpu().numpy()[0]
                util.same(got, fx[pk][k], f"{name} t={t} {pk}")

    check(0)
    for t, a in enumerate(util.actions_of(fx)):
        env.step(torch.from_numpy(a[None, :].copy()).cuda())
        check(t + 1)
    env.check()


def _replica_rng(b):
    st = np.random.RandomState([b]).get_state()
    return np.array(st[1], dtype=np.uint32), int(st[2])


@pytest.mark.parametrize("bases,B,steps,malf_rate,tree", [
    (["base_cfg2_L1", "base_cfg2_L2", "base_cfg2_L3", "base_cfg2_L6"], 16, 260, None, (2, 30)),
    (["base_cfg2_L4", "base_cfg2_L7"], 8, 200, 1 / 30.0, (3, 20)),
    (["base_cfg3_L1", "base_cfg3_L3"], 4, 150, 1 / 200.0, (2, 30)),
])
def test_batched_obs_match_oracle(bases, B, steps, malf_rate, tree):
    from oracle import orc
    from flatland_marl_amd import synth
    fxs = [util.load(n) for n in bases]
    envs, oracles = [], []
    for b in range(B):
        key, pos = _replica_rng(100 + b)
        st = util.static_of(fxs[b % len(fxs)], key, pos)
        if malf_rate is not None:
            st["malf_rate"] = malf_rate
        envs.append(st)
        oracles.append(orc.OracleEnv(st))
    env = util.batched(envs)
    A = env.A
    seed = 5
    tcount = np.zeros(B, dtype=np.int64)
    for it in range(steps):
        kind = 1 if it < steps // 2 else 0      # forward-biased first (agents spread out), then uniform
        env.step_synth(seed, stream_base=0, kind=kind, auto_reset=True)
        o = {k: v.cpu().numpy() for k, v in env.obs_cutils().items()}
        tr = env.obs_tree(*tree).cpu().numpy() if it % 7 == 0 else None
        for b in range(B):
            orc_env = oracles[b]
            fn = synth.forward_biased_actions if kind == 1 else synth.uniform_actions
            _, _, da = orc_env.step(fn(seed, b, int(tcount[b]), A))
            tcount[b] += 1
            if da:
                key, pos = orc_env.get_rng()
                oracles[b] = orc.OracleEnv(envs[b])
                oracles[b].set_rng(key, pos)
                tcount[b] = 0
                # the oracle's fresh env has clean deadlock flags, like the auto-reset on the device
                # (state after the terminal step is compared below before the swap takes effect next step)
            exp = orc_env.obs_cutils(31, 500)
            for got, key in (("agent_attr", "attr"), ("forest", "forest"), ("adjacency", "adjacency"),
                             ("node_order", "node_order"), ("edge_order", "edge_order"), ("valid_actions", "valid"),
                             ("props", "props")):
                util.same(o[got][b], exp[key], f"replica {b} iter {it} {got}")
            if tr is not None:
                util.same(tr[b], orc_env.obs_pytree(*tree), f"replica {b} iter {it} tree{tree}")
    env.check()
