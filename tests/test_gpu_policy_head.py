"""GPU: fl_policy_head / policy.Network against the float64 restatement (tests/policy_head_torch.py) run on the device, and its
actions against the reference's (tests/golden/policy_head_*.npz).

Tolerance: per case (fixture, weight scale) e32 = the error of the reference's float32 forward against the float64 restatement,
stored at capture; the kernel passes when its error is at most R * e32 + one float32 ulp of the largest |output| of the case.
R = 9, set on 2026-10-18 from tests/golden/policy_head_errors.json (MI355X): twice the largest ratio recorded there (4.17), rounded
up to an integer (ratio = (error - the ulp floor, at least 0) / e32).  POLICY_HEAD_ERRORS=<path> makes test_fixture write its
figures to <path> in that file's format.  Of the 40 ratios 32 are below 1.7; the six above 2.1 are all of the two fixtures with ONE
agent an env (synth_b1_a1: 2.71 / 3.48 and 2.43 / 2.42, synth_b3_a1: 4.17 in value at scale 1 and 2.34 in logits), where a case has
1 to 15 outputs and e32 is one draw of the reference's error, not its size (3.4e-9 on values of 0.07, under half an ulp, against
1.8e-8 of the kernel).  torch's eager float32 ops on the same GPU sit at 3.07 and 3.48 on the same cases and at 19.8 on the value
of synth_b1_a1 at the second scale, so the ratios there say little about the kernel's accumulation order; with 7 agents or more
the kernel's largest ratio is 2.04 and eager torch's 2.45.
"""
import os

import numpy as np
import pytest
import torch

from tests import policy_head_torch as ph
from tests import util
from tests.test_policy_head_golden import NAMES, golden_inputs, golden_params, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 9


def _net(params):
    from flatland_marl_amd.policy import Network
    net = Network().to(DEV)
    net.load_state_dict(params)
    return net


def _ratio(err, e32, out):
    floor = ph.tolerance(0.0, out)
    return max(0.0, err - floor) / e32


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name, s):
    """logits and value against the float64 restatement on the device; actions against the reference's, both modes; forward_torch's
    head within the same tolerance"""
    g = load(name)
    params = golden_params(g, s)
    net = _net(params)
    attr, tree, valid = (x.to(DEV).contiguous() for x in golden_inputs(g, s))
    B, A = attr.shape[:2]
    with torch.no_grad():
        (logits,), value, soft = net.head(attr, tree, valid, "soft")
        (logits2,), value2, hard = net.head(attr, tree, valid, "hard")
        (lt,), vt = net.head_torch(attr, tree)
    assert logits.shape == (B, A, 5) and value.shape == (B,) and soft.shape == (B, A) and soft.dtype == torch.uint8
    assert torch.equal(logits, logits2) and torch.equal(value, value2)              # two runs: the same bits
    l64, v64 = ph.head(attr, tree, params)
    err_l, err_v = float((logits.double() - l64).abs().max()), float((value.double() - v64).abs().max())
    e32_l, e32_v = float(g["e32_logits"][s]), float(g["e32_value"][s])
    figs = dict(err_logits=err_l, e32_logits=e32_l, ratio_logits=_ratio(err_l, e32_l, g["logits"][s]),
                err_value=err_v, e32_value=e32_v, ratio_value=_ratio(err_v, e32_v, g["value"][s]))
    print(name, "x%d" % s, " ".join("%s %.3g" % kv for kv in figs.items()))
    util.record_errors("POLICY_HEAD_ERRORS", "cases", "%s-x%d" % (name, s), figs)
    tol_l, tol_v = ph.tolerance(e32_l, g["logits"][s], R), ph.tolerance(e32_v, g["value"][s], R)
    terr_l, terr_v = float((lt.double() - l64).abs().max()), float((vt.double() - v64).abs().max())
    print(name, "x%d" % s, "head_torch: err_logits %.3g (ratio %.3g) err_value %.3g (ratio %.3g)"
          % (terr_l, _ratio(terr_l, e32_l, g["logits"][s]), terr_v, _ratio(terr_v, e32_v, g["value"][s])))
    assert err_l <= tol_l and err_v <= tol_v, figs
    # torch's eager ops on the same device: another float32 summation order, held to the same bound wherever e32 is the size of an
    # error and not one draw of it -- with a single agent an env every output is a single number
    if A >= 7:
        assert terr_l <= tol_l and terr_v <= tol_v, (terr_l, tol_l, terr_v, tol_v)
    # the reference's outputs themselves
    assert float((logits.cpu() - torch.from_numpy(g["logits"][s])).abs().max()) <= tol_l + e32_l
    # actions: the reference's on every agent that eps of error in the logits cannot change; 0 without a valid action
    none = g["valid"].sum(-1) == 0
    for mode, got in (("soft", soft), ("hard", hard)):
        got = got.cpu().numpy()
        ex = ph.exempt(g["logits"][s], g["valid"], mode, tol_l)
        assert ex.sum() <= 0.01 * ex.size
        assert (got == g[mode][s])[~ex].all(), (mode, np.flatnonzero((got != g[mode][s]) & ~ex))
        assert (got[none] == 0).all()
        # ... and the restated choice on the kernel's own logits, for every agent
        assert (got == ph.choose_actions(logits, valid, mode)).all()


def _pair(seed=1, B=2, A=20, scale=(2.5, 3.5)):
    attr, tree, valid = (torch.from_numpy(x).to(DEV) for x in ph.synth_inputs(B, A, seed))
    return attr, tree, valid, ph.seeded_params(7, scale)


def test_envs_are_isolated():
    """replacing env 1's inputs leaves env 0's logits, value and actions bit-identical (A = 20: the 32-row tile straddles the envs)"""
    attr, tree, valid, params = _pair()
    net = _net(params)
    a2, t2, v2 = attr.clone(), tree.clone(), valid.clone()
    a2[1], t2[1], v2[1] = torch.randn_like(a2[1]) * 3, torch.randn_like(t2[1]), 1 - v2[1]
    with torch.no_grad():
        for mode in ("soft", "hard"):
            (l0,), val0, act0 = net.head(attr, tree, valid, mode)
            (l1,), val1, act1 = net.head(a2, t2, v2, mode)
            assert torch.equal(l0[0], l1[0]) and torch.equal(val0[0], val1[0]) and torch.equal(act0[0], act1[0])
            assert not torch.equal(l0[1], l1[1]) and not torch.equal(val0[1], val1[1])
            (l0b,), val0b, act0b = net.head(attr, tree, valid, mode)
            assert torch.equal(l0, l0b) and torch.equal(val0, val0b) and torch.equal(act0, act0b)
        # an env alone gives what it gives in the batch
        (la,), va_, aa = net.head(attr[:1].contiguous(), tree[:1].contiguous(), valid[:1].contiguous(), "soft")
        (lb,), vb, ab = net.head(attr, tree, valid, "soft")
        assert torch.equal(la[0], lb[0]) and torch.equal(va_[0], vb[0]) and torch.equal(aa[0], ab[0])


def test_head_options_and_guards():
    """select = 0 with NULL mask and actions, a NULL value pointer; nothing is written past the outputs; u is used"""
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd.policy import HEAD_PARAM_ORDER
    attr, tree, valid, params = _pair(seed=2, B=3, A=33)
    net = _net(params)
    ws = [dict(net.named_parameters())[k].detach() for k in HEAD_PARAM_ORDER]
    B, A = 3, 33
    with torch.no_grad():
        (ref,), vref, aref = net.head(attr, tree, valid, "soft")
        (l1,), v1 = net.head(attr, tree)
        (l2,), v2 = net.head(attr, tree, value=False)
        assert torch.equal(l1, ref) and torch.equal(v1, vref) and torch.equal(l2, ref) and v2 is None
    lbuf = torch.full((B * A * 5 + 64,), float("nan"), device=DEV)
    vbuf = torch.full((B + 64,), float("nan"), device=DEV)
    abuf = torch.full((B * A + 64,), 77, dtype=torch.uint8, device=DEV)
    hb.policy_head(attr, tree, ws, lbuf[:B * A * 5], vbuf[:B], valid, abuf[:B * A], "soft")
    assert torch.equal(lbuf[:B * A * 5].view(B, A, 5), ref) and torch.equal(vbuf[:B], vref) and torch.equal(abuf[:B * A].view(B, A), aref)
    assert torch.isnan(lbuf[B * A * 5:]).all() and torch.isnan(vbuf[B:]).all() and (abuf[B * A:] == 77).all()
    logits = torch.empty((B, A, 5), device=DEV)
    hb.policy_head(attr, tree, ws, logits)                                 # no value, no mask, no actions
    assert torch.equal(logits, ref)
    for u in (0.0, 0.05, 0.5, 0.95, 0.999999):
        with torch.no_grad():
            got = net.head(attr, tree, valid, "soft", u=u)[2]
        assert (got.cpu().numpy() == ph.choose_actions(ref, valid, "soft", u=u)).all()
    with pytest.raises(ValueError):
        net.head(attr, tree, valid, "soft", u=1.0)
    with pytest.raises(ValueError):
        net.head(attr, tree, valid, "softest")
    with pytest.raises(ValueError):
        net.head(attr, tree, None, "soft")


def _golden_obs(name="cfg2_uniform"):
    from tests.test_tree_lstm_golden import golden_inputs as tree_inputs
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "tree_lstm_%s.npz" % name))
    forest, adj, no, eo = (x.to(DEV).contiguous() for x in tree_inputs(fx))
    ep = np.load(os.path.join(os.path.dirname(__file__), "golden", "%s.npz" % name))
    idx, a = list(fx["obs_index"]), int(fx["agents"])
    attr = torch.from_numpy(np.ascontiguousarray(ep["o_attr"][idx, :a])).to(DEV)
    valid = torch.from_numpy(np.ascontiguousarray(ep["o_valid"][idx, :a])).to(DEV)
    return attr, forest, adj, no, eo, valid


def test_head_equals_forward_and_act():
    net = _net(ph.seeded_params(3, 3.0))
    attr, forest, adj, no, eo, valid = _golden_obs()
    with torch.no_grad():
        (logits,), value = net(attr, forest, adj, no, eo)
        tree = net.tree_lstm.roots(forest, adj, no, eo)
        (l2,), v2, soft = net.head(attr, tree, valid, "soft")
        assert torch.equal(logits, l2) and torch.equal(value, v2)
        for mode, exp in (("soft", soft), ("hard", net.head(attr, tree, valid, "hard")[2])):
            got = net.act(attr, forest, adj, no, eo, valid, mode)
            assert got.dtype == torch.uint8 and got.shape == valid.shape[:2] and torch.equal(got, exp)
        (lt,), vt = net.forward_torch(attr, forest, adj, no, eo)
    l64, v64 = ph.head(attr, tree, dict(net.named_parameters()))
    e32 = float((ph.head(attr, tree, dict(net.named_parameters()), dtype=torch.float32)[0].double() - l64).abs().max())
    tol = ph.tolerance(e32, l64.cpu().numpy(), R)
    assert float((logits.double() - l64).abs().max()) <= tol and float((lt.double() - l64).abs().max()) <= tol


def test_end_to_end_episode_on_the_device():
    """obs_policy -> Network.act -> step for 10 steps of cfg2 x 8, no host synchronisation in act; logits at three steps"""
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs("cfg2", B=8)
    env = BatchedRailEnv(envs)
    net = _net(ph.seeded_params(5, 3.0))
    params = dict(net.named_parameters())
    try:
        seen = set()
        for k in range(10):
            attr, forest, adj, no, eo = env.obs_policy()
            valid = env.obs_outputs()["valid_actions"]
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                actions = net.act(attr, forest, adj, no, eo, valid)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            if k in (0, 4, 9):
                with torch.no_grad():
                    (logits,), value = net(attr, forest, adj, no, eo)
                    tree = net.tree_lstm.roots(forest, adj, no, eo)
                l64, v64 = ph.head(attr, tree, params)
                l32, v32 = ph.head(attr, tree, params, dtype=torch.float32)
                e32 = float((l32.double() - l64).abs().max())
                assert float((logits.double() - l64).abs().max()) <= ph.tolerance(e32, l64.cpu().numpy(), R)
                assert (actions.cpu().numpy() == ph.choose_actions(logits, valid, "soft")).all()
            assert actions.shape == (env.B, env.A) and int(actions.max()) <= 4
            seen |= set(actions.unique().tolist())
            env.step(actions, filter_required=True)
        env.check()
        assert len(seen) >= 2
    finally:
        env.close()


def test_parameter_updates_are_seen():
    attr, tree, valid, params = _pair(seed=4)
    net = _net(params)
    with torch.no_grad():
        a = net.head(attr, tree)[0][0].clone()
        p2 = ph.seeded_params(8, (2.5, 3.5))
        net.load_state_dict(p2)
        b = net.head(attr, tree)[0][0]
        assert not torch.equal(a, b)
        l64, _ = ph.head(attr, tree, p2)
        e32 = float((ph.head(attr, tree, p2, dtype=torch.float32)[0].double() - l64).abs().max())
        assert float((b.double() - l64).abs().max()) <= ph.tolerance(e32, l64.cpu().numpy(), R)
        net.actor_net[4].weight.mul_(0.5)                                     # an in-place update: the next forward sees it
        net.transformer[1].attention.in_proj_weight.mul_(0.9)
        p3 = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        l64, _ = ph.head(attr, tree, p3)
        c = net.head(attr, tree)[0][0]
        assert not torch.equal(b, c)
        assert float((c.double() - l64).abs().max()) <= ph.tolerance(e32, l64.cpu().numpy(), R)


def test_backward_raises_and_forward_torch_has_autograd():
    attr, tree, valid, params = _pair(seed=5)
    net = _net(params)
    (logits,), value = net.head(attr, tree)
    assert logits.requires_grad
    with pytest.raises(NotImplementedError):
        (logits.sum() + value.sum()).backward()
    (lt,), vt = net.head_torch(attr, tree)
    (lt.sum() + vt.sum()).backward()
    assert net.actor_net[0].weight.grad is not None and net.transformer[0].attention.in_proj_weight.grad is not None


def test_input_checks():
    attr, tree, valid, params = _pair(seed=6)
    net = _net(params)
    with pytest.raises(TypeError):
        net.head(attr.double(), tree)
    with pytest.raises(TypeError):
        net.head(attr, tree.half())
    with pytest.raises(TypeError):
        net.head(attr.cpu(), tree)
    with pytest.raises(TypeError):
        net.head(attr, tree, valid.int(), "soft")
    with pytest.raises(ValueError):
        net.head(attr, tree[:, :-1].contiguous())
    with pytest.raises(ValueError):
        net.head(attr.transpose(0, 1), tree)
    with pytest.raises(ValueError):
        net.head(attr, tree, valid[:, :, :4].contiguous(), "soft")
    net.actor_net[0].weight.data = net.actor_net[0].weight.data.double()
    with pytest.raises(TypeError):
        net.head(attr, tree)
