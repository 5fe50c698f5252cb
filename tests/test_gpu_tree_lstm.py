"""GPU: fl_tree_lstm / policy.TreeLSTM against the reference module's outputs (tests/golden/tree_lstm_*.npz) and against the
float64 restatement (tests/tree_lstm_torch.py) on the observations obs_policy() writes for whole batches."""
import numpy as np
import pytest
import torch

from tests import tree_lstm_torch as tl
from tests.test_tree_lstm_golden import NAMES, golden_inputs, golden_params
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _weights(params):
    from flatland_marl_amd.policy import PARAM_ORDER
    return [params[k].to(DEV).contiguous() for k in PARAM_ORDER]


def _run(inputs, params, roots_only, status=None):
    from flatland_marl_amd import hip_backend as hb
    forest, adjacency, node_order, edge_order = inputs
    B, A, N = node_order.shape
    rows = B * A if roots_only else B * A * N
    h = torch.full((rows, 128), float("nan"), device=DEV)
    c = torch.full((rows, 128), float("nan"), device=DEV)
    hb.tree_lstm(forest, adjacency, node_order, edge_order, _weights(params), roots_only, h, c, status)
    return h, c


def _close(h, c, gh, gc, what):
    h, c = h.double().cpu().numpy(), c.double().cpu().numpy()
    assert np.abs(h - gh).max() <= 1e-5, (what, np.abs(h - gh).max())
    assert (np.abs(c - gc) <= 1e-5 * np.maximum(1.0, np.abs(gc))).all(), (what, np.abs(c - gc).max())


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_reference_goldens(name):
    g = np.load(util.GOLD + "/tree_lstm_%s.npz" % name)
    inputs = [x.to(DEV).contiguous() for x in golden_inputs(g)]
    B, A, N = inputs[2].shape
    T, ids = B * A, list(g["tree_ids"])
    pad = (inputs[2] == -2).view(T, N)
    for s, scale in enumerate(g["scales"]):
        params = golden_params(g, scale)
        h, c = _run(inputs, params, False)
        h, c = h.view(T, N, 128), c.view(T, N, 128)
        _close(h[:, 0], c[:, 0], g["root_h"][s], g["root_c"][s], (name, scale, "roots of all-node mode"))
        _close(h[ids], c[ids], g["all_h"][s], g["all_c"][s], (name, scale, "whole trees"))
        assert (h[pad] == 0).all() and (c[pad] == 0).all()
        hr, cr = _run(inputs, params, True)
        _close(hr, cr, g["root_h"][s], g["root_c"][s], (name, scale, "roots only"))
        assert torch.equal(hr, h[:, 0]) and torch.equal(cr, c[:, 0])


def _module(seed=1, scale=1.0):
    from flatland_marl_amd.policy import TreeLSTM
    m = TreeLSTM().to(DEV)
    m.load_state_dict(tl.seeded_params(seed, scale))
    return m


def _golden_dev(name="cfg2_uniform"):
    g = np.load(util.GOLD + "/tree_lstm_%s.npz" % name)
    return [x.to(DEV).contiguous() for x in golden_inputs(g)]


def test_roots_equal_forward_and_runs_bit_identical():
    m = _module(scale=4.0)
    x = _golden_dev()
    B, A, N = x[2].shape
    with torch.no_grad():
        full = m(*x)
        roots = m.roots(*x)
        assert full.shape == (B * A * N, 128) and roots.shape == (B, A, 128)
        assert torch.equal(roots, full.view(B, A, N, 128)[:, :, 0])
        assert torch.equal(m(*x), full) and torch.equal(m.roots(*x), roots)


def _check_batch(env, m, steps, seed):
    params = dict(m.named_parameters())
    for k in range(steps[-1] + 1):
        env.step_synth(seed, 0, 2, auto_reset=True)
        if k not in steps:
            continue
        _, forest, adj, no, eo = env.obs_policy()
        with torch.no_grad():
            h = m(forest, adj, no, eo, check=True)                # (the kernel's own check of the grouping: no violation)
            r = m.roots(forest, adj, no, eo)
        exp_h = tl.tree_lstm(forest, adj, no, eo, params)
        assert (h.double() - exp_h).abs().max().item() <= 1e-5
        B, A, N = no.shape
        assert torch.equal(r, h.view(B, A, N, 128)[:, :, 0])
        assert (h.view(B * A, N, 128)[(no == -2).view(B * A, N)] == 0).all()


@pytest.mark.parametrize("workload, B, max_nodes", [("cfg2", None, 31), ("cfg3", 128, 31), ("cfg2", 64, 64)])
def test_obs_policy_batches_match_the_restatement(workload, B, max_nodes):
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs(workload, B=B) if B else wl.make_envs(workload)
    env = BatchedRailEnv(envs, max_nodes=max_nodes)
    try:
        _check_batch(env, _module(seed=3, scale=2.0), (0, 7, 30), seed)
    finally:
        env.close()


def test_no_host_sync_in_forward():
    m = _module()
    x = _golden_dev("cfg3_uniform")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            m(*x)
            m.roots(*x)
        m(*x)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_load_state_dict_between_forwards():
    m = _module(seed=5)
    x = _golden_dev()
    with torch.no_grad():
        a = m(*x).clone()
        p2 = tl.seeded_params(6, 4.0)
        m.load_state_dict(p2)
        b = m(*x)
        assert not torch.equal(a, b)
        assert (b.double() - tl.tree_lstm(*x, p2)).abs().max().item() <= 1e-5
        m.U_iou.weight.mul_(0.5)                                  # an in-place update: the next forward sees it
        p3 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        assert (m(*x).double() - tl.tree_lstm(*x, p3)).abs().max().item() <= 1e-5


def test_broken_triple_is_counted_and_check_raises():
    from flatland_marl_amd.policy import TreeLSTMViolation
    m = _module()
    forest, adj, no, eo = _golden_dev()
    B, A, N = no.shape
    adj = adj.clone()
    flat = adj.view(B * A, N - 1, 3)
    t = 5
    e = int((eo.view(B * A, N - 1)[t] >= 1).nonzero()[0])       # an edge of a node of height >= 1: move it to another parent
    flat[t, e, 0] = t * N + int((no.view(B * A, N)[t] == 0).nonzero()[0])
    assert tl.triple_rule_violations(adj, no, eo).view(-1).nonzero().flatten().tolist() == [t]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _run((forest, adj, no, eo), tl.seeded_params(1), False, status)
    assert int(status.item()) == 1
    with torch.no_grad():
        with pytest.raises(TreeLSTMViolation):
            m(forest, adj, no, eo, check=True)
        m(forest, adj, no, eo)                                    # not checked: runs, the tree's outputs are unspecified
    bad_no = no.clone()
    bad_no.view(B * A, N)[2, 4] = N + 3
    status.zero_()
    _run((forest, adj, bad_no, eo), tl.seeded_params(1), True, status)
    assert int(status.item()) == 2


def test_backward_raises_and_detach_works():
    m = _module()
    x = _golden_dev()
    out = m(*x)
    assert out.requires_grad
    d = out.detach()
    with torch.no_grad():
        assert torch.equal(d, m(*x))
    with pytest.raises(NotImplementedError):
        out.sum().backward()


def test_input_checks():
    m = _module()
    forest, adj, no, eo = _golden_dev()
    with pytest.raises(TypeError):
        m(forest.double(), adj, no, eo)
    with pytest.raises(TypeError):
        m(forest, adj.int(), no, eo)
    with pytest.raises(TypeError):
        m(forest.cpu(), adj, no, eo)
    with pytest.raises(ValueError):
        m(forest, adj[:, :, :-1].contiguous(), no, eo)
    with pytest.raises(ValueError):
        m(forest.transpose(0, 1), adj, no, eo)
