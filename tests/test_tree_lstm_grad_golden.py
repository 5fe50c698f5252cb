"""CPU: the differentiable TreeLSTM restatement (tests/tree_lstm_grad_torch.py) under autograd against the reference module's own
float64 gradients (tests/golden/grad_tree_lstm_*.npz, tools/capture_tree_lstm_grads.py), include/flatland_train.h against its
ctypes binding and the built library, fl_tree_lstm_backward's refusals (which come before any HIP call and so need no GPU), and
policy.TreeLSTM's trainable switch.

Tolerance of the gradient comparison: 1e-12 of each recorded array's max-abs.  Both sides are float64 autograd through the same
sums in another association; measured when the fixtures were captured, a functional restatement and the reference module agree
to <= 8e-16 of each gradient's max-abs on the weird / chain / rand / mixpad forests, at both scales and both modes."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import tree_lstm_grad_torch as tg
from tests import util
from tests.test_tree_lstm_golden import golden_inputs
from tests.test_tree_lstm_synth import stored_inputs
from tests.tree_lstm_torch import seeded_params

GOLDENS = sorted(glob.glob(os.path.join(util.GOLD, "grad_tree_lstm_*.npz")))
NAMES = [os.path.basename(p)[len("grad_tree_lstm_"):-4] for p in GOLDENS]
SOURCES = ("cfg2_uniform", "synth_weird_n31", "synth_chain_n64", "synth_mixpad_n31", "synth_rand_n4", "synth_allpad_n4")
MODES = ("roots", "all")
WHOLE = ("W_iou.weight", "W_iou.bias", "W_c.bias", "W_f.weight", "W_f.bias")
PROBED = ("U_iou.weight", "W_c.weight", "U_f.weight")
TOL = 1e-12


def inputs_of(source):
    if source.startswith("synth_"):
        return stored_inputs(np.load(os.path.join(util.GOLD, "synth_tree_lstm_%s.npz" % source[len("synth_"):])))
    return golden_inputs(np.load(os.path.join(util.GOLD, "tree_lstm_%s.npz" % source)))


def upstream(g, mode, T, N):
    """the R of the loss sum(R * h): float64 [T, 128] over the roots, [T*N, 128] over every node"""
    rng = np.random.default_rng([int(g["r_seed"]), MODES.index(mode)])
    return torch.from_numpy(rng.standard_normal((T if mode == "roots" else T * N, 128)))


def probes(g, name, shape):
    rng = np.random.default_rng([int(g["probe_seed"]), tg.PARAM_ORDER.index(name)])
    v = rng.standard_normal((shape[1], 2))
    u = rng.standard_normal((2, shape[0]))
    return u, v


def test_goldens_present():
    assert set(NAMES) == {"%s_x%d" % (s, k) for s in SOURCES for k in (1, 4)}
    for p in GOLDENS:
        assert os.path.getsize(p) < 256 * 1024
        g = np.load(p)
        assert list(g["modes"]) == list(MODES)
        assert {k.split("_", 1)[0] for k in g.files} >= {"whole", "left", "right", "maxabs", "sum"}


def _close(mine, ref, what):
    ref = np.asarray(ref)
    bound = TOL * np.abs(ref).max(initial=0)
    err = np.abs(np.asarray(mine) - ref).max(initial=0)
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_autograd_matches_reference(name):
    g = np.load(os.path.join(util.GOLD, "grad_tree_lstm_%s.npz" % name))
    x = inputs_of(str(g["source"]))
    T, N = int(g["T"]), int(g["N"])
    assert x[2].shape[0] * x[2].shape[1] == T and x[2].shape[2] == N
    params = seeded_params(int(g["seed"]), float(g["scale"]))
    some = False
    for m, mode in enumerate(MODES):
        mine = {k: v.numpy() for k, v in tg.grads(x, params, upstream(g, mode, T, N), mode == "roots").items()}
        for k in WHOLE:
            _close(mine[k], g["whole_" + k.replace(".", "_")][m], (mode, k))
        for k in PROBED:
            key = k.replace(".", "_")
            u, v = probes(g, k, mine[k].shape)
            big = float(g["maxabs_" + key][m])
            some |= big > 0
            _close(mine[k] @ v, g["right_" + key][m], (mode, k, "right"))
            _close(u @ mine[k], g["left_" + key][m], (mode, k, "left"))
            assert abs(np.abs(mine[k]).max() - big) <= TOL * big
            assert abs(mine[k].sum() - float(g["sum_" + key][m])) <= TOL * np.abs(mine[k]).sum()       # (a sum: relative to its terms')
    assert some == ("allpad" not in name)                   # nothing but padding: every gradient is exactly zero


def test_float32_restatement_is_close():
    """e32, the GPU tests' yardstick: the same autograd in float32 sits at 1e-7 .. 1e-5 of the float64 one here"""
    g = np.load(os.path.join(util.GOLD, "grad_tree_lstm_synth_weird_n31_x1.npz"))
    x = inputs_of("synth_weird_n31")
    params = seeded_params(int(g["seed"]), 1.0)
    R = upstream(g, "all", int(g["T"]), int(g["N"]))
    e = tg.rel_errors(tg.grads(x, params, R, False, torch.float32), tg.grads(x, params, R, False))
    assert 0 < max(e.values()) < 1e-5, e


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_binding_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    hb.build()                                                             # (the tests below call the library)
    names = [name for _, name, _ in cabi.declarations("flatland_train.h")]
    assert names == list(hb.symbols("flatland_train.h")) == ["fl_tree_lstm_backward_workspace_bytes", "fl_tree_lstm_backward"]
    assert "solution/nn/TreeLSTM.py:33-154" in open(os.path.join(cabi.INCLUDE, "flatland_train.h")).read()


FAKE = 0x10000      # 16-byte aligned, never dereferenced
PTRS = ("forest", "adj", "no", "eo", "w_iou", "b_iou", "u_iou", "w_c", "b_c", "w_f", "b_f", "u_f", "h", "c", "grad_h",
        "da", "dc", "dg", "q", "child", "status", "workspace")


def call(T=2, N=31, roots_only=0, ws=None, **ptrs):
    L = hb.lib()
    p = dict.fromkeys(PTRS, FAKE)
    p["status"] = 0
    p.update(ptrs)
    v = [C.c_void_p(p[k]) if p[k] else None for k in PTRS]
    need = L.fl_tree_lstm_backward_workspace_bytes(max(T, 1), N)
    rc = L.fl_tree_lstm_backward(T, N, *v[:15], roots_only, *v[15:22], need if ws is None else ws, None)
    return rc, L.fl_last_error().decode()


def test_workspace_bytes():
    L = hb.lib()
    assert L.fl_tree_lstm_backward_workspace_bytes(10, 31) == 10 * 31 * 6 * 128 * 4
    assert L.fl_tree_lstm_backward_workspace_bytes(0, 31) == 0 and L.fl_tree_lstm_backward_workspace_bytes(3, 0) == 0


@pytest.mark.parametrize("kw, words", [
    (dict(N=50), "% 3"), (dict(N=65), "bad sizes"), (dict(N=3), "bad sizes"), (dict(T=0), "bad sizes"), (dict(T=-3), "bad sizes"),
    (dict(forest=0), "forest is NULL"), (dict(adj=0), "adjacency is NULL"), (dict(u_f=0), "u_f is NULL"), (dict(h=0), "h is NULL"),
    (dict(c=0), "c is NULL"), (dict(grad_h=0), "grad_h is NULL"), (dict(da=0), "da is NULL"), (dict(q=0), "q is NULL"),
    (dict(child=0), "child is NULL"), (dict(workspace=0), "workspace is NULL"),
    (dict(no=FAKE + 4), "not 8-byte aligned"), (dict(w_c=FAKE + 8), "not 16-byte aligned"), (dict(dg=FAKE + 4), "dg is not 16-byte aligned"),
    (dict(child=FAKE + 2), "child is not 4-byte aligned"), (dict(status=FAKE + 2), "status is not 4-byte aligned"),
    (dict(ws=1000), "workspace"), (dict(ws=2 * 31 * 6 * 512 - 1), "workspace"), (dict(roots_only=2), "roots_only"),
])
def test_refusals(kw, words):
    rc, msg = call(**kw)
    assert rc == 1, (rc, msg)
    assert msg.startswith("fl_tree_lstm_backward:") and words in msg, msg


# ---------------------------------------------------------------------------------------------------------------- the module
def test_trainable_switch():
    from flatland_marl_amd import policy
    from flatland_marl_amd.policy import Network, TreeLSTM
    m = TreeLSTM()
    assert m.trainable is False and TreeLSTM(12, 128, trainable=True).trainable is True
    assert TreeLSTM(trainable=1).trainable is True
    m2 = TreeLSTM.from_module(m)
    m3 = TreeLSTM.from_module(m, trainable=True)
    assert m2.trainable is False and m3.trainable is True
    assert all(a is b for a, b in zip(m.parameters(), m3.parameters()))
    m3.trainable = False
    assert m3.trainable is False and "trainable" not in m3.state_dict()
    assert list(m3.state_dict()) == list(m.state_dict())
    with pytest.raises(ValueError):
        TreeLSTM(12, 64, trainable=True)
    net = Network()
    assert net.tree_lstm.trainable is False
    net.tree_lstm.trainable = True
    assert Network.from_module(net).tree_lstm.trainable is True
    assert isinstance(policy.BACKWARD_CHUNK_TREES, int) and policy.BACKWARD_CHUNK_TREES >= 1
    assert policy.PARAM_ORDER == tg.PARAM_ORDER


def test_param_grads_from_rows_on_the_cpu():
    """tree_lstm_param_grads on hand-made rows (the CPU runs the same torch ops): the sums include/flatland_train.h lists, a
    padding node's NaN features and a read-as-zero child's row 0 left out, the result the same through ragged reduction blocks"""
    from flatland_marl_amd import policy
    rng = np.random.default_rng(3)
    n = 37
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))      # noqa: E731
    x, h, da, dc, dg, q = f(n, 12), f(n, 128), f(n, 384), f(n, 128), f(n, 3, 128), f(n, 384)
    no = torch.from_numpy(rng.integers(0, 3, n))
    no[5] = -2
    x[5] = float("nan")
    da[5], dc[5], dg[5], q[5] = 0, 0, 0, 0
    dg[no == 0], q[no == 0] = 0, 0
    child = torch.from_numpy(rng.integers(-1, n, (n, 3)).astype(np.int32))
    child[no <= 0] = -1
    h[0] = float("inf")
    child[child == 0] = -1
    real = (no >= 0).double().view(n, 1)
    xd = torch.where(real.bool(), x.double(), torch.zeros(()).double())
    hk = torch.stack([torch.where((child[:, j] >= 0).view(n, 1), h.double()[child[:, j].clamp(min=0).long()], torch.zeros(()).double())
                      for j in range(3)], 1)
    dad, dcd, dgd = da.double(), dc.double(), dg.double()
    want = (dad.T @ xd, dad.sum(0), dad.T @ hk.view(n, 384), dcd.T @ q.double(), (dcd * (no >= 1).view(n, 1)).sum(0),
            dgd.sum(1).T @ xd, dgd.sum((0, 1)), sum(dgd[:, j].T @ hk[:, j] for j in range(3)))
    old = policy.REDUCE_BLOCK
    try:
        for block in (old, 8, 37):
            policy.REDUCE_BLOCK = block
            got = policy.tree_lstm_param_grads(x, no, h, da, dc, dg, q, child)
            assert len(got) == 8
            for a, b, k in zip(got, want, policy.PARAM_ORDER):
                assert a.dtype == torch.float32 and a.shape == b.shape, k
                assert float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max()), k
    finally:
        policy.REDUCE_BLOCK = old
