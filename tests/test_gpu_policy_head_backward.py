"""GPU: the trainable policy head -- policy.Network(trainable=True), fl_policy_head_forward_saved / fl_policy_head_backward
(include/flatland_policy_train.h) and the parameter products behind them -- against the float64 autograd of the restatement
(tests/policy_head_grad_torch.py, itself pinned to the reference Network's gradients by tests/test_policy_head_grad_golden.py), run
on the device.

Shapes: tests/policy_head_stages.SHAPES at both SCALES, the upstream gradients standard normal on every logit and every value.
Error per tensor = max |g - g64| / max |g64|; where g64 is identically zero the kernel's gradient must be exactly zero or None.
Tolerance: e32 = the same figure for the restatement's float32 autograd on the device; a tensor passes at R * e32.  R = 6, set on
2026-10-19 from tests/golden/policy_head_grad_errors.json (MI355X) by the project's rule: twice the largest ratio recorded there
(2.95, b1_a1024-x1 transformer.0.attention.out_proj.bias; the median of all 858 ratios is 0.99), rounded up to an integer.
POLICY_HEAD_GRAD_ERRORS=<path> makes the gradient cases write their figures to <path> in that file's format.

Where the rounding comes from.  The first measurement gave ratios up to 3.79 in the 38 gradients (b70_a1-x1 tree) and, stage by stage,
4.16 (b1_a64-x1 dqkv_1) and 36.3 (b1_a1024 with block 2's attention pushed flat, dqkv_2).  The stage test put all of the 36.3 in a
kernel's rows, none in the products: block 2's dq alone (error 8.6e-6 of a largest entry 0.060, torch's float32 softmax backward
2.4e-7; dv 2.6e-8 against 2.2e-8, dk exactly zero as it must be with q = 0).  The attention backward then took D = rowsum(dC o C);
that D is not the sum of the P o dP that dS = P o (dP - D) is made of, sum_k dS = 0 holds only to the rounding of c and of the
64-term product, and dq = sum_k dS K cancels on exactly that where P is flat.  k_pb_attn_q now sums D = rowsum(P o dP) in a pass
of its own from the very P and dP the next pass uses.  After that: flat 3.92 (dq 9.3e-7), b1_a64-x1 1.75, b70_a1-x1 1.46, and the
figures in the file.  What is left at the top: 2.95 (error 6.1e-6 against e32 2.1e-6) and 2.67 at b33_a2-x1 actor_net.4.weight
(2.7e-6 against 1.0e-6); whether those sit in the rows or in the products has not been bisected.
"""
import ctypes as C
import functools
import json
import math
import os
import types

import pytest
import torch

from flatland_marl_amd.hip_backend import POLICY_ROWS_LAYOUT
from tests import policy_head_grad_torch as pg
from tests import policy_head_stages as st
from tests import util

R = 6
ERRORS = os.path.join(util.GOLD, "policy_head_grad_errors.json")
DEV = "cuda:0"
GUARD = st.GUARD
GRAD_CASES = [(B, A, s) for B, A in st.SHAPES for s in range(2)]


def _case_id(B, A, s):
    return "b%d_a%d-x%d" % (B, A, s)


def _pushed_cases():
    out = []
    for B, A in st.PUSHED_SHAPES:
        out += [(B, A, "sharp", st.SHARP_SEEDS[(B, A)][0]), (B, A, "flat", st.INPUT_SEED), (B, A, "constv", st.INPUT_SEED)]
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_R_follows_the_recorded_errors():
    rec = json.load(open(ERRORS))
    ratios = [v for c in rec["cases"].values() for k, v in c.items() if k.startswith("ratio_")]
    assert R == math.ceil(2 * max(ratios)) and rec["R"] == R
    for c in rec["cases"].values():
        for k in pg.NAMES + ["tree"]:
            assert c["ratio_" + k] == (c["err_" + k] / c["e32_" + k] if c["e32_" + k] > 0 else 0.0)
    assert set(rec["cases"]) == {_case_id(*c) for c in GRAD_CASES}


# ---------------------------------------------------------------------------------------------------------------- helpers
def _inputs(B, A, seed=st.INPUT_SEED):
    attr, tree, _ = st.inputs(B, A, seed)
    return attr.to(DEV), tree.to(DEV)


def _net(params, trainable=True):
    from flatland_marl_amd.policy import Network
    net = Network(trainable=trainable).to(DEV)
    net.load_state_dict(params)
    return net


def _kernel_grads(net, attr, tree, Rl, Rv, value=True):
    """forward + backward through the module: {name: gradient or None, "tree": ...}, logits, value"""
    net.zero_grad(set_to_none=True)
    t = tree.detach().clone().requires_grad_(True)
    logits, val = net.head(attr, t, value=value)
    pg.loss_of(logits[0], val, None if Rl is None else Rl.to(DEV), None if Rv is None or not value else Rv.to(DEV)).backward()
    sd = dict(net.named_parameters())
    g = {k: (None if sd[k].grad is None else sd[k].grad.clone()) for k in pg.NAMES}
    g["tree"] = t.grad
    return g, logits[0].detach(), None if val is None else val.detach()


@functools.lru_cache(maxsize=None)
def _reference(B, A, s, mode="both"):
    """(g32, g64) of the restatement's autograd on the device, computed once per case and left unchanged"""
    attr, tree = _inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    Rl, Rv = (Rl if mode != "value" else None), (Rv if mode != "logits" else None)
    p = st.params(s)
    return pg.grads(attr, tree, p, Rl, Rv, torch.float32), pg.grads(attr, tree, p, Rl, Rv, torch.float64)


def _figures(g, g32, g64, names):
    figs = {}
    for k in names:
        gk = torch.zeros_like(g64[k]) if g[k] is None else g[k]                 # (None: no gradient = zero)
        figs["err_" + k], figs["e32_" + k] = pg.rel_error(gk, g64[k]), pg.rel_error(g32[k], g64[k])
        figs["ratio_" + k] = figs["err_" + k] / figs["e32_" + k] if figs["e32_" + k] > 0 else 0.0
    return figs


def _assert_within(g, g32, g64, what, names=tuple(pg.NAMES) + ("tree",), record=False):
    figs = _figures(g, g32, g64, names)
    if record:
        util.record_errors("POLICY_HEAD_GRAD_ERRORS", "cases", what, figs)
    print(what, "largest ratio %.3f" % max(figs["ratio_" + k] for k in names))
    for k in names:
        if float(g64[k].abs().max()) == 0:
            assert g[k] is None or float(g[k].abs().max()) == 0, (what, k, "the gradient is identically zero")
        else:
            assert figs["err_" + k] <= R * figs["e32_" + k], (what, k, figs["err_" + k], figs["e32_" + k])
    return figs


def _guarded(nfloats, fill=0xFF):
    buf = torch.empty(nfloats * 4 + GUARD, dtype=torch.uint8, device=DEV)
    buf[:nfloats * 4].fill_(fill)
    buf[nfloats * 4:].fill_(0xA5)
    return buf, buf[:nfloats * 4].view(torch.float32), buf[nfloats * 4:]


def _call(attr, tree, plist, Rl, Rv, value=True):
    """fl_policy_head_forward_saved and fl_policy_head_backward on torch's current stream with buffers of the test's own: saved,
    rows and the workspace every byte 0xFF before the call (every float a NaN), GUARD bytes of 0xA5 behind each"""
    from flatland_marl_amd import hip_backend as hb
    B, A = attr.shape[:2]
    n = B * A
    out = types.SimpleNamespace(B=B, A=A)
    nsaved, nws = hb.policy_saved_floats(B, A), hb._sym("fl_policy_head_backward_workspace_bytes")(B, A) // 4
    assert hb._sym("fl_policy_head_backward_rows_bytes")(B, A) == n * hb.POLICY_ROW_FLOATS * 4 and nsaved >= n * hb.POLICY_SAVED_FLOATS
    with torch.cuda.device(DEV):
        out.bufs = [_guarded(nsaved), _guarded(n * hb.POLICY_ROW_FLOATS), _guarded(nws)]
        (_, saved, _), (_, rows, _), (_, ws, _) = out.bufs
        out.logits = torch.full((B, A, 5), float("nan"), device=DEV)
        out.value = torch.full((B,), float("nan"), device=DEV) if value else None
        out.gtree = torch.full((B, A, 128), float("nan"), device=DEV)
        ptrs = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in plist])
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        hb._chk(hb._sym("fl_policy_head_forward_saved")(B, A, attr.data_ptr(), tree.data_ptr(), ptrs, out.logits.data_ptr(),
                                                        opt(out.value), saved.data_ptr(), nsaved * 4, s))
        hb._chk(hb._sym("fl_policy_head_backward")(B, A, attr.data_ptr(), tree.data_ptr(), ptrs, saved.data_ptr(), opt(Rl), opt(Rv),
                                                   out.gtree.data_ptr(), rows.data_ptr(), rows.numel() * 4, ws.data_ptr(), nws * 4, s))
    out.saved, out.rows, out.ws = saved, rows, ws
    out.sv = hb.policy_views(saved, hb.POLICY_SAVED_LAYOUT, n)
    out.rw = hb.policy_views(rows, hb.POLICY_ROWS_LAYOUT, n)
    return out


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: _case_id(*c))
def test_gradients_match_the_restatement(case):
    """the 38 parameter gradients and grad_tree through Network(trainable=True).head, both upstream gradients given; the forward's
    values are the inference path's bits"""
    B, A, s = case
    attr, tree = _inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    net = _net(st.params(s))
    g, logits, value = _kernel_grads(net, attr, tree, Rl, Rv)
    with torch.no_grad():
        lg0, v0 = _net(st.params(s), trainable=False).head(attr, tree)
    assert util.same_bits(logits, lg0[0]) and util.same_bits(value, v0)
    g32, g64 = _reference(B, A, s)
    _assert_within(g, g32, g64, _case_id(*case), record=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("logits", "value", "novalue"))
def test_exact_zeros(mode):
    """a logits-only loss leaves the critic's six gradients exactly zero or None, a value-only loss the actor's; value=False runs no
    critic at all; the others stay within the tolerance"""
    B, A, s = 3, 11, 1
    attr, tree = _inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    net = _net(st.params(s))
    g, _, value = _kernel_grads(net, attr, tree, None if mode == "value" else Rl, None if mode == "logits" else Rv, value=mode != "novalue")
    assert (value is None) == (mode == "novalue")
    g32, g64 = _reference(B, A, s, "value" if mode == "value" else "logits")
    zero = pg.ACTOR if mode == "value" else pg.CRITIC
    for k in zero:
        assert float(g64[k].abs().max()) == 0 and (g[k] is None or float(g[k].abs().max()) == 0), k
    if mode == "novalue":
        assert all(g[k] is None for k in pg.CRITIC)
    _assert_within(g, g32, g64, mode)


STAGE_ROWS = [n for n, _ in POLICY_ROWS_LAYOUT]
FORWARD_ROWS = {"attr.h1", "attr.h2", "attr.h3", "o0", "o1", "o2", "actor.u1", "actor.u2", "critic.u1", "critic.u2"}


def _stage_check(attr, tree, p, what):
    B, A = attr.shape[:2]
    Rl, Rv = pg.upstream(B, A)
    out = _call(attr, tree, st.device_params(p, DEV), Rl.to(DEV), Rv.to(DEV))
    g32, g64 = (pg.grads(attr, tree, p, Rl, Rv, dt, stages=True) for dt in (torch.float32, torch.float64))
    got, names = {"tree": out.gtree}, ["tree"]
    for n in STAGE_ROWS:
        ref = "value:do" + n[1:] if n in ("o0", "o1", "o2") else "value:" + n if n in FORWARD_ROWS else n
        row = out.rw[n]
        if n in ("actor.dz4", "critic.dz4"):
            k = 5 if n.startswith("actor") else 1
            assert float(row[:, k:].abs().max()) == 0, n
            row = row[:, :k]
        got[ref] = row.reshape(g64[ref].shape)
        names.append(ref)
    return _assert_within(got, g32, g64, what, tuple(names))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: _case_id(*c))
def test_every_row_matches_the_restatement(case):
    """grad_tree and every array of rows_dev after one call against the float64 autograd's gradient (retain_grad) or value at the
    same place, each held to R * e32: the pin of the row layout include/flatland_policy_train.h documents"""
    B, A, s = case
    attr, tree = _inputs(B, A)
    _stage_check(attr, tree, st.params(s), _case_id(*case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _pushed_cases(), ids=lambda c: "b%d_a%d-%s" % c[:3])
def test_every_row_with_block_2_pushed(case):
    """the same with block 2's attention pushed sharp, flat and to a constant v: dS = P (dP - D) is where a softmax backward cancels"""
    B, A, kind, seed = case
    attr, tree = _inputs(B, A, seed)
    _stage_check(attr, tree, st.pushed_params(kind, A)[0], "b%d_a%d-%s" % (B, A, kind))


@pytest.mark.gpu
def test_no_grad_and_the_default_launch_the_inference_path(monkeypatch):
    """under torch.no_grad() a trainable Network calls fl_policy_head alone; with grad mode on it calls the saved forward (and, with a
    mode, fl_policy_head once more for the choice); an untrained one never calls the saved forward"""
    from flatland_marl_amd import hip_backend as hb
    calls = []
    for name in ("policy_head", "policy_head_forward_saved", "policy_head_backward"):
        monkeypatch.setattr(hb, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(hb, name), name))
    attr, tree = _inputs(3, 11)
    valid = st.inputs(3, 11)[2].to(DEV)
    net = _net(st.params(0))
    with torch.no_grad():
        a = net.head(attr, tree)
    assert calls == ["policy_head"]
    del calls[:]
    b = net.head(attr, tree)
    assert calls == ["policy_head_forward_saved"]
    assert util.same_bits(a[0][0], b[0][0]) and util.same_bits(a[1], b[1]) and b[0][0].requires_grad
    del calls[:]
    c = net.head(attr, tree, valid, "soft")
    assert calls == ["policy_head_forward_saved", "policy_head"]
    with torch.no_grad():
        d = net.head(attr, tree, valid, "soft")
    assert torch.equal(c[2], d[2]) and util.same_bits(c[0][0], a[0][0]) and not c[2].requires_grad
    del calls[:]
    _net(st.params(0), trainable=False).head(attr, tree)
    assert calls == ["policy_head"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((5, 13), (2, 33), (1, 1024)), ids=lambda c: "b%d_a%d" % c)
def test_same_bits_twice(shape):
    """two calls on the same inputs: grad_tree and every row bit-identical (the kernels' promise); the 38 gradients through the
    module are OBSERVED to be bit-identical too -- torch's products do not promise that"""
    B, A = shape
    attr, tree = _inputs(B, A)
    Rl, Rv = (x.to(DEV) for x in pg.upstream(B, A))
    plist = st.device_params(st.params(1), DEV)
    a, b = _call(attr, tree, plist, Rl, Rv), _call(attr, tree, plist, Rl, Rv)
    assert util.same_bits(a.gtree, b.gtree) and util.same_bits(a.rows, b.rows) and util.same_bits(a.saved, b.saved)
    net = _net(st.params(1))
    g1, g2 = _kernel_grads(net, attr, tree, Rl, Rv)[0], _kernel_grads(net, attr, tree, Rl, Rv)[0]
    assert all(util.same_bits(g1[k], g2[k]) for k in g1)


@pytest.mark.gpu
def test_envs_are_isolated():
    """A = 20, B = 2: the 32-row tile straddles the envs; other inputs and another upstream gradient in env 1 leave every row, the
    saved forward and grad_tree of env 0 bit-identical"""
    B, A = 2, 20
    attr, tree = _inputs(B, A)
    attr2, tree2 = _inputs(B, A, st.INPUT_SEED + 1)
    attr2[0], tree2[0] = attr[0], tree[0]
    Rl, Rv = (x.to(DEV) for x in pg.upstream(B, A))
    Rl2, Rv2 = (x.to(DEV) for x in pg.upstream(B, A, 10))
    Rl2[0], Rv2[0] = Rl[0], Rv[0]
    plist = st.device_params(st.params(1), DEV)
    a, b = _call(attr, tree, plist, Rl, Rv), _call(attr2, tree2, plist, Rl2, Rv2)
    assert util.same_bits(a.gtree[0], b.gtree[0]) and not util.same_bits(a.gtree[1], b.gtree[1])
    for views in ("rw", "sv"):
        for n, v in getattr(a, views).items():
            w = getattr(b, views)[n]
            assert util.same_bits(v[:A], w[:A]), n
            assert not util.same_bits(v[A:], w[A:]), n


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("both", "logits", "value", "stream"))
def test_buffers_are_written_and_guards_untouched(mode):
    """saved, rows and the workspace start as NaN bytes with a guard behind each: after the call no NaN is left in anything the
    header says is written (with one upstream gradient NULL the other head's five arrays are not), the guards are untouched; once
    on a side stream"""
    B, A = 5, 13
    attr, tree = _inputs(B, A)
    Rl, Rv = (x.to(DEV) for x in pg.upstream(B, A))
    plist = st.device_params(st.params(0), DEV)
    if mode == "stream":
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            out = _call(attr, tree, plist, Rl, Rv)
        side.synchronize()
    else:
        out = _call(attr, tree, plist, Rl if mode != "value" else None, Rv if mode != "logits" else None)
    for _, _, guard in out.bufs:
        assert bool((guard == 0xA5).all())
    n = B * A
    assert not bool(torch.isnan(out.gtree).any()) and not bool(torch.isnan(out.logits).any()) and not bool(torch.isnan(out.value).any())
    assert not bool(torch.isnan(out.saved[:n * 4097]).any()) and not bool(torch.isnan(out.ws).any())
    skipped = {"logits": "critic.", "value": "actor."}.get(mode, "none")
    for name, v in out.rw.items():
        if name.startswith(skipped):
            assert bool(torch.isnan(v).all()), name
        else:
            assert not bool(torch.isnan(v).any()), name


@pytest.mark.gpu
def test_chunks(monkeypatch):
    """HEAD_BACKWARD_CHUNK_ROWS set so that (5, 13) runs in three chunks of whole envs: the gradients stay within the tolerance, the
    forward's values are the unchunked bits, and the chunked form twice gives bit-identical gradients"""
    from flatland_marl_amd import policy
    B, A, s = 5, 13, 1
    monkeypatch.setattr(policy, "HEAD_BACKWARD_CHUNK_ROWS", 2 * A + 3)
    assert policy.head_chunks(B, A) == [(0, 2), (2, 4), (4, 5)]
    attr, tree = _inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    net = _net(st.params(s))
    g1, logits, value = _kernel_grads(net, attr, tree, Rl, Rv)
    g2 = _kernel_grads(net, attr, tree, Rl, Rv)[0]
    assert all(util.same_bits(g1[k], g2[k]) for k in g1)
    with torch.no_grad():
        lg0, v0 = net.head(attr, tree)
    assert util.same_bits(logits, lg0[0]) and util.same_bits(value, v0)
    _assert_within(g1, *_reference(B, A, s), "chunks")


@pytest.mark.gpu
def test_end_to_end_trains_all_46_parameters():
    """Network(trainable=True) with tree_lstm.trainable on a synthetic forest at (3, 11): one loss.backward() through forward fills
    all 46 gradients, each within R (the head's) or the encoder's R of the float64 autograd through both restatements chained"""
    from tests import tree_lstm_forests as tf
    from tests import tree_lstm_grad_torch as tg
    from tests.test_gpu_tree_lstm_backward import R as R_TREE
    B, A, N = 3, 11, 31
    x = tuple(t.to(DEV) for t in tf.make("rand", B * A, N, 5))
    x = (x[0].view(B, A, N, 12).contiguous(), x[1].view(B, A, N - 1, 3).contiguous(), x[2].view(B, A, N).contiguous(),
         x[3].view(B, A, N - 1).contiguous())
    attr, _ = _inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    params = st.params(0)
    net = _net(params)
    net.tree_lstm.trainable = True
    logits, value = net(attr, *x)
    pg.loss_of(logits[0], value, Rl.to(DEV), Rv.to(DEV)).backward()
    got = {k: v.grad for k, v in net.named_parameters()}
    assert len(got) == 46 and all(v is not None for v in got.values())

    def chained(dtype):
        pt = {k: params["tree_lstm." + k].detach().to(device=DEV, dtype=dtype).clone().requires_grad_(True) for k in tg.PARAM_ORDER}
        ph_ = pg.leaf_params(params, DEV, dtype)
        h = tg.tree_lstm(*x, pt, dtype).view(B, A, N, 128)[:, :, 0]
        lg, v = pg.forward(attr, h, ph_)
        pg.loss_of(lg, v, Rl, Rv).backward()
        return {**{"tree_lstm." + k: t.grad for k, t in pt.items()}, **{k: t.grad for k, t in ph_.items()}}
    g32, g64 = chained(torch.float32), chained(torch.float64)
    for k in got:
        err, e32 = pg.rel_error(got[k], g64[k]), pg.rel_error(g32[k], g64[k])
        print(k, err, e32)
        assert err <= (R_TREE if k.startswith("tree_lstm.") else R) * e32, (k, err, e32)


@pytest.mark.gpu
def test_refusals_and_conversions_on_the_device():
    """agents_attr.requires_grad raises; a non-contiguous upstream gradient is made contiguous (the same gradients as from the
    plain one, bit for bit); float64 inputs and CPU inputs are refused as on the inference path"""
    B, A = 3, 11
    attr, tree = _inputs(B, A)
    net = _net(st.params(0))
    with pytest.raises(ValueError, match="agents_attr gets no gradient"):
        net.head(attr.clone().requires_grad_(True), tree)
    with pytest.raises(TypeError, match="must be torch.float32"):
        net.head(attr.double(), tree)
    with pytest.raises(TypeError, match="must be on a GPU"):
        net.head(attr.cpu(), tree)
    Rl, Rv = pg.upstream(B, A)
    g1 = _kernel_grads(net, attr, tree, Rl, Rv)[0]
    wide = torch.zeros((B, A, 10), dtype=torch.float32, device=DEV)
    wide[..., ::2] = Rl.to(DEV)
    net.zero_grad(set_to_none=True)
    t = tree.detach().clone().requires_grad_(True)
    logits, value = net.head(attr, t)
    torch.autograd.backward([logits[0], value], [wide[..., ::2], Rv.to(DEV)])
    g2 = {k: v.grad for k, v in net.named_parameters() if k in g1}
    g2["tree"] = t.grad
    assert all(util.same_bits(g1[k], g2[k]) for k in g1)
