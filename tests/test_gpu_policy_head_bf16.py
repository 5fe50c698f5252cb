"""fl_policy_head_bf16 (include/flatland_policy_head_bf16.h) on the GPU, stage by stage from the workspace it leaves, on the edge
shapes of tests/policy_head_stages.py and on the reference's fixtures.

Two kinds of check.  qkv (from xb) and ao (from the stored qkv) have all their bf16 operands visible in the workspace: they are
held to the a-priori bounds of tests/policy_head_bf16_bounds.py per element, no recorded number involved.  Between the other
visible stages -- emb[..., :128] from the attributes, xa from emb, xb from xa, logits and val from (emb, xb, ao) -- lie several
rounded layers, and a rounding that lands on the other side of a bf16 tie cannot be bounded a priori.  They follow the encoder's
method (tests/test_gpu_tree_lstm_bf16.py): e16 = the error of the emulation (tests/policy_head_bf16_torch.py) against the float64
restatement without rounding, both from the KERNEL's own previous stage; the kernel passes when its error against that restatement
is at most R16 * e16, R16 = 2: it differs from the emulation by float32 sums and by tie roundings, perturbations the size of those
the emulation makes already, so the expected ratio is 1 (the encoder measured at most 1.22) and 2 is the usual factor of two.
POLICY_HEAD_BF16_ERRORS=<path> makes the cases write their figures to <path> in the format of
tests/golden/policy_head_bf16_errors.json."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import policy_head_bf16_bounds as pb16
from tests import policy_head_bf16_torch as ph16
from tests import policy_head_bounds as pb
from tests import policy_head_stages as phs
from tests import policy_head_torch as ph
from tests import util
from tests.test_policy_head_golden import NAMES, golden_inputs, golden_params, load

DEV = "cuda:0"
R16 = 2
ERRORS = os.path.join(util.GOLD, "policy_head_bf16_errors.json")
PACKED_BYTES = 3342336
ROW_BYTES = 4 * 256 * 4 + 768 * 2 + 4
# the 16 packed matrices: index into the 38 parameters, in the packed buffer's order
MATRICES = (2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 32, 34)
RATIO_STAGES = ("emb_attr", "xa", "xb", "logits", "val")
OBS_FIXTURES = ("cfg1_uniform", "cfg2_uniform", "cfg3_uniform")

SHAPE_CASES = ["b%d_a%d-x%d" % (B, A, s) for B, A in phs.SHAPES for s in range(2)]
PUSH_CASES = [cid for B, A in phs.PUSHED_SHAPES for cid in phs.sharp_cases(B, A) + ["b%d_a%d-%s" % (B, A, k) for k in phs.PUSHES[1:]]]
FIXTURE_CASES = ["fixture-%s-x%d" % (n, s) for n in NAMES for s in range(2)]
OBS_CASES = ["obs-%s-x%d" % (n, s) for n in OBS_FIXTURES for s in range(2)]
IDS = SHAPE_CASES + FIXTURE_CASES + OBS_CASES        # the cases the record holds


def run(attr, tree, plist, packed, valid=None, mode=None, u=None, value=True):
    """one fl_policy_head_bf16 call on torch's current stream, as policy_head_stages.run makes fl_policy_head's: the workspace is
    fl_policy_head_bf16_workspace_bytes long, every byte 0xFF before the call (every float and every bf16 a NaN), with GUARD bytes of
    0xA5 behind it.  Returns logits, value, actions, the stages as [B, A, .] views of the workspace (qkv bfloat16), and guard."""
    from flatland_marl_amd import hip_backend as hb
    B, A = attr.shape[:2]
    R, dev = B * A, attr.device
    nbytes = hb._sym("fl_policy_head_bf16_workspace_bytes")(B, A)
    assert nbytes == (R * ROW_BYTES + 15) // 16 * 16
    out = types.SimpleNamespace(B=B, A=A)
    with torch.cuda.device(dev):
        buf = torch.empty(nbytes + phs.GUARD, dtype=torch.uint8, device=dev)
        buf[:nbytes].fill_(0xFF)
        buf[nbytes:].fill_(0xA5)
        out.logits = torch.full((B, A, 5), float("nan"), device=dev)
        out.value = torch.full((B,), float("nan"), device=dev) if value else None
        out.actions = torch.full((B, A), 77, dtype=torch.uint8, device=dev) if mode else None
        ptrs = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in plist])
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        s = torch.cuda.current_stream(dev).cuda_stream
        hb._chk(hb._sym("fl_policy_head_bf16")(B, A, attr.data_ptr(), tree.data_ptr(), ptrs, packed.data_ptr(), packed.numel(),
                                               opt(valid) if mode else None, hb.POLICY_SELECT[mode],
                                               hb.POLICY_U_REFERENCE if u is None else float(u), out.logits.data_ptr(), opt(out.value),
                                               opt(out.actions), buf.data_ptr(), nbytes, C.c_void_p(s)))
    f32 = buf[:4096 * R].view(torch.float32)
    for i, name in enumerate(("emb", "xa", "xb", "ao")):
        setattr(out, name, f32[256 * R * i:256 * R * (i + 1)].view(B, A, 256))
    out.qkv = buf[4096 * R:5632 * R].view(torch.bfloat16).view(B, A, 768)
    out.val = buf[5632 * R:5636 * R].view(torch.float32).view(B, A)
    out.workspace, out.guard = buf[:nbytes], buf[nbytes:]
    return out


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(t.dtype, t.dtype))


def _differ(a, b, names=("emb", "xa", "xb", "ao", "qkv", "val", "logits", "value", "actions")):
    return [n for n in names if getattr(a, n) is not None and not torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n)))]


def _setup(case):
    from flatland_marl_amd import hip_backend as hb
    attr, tree, valid, params = phs.CASES[case]()
    attr, tree, valid = attr.to(DEV).contiguous(), tree.to(DEV).contiguous(), valid.to(DEV).contiguous()
    plist = phs.device_params(params, DEV)
    return attr, tree, valid, params, plist, hb.policy_head_pack_bf16(plist)


def _intact(st, value=True):
    assert (st.guard == 0xA5).all(), "a write past the workspace"
    for n in ("emb", "xa", "xb", "ao", "qkv", "logits") + (("val", "value") if value else ()):
        assert torch.isfinite(getattr(st, n).float()).all(), n


def _bounded(st, p64, c, case):
    """qkv and ao inside their a-priori bounds; returns the worst |error| / bound of each"""
    ref, bound = pb16.qkv(st.xb.double(), p64, 2)
    w_qkv = phs.worst(st.qkv.double(), ref, bound)
    ref, bound = pb16.attention(st.qkv.double(), c)
    w_ao = phs.worst(st.ao.double(), ref, bound)
    print(case, "a priori: qkv %.3g ao %.3g of the bound" % (w_qkv, w_ao))
    assert w_qkv <= 1.0 and w_ao <= 1.0, (case, w_qkv, w_ao)
    return w_qkv, w_ao


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPE_CASES)
def test_stages(case):
    attr, tree, valid, params, plist, packed = _setup(case)
    st = run(attr, tree, plist, packed, valid, "soft")
    _intact(st)
    assert not _differ(st, run(attr, tree, plist, packed, valid, "soft"))          # two launches: the same bits
    p64 = ph.stage_params(params, DEV)
    c = pb.allowance()
    assert torch.equal(st.emb[..., 128:], tree)
    w_qkv, w_ao = _bounded(st, p64, c, case)
    a64, emb, xa, xb, ao = attr.double(), st.emb.double(), st.xa.double(), st.xb.double(), st.ao.double()
    pairs = {"emb_attr": (emb[..., :128],) + tuple(ph16.stage_attr(a64, p64, r) for r in (False, True)),
             "xa": (xa,) + tuple(ph16.stage_next(emb, p64, 0, r) for r in (False, True)),
             "xb": (xb,) + tuple(ph16.stage_next(xa, p64, 1, r) for r in (False, True))}
    t64, t16 = ph16.stage_tail(emb, xb, ao, p64, False), ph16.stage_tail(emb, xb, ao, p64, True)
    pairs["logits"], pairs["val"] = (st.logits.double(), t64[0], t16[0]), (st.val.double(), t64[1], t16[1])
    figs = dict(qkv_bound=w_qkv, ao_bound=w_ao)
    for name in RATIO_STAGES:
        got, ref, emu = pairs[name]
        err, e16 = float((got - ref).abs().max()), float((emu - ref).abs().max())
        assert e16 > 0, name
        figs["err_" + name], figs["e16_" + name], figs["ratio_" + name] = err, e16, err / e16
    print(case, " ".join("%s %.3g" % (n, figs["ratio_" + n]) for n in RATIO_STAGES))
    util.record_errors("POLICY_HEAD_BF16_ERRORS", "cases", case, figs, R16=R16)
    for name in RATIO_STAGES:
        assert figs["ratio_" + name] <= R16, (case, name, figs)
    assert phs.worst(st.value.double(), ph.stage_value(st.val.double()), pb.value(st.val.double())) <= 1.0
    assert (st.actions.cpu().numpy() == ph.choose_actions(st.logits, valid, "soft")).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", PUSH_CASES)
def test_attention_pushes(case):
    """block 2's in_proj edited (policy_head_stages.pushed_params): sharp -- a few keys take all the weight -- inside the a-priori
    bounds; flat -- every e' equal, so ao is the mean of the stored v within the float32 terms; constv -- every v row the same
    bf16(c), so ao is bf16(c) within constv_tolerance: a row sum over the UNROUNDED e would miss that by about 2^-8 |c| / sqrt(A)"""
    attr, tree, valid, params, plist, packed = _setup(case)
    B, A = attr.shape[:2]
    st = run(attr, tree, plist, packed)
    _intact(st)
    p64 = ph.stage_params(params, DEV)
    c = pb.allowance()
    _bounded(st, p64, c, case)
    kind = case.split("-")[1].split("_")[0]
    qkv64 = st.qkv.double()
    if kind == "flat":
        assert (st.qkv[..., :256] == 0).all()
        mean = qkv64[..., 512:].mean(dim=1, keepdim=True).expand(B, A, 256)
        assert phs.worst(st.ao.double(), mean, pb.attention(qkv64, c)) <= 1.0
    elif kind == "constv":
        cv = ph16.rb(phs.pushed_params("constv", A)[1])
        assert torch.equal(st.qkv[..., 512:].float().cpu(), cv.expand(B, A, 256))
        tol = phs.constv_tolerance(cv, A).to(DEV)
        worst = float(((st.ao.double() - cv.double().to(DEV)).abs() / tol).max())
        print(case, "constv: %.3g of the tolerance" % worst)
        assert worst <= 1.0
    else:
        assert kind.startswith("sharp")


@pytest.mark.gpu
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_reference_fixtures(name, s):
    """the reference's outputs: the kernel's error against the fixture is at most R16 times the emulation's error against it; the
    actions are the restated choice on the kernel's own logits"""
    from flatland_marl_amd import hip_backend as hb
    g = load(name)
    params = golden_params(g, s)
    attr, tree, valid = (x.to(DEV).contiguous() for x in golden_inputs(g, s))
    plist = phs.device_params(params, DEV)
    packed = hb.policy_head_pack_bf16(plist)
    st = run(attr, tree, plist, packed, valid, "soft")
    _intact(st)
    l16, v16 = ph16.head(attr, tree, params)
    gl, gv = torch.from_numpy(g["logits"][s]).double().to(DEV), torch.from_numpy(g["value"][s]).double().to(DEV)
    figs = dict(err_logits=float((st.logits.double() - gl).abs().max()), e16_logits=float((l16 - gl).abs().max()),
                err_value=float((st.value.double() - gv).abs().max()), e16_value=float((v16 - gv).abs().max()))
    figs["ratio_logits"], figs["ratio_value"] = figs["err_logits"] / figs["e16_logits"], figs["err_value"] / figs["e16_value"]
    print(name, "x%d" % s, " ".join("%s %.3g" % kv for kv in figs.items()))
    util.record_errors("POLICY_HEAD_BF16_ERRORS", "cases", "fixture-%s-x%d" % (name, s), figs, R16=R16)
    assert figs["ratio_logits"] <= R16 and figs["ratio_value"] <= R16, figs
    other = 0.8125
    for mode in ("soft", "hard"):
        for u in (None, other):
            got = run(attr, tree, plist, packed, valid, mode, u, value=False)
            assert torch.equal(got.logits, st.logits)
            exp = ph.choose_actions(st.logits, valid, mode, ph.U_REFERENCE if u is None else u)
            assert (got.actions.cpu().numpy() == exp).all(), (mode, u)
    if name in OBS_FIXTURES:
        # recorded, not asserted: how often the bf16 head's "hard" action is another than the float32 head's on real observations
        logits32 = torch.empty_like(st.logits)
        hb.policy_head(attr, tree, plist, logits32)
        a16, a32 = ph.choose_actions(st.logits, valid, "hard"), ph.choose_actions(logits32, valid, "hard")
        obs = dict(agents=int(a16.size), hard_actions_differ=int((a16 != a32).sum()),
                   max_dlogit=float((st.logits - logits32).abs().max()), max_logit=float(logits32.abs().max()))
        print(name, "x%d" % s, obs)
        util.record_errors("POLICY_HEAD_BF16_ERRORS", "cases", "obs-%s-x%d" % (name, s), obs, R16=R16)


def _pack_values(n, starts):
    """float32 values for the matrices: normal ones, exact ties between two bf16 values (both ways round), +-0, subnormals, +-inf and
    the largest finite values (which round to inf): the special set at the head of every matrix and at the very end"""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    bits[((bits >> 23) & 0xFF) == 0xFF] &= np.uint32(0xFF800000)        # random NaNs become inf: NaN has a check of its own
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00008000, 0x00018000,
                        0x007FFFFF, 0x807F8000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF], dtype=np.uint32)
    ties = (rng.integers(0, 0x7F80, size=256 * len(starts), dtype=np.uint64).astype(np.uint32) << 16) | np.uint32(0x8000)
    ties[::2] |= np.uint32(0x80000000)
    for k, off in enumerate(starts):
        bits[off:off + len(special)] = special
        bits[off + 64:off + 64 + 256] = ties[256 * k:256 * (k + 1)]
    bits[-len(special):] = special
    return torch.from_numpy(bits.view(np.float32).copy())


def _as_packed(m):
    """a matrix [R, K] in the order include/flatland_policy_bf16.h documents"""
    R, K = m.shape
    return m.view(R // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)


@pytest.mark.gpu
def test_pack_equals_torchs_rounding():
    from flatland_marl_amd import hip_backend as hb
    shapes = [ph.head_shapes()[i][1] for i in MATRICES]
    starts = np.concatenate([[0], np.cumsum([r * k for r, k in shapes])])
    assert 2 * int(starts[-1]) == PACKED_BYTES == hb.lib().fl_policy_head_bf16_packed_bytes()
    v = _pack_values(int(starts[-1]), starts[:-1])
    assert not torch.isnan(v).any()
    w = [None] * 38
    for i, (r, k), a, b in zip(MATRICES, shapes, starts[:-1], starts[1:]):
        w[i] = v[a:b].view(r, k).to(DEV)
    guard = torch.full((PACKED_BYTES + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    pk = hb.policy_head_pack_bf16(w, guard[:-64])
    assert pk.numel() == PACKED_BYTES and (guard[-64:] == 0xA5).all()
    exp = torch.cat([_as_packed(w[i].cpu().to(torch.bfloat16).view(torch.int16)) for i in MATRICES])
    got = pk.cpu().view(torch.int16)
    assert torch.equal(got, exp), (got != exp).nonzero().flatten()[:8]
    assert torch.equal(hb.policy_head_pack_bf16(w).cpu().view(torch.int16), exp)
    nan = torch.from_numpy(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF], dtype=np.uint32).view(np.float32))
    w[34] = w[34].clone()
    w[34].view(-1)[5:10] = nan.to(DEV)
    got = torch.isnan(hb.policy_head_pack_bf16(w).cpu().view(torch.bfloat16)[int(starts[-2]):])
    assert torch.equal(got, _as_packed(torch.isnan(w[34].cpu()))) and int(got.sum()) == 5      # NaN where the source has one only


@pytest.mark.gpu
def test_launch_behaviour():
    """value = NULL writes no val and no value; a side stream gives the current stream's bits; B = 1"""
    attr, tree, valid, params, plist, packed = _setup("b2_a33-x1")
    st = run(attr, tree, plist, packed, valid, "hard")
    nov = run(attr, tree, plist, packed, valid, "hard", value=False)
    _intact(nov, value=False)
    assert nov.value is None and (nov.workspace[5632 * 66:5636 * 66] == 0xFF).all()
    assert not _differ(st, nov, ("emb", "xa", "xb", "ao", "qkv", "logits", "actions"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run(attr, tree, plist, packed, valid, "hard")
    side.synchronize()
    assert not _differ(st, got)
    one = run(attr[:1].contiguous(), tree[:1].contiguous(), plist, packed, valid[:1].contiguous(), "hard")
    _intact(one)
    assert torch.equal(one.logits[0], st.logits[0]) and torch.equal(one.value[0], st.value[0]) and torch.equal(one.actions[0], st.actions[0])


# ---------------------------------------------------------------------------------------------------------------- the module
def _direct(attr, tree, params, valid=None, mode=None):
    from flatland_marl_amd import hip_backend as hb
    plist = phs.device_params(params, DEV)
    st = run(attr, tree, plist, hb.policy_head_pack_bf16(plist), valid, mode)
    return st.logits, st.value, st.actions


def _head_params(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.mark.gpu
def test_module_runs_the_bf16_launches():
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd.policy import Network
    attr, tree, valid = (x.to(DEV).contiguous() for x in phs.inputs(3, 11))
    params = ph.seeded_params(7, (2.5, 3.5))
    net = Network(head_precision="bf16").to(DEV)
    net.load_state_dict(params)
    logits, value, actions = _direct(attr, tree, params, valid, "soft")
    with torch.no_grad():
        (l1,), v1, a1 = net.head(attr, tree, valid, "soft")
        assert torch.equal(l1, logits) and torch.equal(v1, value) and torch.equal(a1, actions)
        (l2,), v2 = net.head(attr, tree, value=False)
        assert torch.equal(l2, logits) and v2 is None
    net.trainable = True
    with torch.no_grad():
        assert torch.equal(net.head(attr, tree)[0][0], logits)
    with pytest.raises(ValueError, match="inference only"):
        net.head(attr, tree)
    net.trainable = False
    with pytest.raises(NotImplementedError):
        net.head(attr, tree)[0][0].sum().backward()
    # head_precision="f32": hb.policy_head's bits, and not the bf16 launch's
    net32 = Network.from_module(net, head_precision="f32")
    l32 = hb.policy_head(attr, tree, phs.device_params(params, DEV), torch.empty_like(logits))
    with torch.no_grad():
        assert torch.equal(net32.head(attr, tree)[0][0], l32)
    assert not torch.equal(l32, logits)
    assert Network.from_module(net).head_precision == "bf16"
    net32.head_precision = "bf16"
    with torch.no_grad():
        assert torch.equal(net32.head(attr, tree)[0][0], logits)
    net32.head_precision = "half"
    with pytest.raises(ValueError, match="head_precision"):
        net32.head(attr, tree)


@pytest.mark.gpu
def test_module_repacks_after_the_weights_changed():
    from flatland_marl_amd.policy import Network
    attr, tree, _ = (x.to(DEV).contiguous() for x in phs.inputs(3, 11))
    net = Network(head_precision="bf16").to(DEV)
    net.load_state_dict(ph.seeded_params(7, 1.0))
    with torch.no_grad():
        a = net.head(attr, tree)[0][0].clone()
        net.actor_net[2].weight.mul_(0.5)                                      # an in-place update
        b = net.head(attr, tree)[0][0].clone()
        assert not torch.equal(a, b) and torch.equal(b, _direct(attr, tree, _head_params(net))[0])
        p3 = ph.seeded_params(8, (2.5, 3.5))
        net.load_state_dict(p3)
        c = net.head(attr, tree)[0][0].clone()
        assert not torch.equal(b, c) and torch.equal(c, _direct(attr, tree, p3)[0])
        net.attr_embedding[4].weight = torch.nn.Parameter(net.attr_embedding[4].weight.detach() * 0.25)      # another tensor
        d = net.head(attr, tree)[0][0]
        assert not torch.equal(c, d) and torch.equal(d, _direct(attr, tree, _head_params(net))[0])


@pytest.mark.gpu
def test_network_rolls_out_in_bf16():
    from flatland_marl_amd.policy import Network
    from tests.test_gpu_policy_head import _golden_obs
    net = Network(precision="bf16", head_precision="bf16").to(DEV)
    net.load_state_dict(ph.seeded_params(3, 3.0))
    attr, forest, adj, no, eo, valid = _golden_obs()
    with torch.no_grad():
        tree = net.tree_lstm.roots(forest, adj, no, eo)
        (logits,), value = net(attr, forest, adj, no, eo)
        (l2,), v2 = net.head(attr, tree)
        assert torch.equal(logits, l2) and torch.equal(value, v2)
        assert torch.equal(logits, _direct(attr, tree, _head_params(net))[0])
    for mode in ("soft", "hard"):
        act = net.act(attr, forest, adj, no, eo, valid, mode)
        assert act.dtype == torch.uint8 and act.shape == valid.shape[:2]
        assert (act.cpu().numpy() == ph.choose_actions(logits, valid, mode)).all()
        ok = valid.gather(2, act.long().unsqueeze(-1)).squeeze(-1).bool() | ~valid.any(-1)
        assert ok.all()
