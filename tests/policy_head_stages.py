"""fl_policy_head with a workspace of the test's own, so that every intermediate the call leaves there can be checked (the layout:
DESIGN.md, "the workspace layout the tests pin"), the cases of tests/test_policy_head_stages.py (CPU) and
tests/test_gpu_policy_head_stages.py (GPU), and the one table of stage checks both use: each stage's float64 restatement
(tests/policy_head_torch.py) computed from the PREVIOUS stage of whatever is under test, with its a-priori bound
(tests/policy_head_bounds.py)."""
import ctypes as C
import types

import numpy as np
import torch

from tests import policy_head_bounds as pb
from tests import policy_head_torch as ph

NAMES = [n for n, _ in ph.head_shapes()]
GUARD = 4096
# (stage, offset in floats a row, floats a row) of the workspace, R = B * A rows each
LAYOUT = (("emb", 0, 256), ("xa", 256, 256), ("xb", 512, 256), ("ao", 768, 256), ("qkv", 1024, 768), ("val", 1792, 1))
STAGES = tuple(n for n, _, _ in LAYOUT)

SCALES = (1.0, (2.5, 3.5))
SHAPES = ((70, 1), (33, 2), (3, 11), (5, 13), (2, 31), (2, 32), (2, 33), (1, 63), (1, 64), (1, 65), (1, 1024))
PUSHED_SHAPES = ((3, 11), (2, 33), (1, 65), (1, 1024))
PUSHES = ("sharp", "flat", "constv")
PARAM_SEED, INPUT_SEED = 7, 11
# the input seeds at which the float64 reference of the sharp case meets its two conditions (tests/test_policy_head_stages.py).
# At A = 1024 no single seed can: the winners are the few dozen keys of largest norm (24 parameter x 24 input seeds: at most 46
# distinct winning keys, in at most 28 of the 32 chunks), so the case is run at three seeds whose winners together fall in every chunk.
SHARP_SEEDS = {(3, 11): (11,), (2, 33): (12,), (1, 65): (16,), (1, 1024): (16, 6, 1)}
IN_PROJ = "transformer.2.attention.in_proj_"


def device_params(params, dev):
    """the 38 tensors in the header's order, float32 contiguous on dev"""
    return [params[n].detach().to(device=dev, dtype=torch.float32).contiguous() for n in NAMES]


def run(attr, tree, plist, valid=None, mode=None, u=None, fill=0xFF, value=True):
    """one fl_policy_head call on torch's current stream.  The workspace is fl_policy_head_workspace_bytes long, every byte `fill`
    before the call (0xFF: every float a NaN), with GUARD bytes of 0xA5 behind it.  Returns logits [B, A, 5], value [B], actions
    [B, A] (None without a mode), the stages as [B, A, .] views of the workspace, and guard."""
    from flatland_marl_amd import hip_backend as hb
    B, A = attr.shape[:2]
    R, dev = B * A, attr.device
    assert len(plist) == hb.POLICY_HEAD_NPARAMS and attr.is_contiguous() and tree.is_contiguous()
    nbytes = hb._sym("fl_policy_head_workspace_bytes")(B, A)
    assert nbytes >= R * (7 * 256 + 1) * 4
    out = types.SimpleNamespace(B=B, A=A)
    with torch.cuda.device(dev):
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=dev)
        buf[:nbytes].fill_(fill)
        buf[nbytes:].fill_(0xA5)
        out.logits = torch.full((B, A, 5), float("nan"), device=dev)
        out.value = torch.full((B,), float("nan"), device=dev) if value else None
        out.actions = torch.full((B, A), 77, dtype=torch.uint8, device=dev) if mode else None
        ptrs = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in plist])
        opt = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        s = torch.cuda.current_stream(dev).cuda_stream
        hb._chk(hb._sym("fl_policy_head")(B, A, attr.data_ptr(), tree.data_ptr(), ptrs, opt(valid) if mode else None,
                                          hb.POLICY_SELECT[mode], hb.POLICY_U_REFERENCE if u is None else float(u),
                                          out.logits.data_ptr(), opt(out.value), opt(out.actions), buf.data_ptr(), nbytes, C.c_void_p(s)))
    ws = buf[:R * (7 * 256 + 1) * 4].view(torch.float32)
    for name, off, n in LAYOUT:
        st = ws[off * R:(off + n) * R]
        setattr(out, name, st.view(B, A) if n == 1 else st.view(B, A, n))
    out.workspace, out.guard = buf[:nbytes], buf[nbytes:]
    return out


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def same_bits(a, b, names=STAGES + ("logits", "value", "actions")):
    """the names of the stages and outputs whose bits differ between two run() results"""
    return [n for n in names if getattr(a, n) is not None and not torch.equal(bits(getattr(a, n)), bits(getattr(b, n)))]


# ---------------------------------------------------------------------------------------------------------------- the cases
def inputs(B, A, seed=INPUT_SEED):
    return tuple(torch.from_numpy(x) for x in ph.synth_inputs(B, A, seed))


def params(scale_index):
    return ph.seeded_params(PARAM_SEED, SCALES[scale_index])


def pushed_params(kind, A):
    """the second scale's parameters with block 2's in_proj edited: `sharp` q rows x 64, `flat` q rows zero (every score equal),
    `constv` v rows' weight zero and their bias a seeded vector (returned as well)."""
    p = dict(params(1))
    W, b, c = p[IN_PROJ + "weight"].clone(), p[IN_PROJ + "bias"].clone(), None
    if kind == "sharp":
        W[:256] *= 64.0
        b[:256] *= 64.0
    elif kind == "flat":
        W[:256] = 0.0
        b[:256] = 0.0
    else:
        c = torch.from_numpy(np.random.default_rng([5, A]).uniform(-2.0, 2.0, size=256).astype(np.float32))
        W[512:] = 0.0
        b[512:] = c
    p[IN_PROJ + "weight"], p[IN_PROJ + "bias"] = W, b
    return p, c


def constv_tolerance(c, A):
    """f64 [256]: how far ao[..., j] may lie from the constant v c[j]: sum_j p_j c / sum_j p_j with the sum, the accumulation of
    the products and the division at (A + 2) u relatively -- gamma_{A+2} |c| -- and never less than 4 float32 ulps of c.  (4 ulps
    alone is no bound: a float32 sum from the left is 5, 9 and 12 ulps away at A = 11, 33 and 65.)"""
    ulp = torch.from_numpy(np.spacing(np.abs(c.numpy()))).double()
    return torch.maximum(4.0 * ulp, pb.gamma(A + 2) * c.double().abs())


def sharp_cases(B, A):
    """the ids of the sharp cases of a shape, one per seed"""
    return ["b%d_a%d-sharp%s" % (B, A, "_%d" % i if i else "") for i in range(len(SHARP_SEEDS[(B, A)]))]


# the action choice on constructed logits: differences are 0 or 200, so exp gives exactly 1 or exactly 0 (exp(-200) = 1.4e-87 is
# far below the smallest float32 subnormal 1.4e-45) and the float32 softmax is 1 / n or 0 whatever expf is
BIG = 200.0
CHOICE_VECTORS = dict(
    equal=[0.0] * 5,
    holes=[0.0, -BIG, 0.0, -BIG, 0.0],
    holes_complement=[-BIG, 0.0, -BIG, 0.0, -BIG],
    **{"dominant%d" % i: [BIG if j == i else 0.0 for j in range(5)] for i in range(5)},
    tie_0_3=[BIG, -BIG, 0.0, BIG, -BIG],
    tie_1_4=[-BIG, BIG, -BIG, 0.0, BIG],
)
CHOICE_SHAPES = ((1, 32), (2, 33))
MASKS = np.array([[(m >> a) & 1 for a in range(5)] for m in range(32)], dtype=np.uint8)


def choice_masks(B, A):
    """u8 [B, A, 5]: the 32 valid-action masks, repeated over the rows"""
    return MASKS[np.arange(B * A) % 32].reshape(B, A, 5)


def choice_params(vector):
    p = dict(params(1))
    p["actor_net.4.weight"] = torch.zeros_like(p["actor_net.4.weight"])
    p["actor_net.4.bias"] = torch.tensor(CHOICE_VECTORS[vector], dtype=torch.float32)
    return p


def choice_draws(vector):
    """every u the choice is tested at: each distinct step below 1 of the CDF of every mask, its float64 neighbours, 0 and the
    largest double below 1"""
    lg = np.array(CHOICE_VECTORS[vector], dtype=np.float32)
    steps = sorted({float(s) for m in MASKS for s in ph.cdf_of(lg, m) if s < 1.0})
    us = {0.0, float(np.nextafter(1.0, 0.0))}
    for s in steps:
        us |= {s, float(np.nextafter(s, -1.0)), float(np.nextafter(s, 2.0))}
    return sorted(x for x in us if 0.0 <= x < 1.0)


def isolated_attr_params(real):
    """the second scale's parameters with every attr_embedding layer but `real` a rectangular identity with a zero bias: products
    by 1 and 0 and sums of zeros are exact, so emb[..., :128] carries the error of ONE layer (and of four GELUs) and the chained bound
    stays near a single layer's -- through four seeded layers it grows to the size of the embedding itself"""
    p = dict(params(1))
    for i in (0, 2, 4, 6):
        if i != real:
            W = p["attr_embedding.%d.weight" % i]
            p["attr_embedding.%d.weight" % i], p["attr_embedding.%d.bias" % i] = torch.eye(*W.shape), torch.zeros(W.shape[0])
    return p


TAIL_LAYERS = ("out_proj", "att_mlp", "head0", "head2", "head4")


def isolated_tail_params(real):
    """the same for the five layers from (emb, xb, ao) to logits and val: every layer but `real` (head0 / head2 / head4: that layer
    of actor_net AND of critic_net) passes its input on -- out_proj an identity, att_mlp and the heads' first layer [0 | I] (the
    attention's side, the block's side), the later ones a rectangular identity -- with a zero bias"""
    p = dict(params(1))
    eye_right = torch.cat([torch.zeros(256, 256), torch.eye(256)], dim=1)
    names = dict(out_proj=[("transformer.2.attention.out_proj", torch.eye(256))], att_mlp=[("transformer.2.att_mlp.0", eye_right)],
                 head0=[(n + ".0", eye_right) for n in ("actor_net", "critic_net")],
                 head2=[(n + ".2", torch.eye(128, 256)) for n in ("actor_net", "critic_net")],
                 head4=[("actor_net.4", torch.eye(5, 128)), ("critic_net.4", torch.eye(1, 128))])
    for layer, subst in names.items():
        if layer != real:
            for name, W in subst:
                assert p[name + ".weight"].shape == W.shape
                p[name + ".weight"], p[name + ".bias"] = W.clone(), torch.zeros(W.shape[0])
    return p


def golden_case(name, s):
    from tests.test_policy_head_golden import golden_inputs, golden_params, load
    g = load(name)
    return golden_inputs(g, s) + (golden_params(g, s),)


def _cases():
    """id -> a function returning (attr, tree, valid, params) on the CPU, for every case of the stage tests"""
    out = {}
    for B, A in SHAPES:
        for s in range(2):
            out["b%d_a%d-x%d" % (B, A, s)] = lambda B=B, A=A, s=s: inputs(B, A) + (params(s),)
    for name in ("synth_b1_a1", "synth_b3_a1"):
        for s in range(2):
            out["%s-x%d" % (name, s)] = lambda name=name, s=s: golden_case(name, s)
    for B, A in PUSHED_SHAPES:
        for cid, seed in zip(sharp_cases(B, A), SHARP_SEEDS[(B, A)]):
            out[cid] = lambda B=B, A=A, seed=seed: inputs(B, A, seed) + (pushed_params("sharp", A)[0],)
        for kind in PUSHES[1:]:
            out["b%d_a%d-%s" % (B, A, kind)] = lambda B=B, A=A, kind=kind: inputs(B, A) + (pushed_params(kind, A)[0],)
    for real in (0, 2, 4, 6):
        out["b3_a11-attr%d_alone" % real] = lambda real=real: inputs(3, 11) + (isolated_attr_params(real),)
    for real in TAIL_LAYERS:
        out["b3_a11-%s_alone" % real] = lambda real=real: inputs(3, 11) + (isolated_tail_params(real),)
    for B, A in CHOICE_SHAPES:
        for v in CHOICE_VECTORS:
            out["b%d_a%d-choice_%s" % (B, A, v)] = lambda B=B, A=A, v=v: inputs(B, A) + (choice_params(v),)
    return out


CASES = _cases()
STAGE_CASES = [k for k in CASES if "choice" not in k]        # the cases whose stages the GPU test checks and records


# ---------------------------------------------------------------------------------------------------------------- the stage checks
CHECKED = ("emb_attr", "qkv", "ao", "logits", "val", "value")


def stage_checks(st, attr, p64, c, only=CHECKED):
    """name -> (what is under test, float64, its restatement from the previous stage OF WHAT IS UNDER TEST, the bound), per element.
    st: an object or dict with emb, xb, ao, qkv, val [B, A, .] and logits, value; attr on the same device; p64 = ph.stage_params."""
    g = (lambda n: st[n].double()) if isinstance(st, dict) else (lambda n: getattr(st, n).double())
    a64 = attr.double()
    out = {}
    if "emb_attr" in only:
        out["emb_attr"] = (g("emb")[..., :128], ph.stage_attr(a64, p64), pb.attr(a64, p64, c))
    if "qkv" in only:
        out["qkv"] = (g("qkv"), ph.stage_qkv(g("xb"), p64, 2), pb.qkv(g("xb"), p64, 2))
    if "ao" in only:
        out["ao"] = (g("ao"), ph.stage_attention(g("qkv")), pb.attention(g("qkv"), c))
    if "logits" in only or "val" in only:
        logits, val = ph.stage_tail(g("emb"), g("xb"), g("ao"), p64)
        d_logits, d_val = pb.tail(g("emb"), g("xb"), g("ao"), p64, c)
        out["logits"], out["val"] = (g("logits"), logits, d_logits), (g("val"), val, d_val)
    if "value" in only:
        out["value"] = (g("value"), ph.stage_value(g("val")), pb.value(g("val")))
    return out


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (inf where anything is not finite or a zero bound is exceeded)"""
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all() and torch.isfinite(bound).all() and (bound >= 0).all()):
        return float("inf")
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(r.max())


def rms(x):
    return float(x.double().pow(2).mean().sqrt())
