"""The emulation the tolerances of fl_policy_head_bf16 (include/flatland_policy_head_bf16.h) rest on: the restatement of
tests/policy_head_torch.py, float64, with both operands of the 16 bf16 products rounded through bfloat16 once, q k v rounded where
the kernel stores them, and the attention the kernel's: e rounded for e v, the row sum the sum of the ROUNDED e, the quotient last.
attr_embedding.0 (K = 83) and the heads' last layers (K = 128) stay exact; biases, GELU, the maxima and exp are float64.

Built on the mm= hooks of ph.stage_*: the 16 products are exactly those whose K is 256 or 512 (ph.head_shapes), so the hook
rounds by K.  With rounding=False every function is its ph.stage_* counterpart and the chain gives ph.head's bits -- the
attention too: there it IS ph.stage_attention (probabilities first, then p v), as the kernel's order of operations (e v first,
the quotient last) differs from it in the last bit with or without rounding."""
import torch

from tests import policy_head_torch as ph

BF16_K = (256, 512)


def rb(x):
    """x rounded to bfloat16 (to nearest even) in x's own dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def mm16(a, b):
    """the matrix product of the mm= hooks: both operands through bfloat16 where the product is one of the 16"""
    return torch.matmul(rb(a), rb(b)) if a.shape[-1] in BF16_K else torch.matmul(a, b)


def _mm(rounding):
    return mm16 if rounding else torch.matmul


def attention(qkv, rounding=True, dtype=None):
    """[B, A, 256] from q | k | v [B, A, 768] (already rounded when they come from stage_qkv): s = q k^T, e = exp((s - max) / 8),
    e' = bf16(e), (e' v) / sum e'.  dtype: the arithmetic's (None: qkv's)"""
    if not rounding:
        return ph.stage_attention(qkv)
    x = qkv if dtype is None else qkv.to(dtype)
    B, A = x.shape[:2]
    q, k, v = (x[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
    s = torch.matmul(q, k.transpose(-1, -2))
    e = rb(torch.exp((s - s.max(dim=-1, keepdim=True).values) / 8.0))
    ao = torch.matmul(e, v) / e.sum(dim=-1, keepdim=True)
    return ao.permute(0, 2, 1, 3).reshape(B, A, 256)


def stage_attr(attr, p, rounding=True):
    return ph.stage_attr(attr, p, _mm(rounding))


def stage_qkv(y, p, blk, rounding=True):
    out = ph.stage_qkv(y, p, blk, _mm(rounding))
    return rb(out) if rounding else out


def stage_block(y, ao, p, blk, rounding=True):
    return ph.stage_block(y, ao, p, blk, _mm(rounding))


def stage_next(y, p, blk, rounding=True):
    """a whole block from its input: q k v, the attention, out_proj and att_mlp"""
    return stage_block(y, attention(stage_qkv(y, p, blk, rounding), rounding), p, blk, rounding)


def stage_tail(emb, xb, ao, p, rounding=True):
    return ph.stage_tail(emb, xb, ao, p, _mm(rounding))


def stages(agents_attr, tree_embedding, params, rounding=True):
    """every stage chained from the inputs in float64, in ph.stages' names"""
    dtype = torch.float64
    p = ph.stage_params(params, agents_attr.device, dtype)
    out = {}
    out["emb"] = y = torch.cat([stage_attr(agents_attr.to(dtype), p, rounding), tree_embedding.to(dtype)], dim=-1)
    for blk in range(3):
        out["qkv%d" % blk] = stage_qkv(y, p, blk, rounding)
        out["ao%d" % blk] = attention(out["qkv%d" % blk], rounding)
        if blk < 2:
            out[("xa", "xb")[blk]] = y = stage_block(y, out["ao%d" % blk], p, blk, rounding)
    out["qkv"], out["ao"] = out["qkv2"], out["ao2"]
    out["logits"], out["val"] = stage_tail(out["emb"], out["xb"], out["ao"], p, rounding)
    out["value"] = ph.stage_value(out["val"])
    return out


def head(agents_attr, tree_embedding, params, rounding=True):
    """(logits [B, A, 5], value [B]) in float64"""
    st = stages(agents_attr, tree_embedding, params, rounding)
    return st["logits"], st["value"]
