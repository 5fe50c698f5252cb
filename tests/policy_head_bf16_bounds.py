"""A-priori bounds, per element, of the two stages of fl_policy_head_bf16 whose bf16 operands are fully visible in the workspace.
u16 = 2^-8: a bfloat16 has 8 significant bits, so rounding to nearest changes a value by at most u16 relatively (half of the
spacing 2^-7 just above a power of two), as u = 2^-24 of tests/policy_head_bounds.py is float32's.  The float32 terms are that
file's.  Nothing here is fitted to a kernel; tests/test_policy_head_bf16.py holds float32 emulations inside both bounds on the CPU.

  qkv from xb    The kernel rounds xb and in_proj to bf16, sums the (exact) products in float32 from zero, adds the float32 bias
                 and rounds the result to bf16.  ref = the float64 product of the rounded operands plus the bias; d = pb.qkv's
                 bound evaluated ON THE ROUNDED OPERANDS bounds the float32 sum s: |s - ref| <= d.  The stored value is
                 s (1 + delta), |delta| <= u16, so |stored - ref| <= d + u16 |s| <= d + u16 (|ref| + d).

  ao from qkv    From the stored q, k, v: e_j = exp((s_j - max) / 8), o = sum_j e_j v_j / sum_j e_j = sum_j p_j v_j.  The kernel
                 uses e'_j = e_j (1 + delta_j), |delta_j| <= u16, in BOTH sums: o' = sum_j p'_j v_j with
                 p'_j = e_j (1 + delta_j) / sum_k e_k (1 + delta_k) = p_j (1 + delta_j) / (1 + D), D = sum_k p_k delta_k the
                 p-weighted mean of the delta, |D| <= u16.  So |p'_j / p_j - 1| = |delta_j - D| / (1 + D) <= 2 u16 / (1 - u16) and
                 |o' - o| <= sum_j |p'_j - p_j| |v_j| <= 2 u16 / (1 - u16) sum_j p_j |v_j|.
                 On top of it pb.attention's float32 terms (the scores, expf, the two float32 sums, the quotient), which take the
                 place of e_j here: the two perturbations of a weight multiply, (1 + eta)(1 + delta), and the cross term
                 eta * delta -- second order, at most 2^-8 of the float32 terms -- is not carried.
                 ref = ph.stage_attention of the stored q k v, float64."""
import torch

from tests import policy_head_bounds as pb
from tests import policy_head_torch as ph
from tests.policy_head_bf16_torch import rb

U16 = 2.0 ** -8


def qkv(y, p, blk):
    """(ref, bound) [B, A, 768] of the stored q | k | v of block blk from the block's float64 input y (the kernel's own xb)"""
    t = "transformer.%d.attention." % blk
    W, b = rb(p[t + "in_proj_weight"]), p[t + "in_proj_bias"]
    yr = rb(y)
    ref = yr @ W.T + b
    d = pb.linear(yr, W, b)
    return ref, d + U16 * (ref.abs() + d)


def attention(qkv64, c):
    """(ref, bound) [B, A, 256] of the attention output from the stored q | k | v as float64"""
    B, A = qkv64.shape[:2]
    q, k, v = (qkv64[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
    pr = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    extra = (2.0 * U16 / (1.0 - U16)) * (pr @ v.abs()).permute(0, 2, 1, 3).reshape(B, A, 256)
    return ph.stage_attention(qkv64), pb.attention(qkv64, c) + extra
