"""A-priori forward error bounds of fl_policy_head's stages, per output element, in float64 from a stage's actual inputs.  They hold
for a float32 evaluation in ANY summation order, with or without FMA (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3):
u = 2^-24, gamma_n = n u / (1 - n u).  Nothing here is fitted to a kernel; tests/test_policy_head_stages.py holds two float32
restatements inside every bound, on the CPU.

  linear      y = x W^T + b over K terms: |dy| <= gamma_{K+1} (|x| |W|^T + |b|).  An input known only within d_in adds d_in |W|^T
              (and d_in to |x|).
  GELU        0.5 z (1 + erf(z / sqrt 2)): the input's error times 1.13 >= sup |GELU'| = 1.1289, plus the evaluation's own: the
              argument z / sqrt 2 within 2 u (the constant, the product), erf within C ulps of max(|argument|, |result|), the sum
              and the product one rounding each.
  attention   from q, k, v: ds_ij = (gamma_64 sum_d |q_id| |k_jd| + 2 u |s_ij|) / 8 (s = q k^T before the scale),
              eta_i = expm1(max_j ds_ij) + C u, |do_id| <= 2 (eta_i + gamma_{A+2}) sum_j p_ij |v_jd| / (1 - eta_i - gamma_{A+2})
              + u |o_id|.  The shift by the row maximum cancels between numerator and denominator, so only ds enters; the rounding
              of s_ij - max is at most u (|s_ij| + |max|) <= 8 max_j ds_ij.
  value       the mean of A numbers: gamma_{A+1} mean |val| + u |value|.

C, the allowance for erff and expf in float32 ulps, is not taken from a kernel: tests/golden/policy_head_stage_errors.json holds the
largest error of torch's float32 erf and exp on the CPU over the arguments of every test case, and C = twice that, rounded up, at
least 4 (the device's functions are other implementations of the same functions).
"""
import json
import math
import os

import torch

U = 2.0 ** -24
GELU_SLOPE = 1.13
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_head_stage_errors.json")


def gamma(n):
    return n * U / (1.0 - n * U)


def allowance():
    """C of the committed record"""
    return int(json.load(open(RECORD))["c"])


def allowance_of(measured):
    return max(4, int(math.ceil(2.0 * measured)))


def ulps(err, *magnitudes):
    """err in float32 ulps of the largest of the magnitudes (an ulp of m is at most 2^-23 |m|; never below the smallest subnormal)"""
    m = magnitudes[0].abs()
    for x in magnitudes[1:]:
        m = torch.maximum(m, x.abs())
    return err / torch.clamp(m * 2.0 ** -23, min=2.0 ** -149)


def linear(x, W, b, d_in=None):
    """bound of x W^T + b, [..., out]; x [..., K] the input the reference used, d_in [..., K] the bound on the kernel's own input"""
    K = W.shape[1]
    aW = W.abs().T
    if d_in is None:
        return gamma(K + 1) * (x.abs() @ aW + b.abs())
    return gamma(K + 1) * ((x.abs() + d_in) @ aW + b.abs()) + d_in @ aW


def gelu(z, dz, c):
    """bound of GELU evaluated in float32 at an argument within dz of z"""
    zm = z.abs() + dz
    a = zm / math.sqrt(2.0)
    d_erf = GELU_SLOPE * 2 * U * a + c * 2.0 ** -23 * torch.maximum(a, torch.clamp(GELU_SLOPE * a, max=1.0))
    t = torch.clamp(1.0 + torch.erf(z / math.sqrt(2.0)) + GELU_SLOPE * dz / math.sqrt(2.0), max=2.0)       # |1 + erf| at the kernel's argument
    dt = d_erf + U * (t + d_erf)
    h = 0.5 * zm
    return GELU_SLOPE * dz + h * dt + U * h * (t + dt)


def mlp(x, layers, c, d_in=None):
    """(the float64 result, its bound) of a chain of linear layers with no observable intermediate; layers = [(W, b, GELU after?)]"""
    d = d_in
    for W, b, act in layers:
        z = x @ W.T + b
        d = linear(x, W, b, d)
        if act:
            x, d = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))), gelu(z, d, c)
        else:
            x = z
    return x, d


def _layer(p, name, act, weight="weight", bias="bias"):
    return p[name + weight], p[name + bias], act


def attr(attr_in, p, c):
    """bound of emb[..., :128] from agents_attr"""
    return mlp(attr_in, [_layer(p, "attr_embedding.%d." % i, True) for i in (0, 2, 4, 6)], c)[1]


def qkv(y, p, blk):
    return linear(y, p["transformer.%d.attention.in_proj_weight" % blk], p["transformer.%d.attention.in_proj_bias" % blk])


def attention(qkv64, c):
    """bound of the attention output [B, A, 256] from q | k | v [B, A, 768]"""
    B, A = qkv64.shape[:2]
    q, k, v = (qkv64[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
    s = q @ k.transpose(-1, -2)
    ds = (gamma(64) * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * s.abs()) / 8.0
    eta = (torch.expm1(ds.max(dim=-1, keepdim=True).values) + c * U) + gamma(A + 2)
    pr = torch.softmax(s / 8.0, dim=-1)
    d = 2.0 * eta * (pr @ v.abs()) / (1.0 - eta) + U * (pr @ v).abs()
    return d.permute(0, 2, 1, 3).reshape(B, A, 256)


def tail(emb, xb, ao, p, c):
    """bounds of (logits [B, A, 5], val [B, A]) from the workspace's emb, xb and block 2's attention output: five layers each"""
    t = "transformer.2."
    o, d_o = mlp(ao, [_layer(p, t + "attention.out_proj.", False)], c)
    y, d_y = mlp(torch.cat([xb, o], dim=-1), [_layer(p, t + "att_mlp.0.", True)], c, torch.cat([torch.zeros_like(xb), d_o], dim=-1))
    both, d_both = torch.cat([emb, y], dim=-1), torch.cat([torch.zeros_like(emb), d_y], dim=-1)
    out = [mlp(both, [_layer(p, n + ".0.", True), _layer(p, n + ".2.", True), _layer(p, n + ".4.", False)], c, d_both)[1]
           for n in ("actor_net", "critic_net")]
    return out[0], out[1][..., 0]


def value(val):
    """bound of value [B] from val [B, A]"""
    A = val.shape[1]
    return gamma(A + 1) * val.abs().mean(dim=1) + U * val.mean(dim=1).abs()
