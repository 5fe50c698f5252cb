"""The project's own restatement of the policy network after its tree encoder (solution/nn/net_tree.py:82-103) and of the actor's
choice of an action (solution/plfActor.py:30-46), written from the math in plain torch ops (no nn.MultiheadAttention), float64 by
default, on any device.  Pinned to the reference's outputs by tests/test_policy_head_golden.py; the GPU tests compare
fl_policy_head with it.

  x        = attr_embedding(agents_attr): Linear 83 -> 256 -> 256 -> 256 -> 128, exact (erf) GELU after each
  emb      = [x | tree_embedding]                                                           [B, A, 256]
  block i  : q, k, v = rows 0..255, 256..511, 512..767 of in_proj (y) ; head h = columns 64 h .. 64 h + 63
             p = softmax over the A agents of the same env of q k^T / 8 ; o = out_proj([p v of the 4 heads])
             y <- GELU(att_mlp([y | o]))        (y = emb before block 0; no residual, no layer norm)
  logits   = actor_net([emb | y]), value = mean over the agents of critic_net([emb | y])     (512 -> 256 -> 128 -> 5 / 1)

  action   : p = softmax of the valid actions' logits in float32, as numpy on a float32 array.  soft: numpy.random.choice's draw
             with the uniform number u -- float64 cumsum(p) / its last element, searchsorted(u, side="right"); the reference seeds
             numpy with 42 before every draw, so u = U_REFERENCE.  hard: the first largest p.  No valid action: 0.
"""
import math

import numpy as np
import torch

U_REFERENCE = 0.3745401188473625      # numpy.random.RandomState(42).random_sample()
TREE_SHAPES = [("tree_lstm.W_iou.weight", (384, 12)), ("tree_lstm.W_iou.bias", (384,)), ("tree_lstm.U_iou.weight", (384, 384)),
               ("tree_lstm.W_c.weight", (128, 384)), ("tree_lstm.W_c.bias", (128,)), ("tree_lstm.W_f.weight", (128, 12)),
               ("tree_lstm.W_f.bias", (128,)), ("tree_lstm.U_f.weight", (128, 128))]


def head_shapes():
    """(name, shape) of the Network's state_dict without tree_lstm.*, in state_dict order"""
    out = []
    for i, (o, k) in zip((0, 2, 4, 6), ((256, 83), (256, 256), (256, 256), (128, 256))):
        out += [("attr_embedding.%d.weight" % i, (o, k)), ("attr_embedding.%d.bias" % i, (o,))]
    for i in range(3):
        t = "transformer.%d." % i
        out += [(t + "attention.in_proj_weight", (768, 256)), (t + "attention.in_proj_bias", (768,)),
                (t + "attention.out_proj.weight", (256, 256)), (t + "attention.out_proj.bias", (256,)),
                (t + "att_mlp.0.weight", (256, 512)), (t + "att_mlp.0.bias", (256,))]
    for n, last in (("actor_net", 5), ("critic_net", 1)):
        for i, (o, k) in zip((0, 2, 4), ((256, 512), (128, 256), (last, 128))):
            out += [("%s.%d.weight" % (n, i), (o, k)), ("%s.%d.bias" % (n, i), (o,))]
    return out


def seeded_params(seed, scales=1.0, names_shapes=None):
    """the goldens' weights: numpy.random.default_rng(seed), each parameter in state_dict order (tree_lstm.* first), float32,
    uniform in +-scale/sqrt(fan_in) -- a bias takes the bound of the weight before it.  scales: one number, or (scale, the scale
    of the attention's in_proj weights and biases)."""
    scale, in_proj = (scales, scales) if np.isscalar(scales) else (float(scales[0]), float(scales[1]))
    if names_shapes is None:
        names_shapes = TREE_SHAPES + head_shapes()
    rng = np.random.default_rng(seed)
    out, bound = {}, None
    for name, shape in names_shapes:
        if len(shape) == 2:
            bound = (in_proj if "in_proj" in name else scale) / np.sqrt(shape[1])
        out[name] = torch.from_numpy(rng.uniform(-bound, bound, size=shape).astype(np.float32))
    return out


def synth_inputs(B, A, seed):
    """Gaussian agents_attr f32 [B, A, 83] and tree_embedding f32 [B, A, 128] (x 0.5: a TreeLSTM's h lies in (-1, 1)), and a
    random valid-action mask u8 [B, A, 5] in which every fourth agent has no valid action and every fourth a single one"""
    rng = np.random.default_rng([seed, B, A])
    attr = rng.standard_normal((B, A, 83)).astype(np.float32)
    tree = (0.5 * rng.standard_normal((B, A, 128))).astype(np.float32)
    valid = rng.integers(0, 2, size=(B, A, 5)).astype(np.uint8)
    kind = (np.arange(B * A).reshape(B, A) + seed) % 4
    valid[kind == 0] = 0
    one = rng.integers(0, 5, size=(B, A))
    single = np.zeros((B, A, 5), dtype=np.uint8)
    np.put_along_axis(single, one[..., None], 1, axis=2)
    valid[kind == 1] = single[kind == 1]
    return attr, tree, valid


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def head(agents_attr, tree_embedding, params, dtype=torch.float64, with_probs=False):
    """(logits [B, A, 5], value [B]) in `dtype` on the inputs' device; with_probs: also the attention probabilities of the three
    blocks, [B, 4, A, A] each"""
    dev = agents_attr.device
    p = {k: v.detach().to(device=dev, dtype=dtype) for k, v in params.items() if not k.startswith("tree_lstm.")}
    lin = lambda x, name: x @ p[name + ".weight"].T + p[name + ".bias"]     # noqa: E731
    x = agents_attr.to(dtype)
    B, A = x.shape[:2]
    for i in (0, 2, 4, 6):
        x = gelu(lin(x, "attr_embedding.%d" % i))
    emb = torch.cat([x, tree_embedding.to(dtype)], dim=-1)
    y, probs = emb, []
    for i in range(3):
        t = "transformer.%d." % i
        qkv = y @ p[t + "attention.in_proj_weight"].T + p[t + "attention.in_proj_bias"]
        q, k, v = (qkv[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(-1, -2) / 8.0
        s = s - s.max(dim=-1, keepdim=True).values
        e = torch.exp(s)
        pr = e / e.sum(dim=-1, keepdim=True)
        probs.append(pr)
        o = lin((pr @ v).permute(0, 2, 1, 3).reshape(B, A, 256), t + "attention.out_proj")
        y = gelu(lin(torch.cat([y, o], dim=-1), t + "att_mlp.0"))
    both = torch.cat([emb, y], dim=-1)

    def mlp(name):
        h = gelu(lin(both, name + ".0"))
        return lin(gelu(lin(h, name + ".2")), name + ".4")
    logits, value = mlp("actor_net"), mlp("critic_net").mean(dim=1).reshape(-1)
    return (logits, value, probs) if with_probs else (logits, value)


# ---------------------------------------------------------------------------------------------------------------- stage by stage
# The same network cut at the places where fl_policy_head leaves an intermediate in its workspace ("the workspace layout
# the tests pin"), so that a test can compute each stage from the kernel's own previous stage.  Every function takes and returns
# [B, A, .] tensors of one dtype and uses head()'s own ops in head()'s order: chained in float64 they give head()'s bits
# (tests/test_policy_head_stages.py).  mm = the matrix product: torch.matmul, or matmul_seq for a float32 sum in a fixed order.
# rec = None or a dict of lists that takes the arguments of every erf ("erf") and exp ("exp") on the way.
def matmul_seq(a, b):
    """a @ b with the products summed strictly from the left: every product and every sum rounded on its own (no FMA)"""
    acc = a[..., :, 0:1] * b[..., 0:1, :]
    for k in range(1, a.shape[-1]):
        acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return acc


def stage_params(params, device, dtype=torch.float64):
    return {k: v.detach().to(device=device, dtype=dtype) for k, v in params.items() if not k.startswith("tree_lstm.")}


def _gelu(x, rec):
    if rec is not None:
        rec["erf"].append(x / math.sqrt(2.0))
    return gelu(x)


def _lin(x, p, name, mm, weight="weight", bias="bias"):
    return mm(x, p[name + weight].T) + p[name + bias]


def stage_attr(attr, p, mm=torch.matmul, rec=None):
    """emb[..., :128]: the four layers of attr_embedding, GELU after each"""
    x = attr
    for i in (0, 2, 4, 6):
        x = _gelu(_lin(x, p, "attr_embedding.%d." % i, mm), rec)
    return x


def stage_qkv(y, p, blk, mm=torch.matmul):
    """[B, A, 768]: q | k | v of block blk from its input"""
    return _lin(y, p, "transformer.%d.attention." % blk, mm, "in_proj_weight", "in_proj_bias")


def stage_attention(qkv, mm=torch.matmul, rec=None, with_probs=False):
    """[B, A, 256]: softmax(q k^T / 8) v of the four heads side by side, before out_proj"""
    B, A = qkv.shape[:2]
    q, k, v = (qkv[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
    s = mm(q, k.transpose(-1, -2)) / 8.0
    s = s - s.max(dim=-1, keepdim=True).values
    if rec is not None:
        rec["exp"].append(s)
    e = torch.exp(s)
    den = e.sum(dim=-1, keepdim=True) if mm is torch.matmul else mm(e, torch.ones_like(e[..., :1, :]).transpose(-1, -2))
    pr = e / den
    ao = mm(pr, v).permute(0, 2, 1, 3).reshape(B, A, 256)
    return (ao, pr) if with_probs else ao


def stage_block(y, ao, p, blk, mm=torch.matmul, rec=None):
    """the block's output = the next block's input: GELU(att_mlp([y | out_proj(ao)]))"""
    t = "transformer.%d." % blk
    o = _lin(ao, p, t + "attention.out_proj.", mm)
    return _gelu(_lin(torch.cat([y, o], dim=-1), p, t + "att_mlp.0.", mm), rec)


def stage_heads(emb, y, p, mm=torch.matmul, rec=None):
    """(logits [B, A, 5], val [B, A]): actor_net and critic_net on [emb | y]"""
    both = torch.cat([emb, y], dim=-1)

    def mlp(name):
        h = _gelu(_lin(both, p, name + ".0.", mm), rec)
        return _lin(_gelu(_lin(h, p, name + ".2.", mm), rec), p, name + ".4.", mm)
    return mlp("actor_net"), mlp("critic_net")[..., 0]


def stage_tail(emb, xb, ao, p, mm=torch.matmul, rec=None):
    """what k_ph_block<true> computes from the workspace: block 2 after its attention, then the heads"""
    return stage_heads(emb, stage_block(xb, ao, p, 2, mm, rec), p, mm, rec)


def stage_value(val):
    """[B]: the mean of the agents' critic values"""
    return val.unsqueeze(-1).mean(dim=1).reshape(-1)


def stages(agents_attr, tree_embedding, params, dtype=torch.float64, mm=torch.matmul, rec=None):
    """every stage chained from the inputs, in the workspace's names: emb, xa, xb, ao and qkv (block 2's; ao0, ao1, qkv0, qkv1 the
    earlier blocks'), val, and the outputs logits and value"""
    p = stage_params(params, agents_attr.device, dtype)
    out = {}
    out["emb"] = y = torch.cat([stage_attr(agents_attr.to(dtype), p, mm, rec), tree_embedding.to(dtype)], dim=-1)
    for blk in range(3):
        out["qkv%d" % blk] = stage_qkv(y, p, blk, mm)
        out["ao%d" % blk] = stage_attention(out["qkv%d" % blk], mm, rec)
        if blk < 2:
            out[("xa", "xb")[blk]] = y = stage_block(y, out["ao%d" % blk], p, blk, mm, rec)
    out["qkv"], out["ao"] = out["qkv2"], out["ao2"]
    out["logits"], out["val"] = stage_tail(out["emb"], out["xb"], out["ao"], p, mm, rec)
    out["value"] = stage_value(out["val"])
    return out


def _probabilities(logits, valid):
    """the valid actions of one agent and their float32 softmax, as numpy computes it on a float32 array"""
    idx = np.flatnonzero(valid)
    x = np.asarray(logits, dtype=np.float32)[idx]
    e = np.exp(x - x.max())
    return idx, e / e.sum()


def cdf_of(logits, valid):
    """what numpy.random.choice compares u with: the float64 cumulative sum of p over its last element (empty: no valid action)"""
    if not np.any(valid):
        return np.zeros(0)
    _, pr = _probabilities(logits, valid)
    c = np.cumsum(pr.astype(np.float64))
    return c / c[-1]


def choose_actions(logits, valid, mode, u=U_REFERENCE):
    """uint8 [...]: the action of every agent from logits f32 [..., 5] and the mask [..., 5]"""
    lg = np.asarray(logits.detach().cpu() if isinstance(logits, torch.Tensor) else logits, dtype=np.float32).reshape(-1, 5)
    va = np.asarray(valid.cpu() if isinstance(valid, torch.Tensor) else valid).reshape(-1, 5)
    out = np.zeros(len(lg), dtype=np.uint8)
    for i in range(len(lg)):
        if not va[i].any():
            continue
        idx, pr = _probabilities(lg[i], va[i])
        if mode == "hard":
            out[i] = idx[int(np.argmax(pr))]
        else:
            c = np.cumsum(pr.astype(np.float64))
            out[i] = idx[min(int(np.searchsorted(c / c[-1], u, side="right")), len(idx) - 1)]
    return out.reshape(np.asarray(valid.cpu() if isinstance(valid, torch.Tensor) else valid).shape[:-1])


def exempt(logits, valid, mode, eps, u=U_REFERENCE):
    """bool [...]: agents whose action eps of error in the logits may change.  soft: a cumulative probability within 8 eps of u;
    hard: the two largest valid logits within 2 eps of each other."""
    lg = np.asarray(logits, dtype=np.float32).reshape(-1, 5)
    va = np.asarray(valid).reshape(-1, 5)
    out = np.zeros(len(lg), dtype=bool)
    for i in range(len(lg)):
        n = int(np.count_nonzero(va[i]))
        if n < 2:
            continue
        if mode == "hard":
            top = np.sort(lg[i][va[i] != 0].astype(np.float64))
            out[i] = top[-1] - top[-2] <= 2 * eps
        else:
            out[i] = bool((np.abs(cdf_of(lg[i], va[i])[:-1] - u) <= 8 * eps).any())
    return out.reshape(np.asarray(valid).shape[:-1])


def tolerance(e32, out, R=1.0):
    """R * e32 + one float32 ulp of the largest |output| of the case"""
    m = float(np.abs(np.asarray(out, dtype=np.float64)).max())
    return R * float(e32) + float(np.spacing(np.float32(m)))
