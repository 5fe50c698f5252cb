"""A differentiable restatement of the policy network after its tree encoder: tests/policy_head_torch.head's ops in head()'s
order (chained in float64 it gives head()'s bits, tests/test_policy_head_grad_golden.py), on parameters that may require grad, and
keeping every intermediate where fl_policy_head_backward leaves a row (include/flatland_policy_train.h), so that retain_grad gives
the float64 gradient at the same place.  Pinned to the reference Network's own autograd by tests/test_policy_head_grad_golden.py;
what the GPU tests hold fl_policy_head_backward to.

The names of `keep` are the rows' (hip_backend.POLICY_ROWS_LAYOUT): "attr.dz0" is the pre-activation of attr_embedding.0 -- its
gradient is that row -- "attr.h1" the layer's output; "dqkv0" block 0's q | k | v, "dc0" its attention output c, "do0" out_proj's
output o (whose value is the row "o0"), "dz0" att_mlp's pre-activation, "dy0" the block's input (emb), "dy3" the last block's
output; "actor.dz0", ".dz2", ".dz4" the pre-activations of actor_net (".dz4" = the logits), "actor.u1", ".u2" its hidden outputs.
"""
import torch

from tests import policy_head_torch as ph

NAMES = [n for n, _ in ph.head_shapes()]
ACTOR = [n for n in NAMES if n.startswith("actor_net.")]
CRITIC = [n for n in NAMES if n.startswith("critic_net.")]


def leaf_params(params, device, dtype):
    """name -> a fresh leaf that requires grad, for the 38 head parameters"""
    return {k: params[k].detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k in NAMES}


def forward(attr, tree, p, keep=None):
    """(logits [B, A, 5], value [B]) in the dtype of p's tensors, differentiable with respect to them and to tree; keep: a dict that
    takes the intermediates (each with retain_grad)"""
    def note(name, t):
        if keep is not None:
            if t.requires_grad:
                t.retain_grad()
            keep[name] = t
        return t

    def lin(x, name, w="weight", b="bias"):
        return x @ p[name + w].T + p[name + b]
    dtype = p[NAMES[0]].dtype
    x = attr.to(dtype)
    B, A = x.shape[:2]
    for n, i in enumerate((0, 2, 4, 6)):
        x = ph.gelu(note("attr.dz%d" % i, lin(x, "attr_embedding.%d." % i)))
        if i < 6:
            note("attr.h%d" % (n + 1), x)
    y = emb = note("dy0", torch.cat([x, tree.to(dtype)], dim=-1))
    for i in range(3):
        t = "transformer.%d." % i
        qkv = note("dqkv%d" % i, lin(y, t + "attention.", "in_proj_weight", "in_proj_bias"))
        q, k, v = (qkv[..., 256 * j:256 * (j + 1)].reshape(B, A, 4, 64).permute(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(-1, -2) / 8.0
        s = s - s.max(dim=-1, keepdim=True).values
        e = torch.exp(s)
        pr = e / e.sum(dim=-1, keepdim=True)
        c = note("dc%d" % i, (pr @ v).permute(0, 2, 1, 3).reshape(B, A, 256))
        o = note("do%d" % i, lin(c, t + "attention.out_proj."))
        y = note("dy%d" % (i + 1), ph.gelu(note("dz%d" % i, lin(torch.cat([y, o], dim=-1), t + "att_mlp.0."))))
    both = torch.cat([emb, y], dim=-1)

    def mlp(name, tag):
        u1 = note(tag + ".u1", ph.gelu(note(tag + ".dz0", lin(both, name + ".0."))))
        u2 = note(tag + ".u2", ph.gelu(note(tag + ".dz2", lin(u1, name + ".2."))))
        return note(tag + ".dz4", lin(u2, name + ".4."))
    logits, value = mlp("actor_net", "actor"), mlp("critic_net", "critic").mean(dim=1).reshape(-1)
    return logits, value


def loss_of(logits, value, Rl, Rv):
    """sum(Rl * logits) + sum(Rv * value); a None weight leaves its term out"""
    terms = []
    if Rl is not None:
        terms.append((logits * Rl.to(device=logits.device, dtype=logits.dtype)).sum())
    if Rv is not None:
        terms.append((value * Rv.to(device=value.device, dtype=value.dtype)).sum())
    return sum(terms)


def grads(attr, tree, params, Rl, Rv, dtype=torch.float64, stages=False):
    """the gradients of loss_of on the inputs' device: a dict with the 38 parameter names and "tree" (zeros where the loss does not
    reach); stages: the gradient at every name of `keep` too, and "value:<name>" = the intermediate itself"""
    dev = attr.device
    p = leaf_params(params, dev, dtype)
    t = tree.detach().to(dtype).clone().requires_grad_(True)
    keep = {} if stages else None
    logits, value = forward(attr, t, p, keep)
    loss_of(logits, value, Rl, Rv).backward()
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in p.items()}
    out["tree"] = t.grad
    if stages:
        for k, v in keep.items():
            out[k] = torch.zeros_like(v) if v.grad is None else v.grad
            out["value:" + k] = v.detach()
    return out


def rel_error(g, g64):
    """max |g - g64| / max |g64|; where g64 is identically zero: 0.0 if g is too, else inf"""
    den = float(g64.abs().max())
    num = float((g.double() - g64.double()).abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def upstream(B, A, seed=9):
    """(Rl f32 [B, A, 5], Rv f32 [B]): standard normal, non-zero on every output"""
    g = torch.Generator().manual_seed(seed * 1000003 + B * 1031 + A)
    return torch.randn((B, A, 5), generator=g, dtype=torch.float32), torch.randn((B,), generator=g, dtype=torch.float32)
