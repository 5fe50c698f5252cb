#!/usr/bin/env python3
"""Time of the PPO entry points (include/flatland_ppo.h) against what a user of the library writes without them, same device, same
buffers.  No speed is promised; the numbers are recorded as what they are.

Shapes: R = 20 (one env of cfg2), 5 120 (cfg2: 256 x 20), 81 920 (cfg3: 1 024 x 80) and 102 400 (cfg5: 256 x 400) rows.  Per shape:
  loss_ms     fl_ppo_loss (hip_call: hip_backend.ppo_loss on outputs allocated once, the workspace from torch's allocator;
              hip_module: policy.ppo_loss + loss.backward() on leaf logits and value) against torch_eager: the same loss in torch's
              eager float32 ops and its autograd (masked log-softmax, gather, exp, clamp, minimum, entropy, means; backward()), with
              the bool mask and the int64 actions made outside the timed part
  sample_ms   fl_policy_sample (hip_call: outputs and u allocated once; hip_module: policy.sample_actions with u = None, so with
              torch.rand and the three outputs' allocation) against head_again: the extra fl_policy_head call with select = soft that
              the trainable head makes today to choose actions under a mode
and once:
  gae_ms      fl_gae at T = 128, N = 256 (hip_call, hip_module = policy.gae) against torch_loop: a Python loop of torch float32 ops
--parent-lib PARENT.so: fl_policy_head (select = soft) of that library and of this build at cfg2 and cfg3 on the same buffers: its
unit was compiled with one more header and must not have moved.

Every figure is the median over --launches of the time between two HIP events on the stream, after --warmup calls; the sides of a
comparison are interleaved --rounds times, and per side the medians of every round, their median and their spread (largest minus
smallest) are kept.  loss_check is |hip total - torch_eager total| of the shape (float32 eager sums against float64 ones).

Usage:  python tools/ppo_bench.py [--launches 20] [--warmup 5] [--rounds 3] [--parent-lib parent.so] [--out profiles/ppo_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.param_grads_bench import ratio, sides  # noqa: E402
from tools.policy_head_backward_bench import SHAPES, inference_call  # noqa: E402

GAE_SHAPE = (128, 256)


def torch_loss(logits, value, valid_bool, actions_i64, old_logp, adv, returns, w, clip, vf_coef, ent_coef):
    """the loss of include/flatland_ppo.h in torch's eager float32 ops (every row has a valid action and takes one)"""
    import torch
    logp = torch.log_softmax(logits.masked_fill(~valid_bool, -1e30), dim=-1)
    entropy = -torch.where(valid_bool, logp.exp() * logp, torch.zeros_like(logp)).sum(-1)
    rho = (logp.gather(-1, actions_i64.unsqueeze(-1)).squeeze(-1) - old_logp).exp()
    s = torch.minimum(rho * adv, rho.clamp(1.0 - clip, 1.0 + clip) * adv)
    n = w.sum()
    return -(w * s).sum() / n + vf_coef * 0.5 * ((value - returns) ** 2).mean() - ent_coef * (w * entropy).sum() / n


def torch_gae(r, v, d, gamma, lam):
    import torch
    nd = 1.0 - (d != 0).float()
    A = torch.zeros_like(r[0])
    adv = torch.empty_like(r)
    for t in reversed(range(r.shape[0])):
        delta = r[t] + gamma * v[t + 1] * nd[t] - v[t]
        A = delta + gamma * lam * nd[t] * A
        adv[t] = A
    return adv, adv + v[:-1]


def shape(label, B, A, args, dev, parent):
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import policy
    from tests.policy_head_torch import seeded_params, synth_inputs
    net = policy.Network().to(dev)
    net.load_state_dict(seeded_params(7, (2.5, 3.5)))
    plist = net._head_weights(dev)
    attr, tree, valid = (torch.from_numpy(x).to(dev) for x in synth_inputs(B, A, 11))
    valid[..., 2] |= (valid.sum(-1) == 0).to(torch.uint8)          # every row a valid action: torch_eager has no row to leave out
    g = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        (logits,), value = net.head(attr, tree)
    u = torch.rand((B, A), dtype=torch.float64, device=dev, generator=g)
    actions, logp = torch.empty((B, A), dtype=torch.uint8, device=dev), torch.empty((B, A), device=dev)
    entropy = torch.empty((B, A), device=dev)
    r = dict(shape=label, envs=B, agents=A, rows=B * A)

    # ---- sampling
    calls = dict(hip_call=lambda: hb.policy_sample(logits, valid, u, actions, logp, entropy),
                 hip_module=lambda: policy.sample_actions(logits, valid, generator=g),
                 head_again=inference_call(hb.lib(), hb.vp, attr, tree, plist, valid, 1))
    r["sample_ms"] = sides(calls, args.rounds, args.warmup, args.launches)
    r["sample_head_again_over_hip_call"] = ratio(r["sample_ms"]["head_again"], r["sample_ms"]["hip_call"])
    hb.policy_sample(logits, valid, u, actions, logp, entropy)

    # ---- the loss
    old_logp = logp + 0.2 * torch.randn((B, A), device=dev, generator=g)
    adv, returns = torch.randn((B, A), device=dev, generator=g), torch.randn((B,), device=dev, generator=g)
    mask = (torch.rand((B, A), device=dev, generator=g) < 0.9).to(torch.uint8)
    w, valid_bool, actions_i64 = mask.float(), valid != 0, actions.long()
    gl, gv, st = torch.empty_like(logits), torch.empty_like(value), torch.empty(8, dtype=torch.float64, device=dev)
    leaf_l, leaf_v = logits.clone().requires_grad_(True), value.clone().requires_grad_(True)

    def module():
        leaf_l.grad = leaf_v.grad = None
        policy.ppo_loss(leaf_l, leaf_v, valid, actions, old_logp, adv, returns, mask, 0.2, 0.5, 0.01)[0].backward()

    def eager():
        leaf_l.grad = leaf_v.grad = None
        torch_loss(leaf_l, leaf_v, valid_bool, actions_i64, old_logp, adv, returns, w, 0.2, 0.5, 0.01).backward()

    calls = dict(hip_call=lambda: hb.ppo_loss(logits, valid, actions, old_logp, adv, mask, value, returns, 0.2, 0.5, 0.01, gl, gv, st),
                 hip_module=module, torch_eager=eager)
    r["loss_ms"] = sides(calls, args.rounds, args.warmup, args.launches)
    r["loss_torch_eager_over_hip_call"] = ratio(r["loss_ms"]["torch_eager"], r["loss_ms"]["hip_call"])
    r["loss_torch_eager_over_hip_module"] = ratio(r["loss_ms"]["torch_eager"], r["loss_ms"]["hip_module"])
    with torch.no_grad():
        ref = torch_loss(logits, value, valid_bool, actions_i64, old_logp, adv, returns, w, 0.2, 0.5, 0.01)
    hb.ppo_loss(logits, valid, actions, old_logp, adv, mask, value, returns, 0.2, 0.5, 0.01, gl, gv, st)
    eager()
    r["loss_check"] = dict(total=float(st[3]), abs_diff_to_torch_eager=abs(float(st[3]) - float(ref)),
                           grad_logits_max_abs_diff=float((gl - leaf_l.grad).abs().max()), counted_rows=int(st[6]))

    # ---- the inference path of the unit that took the new header
    if parent is not None and label in ("cfg2", "cfg3"):
        calls = dict(parent=inference_call(parent, hb.vp, attr, tree, plist, valid, 1),
                     this=inference_call(hb.lib(), hb.vp, attr, tree, plist, valid, 1))
        r["inference_fl_policy_head_ms"] = sides(calls, args.rounds, args.warmup, args.launches)
    return r


def gae_shape(args, dev):
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import policy
    T, N = GAE_SHAPE
    g = torch.Generator(device=dev).manual_seed(5)
    rw, v = torch.randn((T, N), device=dev, generator=g), torch.randn((T + 1, N), device=dev, generator=g)
    d = (torch.rand((T, N), device=dev, generator=g) < 0.02).to(torch.uint8)
    adv, ret = torch.empty_like(rw), torch.empty_like(rw)
    calls = dict(hip_call=lambda: hb.gae(rw, v, d, 0.99, 0.95, adv, ret), hip_module=lambda: policy.gae(rw, v, d),
                 torch_loop=lambda: torch_gae(rw, v, d, 0.99, 0.95))
    r = dict(steps=T, columns=N, gae_ms=sides(calls, args.rounds, args.warmup, args.launches))
    r["gae_torch_loop_over_hip_call"] = ratio(r["gae_ms"]["torch_loop"], r["gae_ms"]["hip_call"])
    hb.gae(rw, v, d, 0.99, 0.95, adv, ret)
    r["gae_check_max_abs_diff"] = float((adv - torch_gae(rw, v, d, 0.99, 0.95)[0]).abs().max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libflatland_hip.so of the parent commit, for the A/B of fl_policy_head")
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from flatland_marl_amd import hip_backend as hb
    assert torch.cuda.is_available(), "tools/ppo_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    parent = hb.bind(C.CDLL(os.path.abspath(args.parent_lib))) if args.parent_lib else None
    hb.lib()
    results = []
    for label, B, A in SHAPES:
        if args.shapes is not None and label not in args.shapes:
            continue
        r = shape(label, B, A, args, dev, parent)
        results.append(r)
        print(json.dumps(r), flush=True)
    gae = gae_shape(args, dev)
    print(json.dumps(gae), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/ppo_bench.py", device=torch.cuda.get_device_name(0), launches=args.launches, warmup=args.warmup,
                           rounds=args.rounds, parent_lib=bool(args.parent_lib), shapes=results, gae=gae), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
