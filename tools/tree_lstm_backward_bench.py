#!/usr/bin/env python3
"""Time of the trainable tree encoder's backward (policy.TreeLSTM(trainable=True): fl_tree_lstm_backward + the parameter
products) on real trees: obs_policy() of the workload batches after a few synthetic steps, as tools/tree_lstm_bench.py takes them.
Shapes: one cfg2 env (20 trees), cfg2 (5 120), cfg3 (81 920); loss = sum(R * roots).

Per shape:
  inference_forward_ms      roots() under no_grad (the forward's launch, tools/tree_lstm_bench.py's figure)
  train_forward_ms          roots() with grad mode on (every node, c kept, the saved tensors)
  backward_ms               loss.backward() alone: the chunks' kernel launches and parameter products
  backward_kernel_ms        fl_tree_lstm_backward alone over all chunks (HIP events around the launches; buffers allocated before)
  eager_f32_forward_backward_ms / eager_f32_backward_ms
                            torch's eager float32 autograd through the level loop (tests/tree_lstm_grad_torch.py) on the same
                            box and inputs: the comparison (the parent commit has no backward)
  ratios                    backward / inference forward, kernel / inference forward, eager backward / backward
Wall times are medians of --reps runs, each from the call to a device sync.

Usage:  python tools/tree_lstm_backward_bench.py [--reps 10] [--warmup 3] [--shapes cfg2_1env cfg2 cfg3] [--out profiles/tree_lstm_backward_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, workload, envs, max_nodes)
SHAPES = [("cfg2_1env", "cfg2", 1, 31), ("cfg2", "cfg2", 256, 31), ("cfg3", "cfg3", 1024, 31)]


def median_ms(fn, reps, warmup, setup=None):
    import torch
    out = []
    for k in range(warmup + reps):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(arg) if setup else fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return out[len(out) // 2]


def kernel_ms(m, x, h, c, up, reps, warmup):
    """fl_tree_lstm_backward over all chunks, by HIP events (the buffers of the largest chunk are made once)"""
    import torch
    from flatland_marl_amd import hip_backend as hb, policy
    B, A, N = x[2].shape
    T, M = B * A, 128
    chunk = min(T, policy.BACKWARD_CHUNK_TREES)
    n = chunk * N
    dev = x[0].device
    da, dc, dg, q = (torch.empty((n, w), device=dev) for w in (3 * M, M, 3 * M, 3 * M))
    child = torch.empty((n, 3), dtype=torch.int32, device=dev)
    ws = list(m._weights(dev))
    xs = [x[0].view(T, N, 12), x[1].view(T, N - 1, 3), x[2].view(T, N), x[3].view(T, N - 1)]
    adjs = []
    for t0 in range(0, T, chunk):
        a = xs[1][t0:t0 + chunk]
        adjs.append(torch.where(a >= 0, a - t0 * N, a) if t0 else a)      # (the kernel reads the parent and child columns only)
    times = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i, t0 in enumerate(range(0, T, chunk)):
            t1 = min(T, t0 + chunk)
            k_ = (t1 - t0) * N
            hb.tree_lstm_backward(xs[0][t0:t1], adjs[i], xs[2][t0:t1], xs[3][t0:t1], ws, h[t0 * N:t1 * N], c[t0 * N:t1 * N],
                                  up[t0:t1], True, da[:k_], dc[:k_], dg[:k_].view(k_, 3, M), q[:k_], child[:k_])
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_lstm_backward_bench: no GPU visible (the measurement has no CPU path)")
    from flatland_marl_amd import hip_backend as hb, policy
    from tests import tree_lstm_grad_torch as tg
    from tests.tree_lstm_torch import seeded_params
    from tools.tree_lstm_bench import inputs
    m = policy.TreeLSTM(trainable=True).cuda()
    m.load_state_dict(seeded_params(7))
    params = {k: v.detach() for k, v in m.named_parameters()}
    rows = []
    for label, wl_name, B, N in SHAPES:
        if label not in args.shapes:
            continue
        x = inputs(wl_name, B, N)
        T = x[2].shape[0] * x[2].shape[1]
        up = torch.randn(T, 128, device="cuda")

        def infer():
            with torch.no_grad():
                m.roots(*x)

        def fwd():
            return (m.roots(*x).view(T, 128) * up).sum()

        def eager_fwd():
            p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            return (tg.tree_lstm(*x, p, torch.float32).view(T, N, 128)[:, 0] * up).sum()

        r = dict(shape=label, workload=wl_name, envs=B, trees=T, nodes=N, chunk_trees=policy.BACKWARD_CHUNK_TREES,
                 chunks=-(-T // policy.BACKWARD_CHUNK_TREES))
        r["inference_forward_ms"] = median_ms(infer, args.reps, args.warmup)
        r["train_forward_ms"] = median_ms(fwd, args.reps, args.warmup)
        r["backward_ms"] = median_ms(lambda loss: loss.backward(), args.reps, args.warmup, setup=fwd)
        h, c = torch.empty((T * N, 128), device="cuda"), torch.empty((T * N, 128), device="cuda")
        hb.tree_lstm(*x, m._weights(x[0].device), False, h, c)
        r["backward_kernel_ms"] = kernel_ms(m, x, h, c, up, args.reps, args.warmup)
        del h, c
        r["eager_f32_forward_backward_ms"] = median_ms(lambda: eager_fwd().backward(), args.eager_reps, 1)
        r["eager_f32_backward_ms"] = median_ms(lambda loss: loss.backward(), args.eager_reps, 1, setup=eager_fwd)
        r["peak_memory_MB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        r["ratios"] = dict(backward_to_inference_forward=r["backward_ms"] / r["inference_forward_ms"],
                           kernel_to_inference_forward=r["backward_kernel_ms"] / r["inference_forward_ms"],
                           eager_backward_to_backward=r["eager_f32_backward_ms"] / r["backward_ms"],
                           eager_step_to_step=r["eager_f32_forward_backward_ms"] / (r["train_forward_ms"] + r["backward_ms"]))
        r = {k: (round(v, 4) if isinstance(v, float) else {a: round(b, 2) for a, b in v.items()} if isinstance(v, dict) else v)
             for k, v in r.items()}
        rows.append(r)
        print(json.dumps(r), flush=True)
        m.zero_grad(set_to_none=True)
        del x, up
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/tree_lstm_backward_bench.py", device=torch.cuda.get_device_name(0), reps=args.reps,
                           warmup=args.warmup, eager_reps=args.eager_reps, results=rows), f, indent=1)


if __name__ == "__main__":
    main()
