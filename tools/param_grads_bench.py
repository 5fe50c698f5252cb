#!/usr/bin/env python3
"""Time of the parameter gradients: fl_policy_head_param_grads / fl_tree_lstm_param_grads (param_grads="hip",
include/flatland_param_grads.h) against the float32 torch products of policy.policy_head_param_grads / policy.tree_lstm_param_grads
(param_grads="torch"), on the rows a real backward left, same device, same buffers.

Shapes: the head at one env of cfg2 (1 x 20), cfg2 (256 x 20), cfg3 (1 024 x 80) and cfg5 (256 x 400) on synthetic inputs
(tests/policy_head_torch.synth_inputs); the encoder at cfg2 and cfg3 on obs_policy() of the workload batches
(tools/tree_lstm_bench.inputs).  Per shape:
  products_ms         the parameter-gradient step alone over the chunks the module runs, "torch" and "hip", --rounds times interleaved
  module_bwd_ms       backward() through the module, both settings, interleaved likewise;  module_fwd_bwd_ms  forward + backward
  torch_bwd_ms / torch_fwd_bwd_ms   torch's eager float32 autograd (Network.head_torch; the level loop of tests/tree_lstm_grad_torch)
Every figure is the median over --launches of the time between two HIP events on the stream, after --warmup calls; per side the
medians of every round, their median and their spread (largest minus smallest) are kept.  The head's share of the FP32 matrix peak
counts 2 * 1 693 184 FLOP a row (the weights' elements; 3.4 MFLOP) against 157.3 TFLOP/s.

--parent-lib PARENT.so: fl_policy_head (select = soft) and fl_tree_lstm (roots only) of that library and of this build on the same
buffers, --rounds times interleaved: the inference path, which this unit must not move.

Usage:  python tools/param_grads_bench.py [--launches 10] [--warmup 3] [--rounds 3] [--parent-lib parent.so] [--only head|tree]
                                          [--budget-s 500] [--out profiles/param_grads_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.policy_head_backward_bench import SHAPES as HEAD_SHAPES, inference_call, median_events  # noqa: E402

TREE_SHAPES = [("cfg2", "cfg2", 256, 31), ("cfg3", "cfg3", 1024, 31)]
HEAD_FLOP_PER_ROW = 2 * 1693184
FP32_MATRIX_PEAK = 157.3e12


def sides(fns, rounds, warmup, launches, before=None):
    """{side: dict(rounds=[medians, ms], median, spread)} of the closures fns[side], interleaved round by round"""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(round(median_events(fn, warmup, launches, before=None if before is None else before[k]), 4))
    return {k: dict(rounds=v, median=sorted(v)[len(v) // 2], spread=round(max(v) - min(v), 4)) for k, v in out.items()}


def ratio(a, b):
    return round(a["median"] / b["median"], 3)


def head_shape(label, B, A, args, dev, parent):
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import policy
    from tests.policy_head_torch import seeded_params, synth_inputs
    m = policy.Network(trainable=True).to(dev)
    m.load_state_dict(seeded_params(7, (2.5, 3.5)))
    mh = policy.Network.from_module(m, trainable=True, param_grads="hip")
    plist = m._head_weights(dev)
    attr, tree, valid = (torch.from_numpy(x).to(dev) for x in synth_inputs(B, A, 11))
    g = torch.Generator().manual_seed(3)
    Rl, Rv = torch.randn((B, A, 5), generator=g).to(dev), torch.randn((B,), generator=g).to(dev)
    r = dict(shape=label, envs=B, agents=A, rows=B * A, chunks=len(policy.head_chunks(B, A)))
    parts = []
    for e0, e1 in policy.head_chunks(B, A):                     # the rows of a real backward, per chunk
        nb, n = e1 - e0, (e1 - e0) * A
        c = dict(n=n, attr=attr[e0:e1].clone(), saved=torch.empty(hb.policy_saved_floats(nb, A), device=dev),
                 rows=torch.empty(n * hb.POLICY_ROW_FLOATS, device=dev))
        lg, va, gt = torch.empty((nb, A, 5), device=dev), torch.empty((nb,), device=dev), torch.empty((nb, A, 128), device=dev)
        hb.policy_head_forward_saved(c["attr"], tree[e0:e1].clone(), plist, lg, va, c["saved"])
        hb.policy_head_backward(c["attr"], tree[e0:e1].clone(), plist, c["saved"], Rl[e0:e1].clone(), Rv[e0:e1].clone(), gt, c["rows"])
        c["sv"], c["rw"] = hb.policy_views(c["saved"], hb.POLICY_SAVED_LAYOUT, n), hb.policy_views(c["rows"], hb.POLICY_ROWS_LAYOUT, n)
        c["ws"] = torch.empty(max(16, hb._sym("fl_policy_head_param_grads_workspace_bytes")(n, 0)), dtype=torch.uint8, device=dev)
        parts.append(c)
    fns = dict(torch=lambda: [policy.policy_head_param_grads(c["attr"].view(c["n"], 83), c["sv"], c["rw"]) for c in parts],
               hip=lambda: [hb.policy_head_param_grads(c["attr"], c["saved"], c["rows"], workspace=c["ws"]) for c in parts])
    r["products_ms"] = sides(fns, args.rounds, args.warmup, args.launches)
    del parts, fns
    torch.cuda.empty_cache()
    state = {}

    def fwd(head, net):
        net.zero_grad(set_to_none=True)
        t = tree.detach().clone().requires_grad_(True)
        logits, value = head(attr, t)
        state["out"] = (logits[0], value)

    def back():
        torch.autograd.backward(list(state["out"]), [Rl, Rv])
    heads = dict(torch=(m.head, m), hip=(mh.head, mh))
    r["module_bwd_ms"] = sides({k: back for k in heads}, args.rounds, args.warmup, args.launches,
                               before={k: (lambda k=k: fwd(*heads[k])) for k in heads})
    r["module_fwd_bwd_ms"] = sides({k: (lambda k=k: (fwd(*heads[k]), back())) for k in heads}, args.rounds, args.warmup, args.launches)
    eager = dict(eager=back)
    r["torch_bwd_ms"] = sides(eager, args.rounds, args.warmup, args.launches, before=dict(eager=lambda: fwd(m.head_torch, m)))["eager"]
    r["torch_fwd_bwd_ms"] = sides(dict(eager=lambda: (fwd(m.head_torch, m), back())), args.rounds, args.warmup, args.launches)["eager"]
    state.clear()
    p = r["products_ms"]
    r["hip_products_speedup_vs_torch_products"] = ratio(p["torch"], p["hip"])
    r["beyond_both_spreads"] = bool(abs(p["torch"]["median"] - p["hip"]["median"]) > p["torch"]["spread"] + p["hip"]["spread"])
    for side in ("torch", "hip"):
        r["bwd_speedup_vs_torch_autograd_" + side] = ratio(r["torch_bwd_ms"], r["module_bwd_ms"][side])
        r["fwd_bwd_speedup_vs_torch_autograd_" + side] = ratio(r["torch_fwd_bwd_ms"], r["module_fwd_bwd_ms"][side])
    r["hip_products_share_of_fp32_matrix_peak"] = round(B * A * HEAD_FLOP_PER_ROW / (p["hip"]["median"] * 1e-3) / FP32_MATRIX_PEAK, 4)
    if parent is not None:
        calls = dict(parent=inference_call(parent, hb.vp, attr, tree, plist, valid, 1),
                     this=inference_call(hb.lib(), hb.vp, attr, tree, plist, valid, 1))
        r["inference_fl_policy_head_ms"] = sides(calls, args.rounds, args.warmup, args.launches)
    return r


def tree_shape(label, wl_name, B, N, args, dev, parent):
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import policy
    from tests import tree_lstm_grad_torch as tg
    from tests.tree_lstm_torch import seeded_params
    from tools.tree_lstm_bench import inputs
    m = policy.TreeLSTM(trainable=True).to(dev)
    m.load_state_dict(seeded_params(7))
    mh = policy.TreeLSTM.from_module(m, trainable=True, param_grads="hip")
    params = {k: v.detach() for k, v in m.named_parameters()}
    x = inputs(wl_name, B, N)
    T, M = x[2].shape[0] * x[2].shape[1], 128
    up = torch.randn(T, M, device=dev)
    ws = list(m._weights(dev))
    r = dict(shape=label, workload=wl_name, envs=B, trees=T, nodes=N, rows=T * N, chunks=-(-T // policy.BACKWARD_CHUNK_TREES))
    h, c = torch.empty((T * N, M), device=dev), torch.empty((T * N, M), device=dev)
    hb.tree_lstm(*x, ws, False, h, c)
    xs = [x[0].view(T, N, 12), x[1].view(T, N - 1, 3), x[2].view(T, N), x[3].view(T, N - 1)]
    parts = []
    for t0 in range(0, T, policy.BACKWARD_CHUNK_TREES):         # the rows of a real backward, per chunk
        t1 = min(T, t0 + policy.BACKWARD_CHUNK_TREES)
        n = (t1 - t0) * N
        a = xs[1][t0:t1]
        a = torch.where(a >= 0, a - t0 * N, a) if t0 else a       # (the kernel reads the parent and child columns only)
        da, dc, dg, q = (torch.empty(s, device=dev) for s in ((n, 3 * M), (n, M), (n, 3, M), (n, 3 * M)))
        child = torch.empty((n, 3), dtype=torch.int32, device=dev)
        hb.tree_lstm_backward(xs[0][t0:t1], a, xs[2][t0:t1], xs[3][t0:t1], ws, h[t0 * N:t1 * N], c[t0 * N:t1 * N], up[t0:t1], True,
                              da, dc, dg, q, child)
        parts.append((xs[0][t0:t1].reshape(n, 12), xs[2][t0:t1].reshape(n), h[t0 * N:t1 * N], da, dc, dg, q, child))
    wsp = torch.empty(max(16, hb._sym("fl_tree_lstm_param_grads_workspace_bytes")(parts[0][0].shape[0], 0)), dtype=torch.uint8, device=dev)
    fns = dict(torch=lambda: [policy.tree_lstm_param_grads(*p) for p in parts],
               hip=lambda: [hb.tree_lstm_param_grads(*p, workspace=wsp) for p in parts])
    r["products_ms"] = sides(fns, args.rounds, args.warmup, args.launches)
    del parts, fns, h, c
    torch.cuda.empty_cache()
    state = {}

    def fwd(mod):
        mod.zero_grad(set_to_none=True)
        state["loss"] = (mod.roots(*x).view(T, M) * up).sum()

    def eager_fwd():
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        state["loss"] = (tg.tree_lstm(*x, p, torch.float32).view(T, N, M)[:, 0] * up).sum()

    def back():
        state["loss"].backward()
    mods = dict(torch=m, hip=mh)
    r["module_bwd_ms"] = sides({k: back for k in mods}, args.rounds, args.warmup, args.launches,
                               before={k: (lambda k=k: fwd(mods[k])) for k in mods})
    r["module_fwd_bwd_ms"] = sides({k: (lambda k=k: (fwd(mods[k]), back())) for k in mods}, args.rounds, args.warmup, args.launches)
    r["torch_bwd_ms"] = sides(dict(eager=back), args.rounds, 1, args.eager_launches, before=dict(eager=eager_fwd))["eager"]
    r["torch_fwd_bwd_ms"] = sides(dict(eager=lambda: (eager_fwd(), back())), args.rounds, 1, args.eager_launches)["eager"]
    state.clear()
    p = r["products_ms"]
    r["hip_products_speedup_vs_torch_products"] = ratio(p["torch"], p["hip"])
    r["beyond_both_spreads"] = bool(abs(p["torch"]["median"] - p["hip"]["median"]) > p["torch"]["spread"] + p["hip"]["spread"])
    for side in ("torch", "hip"):
        r["bwd_speedup_vs_torch_autograd_" + side] = ratio(r["torch_bwd_ms"], r["module_bwd_ms"][side])
        r["fwd_bwd_speedup_vs_torch_autograd_" + side] = ratio(r["torch_fwd_bwd_ms"], r["module_fwd_bwd_ms"][side])
    if parent is not None:
        out = torch.empty((T, M), device=dev)
        need = hb._sym("fl_tree_lstm_workspace_bytes")(T, N, 1)
        wsi = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(L):
            rc = L.fl_tree_lstm(T, N, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr(), *[w.data_ptr() for w in ws], 1,
                                out.data_ptr(), None, None, wsi.data_ptr(), wsi.numel(), s)
            assert rc == 0, rc
        r["inference_fl_tree_lstm_ms"] = sides(dict(parent=lambda: call(parent), this=lambda: call(hb.lib())), args.rounds, args.warmup,
                                               args.launches)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--eager-launches", type=int, default=3, help="the encoder's eager level loop is slow: fewer calls a round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("head", "tree"), default=None)
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--parent-lib", default=None, help="libflatland_hip.so of the parent commit, for the A/B of the inference path")
    ap.add_argument("--budget-s", type=float, default=500.0, help="no new shape is started after this many seconds")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("param_grads_bench: no GPU visible (the measurement has no CPU path)")
    from flatland_marl_amd import hip_backend as hb
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = hb.bind(C.CDLL(os.path.abspath(args.parent_lib)))
    t0, results, skipped = time.perf_counter(), dict(head=[], tree=[]), []
    jobs = [("head", s) for s in HEAD_SHAPES] + [("tree", s) for s in TREE_SHAPES]
    for kind, shape in jobs:
        if (args.only and kind != args.only) or (args.shapes is not None and shape[0] not in args.shapes):
            continue
        if time.perf_counter() - t0 > args.budget_s:
            skipped.append("%s:%s" % (kind, shape[0]))
            continue
        r = (head_shape if kind == "head" else tree_shape)(*shape, args, dev, parent)
        results[kind].append(r)
        print(json.dumps(dict(kind=kind, **r)), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/param_grads_bench.py", device=torch.cuda.get_device_name(0), launches=args.launches,
                           eager_launches=args.eager_launches, warmup=args.warmup, rounds=args.rounds, parent_lib=bool(args.parent_lib),
                           head_flop_per_row=HEAD_FLOP_PER_ROW, fp32_matrix_peak_flops=FP32_MATRIX_PEAK, skipped=skipped, **results),
                      f, indent=1)


if __name__ == "__main__":
    main()
