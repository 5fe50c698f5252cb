#!/usr/bin/env python3
"""Time of training the policy head: fl_policy_head_forward_saved / fl_policy_head_backward + the parameter products
(flatland_marl_amd.policy.Network(trainable=True).head) against torch's eager float32 autograd on the same parameters
(Network.head_torch), same device and inputs.  Inputs are synthetic (tests/policy_head_torch.synth_inputs) at one env of cfg2
(1 x 20), cfg2 (256 x 20), cfg3 (1 024 x 80) and cfg5 (256 x 400); the upstream gradients are given on the logits and the value.

Every figure is the median over --launches of the time between two HIP events on the stream, after --warmup calls, with every
buffer allocated beforehand where the call takes buffers (the C entry points); the module's own calls allocate from torch's caching
allocator, warm after the warmup.
  inference_fwd      fl_policy_head, no action choice                saved_fwd        fl_policy_head_forward_saved
  backward_kernels   fl_policy_head_backward                          products         policy.policy_head_param_grads on its rows
  (the four above per chunk of policy.head_chunks, the chunks one after the other, as the module runs them)
  module_fwd         Network.head with grad mode on                   module_bwd       backward() behind it
  module_fwd_bwd     both                                             torch_fwd / torch_bwd / torch_fwd_bwd   head_torch likewise

--parent-lib PARENT.so: fl_policy_head_forward_saved and fl_policy_head_backward of that library (the parent commit's build) and of
this build on the same buffers, --rounds times interleaved: every round's medians, the spread (max - min) of the parent's, and
whether this build's median is behind the parent's by no more than that spread.

--inference-libs A.so B.so ...: the inference forward (fl_policy_head through the C entry point, select = soft) of each library
in turn, --rounds times interleaved: the medians of every round per library, for an A/B of two builds on the same box.

Usage:  python tools/policy_head_backward_bench.py [--launches 20] [--warmup 5] [--inference-libs parent.so new.so]
                                                   [--parent-lib parent.so] [--rounds 5]
                                                   [--out profiles/policy_head_backward_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cfg2_one_env", 1, 20), ("cfg2", 256, 20), ("cfg3", 1024, 80), ("cfg5", 256, 400)]


def median_events(fn, warmup, n, before=None):
    """median ms between two events around fn(); before() runs untimed ahead of every call"""
    import torch
    times = []
    for i in range(warmup + n):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def inference_call(L, vp, attr, tree, plist, valid, mode):
    """a closure that enqueues fl_policy_head of library L (bound: hip_backend.bind) on the current stream with buffers allocated here"""
    import torch
    B, A = attr.shape[:2]
    n = L.fl_policy_head_workspace_bytes(B, A)
    ws = torch.empty(n, dtype=torch.uint8, device=attr.device)
    logits = torch.empty((B, A, 5), device=attr.device)
    value = torch.empty((B,), device=attr.device)
    actions = torch.empty((B, A), dtype=torch.uint8, device=attr.device)
    ptrs = (vp * len(plist))(*[w.data_ptr() for w in plist])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (ws, logits, value, actions, ptrs)

    def call(keep=keep):
        rc = L.fl_policy_head(B, A, attr.data_ptr(), tree.data_ptr(), ptrs, valid.data_ptr() if mode else None, mode, 0.3745401188473625,
                              logits.data_ptr(), value.data_ptr(), actions.data_ptr() if mode else None, ws.data_ptr(), n, s)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inference-libs", nargs="*", default=[])
    ap.add_argument("--parent-lib", default=None, help="libflatland_hip.so of the parent commit, for the A/B of the training entry points")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("policy_head_backward_bench: no GPU visible (the measurement has no CPU path)")
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import policy
    from tests.policy_head_torch import seeded_params, synth_inputs
    dev = torch.device("cuda:0")
    m = policy.Network(trainable=True).to(dev)
    m.load_state_dict(seeded_params(7, (2.5, 3.5)))
    plist = m._head_weights(dev)
    vp = hb.vp
    fwd_saved, bwd = hb._sym("fl_policy_head_forward_saved"), hb._sym("fl_policy_head_backward")
    rows_out, ab = [], {}
    train = {"this": (fwd_saved, bwd)}
    if args.parent_lib:
        P = hb.bind(C.CDLL(os.path.abspath(args.parent_lib)))
        train["parent"] = (P.fl_policy_head_forward_saved, P.fl_policy_head_backward)
    libs = [(p, hb.bind(C.CDLL(os.path.abspath(p)))) for p in args.inference_libs]
    for label, B, A in SHAPES:
        attr, tree, valid = (torch.from_numpy(x).to(dev) for x in synth_inputs(B, A, 11))
        g = torch.Generator().manual_seed(3)
        Rl, Rv = torch.randn((B, A, 5), generator=g).to(dev), torch.randn((B,), generator=g).to(dev)
        r = dict(shape=label, envs=B, agents=A, rows=B * A, chunks=len(policy.head_chunks(B, A)))
        # ---- the C entry points per chunk, buffers allocated beforehand
        parts = []
        for e0, e1 in policy.head_chunks(B, A):
            nb, n = e1 - e0, (e1 - e0) * A
            c = dict(nb=nb, n=n, attr=attr[e0:e1].clone(), tree=tree[e0:e1].clone(), gl=Rl[e0:e1].clone(), gv=Rv[e0:e1].clone(),
                     logits=torch.empty((nb, A, 5), device=dev), value=torch.empty((nb,), device=dev),
                     saved=torch.empty(hb.policy_saved_floats(nb, A), device=dev), rows=torch.empty(n * hb.POLICY_ROW_FLOATS, device=dev),
                     gtree=torch.empty((nb, A, 128), device=dev),
                     ws=torch.empty(max(hb._sym("fl_policy_head_backward_workspace_bytes")(nb, A), 16), dtype=torch.uint8, device=dev))
            c["sv"], c["rw"] = hb.policy_views(c["saved"], hb.POLICY_SAVED_LAYOUT, n), hb.policy_views(c["rows"], hb.POLICY_ROWS_LAYOUT, n)
            parts.append(c)
        ptrs = (vp * len(plist))(*[w.data_ptr() for w in plist])
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        inf = [inference_call(hb.lib(), vp, c["attr"], c["tree"], plist, None, 0) for c in parts]

        def saved_forward(fwd_saved=fwd_saved):
            for c in parts:
                hb._chk(fwd_saved(c["nb"], A, c["attr"].data_ptr(), c["tree"].data_ptr(), ptrs, c["logits"].data_ptr(), c["value"].data_ptr(),
                                  c["saved"].data_ptr(), c["saved"].numel() * 4, s))

        def backward_kernels(bwd=bwd):
            for c in parts:
                hb._chk(bwd(c["nb"], A, c["attr"].data_ptr(), c["tree"].data_ptr(), ptrs, c["saved"].data_ptr(), c["gl"].data_ptr(),
                            c["gv"].data_ptr(), c["gtree"].data_ptr(), c["rows"].data_ptr(), c["rows"].numel() * 4, c["ws"].data_ptr(),
                            c["ws"].numel(), s))

        def products():
            for c in parts:
                policy.policy_head_param_grads(c["attr"].view(c["n"], 83), c["sv"], c["rw"])

        r["inference_fwd_ms"] = median_events(lambda: [f() for f in inf], args.warmup, args.launches)
        r["saved_fwd_ms"] = median_events(saved_forward, args.warmup, args.launches)
        r["backward_kernels_ms"] = median_events(backward_kernels, args.warmup, args.launches)
        r["products_ms"] = median_events(products, args.warmup, args.launches)
        if args.parent_lib:                                      # the training entry points of both builds, interleaved
            us = {"%s_%s" % (who, what): [] for who in ("parent", "this") for what in ("saved_fwd", "backward")}
            for _ in range(args.rounds):
                for who in ("parent", "this"):
                    us[who + "_saved_fwd"].append(round(median_events(lambda: saved_forward(train[who][0]), args.warmup, args.launches) * 1e3, 2))
                    us[who + "_backward"].append(round(median_events(lambda: backward_kernels(train[who][1]), args.warmup, args.launches) * 1e3, 2))
            mid = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
            r["parent_ab"] = dict(us_rounds=us, us_median=mid)
            for what in ("saved_fwd", "backward"):
                spread = round(max(us["parent_" + what]) - min(us["parent_" + what]), 2)
                r["parent_ab"][what] = dict(parent_spread_us=spread, behind_parent_us=round(mid["this_" + what] - mid["parent_" + what], 2),
                                            not_behind_by_more_than_parent_spread=bool(mid["this_" + what] - mid["parent_" + what] <= spread))
        del parts, inf
        torch.cuda.empty_cache()
        # ---- through the module, and torch's eager autograd
        state = {}

        def fwd(head):
            m.zero_grad(set_to_none=True)
            t = tree.detach().clone().requires_grad_(True)
            logits, value = head(attr, t)
            state["out"] = (logits[0], value)

        def back():
            torch.autograd.backward(list(state["out"]), [Rl, Rv])

        for tag, head in (("module", m.head), ("torch", m.head_torch)):
            r[tag + "_fwd_ms"] = median_events(lambda: fwd(head), args.warmup, args.launches)
            r[tag + "_bwd_ms"] = median_events(back, args.warmup, args.launches, before=lambda: fwd(head))
            r[tag + "_fwd_bwd_ms"] = median_events(lambda: (fwd(head), back()), args.warmup, args.launches)
        state.clear()
        r = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        r["saved_fwd_over_inference_fwd"] = round(r["saved_fwd_ms"] / r["inference_fwd_ms"], 3)
        for k in ("fwd", "bwd", "fwd_bwd"):
            r["speedup_%s_vs_torch" % k] = round(r["torch_%s_ms" % k] / r["module_%s_ms" % k], 2)
        rows_out.append(r)
        print(json.dumps(r), flush=True)
        # ---- A/B of the inference forward between libraries
        if libs:
            calls = [(p, inference_call(L, vp, attr, tree, plist, valid, 1)) for p, L in libs]
            ab[label] = {p: [] for p, _ in libs}
            for _ in range(args.rounds):
                for p, call in calls:
                    ab[label][p].append(round(median_events(call, args.warmup, args.launches) * 1e3, 2))
            print(json.dumps({label: ab[label]}), flush=True)
            del calls
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/policy_head_backward_bench.py", device=torch.cuda.get_device_name(0), launches=args.launches,
                           warmup=args.warmup, rounds=args.rounds, parent_lib=bool(args.parent_lib), results=rows_out, inference_forward_us_by_library=ab), f, indent=1)


if __name__ == "__main__":
    main()
