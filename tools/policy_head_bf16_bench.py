#!/usr/bin/env python3
"""fl_policy_head_bf16 against fl_policy_head, on the synthetic inputs and seeded weights of tools/policy_head_bench.py: one env of
cfg2 (1 x 20), cfg2 (256 x 20), cfg3 (1 024 x 80) and cfg5 (256 x 400), logits, value and the "soft" action.

Times are HIP-event medians around one call through the C entry points (8 kernel launches), buffers allocated beforehand.  With
--parent-lib the calls alternate in --rounds interleaved rounds between fl_policy_head of that library (the parent commit's
build), fl_policy_head of this build and fl_policy_head_bf16 of this build -- and, where the parent exports it, the parent's own
fl_policy_head_bf16; a round's figure is the median of --launches calls.  Per shape the file holds every round's medians, the
spread (max - min) of the parent's, whether this build's float32 median lies inside the parent's range, and whether the bf16
median is below the parent's by more than that spread; against the parent's bf16, whether the outputs are the same bits and this
build's bf16 median is not above the parent's by more than the spread of the parent's bf16.  fl_policy_head_pack_bf16
is timed on its own: the module calls it when a weight changed, not per step.

--rocprof adds the time of every kernel, bf16 and float32 side by side, from a separate `rocprofv3 --kernel-trace --stats` run of
this script (--kernels-only: the same inputs, the launches alone), so that a kernel that is not faster than its float32
counterpart shows.  The share of the bf16 matrix peak (2 516.8 TF = 16 x the 157.3 TF float32 matrix peak, MI355X_MICROARCH.md)
counts the FLOP of the 16 bf16 matrices and of the attention's two products over the sum of the kernel times.  The weight stream
is counted from the shapes: every 32-row tile re-reads the packed weights (3 342 336 bytes; 6 684 672 in float32) from L2.

Usage:  python tools/policy_head_bf16_bench.py [--parent-lib parent/libflatland_hip.so] [--rounds 3] [--launches 20] [--warmup 5]
                                               [--rocprof] [--out profiles/policy_head_bf16_bench.json]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 16 * 157.3e12
BF16_ROW_MACS = (2 * 256 * 256 + 256 * 128) + 3 * (256 * 768 + 256 * 256 + 512 * 256) + 2 * (512 * 256 + 256 * 128)
ATTN_MACS_PER_KEY = 3 * 4 * 2 * 64          # three blocks, four heads, q k^T and p v over 64
PACKED_BYTES = 2 * BF16_ROW_MACS
SHAPES = [("cfg2_1env", 1, 20), ("cfg2", 256, 20), ("cfg3", 1024, 80), ("cfg5", 256, 400)]
KERNELS_A_CALL = 8
ROWS = 32


def bf16_flop(B, A):
    return 2 * B * A * (BF16_ROW_MACS + ATTN_MACS_PER_KEY * A)


def median_events(fn, warmup, n):
    """median ms between two events around fn()"""
    import torch
    times = []
    for i in range(warmup + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def setup(B, A):
    import torch
    from tests.policy_head_stages import device_params
    from tests.policy_head_torch import seeded_params, synth_inputs
    x = [torch.from_numpy(v).cuda() for v in synth_inputs(B, A, 11)]
    return x, device_params(seeded_params(7, (2.5, 3.5)), x[0].device)


def outputs(B, A, dev):
    import torch
    return (torch.empty((B, A, 5), device=dev), torch.empty((B,), device=dev), torch.empty((B, A), dtype=torch.uint8, device=dev))


def f32_call(L, x, w):
    """a closure that enqueues fl_policy_head of library L (bound: hip_backend.bind) on the current stream with buffers allocated here"""
    import torch
    vp = C.c_void_p
    B, A = x[0].shape[:2]
    ws = torch.empty(max(L.fl_policy_head_workspace_bytes(B, A), 16), dtype=torch.uint8, device=x[0].device)
    out = outputs(B, A, x[0].device)
    ptrs = (vp * 38)(*[v.data_ptr() for v in w])
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(keep=(ws, out, ptrs)):
        rc = L.fl_policy_head(B, A, x[0].data_ptr(), x[1].data_ptr(), ptrs, x[2].data_ptr(), 1, 0.3745401188473625, out[0].data_ptr(),
                              out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, rc
    return call, out


def bf16_call(L, x, w):
    """the same for fl_policy_head_bf16 of library L, on the buffer that L's own fl_policy_head_pack_bf16 packs here"""
    import torch
    vp = C.c_void_p
    fn = L.fl_policy_head_bf16
    B, A = x[0].shape[:2]
    ws = torch.empty(max(L.fl_policy_head_bf16_workspace_bytes(B, A), 16), dtype=torch.uint8, device=x[0].device)
    out = outputs(B, A, x[0].device)
    ptrs = (vp * 38)(*[v.data_ptr() for v in w])
    s = vp(torch.cuda.current_stream().cuda_stream)
    packed = torch.empty(L.fl_policy_head_bf16_packed_bytes(), dtype=torch.uint8, device=x[0].device)
    rc = L.fl_policy_head_pack_bf16(ptrs, packed.data_ptr(), packed.numel(), s)
    assert rc == 0, rc

    def call(keep=(ws, out, ptrs, packed)):
        rc = fn(B, A, x[0].data_ptr(), x[1].data_ptr(), ptrs, packed.data_ptr(), packed.numel(), x[2].data_ptr(), 1, 0.3745401188473625,
                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, rc
    return call, out


def kernels_only(args):
    """(the rocprofv3 child) per shape: warmup + launches calls of fl_policy_head, then as many of fl_policy_head_bf16"""
    import torch
    from flatland_marl_amd import hip_backend as hb
    for label, B, A in SHAPES:
        x, w = setup(B, A)
        for call, _ in (f32_call(hb.lib(), x, w), bf16_call(hb.lib(), x, w)):
            for _ in range(args.warmup + args.launches):
                call()
            torch.cuda.synchronize()
        del x, w
        torch.cuda.empty_cache()


def rocprof_kernel_times(args):
    """per shape and path: us a call per kernel name -- a --kernels-only child under rocprofv3"""
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="policy_head_bf16_prof_")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "policy_head_bf16", "--",
               sys.executable, os.path.abspath(__file__), "--kernels-only", "--launches", str(args.launches), "--warmup", str(args.warmup)]
        subprocess.check_call(cmd, timeout=900)
        rows = []
        for t in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(t) as f:
                rows += [r for r in csv.DictReader(f) if "k_ph_" in r["Kernel_Name"] or "k_ph16_" in r["Kernel_Name"]]      # (not the pack)
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = (args.warmup + args.launches) * KERNELS_A_CALL
        assert len(rows) == 2 * per * len(SHAPES), (len(rows), per)
        out = {}
        for i, (label, B, A) in enumerate(SHAPES):
            for j, path in enumerate(("f32", "bf16")):
                seg = rows[(2 * i + j) * per + args.warmup * KERNELS_A_CALL:(2 * i + j + 1) * per]
                by = {}
                for r in seg:
                    name = r["Kernel_Name"].split("(")[0].replace("void ", "")
                    by[name] = by.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / args.launches
                out[(label, path)] = {k: round(v, 2) for k, v in sorted(by.items())}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libflatland_hip.so of the parent commit, for the A/B")
    ap.add_argument("--kernels-only", action="store_true", help="(the rocprofv3 child) the launches alone")
    ap.add_argument("--rocprof", action="store_true", help="kernel times from a rocprofv3 --kernel-trace --stats child run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # (the profiled child first, a fresh process started before this one has touched the GPU; it fails where there is none)
    ktimes = rocprof_kernel_times(args) if args.rocprof and not args.kernels_only else {}
    import torch
    if not torch.cuda.is_available():
        sys.exit("policy_head_bf16_bench: no GPU visible (the measurement has no CPU path)")
    if args.kernels_only:
        kernels_only(args)
        return
    from flatland_marl_amd import hip_backend as hb
    parent = hb.bind(C.CDLL(os.path.abspath(args.parent_lib))) if args.parent_lib else None
    parent_has_bf16 = parent is not None and hasattr(parent, "fl_policy_head_bf16")
    rows, pack_us = [], None
    for label, B, A in SHAPES:
        x, w = setup(B, A)
        if pack_us is None:
            packed = hb.policy_head_pack_bf16(w)
            pack_us = [round(median_events(lambda: hb.policy_head_pack_bf16(w, packed), args.warmup, args.launches) * 1e3, 2)
                       for _ in range(args.rounds)]
            del packed
        calls = []
        if parent is not None:
            calls.append(("parent_f32", f32_call(parent, x, w)))
        if parent_has_bf16:
            calls.append(("parent_bf16", bf16_call(parent, x, w)))
        calls += [("f32", f32_call(hb.lib(), x, w)), ("bf16", bf16_call(hb.lib(), x, w))]
        med = {k: [] for k, _ in calls}
        for _ in range(args.rounds):
            for k, (call, _) in calls:
                med[k].append(round(median_events(call, args.warmup, args.launches) * 1e3, 2))
        torch.cuda.synchronize()
        outs = {k: o for k, (_, o) in calls}
        mid = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
        tiles = (B * A + ROWS - 1) // ROWS
        r = dict(shape=label, envs=B, agents=A, rows=B * A, row_tiles=tiles, us_rounds=med, us_median=mid,
                 speedup_bf16_vs_f32=round(mid["f32"] / mid["bf16"], 3),
                 max_abs_dlogit_bf16_vs_f32=float((outs["bf16"][0] - outs["f32"][0]).abs().max()),
                 max_abs_logit=float(outs["f32"][0].abs().max()),
                 same_soft_action_share=float((outs["bf16"][2] == outs["f32"][2]).float().mean()),
                 bf16_flop=bf16_flop(B, A), weight_bytes_a_tile=dict(bf16=PACKED_BYTES, f32=2 * PACKED_BYTES),
                 weight_stream_tb_s=dict(bf16=round(tiles * PACKED_BYTES / (mid["bf16"] * 1e-6) / 1e12, 3),
                                         f32=round(tiles * 2 * PACKED_BYTES / (mid["f32"] * 1e-6) / 1e12, 3)))
        if parent is not None:
            assert all(torch.equal(a, b) for a, b in zip(outs["parent_f32"], outs["f32"])), "fl_policy_head differs from the parent's"
            lo, hi = min(med["parent_f32"]), max(med["parent_f32"])
            r.update(f32_bits_equal_parent=True, parent_spread_us=round(hi - lo, 2),
                     f32_median_inside_parent_range=bool(lo <= mid["f32"] <= hi),
                     speedup_bf16_vs_parent_f32=round(mid["parent_f32"] / mid["bf16"], 3),
                     bf16_faster_than_parent_by_more_than_its_spread=bool(mid["parent_f32"] - mid["bf16"] > hi - lo))
        if parent_has_bf16:
            lo, hi = min(med["parent_bf16"]), max(med["parent_bf16"])
            r.update(bf16_bits_equal_parent=all(bool(torch.equal(a, b)) for a, b in zip(outs["parent_bf16"], outs["bf16"])),
                     parent_bf16_spread_us=round(hi - lo, 2),
                     bf16_not_slower_than_parent_bf16_by_more_than_its_spread=bool(mid["bf16"] - mid["parent_bf16"] <= hi - lo))
        if ktimes:
            kf, kb = ktimes[(label, "f32")], ktimes[(label, "bf16")]
            total = sum(kb.values())
            r.update(kernel_us_f32=kf, kernel_us_bf16=kb, kernels_us=dict(f32=round(sum(kf.values()), 2), bf16=round(total, 2)),
                     bf16_tflops=round(bf16_flop(B, A) / (total * 1e-6) / 1e12, 2),
                     share_of_bf16_matrix_peak=round(bf16_flop(B, A) / (total * 1e-6) / PEAK_BF16, 5))
        rows.append(r)
        print(json.dumps(r), flush=True)
        del calls, outs, x, w
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/policy_head_bf16_bench.py", device=torch.cuda.get_device_name(0),
                           compute_units=torch.cuda.get_device_properties(0).multi_processor_count,
                           peak_bf16_matrix_tflops=PEAK_BF16 / 1e12, launches=args.launches, warmup=args.warmup, rounds=args.rounds,
                           parent_lib=bool(parent), pack_us_rounds=pack_us, packed_bytes=PACKED_BYTES, results=rows), f, indent=1)


if __name__ == "__main__":
    main()
