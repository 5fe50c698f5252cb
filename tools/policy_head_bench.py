#!/usr/bin/env python3
"""Time of the policy network after its tree encoder on fl_policy_head (flatland_marl_amd.policy.Network.head, logits + value +
soft actions) against the same parameters through torch's eager ops (Network.head_torch: nn.Linear / nn.MultiheadAttention /
nn.GELU, float32, same device and inputs; without the action choice, which the reference does in numpy on the host).  Inputs are
synthetic (tests/policy_head_torch.synth_inputs) at the shapes of cfg2 (256 envs x 20 agents), cfg3 (1 024 x 80) and cfg5
(256 x 400).

FLOP a forward: 2 * (1 693 184 multiply-adds an agent in the linear layers + 1 536 * A in the attention scores and sums) --
elementwise work not counted.  Module wall time is from the call to a device sync, the median of --launches calls.  Kernel time comes
from a separate `rocprofv3 --kernel-trace --stats` run of this script (--kernels-only: the same inputs, the launches alone), which
--rocprof starts as a child and reads back: the sum over the k_ph_* dispatches of a call, and that sum per kernel; TFLOP/s and the
share of the 157.3 TF FP32 matrix peak (MI355X_MICROARCH.md) are from the kernel time.

Usage:  python tools/policy_head_bench.py [--launches 20] [--warmup 5] [--rocprof] [--out profiles/policy_head_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.3e12
ROW_MACS = (83 * 256 + 2 * 256 * 256 + 256 * 128) + 3 * (256 * 768 + 256 * 256 + 512 * 256) + 2 * (512 * 256 + 256 * 128) + 128 * 6
ATTN_MACS_PER_KEY = 3 * 4 * 2 * 64          # three blocks, four heads, q k^T and p v over 64
SHAPES = [("cfg2", 256, 20), ("cfg3", 1024, 80), ("cfg5", 256, 400)]
KERNELS_A_CALL = 8


def flop(B, A):
    return 2 * B * A * (ROW_MACS + ATTN_MACS_PER_KEY * A)


def inputs(B, A):
    import torch
    from tests.policy_head_torch import synth_inputs
    return [torch.from_numpy(x).cuda() for x in synth_inputs(B, A, 11)]


def module():
    from flatland_marl_amd.policy import Network
    from tests.policy_head_torch import seeded_params
    m = Network().cuda()
    m.load_state_dict(seeded_params(7, (2.5, 3.5)))
    return m


def launches(m, x, n):
    for _ in range(n):
        m.head(x[0], x[1], x[2], "soft")


def kernels_only(args):
    import torch
    m = module()
    with torch.no_grad():
        for label, B, A in SHAPES:
            x = inputs(B, A)
            launches(m, x, args.warmup + args.launches)
            torch.cuda.synchronize()
            del x
            torch.cuda.empty_cache()


def rocprof_kernel_times(args):
    """per shape: us a call over all k_ph_* dispatches, and per kernel name -- a --kernels-only child under rocprofv3"""
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="policy_head_prof_")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "policy_head", "--",
               sys.executable, os.path.abspath(__file__), "--kernels-only", "--launches", str(args.launches), "--warmup", str(args.warmup)]
        subprocess.check_call(cmd, timeout=900)
        rows = []
        for t in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(t) as f:
                rows += [r for r in csv.DictReader(f) if "k_ph_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = (args.warmup + args.launches) * KERNELS_A_CALL
        assert len(rows) == per * len(SHAPES), (len(rows), per)
        out = {}
        for i, (label, B, A) in enumerate(SHAPES):
            seg = rows[i * per + args.warmup * KERNELS_A_CALL:(i + 1) * per]
            by = {}
            for r in seg:
                name = r["Kernel_Name"].split("(")[0].replace("void ", "")
                by[name] = by.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / args.launches
            out[label] = (sum(by.values()), {k: round(v, 2) for k, v in sorted(by.items())})
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def median_wall(fn, warmup, n):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    walls = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
    walls.sort()
    return walls[len(walls) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="(the rocprofv3 child) the launches alone")
    ap.add_argument("--rocprof", action="store_true", help="kernel times from a rocprofv3 --kernel-trace --stats child run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("policy_head_bench: no GPU visible (the measurement has no CPU path)")
    if args.kernels_only:
        kernels_only(args)
        return
    ktimes = rocprof_kernel_times(args) if args.rocprof else {}
    m = module()
    rows = []
    with torch.no_grad():
        for label, B, A in SHAPES:
            x = inputs(B, A)
            hip = median_wall(lambda: m.head(x[0], x[1], x[2], "soft"), args.warmup, args.launches)
            eager = median_wall(lambda: m.head_torch(x[0], x[1]), args.warmup, args.launches)
            r = dict(shape=label, envs=B, agents=A, rows=B * A, flop=flop(B, A), head_wall_ms_median=round(hip, 4),
                     head_torch_wall_ms_median=round(eager, 4), speedup_vs_head_torch=round(eager / hip, 2))
            if label in ktimes:
                k, by = ktimes[label]
                r.update(kernels_us=round(k, 2), kernel_us_by_name=by, tflops=round(flop(B, A) / (k * 1e-6) / 1e12, 2),
                         share_of_fp32_matrix_peak=round(flop(B, A) / (k * 1e-6) / PEAK, 4))
            rows.append(r)
            print(json.dumps(r), flush=True)
            del x
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/policy_head_bench.py", device=torch.cuda.get_device_name(0), peak_fp32_matrix_tflops=PEAK / 1e12,
                           launches=args.launches, warmup=args.warmup, results=rows), f, indent=1)


if __name__ == "__main__":
    main()
