#!/usr/bin/env python3
"""Time of the policy's TreeLSTM forward on fl_tree_lstm (flatland_marl_amd.policy.TreeLSTM) against the masked-loop
restatement (tests/tree_lstm_torch.py, float32, same device and inputs), on real trees: obs_policy() of the workload batches after
a few synthetic steps.  Shapes: one cfg2 env (20 trees), one cfg5 env (400), cfg2 (5 120), cfg3 (81 920), cfg2 at max_nodes = 64
(5 120); modes: all (every node's h, forward) and roots (node 0 of every tree, roots()).

FLOP come from the inputs' own level histogram (leaf 9 216 FLOP: W_iou 12 -> 384; internal node 503 808: W_iou, U_iou 384 -> 384,
W_f once, U_f 128 -> 128 three times, W_c 384 -> 128; elementwise work not counted).  Module wall time is from the call to a
device sync.  Kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (--kernels-only: the same
inputs, the launches alone), which --rocprof starts as a child and reads back; TFLOP/s and the share of the 157.3 TF FP32 matrix
peak (MI355X_MICROARCH.md) are from the kernel time.

Usage:  python tools/tree_lstm_bench.py [--launches 20] [--warmup 5] [--rocprof] [--out profiles/tree_lstm_bench.json]
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
LEAF_FLOP = 2 * 12 * 384
NODE_FLOP = 2 * (12 * 384 + 384 * 384 + 12 * 128 + 3 * 128 * 128 + 384 * 128)
# (label, workload, envs, max_nodes)
SHAPES = [("cfg2_1env", "cfg2", 1, 31), ("cfg5_1env", "cfg5", 1, 31), ("cfg2", "cfg2", 256, 31), ("cfg3", "cfg3", 1024, 31),
          ("cfg2_n64", "cfg2", 256, 64)]
MODES = ("all", "roots")


def tree_flop(node_order):
    """FLOP of one forward from the level histogram of the inputs"""
    leaves = int((node_order == 0).sum())
    internal = int((node_order > 0).sum())
    return leaves * LEAF_FLOP + internal * NODE_FLOP, leaves, internal


def inputs(workload, B, max_nodes, steps=8):
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs(workload, B=B)
    env = BatchedRailEnv(envs, max_nodes=max_nodes)
    for _ in range(steps):
        env.step_synth(seed, 0, 2, auto_reset=True)
    out = [x.clone() for x in env.obs_policy()[1:]]
    env.close()
    return out


def module():
    import torch
    from flatland_marl_amd.policy import TreeLSTM
    from tests.tree_lstm_torch import seeded_params
    m = TreeLSTM().cuda()
    m.load_state_dict(seeded_params(7))
    return m


def launches(m, x, mode, n):
    f = m.roots if mode == "roots" else m.forward
    for _ in range(n):
        f(*x)


def kernels_only(args):
    import torch
    m = module()
    with torch.no_grad():
        for label, wl_name, B, N in SHAPES:
            x = inputs(wl_name, B, N)
            for mode in MODES:
                launches(m, x, mode, args.warmup + args.launches)
                torch.cuda.synchronize()
            del x
            torch.cuda.empty_cache()


def rocprof_kernel_times(args):
    """us a launch per (shape, mode): the k_tree_lstm dispatches of a --kernels-only child under rocprofv3, in launch order"""
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="tree_lstm_prof_")
    try:
        cmd = [rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tree_lstm", "--",
               sys.executable, os.path.abspath(__file__), "--kernels-only", "--launches", str(args.launches), "--warmup", str(args.warmup)]
        subprocess.check_call(cmd, timeout=900)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rows = []
        for t in traces:
            with open(t) as f:
                rows += [r for r in csv.DictReader(f) if "k_tree_lstm" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = args.warmup + args.launches
        assert len(rows) == per * len(SHAPES) * len(MODES), (len(rows), per)
        out, i = {}, 0
        for label, *_ in SHAPES:
            for mode in MODES:
                seg = rows[i + args.warmup:i + per]
                out[(label, mode)] = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / len(seg) / 1e3
                i += per
        stat_rows = []
        for s in stats:
            with open(s) as f:
                stat_rows += [r for r in csv.DictReader(f) if "k_tree_lstm" in r.get("Name", "")]
        return out, stat_rows
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="(the rocprofv3 child) the launches alone")
    ap.add_argument("--rocprof", action="store_true", help="kernel times from a rocprofv3 --kernel-trace --stats child run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_lstm_bench: no GPU visible (the measurement has no CPU path)")
    if args.kernels_only:
        kernels_only(args)
        return
    from tests.tree_lstm_torch import tree_lstm as restated
    ktimes, kstats = rocprof_kernel_times(args) if args.rocprof else ({}, [])
    m = module()
    params = dict(m.named_parameters())
    rows = []
    with torch.no_grad():
        for label, wl_name, B, N in SHAPES:
            x = inputs(wl_name, B, N)
            flop, leaves, internal = tree_flop(x[2])
            T = x[2].shape[0] * x[2].shape[1]
            restated(*x, params, dtype=torch.float32)          # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.baseline_reps):
                restated(*x, params, dtype=torch.float32)
                torch.cuda.synchronize()
            base_ms = (time.perf_counter() - t) * 1e3 / args.baseline_reps
            for mode in MODES:
                launches(m, x, mode, args.warmup)
                torch.cuda.synchronize()
                walls = []
                for _ in range(args.launches):
                    t = time.perf_counter()
                    launches(m, x, mode, 1)
                    torch.cuda.synchronize()
                    walls.append((time.perf_counter() - t) * 1e3)
                walls.sort()
                wall = walls[len(walls) // 2]
                r = dict(shape=label, workload=wl_name, envs=B, trees=T, nodes=N, mode=mode, leaves=leaves, internal_nodes=internal,
                         levels=int(x[2].max()) + 1, flop=flop, module_wall_ms_median=round(wall, 4),
                         restatement_f32_wall_ms=round(base_ms, 3), speedup_vs_restatement=round(base_ms / wall, 1))
                k = ktimes.get((label, mode))
                if k is not None:
                    r.update(kernel_us=round(k, 2), tflops=round(flop / (k * 1e-6) / 1e12, 2),
                             share_of_fp32_matrix_peak=round(flop / (k * 1e-6) / PEAK, 4))
                rows.append(r)
                print(json.dumps(r), flush=True)
            del x
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/tree_lstm_bench.py", device=torch.cuda.get_device_name(0), peak_fp32_matrix_tflops=PEAK / 1e12,
                           launches=args.launches, warmup=args.warmup, results=rows, rocprof_kernel_stats=kstats), f, indent=1)


if __name__ == "__main__":
    main()
