#!/usr/bin/env python3
"""Launch time and effective write rate of fl_predict (ShortestPathPredictorForRailEnv.get(), flatland/envs/predictions.py:97-180) at
cfg2 (256 envs x 20 agents) and cfg3 (1 024 x 80) at depth 30, cfg5 (256 x 400) at depth 30 and, in env chunks, at depth 500; float64
and int32.

bytes = nb * A * (max_depth + 1) * 5 * elem_bytes (the rows; the reads -- 36 B an agent and the walk's table gathers -- are left
out).  Times: after `--warmup` launches, the median of `--rounds` device-event timings of `--launches` back-to-back launches each,
the stream drained before and after every round.  Kernel times come from separate `rocprofv3 --kernel-trace --stats` runs of this
script (the program after `--`), one per shape and depth, merged in with --kernel-stats; registers / LDS / scratch from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (--resources: compiles fl_host.hip once, needs no GPU).

Usage:  python tools/predictions_bench.py [--only cfg2_d30 ...] [--dtypes float64 int32] [--launches 50] [--rounds 9] [--warmup 10] [--out FILE.json]
        python tools/predictions_bench.py --resources [--out FILE.json]
        python tools/predictions_bench.py --kernel-stats DIR [--out FILE.json]     DIR/<label>/**/*kernel_stats.csv of the rocprofv3 runs
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# label -> (workload, max_depth, envs a call)
SHAPES = {"cfg2_d30": ("cfg2", 30, None), "cfg3_d30": ("cfg3", 30, None), "cfg5_d30": ("cfg5", 30, None), "cfg5_d500": ("cfg5", 500, 64)}
DEFAULT_OUT = os.path.join(ROOT, "profiles", "predictions_bench.json")
OBS_GLOBAL_TBPS = 5.9          # what fl_obs_global reaches on the same machine (profiles/global_obs_bench.json)
FUSED_OBS_CFG2_US = 37.0       # the whole fused observation launch at cfg2


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return dict(tool="tools/predictions_bench.py", results={}, kernel_stats={}, resources={})


def save(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def run(label, dtypes, launches, rounds, warmup, steps=24):
    import numpy as np
    import torch
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    shape, depth, chunk = SHAPES[label]
    envs, seed = wl.make_envs(shape)
    env = BatchedRailEnv(envs)
    for _ in range(steps):              # trains on the map: paths of every length, not all from the start cells
        env.step_synth(seed, 0, 2, auto_reset=True)
    nb = chunk or env.B
    ranges = [(b, b + nb) for b in range(0, env.B, nb)]
    rows = {}
    for dt in dtypes:
        dtype = getattr(torch, dt)
        for _ in range(warmup):
            for r in ranges:
                env.predictions(depth, dtype, envs=r)
        ts = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                for r in ranges:
                    env.predictions(depth, dtype, envs=r)
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1) * 1e3 / (launches * len(ranges)))
        env.check()
        us = float(np.median(ts))
        eb = 8 if dt == "float64" else 4
        nbytes = nb * env.A * (depth + 1) * 5 * eb
        rate = nbytes / (us * 1e-6)
        rows[dt] = dict(workload=shape, max_depth=depth, dtype=dt, B=env.B, A=env.A, envs_per_launch=nb, launches_per_round=launches * len(ranges),
                        rounds=rounds, us_per_launch_median=round(us, 2), us_per_launch_min=round(min(ts), 2), us_per_launch_max=round(max(ts), 2),
                        bytes_written_per_launch=int(nbytes), write_TBps=round(rate / 1e12, 3),
                        share_of_fl_obs_global_rate=round(rate / 1e12 / OBS_GLOBAL_TBPS, 3))
        if label == "cfg2_d30":
            rows[dt]["share_of_fused_obs_launch_cfg2"] = round(us / FUSED_OBS_CFG2_US, 3)
        print("%s %s: %9.1f us/launch (min %.1f max %.1f)  %8.1f MB  %.3f TB/s" % (
            label, dt, us, min(ts), max(ts), nbytes / 1e6, rate / 1e12), flush=True)
    env.close()
    del env
    torch.cuda.empty_cache()
    return rows


def resources():
    """registers / LDS / scratch of the two k_predict instantiations: fl_host.hip compiled with the build's own flags"""
    build = os.path.join(ROOT, "flatland_marl_amd", "csrc", "build.sh")
    flags = subprocess.check_output([build, "--compile-args", "fl_host"], text=True).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull], capture_output=True, text=True, check=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*(.*)$", line)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: (\S+)", text)
        if f:
            name = f.group(1)
            if "k_predict" in name:
                out[name] = {}
            continue
        kv = re.match(r"([A-Za-z ]+(?:\[.*?\])?): (\d+)", text)
        if kv and name in out:
            out[name][kv.group(1).strip()] = int(kv.group(2))
    return out


def kernel_stats(directory):
    out = {}
    for label in SHAPES:
        for path in glob.glob(os.path.join(directory, label, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "k_predict" in row.get("Name", ""):
                        kind = "float64" if "double" in row["Name"] or "IdE" in row["Name"] else "int32"
                        out.setdefault(label, {})[kind] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2),
                                                               min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--dtypes", nargs="*", default=["float64", "int32"])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    ap.add_argument("--no-write", action="store_true", help="print only (the rocprofv3 runs)")
    args = ap.parse_args()
    doc = load(args.out) if os.path.exists(args.out) else load(DEFAULT_OUT)
    if args.resources:
        doc["resources"] = resources()
        print(json.dumps(doc["resources"], indent=1))
    elif args.kernel_stats:
        doc["kernel_stats"] = kernel_stats(args.kernel_stats)
        print(json.dumps(doc["kernel_stats"], indent=1))
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("predictions_bench: no GPU visible (the measurement has no CPU path)")
        doc["device"] = torch.cuda.get_device_name(0)
        doc["reference_points"] = dict(fl_obs_global_TBps=OBS_GLOBAL_TBPS, fused_obs_launch_cfg2_us=FUSED_OBS_CFG2_US)
        for label in (args.only or SHAPES):
            lo, ro = (3, 3) if label == "cfg5_d500" and args.launches > 3 else (args.launches, args.rounds)
            doc["results"].setdefault(label, {}).update(run(label, args.dtypes, lo, ro, min(args.warmup, 2) if label == "cfg5_d500" else args.warmup))
    if not args.no_write:
        save(args.out, doc)


if __name__ == "__main__":
    main()
