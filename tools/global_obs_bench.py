#!/usr/bin/env python3
"""Launch time and effective write bandwidth of fl_obs_global (GlobalObsForRailEnv, flatland/envs/observations.py:535-611) at the
cfg2 (256 envs x 30x30 / 20 agents) and cfg3 (1 024 envs x 35x30 / 80 agents) shapes, float32 and float64, whole batch in one call.

The kernel is a pure streaming write: bytes = nb * (H*W*16 + A*H*W*(5 + 2)) * elem_bytes (rail + agents_state + targets; the
reads -- the agents' 28 B and the band's grid cells -- are left out).  Times are device events around `--launches` back-to-back
launches after `--warmup` ones; the shares are of the plain-store rate measured on this GPU (6.0-6.2 TB/s, MI355X_MICROARCH.md
"Global float atomics", plain stores row) and of the 8 TB/s HBM spec.  Take kernel times from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

Usage:  python tools/global_obs_bench.py [--launches 200] [--warmup 20] [--shapes cfg2 cfg3] [--dtypes float32 float64] [--out FILE.json]
        [--lib ab_libs/libfl_NAME.so]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORE_RATE = (6.0e12, 6.2e12)
HBM_SPEC = 8.0e12


def run(shape, dtype, launches, warmup, steps=24):
    import torch
    from flatland_marl_amd import workload as wl
    from flatland_marl_amd.hip_backend import BatchedRailEnv
    envs, seed = wl.make_envs(shape)
    env = BatchedRailEnv(envs)
    for _ in range(steps):              # trains on the map: the patches and the ch1..ch4 cells are not all at their defaults
        env.step_synth(seed, 0, 2, auto_reset=True)
    for _ in range(warmup):
        env.obs_global(dtype)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        env.obs_global(dtype)
    t1.record()
    torch.cuda.synchronize()
    env.check()
    us = t0.elapsed_time(t1) * 1e3 / launches
    eb = 8 if dtype == torch.float64 else 4
    HW = env.H * env.W
    nbytes = env.B * (HW * 16 + env.A * HW * 7) * eb
    rate = nbytes / (us * 1e-6)
    env.close()
    del env
    torch.cuda.empty_cache()
    return dict(shape=shape, dtype=str(dtype).replace("torch.", ""), B=len(envs), A=int(len(envs[0]["init_dir"])),
                H=int(envs[0]["grid"].shape[0]), W=int(envs[0]["grid"].shape[1]), launches=launches, us_per_launch=round(us, 2),
                bytes_written=int(nbytes), effective_TBps=round(rate / 1e12, 3),
                share_of_store_rate=[round(rate / STORE_RATE[1], 3), round(rate / STORE_RATE[0], 3)],
                share_of_8TBps_spec=round(rate / HBM_SPEC, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", nargs="*", default=["cfg2", "cfg3"])
    ap.add_argument("--dtypes", nargs="*", default=["float32", "float64"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="diagnostic: load this build of the C-ABI library instead of the in-tree one (A/B runs)")
    args = ap.parse_args()
    if args.lib:
        from flatland_marl_amd import hip_backend
        hip_backend.LIB_PATH = os.path.abspath(args.lib)
    import torch
    if not torch.cuda.is_available():
        sys.exit("global_obs_bench: no GPU visible (the measurement has no CPU path)")
    rows = []
    for shape in args.shapes:
        for dt in args.dtypes:
            r = run(shape, getattr(torch, dt), args.launches, args.warmup)
            rows.append(r)
            print("%s %s: %8.1f us/launch  %7.1f MB  %.2f TB/s  (%.0f-%.0f %% of 6.0-6.2 TB/s plain stores, %.0f %% of 8 TB/s)" % (
                shape, r["dtype"], r["us_per_launch"], r["bytes_written"] / 1e6, r["effective_TBps"],
                100 * r["share_of_store_rate"][0], 100 * r["share_of_store_rate"][1], 100 * r["share_of_8TBps_spec"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/global_obs_bench.py", device=torch.cuda.get_device_name(0), lib=args.lib, results=rows), f, indent=1)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
