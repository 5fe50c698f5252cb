#!/usr/bin/env python3
"""Launch time of fl_action_space (the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py) at cfg2 (256 envs x 20
agents), cfg3 (1 024 x 80) and cfg5 (256 x 400):
  all       every output at once -- lists, flags and the translation -- with float64 and with int32 distances
  translate the translation alone (BatchedRailEnv.reduced_actions)
  step / step_shortest_path   the tick alone and translation + tick on the same batch in the same state (the state is restored before
            every round): their difference is what the reduced action space adds to a step

Times: after `--warmup` launches, the median of `--rounds` device-event timings of `--launches` back-to-back launches each, the
stream drained before and after every round.  Registers / LDS / scratch from the compiler's -Rpass-analysis=kernel-resource-usage
remarks (--resources: compiles fl_host.hip once, needs no GPU).

Usage:  python tools/action_space_bench.py [--only cfg2 ...] [--launches 50] [--rounds 9] [--warmup 10] [--out FILE.json]
        python tools/action_space_bench.py --resources [--out FILE.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("cfg2", "cfg3", "cfg5")
DEFAULT_OUT = os.path.join(ROOT, "profiles", "action_space_bench.json")
KERNELS = ("k_action_space", "k_decision_cells")


def load(path):
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return dict(tool="tools/action_space_bench.py", results={}, resources={})


def save(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def timed(fn, launches, rounds, warmup, before=None):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3 / launches)
    return dict(us_median=round(float(np.median(ts)), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2), launches_per_round=launches,
                rounds=rounds)


def run(shape, launches, rounds, warmup, steps=24):
    import numpy as np
    import torch
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd import workload as wl
    envs, seed = wl.make_envs(shape)
    env = hb.BatchedRailEnv(envs)
    for _ in range(steps):              # trains on the map, not all on their start cells
        env.step_synth(seed, 0, 2, auto_reset=True)
    B, A, dev = env.B, env.A, env.device
    L = hb.lib()
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)      # noqa: E731
    act, cnt, dec, out = u8(B, A, 3), u8(B, A), u8(B, A), u8(B, A)
    reduced = torch.as_tensor(np.random.RandomState(0).randint(0, 3, (B, A)).astype(np.uint8)).to(dev)
    rows = dict(workload=shape, B=B, A=A)
    for kind, dt in ((0, torch.float64), (1, torch.int32)):
        dist = torch.empty((B, A, 3), dtype=dt, device=dev)

        def every_output():
            rc = L.fl_action_space(env.h, 0, B, kind, act.data_ptr(), dist.data_ptr(), cnt.data_ptr(), dec.data_ptr(), reduced.data_ptr(),
                                   out.data_ptr())
            assert rc == 0, L.fl_last_error()

        rows["all_" + str(dt).split(".")[-1]] = timed(every_output, launches, rounds, warmup)
    rows["translate"] = timed(lambda: env.reduced_actions(reduced), launches, rounds, warmup)
    rows["decision_cells"] = timed(lambda: env.decision_cells(), launches, rounds, warmup)
    # the tick with and without the translation in front of it: the same actions, from the same state
    plain = env.reduced_actions(reduced).clone()
    st, el = env.state()
    aux = env.state_aux()
    restore = lambda: env.set_state(st, aux, el)      # noqa: E731
    n = min(launches, 20)      # (a short run from the restored state: the agents stay spread over the map)
    rows["step"] = timed(lambda: env.step(plain), n, rounds, 2, before=restore)
    rows["step_shortest_path"] = timed(lambda: env.step_shortest_path(reduced), n, rounds, 2, before=restore)
    rows["added_us_per_step"] = round(rows["step_shortest_path"]["us_median"] - rows["step"]["us_median"], 2)
    env.check()
    for k, v in rows.items():
        if isinstance(v, dict):
            print("%s %-20s %8.2f us (min %.2f max %.2f)" % (shape, k, v["us_median"], v["us_min"], v["us_max"]), flush=True)
    print("%s added per step: %.2f us" % (shape, rows["added_us_per_step"]), flush=True)
    env.close()
    del env
    torch.cuda.empty_cache()
    return rows


def resources():
    """registers / LDS / scratch of the kernels of fl_wrappers.h: fl_host.hip compiled with the build's own flags"""
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
            if any(k in name for k in KERNELS):
                out[name] = {}
            continue
        kv = re.match(r"([A-Za-z ]+(?:\[.*?\])?): (\d+)", text)
        if kv and name in out:
            out[name][kv.group(1).strip()] = int(kv.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    doc = load(args.out) if os.path.exists(args.out) else load(DEFAULT_OUT)
    if args.resources:
        doc["resources"] = resources()
        print(json.dumps(doc["resources"], indent=1))
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("action_space_bench: no GPU visible (the measurement has no CPU path)")
        doc["device"] = torch.cuda.get_device_name(0)
        for shape in (args.only or SHAPES):
            doc["results"][shape] = run(shape, args.launches, args.rounds, args.warmup)
    save(args.out, doc)


if __name__ == "__main__":
    main()
