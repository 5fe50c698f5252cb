#!/usr/bin/env python3
"""The launch plans of the observation launcher, asked of the library's CPU hook fl_debug_obs_plan (no GPU needed): which kernel, launch class
and split every fl_obs_* call would run for a batch, as the record fl_debug_last_obs_launch reports after the launch.

    tools/obs_plan_sweep.py [--lib LIB]                  the differential sweep: query count and a digest of every output word -- run it
                                                         against two builds (and under each diagnostic switch: the launcher reads its
                                                         switches once per process) and compare the lines
    tools/obs_plan_sweep.py [--lib LIB] --table PATH     write the reduced set that tests/test_obs_plan.py replays (tests/obs_plan_table.json)

A change to the class table of csrc/fl_obs_layout.h or to the selection code of csrc/fl_obs.hip that is meant to keep every choice leaves
both outputs as they were; one that is meant to change choices re-captures the table and says which rows moved."""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 25                        # FL_OBS_LAUNCH_WORDS (csrc/fl_obs.h)
KINDS = {"cutils": 0, "both": 1, "tree": 2}
FIELDS = ("kind", "A", "U", "tall", "max_branch", "max_nodes", "pred_depth", "max_depth", "tree_pred", "keep_mode", "label", "n_cu", "levels")


class Hook:
    def __init__(self, lib):
        self.fn = ctypes.CDLL(lib).fl_debug_obs_plan
        self.rec = (ctypes.c_int * WORDS)()
        self.n_fit = ctypes.c_int()
        self.arrays = {}

    def __call__(self, kind, A, U, tall, max_branch, max_nodes, pred_depth, max_depth, tree_pred, keep_mode, label, n_cu, levels):
        """levels: ((rail cells, envs), ...) -- the batch's envs in this order.  Returns [rc, envs on the class's body, the record's words]."""
        R = self.arrays.get(levels)
        if R is None:
            cells = [r for r, n in levels for _ in range(n)]
            R = self.arrays[levels] = (ctypes.c_int * len(cells))(*cells)
        rc = self.fn(KINDS[kind], A, U, tall, max_branch, max_nodes, pred_depth, max_depth, tree_pred, keep_mode, label, n_cu, R, len(R), self.rec, ctypes.byref(self.n_fit))
        return [rc, self.n_fit.value] + list(self.rec)


def two_levels(lo, hi, n_lo, B):
    return tuple((r, n) for r, n in ((lo, n_lo), (hi, B - n_lo)) if n)


def shares(B):
    """envs on the lower level: none, just under half, exactly half (exact_split_covers_most turns at 2 * n >= B), all"""
    return (0, (B - 1) // 2, (B + 1) // 2, B)


# agents / rail cells / unique targets at the capacities of the launch classes (csrc/fl_obs_layout.h)
CAPS = ((32, 256, 8), (80, 232, 10), (80, 680, 24), (100, 1344, 30), (432, 2816, 53), (432, 3200, 53))
N_CU = 256
CALLS = (("cutils", 0), ("both", 2), ("both", 3))    # (kind, depth of the upstream tree)


def q(kind, A, U, levels, depth=0, tall=0, max_branch=2, max_nodes=31, pred=500, tree_pred=30, keep=0, label=0):
    return (kind, A, U, tall, max_branch, max_nodes, pred, depth, tree_pred, keep, label, N_CU, levels)


def reduced_queries():
    out = []
    # both sides of every class's agent and rail-cell capacity, one env per CU and several (obs_batch_is_wide: 512 envs on 256 CUs)
    for (A, R, U), (kind, depth), B in itertools.product(CAPS, CALLS, (4, 512)):
        for a, r in ((A, R), (A - 1, R), (A + 1, R), (A, R + 1)):
            out.append(q(kind, a, U, ((r, B),), depth))
    for (kind, depth), B in itertools.product(CALLS, (4, 512)):    # maps taller than wide: classes 16 / 20
        for a, r in ((100, 1280), (101, 1280), (100, 1281)):
            out.append(q(kind, a, 30, ((r, B),), depth, tall=1))
    # split launches: two levels on either side of a class's rail cells, at every share of the lower level; keep-rows on and off
    for (A, U, lo, hi), (kind, depth), keep in itertools.product(((80, 10, 232, 233), (80, 10, 232, 681), (80, 24, 680, 681), (200, 53, 2816, 2817),
                                                                  (432, 53, 2816, 3200), (432, 53, 2816, 3201), (432, 53, 3200, 3201)), CALLS, (0, 1)):
        for n_lo in shares(8):
            out.append(q(kind, A, U, two_levels(lo, hi, n_lo, 8), depth, keep=keep))
    # FL_OBS_KEEP_TREE_ROWS against classes 1, 5 and 11 (and their neighbours), narrow and wide
    for B, depth, (A, R) in itertools.product((4, 512), (2, 3), ((32, 256), (20, 213), (33, 200))):
        out.append(q("both", A, 8, ((R, B),), depth, keep=1))
    # a handle subset, larger trees, the upstream builder alone
    for (A, R, U), label, nodes in itertools.product(CAPS, (0, 1), (31, 32, 45)):
        out.append(q("cutils", A, U, ((R, 4),), label=label, max_nodes=nodes))
    for A, R, U in CAPS[:3]:
        for nodes in (32, 45):
            out.append(q("both", A, U, ((R, 4),), 2, max_nodes=nodes))
        for depth, mb, label in ((2, 2, 0), (3, 2, 1), (4, 2, 0), (3, 3, 0), (4, 3, 0)):
            out.append(q("tree", A, U, ((R, 4),), depth, max_branch=mb, label=label))
    return out


def sweep_queries():
    As = (1, 7, 16, 17, 20, 31, 32, 33, 50, 79, 80, 81, 100, 101, 200, 400, 425, 432, 433)
    pairs = ((64, 64), (231, 232), (232, 233), (232, 680), (256, 257), (680, 681), (680, 1344), (1280, 1281), (2745, 2816), (2816, 2817), (2816, 3200), (3200, 3201))
    batches = [two_levels(lo, hi, n, B) for lo, hi in pairs for B in (8, 256, 257, 512, 513) for n in (shares(B) if B == 8 else shares(B)[1:3])]
    calls = (("cutils", 0), ("both", 1), ("both", 2), ("both", 3), ("tree", 2), ("tree", 4))
    for A, levels, (kind, depth), keep, label, nodes, tall, mb, (pred, tp) in itertools.product(
            As, batches, calls, (0, 1), (0, 1), (31, 32, 45), (0, 1), (2, 3), ((500, 30), (500, 60), (63, 30))):
        for U in ((8, 60) if A <= 33 else (24,)):
            if U <= A:
                yield q(kind, A, U, levels, depth, tall, mb, nodes, pred, tp, keep, label)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "flatland_marl_amd", "csrc", "libflatland_hip.so"))
    ap.add_argument("--table")
    args = ap.parse_args()
    hook = Hook(args.lib)
    if args.table:
        rows = [dict(zip(FIELDS, query), out=hook(*query)) for query in reduced_queries()]
        with open(args.table, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
        print(len(rows), "rows ->", args.table)
        sys.exit(0)
    n, fails, h, seen, t0 = 0, 0, hashlib.sha256(), {}, time.time()
    for query in sweep_queries():
        out = hook(*query)
        n += 1
        fails += out[0] != 0
        seen[(out[4], out[5])] = seen.get((out[4], out[5]), 0) + 1     # (launch class, split kind)
        h.update(bytes(str(out), "ascii"))
    print(n, "queries,", fails, "without a plan, %.1f s," % (time.time() - t0), "digest", h.hexdigest()[:16])
    print("(class, split): queries", sorted(seen.items()))
