#!/usr/bin/env python3
"""fl_tree_lstm_bf16 against fl_tree_lstm, on real trees (obs_policy() of the workload batches after a few synthetic steps, as
tools/tree_lstm_bench.py takes them): one env of cfg2 (20 trees), cfg2 (5 120) and cfg3 (81 920), every node's h ("all") and the
roots alone ("roots", what Network.act launches).

Times are HIP-event medians around one launch through the C entry points, buffers allocated beforehand.  With --parent-lib the
launches alternate in --rounds interleaved rounds between fl_tree_lstm of that library (the parent commit's build), fl_tree_lstm
of this build and fl_tree_lstm_bf16 of this build -- and, where the parent exports it, the parent's own fl_tree_lstm_bf16; a
round's figure is the median of --launches launches.  Per shape and mode the file holds every round's medians, the spread (max -
min) of the parent's, and whether this build's float32 median lies inside the parent's range and the bf16 median is below the
parent's by more than that spread; against the parent's bf16, whether the outputs are the same bits and this build's bf16 median is
not above the parent's by more than the spread of the parent's bf16.

The achieved share of the bf16 matrix peak (2 516.8 TF = 16 x the 157.3 TF float32 matrix peak, MI355X_MICROARCH.md) counts the
FLOP of the three recurrent products alone (491 520 a node above height 0).  The weight stream is counted from the inputs: a
workgroup re-reads the packed recurrent weights (425 984 bytes; 851 968 in float32) from L2 for every 32-row tile of a level
above height 0, tiles = sum over workgroups and levels of ceil(nodes / 32) with ftl_group's grouping.

On tests/golden/policy_head_cfg*_uniform.npz (the reference's observations and seeded weights at both scales): the share of agents
whose "hard" action under the bf16 encoder equals the float32 encoder's, and the largest |difference| of a logit.  Recorded, not
asserted.

Usage:  python tools/tree_lstm_bf16_bench.py [--parent-lib parent/libflatland_hip.so] [--rounds 5] [--launches 20] [--warmup 5]
                                             [--out profiles/tree_lstm_bf16_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 16 * 157.3e12
RECURRENT_FLOP = 2 * (384 * 384 + 3 * 128 * 128 + 384 * 128)      # a node above height 0
PACKED_BYTES = 2 * (384 * 384 + 128 * 384 + 128 * 128)
SHAPES = [("cfg2_1env", "cfg2", 1, 31), ("cfg2", "cfg2", 256, 31), ("cfg3", "cfg3", 1024, 31)]
MODES = ("all", "roots")
ROWS = 32


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


def inner_tiles(node_order, G):
    """32-row tiles of levels above height 0, over the workgroups of G trees"""
    import numpy as np
    no = node_order.reshape(-1, node_order.shape[-1]).cpu().numpy()
    tiles = 0
    for g in range(0, len(no), G):
        v, c = np.unique(no[g:g + G][no[g:g + G] > 0], return_counts=True)
        tiles += int(((c + ROWS - 1) // ROWS).sum())
    return tiles


def f32_call(L, x, w, roots_only):
    """a closure that enqueues fl_tree_lstm of library L (bound: hip_backend.bind) on the current stream with buffers allocated here"""
    import torch
    vp = C.c_void_p
    N = x[0].shape[-2]
    T = x[0].numel() // (N * 12)
    n = L.fl_tree_lstm_workspace_bytes(T, N, roots_only)
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=x[0].device)
    h = torch.empty((T if roots_only else T * N, 128), device=x[0].device)
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(keep=(ws, h)):
        rc = L.fl_tree_lstm(T, N, *[v.data_ptr() for v in x], *[v.data_ptr() for v in w], roots_only, h.data_ptr(), None, None,
                            ws.data_ptr(), ws.numel(), s)
        assert rc == 0, rc
    return call, h


def bf16_call(L, x, w, roots_only):
    """the same for fl_tree_lstm_bf16 of library L, on the buffer that L's own fl_tree_lstm_pack_bf16 packs here"""
    import torch
    vp = C.c_void_p
    fn = L.fl_tree_lstm_bf16
    N = x[0].shape[-2]
    T = x[0].numel() // (N * 12)
    s = vp(torch.cuda.current_stream().cuda_stream)
    packed = torch.empty(L.fl_tree_lstm_bf16_packed_bytes(), dtype=torch.uint8, device=x[0].device)
    rc = L.fl_tree_lstm_pack_bf16(w[2].data_ptr(), w[3].data_ptr(), w[7].data_ptr(), packed.data_ptr(), packed.numel(), s)
    assert rc == 0, rc
    n = L.fl_tree_lstm_bf16_workspace_bytes(T, N, roots_only)
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=x[0].device)
    h = torch.empty((T if roots_only else T * N, 128), device=x[0].device)

    def call(keep=(ws, h, packed)):
        rc = fn(T, N, *[v.data_ptr() for v in x], *[w[i].data_ptr() for i in (0, 1, 4, 5, 6)], packed.data_ptr(), packed.numel(),
                roots_only, h.data_ptr(), None, None, ws.data_ptr(), ws.numel(), s)
        assert rc == 0, rc
    return call, h


def action_agreement(dev):
    """per policy-head fixture and weight scale: hard actions under the bf16 encoder against the float32 encoder's"""
    import numpy as np
    import torch
    from flatland_marl_amd.policy import Network
    from tests import util
    from tests.test_policy_head_golden import golden_params, load
    from tests.tree_lstm_torch import modify_adjacency
    out = []
    for name in ("cfg1_uniform", "cfg2_uniform", "cfg3_uniform"):
        g = load(name)
        fx = util.load(str(g["fixture"]))
        idx = list(g["obs_index"])
        attr = torch.from_numpy(np.ascontiguousarray(fx["o_attr"][idx])).to(dev)
        forest = torch.from_numpy(np.ascontiguousarray(fx["o_forest"][idx])).to(dev)
        adj = modify_adjacency(np.ascontiguousarray(fx["o_adjacency"][idx])).to(dev).contiguous()
        no = torch.from_numpy(np.ascontiguousarray(fx["o_node_order"][idx])).to(torch.int64).to(dev)
        eo = torch.from_numpy(np.ascontiguousarray(fx["o_edge_order"][idx])).to(torch.int64).to(dev)
        valid = torch.from_numpy(np.ascontiguousarray(g["valid"])).to(dev)
        for s in range(len(g["scales"])):
            net = Network().to(dev)
            net.load_state_dict(golden_params(g, s))
            net16 = Network.from_module(net, precision="bf16")
            with torch.no_grad():
                (l32,), _ = net(attr, forest, adj, no, eo)
                (l16,), _ = net16(attr, forest, adj, no, eo)
                a32 = net.act(attr, forest, adj, no, eo, valid, "hard")
                a16 = net16.act(attr, forest, adj, no, eo, valid, "hard")
                t32, t16 = net.tree_lstm.roots(forest, adj, no, eo), net16.tree_lstm.roots(forest, adj, no, eo)
            out.append(dict(fixture=name, scales=[float(v) for v in g["scales"][s]], agents=int(a32.numel()),
                            same_hard_action_share=float((a32 == a16).float().mean()),
                            max_abs_dlogit=float((l32 - l16).abs().max()), max_abs_logit=float(l32.abs().max()),
                            max_abs_dtree=float((t32 - t16).abs().max())))
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libflatland_hip.so of the parent commit, for the A/B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_lstm_bf16_bench: no GPU visible (the measurement has no CPU path)")
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd.policy import PARAM_ORDER
    from tests.tree_lstm_torch import seeded_params
    from tools.tree_lstm_bench import inputs
    dev = torch.device("cuda:0")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    params = seeded_params(7)
    w = [params[k].to(dev).contiguous() for k in PARAM_ORDER]
    parent = hb.bind(C.CDLL(os.path.abspath(args.parent_lib))) if args.parent_lib else None
    parent_has_bf16 = parent is not None and hasattr(parent, "fl_tree_lstm_bf16")
    rows = []
    for label, wl_name, B, N in SHAPES:
        x = inputs(wl_name, B, N)
        T = x[1].shape[0] * x[1].shape[1]
        G = max(1, min(16, (T + 2 * cu - 1) // (2 * cu)))
        internal = int((x[2] > 0).sum())
        tiles = inner_tiles(x[2], G)
        for mode in MODES:
            ro = int(mode == "roots")
            calls = []
            if parent is not None:
                calls.append(("parent_f32", f32_call(parent, x, w, ro)))
            if parent_has_bf16:
                calls.append(("parent_bf16", bf16_call(parent, x, w, ro)))
            calls += [("f32", f32_call(hb.lib(), x, w, ro)), ("bf16", bf16_call(hb.lib(), x, w, ro))]
            med = {k: [] for k, _ in calls}
            for _ in range(args.rounds):
                for k, (call, _) in calls:
                    med[k].append(round(median_events(call, args.warmup, args.launches) * 1e3, 2))
            torch.cuda.synchronize()
            outs = {k: h for k, (_, h) in calls}
            mid = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
            flop = internal * RECURRENT_FLOP
            r = dict(shape=label, workload=wl_name, envs=B, trees=T, nodes=N, mode=mode, trees_a_workgroup=G, internal_nodes=internal,
                     inner_tiles=tiles, us_rounds=med, us_median=mid,
                     max_abs_dh_bf16_vs_f32=float((outs["bf16"] - outs["f32"]).abs().max()),
                     speedup_bf16_vs_f32=round(mid["f32"] / mid["bf16"], 3),
                     recurrent_flop=flop, bf16_tflops=round(flop / (mid["bf16"] * 1e-6) / 1e12, 2),
                     share_of_bf16_matrix_peak=round(flop / (mid["bf16"] * 1e-6) / PEAK_BF16, 5),
                     weight_bytes_a_tile=dict(bf16=PACKED_BYTES, f32=2 * PACKED_BYTES),
                     weight_stream_tb_s=dict(bf16=round(tiles * PACKED_BYTES / (mid["bf16"] * 1e-6) / 1e12, 3),
                                             f32=round(tiles * 2 * PACKED_BYTES / (mid["f32"] * 1e-6) / 1e12, 3)))
            if parent is not None:
                assert torch.equal(outs["parent_f32"], outs["f32"]), "fl_tree_lstm of this build differs from the parent's"
                lo, hi = min(med["parent_f32"]), max(med["parent_f32"])
                r.update(f32_bits_equal_parent=True, parent_spread_us=round(hi - lo, 2),
                         f32_median_inside_parent_range=bool(lo <= mid["f32"] <= hi),
                         speedup_bf16_vs_parent_f32=round(mid["parent_f32"] / mid["bf16"], 3),
                         bf16_faster_than_parent_by_more_than_its_spread=bool(mid["parent_f32"] - mid["bf16"] > hi - lo))
            if parent_has_bf16:
                lo, hi = min(med["parent_bf16"]), max(med["parent_bf16"])
                r.update(bf16_bits_equal_parent=bool(torch.equal(outs["parent_bf16"], outs["bf16"])),
                         parent_bf16_spread_us=round(hi - lo, 2),
                         bf16_not_slower_than_parent_bf16_by_more_than_its_spread=bool(mid["bf16"] - mid["parent_bf16"] <= hi - lo))
            rows.append(r)
            print(json.dumps(r), flush=True)
            del calls, outs
        del x
        torch.cuda.empty_cache()
    agree = action_agreement(dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/tree_lstm_bf16_bench.py", device=torch.cuda.get_device_name(0), compute_units=cu,
                           peak_bf16_matrix_tflops=PEAK_BF16 / 1e12, launches=args.launches, warmup=args.warmup, rounds=args.rounds,
                           parent_lib=bool(parent), results=rows, hard_action_agreement=agree), f, indent=1)


if __name__ == "__main__":
    main()
