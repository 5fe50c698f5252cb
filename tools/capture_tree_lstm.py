#!/usr/bin/env python3
"""Golden vectors of the policy's TreeLSTM forward (solution/nn/TreeLSTM.py) from the REAL reference module.

The reference's TreeLSTM and Network.modify_adjacency are imported at capture time (nothing of them is copied).  They are fed
trees already in tests/golden (the flatland_cutils observations o_forest / o_adjacency / o_node_order / o_edge_order of the
episode fixtures below, at the listed obs indices, the first `agents` agents), with weights from numpy.random.default_rng(SEED):
each parameter in state_dict order, uniform in +-scale/sqrt(fan_in), float32, at scale 1 and 4 (4 drives the gates into
saturation).  The forward is run as the module's own forward does it (zeroed h / c, _run_lstm per level) so that c can be kept
too; its h is asserted equal to module.forward's bit for bit.  -> tests/golden/tree_lstm_<fixture>.npz:
  fixture (str), obs_index i64[B], agents i64, seed i64, scales f32[S], param_names (str[8]), param_shapes i64[8][2] (-1 pad),
  root_h / root_c f32[S][B*agents][128], tree_ids i64[K], all_h / all_c f32[S][K][N][128] (K trees whole, one with padding),
  nodes50_exception (str): the class of what the reference raises on the N = 50 fixture (nodes50_cfg2).

Synthetic recipes (SYNTH below, names synth_*): forests from tests/tree_lstm_forests.py -- tree shapes the contract allows and no
observation has (chains, gapped heights, permuted ids, children that read as zero, all-padding trees) -- fed to the same reference
module.  -> tests/golden/synth_tree_lstm_<name>.npz, which holds the inputs themselves next to the generator's arguments:
  kind / feat / base (str), T, N, gen_seed, L, m (i64; L / m i64[k], empty = unused), forest f32[T][N][12], node_order i8[T][N],
  edge_order i8[T][N-1], adjacency i8[T][N-1][3] (tree-local ids, -2 padding), seed, scales, param_names, param_shapes, tree_ids,
  root_h / root_c, all_h / all_c as above, exception (str): the class of what the reference raised on this forest ("" = nothing;
  then the four outputs are empty and the tests compare that kind with the restatement only).

Usage:  python tools/capture_tree_lstm.py [--only NAME ...]
        python tools/capture_tree_lstm.py --check [NAME ...]   re-capture into a temporary directory, compare bit for bit
"""
import argparse
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("REF", "/root/reference")
sys.path[:0] = [os.path.join(REF, "solution"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from nn.net_tree import Network  # noqa: E402  (the reference's policy network module)
from nn.TreeLSTM import TreeLSTM  # noqa: E402

from tests import tree_lstm_forests as tf  # noqa: E402
from tests import util  # noqa: E402
from tests.tree_lstm_torch import seeded_params  # noqa: E402

SEED = 20261016
SCALES = (1.0, 4.0)
# fixture -> (obs indices, agents)
RECIPES = {
    "cfg2_uniform": ((8, 40), 20),          # obs 8 (step 64): padding edges and nodes (agent 3)
    "cfg0_tall_uniform": ((62, 20), 20),    # obs 62: padding (agent 17)
    "cfg3_uniform": ((7,), 80),             # 80 agents
    "nodes64_cfg3": ((2,), 40),             # N = 64, 8 levels
}

# synthetic recipes: name -> arguments of tree_lstm_forests.make (one small T per kind; N = 4, 31 and 64)
FX = "fixture:cfg2_uniform"
SYNTH = {
    "synth_rand_n4": dict(kind="rand", T=12, N=4, seed=101),
    "synth_rand_n31": dict(kind="rand", T=10, N=31, seed=102, feat=FX),
    "synth_rand_n64": dict(kind="rand", T=6, N=64, seed=103),
    "synth_chain_n4": dict(kind="chain", T=6, N=4, seed=104, feat=FX),
    "synth_chain_n31": dict(kind="chain", T=6, N=31, seed=105),
    "synth_chain_n64": dict(kind="chain", T=6, N=64, seed=106),
    "synth_full_n4": dict(kind="full", T=6, N=4, seed=107),
    "synth_full_n31": dict(kind="full", T=6, N=31, seed=108),
    "synth_full_n64": dict(kind="full", T=6, N=64, seed=109, feat=FX),
    "synth_perm_n31": dict(kind="perm", T=10, N=31, seed=110),
    "synth_perm_n64": dict(kind="perm", T=6, N=64, seed=111),
    "synth_gaps_n4": dict(kind="gaps", T=12, N=4, seed=112),
    "synth_gaps_n31": dict(kind="gaps", T=10, N=31, seed=113, feat=FX),
    "synth_gaps_n64": dict(kind="gaps", T=6, N=64, seed=114),
    "synth_flat_n4": dict(kind="flat", T=6, N=4, seed=115, L=(1, 3, 4)),
    "synth_flat_n64": dict(kind="flat", T=6, N=64, seed=116, L=(31, 32, 33, 64)),
    "synth_lvl1_n31": dict(kind="lvl1", T=8, N=31, seed=117, m=(0, 1, 2, 3, 4, 5, 6)),
    "synth_weird_n4": dict(kind="weird", T=12, N=4, seed=118),
    "synth_weird_n31": dict(kind="weird", T=10, N=31, seed=119),
    "synth_weird_n64": dict(kind="weird", T=6, N=64, seed=120, feat=FX),
    "synth_mixpad_n31": dict(kind="mixpad", T=10, N=31, seed=121, base="weird"),
    "synth_mixpad_n64": dict(kind="mixpad", T=7, N=64, seed=122, base="gaps"),
    "synth_allpad_n4": dict(kind="flat", T=3, N=4, seed=123, L=0),           # nothing but padding
}


def inputs(name):
    obs, agents = RECIPES[name]
    fx = util.load(name)
    idx = list(obs)
    forest = torch.from_numpy(np.ascontiguousarray(fx["o_forest"][idx, :agents]))
    adjacency = torch.from_numpy(np.ascontiguousarray(fx["o_adjacency"][idx, :agents])).to(torch.int64)
    node_order = torch.from_numpy(np.ascontiguousarray(fx["o_node_order"][idx, :agents])).to(torch.int64)
    edge_order = torch.from_numpy(np.ascontiguousarray(fx["o_edge_order"][idx, :agents])).to(torch.int64)
    adjacency = Network.modify_adjacency(None, adjacency, torch.device("cpu"))     # (self is not used)
    return forest, adjacency, node_order, edge_order


def run_reference(m, forest, adjacency, node_order, edge_order):
    """TreeLSTM.forward (TreeLSTM.py:33-56) with its c kept: the same zeroed buffers and _run_lstm calls"""
    f, a, no, eo = forest.flatten(0, 2), adjacency.flatten(0, 2), node_order.flatten(0, 2), edge_order.flatten(0, 2)
    h = torch.zeros(no.shape[0], m.out_features)
    c = torch.zeros(no.shape[0], m.out_features)
    for n in range(no.max() + 1):
        m._run_lstm(n, h, c, f, no, a, eo)
    assert torch.equal(h, m.forward(forest, adjacency, node_order, edge_order))
    return h, c


def nodes50_exception():
    fx = util.load("nodes50_cfg2")
    forest = torch.from_numpy(fx["o_forest"][:2])
    adjacency = Network.modify_adjacency(None, torch.from_numpy(fx["o_adjacency"][:2]).to(torch.int64), torch.device("cpu"))
    m = TreeLSTM(12, 128)
    try:
        with torch.no_grad():
            m(forest, adjacency, torch.from_numpy(fx["o_node_order"][:2]).to(torch.int64),
              torch.from_numpy(fx["o_edge_order"][:2]).to(torch.int64))
    except Exception as e:      # noqa: BLE001  (recording which one)
        return type(e).__name__
    return ""


def path_of(name, gold_dir):
    return os.path.join(gold_dir, ("%s.npz" if name in SYNTH else "tree_lstm_%s.npz") % name.replace("synth_", "synth_tree_lstm_"))


def capture(name, gold_dir):
    torch.set_num_threads(1)
    if name in SYNTH:
        return capture_synth(name, gold_dir)
    forest, adjacency, node_order, edge_order = inputs(name)
    B, A, N = node_order.shape
    T = B * A
    m = TreeLSTM(12, 128)
    sd = m.state_dict()
    names = list(sd)
    shapes = np.full((len(names), 2), -1, dtype=np.int64)
    for i, k in enumerate(names):
        shapes[i, :sd[k].dim()] = tuple(sd[k].shape)
    no = node_order.reshape(T, N)
    pad = [t for t in range(T) if (no[t] == -2).any() and (no[t] >= 0).any()]
    deep = int(torch.argmax(no.max(1).values))
    tree_ids = sorted(set(([pad[0]] if pad else []) + [deep] + ([] if name in ("cfg3_uniform", "nodes64_cfg3") else [T - 1])))
    if name in ("cfg3_uniform", "nodes64_cfg3"):
        tree_ids = [pad[0]] if pad else [deep]
    out = dict(fixture=np.array(name), obs_index=np.array(RECIPES[name][0], dtype=np.int64), agents=np.array(A, dtype=np.int64),
               seed=np.array(SEED, dtype=np.int64), scales=np.array(SCALES, dtype=np.float32), param_names=np.array(names),
               param_shapes=shapes, tree_ids=np.array(tree_ids, dtype=np.int64), nodes50_exception=np.array(nodes50_exception()))
    rh, rc, ah, ac = [], [], [], []
    for scale in SCALES:
        m.load_state_dict(seeded_params(SEED, scale, [(k, tuple(v.shape)) for k, v in sd.items()]))
        with torch.no_grad():
            h, c = run_reference(m, forest, adjacency.clone(), node_order, edge_order)
        h, c = h.view(T, N, -1), c.view(T, N, -1)
        rh.append(h[:, 0].numpy())
        rc.append(c[:, 0].numpy())
        ah.append(h[tree_ids].numpy())
        ac.append(c[tree_ids].numpy())
    out.update(root_h=np.stack(rh), root_c=np.stack(rc), all_h=np.stack(ah), all_c=np.stack(ac))
    path = os.path.join(gold_dir, "tree_lstm_%s.npz" % name)
    np.savez_compressed(path, **out)
    print(f"tree_lstm_{name}: {T} trees of {N} nodes, whole trees {tree_ids} -> {os.path.getsize(path) / 1024:.0f} KB")
    return path


def capture_synth(name, gold_dir):
    args = dict(feat="gauss", base="rand", L=None, m=None)
    args.update(SYNTH[name])
    no, eo, adj = tf.structure(*(args[k] for k in ("kind", "T", "N", "seed", "base", "L", "m")))
    x = tf.features(args["feat"], args["T"], args["N"], np.random.default_rng([args["seed"], 1]))
    forest, adjacency, node_order, edge_order = tf.to_policy(x, no, eo, adj)
    T, N = no.shape
    m = TreeLSTM(12, 128)
    sd = m.state_dict()
    names = list(sd)
    shapes = np.full((len(names), 2), -1, dtype=np.int64)
    for i, k in enumerate(names):
        shapes[i, :sd[k].dim()] = tuple(sd[k].shape)
    # whole trees: the tallest, then trees with padding and with real nodes, as many as keep the file small
    order = sorted(range(T), key=lambda t: (-int(no[t].max()), not ((no[t] == -2).any() and (no[t] >= 0).any()), t))
    tree_ids = sorted(order[:max(1, min(3, 80 // N))])
    seq = lambda v: np.array([] if v is None else np.atleast_1d(v), dtype=np.int64)     # noqa: E731
    out = dict(kind=np.array(args["kind"]), feat=np.array(args["feat"]), base=np.array(args["base"]), T=np.array(T, dtype=np.int64),
               N=np.array(N, dtype=np.int64), gen_seed=np.array(args["seed"], dtype=np.int64), L=seq(args["L"]), m=seq(args["m"]),
               forest=x, node_order=no.astype(np.int8), edge_order=eo.astype(np.int8), adjacency=adj.astype(np.int8),
               seed=np.array(SEED, dtype=np.int64), scales=np.array(SCALES, dtype=np.float32), param_names=np.array(names),
               param_shapes=shapes, tree_ids=np.array(tree_ids, dtype=np.int64))
    rh, rc, ah, ac, exc = [], [], [], [], ""
    for scale in SCALES:
        m.load_state_dict(seeded_params(SEED, scale, [(k, tuple(v.shape)) for k, v in sd.items()]))
        try:
            with torch.no_grad():
                h, c = run_reference(m, forest, adjacency.clone(), node_order, edge_order)
        except Exception as e:      # noqa: BLE001  (recording which one)
            exc = type(e).__name__
            break
        h, c = h.view(T, N, -1), c.view(T, N, -1)
        rh.append(h[:, 0].numpy())
        rc.append(c[:, 0].numpy())
        ah.append(h[tree_ids].numpy())
        ac.append(c[tree_ids].numpy())
    empty = np.zeros((0,), dtype=np.float32)
    out.update(exception=np.array(exc), root_h=empty if exc else np.stack(rh), root_c=empty if exc else np.stack(rc),
               all_h=empty if exc else np.stack(ah), all_c=empty if exc else np.stack(ac))
    path = path_of(name, gold_dir)
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {T} trees of {N} nodes, whole trees {tree_ids}, exception {exc!r} "
          f"-> {os.path.getsize(path) / 1024:.0f} KB")
    return path


def check(names):
    tmp = tempfile.mkdtemp(prefix="tree_lstm_check_")
    problems = []
    try:
        for name in names:
            new = np.load(capture(name, tmp))
            old_path = path_of(name, util.GOLD)
            if not os.path.exists(old_path):
                problems.append(f"{os.path.basename(old_path)}: no committed fixture")
                continue
            old = np.load(old_path)
            for k in sorted(set(new.files) | set(old.files)):
                if k not in new.files or k not in old.files:
                    problems.append(f"tree_lstm_{name}: key {k} only on one side")
                elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape or new[k].tobytes() != old[k].tobytes():
                    problems.append(f"tree_lstm_{name}: {k} differs from the reference's output")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", nargs="*", default=None, metavar="FIXTURE")
    args = ap.parse_args()
    if args.check is not None:
        bad = check(args.check or list(RECIPES) + list(SYNTH))
        for line in bad:
            print("MISMATCH", line)
        print("tree-lstm golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for name in (args.only or list(RECIPES) + list(SYNTH)):
        capture(name, util.GOLD)
