#!/usr/bin/env python3
"""Golden gradients of the policy's TreeLSTM (solution/nn/TreeLSTM.py) from the REAL reference module under torch's autograd, in
float64.

The reference's TreeLSTM is imported at capture time (nothing of it is copied), cast to float64 and fed
  cfg2_uniform                      the trees of tests/golden/tree_lstm_cfg2_uniform.npz (tools/capture_tree_lstm.py's recipe)
  synth_{weird_n31, chain_n64, mixpad_n31, rand_n4, allpad_n4}
                                    the inputs stored in tests/golden/synth_tree_lstm_<name>.npz
with the seeded weights of tools/capture_tree_lstm.py at scale 1 and 4.  Loss: sum(R * h) over the roots ("roots") and over every
node ("all"), R from numpy.random.default_rng([R_SEED, mode]).standard_normal, float64 (R is non-zero on padding nodes and on
nodes no root reaches, too).  -> tests/golden/grad_tree_lstm_<source>_x<scale>.npz, one file per source and scale (under 256 KB):
  source (str), scale f64, r_seed / probe_seed / seed i64, T, N i64, modes (str[2]) = roots, all; and per parameter P
  (W_iou.weight, ... with "." written "_"):
    whole_P   f64[2][shape]      the gradient itself, per mode (W_iou.weight, W_f.weight and the three biases)
    right_P   f64[2][rows][K]    g @ v     for U_iou.weight, W_c.weight, U_f.weight: v f64[cols][K], u f64[K][rows] from
    left_P    f64[2][K][cols]    u @ g     numpy.random.default_rng([PROBE_SEED, index of P]).standard_normal, v first
    maxabs_P, sum_P  f64[2]      max |g| and the sum of g
(The name does not begin with tree_lstm_: tests/test_tree_lstm_golden.py takes every tests/golden/tree_lstm_*.npz for a forward
golden.)

Usage:  python tools/capture_tree_lstm_grads.py [--only SOURCE ...]
        python tools/capture_tree_lstm_grads.py --check [SOURCE ...]   re-capture into a temporary directory, compare (float64
                                                                       to 1e-13 of each array's max-abs: the BLAS's thread count may differ)
"""
import argparse
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO]
import capture_tree_lstm as cap  # noqa: E402  (puts the reference on sys.path and imports its TreeLSTM)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import util  # noqa: E402
from tests.tree_lstm_torch import seeded_params  # noqa: E402

R_SEED = 20261018
PROBE_SEED = 20261019
K = 2
MODES = ("roots", "all")
SOURCES = ("cfg2_uniform", "synth_weird_n31", "synth_chain_n64", "synth_mixpad_n31", "synth_rand_n4", "synth_allpad_n4")
WHOLE = ("W_iou.weight", "W_iou.bias", "W_c.bias", "W_f.weight", "W_f.bias")
PROBED = ("U_iou.weight", "W_c.weight", "U_f.weight")
ORDER = ("W_iou.weight", "W_iou.bias", "U_iou.weight", "W_c.weight", "W_c.bias", "W_f.weight", "W_f.bias", "U_f.weight")


def stored_inputs(source):
    """the four input tensors of a source, from files already in tests/golden"""
    if source.startswith("synth_"):
        from tests import tree_lstm_forests as tf
        g = np.load(os.path.join(util.GOLD, "synth_tree_lstm_%s.npz" % source[len("synth_"):]))
        return tf.to_policy(g["forest"], g["node_order"].astype(np.int64), g["edge_order"].astype(np.int64),
                            g["adjacency"].astype(np.int64))
    return cap.inputs(source)


def upstream(mode, T, N):
    rng = np.random.default_rng([R_SEED, MODES.index(mode)])
    return rng.standard_normal((T if mode == "roots" else T * N, 128))


def probes(name, shape):
    rng = np.random.default_rng([PROBE_SEED, ORDER.index(name)])
    v = rng.standard_normal((shape[1], K))
    u = rng.standard_normal((K, shape[0]))
    return u, v


def summarise(grads):
    """{mode: {parameter: float64 array}} -> the arrays of a fixture"""
    out = {}
    for name in WHOLE:
        out["whole_" + name.replace(".", "_")] = np.stack([grads[m][name] for m in MODES])
    for name in PROBED:
        u, v = probes(name, grads[MODES[0]][name].shape)
        key = name.replace(".", "_")
        out["right_" + key] = np.stack([grads[m][name] @ v for m in MODES])
        out["left_" + key] = np.stack([u @ grads[m][name] for m in MODES])
        out["maxabs_" + key] = np.array([np.abs(grads[m][name]).max() for m in MODES])
        out["sum_" + key] = np.array([grads[m][name].sum() for m in MODES])
    return out


def reference_grads(x, scale):
    forest, adjacency, node_order, edge_order = x
    B, A, N = node_order.shape
    T = B * A
    torch.set_default_dtype(torch.float64)
    try:
        m = cap.TreeLSTM(12, 128).double()
        m.load_state_dict({k: v.double() for k, v in seeded_params(cap.SEED, scale).items()})
        grads = {}
        for mode in MODES:
            m.zero_grad()
            h = m(forest.double(), adjacency.clone(), node_order, edge_order).view(T, N, 128)
            out = h[:, 0] if mode == "roots" else h.reshape(T * N, 128)
            loss = (out * torch.from_numpy(upstream(mode, T, N))).sum()
            if loss.requires_grad:                       # (nothing but padding: no node was computed, every gradient is zero)
                loss.backward()
            grads[mode] = {k: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy()) for k, p in m.named_parameters()}
    finally:
        torch.set_default_dtype(torch.float32)
    return grads


def path_of(source, scale, gold_dir):
    return os.path.join(gold_dir, "grad_tree_lstm_%s_x%d.npz" % (source, scale))


def capture(source, gold_dir):
    torch.set_num_threads(1)
    x = stored_inputs(source)
    B, A, N = x[2].shape
    paths = []
    for scale in cap.SCALES:
        out = dict(source=np.array(source), scale=np.array(scale, dtype=np.float64), r_seed=np.array(R_SEED, dtype=np.int64),
                   probe_seed=np.array(PROBE_SEED, dtype=np.int64), seed=np.array(cap.SEED, dtype=np.int64),
                   T=np.array(B * A, dtype=np.int64), N=np.array(N, dtype=np.int64), modes=np.array(MODES))
        out.update(summarise(reference_grads(x, scale)))
        path = path_of(source, scale, gold_dir)
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {B * A} trees of {N} nodes -> {os.path.getsize(path) / 1024:.0f} KB")
        assert os.path.getsize(path) < 256 * 1024
        paths.append(path)
    return paths


def check(sources):
    tmp = tempfile.mkdtemp(prefix="tree_lstm_grad_check_")
    problems = []
    try:
        for source in sources:
            for new_path in capture(source, tmp):
                old_path = os.path.join(util.GOLD, os.path.basename(new_path))
                if not os.path.exists(old_path):
                    problems.append(f"{os.path.basename(old_path)}: no committed fixture")
                    continue
                new, old = np.load(new_path), np.load(old_path)
                for k in sorted(set(new.files) | set(old.files)):
                    if k not in new.files or k not in old.files:
                        problems.append(f"{os.path.basename(old_path)}: key {k} only on one side")
                    elif new[k].dtype != old[k].dtype or new[k].shape != old[k].shape:
                        problems.append(f"{os.path.basename(old_path)}: {k} has another type or shape")
                    elif new[k].dtype == np.float64:
                        if np.abs(new[k] - old[k]).max(initial=0) > 1e-13 * np.abs(old[k]).max(initial=0):
                            problems.append(f"{os.path.basename(old_path)}: {k} differs from the reference's gradient")
                    elif new[k].tobytes() != old[k].tobytes():
                        problems.append(f"{os.path.basename(old_path)}: {k} differs")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return problems


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", nargs="*", default=None, metavar="SOURCE")
    args = ap.parse_args()
    if args.check is not None:
        bad = check(args.check or list(SOURCES))
        for line in bad:
            print("MISMATCH", line)
        print("tree-lstm gradient golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for source in (args.only or SOURCES):
        capture(source, util.GOLD)
