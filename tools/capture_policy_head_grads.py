#!/usr/bin/env python3
"""Golden gradients of the policy network after its tree encoder (solution/nn/net_tree.py:82-103) from the REAL reference Network
under torch's autograd, in float64.

The reference's Network is imported at capture time (nothing of it is copied), cast to float64 and fed the inputs the committed
tests/golden/policy_head_<name>.npz already define (tools/capture_policy_head.py's recipes: the three observation recipes and six
of the synthetic ones), with that tool's seeded weights at both scales of each recipe.  A stand-in for tree_lstm returns the
recipe's tree embedding as a float64 leaf that requires grad, so the reference's own forward and autograd deliver the gradient on
the tree embedding too.  Loss: sum(Rl * logits) + sum(Rv * value), Rl f64[B][A][5] and Rv f64[B] from
numpy.random.default_rng([R_SEED, scale index]).standard_normal (Rl first), in three modes: "logits" (the first term alone),
"value" (the second alone), "both".
-> tests/golden/grad_policy_head_<name>_x<scale index>.npz, one file per recipe and scale, data only:
  name (str), scale_index, r_seed, probe_seed i64, B, A i64, modes (str[3]) = logits, value, both; and per tensor P (the 38 head
  parameters, "." written "_", and "tree" = the tree embedding as [B*A][128]):
    whole_P   f64[3][shape]      the gradient itself, per mode: every bias, actor_net.4.weight, critic_net.4.weight
    right_P   f64[3][rows][K]    g @ v     every other matrix and tree: v f64[cols][K], u f64[K][rows] from
    left_P    f64[3][K][cols]    u @ g     numpy.random.default_rng([PROBE_SEED, index of P]).standard_normal, v first (tree: index 38)
    maxabs_P, sum_P  f64[3]      max |g| and the sum of g

Usage:  python tools/capture_policy_head_grads.py [--only NAME ...]
        python tools/capture_policy_head_grads.py --check [NAME ...]   re-capture into a temporary directory, compare (float64 to
                                                                       1e-13 of each array's max-abs: the BLAS's thread count may differ)
"""
import argparse
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO]
import capture_policy_head as cap  # noqa: E402  (puts the reference on sys.path and imports its Network)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import policy_head_torch as ph  # noqa: E402
from tests import util  # noqa: E402
from tests.test_policy_head_golden import golden_inputs, golden_params, load  # noqa: E402

R_SEED = 20261019
PROBE_SEED = 20261020
K = 2
MODES = ("logits", "value", "both")
NAMES = ("cfg1_uniform", "cfg2_uniform", "cfg3_uniform", "synth_b1_a1", "synth_b3_a1", "synth_b5_a20", "synth_b2_a33", "synth_b3_a64",
         "synth_b1_a130")
ORDER = tuple(n for n, _ in ph.head_shapes()) + ("tree",)
WHOLE = tuple(n for n in ORDER if n.endswith(".bias") or n.endswith("in_proj_bias") or n in ("actor_net.4.weight", "critic_net.4.weight"))
PROBED = tuple(n for n in ORDER if n not in WHOLE)


class GivenTree(torch.nn.Module):
    """stands in for tree_lstm: h of the single node of every tree, a float64 leaf"""

    def __init__(self, tree):
        super().__init__()
        self.tree = tree

    def forward(self, forest, adjacency, node_order, edge_order):
        return self.tree.reshape(-1, self.tree.shape[-1])


def upstream(s, B, A):
    rng = np.random.default_rng([R_SEED, s])
    return rng.standard_normal((B, A, 5)), rng.standard_normal((B,))


def probes(name, shape):
    rng = np.random.default_rng([PROBE_SEED, ORDER.index(name)])
    v = rng.standard_normal((shape[1], K))
    u = rng.standard_normal((K, shape[0]))
    return u, v


def summarise(grads):
    """{mode: {tensor: float64 array}} -> the arrays of a fixture"""
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


def reference_grads(g, s):
    attr, tree, _ = golden_inputs(g, s)
    B, A = attr.shape[:2]
    Rl, Rv = (torch.from_numpy(x) for x in upstream(s, B, A))
    rest = [torch.zeros((B, A, 1, 12), dtype=torch.float64), torch.zeros((B, A, 0, 3), dtype=torch.int64),
            torch.zeros((B, A, 1), dtype=torch.int64), torch.zeros((B, A, 0), dtype=torch.int64)]
    torch.set_default_dtype(torch.float64)
    try:
        net = cap.Network().double()
        net.load_state_dict({k: v.double() for k, v in golden_params(g, s).items()})
        leaf = tree.double().clone().requires_grad_(True)
        net.tree_lstm = GivenTree(leaf)
        grads = {}
        for mode in MODES:
            net.zero_grad()
            leaf.grad = None
            (logits,), value = net(attr.double(), *[t.clone() for t in rest])
            loss = ((logits * Rl).sum() if mode != "value" else 0.0) + ((value * Rv).sum() if mode != "logits" else 0.0)
            loss.backward()
            sd = dict(net.named_parameters())
            grads[mode] = {k: (np.zeros(tuple(sd[k].shape)) if sd[k].grad is None else sd[k].grad.numpy().copy()) for k in ORDER[:-1]}
            grads[mode]["tree"] = leaf.grad.numpy().reshape(B * A, 128).copy()
    finally:
        torch.set_default_dtype(torch.float32)
    return grads


def path_of(name, s, gold_dir):
    return os.path.join(gold_dir, "grad_policy_head_%s_x%d.npz" % (name, s))


def capture(name, gold_dir):
    torch.set_num_threads(1)
    g = load(name)
    B, A = int(g["B"]), int(g["A"])
    paths = []
    for s in range(len(g["scales"])):
        out = dict(name=np.array(name), scale_index=np.array(s, dtype=np.int64), r_seed=np.array(R_SEED, dtype=np.int64),
                   probe_seed=np.array(PROBE_SEED, dtype=np.int64), B=np.array(B, dtype=np.int64), A=np.array(A, dtype=np.int64),
                   modes=np.array(MODES))
        out.update(summarise(reference_grads(g, s)))
        path = path_of(name, s, gold_dir)
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {B} x {A} -> {os.path.getsize(path) / 1024:.0f} KB")
        assert os.path.getsize(path) < 1024 * 1024
        paths.append(path)
    return paths


def check(names):
    tmp = tempfile.mkdtemp(prefix="policy_head_grad_check_")
    problems = []
    try:
        for name in names:
            for new_path in capture(name, tmp):
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
    ap.add_argument("--check", nargs="*", default=None, metavar="NAME")
    args = ap.parse_args()
    if args.check is not None:
        bad = check(args.check or list(NAMES))
        for line in bad:
            print("MISMATCH", line)
        print("policy-head gradient golden check:", "OK" if not bad else f"{len(bad)} difference(s)")
        sys.exit(1 if bad else 0)
    for name in (args.only or NAMES):
        capture(name, util.GOLD)
