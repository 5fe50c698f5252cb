"""bench.py --dump-outputs: what the last timed step handed its caller, as float32 / float64 .npy files of finite numbers, at most
DUMP_LIMIT bytes in all (CPU: the naming, the exact round trip of non-finite entries through <name>_nonfinite.npy, the sampling; GPU:
a plain run and a --full run of the same arguments write the same arrays, and the plain line carries the headline only)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CUTILS_KEYS = ("agent_attr", "forest", "adjacency", "node_order", "edge_order", "valid_actions", "props")
FLOAT_KEYS = ("agent_attr", "forest", "props", "tree")       # (their files have a <name>_nonfinite.npy beside them)


def fake_outputs(B, A=3, N=5):
    g = torch.Generator().manual_seed(7)
    o = dict(agent_attr=torch.rand(B, A, 83, generator=g), forest=torch.rand(B, A, N, 12, generator=g),
             adjacency=torch.randint(-2, 9, (B, A, N - 1, 3), generator=g, dtype=torch.int32),
             node_order=torch.randint(0, 9, (B, A, N), generator=g, dtype=torch.int32),
             edge_order=torch.randint(0, 9, (B, A, N - 1), generator=g, dtype=torch.int32),
             valid_actions=torch.randint(0, 2, (B, A, 5), generator=g, dtype=torch.uint8),
             props=torch.rand(B, A, 3, generator=g, dtype=torch.float64))
    step = (torch.randint(-1, 2, (B, A), generator=g, dtype=torch.int32), torch.randint(0, 2, (B, A), generator=g, dtype=torch.uint8),
            torch.randint(0, 2, (B,), generator=g, dtype=torch.uint8))
    tree = torch.full((B, A, 21, 12), -np.inf, dtype=torch.float64)
    tree[:, :, 0] = torch.rand(B, A, 12, generator=g, dtype=torch.float64)
    tree[:, :, 0, 3] = np.inf                   # (the upstream tree's unreachable distances)
    tree[0, 0, 1, 1] = np.nan
    return step, o, tree


def load_dump(d, name):
    """the output as it was: <name>.npy with its non-finite entries restored from <name>_nonfinite.npy, when that exists"""
    a = np.load(os.path.join(d, name + ".npy"))
    assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    code_path = os.path.join(d, name + "_nonfinite.npy")
    if os.path.exists(code_path):
        c = np.load(code_path)
        assert c.dtype == np.float32 and c.shape == a.shape and set(np.unique(c)) <= {-1.0, 0.0, 1.0, 2.0}, name
        assert (a[c != 0] == 0).all(), name
        a = a.copy()
        a[c == 1], a[c == -1], a[c == 2] = np.inf, -np.inf, np.nan
    return a


def test_named_outputs_of_the_fused_and_the_policy_paths():
    step, o, tree = fake_outputs(4)
    fused = [(None, "step"), (None, "obs_cutils_tree_fused")]
    n = bench.named_outputs(fused, [step, (o, tree)])
    assert list(n) == ["rewards", "dones", "done_all"] + list(CUTILS_KEYS) + ["tree"]
    assert n["tree"] is tree and n["rewards"] is step[0]
    # fl_obs_cutils + fl_policy_pack: the pack returns the cutils buffers' attr / forest again (named once) and int64 index tensors
    # of its own (named after their stage); the masked distance-map rebuild hands the caller nothing
    pol = (o["agent_attr"], o["forest"], o["adjacency"].long(), o["node_order"].long(), o["edge_order"].long())
    stages = [(None, "step"), (None, "obs_cutils"), (None, "policy_pack"), (None, "dm_rebuild_masked")]
    n = bench.named_outputs(stages, [step, o, pol, None])
    assert list(n) == ["rewards", "dones", "done_all"] + list(CUTILS_KEYS) + ["policy_pack.adjacency", "policy_pack.node_order",
                                                                              "policy_pack.edge_order"]


def test_dump_writes_float_arrays_exactly(tmp_path):
    step, o, tree = fake_outputs(4)
    n = bench.named_outputs([(None, "step"), (None, "obs_cutils_tree_fused")], [step, (o, tree)])
    bench.dump_outputs(n, str(tmp_path), 4)
    # every file finite; every floating-point output has its code array (non-finite entries of the tree: -inf, +inf, NaN)
    assert sorted(os.listdir(tmp_path)) == sorted([k + ".npy" for k in n] + [k + "_nonfinite.npy" for k in FLOAT_KEYS])
    assert not np.load(os.path.join(tmp_path, "forest_nonfinite.npy")).any()
    for f in os.listdir(tmp_path):
        assert np.isfinite(np.load(os.path.join(tmp_path, f))).all(), f
    for k, t in n.items():
        a = load_dump(str(tmp_path), k)
        assert a.dtype == (np.float64 if t.dtype in (torch.float64, torch.int32, torch.int64) else np.float32), k
        np.testing.assert_array_equal(a, t.numpy().astype(a.dtype), err_msg=k)
        if t.dtype.is_floating_point:
            assert np.array_equal(a.astype(t.numpy().dtype), t.numpy(), equal_nan=True), k     # no value lost in the conversion
        else:
            assert np.array_equal(a.astype(t.numpy().dtype), t.numpy()), k
    assert np.isneginf(load_dump(str(tmp_path), "tree")).sum() == (~torch.isfinite(tree)).sum().item() - 4 * 3 - 1


def test_dump_over_the_limit_keeps_the_same_seeded_sample_of_envs(tmp_path):
    B = 64
    step, o, tree = fake_outputs(B)
    n = bench.named_outputs([(None, "step"), (None, "obs_cutils_tree_fused")], [step, (o, tree)])
    full_bytes = sum(t.numel() * (8 if t.dtype in (torch.float64, torch.int32, torch.int64) else 4) for t in n.values())
    limit = full_bytes // 5
    for d in ("a", "b"):
        bench.dump_outputs(n, str(tmp_path / d), B, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "tree_nonfinite.npy" in files
    assert sum(np.load(os.path.join(tmp_path, "a", f)).nbytes for f in files) <= limit
    got = {k: load_dump(str(tmp_path / "a"), k) for k in n}
    kept = len(got["rewards"])
    assert 1 <= kept < B and all(len(a) == kept for a in got.values())
    # the same envs of every output (in order), the same envs from run to run
    rows = [next(b for b in range(B) if np.array_equal(got["forest"][i], o["forest"][b].numpy())) for i in range(kept)]
    assert rows == sorted(rows)
    for k, t in n.items():
        np.testing.assert_array_equal(got[k], t.numpy()[rows].astype(got[k].dtype), err_msg=k)
        np.testing.assert_array_equal(got[k], load_dump(str(tmp_path / "b"), k), err_msg=k)


def _bench(args, tmp):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--envs", "8"] + args,
                       capture_output=True, text=True, timeout=300, cwd=tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")], str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 6 and plain["agent_steps"] == 8 * plain["config"]["agents"] * 6
    assert abs(plain["value"] - plain["agent_steps"] / (plain["ms_per_step"] * 6 * 1e-3)) <= 2e-5 * plain["value"]
    for k in ("roofline", "kernel_ms", "cpu_baseline", "workloads", "detail_file"):
        assert k not in plain, k
    full = _bench(["--full", "--no-cpu-baseline", "--no-extra-workloads", "--detail", str(tmp_path / "detail.json"),
                   "--dump-outputs", str(tmp_path / "full")], str(tmp_path))
    assert full["roofline"]["frac"] > 0 and set(full["kernel_ms"]) == {"step", "obs_cutils_tree_fused"}
    names = sorted(os.listdir(tmp_path / "plain"))
    # the upstream tree's absent branches are -inf: written as 0, the code arrays beside every floating-point output
    assert names == sorted([k + ".npy" for k in ("rewards", "dones", "done_all", "tree") + CUTILS_KEYS] + [k + "_nonfinite.npy" for k in FLOAT_KEYS])
    assert names == sorted(os.listdir(tmp_path / "full"))
    A = plain["config"]["agents"]
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape[:2] == ((8, A) if f != "done_all.npy" else (8,)), f
        assert np.isfinite(a).all() and a.dtype == b.dtype and np.array_equal(a, b), f
    tree = load_dump(str(tmp_path / "plain"), "tree")
    assert np.isneginf(tree).any() and np.isfinite(tree[:, :, 0]).any()
