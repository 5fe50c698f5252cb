"""CPU: the TreeLSTM restatement (tests/tree_lstm_torch.py) against the reference module's outputs (tests/golden/tree_lstm_*.npz,
tools/capture_tree_lstm.py), the GPU module's parameter names against the reference's, and fl_tree_lstm's refusals, which come
before any HIP call and so need no GPU."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import util
from tests import tree_lstm_torch as tl

GOLDENS = sorted(glob.glob(os.path.join(util.GOLD, "tree_lstm_*.npz")))
NAMES = [os.path.basename(p)[len("tree_lstm_"):-4] for p in GOLDENS]


def golden_inputs(g):
    """the inputs a golden was captured on: its fixture's observations at its obs indices, first `agents` agents, adjacency
    modified as Network.modify_adjacency does"""
    fx = util.load(str(g["fixture"]))
    idx, a = list(g["obs_index"]), int(g["agents"])
    forest = torch.from_numpy(np.ascontiguousarray(fx["o_forest"][idx, :a]))
    adjacency = tl.modify_adjacency(np.ascontiguousarray(fx["o_adjacency"][idx, :a]))
    node_order = torch.from_numpy(np.ascontiguousarray(fx["o_node_order"][idx, :a])).to(torch.int64)
    edge_order = torch.from_numpy(np.ascontiguousarray(fx["o_edge_order"][idx, :a])).to(torch.int64)
    return forest, adjacency, node_order, edge_order


def golden_params(g, scale):
    return tl.seeded_params(int(g["seed"]), float(scale), [(str(n), tuple(int(v) for v in s if v >= 0))
                                                           for n, s in zip(g["param_names"], g["param_shapes"])])


def assert_close(h, c, gh, gc):
    h, c = np.asarray(h, dtype=np.float64), np.asarray(c, dtype=np.float64)
    assert np.abs(h - gh).max() <= 1e-5, np.abs(h - gh).max()
    assert (np.abs(c - gc) <= 1e-5 * np.maximum(1.0, np.abs(gc))).all(), np.abs(c - gc).max()


def test_goldens_present():
    assert set(NAMES) >= {"cfg2_uniform", "cfg0_tall_uniform", "cfg3_uniform", "nodes64_cfg3"}
    for p in GOLDENS:
        assert os.path.getsize(p) < 256 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = np.load(os.path.join(util.GOLD, "tree_lstm_%s.npz" % name))
    forest, adjacency, node_order, edge_order = golden_inputs(g)
    B, A, N = node_order.shape
    assert not tl.triple_rule_violations(adjacency, node_order, edge_order).any()
    ids = list(g["tree_ids"])
    for s, scale in enumerate(g["scales"]):
        h, c = tl.tree_lstm(forest, adjacency, node_order, edge_order, golden_params(g, scale), with_c=True)
        h, c = h.view(B * A, N, -1), c.view(B * A, N, -1)
        assert_close(h[:, 0], c[:, 0], g["root_h"][s], g["root_c"][s])
        assert_close(h[ids], c[ids], g["all_h"][s], g["all_c"][s])
        pad = node_order.view(B * A, N) == -2
        assert pad.any() or name in ("cfg3_uniform", "nodes64_cfg3")
        assert (h[pad] == 0).all() and (c[pad] == 0).all()


def test_golden_saturation_scale():
    """the x4 weights drive the gates into saturation (what the second scale is for)"""
    g = np.load(os.path.join(util.GOLD, "tree_lstm_cfg2_uniform.npz"))
    assert list(g["scales"]) == [1.0, 4.0]
    assert np.abs(g["root_h"][1]).max() > np.abs(g["root_h"][0]).max()


def test_state_dict_matches_reference():
    from flatland_marl_amd.policy import TreeLSTM
    g = np.load(os.path.join(util.GOLD, "tree_lstm_cfg2_uniform.npz"))
    ref = [(str(n), tuple(int(v) for v in s if v >= 0)) for n, s in zip(g["param_names"], g["param_shapes"])]
    mine = [(k, tuple(v.shape)) for k, v in TreeLSTM().state_dict().items()]
    assert mine == ref
    # a reference state_dict loads unchanged, and from_module shares the parameters
    m = TreeLSTM()
    m.load_state_dict(golden_params(g, 1.0))
    m2 = TreeLSTM.from_module(m)
    assert all(a is b for a, b in zip(m.parameters(), m2.parameters()))
    with pytest.raises(ValueError):
        TreeLSTM(12, 64)


def test_nodes50_reference_raises():
    """N = 50: (N - 1) % 3 != 0, the reference's edge triples do not divide -- it raises; fl_tree_lstm refuses the size"""
    g = np.load(os.path.join(util.GOLD, "tree_lstm_cfg2_uniform.npz"))
    assert str(g["nodes50_exception"]) == "RuntimeError"


# ---- fl_tree_lstm refusals: every call below fails a check that comes before any HIP call (the pointers are never used)
FAKE = 0x10000      # 16-byte aligned, never dereferenced


def call(T=2, N=31, roots_only=0, ws=None, **null):
    L = hb.lib()
    names = ("forest", "adj", "no", "eo", "w_iou", "b_iou", "u_iou", "w_c", "b_c", "w_f", "b_f", "u_f", "h")
    ptrs = dict.fromkeys(names, FAKE)
    ptrs.update(null)
    p = [C.c_void_p(ptrs[k]) if ptrs[k] else None for k in names]
    need = L.fl_tree_lstm_workspace_bytes(max(T, 1), N, 1 if roots_only else 0)
    rc = L.fl_tree_lstm(T, N, *p[:12], roots_only, p[12], None, None, C.c_void_p(FAKE), need if ws is None else ws, None)
    return rc, L.fl_last_error().decode()


def test_workspace_bytes():
    L = hb.lib()
    assert L.fl_tree_lstm_workspace_bytes(10, 31, 0) == 10 * 31 * 128 * 4
    assert L.fl_tree_lstm_workspace_bytes(10, 31, 1) == 2 * 10 * 31 * 128 * 4
    assert L.fl_tree_lstm_workspace_bytes(0, 31, 0) == 0


@pytest.mark.parametrize("kw, words", [
    (dict(N=50), "% 3"), (dict(N=65), "bad sizes"), (dict(T=0), "bad sizes"), (dict(T=-3), "bad sizes"),
    (dict(forest=0), "forest is NULL"), (dict(adj=0), "adjacency is NULL"), (dict(u_f=0), "u_f is NULL"), (dict(h=0), "h is NULL"),
    (dict(no=FAKE + 4), "not 8-byte aligned"), (dict(w_c=FAKE + 8), "not 16-byte aligned"),
    (dict(ws=1000), "workspace"), (dict(roots_only=1, ws=2 * 31 * 512), "workspace"), (dict(roots_only=2), "roots_only"),
])
def test_refusals(kw, words):
    rc, msg = call(**kw)
    assert rc == 1, (rc, msg)
    assert words in msg, msg
