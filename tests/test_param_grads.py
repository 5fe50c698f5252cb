"""CPU: the parameter-gradient entry points (include/flatland_param_grads.h) -- the header, the binding and the library agree; the
byte functions; the param_grads switch of policy.TreeLSTM / policy.Network; and the numpy restatement of the summation scheme
(tests/param_grads_np.py) inside its a-priori bound.  The kernels themselves: tests/test_gpu_param_grads.py."""
import os
import re

import numpy as np
import pytest

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import param_grads_np as pn

NAMES = ["fl_policy_head_param_grads_workspace_bytes", "fl_policy_head_param_grads", "fl_tree_lstm_param_grads_workspace_bytes",
         "fl_tree_lstm_param_grads"]
HEAD_DOUBLES = sum(s[0] * (s[1] + 1) for s in hb.POLICY_HEAD_PARAM_SHAPES if len(s) == 2)
HEAD_AUTO, TREE_AUTO = 2, 15      # the automatic rule's ceilings, as the header states them
TREE_DOUBLES = 384 * 13 + 384 * 384 + 128 * 385 + 128 * 13 + 128 * 128       # W_iou + b, U_iou, W_c + b, W_f + b, U_f


def test_header_binding_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    hb.build()                                                             # (the tests below call the library)
    hdr, decls = cabi.text("flatland_param_grads.h"), cabi.declarations("flatland_param_grads.h")
    assert [n for _, n, _ in decls] == list(hb.symbols("flatland_param_grads.h")) == NAMES
    assert '#include "flatland_policy_train.h"' in hdr and '#include "flatland_train.h"' in hdr
    params = {n: ps for _, n, ps in decls}
    assert params["fl_policy_head_param_grads"] == [
        "int n_envs", "int n_agents", "const float *attr_dev", "const void *saved_dev", "const void *rows_dev", "int actor", "int critic",
        "float *const *grads", "int slices", "void *workspace_dev", "size_t workspace_bytes", "void *hip_stream"]
    assert params["fl_tree_lstm_param_grads"] == [
        "int n_rows", "const float *x_dev", "const int64_t *node_order_dev", "const float *h_dev", "const float *da_dev",
        "const float *dc_dev", "const float *dg_dev", "const float *q_dev", "const int32_t *child_dev", "float *const *grads",
        "int slices", "void *workspace_dev", "size_t workspace_bytes", "void *hip_stream"]
    assert callable(hb.policy_head_param_grads) and callable(hb.tree_lstm_param_grads)


def test_the_existing_headers_declare_what_they_did():
    for header in ("flatland_policy_train.h", "flatland_train.h"):
        assert "flatland_param_grads.h" in open(os.path.join(cabi.INCLUDE, header)).read()      # the pointer, in the comment
        assert "param_grads" not in cabi.text(header)
        assert re.findall(r"\b(fl_[a-z_0-9]+)\s*\(", cabi.text(header)) == list(hb.symbols(header))


def test_shapes_and_orders_are_the_modules():
    from flatland_marl_amd import policy
    assert policy.REDUCE_BLOCK == pn.REDUCE_BLOCK
    net = policy.Network()
    sd = dict(net.named_parameters())
    assert [tuple(sd[k].shape) for k in policy.HEAD_PARAM_ORDER] == list(hb.POLICY_HEAD_PARAM_SHAPES)
    assert [tuple(sd["tree_lstm." + k].shape) for k in policy.PARAM_ORDER] == list(hb.TREE_LSTM_PARAM_SHAPES)
    assert HEAD_DOUBLES == 1698694 and TREE_DOUBLES == 219776                    # the figures of the header


def test_byte_functions():
    cap = hb.PARAM_GRADS_MAX_SLICES
    for name, doubles, auto in (("fl_policy_head_param_grads_workspace_bytes", HEAD_DOUBLES, HEAD_AUTO),
                                ("fl_tree_lstm_param_grads_workspace_bytes", TREE_DOUBLES, TREE_AUTO)):
        fn = hb._sym(name)
        for rows, slices in ((0, 1), (-1, 0), (5, -1), (5, cap + 1)):
            assert fn(rows, slices) == 0
        for rows in (1, 255, 256, 257, 513, 100000):
            assert fn(rows, 1) == 0
            for s in (2, 3, cap):
                assert fn(rows, s) == s * doubles * 8
            blocks = -(-rows // 256)
            chosen = min(blocks, auto)
            assert fn(rows, 0) == (0 if chosen == 1 else chosen * doubles * 8)


def test_param_grads_switch():
    from flatland_marl_amd.policy import PARAM_GRADS, Network, TreeLSTM
    assert PARAM_GRADS == ("torch", "hip")
    m = TreeLSTM()
    assert m.param_grads == "torch" and TreeLSTM(param_grads="hip").param_grads == "hip"
    net = Network()
    assert net.param_grads == "torch" and net.tree_lstm.param_grads == "torch"
    both = Network(param_grads="hip")
    assert both.param_grads == "hip" and both.tree_lstm.param_grads == "hip"
    for bad in ("HIP", "", None, 1, "blas"):
        with pytest.raises(ValueError, match="param_grads must be 'torch' or 'hip'"):
            TreeLSTM(param_grads=bad)
        with pytest.raises(ValueError, match="param_grads must be 'torch' or 'hip'"):
            Network(param_grads=bad)
        with pytest.raises(ValueError, match="param_grads must be 'torch' or 'hip'"):
            TreeLSTM.from_module(m, param_grads=bad)
        if bad is not None:                                   # (None: the module's own)
            with pytest.raises(ValueError, match="param_grads must be 'torch' or 'hip'"):
                Network.from_module(net, param_grads=bad)
    # from_module: the given value, else the module's own; the encoder keeps its own
    assert TreeLSTM.from_module(m).param_grads == "torch" and TreeLSTM.from_module(m, param_grads="hip").param_grads == "hip"
    assert TreeLSTM.from_module(m, param_grads="hip").W_iou is m.W_iou
    net.param_grads = "hip"
    copy = Network.from_module(net)
    assert copy.param_grads == "hip" and copy.tree_lstm.param_grads == "torch"
    net.tree_lstm.param_grads = "hip"
    net.param_grads = "torch"
    copy = Network.from_module(net)
    assert copy.param_grads == "torch" and copy.tree_lstm.param_grads == "hip"
    given = Network.from_module(Network(), param_grads="hip")
    assert given.param_grads == "hip" and given.tree_lstm.param_grads == "hip"
    assert Network.from_module(both, trainable=True).trainable is True and Network.from_module(both).param_grads == "hip"


def test_slices_are_whole_blocks():
    assert pn.slice_blocks(1, 1) == [(0, 1)]
    assert pn.slice_blocks(513, 2) == [(0, 2), (2, 3)]
    assert pn.slice_blocks(513, 3) == [(0, 1), (1, 2), (2, 3)]
    assert pn.slice_blocks(257, 4) == [(0, 1), (1, 2), (2, 2), (2, 2)]
    for rows in (1, 255, 256, 257, 513, 1025, 5000):
        for s in (1, 2, 3, 7, 32):
            cut = pn.slice_blocks(rows, s)
            assert len(cut) == s and cut[0][0] == 0 and cut[-1][1] == -(-rows // 256)
            assert all(a[1] == b[0] for a, b in zip(cut, cut[1:]))


@pytest.mark.parametrize("slices", (1, 2, 3))
@pytest.mark.parametrize("R", (1, 255, 256, 257, 513))
def test_restatement_is_inside_the_bound(R, slices):
    """random rows, every shape class of the kernels' matrices (1, 5, 12, 83, 128 columns), the float64 product as the reference"""
    rng = np.random.default_rng([R, slices])
    for p, q in ((5, 128), (1, 128), (128, 12), (128, 83), (96, 130)):
        dz = rng.standard_normal((R, p)).astype(np.float32)
        x = rng.standard_normal((R, q)).astype(np.float32)
        dz64, x64 = dz.astype(np.float64), x.astype(np.float64)
        g64 = dz64.T @ x64
        g = pn.tn(dz, x, slices)
        assert g.dtype == np.float32 and g.shape == (p, q)
        frac = pn.fraction(g.astype(np.float64), g64, pn.weight_bound(dz64, x64, g64))
        assert frac <= 1.0, (p, q, frac)
        b64 = dz64.sum(0)
        b = pn.colsum(dz, slices)
        assert pn.fraction(b.astype(np.float64), b64, pn.bias_bound(dz64, b64)) <= 1.0
    # one slice of whole blocks is policy._tn's scheme: the blocks' float32 products added in float64, then the ragged rest
    if slices == 1:
        import torch
        from flatland_marl_amd import policy
        t = policy._tn(torch.from_numpy(dz), torch.from_numpy(x)).numpy()
        assert pn.fraction(t.astype(np.float64), g64, pn.weight_bound(dz64, x64, g64)) <= 1.0


def test_the_bound_is_not_vacuous():
    """a sequential float32 sum over all rows (no blocks, no float64) of a long positive column leaves the bias bound, the block scheme stays in"""
    n = 4096
    dz = np.random.default_rng(3).random((n, 1)).astype(np.float32)
    dz64 = dz.astype(np.float64)
    b64 = dz64.sum(0)
    naive = np.float32(0)
    for v in dz[:, 0]:
        naive = np.float32(naive + v)
    bound = pn.bias_bound(dz64, b64)
    assert pn.fraction(np.array([naive], dtype=np.float64), b64, bound) > 1.0
    assert pn.fraction(pn.colsum(dz).astype(np.float64), b64, bound) <= 1.0
