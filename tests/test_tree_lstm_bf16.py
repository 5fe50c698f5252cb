"""CPU: include/flatland_policy_bf16.h against its ctypes table and the built library, fl_tree_lstm_bf16's refusals (before any HIP
call), the precision switch of policy.TreeLSTM / policy.Network, the emulation the GPU tolerance rests on
(tests/tree_lstm_bf16_torch.py) against the float64 restatement, and the recorded errors
(tests/golden/synth_tree_lstm_bf16_errors.json) against the GPU test's cases and its factor R16."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import test_gpu_tree_lstm_bf16 as gpu
from tests import tree_lstm_bf16_torch as tl16
from tests import tree_lstm_forests as tf
from tests import tree_lstm_torch as tl
from tests import util
from tests.test_tree_lstm_golden import golden_params

NAMES = ["fl_tree_lstm_bf16_packed_bytes", "fl_tree_lstm_pack_bf16", "fl_tree_lstm_bf16_workspace_bytes", "fl_tree_lstm_bf16"]


def test_header_table_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    decls = cabi.declarations("flatland_policy_bf16.h")
    assert [name for _, name, _ in decls] == list(hb.symbols("flatland_policy_bf16.h")) == NAMES
    assert [r for r, _, _ in decls] == ["size_t", "int", "size_t", "int"]
    nargs = [len(p) for _, _, p in decls]
    assert nargs == [len(hb.ABI["flatland_policy_bf16.h"][n][0]) for n in NAMES] == [0, 6, 3, 20]
    assert '#include "flatland_hip.h"' in cabi.text("flatland_policy_bf16.h")
    hb.build()
    fn = hb.lib().fl_tree_lstm_bf16
    assert len(fn.argtypes) == 20 and fn.restype is C.c_int
    assert hb.lib().fl_tree_lstm_bf16_packed_bytes() == 2 * (384 * 384 + 128 * 384 + 128 * 128) == 425984
    assert hb.lib().fl_tree_lstm_bf16_workspace_bytes(10, 31, 1) == hb.lib().fl_tree_lstm_workspace_bytes(10, 31, 1)
    assert callable(hb.tree_lstm_pack_bf16) and callable(hb.tree_lstm_bf16)


FAKE = 0x10000      # 16-byte aligned, never dereferenced


def call(T=2, N=31, roots_only=0, ws=None, pk=425984, **null):
    L = hb.lib()
    names = ("forest", "adj", "no", "eo", "w_iou", "b_iou", "b_c", "w_f", "b_f", "packed", "h")
    ptrs = dict.fromkeys(names, FAKE)
    ptrs.update(null)
    p = [C.c_void_p(ptrs[k]) if ptrs[k] else None for k in names]
    need = L.fl_tree_lstm_bf16_workspace_bytes(max(T, 1), N, 1 if roots_only else 0)
    rc = L.fl_tree_lstm_bf16(T, N, *p[:10], pk, roots_only, p[10], None, None, C.c_void_p(FAKE), need if ws is None else ws, None)
    return rc, L.fl_last_error().decode()


@pytest.mark.parametrize("kw, words", [
    (dict(N=50), "% 3"), (dict(N=65), "bad sizes"), (dict(T=0), "bad sizes"), (dict(T=-3), "bad sizes"),
    (dict(forest=0), "forest is NULL"), (dict(adj=0), "adjacency is NULL"), (dict(packed=0), "packed is NULL"), (dict(h=0), "h is NULL"),
    (dict(no=FAKE + 4), "not 8-byte aligned"), (dict(packed=FAKE + 8), "not 16-byte aligned"), (dict(b_c=FAKE + 8), "not 16-byte aligned"),
    (dict(ws=1000), "workspace"), (dict(roots_only=1, ws=2 * 31 * 512), "workspace"), (dict(roots_only=2), "roots_only"),
    (dict(pk=425983), "packed buffer"),
])
def test_refusals_are_those_of_fl_tree_lstm(kw, words):
    rc, msg = call(**kw)
    assert rc == 1, (rc, msg)
    assert words in msg and msg.startswith("fl_tree_lstm_bf16:"), msg


def test_pack_refusals():
    L = hb.lib()
    ok = [C.c_void_p(FAKE)] * 4
    for i, word in enumerate(("u_iou", "w_c", "u_f", "packed")):
        a = list(ok)
        a[i] = None
        assert L.fl_tree_lstm_pack_bf16(*a, 425984, None) == 1 and (word + " is NULL") in L.fl_last_error().decode()
        a[i] = C.c_void_p(FAKE + 4)
        assert L.fl_tree_lstm_pack_bf16(*a, 425984, None) == 1 and (word + " is not 16-byte aligned") in L.fl_last_error().decode()
    assert L.fl_tree_lstm_pack_bf16(*ok, 425983, None) == 1 and "packed buffer" in L.fl_last_error().decode()


def test_precision_switch():
    from flatland_marl_amd.policy import Network, TreeLSTM
    g = np.load(os.path.join(util.GOLD, "tree_lstm_cfg2_uniform.npz"))
    m = TreeLSTM(precision="bf16")
    assert m.precision == "bf16" and TreeLSTM().precision == "f32"
    m.load_state_dict(golden_params(g, 1.0))                  # a reference state dict: the packed weights are no part of it
    assert list(m.state_dict()) == [str(n) for n in g["param_names"]]
    m2 = TreeLSTM.from_module(m, precision="bf16")
    assert m2.precision == "bf16" and TreeLSTM.from_module(m).precision == "f32"
    assert all(a is b for a, b in zip(m.parameters(), m2.parameters()))
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError):
            TreeLSTM(precision=bad)
        with pytest.raises(ValueError):
            TreeLSTM.from_module(m, precision=bad)
        with pytest.raises(ValueError):
            Network(precision=bad)
    net = Network(precision="bf16")
    assert net.tree_lstm.precision == "bf16" and Network().tree_lstm.precision == "f32"
    from tests import policy_head_torch as ph
    net.load_state_dict(ph.seeded_params(3, 3.0))
    assert Network.from_module(net).tree_lstm.precision == "bf16"
    assert Network.from_module(net, precision="f32").tree_lstm.precision == "f32"
    assert Network.from_module(Network(), precision="bf16").tree_lstm.precision == "bf16"


def test_bf16_with_trainable_raises_under_grad_mode_before_any_input_check():
    from flatland_marl_amd.policy import TreeLSTM
    x = tf.make("rand", 3, 31, 1)                             # CPU tensors: every input check would refuse them with TypeError
    m = TreeLSTM(precision="bf16", trainable=True)
    with pytest.raises(ValueError, match="inference only"):
        m(*x)
    with pytest.raises(ValueError, match="inference only"):
        m.roots(*x)
    with torch.no_grad(), pytest.raises(TypeError):           # no_grad: past that check, on to the inputs'
        m(*x)
    m.trainable = False
    with pytest.raises(TypeError):
        m(*x)
    m.precision = "f64"                                       # a plain attribute: a bad value is found at the next call
    with pytest.raises(ValueError, match="precision"):
        m(*x)


@pytest.mark.parametrize("kind", ["rand", "weird", "mixpad"])
def test_emulation_is_the_restatement_at_height_0_and_not_above(kind):
    x = tf.make(kind, 40, 31, 5, base="weird")
    params = tl.seeded_params(11, 1.0)
    h64, c64 = tl.tree_lstm(*x, params, with_c=True)
    he, ce = tl16.tree_lstm(*x, params, with_c=True)
    no = x[2].view(-1)
    low = no <= 0                                             # height 0 and padding
    assert (no == 0).sum() > 100 and (no > 0).sum() > 30
    assert torch.equal(he[low], h64[low]) and torch.equal(ce[low], c64[low])
    up = no > 0
    # (a node whose three children all read as zero -- the weird kind has a few -- has no recurrent term to round)
    assert (he[up] != h64[up]).any(1).float().mean() > 0.9 and (ce[up] != c64[up]).any(1).float().mean() > 0.9
    err = float((he - h64).abs().max())
    assert 1e-5 < err < 2e-2, err                             # bf16 has 8 bits: far above float32's 1e-7, far below the values
    # float32 sums on top of the same roundings change the error by much less than the error itself
    h32 = tl16.tree_lstm(*x, params, dtype=torch.float32)
    assert abs(float((h32.double() - h64).abs().max()) - err) < 0.05 * err


def test_recorded_errors_are_consistent():
    rec = json.load(open(gpu.ERRORS))
    assert gpu.R16 == 2 and rec["R16"] == 2
    assert set(rec["cases"]) == set(gpu.IDS) and len(gpu.IDS) == len(set(gpu.IDS))
    for name, c in rec["cases"].items():
        if name.startswith("flat-"):      # no node above height 0: e16 = 0, the case is held to the leaves' float32 bound alone
            assert c["e16_h"] == 0 and c["e16_c"] == 0 and c["ratio_h"] == 0 and c["ratio_c"] == 0
            assert 0 < c["err_h"] < 1e-5
            continue
        assert c["ratio_h"] == c["err_h"] / c["e16_h"] and c["ratio_c"] == c["err_c"] / c["e16_c"]
        assert c["ratio_h"] <= gpu.R16 and c["ratio_c"] <= gpu.R16, (name, c)
