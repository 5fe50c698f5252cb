"""CPU: include/flatland_policy.h against its ctypes binding and the built library, fl_policy_head's refusals (which come before
any HIP call and so need no GPU), policy.Network's parameter names against the reference's, and the restatement of the head and
of the action choice (tests/policy_head_torch.py) against the reference's outputs in tests/golden/policy_head_*.npz
(tools/capture_policy_head.py)."""
import ctypes as C
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import policy_head_torch as ph
from tests import util

GOLDENS = sorted(glob.glob(os.path.join(util.GOLD, "policy_head_*.npz")))
NAMES = [os.path.basename(p)[len("policy_head_"):-4] for p in GOLDENS]
SYNTH_SHAPES = {(1, 1), (3, 1), (5, 20), (2, 33), (3, 64), (1, 130), (1, 432)}
ERRORS = os.path.join(util.GOLD, "policy_head_errors.json")


def load(name):
    return np.load(os.path.join(util.GOLD, "policy_head_%s.npz" % name))


def golden_inputs(g, s):
    """(agents_attr f32 [B, A, 83], tree_embedding f32 [B, A, 128], valid u8 [B, A, 5]) of scale index s of a golden"""
    B, A = int(g["B"]), int(g["A"])
    if str(g["fixture"]):
        fx = util.load(str(g["fixture"]))
        attr, tree = np.ascontiguousarray(fx["o_attr"][list(g["obs_index"])]), g["tree"][s]
    else:
        attr, tree, valid = ph.synth_inputs(B, A, int(g["gen_seed"]))
        assert valid.tobytes() == g["valid"].tobytes()
        if g["attr"].size:
            assert attr.tobytes() == g["attr"].tobytes()            # the generator reproduces what the reference was fed
    assert attr.shape == (B, A, 83) and tree.shape == (B, A, 128)
    return torch.from_numpy(attr), torch.from_numpy(np.ascontiguousarray(tree)), torch.from_numpy(g["valid"])


def golden_params(g, s):
    return ph.seeded_params(int(g["seed"]), tuple(float(v) for v in g["scales"][s]),
                            [(str(n), tuple(int(v) for v in sh if v >= 0)) for n, sh in zip(g["param_names"], g["param_shapes"])])


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_binding_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    hb.build()                                                             # (the tests below call the library)
    names = [name for _, name, _ in cabi.declarations("flatland_policy.h")]
    assert names == list(hb.symbols("flatland_policy.h")) == ["fl_policy_head_workspace_bytes", "fl_policy_head"]
    hdr = open(os.path.join(cabi.INCLUDE, "flatland_policy.h")).read()
    assert hb.POLICY_HEAD_NPARAMS == len(ph.head_shapes()) and hb.POLICY_U_REFERENCE == ph.U_REFERENCE      # (both are the header's)
    assert np.random.RandomState(42).random_sample() == ph.U_REFERENCE
    # the header lists every parameter, in order, with its shape
    for i, (name, shape) in enumerate(ph.head_shapes()):
        if not name.startswith("transformer."):
            assert re.search(r"\b%d\s+%s %s" % (i, re.escape(name), re.escape("".join("[%d]" % v for v in shape))), hdr), (i, name)


FAKE = 0x10000      # 16-byte aligned, never dereferenced


def call(B=2, A=20, select=0, u=0.5, ws=None, null_param=None, bad_param=None, **ptrs):
    L = hb.lib()
    p = dict(attr=FAKE, tree=FAKE, valid=None, logits=FAKE, value=FAKE, actions=None, workspace=FAKE, params=True)
    p.update(ptrs)
    arr = (C.c_void_p * 38)(*[FAKE] * 38)
    if null_param is not None:
        arr[null_param] = None
    if bad_param is not None:
        arr[bad_param] = FAKE + 4
    need = L.fl_policy_head_workspace_bytes(max(B, 1), max(A, 1))
    rc = L.fl_policy_head(B, A, p["attr"], p["tree"], arr if p["params"] else None, p["valid"], select, u, p["logits"], p["value"],
                          p["actions"], p["workspace"], need if ws is None else ws, None)
    return rc, L.fl_last_error().decode()


def test_workspace_bytes():
    L = hb.lib()
    assert L.fl_policy_head_workspace_bytes(3, 20) == 3 * 20 * (7 * 256 + 1) * 4
    assert L.fl_policy_head_workspace_bytes(1, 1) == 7184                   # rounded up to 16 bytes
    assert L.fl_policy_head_workspace_bytes(0, 20) == 0 and L.fl_policy_head_workspace_bytes(3, 0) == 0


@pytest.mark.parametrize("kw, words", [
    (dict(B=0), "bad sizes"), (dict(B=-2), "bad sizes"), (dict(A=0), "bad sizes"), (dict(A=1025), "bad sizes"),
    (dict(attr=None), "attr is NULL"), (dict(tree=None), "tree is NULL"), (dict(params=False), "params is NULL"),
    (dict(null_param=0), "parameter 0 is NULL"), (dict(null_param=37), "parameter 37 is NULL"), (dict(logits=None), "logits is NULL"),
    (dict(workspace=None), "workspace is NULL"),
    (dict(attr=FAKE + 4), "attr is not 16-byte aligned"), (dict(tree=FAKE + 8), "tree is not 16-byte aligned"),
    (dict(logits=FAKE + 4), "logits is not 16-byte aligned"), (dict(value=FAKE + 4), "value is not 16-byte aligned"),
    (dict(bad_param=30), "parameter 30 is not 16-byte aligned"),
    (dict(select=3), "select must be"), (dict(select=-1), "select must be"),
    (dict(select=1, valid=None, actions=FAKE), "needs valid_actions"), (dict(select=2, valid=FAKE, actions=None), "needs valid_actions"),
    (dict(u=1.0), "u must be"), (dict(u=-0.1), "u must be"), (dict(u=float("nan")), "u must be"),
    (dict(ws=1000), "workspace of 1000 bytes"), (dict(A=1024, ws=2 * 1024 * 7172 - 16), "workspace"),
    (dict(B=3000, A=1024), "bad sizes"),        # 3 072 000 rows, above INT32_MAX / 768 = 2 796 202
])
def test_refusals(kw, words):
    rc, msg = call(**kw)
    assert rc == 1, (rc, msg)
    assert words in msg, msg


def test_a_good_call_passes_the_checks():
    """the same fake pointers with nothing wrong get past every check: without a GPU the first HIP call fails (FL_ERR_HIP)"""
    if hb.lib().fl_device_count() > 0:
        return
    for kw in (dict(), dict(value=None), dict(select=1, valid=FAKE, actions=FAKE, u=0.0), dict(A=1024), dict(A=1),
               dict(B=2730, A=1024)):        # 2 795 520 rows: the largest multiple of 1024 at or under INT32_MAX / 768
        rc, msg = call(**kw)
        assert rc == 2, (kw, rc, msg)


# ---------------------------------------------------------------------------------------------------------------- the module
def test_state_dict_matches_reference():
    from flatland_marl_amd.policy import HEAD_PARAM_ORDER, Network, TreeLSTM
    g = load("cfg2_uniform")
    ref = [(str(n), tuple(int(v) for v in s if v >= 0)) for n, s in zip(g["param_names"], g["param_shapes"])]
    assert len(ref) == 46 and ref == ph.TREE_SHAPES + ph.head_shapes()
    net = Network()
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == ref
    assert list(HEAD_PARAM_ORDER) == [n for n, _ in ref if not n.startswith("tree_lstm.")] and len(HEAD_PARAM_ORDER) == 38
    assert isinstance(net.tree_lstm, TreeLSTM) and isinstance(net.transformer[0].attention, torch.nn.MultiheadAttention)
    assert sum(v.numel() for v in net.state_dict().values()) * 4 > 6.5e6
    net.load_state_dict(golden_params(g, 1))                           # a reference state_dict loads unchanged
    m2 = Network.from_module(net)
    assert all(a is b for a, b in zip(net.parameters(), m2.parameters()))
    assert list(m2.state_dict()) == list(net.state_dict())


def test_forward_torch_is_the_reference_forward_on_the_cpu():
    """head_torch -- torch's own modules on the shared parameters -- gives the reference's float32 outputs within e32"""
    from flatland_marl_amd.policy import Network
    for name in ("cfg2_uniform", "synth_b2_a33", "synth_b3_a1"):
        g = load(name)
        for s in range(2):
            net = Network()
            net.load_state_dict(golden_params(g, s))
            attr, tree, _ = golden_inputs(g, s)
            (logits,), value = net.head_torch(attr, tree)
            assert logits.requires_grad and value.shape == (int(g["B"]),)
            tol = ph.tolerance(2 * g["e32_logits"][s], g["logits"][s])
            assert float((logits.detach() - torch.from_numpy(g["logits"][s])).abs().max()) <= tol
            assert float((value.detach() - torch.from_numpy(g["value"][s])).abs().max()) <= ph.tolerance(2 * g["e32_value"][s], g["value"][s])


# ---------------------------------------------------------------------------------------------------------------- the goldens
def test_goldens_present():
    assert set(NAMES) >= {"cfg1_uniform", "cfg2_uniform", "cfg3_uniform"}
    shapes = {(int(load(n)["B"]), int(load(n)["A"])) for n in NAMES if n.startswith("synth_")}
    assert shapes == SYNTH_SHAPES
    assert {int(load(n)["A"]) for n in NAMES if not n.startswith("synth_")} == {7, 20, 80}
    for p in GOLDENS:
        assert os.path.getsize(p) < 256 * 1024
        g = np.load(p)
        assert g["scales"].shape == (2, 2) and list(g["scales"][0]) == [1.0, 1.0] and g["scales"][1].min() > 2.0
        assert 2 <= len(g["obs_index"]) <= 3 or not str(g["fixture"])
        assert "weight" not in "".join(g.files)                      # the weights are regenerated, never stored


def test_synthetic_masks_exercise_the_choice():
    for n in NAMES:
        g = load(n)
        nv = g["valid"].reshape(-1, 5).astype(bool).sum(-1)
        if n.startswith("synth_") and int(g["A"]) >= 20:
            assert (nv == 0).mean() >= 0.2 and (nv == 1).mean() >= 0.2 and (nv >= 2).mean() >= 0.3
            assert (g["hard_raised"][0] == (nv == 0).reshape(g["hard_raised"][0].shape)).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load(name)
    for s in range(2):
        attr, tree, valid = golden_inputs(g, s)
        logits, value = ph.head(attr, tree, golden_params(g, s))
        el = float((logits - torch.from_numpy(g["logits"][s]).double()).abs().max())
        ev = float((value - torch.from_numpy(g["value"][s]).double()).abs().max())
        assert el <= ph.tolerance(g["e32_logits"][s], g["logits"][s]) and ev <= ph.tolerance(g["e32_value"][s], g["value"][s]), (el, ev)
        # float32 on the same restatement: the size of error the stored e32 stands for
        l32, v32 = ph.head(attr, tree, golden_params(g, s), dtype=torch.float32)
        assert float((l32.double() - logits).abs().max()) <= ph.tolerance(4 * g["e32_logits"][s], g["logits"][s])


@pytest.mark.parametrize("name", NAMES)
def test_restated_choice_matches_reference(name):
    g = load(name)
    for s in range(2):
        attr, tree, valid = golden_inputs(g, s)
        none = g["valid"].sum(-1) == 0
        assert (g["hard_raised"][s] == none).all() and (g["soft"][s][none] == 0).all() and (g["hard"][s][none] == 0).all()
        eps = ph.tolerance(g["e32_logits"][s], g["logits"][s])
        logits64, _ = ph.head(attr, tree, golden_params(g, s))
        for mode in ("soft", "hard"):
            # on the reference's own logits: the same action for every agent
            assert (ph.choose_actions(g["logits"][s], g["valid"], mode) == g[mode][s]).all()
            # on the restatement's logits: the same wherever eps of error cannot change it (at most 1 % may)
            ex = ph.exempt(g["logits"][s], g["valid"], mode, eps)
            assert ex.sum() <= 0.01 * ex.size
            got = ph.choose_actions(logits64.float(), g["valid"], mode)
            assert (got == g[mode][s])[~ex].all()


def test_choice_by_hand():
    lg = np.array([[0.0, 1.0, 2.0, 3.0, 4.0]] * 4, dtype=np.float32)
    va = np.array([[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [1, 1, 0, 0, 0]], dtype=np.uint8)
    assert ph.choose_actions(lg, va, "hard").tolist() == [4, 0, 2, 1]
    # p = softmax: cdf of row 0 = .0117 .0434 .1296 .3639 1 -> u = .3745 falls in the last; row 3: cdf = .2689 1 -> the second
    assert ph.choose_actions(lg, va, "soft").tolist() == [4, 0, 2, 1]
    assert ph.choose_actions(lg, va, "soft", u=0.2).tolist() == [3, 0, 2, 0]
    assert ph.choose_actions(lg, va, "soft", u=0.0).tolist() == [0, 0, 2, 0]
    assert ph.exempt(lg, va, "hard", 0.6).tolist() == [True, False, False, True]
    assert ph.exempt(lg, va, "soft", 0.002).tolist() == [True, False, False, False]      # |.3639 - .3745| <= 8 * .002


def test_R_follows_the_recorded_errors():
    from tests.test_gpu_policy_head import R
    rec = json.load(open(ERRORS))
    ratios = [c[k] for c in rec["cases"].values() for k in ("ratio_logits", "ratio_value")]
    assert R == math.ceil(2 * max(ratios)) and rec["R"] == R
    assert set(rec["cases"]) == {"%s-x%d" % (n, s) for n in NAMES for s in range(2)}
