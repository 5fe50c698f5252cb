"""CPU: what the trainable policy head rests on.  The differentiable restatement (tests/policy_head_grad_torch.py) against the
reference Network's own float64 autograd (tests/golden/grad_policy_head_*.npz, tools/capture_policy_head_grads.py); the C-ABI of
include/flatland_policy_train.h: header, ctypes table and library agree, the byte functions, every refusal; the trainable switch
of policy.Network; the parameter products from hand-made rows; the chunking arithmetic."""
import glob
import os

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import policy_head_grad_torch as pg
from tests import policy_head_torch as ph
from tests import util
from tests.test_policy_head_golden import golden_inputs, golden_params, load

MODES = ("logits", "value", "both")
R_SEED, PROBE_SEED, K = 20261019, 20261020, 2
ORDER = pg.NAMES + ["tree"]
FILES = sorted(os.path.basename(p)[len("grad_policy_head_"):-len(".npz")] for p in glob.glob(os.path.join(util.GOLD, "grad_policy_head_*.npz")))
REQUIRED = {"cfg1_uniform", "cfg2_uniform", "cfg3_uniform", "synth_b1_a1", "synth_b3_a1", "synth_b5_a20", "synth_b2_a33", "synth_b3_a64",
            "synth_b1_a130"}
# float32 autograd of the restatement against its float64: a sanity bound, not a tolerance.  Unit roundoff 6e-8 through some twenty
# layers and three softmaxes of a network without normalisation; a wrong formula or a missing path is an error of order 1.
SANITY_32 = 1e-3


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_the_fixtures_are_the_ones_the_issue_lists():
    assert {f[:-3] for f in FILES} >= REQUIRED and all(f.endswith(("_x0", "_x1")) for f in FILES)
    for f in FILES:
        assert os.path.getsize(os.path.join(util.GOLD, "grad_policy_head_%s.npz" % f)) < 1024 * 1024


def test_the_restatement_in_float64_is_head_bit_for_bit():
    g = load("synth_b2_a33")
    attr, tree, _ = golden_inputs(g, 1)
    params = golden_params(g, 1)
    p = {k: params[k].double() for k in pg.NAMES}
    logits, value = pg.forward(attr, tree, p)
    l64, v64 = ph.head(attr, tree, params)
    assert torch.equal(logits, l64) and torch.equal(value, v64)


@pytest.mark.parametrize("name", FILES)
def test_restatement_gradients_match_the_reference(name):
    """every array of a fixture, in every mode, within 1e-12 of its max-abs; the float32 autograd within the sanity bound"""
    fx = np.load(os.path.join(util.GOLD, "grad_policy_head_%s.npz" % name))
    s = int(fx["scale_index"])
    assert list(fx["modes"]) == list(MODES) and int(fx["r_seed"]) == R_SEED and int(fx["probe_seed"]) == PROBE_SEED
    g = load(str(fx["name"]))
    attr, tree, _ = golden_inputs(g, s)
    params = golden_params(g, s)
    B, A = attr.shape[:2]
    rng = np.random.default_rng([R_SEED, s])
    Rl, Rv = torch.from_numpy(rng.standard_normal((B, A, 5))), torch.from_numpy(rng.standard_normal((B,)))
    torch.set_num_threads(1)
    for m, mode in enumerate(MODES):
        rl, rv = (Rl if mode != "value" else None), (Rv if mode != "logits" else None)
        g64 = pg.grads(attr, tree, params, rl, rv)
        g64["tree"] = g64["tree"].reshape(B * A, 128)
        for i, k in enumerate(ORDER):
            key, got = k.replace(".", "_"), g64[k].numpy()

            def close(a, b):
                assert a.shape == b.shape, (name, mode, k)
                assert np.abs(a - b).max(initial=0) <= 1e-12 * np.abs(b).max(initial=0), (name, mode, k)
            if "whole_" + key in fx:
                close(got, fx["whole_" + key][m])
            else:
                prng = np.random.default_rng([PROBE_SEED, i])
                v = prng.standard_normal((got.shape[1], K))
                u = prng.standard_normal((K, got.shape[0]))
                close(got @ v, fx["right_" + key][m])
                close(u @ got, fx["left_" + key][m])
                close(np.array(np.abs(got).max()), fx["maxabs_" + key][m])
                assert abs(got.sum() - fx["sum_" + key][m]) <= 1e-12 * max(np.abs(got).sum(), 1e-300), (name, mode, k)
        if mode == "both":
            g32 = pg.grads(attr, tree, params, None if rl is None else rl.float(), None if rv is None else rv.float(), torch.float32)
            g32["tree"] = g32["tree"].reshape(B * A, 128)
            worst = max(pg.rel_error(g32[k], g64[k]) for k in ORDER)
            print(name, "float32 autograd: largest relative error %.3g" % worst)
            assert worst <= SANITY_32, (name, worst)


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_binding_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    hb.build()                                                             # (the tests below call the library)
    decls = cabi.declarations("flatland_policy_train.h")
    assert [n for _, n, _ in decls] == list(hb.symbols("flatland_policy_train.h")) == [
        "fl_policy_head_saved_bytes", "fl_policy_head_forward_saved", "fl_policy_head_backward_rows_bytes",
        "fl_policy_head_backward_workspace_bytes", "fl_policy_head_backward"]
    assert '#include "flatland_policy.h"' in cabi.text("flatland_policy_train.h")
    params = {n: ps for _, n, ps in decls}
    assert params["fl_policy_head_backward"] == [
        "int n_envs", "int n_agents", "const float *attr_dev", "const float *tree_dev", "const float *const *params",
        "const void *saved_dev", "const float *grad_logits_dev", "const float *grad_value_dev", "float *grad_tree_dev", "void *rows_dev",
        "size_t rows_bytes", "void *workspace_dev", "size_t workspace_bytes", "void *hip_stream"]
    assert params["fl_policy_head_forward_saved"] == [
        "int n_envs", "int n_agents", "const float *attr_dev", "const float *tree_dev", "const float *const *params", "float *logits_dev",
        "float *value_dev", "void *saved_dev", "size_t saved_bytes", "void *hip_stream"]
    assert callable(hb.policy_head_forward_saved) and callable(hb.policy_head_backward)


BYTES = ("fl_policy_head_saved_bytes", "fl_policy_head_backward_rows_bytes", "fl_policy_head_backward_workspace_bytes")


def test_byte_functions():
    for name, per_row in zip(BYTES, (4097 * 4, 9612 * 4, 48)):
        fn = hb._sym(name)
        for B, A in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
            assert fn(B, A) == 0, (name, B, A)
        for B, A in ((1, 1), (3, 11), (256, 20), (1024, 80), (1, 1024)):
            n = fn(B, A)
            assert B * A * per_row <= n < B * A * per_row + 16 and n % 16 == 0, (name, B, A)
            assert fn(B + 1, A) > n and fn(B, A + 1) > n, (name, B, A)


def _backward_args(**over):
    """a good call's arguments with fake 16-byte-aligned addresses (never dereferenced: every refusal comes before any HIP call)"""
    B, A = over.pop("B", 3), over.pop("A", 11)
    ptrs = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[0x20000 + 16 * i for i in range(hb.POLICY_HEAD_NPARAMS)])
    a = dict(B=B, A=A, attr=0x10000, tree=0x10010, params=ptrs, saved=0x10020, gl=0x10030, gv=0x10040, gtree=0x10050, rows=0x10060,
             rows_bytes=hb._sym("fl_policy_head_backward_rows_bytes")(max(B, 0), max(A, 0)), ws=0x10070,
             ws_bytes=hb._sym("fl_policy_head_backward_workspace_bytes")(max(B, 0), max(A, 0)), stream=None)
    a.update(over)
    return [a[k] for k in ("B", "A", "attr", "tree", "params", "saved", "gl", "gv", "gtree", "rows", "rows_bytes", "ws", "ws_bytes", "stream")]


def _forward_args(**over):
    B, A = over.pop("B", 3), over.pop("A", 11)
    ptrs = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[0x20000 + 16 * i for i in range(hb.POLICY_HEAD_NPARAMS)])
    a = dict(B=B, A=A, attr=0x10000, tree=0x10010, params=ptrs, logits=0x10020, value=0x10030, saved=0x10040,
             saved_bytes=hb._sym("fl_policy_head_saved_bytes")(max(B, 0), max(A, 0)), stream=None)
    a.update(over)
    return [a[k] for k in ("B", "A", "attr", "tree", "params", "logits", "value", "saved", "saved_bytes", "stream")]


def _null_param(i):
    p = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[0x20000 + 16 * j for j in range(hb.POLICY_HEAD_NPARAMS)])
    p[i] = None
    return p


def _odd_param(i):
    p = (hb.vp * hb.POLICY_HEAD_NPARAMS)(*[0x20000 + 16 * j for j in range(hb.POLICY_HEAD_NPARAMS)])
    p[i] = 0x20004
    return p


BACKWARD_REFUSALS = [
    (dict(B=0), "bad sizes"), (dict(A=0), "bad sizes"), (dict(A=1025), "bad sizes"), (dict(B=-2), "bad sizes"),
    (dict(params=None), "params is NULL"), (dict(attr=None), "attr is NULL"), (dict(tree=None), "tree is NULL"),
    (dict(saved=None), "saved is NULL"), (dict(gtree=None), "grad_tree is NULL"), (dict(rows=None), "rows is NULL"),
    (dict(ws=None), "workspace is NULL"), (dict(gl=None, gv=None), "grad_logits and grad_value are both NULL"),
    (dict(attr=0x10004), "attr is not 16-byte aligned"), (dict(tree=0x10008), "tree is not 16-byte aligned"),
    (dict(saved=0x10024), "saved is not 16-byte aligned"), (dict(gtree=0x10054), "grad_tree is not 16-byte aligned"),
    (dict(rows=0x10064), "rows is not 16-byte aligned"), (dict(ws=0x10074), "workspace is not 16-byte aligned"),
    (dict(gl=0x10034), "grad_logits is not 16-byte aligned"), (dict(gv=0x10044), "grad_value is not 16-byte aligned"),
    (dict(params=_null_param(17)), "parameter 17 is NULL"), (dict(params=_odd_param(37)), "parameter 37 is not 16-byte aligned"),
    (dict(rows_bytes=3 * 11 * 9612 * 4 - 1), "rows of 1268783 bytes, 1268784 needed"),
    (dict(ws_bytes=3 * 11 * 48 - 16), "workspace of 1568 bytes, 1584 needed"),
]
FORWARD_REFUSALS = [
    (dict(B=0), "bad sizes"), (dict(A=1025), "bad sizes"), (dict(params=None), "params is NULL"), (dict(attr=None), "attr is NULL"),
    (dict(tree=None), "tree is NULL"), (dict(logits=None), "logits is NULL"), (dict(saved=None), "saved is NULL"),
    (dict(logits=0x10024), "logits is not 16-byte aligned"), (dict(value=0x10034), "value is not 16-byte aligned"),
    (dict(saved=0x10048), "saved is not 16-byte aligned"), (dict(params=_null_param(0)), "parameter 0 is NULL"),
    (dict(saved_bytes=540815), "saved buffer of 540815 bytes, 540816 needed"),
]


@pytest.mark.parametrize("over,message", BACKWARD_REFUSALS, ids=[m for _, m in BACKWARD_REFUSALS])
def test_backward_refusals(over, message):
    """FL_ERR_ARG with its message, before any HIP call: the pointers are fake"""
    rc = hb._sym("fl_policy_head_backward")(*_backward_args(**over))
    assert rc == 1, rc                                  # FL_ERR_ARG
    msg = hb.lib().fl_last_error().decode()
    assert msg.startswith("fl_policy_head_backward: ") and message in msg, msg


@pytest.mark.parametrize("over,message", FORWARD_REFUSALS, ids=[m for _, m in FORWARD_REFUSALS])
def test_forward_saved_refusals(over, message):
    rc = hb._sym("fl_policy_head_forward_saved")(*_forward_args(**over))
    assert rc == 1, rc                                  # FL_ERR_ARG
    msg = hb.lib().fl_last_error().decode()
    assert msg.startswith("fl_policy_head_forward_saved: ") and message in msg, msg


# ---------------------------------------------------------------------------------------------------------------- the switch
def test_trainable_switch():
    from flatland_marl_amd.policy import Network
    net = Network()
    assert net.trainable is False and Network(trainable=True).trainable is True
    other = Network.from_module(net, trainable=True)
    assert other.trainable is True and Network.from_module(net).trainable is False
    assert list(other.state_dict()) == list(net.state_dict()) and len(net.state_dict()) == 46
    assert all(a is b for a, b in zip(other.parameters(), net.parameters()))
    other.trainable = False
    assert list(other.state_dict()) == list(net.state_dict())


# ---------------------------------------------------------------------------------------------------------------- the products
def _hand_rows(R, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(R * hb.POLICY_ROW_FLOATS, generator=g)
    saved = torch.randn(R * hb.POLICY_SAVED_FLOATS, generator=g)
    attr = torch.randn(R, 83, generator=g)
    return attr, hb.policy_views(saved, hb.POLICY_SAVED_LAYOUT, R), hb.policy_views(rows, hb.POLICY_ROWS_LAYOUT, R)


def _expected(attr, sv, rw):
    """the sums include/flatland_policy_train.h lists, in float64"""
    d = lambda t: t.double()  # noqa: E731
    out = []
    for dz, x in (("attr.dz0", d(attr)), ("attr.dz2", d(rw["attr.h1"])), ("attr.dz4", d(rw["attr.h2"])), ("attr.dz6", d(rw["attr.h3"]))):
        out += [d(rw[dz]).T @ x, d(rw[dz]).sum(0)]
    for i, y in enumerate(("emb", "y1", "y2")):
        out += [d(rw["dqkv%d" % i]).T @ d(sv[y]), d(rw["dqkv%d" % i]).sum(0), d(rw["do%d" % i]).T @ d(sv["c%d" % i]), d(rw["do%d" % i]).sum(0),
                d(rw["dz%d" % i]).T @ torch.cat([d(sv[y]), d(rw["o%d" % i])], 1), d(rw["dz%d" % i]).sum(0)]
    for h, n in (("actor", 5), ("critic", 1)):
        out += [d(rw[h + ".dz0"]).T @ torch.cat([d(sv["emb"]), d(sv["y3"])], 1), d(rw[h + ".dz0"]).sum(0),
                d(rw[h + ".dz2"]).T @ d(rw[h + ".u1"]), d(rw[h + ".dz2"]).sum(0),
                d(rw[h + ".dz4"][:, :n]).T @ d(rw[h + ".u2"]), d(rw[h + ".dz4"][:, :n]).sum(0)]
    return out


def _abs(attr, sv, rw):
    return attr.abs(), {k: v.abs() for k, v in sv.items()}, {k: v.abs() for k, v in rw.items()}


def _bound(policy, S):
    """a float32 product over at most REDUCE_BLOCK rows is within REDUCE_BLOCK u of the sum S of its |terms| in any order (u = 2^-24);
    the float64 sum of the blocks adds nothing at this size; the result is rounded to float32 once more: (REDUCE_BLOCK + 1) u S"""
    return (policy.REDUCE_BLOCK + 1) * 2.0 ** -24 * S


@pytest.mark.parametrize("R", (1, 37, 256, 700))
def test_parameter_products_from_hand_made_rows(R):
    """the 38 sums from random rows, at row counts below, at and not a multiple of REDUCE_BLOCK; the shapes are the parameters'"""
    from flatland_marl_amd import policy
    attr, sv, rw = _hand_rows(R, 3)
    got, want, S = policy.policy_head_param_grads(attr, sv, rw), _expected(attr, sv, rw), _expected(*_abs(attr, sv, rw))
    shapes = dict(zip(policy.HEAD_PARAM_ORDER, hb.POLICY_HEAD_PARAM_SHAPES))
    assert len(got) == 38
    for name, g, w, s in zip(policy.HEAD_PARAM_ORDER, got, want, S):
        assert tuple(g.shape) == shapes[name] and g.dtype == torch.float32, name
        assert bool(((g.double() - w).abs() <= _bound(policy, s)).all()), name
    off = policy.policy_head_param_grads(attr, sv, rw, actor=False, critic=True)
    assert all(g is None for g in off[26:32]) and all(g is not None for g in off[:26] + off[32:])
    off = policy.policy_head_param_grads(attr, sv, rw, actor=True, critic=False)
    assert all(g is None for g in off[32:]) and all(g is not None for g in off[:32])


def test_two_chunks_are_added_in_order():
    from flatland_marl_amd import policy
    # what _HeadTrain.backward does with two chunks: the second chunk's gradients added to the first's = the sums over all rows
    # (one more float32 rounding of the total)
    a, b = _hand_rows(300, 4), _hand_rows(41, 5)
    ga, gb = policy.policy_head_param_grads(*a), policy.policy_head_param_grads(*b)
    wa, wb, sa, sb = _expected(*a), _expected(*b), _expected(*_abs(*a)), _expected(*_abs(*b))
    for x, y, u, v, s, t in zip(ga, gb, wa, wb, sa, sb):
        assert bool((((x + y).double() - (u + v)).abs() <= _bound(policy, s + t) + 2.0 ** -24 * (u + v).abs()).all())


@pytest.mark.parametrize("A", (1, 13, 1024))
@pytest.mark.parametrize("rows", (1, 29, 8192))
def test_chunks_cover_whole_envs_once(monkeypatch, A, rows):
    from flatland_marl_amd import policy
    monkeypatch.setattr(policy, "HEAD_BACKWARD_CHUNK_ROWS", rows)
    for B in (1, 2, 7, 100):
        chunks = policy.head_chunks(B, A)
        assert chunks[0][0] == 0 and chunks[-1][1] == B
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(e0 < e1 for e0, e1 in chunks)
        per = max(1, rows // A)
        assert all(e1 - e0 <= per for e0, e1 in chunks) and all(e1 - e0 == per for e0, e1 in chunks[:-1])
        assert all((e1 - e0) * A <= rows or e1 - e0 == 1 for e0, e1 in chunks)
