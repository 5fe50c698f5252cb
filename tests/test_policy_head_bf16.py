"""CPU: include/flatland_policy_head_bf16.h against its ctypes table and the built library, the sizes and offsets it documents, the
refusals of fl_policy_head_bf16 and fl_policy_head_pack_bf16 (before any HIP call), the emulation the GPU tolerance rests on
(tests/policy_head_bf16_torch.py) against the float64 restatement, float32 emulations of the two a-priori bounded stages against
tests/policy_head_bf16_bounds.py, the head_precision switch of policy.Network, and the recorded errors
(tests/golden/policy_head_bf16_errors.json) against the GPU test's cases and its factor R16."""
import ctypes as C
import json
import os

import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import policy_head_bf16_bounds as pb16
from tests import policy_head_bf16_torch as ph16
from tests import policy_head_bounds as pb
from tests import policy_head_stages as phs
from tests import policy_head_torch as ph
from tests import test_gpu_policy_head_bf16 as gpu
from tests import util

NAMES = ["fl_policy_head_bf16_packed_bytes", "fl_policy_head_pack_bf16", "fl_policy_head_bf16_workspace_bytes", "fl_policy_head_bf16"]
HEADER = os.path.join(util.ROOT, "include", "flatland_policy_head_bf16.h")


def test_header_table_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    decls = cabi.declarations("flatland_policy_head_bf16.h")
    assert [name for _, name, _ in decls] == list(hb.symbols("flatland_policy_head_bf16.h")) == NAMES
    assert [r for r, _, _ in decls] == ["size_t", "int", "size_t", "int"]
    nargs = [len(p) for _, _, p in decls]
    assert nargs == [len(hb.ABI["flatland_policy_head_bf16.h"][n][0]) for n in NAMES] == [0, 4, 2, 16]
    assert nargs[3] == len(hb.ABI["flatland_policy.h"]["fl_policy_head"][0]) + 2     # fl_policy_head's, and packed / packed_bytes
    assert '#include "flatland_hip.h"' in cabi.text("flatland_policy_head_bf16.h")
    hb.build()
    fn = hb.lib().fl_policy_head_bf16
    assert len(fn.argtypes) == 16 and fn.restype is C.c_int and hb.lib().fl_policy_head_bf16_packed_bytes.restype is C.c_size_t
    assert callable(hb.policy_head_pack_bf16) and callable(hb.policy_head_bf16)


def _spaced(n):
    return "{:,}".format(n).replace(",", " ")


def test_sizes_and_offsets_are_the_documented_ones():
    L = hb.lib()
    shapes = ph.head_shapes()
    names = [shapes[i][0] for i in hb.POLICY_HEAD_BF16_MATRICES]
    # the 16: every weight matrix but attr_embedding.0 and the heads' last layers, in state_dict order
    assert names == [n for n, s in shapes if len(s) == 2 and n not in ("attr_embedding.0.weight", "actor_net.4.weight", "critic_net.4.weight")]
    assert hb.POLICY_HEAD_BF16_MATRICES == gpu.MATRICES
    sizes = [shapes[i][1][0] * shapes[i][1][1] for i in hb.POLICY_HEAD_BF16_MATRICES]
    assert all(shapes[i][1][0] % 32 == 0 and shapes[i][1][1] in ph16.BF16_K for i in hb.POLICY_HEAD_BF16_MATRICES)
    macs = [s[0] * s[1] for _, s in shapes if len(s) == 2]
    assert abs(sum(sizes) / sum(macs) - 0.987) < 0.0005                              # 98.7 % of the head's multiply-adds
    offsets = [sum(sizes[:k]) for k in range(17)]
    assert L.fl_policy_head_bf16_packed_bytes() == 2 * offsets[16] == 3342336 == gpu.PACKED_BYTES
    assert offsets == [0, 65536, 131072, 163840, 360448, 425984, 557056, 753664, 819200, 950272, 1146880, 1212416, 1343488, 1474560,
                       1507328, 1638400, 1671168]
    doc = " ".join(open(HEADER).read().split())
    for n, off in zip(names, offsets):
        if n.startswith("transformer."):
            blk, rest = int(n.split(".")[1]), n.split(".", 2)[2]
            rel = off - (163840 + 393216 * blk)
            assert rel == {"attention.in_proj_weight": 0, "attention.out_proj.weight": 196608, "att_mlp.0.weight": 262144}[rest]
            assert "%s %s +%s" % (rest, "".join("[%d]" % v for v in dict(shapes)[n]), _spaced(rel)) in doc, n
        else:
            assert "%s %s %s" % (n, "".join("[%d]" % v for v in dict(shapes)[n]), _spaced(off)) in doc, n
    assert "163 840 + 393 216 i" in doc and "3 342 336 bytes" in doc and "end: 1 671 168" in doc
    assert L.fl_policy_head_bf16_workspace_bytes(3, 11) == (33 * 5636 + 15) // 16 * 16 == 186000 and 33 * 5636 % 16 != 0
    assert L.fl_policy_head_bf16_workspace_bytes(1, 1) == 5648
    assert L.fl_policy_head_bf16_workspace_bytes(0, 20) == 0 and L.fl_policy_head_bf16_workspace_bytes(3, 0) == 0
    assert "byte 4096 R" in doc and "byte 5632 R" in doc and gpu.ROW_BYTES == 5636


FAKE = 0x10000      # 16-byte aligned, never dereferenced


def call(B=2, A=20, select=0, u=0.5, ws=None, pk=3342336, null_param=None, bad_param=None, **ptrs):
    L = hb.lib()
    p = dict(attr=FAKE, tree=FAKE, valid=None, logits=FAKE, value=FAKE, actions=None, workspace=FAKE, packed=FAKE, params=True)
    p.update(ptrs)
    arr = (C.c_void_p * 38)(*[FAKE] * 38)
    if null_param is not None:
        arr[null_param] = None
    if bad_param is not None:
        arr[bad_param] = FAKE + 4
    need = L.fl_policy_head_bf16_workspace_bytes(max(B, 1), max(A, 1))
    rc = L.fl_policy_head_bf16(B, A, p["attr"], p["tree"], arr if p["params"] else None, p["packed"], pk, p["valid"], select, u,
                               p["logits"], p["value"], p["actions"], p["workspace"], need if ws is None else ws, None)
    return rc, L.fl_last_error().decode()


@pytest.mark.parametrize("kw, words", [
    # fl_policy_head's (tests/test_policy_head_golden.py)
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
    (dict(ws=1000), "workspace of 1000 bytes"), (dict(A=1024, ws=2 * 1024 * 5636 - 16), "workspace"),
    (dict(B=3000, A=1024), "bad sizes"),
    # its own
    (dict(packed=None), "packed is NULL"), (dict(packed=FAKE + 8), "packed is not 16-byte aligned"),
    (dict(pk=3342335), "packed buffer of 3342335 bytes"), (dict(pk=0), "packed buffer"),
])
def test_refusals(kw, words):
    rc, msg = call(**kw)
    assert rc == 1, (rc, msg)
    assert words in msg and msg.startswith("fl_policy_head_bf16:"), msg


def test_a_good_call_passes_the_checks():
    """the same fake pointers with nothing wrong get past every check: without a GPU the first HIP call fails (FL_ERR_HIP)"""
    if hb.lib().fl_device_count() > 0:
        return
    for kw in (dict(), dict(value=None), dict(select=1, valid=FAKE, actions=FAKE, u=0.0), dict(A=1024), dict(A=1)):
        rc, msg = call(**kw)
        assert rc == 2, (kw, rc, msg)


def test_pack_refusals():
    L = hb.lib()

    def pack(params=True, null_param=None, bad_param=None, packed=FAKE, pk=3342336):
        arr = (C.c_void_p * 38)(*[FAKE] * 38)
        if null_param is not None:
            arr[null_param] = None
        if bad_param is not None:
            arr[bad_param] = FAKE + 4
        return L.fl_policy_head_pack_bf16(arr if params else None, packed, pk, None), L.fl_last_error().decode()
    cases = [(dict(params=False), "params is NULL"), (dict(packed=None), "packed is NULL"),
             (dict(packed=FAKE + 8), "packed is not 16-byte aligned"), (dict(pk=3342335), "packed buffer of 3342335 bytes")]
    for i in hb.POLICY_HEAD_BF16_MATRICES:
        cases += [(dict(null_param=i), "parameter %d is NULL" % i), (dict(bad_param=i), "parameter %d is not 16-byte aligned" % i)]
    for kw, words in cases:
        rc, msg = pack(**kw)
        assert rc == 1 and words in msg and msg.startswith("fl_policy_head_pack_bf16:"), (kw, rc, msg)
    if L.fl_device_count() == 0:
        # a parameter the pack does not read may be anything; then the first HIP call fails
        assert pack(null_param=0)[0] == 2 and pack(bad_param=30)[0] == 2


@pytest.mark.parametrize("case", ["b3_a11-x0", "b2_a33-x1", "b1_a65-x1", "b70_a1-x0"])
def test_emulation_without_rounding_is_the_restatement(case):
    attr, tree, _, params = phs.CASES[case]()
    l64, v64 = ph.head(attr, tree, params)
    l, v = ph16.head(attr, tree, params, rounding=False)
    assert torch.equal(l, l64) and torch.equal(v, v64)
    ref, st = ph.stages(attr, tree, params), ph16.stages(attr, tree, params, rounding=False)
    assert set(ref) == set(st) and all(torch.equal(ref[k], st[k]) for k in ref)
    # ... and with it: bf16 has 8 bits, so the error is far above float32's 1e-7 and far below the values
    l16, v16 = ph16.head(attr, tree, params)
    err = float((l16 - l64).abs().max())
    assert 1e-5 < err < 0.05 * float(l64.abs().max()) + 0.05, err
    st16 = ph16.stages(attr, tree, params)
    assert torch.equal(st16["qkv"], ph16.rb(st16["qkv"])) and torch.equal(st16["emb"][..., 128:], tree.double())


def test_only_the_16_products_are_rounded():
    """the hook rounds by K: 256 and 512 are the 16 matrices, 83 (attr_embedding.0) and 128 (the heads' last layers) stay exact"""
    g = torch.Generator().manual_seed(3)
    for K, rounded in ((83, False), (128, False), (256, True), (512, True)):
        a, b = torch.randn(5, K, generator=g, dtype=torch.float64), torch.randn(K, 7, generator=g, dtype=torch.float64)
        assert torch.equal(ph16.mm16(a, b), a @ b) != rounded
        assert torch.equal(ph16.mm16(a, b), ph16.rb(a) @ ph16.rb(b)) == rounded
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    assert ph16.rb(x).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7]      # ties to even, both ways; above a tie: up


SMALL = [c for c in gpu.SHAPE_CASES if int(c.split("_a")[1].split("-")[0]) <= 65]


@pytest.mark.parametrize("case", SMALL)
def test_float32_emulations_stay_inside_the_bounds(case):
    """qkv from xb and ao from the stored qkv as the kernel computes them -- rounded operands, float32 sums in two orders, the
    result rounded -- inside tests/policy_head_bf16_bounds.py"""
    attr, tree, _, params = phs.CASES[case]()
    p64 = ph.stage_params(params, "cpu")
    c = pb.allowance()
    xb = ph16.stages(attr, tree, params)["xb"].float()                       # a float32 xb, as the kernel leaves one
    ref, bound = pb16.qkv(xb.double(), p64, 2)
    W = ph16.rb(params[phs.IN_PROJ + "weight"].float())
    b = params[phs.IN_PROJ + "bias"].float()
    stored = None
    for mm in (torch.matmul, ph.matmul_seq):
        stored = (mm(ph16.rb(xb), W.T) + b).to(torch.bfloat16)
        w = phs.worst(stored.double(), ref, bound)
        assert 0 < w <= 1.0, (case, mm.__name__, w)
    ref, bound = pb16.attention(stored.double(), c)
    ao = ph16.attention(stored, dtype=torch.float32)
    assert ao.dtype == torch.float32
    w = phs.worst(ao.double(), ref, bound)
    assert w <= 1.0, (case, w)
    # the bound is the size of the rounding it allows for, not a multiple of the values
    assert float((bound / (ref.abs() + 1e-3)).median()) < 0.05


def test_head_precision_switch():
    from flatland_marl_amd.policy import Network
    net = Network(head_precision="bf16")
    assert net.head_precision == "bf16" and net.tree_lstm.precision == "f32" and Network().head_precision == "f32"
    assert Network(precision="bf16").head_precision == "f32"                         # precision stays the encoder's
    full = Network(precision="bf16", head_precision="bf16")
    assert full.tree_lstm.precision == "bf16" and full.head_precision == "bf16"
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match="head_precision"):
            Network(head_precision=bad)
        if bad is not None:                                   # (None there: the module's own)
            with pytest.raises(ValueError, match="head_precision"):
                Network.from_module(net, head_precision=bad)
    params = ph.seeded_params(3, 3.0)
    net.load_state_dict(params)                               # a reference state dict: the packed weights are no part of it
    assert list(net.state_dict()) == list(params)
    assert Network.from_module(net).head_precision == "bf16"
    assert Network.from_module(net, head_precision="f32").head_precision == "f32"
    assert Network.from_module(Network(), head_precision="bf16").head_precision == "bf16"
    assert Network.from_module(Network()).head_precision == "f32"
    assert Network.from_module(full).tree_lstm.precision == "bf16" and Network.from_module(full).head_precision == "bf16"
    assert all(a is b for a, b in zip(net.parameters(), Network.from_module(net).parameters()))


def test_bf16_head_with_trainable_raises_under_grad_mode_before_any_input_check():
    from flatland_marl_amd.policy import Network
    attr, tree, _ = phs.inputs(3, 11)                         # CPU tensors: every input check would refuse them with TypeError
    net = Network(trainable=True, head_precision="bf16")
    with pytest.raises(ValueError, match="inference only"):
        net.head(attr, tree)
    with torch.no_grad(), pytest.raises(TypeError):           # no_grad: past that check, on to the inputs'
        net.head(attr, tree)
    net.trainable = False
    with pytest.raises(TypeError):
        net.head(attr, tree)
    net.head_precision = "f64"                                # a plain attribute: a bad value is found at the next call
    with pytest.raises(ValueError, match="head_precision"):
        net.head(attr, tree)


def test_recorded_errors_are_consistent():
    rec = json.load(open(gpu.ERRORS))
    assert gpu.R16 == 2 and rec["R16"] == 2
    assert set(rec["cases"]) == set(gpu.IDS) and len(gpu.IDS) == len(set(gpu.IDS))
    for name, c in rec["cases"].items():
        if name.startswith("obs-"):
            assert 0 <= c["hard_actions_differ"] <= c["agents"] and c["max_dlogit"] > 0
            continue
        stages = ("logits", "value") if name.startswith("fixture-") else gpu.RATIO_STAGES
        for s in stages:
            assert c["ratio_" + s] == c["err_" + s] / c["e16_" + s] and c["ratio_" + s] <= gpu.R16, (name, s, c)
        if not name.startswith("fixture-"):
            assert 0 < c["qkv_bound"] <= 1 and 0 <= c["ao_bound"] <= 1
