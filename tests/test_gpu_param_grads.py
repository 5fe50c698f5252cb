"""GPU: fl_policy_head_param_grads and fl_tree_lstm_param_grads (include/flatland_param_grads.h) -- first the products alone on
constructed rows against float64 matrix products of the very buffers the kernel read, inside the a-priori bound of
tests/param_grads_np.py; then the refusals; then through policy.Network / policy.TreeLSTM with param_grads="hip" against the
float64 autograd of the restatements, with the measures and the R of tests/test_gpu_policy_head_backward.py (6) and
tests/test_gpu_tree_lstm_backward.py (5); then the other switches under "hip".

The oracle of dW_f and db_f takes dgs = (dg_1 + dg_2) + dg_3 in float32, as the header states it, then float64.

PARAM_GRADS_ERRORS=<path> makes the product cases write the largest observed fraction of the bound per matrix to <path> in the
format of tests/golden/param_grads_errors.json (a record; nothing is asserted against it).
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import param_grads_np as pn
from tests import policy_head_grad_torch as pg
from tests import policy_head_stages as st
from tests import test_gpu_policy_head_backward as hbw
from tests import test_gpu_tree_lstm_backward as tbw
from tests import tree_lstm_grad_torch as tg
from tests import tree_lstm_torch as tl
from tests import util

DEV = "cuda:0"
GUARD = 4096
CAP = hb.PARAM_GRADS_MAX_SLICES
ERRORS = os.path.join(util.GOLD, "param_grads_errors.json")
HEAD_SHAPES = {1: (1, 1), 31: (1, 31), 33: (1, 33), 255: (1, 255), 256: (2, 128), 257: (1, 257), 513: (3, 171), 1025: (5, 205)}
ROWS = tuple(HEAD_SHAPES)
CASES = [(n, 0) for n in ROWS] + [(n, s) for n in (513, 1025) for s in (1, 2, 3, CAP)]
HEAD_NAMES = list(pg.NAMES)
TREE_NAMES = list(tg.PARAM_ORDER)


def test_the_record_names_every_matrix():
    rec = json.load(open(ERRORS))
    assert set(rec["head"]) == set(HEAD_NAMES) and set(rec["tree"]) == set(TREE_NAMES)
    assert all(v >= 0 for part in ("head", "tree") for v in rec[part].values())


def test_head_shapes_are_the_issue_s():
    assert all(B * A == n for n, (B, A) in HEAD_SHAPES.items())
    from flatland_marl_amd import policy
    assert HEAD_NAMES == list(policy.HEAD_PARAM_ORDER) and TREE_NAMES == list(policy.PARAM_ORDER)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _guarded(nbytes):
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    buf[:nbytes].fill_(0xFF)
    buf[nbytes:].fill_(0xA5)
    return buf


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _outputs(shapes, on):
    """a guarded 0xFF buffer per gradient (None where off): [(buffer, float view)]"""
    out = []
    for s, k in zip(shapes, on):
        if not k:
            out.append(None)
            continue
        n = 1
        for d in s:
            n *= d
        buf = _guarded(4 * n)
        out.append((buf, buf[:4 * n].view(torch.float32).view(s)))
    return out


def _raw(name, rows, shapes, on, slices, args, ws_bytes=None):
    """fl_<name>(*args, grads, slices, workspace, bytes, stream) on torch's current stream with guarded outputs and workspace;
    returns (rc, outputs, workspace buffer, its bytes)"""
    outs = _outputs(shapes, on)
    need = hb._sym("fl_%s_workspace_bytes" % name)(rows, slices) if ws_bytes is None else ws_bytes
    ws = _guarded(need)
    ptrs = (hb.vp * len(shapes))(*[None if o is None else o[1].data_ptr() for o in outs])
    with torch.cuda.device(DEV):
        rc = hb._sym("fl_" + name)(*args, ptrs, slices, ws.data_ptr(), need, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    return rc, outs, ws, need


def _check_buffers(outs, ws, need):
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            buf, view = o
            assert bool((buf[view.numel() * 4:] == 0xA5).all()), "a guard was written"
            assert not bool(torch.isnan(view).any()), "an output float was left unwritten"
    assert bool((ws[need:] == 0xA5).all()), "the workspace's guard was written"


_worst = {"head": {}, "tree": {}}


def _note(part, name, frac):
    _worst[part][name] = max(_worst[part].get(name, 0.0), frac)
    path = os.environ.get("PARAM_GRADS_ERRORS")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else dict(device=torch.cuda.get_device_name(0), head={}, tree={})
        rec[part][name] = max(rec[part].get(name, 0.0), frac)
        json.dump(rec, open(path, "w"), indent=1, sort_keys=True)


def _hold(part, names, got, problems, what):
    """every gradient inside its bound; problems: name -> (dz64, x64 or None for a bias)"""
    for name, g in zip(names, got):
        if g is None:
            continue
        dz, x = problems[name]
        if x is None:
            g64 = dz.sum(0)
            bound = pn.bias_bound(dz, g64)
        else:
            g64 = dz.T @ x
            bound = pn.weight_bound(dz, x, g64)
        assert g.shape == g64.shape, (what, name)
        frac = pn.fraction(g.double(), g64, bound)
        _note(part, name, frac)
        print(what, name, "fraction of the bound %.4f" % frac)
        assert frac <= 1.0, (what, name, frac)


# ---- the head
@functools.lru_cache(maxsize=None)
def _head_rows(B, A, nan_head=None):
    """attr, saved, rows of seeded normal values; nan_head "actor" / "critic": that head's five arrays of the rows are NaN"""
    g = torch.Generator().manual_seed(1000 * B + A)
    n = B * A
    attr = torch.randn((B, A, 83), generator=g).to(DEV)
    saved = torch.randn(hb.policy_saved_floats(B, A), generator=g).to(DEV)
    rows = torch.randn(n * hb.POLICY_ROW_FLOATS, generator=g).to(DEV)
    if nan_head:
        for k, v in hb.policy_views(rows, hb.POLICY_ROWS_LAYOUT, n).items():
            if k.startswith(nan_head + "."):
                v.fill_(float("nan"))
    return attr, saved, rows


def _head_problems(attr, saved, rows, actor=True, critic=True):
    """name -> (dZ, X or None) in float64, as include/flatland_param_grads.h lists them, from the buffers themselves"""
    n = attr.shape[0] * attr.shape[1]
    sv = {k: v.double() for k, v in hb.policy_views(saved, hb.POLICY_SAVED_LAYOUT, n).items() if k != "val"}
    rw = {k: v.double() for k, v in hb.policy_views(rows, hb.POLICY_ROWS_LAYOUT, n).items()}
    out = {}

    def lin(name, dz, *xs, bias="bias", weight="weight"):
        out[name + weight], out[name + bias] = (dz, torch.cat(xs, 1)), (dz, None)
    lin("attr_embedding.0.", rw["attr.dz0"], attr.view(n, 83).double())
    for i, h in ((2, "h1"), (4, "h2"), (6, "h3")):
        lin("attr_embedding.%d." % i, rw["attr.dz%d" % i], rw["attr." + h])
    for i, y in enumerate(("emb", "y1", "y2")):
        t = "transformer.%d." % i
        lin(t + "attention.in_proj_", rw["dqkv%d" % i], sv[y])
        lin(t + "attention.out_proj.", rw["do%d" % i], sv["c%d" % i])
        lin(t + "att_mlp.0.", rw["dz%d" % i], sv[y], rw["o%d" % i])
    for head, k, on in (("actor", 5, actor), ("critic", 1, critic)):
        if on:
            lin(head + "_net.0.", rw[head + ".dz0"], sv["emb"], sv["y3"])
            lin(head + "_net.2.", rw[head + ".dz2"], rw[head + ".u1"])
            lin(head + "_net.4.", rw[head + ".dz4"][:, :k], rw[head + ".u2"])
    return out


def _head_call(B, A, bufs, slices, actor=True, critic=True):
    attr, saved, rows = bufs
    on = [True] * 26 + [actor] * 6 + [critic] * 6
    rc, outs, ws, need = _raw("policy_head_param_grads", B * A, hb.POLICY_HEAD_PARAM_SHAPES, on, slices,
                              (B, A, attr.data_ptr(), saved.data_ptr(), rows.data_ptr(), int(actor), int(critic)))
    assert rc == 0, hb.lib().fl_last_error().decode()
    _check_buffers(outs, ws, need)
    return [None if o is None else o[1] for o in outs]


# ---- the encoder
@functools.lru_cache(maxsize=None)
def _tree_rows(n):
    g = torch.Generator().manual_seed(77 + n)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    x, h, da, dc, dg, q = r(n, 12), r(n, 128), r(n, 384), r(n, 128), r(n, 3, 128), r(n, 384)
    order = torch.randint(-1, 4, (n,), generator=g, dtype=torch.int64)
    x[order < 0] = float("nan")                                   # a padding node's features must not reach a sum
    child = torch.randint(0, n, (n, 3), generator=g, dtype=torch.int32)
    child[torch.rand((n, 3), generator=g) < 0.3] = -1
    child[0] = torch.tensor([0, n - 1, -1], dtype=torch.int32)    # both ends of the range, a -1
    if n > 2:
        child[n // 2] = n // 3                                    # one child in all three slots
        child[n - 1] = torch.tensor([n - 1, n - 1, 0], dtype=torch.int32)
        order[1], order[2] = 0, 1                                 # (both sides of db_c's predicate are there)
        x[1] = torch.randn(12, generator=g)
        x[2] = torch.randn(12, generator=g)
    return tuple(t.to(DEV) for t in (x, order, h, da, dc, dg, q, child))


def _tree_problems(x, order, h, da, dc, dg, q, child):
    n = x.shape[0]
    zero = torch.zeros((), dtype=torch.float64, device=DEV)
    xz = torch.where((order >= 0).view(n, 1), x.double(), zero)
    hk = torch.where((child >= 0).view(n, 3, 1), h.double()[child.clamp(min=0).long()], zero)
    dgs = ((dg[:, 0] + dg[:, 1]) + dg[:, 2]).double()             # float32 additions, in the header's order
    da, dc, q = da.double(), dc.double(), q.double()
    return {"W_iou.weight": (da, xz), "W_iou.bias": (da, None), "U_iou.weight": (da, hk.view(n, 384)), "W_c.weight": (dc, q),
            "W_c.bias": (torch.where((order >= 1).view(n, 1), dc, zero), None), "W_f.weight": (dgs, xz), "W_f.bias": (dgs, None),
            "U_f.weight": (dg.double().view(3 * n, 128), hk.view(3 * n, 128))}


def _tree_call(bufs, slices):
    n = bufs[0].shape[0]
    rc, outs, ws, need = _raw("tree_lstm_param_grads", n, hb.TREE_LSTM_PARAM_SHAPES, [True] * 8, slices,
                              (n,) + tuple(t.data_ptr() for t in bufs))
    assert rc == 0, hb.lib().fl_last_error().decode()
    _check_buffers(outs, ws, need)
    return [o[1] for o in outs]


def _same_lists(a, b):
    return all((u is None and v is None) or torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- 1. the products
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "r%d-s%d" % c)
def test_head_products(case):
    n, slices = case
    B, A = HEAD_SHAPES[n]
    bufs = _head_rows(B, A)
    before = [t.clone() for t in bufs]
    got = _head_call(B, A, bufs, slices)
    again = _head_call(B, A, bufs, slices)
    assert _same_lists(got, again), "two calls with the same slice count differ"
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(before, bufs)), "an input was written"
    _hold("head", HEAD_NAMES, got, _head_problems(*bufs), "head r%d s%d" % case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "r%d-s%d" % c)
def test_tree_products(case):
    n, slices = case
    bufs = _tree_rows(n)
    before = [t.clone() for t in bufs]
    got = _tree_call(bufs, slices)
    again = _tree_call(bufs, slices)
    assert _same_lists(got, again), "two calls with the same slice count differ"
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(before, bufs)), "an input was written"
    _hold("tree", TREE_NAMES, got, _tree_problems(*bufs), "tree r%d s%d" % case)


@pytest.mark.gpu
@pytest.mark.parametrize("off", ("actor", "critic"))
@pytest.mark.parametrize("n", (33, 257))
def test_head_with_one_head_switched_off(off, n):
    """that head's six pointers NULL, its rows NaN: nothing of it is read, the other 32 gradients stay inside the bound"""
    B, A = HEAD_SHAPES[n]
    bufs = _head_rows(B, A, off)
    actor, critic = off != "actor", off != "critic"
    got = _head_call(B, A, bufs, 0, actor, critic)
    assert [g is None for g in got] == [False] * 26 + [not actor] * 6 + [not critic] * 6
    _hold("head", HEAD_NAMES, got, _head_problems(*bufs, actor=actor, critic=critic), "head r%d without the %s" % (n, off))


@pytest.mark.gpu
def test_side_stream_and_the_wrappers():
    """one case of each on a side stream through hip_backend's wrappers (their own workspace, then the caller's): the bits of the
    raw call on the default stream"""
    B, A = HEAD_SHAPES[513]
    hbufs, tbufs = _head_rows(B, A), _tree_rows(513)
    href, tref = _head_call(B, A, hbufs, 3), _tree_call(tbufs, 3)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        hgot = hb.policy_head_param_grads(*hbufs, slices=3)
        tgot = hb.tree_lstm_param_grads(*tbufs, slices=3)
        ws = torch.empty(hb._sym("fl_policy_head_param_grads_workspace_bytes")(B * A, 3), dtype=torch.uint8, device=DEV)
        hgot2 = hb.policy_head_param_grads(*hbufs, slices=3, workspace=ws)
        with pytest.raises(ValueError, match="workspace must be a contiguous tensor of at least"):
            hb.policy_head_param_grads(*hbufs, slices=3, workspace=ws[:-8])
        with pytest.raises(ValueError, match="slices must be 0"):
            hb.tree_lstm_param_grads(*tbufs, slices=CAP + 1)
    side.synchronize()
    assert _same_lists(href, hgot) and _same_lists(href, hgot2) and _same_lists(tref, tgot)
    assert [tuple(g.shape) for g in hgot] == list(hb.POLICY_HEAD_PARAM_SHAPES)
    off = hb.policy_head_param_grads(*hbufs, critic=False)
    assert all(g is None for g in off[32:]) and all(g is not None for g in off[:32])


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def _head_args(**over):
    B, A = 2, 5
    attr, saved, rows = _head_rows(B, A)
    a = dict(n_envs=B, n_agents=A, attr=attr.data_ptr(), saved=saved.data_ptr(), rows=rows.data_ptr(), actor=1, critic=1)
    a.update({k: v for k, v in over.items() if k in a})
    return B * A, tuple(a.values())


HEAD_REFUSALS = [
    (dict(n_envs=0), "bad sizes"), (dict(n_envs=-3), "bad sizes"), (dict(n_agents=0), "bad sizes"), (dict(n_agents=1025), "bad sizes"),
    (dict(actor=2), "actor and critic must be 0 or 1"), (dict(critic=-1), "actor and critic must be 0 or 1"),
    (dict(actor=0, critic=0), "both 0"),
    (dict(attr=None), "attr is NULL"), (dict(saved=None), "saved is NULL"), (dict(rows=None), "rows is NULL"),
    (dict(attr="+4"), "attr is not 16-byte aligned"), (dict(saved="+4"), "saved is not 16-byte aligned"),
    (dict(rows="+8"), "rows is not 16-byte aligned"),
    (dict(slices=-1), "slices must be 0"), (dict(slices=CAP + 1), "slices must be 0"),
    (dict(grads=None), "grads is NULL"), (dict(null_grad=0), "gradient 0 is NULL"), (dict(null_grad=37), "gradient 37 is NULL"),
    (dict(null_grad=26, critic=1), "gradient 26 is NULL"), (dict(odd_grad=5), "gradient 5 is not 16-byte aligned"),
    (dict(slices=2, ws=None), "workspace is NULL"), (dict(slices=2, ws="+8"), "workspace is not 16-byte aligned"),
    (dict(slices=2, short=16), "workspace of"), (dict(slices=3, short=1), "workspace of"),
]
TREE_INPUTS = ("x", "node_order", "h", "da", "dc", "dg", "q", "child")
TREE_REFUSALS = [
    (dict(n_rows=0), "bad size"), (dict(n_rows=-1), "bad size"), (dict(n_rows=2 ** 31 // 384 + 1), "bad size")
] + [({k: None}, k + " is NULL") for k in TREE_INPUTS] + [
    ({k: "+4"}, k + " is not 16-byte aligned") for k in TREE_INPUTS if k not in ("node_order", "child")
] + [
    (dict(node_order="+4"), "node_order is not 8-byte aligned"), (dict(child="+2"), "child is not 4-byte aligned"),
    (dict(slices=-1), "slices must be 0"), (dict(slices=CAP + 1), "slices must be 0"),
    (dict(grads=None), "grads is NULL"), (dict(null_grad=7), "gradient 7 is NULL"), (dict(odd_grad=2), "gradient 2 is not 16-byte aligned"),
    (dict(slices=3, ws=None), "workspace is NULL"), (dict(slices=3, ws="+8"), "workspace is not 16-byte aligned"),
    (dict(slices=3, short=8), "workspace of"),
]


def _refused(name, rows, shapes, args, over, message):
    """the call with one argument spoilt: FL_ERR_ARG with its message, and every byte of the outputs and of the workspace as before"""
    slices = over.get("slices", 0)
    outs = _outputs(shapes, [True] * len(shapes))
    need = hb._sym("fl_%s_workspace_bytes" % name)(rows, min(max(slices, 0), CAP)) if 0 <= slices <= CAP else 0
    ws = _guarded(need)
    ptrs = [o[1].data_ptr() for o in outs]
    if "null_grad" in over:
        ptrs[over["null_grad"]] = None
    if "odd_grad" in over:
        ptrs[over["odd_grad"]] += 4
    grads = None if "grads" in over else (hb.vp * len(shapes))(*ptrs)
    wsp = ws.data_ptr()
    if "ws" in over:
        wsp = None if over["ws"] is None else wsp + int(over["ws"])
    rc = hb._sym("fl_" + name)(*args, grads, slices, wsp, need - over.get("short", 0), None)
    assert rc == 1, rc                                            # FL_ERR_ARG
    msg = hb.lib().fl_last_error().decode()
    assert msg.startswith("fl_%s: " % name) and message in msg, msg
    torch.cuda.synchronize()
    for buf, _ in outs:
        assert bool((buf[:-GUARD] == 0xFF).all()) and bool((buf[-GUARD:] == 0xA5).all())
    assert bool((ws[:need] == 0xFF).all()) and bool((ws[need:] == 0xA5).all())


def _spoil(args, names, over):
    out = []
    for k, v in zip(names, args):
        if k in over:
            v = None if over[k] is None else (v + int(over[k]) if isinstance(over[k], str) else over[k])
        out.append(v)
    return tuple(out)


@pytest.mark.gpu
@pytest.mark.parametrize("over,message", HEAD_REFUSALS, ids=["%s-%d" % (m.replace(" ", "_"), i) for i, (_, m) in enumerate(HEAD_REFUSALS)])
def test_head_refusals(over, message):
    rows, args = _head_args()
    args = _spoil(args, ("n_envs", "n_agents", "attr", "saved", "rows", "actor", "critic"), over)
    _refused("policy_head_param_grads", rows, hb.POLICY_HEAD_PARAM_SHAPES, args, over, message)


@pytest.mark.gpu
@pytest.mark.parametrize("over,message", TREE_REFUSALS, ids=["%s-%d" % (m.replace(" ", "_"), i) for i, (_, m) in enumerate(TREE_REFUSALS)])
def test_tree_refusals(over, message):
    bufs = _tree_rows(33)
    args = _spoil((33,) + tuple(t.data_ptr() for t in bufs), ("n_rows",) + TREE_INPUTS, over)
    _refused("tree_lstm_param_grads", 33, hb.TREE_LSTM_PARAM_SHAPES, args, over, message)


# ---------------------------------------------------------------------------------------------------------------- 3. the head's module
def _hip_net(params, both=False):
    net = hbw._net(params)
    net.param_grads = "hip"
    if both:
        net.tree_lstm.trainable, net.tree_lstm.param_grads = True, "hip"
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("case", hbw.GRAD_CASES, ids=lambda c: hbw._case_id(*c))
def test_head_gradients_through_the_module(case):
    """Network(trainable=True, param_grads="hip").head against the float64 autograd of the restatement: the existing test's measure
    and its R = 6"""
    B, A, s = case
    attr, tree = hbw._inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    net = _hip_net(st.params(s))
    g, logits, value = hbw._kernel_grads(net, attr, tree, Rl, Rv)
    g32, g64 = hbw._reference(B, A, s)
    hbw._assert_within(g, g32, g64, "hip " + hbw._case_id(*case))


def test_the_constructor_reaches_the_same_switches():
    from flatland_marl_amd.policy import Network
    net = Network(trainable=True, param_grads="hip")
    assert (net.trainable, net.param_grads, net.tree_lstm.param_grads) == (True, "hip", "hip")


# ---------------------------------------------------------------------------------------------------------------- 4. the encoder's module
@pytest.mark.gpu
@pytest.mark.parametrize("case", tbw.ALL, ids=lambda c: tbw._case_id(*c))
def test_tree_gradients_through_the_module(case):
    """TreeLSTM(trainable=True, param_grads="hip") on the forests and sizes of the backward's test: its measure and its R = 5"""
    from flatland_marl_amd.policy import TreeLSTM
    kind, size, N, extra, roots, scale, feat = case
    x = tbw._forest(kind, size, N, extra, feat, tbw._cu())
    T = x[2].shape[1]
    params = tl.seeded_params(11, scale)
    up = tbw._upstream(T, N, roots)
    m = TreeLSTM(trainable=True, param_grads="hip").to(DEV)
    m.load_state_dict(params)
    g, _ = tbw._kernel_grads(m, x, up, roots)
    g2, _ = tbw._kernel_grads(m, x, up, roots)
    for k in tg.PARAM_ORDER:
        assert torch.equal(g[k], g2[k]), (k, "two backward passes differ")
    g64 = tg.grads(x, params, up, roots)
    g32 = tg.grads(x, params, up, roots, torch.float32)
    figs = tbw._figures(g, g32, g64)
    print("hip", tbw._case_id(*case), " ".join("%s %.3g" % (k[6:], v) for k, v in figs.items() if k.startswith("ratio_")))
    tbw._assert_within(g, g32, g64, "hip " + tbw._case_id(*case))


# ---------------------------------------------------------------------------------------------------------------- 5. the other switches
def _forest_3_11():
    from tests import tree_lstm_forests as tf
    B, A, N = 3, 11, 31
    x = tuple(t.to(DEV) for t in tf.make("rand", B * A, N, 5))
    return (x[0].view(B, A, N, 12).contiguous(), x[1].view(B, A, N - 1, 3).contiguous(), x[2].view(B, A, N).contiguous(),
            x[3].view(B, A, N - 1).contiguous())


def _all_46(net, attr, x, Rl, Rv):
    net.zero_grad(set_to_none=True)
    logits, value = net(attr, *x)
    pg.loss_of(logits[0], value, Rl.to(DEV), Rv.to(DEV)).backward()
    return {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}


def _chained(params, attr, x, Rl, Rv, dtype):
    B, A, N = x[0].shape[:3]
    pt = {k: params["tree_lstm." + k].detach().to(device=DEV, dtype=dtype).clone().requires_grad_(True) for k in tg.PARAM_ORDER}
    ph_ = pg.leaf_params(params, DEV, dtype)
    h = tg.tree_lstm(*x, pt, dtype).view(B, A, N, 128)[:, :, 0]
    lg, v = pg.forward(attr, h, ph_)
    pg.loss_of(lg, v, Rl, Rv).backward()
    return {**{"tree_lstm." + k: t.grad for k, t in pt.items()}, **{k: t.grad for k, t in ph_.items()}}


@pytest.mark.gpu
@pytest.mark.parametrize("chunked", (False, True), ids=("one_chunk", "chunks"))
def test_one_backward_trains_all_46_parameters(monkeypatch, chunked):
    """both switches set, both param_grads "hip": one loss.backward() through forward gives all 46 gradients, each within the head's
    or the encoder's R of the float64 autograd through both restatements, the same bits on a second backward, and the torch
    products are not called; chunked: HEAD_BACKWARD_CHUNK_ROWS and BACKWARD_CHUNK_TREES down to 25 rows / 16 trees, so that the
    head runs in two chunks of whole envs and the encoder in three"""
    from flatland_marl_amd import policy
    calls = []
    for mod, name in ((policy, "tree_lstm_param_grads"), (policy, "policy_head_param_grads"), (hb, "tree_lstm_param_grads"),
                      (hb, "policy_head_param_grads")):
        tag = ("torch." if mod is policy else "hip.") + name
        monkeypatch.setattr(mod, name, (lambda f, tag: lambda *a, **k: (calls.append(tag), f(*a, **k))[1])(getattr(mod, name), tag))
    if chunked:
        monkeypatch.setattr(policy, "HEAD_BACKWARD_CHUNK_ROWS", 25)
        monkeypatch.setattr(policy, "BACKWARD_CHUNK_TREES", 16)
        assert policy.head_chunks(3, 11) == [(0, 2), (2, 3)]
    x = _forest_3_11()
    attr, _ = hbw._inputs(3, 11)
    Rl, Rv = pg.upstream(3, 11)
    params = st.params(0)
    net = _hip_net(params, both=True)
    got = _all_46(net, attr, x, Rl, Rv)
    assert len(got) == 46
    assert calls == ["hip.policy_head_param_grads"] * (2 if chunked else 1) + ["hip.tree_lstm_param_grads"] * (3 if chunked else 1)
    again = _all_46(net, attr, x, Rl, Rv)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got)
    g32, g64 = (_chained(params, attr, x, Rl, Rv, dt) for dt in (torch.float32, torch.float64))
    for k in got:
        err, e32 = pg.rel_error(got[k], g64[k]), pg.rel_error(g32[k], g64[k])
        print(k, err, e32)
        assert err <= (tbw.R if k.startswith("tree_lstm.") else hbw.R) * e32, (k, err, e32)


@pytest.mark.gpu
def test_value_false_and_no_grad_under_hip(monkeypatch):
    """value=False: the critic's six gradients are None, the others inside R; under torch.no_grad() the launches are the inference
    path's -- no saved forward, no backward, no parameter gradients"""
    B, A, s = 3, 11, 1
    attr, tree = hbw._inputs(B, A)
    Rl, Rv = pg.upstream(B, A)
    net = _hip_net(st.params(s))
    g, _, value = hbw._kernel_grads(net, attr, tree, Rl, None, value=False)
    assert value is None and all(g[k] is None for k in pg.CRITIC)
    g32, g64 = hbw._reference(B, A, s, "logits")
    hbw._assert_within(g, g32, g64, "hip novalue")
    calls = []
    for name in ("policy_head", "policy_head_forward_saved", "policy_head_backward", "policy_head_param_grads", "tree_lstm",
                 "tree_lstm_backward", "tree_lstm_param_grads"):
        monkeypatch.setattr(hb, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(hb, name), name))
    both = _hip_net(st.params(s), both=True)
    with torch.no_grad():
        a = both(attr, *_forest_3_11())
    assert calls == ["tree_lstm", "policy_head"] and not a[0][0].requires_grad
    with torch.no_grad():
        b = hbw._net(st.params(s), trainable=False)(attr, *_forest_3_11())
    assert torch.equal(_bits(a[0][0]), _bits(b[0][0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.gpu
def test_a_library_without_the_symbols_is_refused(monkeypatch):
    """param_grads="hip" on a library that predates the entry points: _sym's error, not a fall-back to the torch products"""
    real = hb._sym

    def older(name):
        if "param_grads" in name:
            raise hb.FlatlandHipError(1, "the loaded library has no %s (an older build loaded through --lib?)" % name)
        return real(name)
    monkeypatch.setattr(hb, "_sym", older)
    attr, tree = hbw._inputs(3, 11)
    net = _hip_net(st.params(0))
    logits, value = net.head(attr, tree.clone().requires_grad_(True))
    with pytest.raises(hb.FlatlandHipError, match="has no fl_policy_head_param_grads"):
        (logits[0].sum() + value.sum()).backward()
