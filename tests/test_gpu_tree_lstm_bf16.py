"""fl_tree_lstm_bf16 (include/flatland_policy_bf16.h) on the GPU: the tree encoder with bf16 operands in its three recurrent
products, on the synthetic forests of tests/tree_lstm_forests.py and on the reference's fixtures.

The kernel groups the trees with ftl_group and tiles a level in 32 rows, as k_tree_lstm does, so `sizes`, `group_of` and the tile
edges of tests/test_tree_lstm_synth.py are this kernel's own; CASES below is a smaller choice from the same grid.

Tolerance.  e16 = the error of the emulation (tests/tree_lstm_bf16_torch.py: the restatement with the recurrent products'
operands rounded to bf16, float64 everywhere else) against the float64 restatement on the same inputs, with the two measures of
test_tree_lstm_synth._errors (max |dh|, max |dc| / max(1, |c|)).  The kernel passes when its error is at most R16 * e16, R16 = 2:
it differs from the emulation by float32 sums and by roundings that land on the other side of a bf16 tie, perturbations the size
of those the emulation makes already (on the CPU the emulation with float32 sums has the float64-sum emulation's error to three
digits), so 2 is the usual factor of two over the expected ratio of 1.  The nodes of height 0 see no bf16 operand: they are held
to the float32 kernel's bound, R = 3 times e32 (the float32 restatement's error) over those nodes.
TREE_LSTM_BF16_ERRORS=<path> makes the cases write err, e16 and their ratio to <path> in the format of
tests/golden/synth_tree_lstm_bf16_errors.json."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import tree_lstm_bf16_torch as tl16
from tests import tree_lstm_forests as tf
from tests import tree_lstm_torch as tl
from tests import util
from tests.test_tree_lstm_golden import golden_inputs, golden_params
from tests.test_tree_lstm_synth import (CONDITIONS, DEV, FX, GUARD, R, TILE_EDGES, _case_id, _cu, _errors, _forest, _guarded,
                                        _structure, _violations, _weights, group_of, sizes)

R16 = 2
ERRORS = os.path.join(util.GOLD, "synth_tree_lstm_bf16_errors.json")
FIXTURES = sorted(os.path.basename(p)[len("tree_lstm_"):-4] for p in glob.glob(os.path.join(util.GOLD, "tree_lstm_*.npz"))
                  if "grad" not in os.path.basename(p) and "errors" not in os.path.basename(p))

# kind, size (a key of sizes()), N, extra arguments of the generator
CASES = [
    ("rand", "g16_full", 64, {}), ("chain", "g16_tail1", 64, {}), ("perm", "g16_tail15", 31, {}),
    ("mixpad", "g16_full", 31, dict(base="weird")),
    ("full", "g5_tail3", 4, {}), ("full", "g2_tail1", 31, {}), ("rand", "g2_tail1", 34, {}), ("rand", "g1", 4, {}),
    ("chain", "g6_tail2", 7, {}), ("gaps", "g7_tail1", 64, {}), ("gaps", "g1", 34, {}), ("weird", "g5_tail3", 7, {}),
    ("weird", "g1", 64, {}), ("perm", "g1", 31, {}), ("mixpad", "g7_tail1", 7, dict(base="chain")),
    ("flat", "g1", 64, dict(L=(31, 32, 33, 64))), ("flat", "g2_tail1", 64, dict(L="edges")),
    ("lvl1", "g6_tail2", 64, dict(m="edges")), ("lvl1", "g16_tail15", 31, dict(m="edges")),
]


def _combos(size):
    """(features, weight scale): both kinds of features and both scales, crossed the other way at the largest sizes"""
    return [("gauss", 4.0), (FX, 1.0)] if size.startswith("g16") else [("gauss", 1.0), (FX, 4.0)]


ALL = [c + fs for c in CASES for fs in _combos(c[1])]
IDS = [_case_id(*c) for c in ALL]


def _packed(w):
    from flatland_marl_amd import hip_backend as hb
    return hb.tree_lstm_pack_bf16(w)


def _launch(x, w, packed, roots_only, with_c, status):
    """one fl_tree_lstm_bf16 launch into NaN-filled outputs, which go on for GUARD more trees that must stay NaN"""
    from flatland_marl_amd import hip_backend as hb
    T, N = x[2].shape[1:]
    rows, more = (T, GUARD) if roots_only else (T * N, GUARD * N)
    hb_, cb_ = [torch.full((rows + more, 128), float("nan"), device=DEV) if k else None for k in (True, with_c)]
    h, c = hb_[:rows], cb_[:rows] if with_c else None
    hb.tree_lstm_bf16(*x, w, packed, roots_only, h, c, status)
    assert torch.isnan(hb_[rows:]).all() and (not with_c or torch.isnan(cb_[rows:]).all()), "a write past the last tree"
    return h, c


@pytest.mark.gpu
def test_sizes_cover_the_groupings():
    """the new kernel groups with ftl_group: G = 1 (T = 37); G = 2 with a one-tree tail; 2 < G < 16 with 1, 2 and 3 trees in the
    last set-up pass (tb += 4), in full groups and in tails; G = 16 full, with a one-tree and a 15-tree tail -- on this device"""
    cu = _cu()
    got = {}
    for name, T in sizes(cu).items():
        G = group_of(T, cu)
        got[name] = (G, T - (-(-T // G) - 1) * G)
    assert sizes(cu)["g1"] == 37 and got["g1"] == (1, 1) and got["g2_tail1"] == (2, 1)
    assert got["g5_tail3"] == (5, 3) and got["g6_tail2"] == (6, 2) and got["g7_tail1"] == (7, 1)
    assert got["g16_full"] == (16, 16) and got["g16_tail1"] == (16, 1) and got["g16_tail15"] == (16, 15)
    mid = [v for v in got.values() if 2 < v[0] < 16]
    assert {g % 4 for g, _ in mid} >= {1, 2, 3} and {t % 4 for _, t in mid} >= {1, 2, 3}
    assert {c[1] for c in CASES} == set(got)
    assert {c[2] for c in CASES} == {4, 7, 31, 34, 64}
    assert {c[0] for c in CASES} == set(tf.KINDS)


@pytest.mark.gpu
def test_level_populations_sit_on_the_tile_edges():
    """the flat and lvl1 cases put 31, 32, 33, 64 and 65 nodes (rows - 1 .. 2 rows + 1 of the 32-row tile) on a level of one
    workgroup: at height 0 and above it"""
    cu = _cu()
    level0, above = set(), set()
    for kind, size, N, extra in CASES:
        if kind in ("flat", "lvl1"):
            no = _structure(kind, size, N, tuple(sorted(extra.items())), cu)[0]
            pops = tf.level_populations(torch.from_numpy(no), group_of(sizes(cu)[size], cu))
            level0 |= {v for (_, n), v in pops.items() if n == 0}
            above |= {v for (_, n), v in pops.items() if n >= 1}
    assert level0 >= set(TILE_EDGES), sorted(level0)
    assert above >= set(TILE_EDGES), sorted(above)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_kernel_matches_the_emulation(case):
    kind, size, N, extra, feat, scale = case
    x = _forest(kind, size, N, extra, feat, _cu())
    T = x[2].shape[1]
    assert _violations([v[:, :300] for v in x]) == 0
    params = tl.seeded_params(11, scale)
    w = _weights(params)
    pk = _packed(w)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    h, c = _launch(x, w, pk, False, True, status)             # every node, c given
    h2, c2 = _launch(x, w, pk, False, True, status)
    hn, _ = _launch(x, w, pk, False, False, status)           # every node, c in the workspace: the module's path
    hr, cr = _launch(x, w, pk, True, True, status)            # roots only
    hq, _ = _launch(x, w, pk, True, False, status)
    assert int(status.item()) == 0
    assert torch.equal(h, h2) and torch.equal(c, c2)
    pad = (x[2] == -2).view(-1)
    assert (h[pad] == 0).all() and (c[pad] == 0).all() and (hn[pad] == 0).all()
    assert torch.equal(hr, h.view(T, N, 128)[:, 0]) and torch.equal(cr, c.view(T, N, 128)[:, 0])
    assert torch.equal(hq, hr) and torch.equal(hn, h)
    del h2, c2, hq, hn
    h64, c64 = tl.tree_lstm(*x, params, with_c=True)
    # the nodes of height 0: float32 arithmetic only, the float32 kernel's bound
    leaf = (x[2] == 0).view(-1)
    if leaf.any():
        h32, c32 = tl.tree_lstm(*x, params, dtype=torch.float32, with_c=True)
        e32 = _errors(h32[leaf], c32[leaf], h64[leaf], c64[leaf])
        err0 = _errors(h[leaf], c[leaf], h64[leaf], c64[leaf])
        print(_case_id(*case), "leaves: err %.3g %.3g e32 %.3g %.3g" % (err0 + e32))
        assert err0[0] <= R * e32[0] and err0[1] <= R * e32[1], (err0, e32)
        del h32, c32
    # every node
    he, ce = tl16.tree_lstm(*x, params, with_c=True)
    e16_h, e16_c = _errors(he, ce, h64, c64)
    err_h, err_c = _errors(h, c, h64, c64)
    if int(x[2].max()) <= 0:       # a flat forest: the emulation is the restatement, e16 = 0 and the bound above is the one there is
        assert kind == "flat" and e16_h == 0 and e16_c == 0
        figs = dict(err_h=err_h, e16_h=e16_h, ratio_h=0.0, err_c=err_c, e16_c=e16_c, ratio_c=0.0)
    else:
        figs = dict(err_h=err_h, e16_h=e16_h, ratio_h=err_h / e16_h, err_c=err_c, e16_c=e16_c, ratio_c=err_c / e16_c)
    print(_case_id(*case), "T %d" % T, " ".join("%s %.3g" % kv for kv in figs.items()))
    util.record_errors("TREE_LSTM_BF16_ERRORS", "cases", _case_id(*case), figs, R16=R16)
    if int(x[2].max()) > 0:
        assert err_h <= R16 * e16_h, figs
        assert err_c <= R16 * e16_c, figs
        e_h, e_c = _errors(hr, cr, h64.view(T, N, 128)[:, 0], c64.view(T, N, 128)[:, 0])
        assert e_h <= R16 * e16_h and e_c <= R16 * e16_c


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures(name):
    """the reference module's outputs (tools/capture_tree_lstm.py, seeded weights at both scales): the kernel's error against the
    fixture is at most R16 times the emulation's error against it"""
    g = np.load(os.path.join(util.GOLD, "tree_lstm_%s.npz" % name))
    x = [v.to(DEV).contiguous() for v in golden_inputs(g)]
    B, A, N = x[2].shape
    T = B * A
    ids = list(g["tree_ids"])
    assert list(g["scales"]) == [1.0, 4.0]
    for s, scale in enumerate(g["scales"]):
        params = golden_params(g, scale)
        w = _weights(params)
        h, c = torch.empty(T * N, 128, device=DEV), torch.empty(T * N, 128, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        from flatland_marl_amd import hip_backend as hb
        hb.tree_lstm_bf16(*x, w, _packed(w), False, h, c, status)
        assert int(status.item()) == 0
        he, ce = tl16.tree_lstm(*x, params, with_c=True)
        ref = [torch.from_numpy(np.asarray(g[k][s], dtype=np.float64)).to(DEV) for k in ("root_h", "root_c", "all_h", "all_c")]

        def errs(hh, cc):
            hh, cc = hh.view(T, N, 128), cc.view(T, N, 128)
            a = _errors(hh[:, 0], cc[:, 0], ref[0], ref[1])
            b = _errors(hh[ids], cc[ids], ref[2], ref[3])
            return max(a[0], b[0]), max(a[1], b[1])
        err, e16 = errs(h, c), errs(he, ce)
        print(name, "x%d" % scale, "err %.3g %.3g e16 %.3g %.3g" % (err + e16))
        assert err[0] <= R16 * e16[0] and err[1] <= R16 * e16[1], (err, e16)


@pytest.mark.gpu
@pytest.mark.parametrize("cond", list(CONDITIONS))
def test_bad_trees_are_counted_as_the_f32_kernel_counts_them(cond):
    """complete ternary trees of 13 nodes in N = 31 with one condition injected into three of them (test_tree_lstm_synth): the
    status word equals fl_tree_lstm's, the other trees' outputs equal those of the clean forest bit for bit"""
    from flatland_marl_amd import hip_backend as hb
    cu, N = _cu(), 31
    T = sizes(cu)["g5_tail3"]
    G = group_of(T, cu)
    BAD = [G + 2, G + 3, T - 1]                               # two in one full group, one in the tail group
    forest, adj, no, eo = [v[0].clone() for v in tf.make("full", T, N, 3)]
    clean = [forest[None], adj.clone()[None], no.clone()[None], eo.clone()[None]]
    for t in BAD:
        clean[1][0, t], clean[2][0, t], clean[3][0, t] = -2, -2, -2                   # all padding
        CONDITIONS[cond](t, t * N, N, no, eo, adj)
    no[BAD[2], 25] = N + 3                                     # a second violation in one of them
    x, clean = _guarded([forest[None], adj[None], no[None], eo[None]]), _guarded(clean)
    w = _weights(tl.seeded_params(11, 1.0))
    pk = _packed(w)
    st32 = torch.zeros(1, dtype=torch.int32, device=DEV)
    hb.tree_lstm(*x, w, False, torch.empty(T * N, 128, device=DEV), None, st32)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    h, c = _launch(x, w, pk, False, True, status)
    assert int(status.item()) == int(st32.item()) == len(BAD)
    status.zero_()
    hr, cr = _launch(x, w, pk, True, True, status)
    assert int(status.item()) == len(BAD)
    status.zero_()
    h0, c0 = _launch(clean, w, pk, False, True, status)
    hr0, cr0 = _launch(clean, w, pk, True, True, status)
    assert int(status.item()) == 0
    others = torch.ones(T, dtype=torch.bool, device=DEV)
    others[BAD] = False
    assert not torch.isnan(h0).any() and not torch.isnan(c0).any()
    for a, b in ((h, h0), (c, c0)):
        assert torch.equal(a.view(T, N, 128)[others], b.view(T, N, 128)[others])
    assert torch.equal(hr[others], hr0[others]) and torch.equal(cr[others], cr0[others])
    assert torch.equal(hr0, h0.view(T, N, 128)[:, 0])


def _pack_values():
    """float32 values for the three matrices: normal ones, exact ties between two bf16 values (both ways round), +-0, subnormals,
    +-inf, and the largest finite values (which round to inf)"""
    rng = np.random.default_rng(5)
    n = 384 * 384 + 128 * 384 + 128 * 128
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    exp = (bits >> 23) & 0xFF
    bits[exp == 0xFF] &= np.uint32(0xFF800000)                          # random NaNs become inf: NaN has a test of its own
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00008000, 0x00018000,
                        0x007FFFFF, 0x807F8000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF], dtype=np.uint32)
    ties = (rng.integers(0, 0x7F80, size=4096, dtype=np.uint64).astype(np.uint32) << 16) | np.uint32(0x8000)
    ties[::2] |= np.uint32(0x80000000)
    for k, off in enumerate((0, 384 * 384, 384 * 384 + 128 * 384)):                 # the same set at the head of every matrix
        bits[off:off + len(special)] = special
        bits[off + 64:off + 64 + 1024] = ties[1024 * k:1024 * (k + 1)]
    bits[-len(special):] = special                                                  # ... and at the very end of the buffer
    return torch.from_numpy(bits.view(np.float32).copy())


def _as_packed(m):
    """a matrix [R, K] in the order include/flatland_policy_bf16.h documents: blocks of 32 rows, a block's K / 16 steps, a step's 64
    lanes (l = 32 * (k half of the step) + row of the block), 8 elements a lane"""
    R, K = m.shape
    return m.view(R // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def test_packed_order_is_the_documented_formula():
    m = torch.arange(64 * 32, dtype=torch.int32).view(64, 32)
    got = _as_packed(m)
    for b, s, l, j in ((0, 0, 0, 0), (0, 1, 5, 3), (1, 0, 63, 7), (1, 1, 32, 0), (0, 0, 31, 7), (1, 1, 40, 2)):
        assert int(got[512 * (b * 2 + s) + 8 * l + j]) == int(m[32 * b + (l & 31), 16 * s + 8 * (l >> 5) + j])


@pytest.mark.gpu
def test_pack_equals_torchs_rounding():
    from flatland_marl_amd import hip_backend as hb
    v = _pack_values()
    assert not torch.isnan(v).any()
    a, b = 384 * 384, 384 * 384 + 128 * 384
    w = [None] * 8
    w[2], w[3], w[7] = v[:a].view(384, 384).to(DEV), v[a:b].view(128, 384).to(DEV), v[b:].view(128, 128).to(DEV)
    guard = torch.full((hb.lib().fl_tree_lstm_bf16_packed_bytes() + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    pk = hb.tree_lstm_pack_bf16(w, guard[:-64])
    assert pk.numel() == 2 * v.numel() == 425984 and (guard[-64:] == 0xA5).all()
    got = pk.cpu().view(torch.int16)
    exp = torch.cat([_as_packed(m.cpu().to(torch.bfloat16).view(torch.int16)) for m in (w[2], w[3], w[7])])
    assert torch.equal(got, exp), (got != exp).nonzero().flatten()[:8]
    assert torch.equal(hb.tree_lstm_pack_bf16(w).cpu().view(torch.int16), exp)
    nan = torch.from_numpy(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF], dtype=np.uint32).view(np.float32))
    assert torch.isnan(nan).all()
    w[7] = w[7].clone()
    w[7].view(-1)[5:10] = nan.to(DEV)
    got = torch.isnan(hb.tree_lstm_pack_bf16(w).cpu().view(torch.bfloat16)[b:])
    assert torch.equal(got, _as_packed(torch.isnan(w[7].cpu())))             # NaN where the source has one, nowhere else
    assert int(got.sum()) == 5


# ---------------------------------------------------------------------------------------------------------------- the module
def _inputs(T=23, N=31, seed=9):
    return [v.to(DEV).contiguous() for v in tf.make("rand", T, N, seed)]


def _direct(x, params, roots_only):
    from flatland_marl_amd import hip_backend as hb
    T, N = x[2].shape[1:]
    w = _weights(params)
    h = torch.empty((T if roots_only else T * N, 128), device=DEV)
    return hb.tree_lstm_bf16(*x, w, _packed(w), roots_only, h)


@pytest.mark.gpu
def test_module_runs_the_bf16_launch_on_the_current_and_on_a_side_stream():
    from flatland_marl_amd import hip_backend as hb
    from flatland_marl_amd.policy import TreeLSTM
    x = _inputs()
    T, N = x[2].shape[1:]
    params = tl.seeded_params(11, 1.0)
    m = TreeLSTM(precision="bf16").to(DEV)
    m.load_state_dict(params)
    exp, exp_r = _direct(x, params, False), _direct(x, params, True)
    with torch.no_grad():
        assert torch.equal(m(*x), exp) and torch.equal(m.roots(*x), exp_r.view(1, T, 128))
        assert torch.equal(m(*x, check=True), exp)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        got, got_r = m(*x), m.roots(*x)
    side.synchronize()
    assert torch.equal(got, exp) and torch.equal(got_r.view(T, 128), exp_r)
    # trainable: the bf16 launch under no_grad, ValueError under grad mode
    m.trainable = True
    with torch.no_grad():
        assert torch.equal(m(*x), exp)
    with pytest.raises(ValueError):
        m(*x)
    with pytest.raises(NotImplementedError):
        m.trainable = False
        m(*x).sum().backward()
    # precision="f32": hb.tree_lstm's bits, and not the bf16 launch's
    m32 = TreeLSTM.from_module(m)
    assert m32.precision == "f32"
    h32 = hb.tree_lstm(*x, _weights(params), False, torch.empty(T * N, 128, device=DEV))
    with torch.no_grad():
        assert torch.equal(m32(*x), h32)
    assert not torch.equal(h32, exp)
    m32.precision = "bf16"
    with torch.no_grad():
        assert torch.equal(m32(*x), exp)
    m32.precision = "half"
    with pytest.raises(ValueError):
        m32(*x)


@pytest.mark.gpu
def test_module_repacks_after_the_weights_changed():
    from flatland_marl_amd.policy import TreeLSTM
    x = _inputs()
    m = TreeLSTM(precision="bf16").to(DEV)
    m.load_state_dict(tl.seeded_params(11, 1.0))
    with torch.no_grad():
        a = m(*x).clone()
        m.U_f.weight.mul_(0.5)                                                # an in-place update
        p2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        b = m(*x).clone()
        assert not torch.equal(a, b) and torch.equal(b, _direct(x, p2, False))
        p3 = tl.seeded_params(12, 4.0)
        m.load_state_dict(p3)
        c = m(*x).clone()
        fresh = TreeLSTM(precision="bf16").to(DEV)
        fresh.load_state_dict(p3)
        assert not torch.equal(b, c) and torch.equal(c, fresh(*x)) and torch.equal(c, _direct(x, p3, False))
        m.W_c.weight = torch.nn.Parameter(m.W_c.weight.detach() * 0.25)        # another tensor
        p4 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        assert torch.equal(m(*x), _direct(x, p4, False))


@pytest.mark.gpu
def test_network_with_a_bf16_encoder():
    from flatland_marl_amd.policy import Network
    from tests import policy_head_torch as ph
    from tests.test_gpu_policy_head import _golden_obs
    params = ph.seeded_params(3, 3.0)
    net = Network(precision="bf16").to(DEV)
    net.load_state_dict(params)
    net32 = Network.from_module(net, precision="f32")
    assert net.tree_lstm.precision == "bf16" and net32.tree_lstm.precision == "f32"
    assert Network.from_module(net).tree_lstm.precision == "bf16"
    attr, forest, adj, no, eo, valid = _golden_obs()
    with torch.no_grad():
        (logits,), value = net(attr, forest, adj, no, eo)
        tree = net.tree_lstm.roots(forest, adj, no, eo)
        tree32 = net32.tree_lstm.roots(forest, adj, no, eo)
        assert not torch.equal(tree, tree32)
        (l2,), v2 = net.head(attr, tree)
        assert torch.equal(logits, l2) and torch.equal(value, v2)
        (l32,), _ = net32(attr, forest, adj, no, eo)
        assert torch.equal(l32, net32.head(attr, tree32)[0][0])               # precision="f32": today's launches
        for mode in ("soft", "hard"):
            act = net.act(attr, forest, adj, no, eo, valid, mode)
            assert act.dtype == torch.uint8 and act.shape == valid.shape[:2]
            assert torch.equal(act, net.head(attr, tree, valid, mode)[2])
            ok = valid.gather(2, act.long().unsqueeze(-1)).squeeze(-1).bool() | ~valid.any(-1)
            assert ok.all()
