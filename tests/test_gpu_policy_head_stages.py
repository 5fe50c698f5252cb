"""GPU: fl_policy_head stage by stage.  The caller owns the workspace, so after a call it holds every intermediate that was not
overwritten (tests/policy_head_stages.py: emb, xa, xb, block 2's ao and qkv, val).  Each stage is compared with its float64
restatement computed FROM THE KERNEL'S OWN PREVIOUS STAGE, so a check isolates one piece of kernel code, and the pass criterion is
an a-priori forward error bound per element (tests/policy_head_bounds.py), valid for any summation order -- not a ratio fitted to
the kernel.  tests/test_policy_head_stages.py holds two float32 restatements inside the same bounds on the CPU.

The bounds of the chains without an observable intermediate (the four attr layers; the five layers from (emb, xb, ao) to logits and
val) grow by |W| a layer and end far above a float32 evaluation's error (tests/golden/policy_head_stage_errors.json: max_over_bound
of 1e-6 to 1e-7), so the *_alone cases put ONE seeded layer of such a chain among identities, where the same bound is a single
layer's.

POLICY_HEAD_ERRORS=<path> makes test_stages write, for every stage of at least 4096 outputs, rms(kernel error) / rms(error of
torch's eager float32 ops on the same inputs) and max(kernel error / bound) into <path>, in the format of
tests/golden/policy_head_stage_errors.json, whose "stages" are the MI355X figures.  Recorded, not asserted: no ratio is fixed here.
"""
import functools

import numpy as np
import pytest
import torch

from tests import policy_head_bounds as pb
from tests import policy_head_stages as phs
from tests import policy_head_torch as ph
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_ULPS = pb.allowance()


@functools.lru_cache(maxsize=2)
def _case(case):
    attr, tree, valid, P = phs.CASES[case]()
    return (attr.to(DEV).contiguous(), tree.to(DEV).contiguous(), valid.to(DEV).contiguous(), phs.device_params(P, DEV),
            ph.stage_params(P, DEV), ph.stage_params(P, DEV, torch.float32))


def _sound(k):
    """a call on a workspace of NaNs: every element of every stage and output was written, nothing behind the workspace was"""
    for n in phs.STAGES + ("logits", "value"):
        assert bool(torch.isfinite(getattr(k, n)).all()), n
    assert bool((k.guard == 0xA5).all()) and k.guard.numel() == phs.GUARD


def _eager32(k, attr, p32):
    """torch's eager float32 ops on the kernel's own previous stages"""
    logits, val = ph.stage_tail(k.emb, k.xb, k.ao, p32)
    return dict(emb_attr=ph.stage_attr(attr, p32), qkv=ph.stage_qkv(k.xb, p32, 2), ao=ph.stage_attention(k.qkv), logits=logits, val=val)


@pytest.mark.parametrize("case", phs.STAGE_CASES)
def test_stages(case):
    """emb[:, :128] from attr, qkv from xb, ao from qkv, logits and val from (emb, xb, ao), value from val: each within its bound;
    emb[:, 128:] is tree and, with one agent, ao is v, bit for bit; two calls give the same bits in every stage; the actions are the
    restated choice on the kernel's logits.

    The cases synth_b1_a1 and synth_b3_a1 (the golden fixtures with ONE agent an env) are the verdict on one-agent envs: they
    replace the ratio to a single draw of the reference's float32 error, which tests/test_gpu_policy_head.py leaves above 4 on the
    value of synth_b3_a1, by a bound per element at every stage.

    sharp (block 2's q x 64: the row maximum decides everything): ao within its bound and finite.  flat (q = 0: every score
    equal): ao within the bound of the per-head mean of v -- a key past A that took part would move it by about A / 32.  constv
    (v = a constant vector c whatever the row): ao[:, j] within phs.constv_tolerance of c[j] whatever q and k are."""
    attr, tree, valid, plist, p64, p32 = _case(case)
    B, A = attr.shape[:2]
    k = phs.run(attr, tree, plist, valid, "soft")
    _sound(k)
    assert phs.same_bits(k, phs.run(attr, tree, plist, valid, "soft")) == []
    assert torch.equal(phs.bits(k.emb[..., 128:]), phs.bits(tree))
    if A == 1:
        assert torch.equal(k.ao, k.qkv[..., 512:])                  # one key: its probability is exactly 1
    checks = phs.stage_checks(k, attr, p64, C_ULPS)
    over = {n: phs.worst(*v) for n, v in checks.items()}
    figs, eager = {}, _eager32(k, attr, p32)
    for n, (got, ref, bound) in checks.items():
        if n in eager and got.numel() >= 4096:
            e_k, e_32 = phs.rms(got - ref), phs.rms(eager[n].double() - ref)
            figs[n] = dict(rms_ratio=e_k / e_32 if e_k > 0 else 0.0, max_over_bound=over[n])
    print(case, " ".join("%s %.3g" % kv for kv in over.items()), figs)
    util.record_errors("POLICY_HEAD_ERRORS", "stages", case, figs)
    assert all(w <= 1.0 for w in over.values()), over
    assert (k.actions.cpu().numpy() == ph.choose_actions(k.logits, valid, "soft")).all()
    if case.endswith("flat"):
        assert not bool(k.qkv[..., :256].any())
        mean_v = k.qkv[..., 512:].double().mean(dim=1, keepdim=True).expand(B, A, 256)
        assert float((checks["ao"][1] - mean_v).abs().max()) <= 1e-12
    if case.endswith("constv"):
        c = phs.pushed_params("constv", A)[1]
        assert torch.equal(k.qkv[..., 512:], c.to(DEV).expand(B, A, 256))
        err = (k.ao.double() - c.to(DEV).double()).abs()
        assert bool((err <= phs.constv_tolerance(c, A).to(DEV)).all()), float(err.max())


@pytest.mark.parametrize("B, A", [(5, 13), (2, 33)])
def test_workspace_hygiene(B, A):
    """a workspace of NaNs and one of zeros give the same bits in every stage and output (rows past `rows` of a tile and the
    clamped rows past A read nothing stale), and 4096 bytes behind the workspace stay untouched"""
    attr, tree, valid, plist, _, _ = _case("b%d_a%d-x1" % (B, A))
    nan, zero = phs.run(attr, tree, plist, valid, "hard", fill=0xFF), phs.run(attr, tree, plist, valid, "hard", fill=0x00)
    _sound(nan)
    _sound(zero)
    assert phs.same_bits(nan, zero) == []
    pad = nan.workspace[B * A * (7 * 256 + 1) * 4:]                     # the workspace's size is rounded up to 16 bytes
    assert bool((pad == 0xFF).all())


def test_side_stream():
    """the same call on a side stream gives the default stream's bits"""
    attr, tree, valid, plist, _, _ = _case("b2_a33-x1")
    ref = phs.run(attr, tree, plist, valid, "soft")
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        got = phs.run(attr, tree, plist, valid, "soft")
    torch.cuda.current_stream(DEV).wait_stream(s)
    s.synchronize()
    _sound(got)
    assert phs.same_bits(ref, got) == []


@pytest.mark.parametrize("vector", list(phs.CHOICE_VECTORS))
@pytest.mark.parametrize("B, A", phs.CHOICE_SHAPES)
def test_choice_on_constructed_logits(B, A, vector):
    """actor_net.4 = (0, a chosen bias): every row's logits are that vector bit for bit, and its float32 softmax is exact whatever
    expf is, so the kernel's CDF steps are the restatement's.  The rows carry the 32 valid-action masks.  For soft and hard, at
    every distinct CDF step below 1 of every mask, at its two float64 neighbours, at 0 and at the largest double below 1, the
    actions equal ph.choose_actions on EVERY row: exact ties take the first largest, zero-probability actions inside the CDF are
    stepped over, and a draw on a step goes to the next action (searchsorted side="right" is <=)."""
    attr, tree, _, plist, _, _ = _case("b%d_a%d-choice_%s" % (B, A, vector))
    masks = phs.choice_masks(B, A)
    valid = torch.from_numpy(masks).to(DEV)
    bias = torch.tensor(phs.CHOICE_VECTORS[vector], dtype=torch.float32)
    count = masks.sum(-1)
    only = masks.argmax(-1)
    for mode in ("soft", "hard"):
        for i, u in enumerate(phs.choice_draws(vector)):
            k = phs.run(attr, tree, plist, valid, mode, u=u)
            got = k.actions.cpu().numpy()
            if i == 0:
                assert torch.equal(phs.bits(k.logits.cpu()), phs.bits(bias.expand(B, A, 5)))
                _sound(k)
            assert (got == ph.choose_actions(bias.expand(B, A, 5), masks, mode, u=u)).all(), (mode, u)
            assert (got[count == 0] == 0).all() and (got[count == 1] == only[count == 1]).all(), (mode, u)
