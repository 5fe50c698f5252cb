"""CPU: what tests/test_gpu_policy_head_stages.py relies on, checked without a GPU.  The stage-wise restatement
(tests/policy_head_torch.py) chained in float64 is head() bit for bit; the a-priori bounds (tests/policy_head_bounds.py) hold for
two float32 restatements -- torch's eager ops, and every product summed strictly from the left -- on every case of the GPU tests
(a bound that a float32 reference breaks is a bug in the bound); the allowance C for erff / expf follows the error of torch's
float32 erf / exp measured over every case's arguments; the pushed-attention cases are as sharp and as spread as they are meant to
be; the constructed logits of the action-choice tests have an exact float32 softmax; the committed record of the MI355X figures is
complete."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import policy_head_bounds as pb
from tests import policy_head_stages as phs
from tests import policy_head_torch as ph
from tests import util

C_ULPS = pb.allowance()
SEQ_ROWS = 70          # the strictly sequential float32 restatement runs up to this many rows


@pytest.mark.parametrize("case", ["b3_a11-x0", "b5_a13-x1", "b70_a1-x1", "b2_a33-x1", "b1_a65-x0", "synth_b3_a1-x1", "b2_a33-sharp"])
def test_stages_chain_is_head(case):
    """chained from the inputs in float64 the stages give head()'s logits and value bit for bit (and head()'s probabilities)"""
    attr, tree, _, P = phs.CASES[case]()
    logits, value, probs = ph.head(attr, tree, P, with_probs=True)
    st = ph.stages(attr, tree, P)
    assert torch.equal(st["logits"], logits) and torch.equal(st["value"], value)
    assert torch.equal(ph.stage_attention(st["qkv"], with_probs=True)[1], probs[2])
    B, A = attr.shape[:2]
    assert {k: tuple(v.shape[2:]) for k, v in st.items() if k in phs.STAGES} == {n: (w,) if w > 1 else () for n, _, w in phs.LAYOUT}
    assert torch.equal(st["emb"][..., 128:], tree.double()) and st["val"].shape == (B, A)


def test_layout_is_the_documented_one():
    doc = open(os.path.join(util.ROOT, "DESIGN.md")).read()
    for name, off, n in phs.LAYOUT:
        assert re.search(r"\| `%s` \| %s \| \[R\]%s \|" % (name, "0" if off == 0 else "%d R" % off, r"\[%d\]" % n if n > 1 else ""), doc), name
    assert sum(n for _, _, n in phs.LAYOUT) == 7 * 256 + 1 and [o for _, o, _ in phs.LAYOUT] == [0, 256, 512, 768, 1024, 1792]


def test_matmul_seq_sums_from_the_left():
    a = torch.tensor([[1.0, 2.0 ** -24, 2.0 ** -24, -1.0]], dtype=torch.float32)
    ones = torch.ones((4, 1), dtype=torch.float32)
    assert float(ph.matmul_seq(a, ones)) == 0.0                       # ((1 + 2^-24) + 2^-24) - 1 with every sum rounded
    assert float(ph.matmul_seq(a.flip(1), ones)) == 2.0 ** -23        # ((-1 + 2^-24) + 2^-24) + 1 is exact
    x, w = torch.randn(3, 5, 7, dtype=torch.float64), torch.randn(3, 7, 4, dtype=torch.float64)
    assert float((ph.matmul_seq(x, w) - x @ w).abs().max()) < 1e-14


@pytest.mark.parametrize("case", list(phs.CASES))
def test_float32_restatements_stay_inside_the_bounds(case):
    """each float32 stage against the float64 restatement of it from the float32 restatement's own previous stage"""
    attr, tree, _, P = phs.CASES[case]()
    p64 = ph.stage_params(P, "cpu")
    R = attr.shape[0] * attr.shape[1]
    for label, mm in (("eager", torch.matmul), ("from the left", ph.matmul_seq)):
        if mm is ph.matmul_seq and R > SEQ_ROWS:
            continue
        st = ph.stages(attr, tree, P, dtype=torch.float32, mm=mm)
        for name, (got, ref, bound) in phs.stage_checks(st, attr, p64, C_ULPS).items():
            assert got.shape == ref.shape == bound.shape
            w = phs.worst(got, ref, bound)
            assert w <= 1.0, (case, label, name, w)
        if case.endswith("constv"):
            c = phs.pushed_params("constv", attr.shape[1])[1]
            assert ((st["ao"].double() - c.double()).abs() <= phs.constv_tolerance(c, attr.shape[1])).all(), (case, label)


def _ulp_errors(args32, fn):
    """the largest error of float32 fn over the float32 arguments, in ulps of max(|argument|, |result|) and in ulps of the result
    alone (where that is a normal number)"""
    got, ref = fn(args32).double(), fn(args32.double())
    err = (got - ref).abs()
    normal = ref.abs() >= 2.0 ** -126
    of_result = float(pb.ulps(err[normal], ref[normal]).max()) if bool(normal.any()) else 0.0
    return float(pb.ulps(err, args32.double(), ref).max()), of_result


def measure_activations():
    """over the erf and exp arguments of the float64 restatement of every case"""
    worst = dict(erf=0.0, exp=0.0, exp_of_result=0.0)
    for case, make in phs.CASES.items():
        attr, tree, _, P = make()
        rec = dict(erf=[], exp=[])
        ph.stages(attr, tree, P, rec=rec)
        e, _ = _ulp_errors(torch.cat([x.reshape(-1) for x in rec["erf"]]).float(), torch.erf)
        x, xr = _ulp_errors(torch.cat([x.reshape(-1) for x in rec["exp"]]).float(), torch.exp)
        worst = dict(erf=max(worst["erf"], e), exp=max(worst["exp"], x), exp_of_result=max(worst["exp_of_result"], xr))
    return worst


def test_allowance_follows_the_measured_errors():
    """C = twice the largest measured error (of the result alone for exp, the larger figure: eta takes C u relative to exp's result),
    rounded up, at least 4 -- on the record, and no smaller than what this machine's torch gives"""
    rec = json.load(open(pb.RECORD))
    assert rec["c"] == C_ULPS == pb.allowance_of(max(rec["measured_ulps"].values())) >= 4
    now = measure_activations()
    print("measured", now, "recorded", rec["measured_ulps"])
    assert pb.allowance_of(max(now.values())) <= C_ULPS, now


@pytest.mark.parametrize("B, A", phs.PUSHED_SHAPES)
def test_sharp_case_is_sharp_and_spread(B, A):
    """the float64 reference of the sharp case: the mean largest probability is at least 0.9 (at every seed of the case), and the
    winning keys fall in every 32-key chunk, the partial last one included (at A = 1024: those of the case's three seeds together);
    the flat case: every probability is 1 / A"""
    chunks = set()
    for cid in phs.sharp_cases(B, A):
        attr, tree, _, P = phs.CASES[cid]()
        pr = ph.stage_attention(ph.stages(attr, tree, P)["qkv"], with_probs=True)[1]
        top = pr.max(dim=-1)
        assert float(top.values.mean()) >= 0.9
        chunks |= set((top.indices.reshape(-1) // 32).tolist())
    assert chunks == set(range((A + 31) // 32)) and (len(phs.sharp_cases(B, A)) == 1 or A == 1024)
    attr, tree, _, P = phs.CASES["b%d_a%d-flat" % (B, A)]()
    st = ph.stages(attr, tree, P)
    pr = ph.stage_attention(st["qkv"], with_probs=True)[1]
    assert float((pr - 1.0 / A).abs().max()) <= 1e-15 and not bool(st["qkv"][..., :256].any())
    mean_v = st["qkv"][..., 512:].mean(dim=1, keepdim=True).expand(B, A, 256)
    assert float((st["ao"] - mean_v).abs().max()) <= 1e-13


def test_constructed_logits_have_an_exact_softmax():
    """differences of 0 or at least 200: exp is exactly 1 or exactly 0 in float32, so p = 1 / n on the largest valid logits and 0
    elsewhere, and the CDF's steps are multiples of 1 / n"""
    assert float(np.exp(np.float32(-phs.BIG))) == 0.0 and math.exp(-phs.BIG) < 2.0 ** -150 * 1e-20
    assert len(phs.CHOICE_VECTORS) == 10
    calls = 0
    for name, vec in phs.CHOICE_VECTORS.items():
        lg = np.array(vec, dtype=np.float32)
        d = np.abs(lg[:, None] - lg[None, :])
        assert ((d == 0) | (d >= 200)).all()
        for m in phs.MASKS[1:]:
            idx, pr = ph._probabilities(lg, m)
            top = lg[idx] == lg[idx].max()
            assert (pr[top] == np.float32(1.0) / np.float32(top.sum())).all() and (pr[~top] == 0).all()
        us = phs.choice_draws(name)
        assert us[0] == 0.0 and us[-1] == np.nextafter(1.0, 0.0) and all(0.0 <= u < 1.0 for u in us)
        calls += 2 * len(us) * len(phs.CHOICE_SHAPES)
    assert calls <= 700, calls                 # about a millisecond each
    # zero-probability actions inside the CDF and at both ends, steps that are hit exactly, ties
    assert ph.cdf_of(np.array(phs.CHOICE_VECTORS["holes"], np.float32), phs.MASKS[31]).tolist() == [1 / 3, 1 / 3, 2 / 3, 2 / 3, 1.0]
    assert ph.cdf_of(np.array(phs.CHOICE_VECTORS["holes_complement"], np.float32), phs.MASKS[31]).tolist() == [0.0, 0.5, 0.5, 1.0, 1.0]
    assert 0.5 in phs.choice_draws("tie_0_3") and 1 / 3 in phs.choice_draws("holes") and 0.2 in phs.choice_draws("equal")
    assert phs.choice_masks(2, 33).reshape(-1, 5)[32:35].tolist() == phs.MASKS[0:3].tolist()


def test_record_is_complete():
    """the committed MI355X figures: for every stage case, every checked stage of at least 4096 outputs"""
    rec = json.load(open(pb.RECORD))
    assert set(rec["stages"]) == set(phs.STAGE_CASES)
    for case, figs in rec["stages"].items():
        attr = phs.CASES[case]()[0]
        R = attr.shape[0] * attr.shape[1]
        want = {n for n, w in (("emb_attr", 128), ("qkv", 768), ("ao", 256), ("logits", 5), ("val", 1)) if R * w >= 4096}
        assert set(figs) == want, case
        for f in figs.values():
            assert 0.0 <= f["max_over_bound"] <= 1.0 and f["rms_ratio"] >= 0.0


if __name__ == "__main__":      # python -m tests.test_policy_head_stages: measure the activations again and put them and C on the record
    rec = json.load(open(pb.RECORD)) if os.path.exists(pb.RECORD) else dict(stages={})
    rec["measured_ulps"] = measure_activations()
    rec["c"] = pb.allowance_of(max(rec["measured_ulps"].values()))
    json.dump(rec, open(pb.RECORD, "w"), indent=1, sort_keys=True)
    print(rec["measured_ulps"], "c =", rec["c"])
