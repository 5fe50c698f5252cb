"""CPU: the PPO entry points (include/flatland_ppo.h) -- the header, the binding and the library agree; every refusal, called
through ctypes without a device (the refusals come before any HIP call); the byte function; and the numpy restatements of
tests/ppo_np.py pinned: the draw to the reference actor's actions of the fixtures, the closed-form gradients to torch's float64
autograd of the plain formula, GAE to an independent evaluation.  The kernels themselves: tests/test_gpu_ppo.py."""
import functools
import glob
import math
import os
import re

import numpy as np
import pytest

from flatland_marl_amd import hip_backend as hb
from tests import cabi
from tests import policy_head_torch as pht
from tests import ppo_np as pn
from tests import util

NAMES = ["fl_policy_sample", "fl_ppo_loss_workspace_bytes", "fl_ppo_loss", "fl_gae"]
OK = 0x10000          # a pointer that is there and 16-byte aligned; no refused call reads it
ODD = OK + 4
MAX_ROWS = 1 << 28    # FL_PPO_MAX_ROWS
FIXTURES = sorted(glob.glob(os.path.join(util.ROOT, "tests", "golden", "policy_head_*.npz")))


def kernel_constant(name):
    """the integer of `#define name value` in csrc/fl_ppo.h, comments apart (tests/cabi.py reads the public headers the same way)"""
    src = open(os.path.join(util.ROOT, "flatland_marl_amd", "csrc", "fl_ppo.h")).read()
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", src, flags=re.S))
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(\d+)[ \t]*$" % name, src, re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


FPP_THREADS = kernel_constant("FPP_THREADS")
FPP_COUNT_GROUPS = kernel_constant("FPP_COUNT_GROUPS")
FPP_SUMS = kernel_constant("FPP_SUMS")
E1 = FPP_THREADS * FPP_THREADS            # the last row count at which fpp_counts and k_ppo_final add their slots in a single trip
E2 = FPP_COUNT_GROUPS * FPP_THREADS       # the last row count at which k_ppo_count does not stride
# (R, B) past each edge and what takes its first second trip there; tests/test_gpu_ppo.py runs the kernels on them
LARGE_CASES = (
    (E1, 3),                # nothing: the last single-trip size, the control
    (E1 + 1, 257),          # fpp_counts and k_ppo_final: 257 groups, 257 count groups
    (102400, 256),          # the shape tools/ppo_bench.py times as cfg5: 400 groups
    (E2, 1),                # FPP_COUNT_GROUPS groups: four trips of the slot loops, no stride yet
    (E2 + 1, 257),          # k_ppo_count strides for one row only; one more sum slot than count slots
    (3 * E2 + 1, 3),        # three full strides and a ragged fourth
    (1, E1 + 1),            # groups set by the values: 257 sum slots, one count slot, 256 workgroups without a row
    (300, E1 + 1),          # the same with two row workgroups
)
LARGE_SEED = 4
PLACE_R, PLACE_B = 2 * E2 + 1, 3          # the placement cases: two full strides of k_ppo_count and one row of a third
PLACE_ROWS = (0, E1 - 1, E1, E2 - 1, E2, PLACE_R - 1)


def test_header_binding_and_library_agree():
    """what is this header's own; names in order against the table, types, counts, exports: tests/test_cabi_headers.py"""
    hb.build()                                                             # (the tests below call the library)
    decls = cabi.declarations("flatland_ppo.h")
    assert [n for _, n, _ in decls] == list(hb.symbols("flatland_ppo.h")) == NAMES
    assert '#include "flatland_policy.h"' in cabi.text("flatland_ppo.h")
    params = {n: ps for _, n, ps in decls}
    assert params["fl_policy_sample"] == [
        "int n_rows", "const float *logits_dev", "const uint8_t *valid_dev", "const double *u_dev", "uint8_t *actions_dev",
        "float *logp_dev", "float *entropy_dev", "void *hip_stream"]
    assert params["fl_ppo_loss"] == [
        "int n_rows", "int n_envs", "const float *logits_dev", "const uint8_t *valid_dev", "const uint8_t *actions_dev",
        "const float *old_logp_dev", "const float *adv_dev", "const uint8_t *mask_dev", "const float *value_dev",
        "const float *returns_dev", "double clip_eps", "double vf_coef", "double ent_coef", "float *grad_logits_dev",
        "float *grad_value_dev", "double *stats_dev", "void *workspace_dev", "size_t workspace_bytes", "void *hip_stream"]
    assert params["fl_gae"] == [
        "int n_steps", "int n_cols", "const float *rewards_dev", "const float *values_dev", "const uint8_t *dones_dev", "double gamma",
        "double lam", "float *adv_dev", "float *returns_dev", "void *hip_stream"]
    assert callable(hb.policy_sample) and callable(hb.ppo_loss) and callable(hb.gae)
    from flatland_marl_amd import policy
    for name in ("sample_actions", "ppo_loss", "gae"):
        assert callable(getattr(policy, name))
    assert callable(policy.Network.rollout)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(name, args, *needles):
    rc = hb._sym(name)(*args)
    assert rc == 1, (name, needles, rc)                              # FL_ERR_ARG
    msg = hb.lib().fl_last_error().decode()
    assert msg.startswith(name + ": "), msg
    for needle in needles:
        assert needle in msg, msg


def _sample_args(**over):
    a = dict(n_rows=7, logits=OK, valid=OK, u=OK, actions=OK, logp=OK, entropy=OK)
    a.update(over)
    return [a[k] for k in ("n_rows", "logits", "valid", "u", "actions", "logp", "entropy")] + [None]


def test_policy_sample_refusals():
    for n in (0, -1, MAX_ROWS + 1):
        _refused("fl_policy_sample", _sample_args(n_rows=n), "n_rows")
    for arg in ("logits", "valid", "u", "actions"):
        _refused("fl_policy_sample", _sample_args(**{arg: None}), arg, "NULL")
    for arg in ("logits", "u", "logp", "entropy"):
        _refused("fl_policy_sample", _sample_args(**{arg: ODD}), arg, "aligned")


LOSS_ORDER = ("n_rows", "n_envs", "logits", "valid", "actions", "old_logp", "adv", "mask", "value", "returns", "clip_eps", "vf_coef",
              "ent_coef", "grad_logits", "grad_value", "stats", "workspace", "workspace_bytes")


def _loss_args(**over):
    a = dict(n_rows=300, n_envs=3, logits=OK, valid=OK, actions=OK, old_logp=OK, adv=OK, mask=OK, value=OK, returns=OK, clip_eps=0.2,
             vf_coef=0.5, ent_coef=0.01, grad_logits=OK, grad_value=OK, stats=OK, workspace=OK, workspace_bytes=1 << 20)
    a.update(over)
    return [a[k] for k in LOSS_ORDER] + [None]


def test_ppo_loss_refusals():
    fn = "fl_ppo_loss"
    for over in (dict(n_rows=0), dict(n_rows=-3), dict(n_envs=-1), dict(n_envs=0), dict(n_rows=MAX_ROWS + 1), dict(n_envs=MAX_ROWS + 1)):
        _refused(fn, _loss_args(**over), "n_rows", "n_envs")
    for arg in ("logits", "valid", "actions", "old_logp", "adv", "grad_logits", "stats", "workspace"):
        _refused(fn, _loss_args(**{arg: None}), arg, "NULL")
    for missing in (("value",), ("returns",), ("grad_value",), ("value", "returns"), ("value", "grad_value"), ("returns", "grad_value")):
        _refused(fn, _loss_args(**{k: None for k in missing}), "value", "returns", "grad_value")
    for arg in ("clip_eps", "vf_coef", "ent_coef"):
        for bad in (math.nan, math.inf, -math.inf):
            _refused(fn, _loss_args(**{arg: bad}), arg, "finite")
    _refused(fn, _loss_args(clip_eps=-1e-9), "clip_eps")
    for arg in ("logits", "old_logp", "adv", "value", "returns", "grad_logits", "grad_value", "stats", "workspace"):
        _refused(fn, _loss_args(**{arg: ODD}), arg, "aligned")
    _refused(fn, _loss_args(stats=OK + 8), "stats", "aligned")       # a double pointer on 8 bytes is not enough
    need = hb._sym("fl_ppo_loss_workspace_bytes")(300, 3)
    assert need > 0
    _refused(fn, _loss_args(workspace_bytes=need - 1), "workspace", "fl_ppo_loss_workspace_bytes", str(need))
    _refused(fn, _loss_args(workspace_bytes=0), "workspace")
    none = dict(value=None, returns=None, grad_value=None)
    short = hb._sym("fl_ppo_loss_workspace_bytes")(300, 0)
    assert 0 < short <= need
    _refused(fn, _loss_args(n_envs=0, workspace_bytes=short - 1, **none), "workspace")     # n_envs 0 is a size, not a refusal, here
    _refused(fn, _loss_args(n_envs=0, workspace_bytes=short - 1, mask=None, **none), "workspace")


def _gae_args(**over):
    a = dict(n_steps=4, n_cols=9, rewards=OK, values=OK, dones=OK, gamma=0.99, lam=0.95, adv=OK, returns=OK)
    a.update(over)
    return [a[k] for k in ("n_steps", "n_cols", "rewards", "values", "dones", "gamma", "lam", "adv", "returns")] + [None]


def test_gae_refusals():
    for over in (dict(n_steps=0), dict(n_steps=-1), dict(n_cols=0), dict(n_cols=-5), dict(n_cols=MAX_ROWS + 1)):
        _refused("fl_gae", _gae_args(**over), "n_steps", "n_cols")
    for arg in ("rewards", "values", "dones", "adv", "returns"):
        _refused("fl_gae", _gae_args(**{arg: None}), arg, "NULL")
    for arg in ("gamma", "lam"):
        for bad in (math.nan, math.inf, -math.inf, -1e-9, 1.0 + 1e-9):
            _refused("fl_gae", _gae_args(**{arg: bad}), arg)
    for arg in ("rewards", "values", "adv", "returns"):
        _refused("fl_gae", _gae_args(**{arg: ODD}), arg, "aligned")


def test_workspace_bytes():
    fn = hb._sym("fl_ppo_loss_workspace_bytes")
    for rows, envs in ((0, 1), (-1, 1), (0, 0), (5, -1), (-5, -5), (MAX_ROWS + 1, 1), (5, MAX_ROWS + 1)):
        assert fn(rows, envs) == 0
    sizes = (1, 255, 256, 257, 1025, 5120, 102400, 300000, 3000000, MAX_ROWS)
    for envs in (0, 1, 3, 257, 100000):
        got = [fn(r, envs) for r in sizes]
        assert all(g > 0 and g % 16 == 0 for g in got)
        assert all(a <= b for a, b in zip(got, got[1:])), (envs, got)
    for rows in sizes:
        got = [fn(rows, e) for e in (0, 1, 3, 256, 257, 513, 100000, 5000000, MAX_ROWS)]
        assert all(a <= b for a, b in zip(got, got[1:])), (rows, got)
    # a workgroup's five float64 sums and the count kernel's two integers per workgroup
    assert fn(1, 1) == 48 and fn(257, 1) == 96 and fn(1, 257) == 96


def test_workspace_bytes_at_the_kernels_own_edges():
    """E1, E2 and the sizes of LARGE_CASES come from FPP_THREADS and FPP_COUNT_GROUPS of csrc/fl_ppo.h; the library's byte function
    shows the same groups and the same cap.  If a constant moves, the literals here name what moves with it"""
    assert (FPP_THREADS, FPP_COUNT_GROUPS, FPP_SUMS) == (256, 1024, 5) and (E1, E2) == (65536, 262144)
    fn = hb._sym("fl_ppo_loss_workspace_bytes")
    sums, counts = FPP_SUMS * 8, 2 * 4                                  # a workgroup's float64 sums, a count workgroup's two integers
    assert (sums, counts) == (40, 8)
    up16 = lambda n: (n + 15) // 16 * 16                                # noqa: E731
    assert fn(E2, 0) == 1024 * 40 + 1024 * 8 == FPP_COUNT_GROUPS * (sums + counts)
    assert fn(E2 + 1, 0) == up16(1025 * 40 + 1024 * 8) == up16((FPP_COUNT_GROUPS + 1) * sums + FPP_COUNT_GROUPS * counts)   # the cap holds
    assert fn(3 * E2 + 1, 0) == up16((3 * FPP_COUNT_GROUPS + 1) * sums + FPP_COUNT_GROUPS * counts)
    assert fn(1, E1 + 1) == up16(257 * 40 + 8) == up16((FPP_THREADS + 1) * sums + counts)       # 257 groups, one count group
    assert fn(E1, 0) == FPP_THREADS * (sums + counts) and fn(E1 + 1, 0) == up16((FPP_THREADS + 1) * (sums + counts))
    for R, B in LARGE_CASES:
        groups = max(-(-R // FPP_THREADS), -(-B // FPP_THREADS))
        assert fn(R, B) == up16(groups * sums + min(-(-R // FPP_THREADS), FPP_COUNT_GROUPS) * counts), (R, B)
    assert any(-(-R // FPP_THREADS) > FPP_COUNT_GROUPS for R, _ in LARGE_CASES)
    assert any(-(-B // FPP_THREADS) > FPP_THREADS >= -(-R // FPP_THREADS) for R, B in LARGE_CASES)


# ---------------------------------------------------------------------------------------------------------------- the restatements
def loss_inputs(R, B, seed, scale=1.0):
    """seeded inputs of the loss with every kind of row: no valid action, a single one, masked, an action that is not valid (masked
    out and >= 5), both clip sides on both signs of A, A = 0"""
    rng = np.random.default_rng([seed, R, B])
    logits = (scale * rng.standard_normal((R, 5))).astype(np.float32)
    valid = rng.integers(0, 2, size=(R, 5)).astype(np.uint8)
    kind = (np.arange(R) + seed) % 8
    valid[kind == 0] = 0
    valid[kind == 1] = 0
    valid[kind == 1, rng.integers(0, 5, size=int((kind == 1).sum()))] = 1
    valid[(kind > 1) & (valid.sum(axis=1) == 0), 2] = 1
    actions, logp, _ = pn.sample(logits, valid, rng.random(R))
    actions = actions.copy()
    bad = np.flatnonzero(kind == 2)
    for i, r in enumerate(bad):
        off = np.flatnonzero(valid[r] == 0)
        actions[r] = off[0] if len(off) and i % 2 == 0 else 5 + i % 250
    old_logp = (logp + 0.3 * rng.standard_normal(R)).astype(np.float32)
    adv = rng.standard_normal(R).astype(np.float32)
    adv[kind == 3] = 0.0
    mask = (rng.random(R) < 0.8).astype(np.uint8)
    value = rng.standard_normal(B).astype(np.float32)
    returns = rng.standard_normal(B).astype(np.float32)
    return dict(logits=logits, valid=valid, actions=actions, old_logp=old_logp, adv=adv, mask=mask, value=value, returns=returns)


def off_the_clip_boundary(x, clip):
    """every counted row's rho at least 1e-9 away from 1 - clip and 1 + clip: the device's exp may differ from numpy's in the last
    bit, and a row on the boundary would test the libm, not the kernel"""
    rho = pn.ratio(x["logits"], x["valid"], x["actions"], x["old_logp"])
    w, _ = pn.weights(x["valid"], x["actions"], x["mask"])
    return bool((np.minimum(np.abs(rho[w] - (1.0 - clip)), np.abs(rho[w] - (1.0 + clip))) >= 1e-9).all())


def loss_inputs_large(R, B, seed, well_formed=False):
    """loss_inputs's kinds of row (by row index mod 8: no valid action, a single one, an action that is not valid -- masked out or
    >= 5 --, A = 0; about one row in five masked) without a Python loop over rows, for the sizes of LARGE_CASES.  Its own bits, not
    loss_inputs's: the action is a uniform draw among the valid ones, not pn.sample's.  well_formed: every row has a valid action
    and takes one, and mask is 1 everywhere (the single-action rows of kind 1 and the A = 0 rows stay; every other row has two
    valid actions or more, so its gradient row is not zero)"""
    rng = np.random.default_rng([seed, R, B, 1])
    logits = rng.standard_normal((R, 5), dtype=np.float32)
    valid = rng.integers(0, 2, size=(R, 5), dtype=np.uint8)
    kind = (np.arange(R) + seed) % 8
    valid[kind == 1] = 0
    one = np.flatnonzero(kind == 1)
    valid[one, rng.integers(0, 5, size=len(one))] = 1
    valid[(kind != 1) & (valid.sum(axis=1) == 0), 2] = 1
    if well_formed:                                                  # only the rows of kind 1 have a single action: theirs is a zero gradient
        few = (kind != 1) & (valid.sum(axis=1) < 2)
        valid[few, 1] = valid[few, 3] = 1
    nth =(rng.random(R) * valid.sum(axis=1)).astype(np.int64)       # the nth valid action of the row, n uniform
    actions = ((valid != 0) & (np.cumsum(valid, axis=1) - 1 == nth[:, None])).argmax(axis=1).astype(np.uint8)
    logp = pn.log_softmax(logits, valid)[0][np.arange(R), actions]
    old_logp = (logp + 0.3 * rng.standard_normal(R)).astype(np.float32)
    adv = rng.standard_normal(R, dtype=np.float32)
    adv[kind == 3] = 0.0
    mask = (rng.random(R) < 0.8).astype(np.uint8)
    value = rng.standard_normal(B, dtype=np.float32)
    returns = rng.standard_normal(B, dtype=np.float32)
    if well_formed:
        mask[:] = 1
    else:
        valid[kind == 0] = 0
        actions[kind == 0] = 0
        bad = np.flatnonzero(kind == 2)
        i = np.arange(len(bad))
        off = valid[bad] == 0
        actions[bad] = np.where(off.any(axis=1) & (i % 2 == 0), off.argmax(axis=1), 5 + i % 250).astype(np.uint8)
    return dict(logits=logits, valid=valid, actions=actions, old_logp=old_logp, adv=adv, mask=mask, value=value, returns=returns)


@functools.lru_cache(maxsize=2)
def large_inputs(R, B, well_formed=False):
    """loss_inputs_large at LARGE_SEED, built once for the tests that share a size, read-only so that it stays as it was built"""
    x = loss_inputs_large(R, B, LARGE_SEED, well_formed)
    for a in x.values():
        a.setflags(write=False)
    return x


def test_large_inputs_hold_every_kind_of_row():
    R, B = E1 + 1, 257
    x = large_inputs(R, B)
    w, bad = pn.weights(x["valid"], x["actions"], x["mask"])
    nv = (x["valid"] != 0).sum(axis=1)
    assert (nv == 0).any() and (nv == 1).any() and 0.15 * R < (x["mask"] == 0).sum() < 0.25 * R
    masked_out = (x["actions"] < 5) & (x["valid"][np.arange(R), np.minimum(x["actions"], 4)] == 0) & (nv > 0)
    assert (bad & masked_out).any() and (bad & (x["actions"] >= 5)).any() and x["actions"].max() > 250
    assert (w & (x["adv"] == 0)).any() and (w & (nv == 1)).any() and 0 < w.sum() < R and bad.sum() > 0
    rho, A = pn.ratio(x["logits"], x["valid"], x["actions"], x["old_logp"])[w], x["adv"][w].astype(np.float64)
    for sign in (A > 0, A < 0):
        assert (sign & (rho > 1.2)).any() and (sign & (rho < 0.8)).any() and (sign & (np.abs(rho - 1) < 0.2)).any()
    # every 256-row group and every lane takes part, so a slot that is dropped changes the sums
    assert (np.add.reduceat(w, np.arange(0, R, FPP_THREADS)) > 0).all()
    # well formed: every row counts once the mask says so
    y = large_inputs(PLACE_R, PLACE_B, True)
    w, bad = pn.weights(y["valid"], y["actions"], y["mask"])
    nv = (y["valid"] != 0).sum(axis=1)
    assert w.all() and not bad.any() and (nv == 1).any() and (y["adv"] == 0).any() and (nv[list(PLACE_ROWS)] >= 2).all()
    assert off_the_clip_boundary(y, 0.2)


@pytest.mark.parametrize("R,B", LARGE_CASES)
def test_large_inputs_are_off_the_clip_boundary(R, B):
    """a condition of the GPU comparison (tests/test_gpu_ppo.py asserts it again on what it runs), with the mask on and, as
    check_loss asks, with every row's mask set; and the row counts the GPU cases rely on"""
    x = large_inputs(R, B)
    assert off_the_clip_boundary(x, 0.2) and off_the_clip_boundary(dict(x, mask=np.ones(R, dtype=np.uint8)), 0.2)
    for mask in (x["mask"], None):
        w, bad = pn.weights(x["valid"], x["actions"], mask)
        assert w.sum() >= 1                                            # (the single row of R = 1 counts)
        if R > FPP_THREADS:
            assert 0 < w.sum() < R and bad.sum() > 0
    assert len(x["value"]) == B and x["logits"].shape == (R, 5) and x["logits"].dtype == np.float32


def test_closed_form_gradients_are_torch_autograd_past_256_groups():
    x = large_inputs(E1 + 1, 257)
    out = pn.ppo_loss(clip=0.2, vf_coef=0.5, ent_coef=0.01, **x)
    total, leaf, v = pn.plain_loss_torch(clip=0.2, vf_coef=0.5, ent_coef=0.01, **x)
    total.backward()
    w, bad = pn.weights(x["valid"], x["actions"], x["mask"])
    assert np.abs(out["grad_logits"] - leaf.grad.numpy()).max() <= 1e-15
    assert np.abs(out["grad_value"] - v.grad.numpy()).max() <= 1e-15
    assert abs(out["stats"][3] - float(total.detach())) <= 1e-13
    assert out["stats"][6] == w.sum() and out["stats"][7] == bad.sum()
    assert (out["grad_logits"][x["valid"] == 0] == 0).all() and (out["grad_logits"][~w] == 0).all()


@pytest.mark.parametrize("R,B,seed,clip,ent", ((4099, 7, 1, 0.2, 0.01), (257, 3, 2, 0.1, 0.0), (64, 1, 3, 0.3, 0.5), (1025, 257, 4, 0.2, 0.01)))
def test_closed_form_gradients_are_torch_autograd(R, B, seed, clip, ent):
    x = loss_inputs(R, B, seed)
    assert off_the_clip_boundary(x, clip)
    out = pn.ppo_loss(clip=clip, vf_coef=0.5, ent_coef=ent, **x)
    w, bad = pn.weights(x["valid"], x["actions"], x["mask"])
    rho, A = out["rho"][w], x["adv"][w].astype(np.float64)
    # the inputs hold what they promise
    assert (x["valid"].sum(axis=1) == 0).any() and (x["valid"].sum(axis=1) == 1).any() and (x["mask"] == 0).any() and bad.any()
    assert (x["actions"] >= 5).any() and (A == 0).any()
    if R >= 257:
        for sign in (A > 0, A < 0):
            assert (sign & (rho > 1 + clip)).any() and (sign & (rho < 1 - clip)).any() and (sign & (np.abs(rho - 1) < clip)).any()
    total, leaf, v = pn.plain_loss_torch(clip=clip, vf_coef=0.5, ent_coef=ent, **x)
    total.backward()
    assert np.abs(out["grad_logits"] - leaf.grad.numpy()).max() <= 1e-15
    assert np.abs(out["grad_value"] - v.grad.numpy()).max() <= 1e-15
    assert abs(out["stats"][3] - float(total.detach())) <= 1e-13
    assert out["stats"][6] == w.sum() and out["stats"][7] == bad.sum()
    assert (out["grad_logits"][x["valid"] == 0] == 0).all() and (out["grad_logits"][~w] == 0).all()


def test_closed_form_gradients_without_a_counted_row_or_a_critic():
    x = loss_inputs(130, 3, 5)
    x["mask"][:] = 0
    out = pn.ppo_loss(**x)
    total, leaf, v = pn.plain_loss_torch(**x)
    total.backward()
    assert out["stats"][6] == 0 and (out["grad_logits"] == 0).all() and (leaf.grad.numpy() == 0).all()
    assert (out["stats"][[0, 2, 4, 5, 7]] == 0).all() and np.isfinite(out["stats"]).all()
    assert np.abs(out["grad_value"] - v.grad.numpy()).max() <= 1e-15
    x = loss_inputs(130, 3, 6)
    x["value"] = x["returns"] = None
    out = pn.ppo_loss(**x)
    total, leaf, v = pn.plain_loss_torch(**x)
    total.backward()
    assert v is None and out["grad_value"] is None and out["stats"][1] == 0
    assert np.abs(out["grad_logits"] - leaf.grad.numpy()).max() <= 1e-15


def test_sampling_restatement_is_the_reference_actor_on_the_fixtures():
    assert len(FIXTURES) >= 10
    agents = 0
    for path in FIXTURES:
        z = np.load(path)
        for k in range(z["logits"].shape[0]):
            actions, logp, H = pn.sample(z["logits"][k], z["valid"], pht.U_REFERENCE)
            assert np.array_equal(actions.reshape(z["soft"][k].shape), z["soft"][k]), path
            assert np.array_equal(actions.reshape(z["soft"][k].shape), pht.choose_actions(z["logits"][k], z["valid"], "soft"))
            assert np.isfinite(logp).all() and (logp <= 0).all() and (H >= 0).all() and (H <= math.log(5) + 1e-12).all()
            agents += actions.size
    assert agents == 2290


def test_sampling_restatement_log_probabilities():
    rng = np.random.default_rng(11)
    logits = (30 * rng.standard_normal((500, 5))).astype(np.float32)
    valid = rng.integers(0, 2, size=(500, 5)).astype(np.uint8)
    actions, logp, H = pn.sample(logits, valid, rng.random(500))
    lp, p, H2, _ = pn.log_softmax(logits, valid)
    some = valid.any(axis=1)
    assert np.allclose(p.sum(axis=1)[some], 1.0, atol=1e-15) and (p[valid == 0] == 0).all()
    assert (valid[np.arange(500), actions][some] == 1).all() and (actions[~some] == 0).all()
    assert (logp[~some] == 0).all() and (H[~some] == 0).all()
    single = valid.sum(axis=1) == 1
    assert single.any() and (logp[single] == 0).all() and (H[single] == 0).all()
    with np.errstate(divide="ignore"):
        ref = np.log(p[np.arange(500), actions][some])
    assert np.abs(logp[some] - ref)[np.isfinite(ref)].max() <= 1e-12


@pytest.mark.parametrize("gamma,lam", ((0.0, 0.0), (0.95, 0.95), (1.0, 1.0), (0.99, 0.0), (1.0, 0.95)))
def test_gae_restatement(gamma, lam):
    rng = np.random.default_rng(21)
    T, N = 40, 17
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = rng.standard_normal((T + 1, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.1).astype(np.uint8)
    adv, ret, A = pn.gae(r, v, d, gamma, lam)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    assert np.abs(A - pn.gae_direct(r, v, d, gamma, lam)).max() <= 1e-13
    assert np.array_equal(adv, A.astype(np.float32)) and np.array_equal(ret, (A + v[:-1].astype(np.float64)).astype(np.float32))
    # a done cuts the column: the steps up to it do not see what follows
    v2, r2 = v.copy(), r.copy()
    t0 = int(np.flatnonzero(d[:, 0])[0]) if d[:, 0].any() else None
    if t0 is not None:
        v2[t0 + 1:, 0] += 5.0
        r2[t0 + 1:, 0] -= 3.0
        assert np.array_equal(pn.gae(r2, v2, d, gamma, lam)[2][:t0 + 1, 0], A[:t0 + 1, 0])
