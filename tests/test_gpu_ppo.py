"""GPU: the PPO entry points (include/flatland_ppo.h) against the float64 restatements of tests/ppo_np.py -- fl_policy_sample,
fl_ppo_loss and fl_gae through ctypes with every output and the workspace in guarded buffers, two calls that must give equal bits --
and the modules on top of them: policy.sample_actions, policy.ppo_loss, policy.gae, Network.rollout.

Tolerances (none fitted to the kernels): logp, entropy and the gradients are float32 roundings of float64 values, so one float32 ulp
of the restatement's value, plus the float64 evaluation's own error: 1e-12 times the magnitude of what an element is formed from
(float64 roundoff is 1.1e-16, the device's exp / log are within a few float64 ulps, the log-softmax is conditioned by the logit
spread, <= ~100 here: two orders of margin).  The statistics are float64 sums: 1e-12 of the mean of the absolute row terms.  The
actions are the restatement's except where policy_head_torch.exempt allows the float32 expf of record to differ (at most 1 % of a
case's rows, counted); fl_gae is bit for bit.

The loss at training sizes (LARGE_CASES of tests/test_ppo.py, from the kernel's own constants): three loops of csrc/fl_ppo.h take one
trip at every row count up to 65 536 -- fpp_counts over the count slots, k_ppo_final over the sum slots, k_ppo_count over the rows --
so the cases up to 1 025 rows cannot tell a wrong bound, stride or slot index in them.  The same tolerances hold there by derivation,
not by fit: a float64 sum of n <= 8e5 terms, in the kernel's fixed tree or in numpy's pairwise order, errs by at most about
log2(n) * 1.1e-16 * sum |t|, that is 2e-15 times the mean absolute term, three orders of magnitude under the 1e-12 the statistics are
held to; a gradient element is one row's float64 value divided by n and rounded to float32 at any size.  The placement cases count
one row at a time, so that a dropped, doubled or misplaced slot changes an integer and not a rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

from flatland_marl_amd import hip_backend as hb
from tests import policy_head_bounds as pb
from tests import policy_head_torch as pht
from tests import ppo_np as pn
from tests import util
from tests.test_policy_head_golden import NAMES, golden_inputs, golden_params, load
from tests.test_ppo import (E1, E2, FPP_THREADS, LARGE_CASES, PLACE_B, PLACE_R, PLACE_ROWS, large_inputs, loss_inputs,
                            off_the_clip_boundary)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 4096
ROWS = (1, 63, 64, 65, 255, 256, 257, 1025)
EPS = pb.allowance() * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- helpers
def _guarded(nbytes):
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    buf[:nbytes].fill_(0xFF)
    buf[nbytes:].fill_(0xA5)
    return buf


def _out(shape, dtype):
    """a guarded 0xFF buffer and its typed view (0xFF: NaN as a float or double, 255 as an action)"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = _guarded(n)
    return buf, buf[:n].view(dtype).view(shape)


def _intact(*outs):
    torch.cuda.synchronize()
    for buf, view in outs:
        assert bool((buf[view.numel() * view.element_size():] == 0xA5).all()), "a guard was written"


def _dev(a):
    return None if a is None else torch.from_numpy(np.require(a, requirements="CW")).to(DEV)     # (a shared, read-only input: a copy)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _on_side_stream(fn):
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def raw_sample(logits, valid, u, logp=True, entropy=True):
    """fl_policy_sample twice on guarded outputs: (actions u8 [R], logp f32 [R] or None, entropy f32 [R] or None) as numpy"""
    R = len(u)
    lg, va, ud = _dev(np.asarray(logits, dtype=np.float32).reshape(R, 5)), _dev(np.asarray(valid, dtype=np.uint8).reshape(R, 5)), \
        _dev(np.asarray(u, dtype=np.float64))
    runs = []
    for _ in range(2):
        a, lp, h = _out((R,), torch.uint8), _out((R,), torch.float32) if logp else None, _out((R,), torch.float32) if entropy else None
        with torch.cuda.device(DEV):
            rc = hb._sym("fl_policy_sample")(R, lg.data_ptr(), va.data_ptr(), ud.data_ptr(), a[1].data_ptr(),
                                             _ptr(lp and lp[1]), _ptr(h and h[1]), _stream())
        assert rc == 0, hb.lib().fl_last_error().decode()
        _intact(*[o for o in (a, lp, h) if o])
        runs.append((a, lp, h))
    for x, y in zip(*runs):
        assert (x is None and y is None) or _same_bits(x[1], y[1]), "two calls, different bits"
    a, lp, h = runs[0]
    assert int(a[1].max()) <= 4
    for o in (lp, h):
        assert o is None or not bool(torch.isnan(o[1]).any()), "an output was left unwritten"
    return a[1].cpu().numpy(), lp and lp[1].cpu().numpy(), h and h[1].cpu().numpy()


def raw_loss(x, clip=0.2, vf_coef=0.5, ent_coef=0.01, mask=True, critic=True):
    """fl_ppo_loss twice on guarded outputs and workspace: (grad_logits f32 [R, 5], grad_value f32 [B] or None, stats f64 [8])"""
    R = len(x["actions"])
    B = len(x["value"]) if critic else 0
    d = {k: _dev(x[k]) for k in ("logits", "valid", "actions", "old_logp", "adv")}
    m = _dev(x["mask"]) if mask else None
    v, ret = (_dev(x["value"]), _dev(x["returns"])) if critic else (None, None)
    need = hb._sym("fl_ppo_loss_workspace_bytes")(R, B)
    runs = []
    for k in range(2):
        gl, gv, st = _out((R, 5), torch.float32), _out((B,), torch.float32) if critic else None, _out((8,), torch.float64)
        ws = _guarded(need)
        if k:
            ws[:need].fill_(0x3C)                                    # what the workspace held before the call does not matter
        with torch.cuda.device(DEV):
            rc = hb._sym("fl_ppo_loss")(R, B, d["logits"].data_ptr(), d["valid"].data_ptr(), d["actions"].data_ptr(),
                                        d["old_logp"].data_ptr(), d["adv"].data_ptr(), _ptr(m), _ptr(v), _ptr(ret), clip, vf_coef,
                                        ent_coef, gl[1].data_ptr(), _ptr(gv and gv[1]), st[1].data_ptr(), ws.data_ptr(), need, _stream())
        assert rc == 0, hb.lib().fl_last_error().decode()
        _intact(*[o for o in (gl, gv, st) if o])
        assert bool((ws[need:] == 0xA5).all()), "the workspace's guard was written"
        runs.append((gl, gv, st))
    for a, b in zip(*runs):
        assert (a is None and b is None) or _same_bits(a[1], b[1]), "two calls, different bits"
    gl, gv, st = runs[0]
    for o in (gl, gv, st):
        assert o is None or not bool(torch.isnan(o[1]).any()), "an output was left unwritten"
    return gl[1].cpu().numpy(), gv and gv[1].cpu().numpy(), st[1].cpu().numpy()


def raw_gae(r, v, d, gamma, lam):
    T, N = r.shape
    rd, vd, dd = _dev(r), _dev(v), _dev(d)
    runs = []
    for _ in range(2):
        adv, ret = _out((T, N), torch.float32), _out((T, N), torch.float32)
        with torch.cuda.device(DEV):
            rc = hb._sym("fl_gae")(T, N, rd.data_ptr(), vd.data_ptr(), dd.data_ptr(), gamma, lam, adv[1].data_ptr(), ret[1].data_ptr(),
                                   _stream())
        assert rc == 0, hb.lib().fl_last_error().decode()
        _intact(adv, ret)
        runs.append((adv, ret))
    for a, b in zip(*runs):
        assert _same_bits(a[1], b[1])
    return runs[0][0][1].cpu().numpy(), runs[0][1][1].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- sampling
def sample_inputs(R, scale, seed):
    rng = np.random.default_rng([seed, R, int(scale)])
    logits = (scale * rng.standard_normal((R, 5))).astype(np.float32)
    valid = pht.synth_inputs(1, R, seed)[2].reshape(R, 5)            # every fourth row without a valid action, every fourth with one
    return logits, valid, rng.random(R)


def check_sample(logits, valid, u, got, cap=0.01):
    """actions against the restatement (exempt rows counted and capped), logp / entropy within one float32 ulp + 1e-12 (1 + spread)"""
    actions, logp, entropy = got
    R = len(u)
    ref_a, _, ref_h = pn.sample(logits, valid, u)
    ex = np.array([bool(pht.exempt(logits[r], valid[r], "soft", EPS, u=u[r])) for r in range(R)])
    assert ex.sum() <= cap * R, ex.sum()
    assert (actions == ref_a)[~ex].all(), np.flatnonzero((actions != ref_a) & ~ex)
    some = valid.any(axis=1)
    assert (valid[np.arange(R), actions][some] != 0).all()           # an exempt row's action is a valid one too
    assert (actions[~some] == 0).all() and (logp[~some] == 0).all() and (entropy[~some] == 0).all()
    single = (valid != 0).sum(axis=1) == 1
    assert (logp[single] == 0).all() and (entropy[single] == 0).all()
    lp_all, _, _, m = pn.log_softmax(logits, valid)
    ref_lp = np.where(some, lp_all[np.arange(R), actions], 0.0)      # the log-probability of the action the kernel drew
    spread = np.where(valid != 0, np.abs(logits.astype(np.float64) - m[:, None]), 0.0).max(axis=1)
    for name, g, ref in (("logp", logp, ref_lp), ("entropy", entropy, ref_h)):
        err, tol = np.abs(g.astype(np.float64) - ref), _ulp32(ref) + 1e-12 * (1.0 + spread)
        print(name, "R", R, "worst err / tol %.3g" % float((err / tol).max()), "exempt", int(ex.sum()))
        assert (err <= tol).all(), (name, np.flatnonzero(err > tol)[:5])
    return int(ex.sum())


@pytest.mark.parametrize("scale", (1.0, 30.0))
@pytest.mark.parametrize("R", ROWS)
def test_sample_against_the_restatement(R, scale):
    logits, valid, u = sample_inputs(R, scale, 3)
    run = lambda: raw_sample(logits, valid, u)                      # noqa: E731
    got = _on_side_stream(run) if (R, scale) == (257, 1.0) else run()
    check_sample(logits, valid, u, got)
    # without logp / entropy the actions are the same
    a2, lp2, h2 = raw_sample(logits, valid, u, logp=False, entropy=R % 2 == 0)
    assert lp2 is None and (h2 is None) == (R % 2 == 1) and np.array_equal(a2, got[0])
    assert h2 is None or np.array_equal(h2, got[2])


def test_sample_seeded_batch_leaves_out_no_row():
    logits, valid, u = sample_inputs(4099, 1.0, 5)
    assert check_sample(logits, valid, u, raw_sample(logits, valid, u)) == 0


def test_sample_exact_cases():
    """equal logits: expf(0) = 1 on any implementation, so kernel and restatement hold the same CDF.  Every non-empty mask, u on
    every CDF step, just below it, 0 and 1 - 2^-53: exact equality, no exemption"""
    rows = []
    for bits in range(1, 63):                                        # every non-empty mask at two levels of the logits: 2 workgroups
        valid = np.array([(bits % 31 + 1 >> j) & 1 for j in range(5)], dtype=np.uint8)
        logits = np.full(5, np.float32(0.7 * bits - 9.0))
        logits[valid == 0] = np.float32(50.0)                        # what is masked out does not matter, however large
        steps = pht.cdf_of(logits, valid)
        for u in list(steps[:-1]) + [np.nextafter(s, 0.0) for s in steps] + [0.0, 1.0 - 2.0 ** -53]:
            rows.append((logits, valid, u))
    logits, valid, u = (np.array([r[k] for r in rows]) for k in range(3))
    assert len(u) > 256
    actions, logp, entropy = raw_sample(logits, valid, u)
    ref_a, ref_lp, ref_h = pn.sample(logits, valid, u)
    assert np.array_equal(actions, ref_a)
    n = valid.sum(axis=1)
    # u on step k picks action k + 1 of the valid ones (side = "right"), just below it action k: both happen
    assert len(set(zip(n.tolist(), [int(valid[i, :a].sum()) for i, a in enumerate(actions)]))) == 15
    assert np.abs(logp - (-np.log(n))).max() <= 2.0 ** -23 and np.abs(entropy - np.log(n)).max() <= 2.0 ** -22
    assert (logp[n == 1] == 0).all() and (entropy[n == 1] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_sample_reference_u_is_the_fixtures_soft(name):
    g = load(name)
    for s in range(g["logits"].shape[0]):
        lg, va = g["logits"][s].reshape(-1, 5), g["valid"].reshape(-1, 5)
        actions, _, _ = raw_sample(lg, va, np.full(len(lg), pht.U_REFERENCE))
        assert np.array_equal(actions, g["soft"][s].reshape(-1)), name


def test_sample_reference_u_is_fl_policy_head_select_1():
    """on logits that fl_policy_head just produced, with u = FL_POLICY_U_REFERENCE for every row: its select = 1 actions, bit for bit"""
    from flatland_marl_amd.policy import Network, sample_actions
    g = load("synth_b2_a33")
    net = Network().to(DEV)
    net.load_state_dict(golden_params(g, 0))
    attr, tree, valid = (x.to(DEV).contiguous() for x in golden_inputs(g, 0))
    with torch.no_grad():
        (logits,), _, soft = net.head(attr, tree, valid, "soft")
    actions, logp, entropy = sample_actions(logits, valid, hb.POLICY_U_REFERENCE)
    assert actions.dtype == torch.uint8 and torch.equal(actions, soft)
    for u in (0.0, 0.05, 0.95):
        with torch.no_grad():
            assert torch.equal(sample_actions(logits, valid, u)[0], net.head(attr, tree, valid, "soft", u=u)[2])


# ---------------------------------------------------------------------------------------------------------------- the loss
def check_loss(x, got, clip=0.2, vf_coef=0.5, ent_coef=0.01, mask=True, critic=True):
    gl, gv, st = got
    y = dict(x, mask=x["mask"] if mask else None)
    if not critic:
        y["value"] = y["returns"] = None
    assert off_the_clip_boundary(dict(y, mask=np.ones(len(x["actions"]), dtype=np.uint8)), clip)
    ref = pn.ppo_loss(clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, **y)
    err, tol = np.abs(gl.astype(np.float64) - ref["grad_logits"]), _ulp32(ref["grad_logits"]) + 1e-12 * ref["grad_logits_terms"]
    assert (err <= tol).all(), ("grad_logits", np.argwhere(err > tol)[:5])
    assert (gl[x["valid"] == 0] == 0).all() and (gl[~ref["w"]] == 0).all()
    worst = [float((err / np.maximum(tol, 1e-300)).max())]
    if critic:
        err, tol = np.abs(gv.astype(np.float64) - ref["grad_value"]), _ulp32(ref["grad_value"]) + 1e-12 * ref["grad_value_terms"]
        assert (err <= tol).all(), ("grad_value", np.flatnonzero(err > tol)[:5])
        worst.append(float((err / np.maximum(tol, 1e-300)).max()))
    else:
        assert gv is None and st[1] == 0
    assert st[6] == ref["stats"][6] and st[7] == ref["stats"][7]
    serr = np.abs(st[:6] - ref["stats"][:6])
    print("R", len(gl), "n", int(st[6]), "grad err / tol", worst, "stats err / terms", (serr / np.maximum(ref["stats_terms"], 1e-300)).tolist())
    assert (serr <= 1e-12 * ref["stats_terms"]).all(), (st, ref["stats"])
    return ref


@pytest.mark.parametrize("B", (1, 3, 257))
@pytest.mark.parametrize("R", ROWS)
def test_loss_against_the_restatement(R, B):
    x = loss_inputs(R, B, 4)
    run = lambda: raw_loss(x)                                       # noqa: E731
    got = _on_side_stream(run) if (R, B) == (257, 3) else run()
    ref = check_loss(x, got)
    if R >= 63:
        assert 0 < ref["stats"][6] < R and ref["stats"][7] > 0


@pytest.mark.parametrize("case", ("masks on", "masks off", "no mask", "no critic", "no mask, no critic", "ent_coef 0", "clip_eps 0",
                                  "scale 30"))
def test_loss_options(case):
    x = loss_inputs(321, 5, 9, scale=30.0 if case == "scale 30" else 1.0)
    kw = {}
    if case == "masks on":
        x["mask"][:] = 1
    elif case == "masks off":
        x["mask"][:] = 0
    elif case == "ent_coef 0":
        kw["ent_coef"] = 0.0
    elif case == "clip_eps 0":
        kw["clip"] = 0.0
    kw["mask"] = "no mask" not in case
    kw["critic"] = "no critic" not in case
    gl, gv, st = got = raw_loss(x, **kw)
    ref = check_loss(x, got, **kw)
    if case == "masks off":                                          # n = 0: zeros, no NaN; the critic terms do not depend on n
        assert st[6] == 0 and (gl == 0).all() and (st[[0, 2, 4, 5, 7]] == 0).all() and np.isfinite(st).all()
        assert st[1] > 0 and st[3] == 0.5 * st[1] and (gv != 0).any()
    if case == "clip_eps 0":                                         # every counted row is outside [1, 1]
        assert st[5] == 1.0
    if case in ("no mask", "masks on"):
        w, bad = pn.weights(x["valid"], x["actions"], None)
        assert st[6] == w.sum() and st[7] == bad.sum() > 0


def test_loss_rows_deep_inside_and_far_outside_the_clip_range():
    """rho = 1.01, 0.99 (inside), 3 and 0.2 (outside) on both signs of A, ent_coef = 0: the clipped side's gradient rows are exactly
    zero, every other row's is not"""
    rng = np.random.default_rng(17)
    targets = np.array([1.01, 0.99, 3.0, 0.2])
    R = 8 * 40
    logits = rng.standard_normal((R, 5)).astype(np.float32)
    valid = np.ones((R, 5), dtype=np.uint8)
    valid[np.arange(R), rng.integers(0, 5, R)] = 0
    actions, logp, _ = pn.sample(logits, valid, rng.random(R))
    rho = targets[np.arange(R) % 4]
    adv = np.where((np.arange(R) // 4) % 2 == 0, 1.5, -1.5).astype(np.float32)
    x = dict(logits=logits, valid=valid, actions=actions, old_logp=(logp - np.log(rho)).astype(np.float32), adv=adv,
             mask=np.ones(R, dtype=np.uint8), value=np.zeros(2, dtype=np.float32), returns=np.ones(2, dtype=np.float32))
    gl, gv, st = got = raw_loss(x, ent_coef=0.0)
    check_loss(x, got, ent_coef=0.0)
    clipped = ((adv > 0) & (rho > 1.2)) | ((adv < 0) & (rho < 0.8))
    assert clipped.sum() == R // 4
    assert (gl[clipped] == 0).all() and (np.abs(gl[~clipped]).max(axis=1) > 0).all()
    assert st[5] == 0.5 and st[6] == R


# ---- past the edges of the slot loops (more than 256 workgroups) and of k_ppo_count's stride (more than 1 024 count workgroups)
@pytest.mark.parametrize("R,B", LARGE_CASES)
def test_loss_against_the_restatement_past_each_edge(R, B):
    x = large_inputs(R, B)
    run = lambda: raw_loss(x)                                       # noqa: E731
    got = _on_side_stream(run) if (R, B) == (E1 + 1, 257) else run()
    check_loss(x, got)
    if R > FPP_THREADS:
        assert 0 < got[2][6] < R and got[2][7] > 0


@pytest.mark.parametrize("kw", (dict(mask=False), dict(critic=False)), ids=("no mask", "no critic"))
def test_loss_options_where_the_count_kernel_strides(kw):
    R = E2 + 1
    x = large_inputs(R, 257)
    got = raw_loss(x, **kw)
    check_loss(x, got, **kw)
    assert 0 < got[2][6] < R and got[2][7] > 0


def _counted_only(x, rows):
    mask = np.zeros(len(x["actions"]), dtype=np.uint8)
    mask[rows] = 1
    return dict(x, mask=mask)


@pytest.mark.parametrize("k", PLACE_ROWS)
def test_loss_one_counted_row_wherever_it_lies(k):
    """every row well formed, the mask 0 except on row k: n = 1, and every other sum slot holds an exact 0.0, every other count slot
    an integer 0, so the statistics and row k's gradients are, bit for bit, those of a call on that row alone"""
    x = large_inputs(PLACE_R, PLACE_B, True)
    y = _counted_only(x, [k])
    gl, gv, st = got = raw_loss(y)
    assert st[6] == 1 and st[7] == 0
    assert (gl[:k] == 0).all() and (gl[k + 1:] == 0).all() and (gl[k] != 0).any()
    check_loss(y, got)
    alone = {key: x[key][k:k + 1] for key in ("logits", "valid", "actions", "old_logp", "adv")}
    gl1, gv1, st1 = raw_loss(dict(alone, mask=np.ones(1, dtype=np.uint8), value=x["value"], returns=x["returns"]))
    assert st1[6] == 1 and st[1] != 0 and st[2] != 0 and st[4] != 0
    assert np.array_equal(st.view(np.uint64), st1.view(np.uint64)), (st, st1)
    assert np.array_equal(gl[k].view(np.uint32), gl1[0].view(np.uint32)) and np.array_equal(gv.view(np.uint32), gv1.view(np.uint32))


def test_loss_one_counted_row_in_every_workgroup():
    """the last row of every 256-row group, and of the ragged last one: a count slot that is dropped or added twice changes n"""
    x = large_inputs(PLACE_R, PLACE_B, True)
    rows = np.unique(np.minimum(np.arange(FPP_THREADS - 1, PLACE_R + FPP_THREADS - 1, FPP_THREADS), PLACE_R - 1))
    assert len(rows) == 2 * (E2 // FPP_THREADS) + 1 == 2049
    y = _counted_only(x, rows)
    got = raw_loss(y)
    assert got[2][6] == len(rows) and got[2][7] == 0
    check_loss(y, got)


def test_loss_rows_with_an_invalid_action_only_where_the_count_kernel_strides():
    """every row's mask set, the action not a valid one exactly on the rows from E2 on: the rows a workgroup of k_ppo_count reaches
    on its second and third trip"""
    x = large_inputs(PLACE_R, PLACE_B, True)
    actions = x["actions"].copy()
    late = np.arange(E2, PLACE_R)
    off = x["valid"][late] == 0
    actions[late] = np.where(off.any(axis=1) & (late % 2 == 0), off.argmax(axis=1), 5 + late % 250).astype(np.uint8)
    y = dict(x, actions=actions)
    got = raw_loss(y)
    ref = check_loss(y, got)
    assert got[2][6] == ref["stats"][6] == E2 and got[2][7] == ref["stats"][7] == PLACE_R - E2


# ---- valid[j] != 0 and mask_r == 0 are what the header tests: any non-zero byte is a 1
OTHER_BYTES = np.array([2, 0x80, 0xFF], dtype=np.uint8)


def _other_bytes(a):
    """a's non-zero bytes replaced by 2, 0x80 or 0xFF, by row index"""
    by_row = OTHER_BYTES[np.arange(len(a)) % 3].reshape((-1,) + (1,) * (a.ndim - 1))
    out = np.where(a != 0, by_row, 0).astype(np.uint8)
    assert set(np.unique(out)) == {0, 2, 0x80, 0xFF} and np.array_equal(out != 0, a != 0)
    return out


def test_loss_takes_any_nonzero_byte_of_valid_and_mask_as_set():
    x = loss_inputs(257, 3, 4)
    assert set(np.unique(x["valid"])) == {0, 1} and set(np.unique(x["mask"])) == {0, 1}
    y = dict(x, valid=_other_bytes(x["valid"]), mask=_other_bytes(x["mask"]))
    for kw in ({}, dict(mask=False)):
        want, got = raw_loss(x, **kw), raw_loss(y, **kw)
        for a, b in zip(want, got):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        check_loss(y, got, **kw)


def test_sample_takes_any_nonzero_byte_of_valid_as_set():
    """kernel against kernel on the same logits and u: every bit equal, no row exempt"""
    logits, valid, u = sample_inputs(257, 1.0, 3)
    assert set(np.unique(valid)) == {0, 1}
    other = _other_bytes(valid)
    want, got = raw_sample(logits, valid, u), raw_sample(logits, other, u)
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    check_sample(logits, other, u, got)


# ---------------------------------------------------------------------------------------------------------------- GAE
def _dones(kind, T, N, rng):
    d = np.zeros((T, N), dtype=np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[-1] = 1
    elif kind == "random":
        d = (rng.random((T, N)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (T, N)).astype(np.uint8)     # non-zero = done
    return d


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("T", (1, 2, 129))
def test_gae_bit_for_bit(T, N):
    rng = np.random.default_rng([T, N])
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = (3 * rng.standard_normal((T + 1, N))).astype(np.float32)
    for kind in ("none", "all", "first", "last", "random"):
        d = _dones(kind, T, N, rng)
        for gamma in (0.0, 0.95, 1.0):
            for lam in (0.0, 0.95, 1.0):
                run = lambda: raw_gae(r, v, d, gamma, lam)         # noqa: E731
                adv, ret = _on_side_stream(run) if (T, N, kind, gamma, lam) == (129, 65, "random", 0.95, 0.95) else run()
                ref_adv, ref_ret, _ = pn.gae(r, v, d, gamma, lam)
                assert np.array_equal(adv.view(np.uint32), ref_adv.view(np.uint32)), (kind, gamma, lam)
                assert np.array_equal(ret.view(np.uint32), ref_ret.view(np.uint32)), (kind, gamma, lam)


# ---------------------------------------------------------------------------------------------------------------- modules
def test_sample_actions_float_tensor_and_generator():
    from flatland_marl_amd.policy import sample_actions
    logits_np, valid_np, u_np = sample_inputs(6 * 43, 1.0, 8)
    logits, valid = _dev(logits_np).view(6, 43, 5), _dev(valid_np).view(6, 43, 5)
    a, lp, h = sample_actions(logits, valid, _dev(u_np).view(6, 43))
    assert (a.shape, a.dtype, lp.shape, lp.dtype, h.shape, h.dtype) == ((6, 43), torch.uint8, (6, 43), torch.float32, (6, 43), torch.float32)
    ra, rlp, rh = raw_sample(logits_np, valid_np, u_np)
    assert np.array_equal(a.cpu().numpy().reshape(-1), ra) and np.array_equal(lp.cpu().numpy().reshape(-1), rlp)
    assert np.array_equal(h.cpu().numpy().reshape(-1), rh)
    a2 = sample_actions(logits, valid, 0.25)[0]
    assert np.array_equal(a2.cpu().numpy().reshape(-1), raw_sample(logits_np, valid_np, np.full(len(u_np), 0.25))[0])
    gen = torch.Generator(device=DEV)
    draws = []
    for seed in (5, 5, 6):
        gen.manual_seed(seed)
        draws.append(sample_actions(logits, valid, generator=gen))
    assert all(torch.equal(x, y) for x, y in zip(draws[0], draws[1])) and not torch.equal(draws[0][0], draws[2][0])
    gen.manual_seed(5)
    u = torch.rand((6, 43), dtype=torch.float64, device=DEV, generator=gen)
    assert torch.equal(sample_actions(logits, valid, u)[0], draws[0][0])
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            sample_actions(logits, valid, bad)
    with pytest.raises(ValueError):
        sample_actions(logits, valid, u.float())
    with pytest.raises(ValueError):
        sample_actions(logits.double(), valid)


def test_ppo_loss_module_scales_the_kernels_gradients():
    from flatland_marl_amd import policy
    x = loss_inputs(4 * 65, 4, 12)
    gl, gv, st = raw_loss(x)
    t = {k: _dev(v) for k, v in x.items()}
    shape = (4, 65)
    args = (t["valid"].view(4, 65, 5), t["actions"].view(shape), t["old_logp"].view(shape), t["adv"].view(shape))
    logits = t["logits"].view(4, 65, 5).clone().requires_grad_(True)
    value = t["value"].clone().requires_grad_(True)
    loss, stats = policy.ppo_loss(logits, value, *args, t["returns"], mask=t["mask"].view(shape))
    assert loss.dim() == 0 and loss.dtype == torch.float64 and stats.shape == (8,) and stats.dtype == torch.float64
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), st.view(np.uint64)) and float(loss.detach()) == st[3]
    assert not stats.requires_grad
    (2 * loss).backward()
    assert np.array_equal(logits.grad.cpu().numpy().reshape(-1, 5).view(np.uint32), (2 * gl).view(np.uint32))
    assert np.array_equal(value.grad.cpu().numpy().view(np.uint32), (2 * gv).view(np.uint32))
    # without the critic terms, without a mask
    gl2, _, st2 = raw_loss(x, mask=False, critic=False)
    logits.grad = None
    loss2, stats2 = policy.ppo_loss(logits, None, *args, None)
    loss2.backward()
    assert np.array_equal(logits.grad.cpu().numpy().reshape(-1, 5).view(np.uint32), gl2.view(np.uint32)) and float(loss2.detach()) == st2[3]
    with pytest.raises(ValueError):
        policy.ppo_loss(logits, value, *args, None)
    with pytest.raises(ValueError):
        policy.ppo_loss(logits, None, *args, None, clip=-0.1)


def test_ppo_loss_module_at_the_benchmarked_shape():
    """(256, 400, 5) logits and 256 values, tools/ppo_bench.py's cfg5: 400 workgroups, the slot loops' second trip, through the module"""
    from flatland_marl_amd import policy
    shape = (256, 400)
    x = large_inputs(shape[0] * shape[1], shape[0])
    gl, gv, st = raw_loss(x)
    t = {k: _dev(v) for k, v in x.items()}
    logits = t["logits"].view(*shape, 5).clone().requires_grad_(True)
    value = t["value"].clone().requires_grad_(True)
    loss, stats = policy.ppo_loss(logits, value, t["valid"].view(*shape, 5), t["actions"].view(shape), t["old_logp"].view(shape),
                                  t["adv"].view(shape), t["returns"], mask=t["mask"].view(shape))
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), st.view(np.uint64)) and float(loss.detach()) == st[3]
    loss.backward()
    assert np.array_equal(logits.grad.cpu().numpy().reshape(-1, 5).view(np.uint32), gl.view(np.uint32))
    assert np.array_equal(value.grad.cpu().numpy().view(np.uint32), gv.view(np.uint32))


def test_gae_module():
    from flatland_marl_amd import policy
    rng = np.random.default_rng(31)
    T, N = 33, 70
    r, v = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal((T + 1, N)).astype(np.float32)
    d = _dones("random", T, N, rng)
    adv, ret = policy.gae(_dev(r), _dev(v), _dev(d))
    ref_adv, ref_ret, _ = pn.gae(r, v, d, 0.99, 0.95)
    assert adv.dtype == torch.float32 and adv.shape == (T, N) and ret.shape == (T, N)
    assert np.array_equal(adv.cpu().numpy().view(np.uint32), ref_adv.view(np.uint32))
    assert np.array_equal(ret.cpu().numpy().view(np.uint32), ref_ret.view(np.uint32))
    with pytest.raises(ValueError):
        policy.gae(_dev(r), _dev(v[:-1]), _dev(d))
    with pytest.raises(ValueError):
        policy.gae(_dev(r), _dev(v), _dev(d), gamma=1.5)


def _fixture_obs(B=2, A=5):
    """B observations of the smallest fixture (cfg1: 7 agents), its first A agents, as Network.forward takes them"""
    from tests import tree_lstm_torch as tl
    fx = util.load("cfg1_uniform")
    idx = [3, 40][:B]
    attr = torch.from_numpy(np.ascontiguousarray(fx["o_attr"][idx, :A])).to(DEV)
    forest = torch.from_numpy(np.ascontiguousarray(fx["o_forest"][idx, :A])).to(DEV)
    adj = tl.modify_adjacency(np.ascontiguousarray(fx["o_adjacency"][idx, :A])).to(DEV)
    no = torch.from_numpy(np.ascontiguousarray(fx["o_node_order"][idx, :A])).to(torch.int64).to(DEV)
    eo = torch.from_numpy(np.ascontiguousarray(fx["o_edge_order"][idx, :A])).to(torch.int64).to(DEV)
    valid = torch.from_numpy(np.ascontiguousarray(fx["o_valid"][idx, :A]).astype(np.uint8)).to(DEV)
    return attr, forest, adj, no, eo, valid


def test_ppo_loss_trains_all_46_parameters_and_the_plumbing_adds_nothing():
    from flatland_marl_amd import policy
    net = policy.Network(trainable=True).to(DEV)
    net.load_state_dict(pht.seeded_params(3, 3.0))
    net.tree_lstm.trainable = True
    attr, forest, adj, no, eo, valid = _fixture_obs()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    actions, logp, entropy, value0, logits0 = net.rollout(attr, forest, adj, no, eo, valid, generator=gen)
    rng = np.random.default_rng(2)
    old_logp = logp + _dev((0.2 * rng.standard_normal((2, 5))).astype(np.float32))
    adv, returns = _dev(rng.standard_normal((2, 5)).astype(np.float32)), _dev(rng.standard_normal(2).astype(np.float32))

    (logits,), value = net(attr, forest, adj, no, eo)
    assert torch.equal(logits, logits0) and torch.equal(value, value0)           # the trainable forward: the roll-out's bits
    loss, stats = policy.ppo_loss(logits, value, valid, actions, old_logp, adv, returns)
    assert float(stats[6]) > 0
    loss.backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    assert len(got) == 46
    for k, g in got.items():
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), k

    # the kernel's own gradients handed to the same graph
    gl = torch.empty_like(logits0)
    gv = torch.empty_like(value0)
    st = torch.empty(8, dtype=torch.float64, device=DEV)
    hb.ppo_loss(logits0, valid, actions, old_logp, adv, None, value0, returns, 0.2, 0.5, 0.01, gl, gv, st)
    assert torch.equal(st, stats)
    net.zero_grad(set_to_none=True)
    (logits,), value = net(attr, forest, adj, no, eo)
    torch.autograd.backward([logits, value], [gl, gv])
    for k, p in net.named_parameters():
        assert _same_bits(p.grad, got[k]), k


@pytest.mark.parametrize("precision,head_precision", (("f32", "f32"), ("bf16", "bf16")))
def test_rollout_shapes_and_dtypes(precision, head_precision):
    from flatland_marl_amd import policy
    net = policy.Network(precision=precision, head_precision=head_precision).to(DEV)
    net.load_state_dict(pht.seeded_params(3, 3.0))
    attr, forest, adj, no, eo, valid = _fixture_obs()
    out = net.rollout(attr, forest, adj, no, eo, valid, u=hb.POLICY_U_REFERENCE)
    actions, logp, entropy, value, logits = out
    assert [(tuple(t.shape), t.dtype) for t in out] == [((2, 5), torch.uint8), ((2, 5), torch.float32), ((2, 5), torch.float32),
                                                        ((2,), torch.float32), ((2, 5, 5), torch.float32)]
    assert not any(t.requires_grad for t in out)
    assert torch.equal(actions, net.act(attr, forest, adj, no, eo, valid, "soft"))          # the reference's u: the reference's draw
    ref_a, ref_lp, ref_h = pn.sample(logits.cpu().numpy(), valid.cpu().numpy(), hb.POLICY_U_REFERENCE)
    assert np.array_equal(actions.cpu().numpy().reshape(-1), ref_a)
    assert np.abs(logp.cpu().numpy().reshape(-1) - ref_lp).max() <= 1e-6 and bool((entropy >= 0).all())


def test_rollout_actions_step_the_env():
    from flatland_marl_amd import policy, workload as wl
    envs, _ = wl.make_envs("cfg1", B=2)
    env = hb.BatchedRailEnv(envs)
    net = policy.Network().to(DEV)
    net.load_state_dict(pht.seeded_params(5, 3.0))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    try:
        seen = set()
        for _ in range(5):
            attr, forest, adj, no, eo = env.obs_policy()
            valid = env.obs_outputs()["valid_actions"]
            actions, logp, entropy, value, logits = net.rollout(attr, forest, adj, no, eo, valid, generator=gen)
            assert actions.shape == (env.B, env.A) and actions.dtype == torch.uint8 and int(actions.max()) <= 4
            assert logp.shape == (env.B, env.A) and value.shape == (env.B,) and bool((logp <= 0).all())
            seen |= set(actions.unique().tolist())
            env.step(actions, filter_required=True)
        env.check()
        assert len(seen) >= 2
    finally:
        env.close()
