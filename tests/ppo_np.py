"""The project's own float64 restatements, in numpy, of the three functions of include/flatland_ppo.h -- the per-row draw with
its log-probability and entropy, the PPO loss with its closed-form gradients, and generalised advantage estimation -- written
from the header's formulas, in its operation order.  tests/test_ppo.py pins them: the draw to the reference actor's actions in the
fixtures, the gradients to torch's float64 autograd of the plain formula (plain_loss_torch below), GAE to an independent
evaluation.  tests/test_gpu_ppo.py compares the kernels with them."""
import numpy as np
import torch

from tests import policy_head_torch as pht

ACT = 5
NEG = -1.0e30      # the mask of plain_loss_torch: large, finite (torch's autograd of a -inf masked log-softmax gives NaN)


# ---------------------------------------------------------------------------------------------------------------- sampling
def log_softmax(logits, valid):
    """(logp [R, 5], p [R, 5], H [R], m [R]) in float64 from float32 logits over the valid actions, the sums in ascending j; 0
    where an action is not valid, and everywhere in a row without a valid action"""
    x = np.asarray(logits, dtype=np.float32).reshape(-1, ACT).astype(np.float64)
    va = np.asarray(valid).reshape(-1, ACT) != 0
    some = va.any(axis=1)
    m = np.where(some, np.where(va, x, -np.inf).max(axis=1), 0.0)
    e = np.where(va, np.exp(np.where(va, x - m[:, None], 0.0)), 0.0)
    S = np.zeros(len(x))
    for j in range(ACT):
        S = S + e[:, j]
    logS = np.log(np.where(some, S, 1.0))
    logp = np.where(va, (x - m[:, None]) - logS[:, None], 0.0)
    p = np.where(va, e / np.where(some, S, 1.0)[:, None], 0.0)
    acc = np.zeros(len(x))
    for j in range(ACT):
        acc = acc + p[:, j] * logp[:, j]
    return logp, p, 0.0 - acc, m


def sample(logits, valid, u):
    """(actions u8 [R], logp f64 [R], entropy f64 [R]): Actor._choose_action's soft draw (policy_head_torch._probabilities and
    cdf_of: the float32 softmax, the float64 CDF) with the row's own u, and the float64 log-probability of that action"""
    lg = np.asarray(logits, dtype=np.float32).reshape(-1, ACT)
    va = np.asarray(valid).reshape(-1, ACT)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (len(lg),)) if np.ndim(u) == 0 else np.asarray(u, dtype=np.float64).reshape(-1)
    actions = np.zeros(len(lg), dtype=np.uint8)
    for i in range(len(lg)):
        if not va[i].any():
            continue
        idx, _ = pht._probabilities(lg[i], va[i])
        k = int(np.searchsorted(pht.cdf_of(lg[i], va[i]), u[i], side="right"))
        actions[i] = idx[min(k, len(idx) - 1)]
    logp, _, H, _ = log_softmax(lg, va)
    la = np.where(va.any(axis=1), logp[np.arange(len(lg)), actions], 0.0)
    return actions, la, H


# ---------------------------------------------------------------------------------------------------------------- the loss
def weights(valid, actions, mask):
    """(w bool [R], rows left out for their action alone bool [R])"""
    va = np.asarray(valid).reshape(-1, ACT) != 0
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    on = np.ones(len(va), dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    ok = (a < ACT) & va[np.arange(len(va)), np.minimum(a, ACT - 1)]
    some = va.any(axis=1)
    return on & some & ok, on & some & ~ok


def ratio(logits, valid, actions, old_logp):
    """rho [R] in float64 (1 where the action is not a valid one)"""
    logp, _, _, _ = log_softmax(logits, valid)
    va = np.asarray(valid).reshape(-1, ACT) != 0
    a = np.minimum(np.asarray(actions).reshape(-1).astype(np.int64), ACT - 1)
    la = logp[np.arange(len(logp)), a]
    return np.where(va[np.arange(len(logp)), a], np.exp(la - np.asarray(old_logp, dtype=np.float64).reshape(-1)), 1.0)


def ppo_loss(logits, valid, actions, old_logp, adv, mask=None, value=None, returns=None, clip=0.2, vf_coef=0.5, ent_coef=0.01):
    """dict: grad_logits f64 [R, 5], grad_value f64 [B] or None, stats f64 [8], and what the tolerances of the GPU tests are made
    of -- grad_logits_terms / grad_value_terms (the sum of the magnitudes of the terms an element is formed from) and stats_terms
    [6] (the mean of the absolute row terms of stats[0..5])"""
    logp, p, H, _ = log_softmax(logits, valid)
    va = np.asarray(valid).reshape(-1, ACT) != 0
    R = len(logp)
    w, bad = weights(valid, actions, mask)
    n = int(w.sum())
    a = np.minimum(np.asarray(actions).reshape(-1).astype(np.int64), ACT - 1)
    la = logp[np.arange(R), a]
    old = np.asarray(old_logp, dtype=np.float32).reshape(-1).astype(np.float64)
    A = np.asarray(adv, dtype=np.float32).reshape(-1).astype(np.float64)
    lo, hi = 1.0 - clip, 1.0 + clip
    with np.errstate(over="ignore", invalid="ignore"):
        rho = np.exp(la - old)
        s = np.minimum(rho * A, np.minimum(np.maximum(rho, lo), hi) * A)
        gs = np.where(((A >= 0) & (rho <= hi)) | ((A < 0) & (rho >= lo)), rho * A, 0.0)
    delta = np.zeros((R, ACT))
    delta[np.arange(R), a] = 1.0
    g = np.zeros((R, ACT))
    terms = np.zeros((R, ACT))
    if n:
        full = (-gs[:, None] * (delta - p) + ent_coef * (p * (logp + H[:, None]))) / n
        g = np.where(va & w[:, None], full, 0.0)
        terms = np.where(va & w[:, None], (np.abs(gs)[:, None] + ent_coef * p * (np.abs(logp) + np.abs(H)[:, None])) / n, 0.0)
    stats = np.zeros(8)
    row_terms = np.zeros(6)
    if n:
        kl = old - la
        far = np.abs(rho - 1.0) > clip
        stats[0] = -s[w].sum() / n
        stats[2] = H[w].sum() / n
        stats[4] = kl[w].sum() / n
        stats[5] = far[w].sum() / n
        row_terms[[0, 2, 4, 5]] = np.abs(s[w]).mean(), np.abs(H[w]).mean(), np.abs(kl[w]).mean(), far[w].mean()
    gv = gv_terms = None
    if value is not None:
        d = np.asarray(value, dtype=np.float32).reshape(-1).astype(np.float64) - np.asarray(returns, dtype=np.float32).reshape(-1).astype(np.float64)
        stats[1] = 0.5 * (d * d).sum() / len(d)
        row_terms[1] = 0.5 * (d * d).mean()
        gv = vf_coef * d / len(d)
        gv_terms = vf_coef * np.abs(d) / len(d)
    stats[3] = (stats[0] + vf_coef * stats[1]) - ent_coef * stats[2]
    row_terms[3] = row_terms[0] + vf_coef * row_terms[1] + ent_coef * row_terms[2]
    stats[6], stats[7] = n, int(bad.sum())
    return dict(grad_logits=g, grad_value=gv, stats=stats, grad_logits_terms=terms, grad_value_terms=gv_terms, stats_terms=row_terms,
                rho=rho, w=w)


def plain_loss_torch(logits, valid, actions, old_logp, adv, mask=None, value=None, returns=None, clip=0.2, vf_coef=0.5, ent_coef=0.01):
    """the plain formula in torch float64 ops, for autograd: (total, logits leaf [R, 5], value leaf [B] or None).  The mask is a
    large finite negative; a row that does not count enters with weight 0 (its action clamped into range for the gather)."""
    x = torch.tensor(np.asarray(logits, dtype=np.float32).reshape(-1, ACT).astype(np.float64), requires_grad=True)
    va = torch.tensor(np.asarray(valid).reshape(-1, ACT) != 0)
    w_np, _ = weights(valid, actions, mask)
    w = torch.tensor(w_np.astype(np.float64))
    n = max(int(w_np.sum()), 1)
    a = torch.tensor(np.minimum(np.asarray(actions).reshape(-1).astype(np.int64), ACT - 1))
    logp = torch.log_softmax(torch.where(va, x, torch.full_like(x, NEG)), dim=1)
    la = logp.gather(1, a[:, None])[:, 0]
    H = -torch.where(va, logp.exp() * logp, torch.zeros_like(logp)).sum(dim=1)
    la = torch.where(w > 0, la, torch.zeros_like(la))                 # (a row that does not count: no exp of a masked -1e30)
    rho = torch.exp(la - torch.tensor(np.asarray(old_logp, dtype=np.float32).reshape(-1).astype(np.float64)) * (w > 0))
    A = torch.tensor(np.asarray(adv, dtype=np.float32).reshape(-1).astype(np.float64))
    s = torch.minimum(rho * A, torch.clamp(rho, 1.0 - clip, 1.0 + clip) * A)
    total = -(w * s).sum() / n - ent_coef * (w * H).sum() / n
    v = None
    if value is not None:
        v = torch.tensor(np.asarray(value, dtype=np.float32).reshape(-1).astype(np.float64), requires_grad=True)
        ret = torch.tensor(np.asarray(returns, dtype=np.float32).reshape(-1).astype(np.float64))
        total = total + vf_coef * 0.5 * ((v - ret) ** 2).mean()
    return total, x, v


# ---------------------------------------------------------------------------------------------------------------- GAE
def gae(rewards, values, dones, gamma, lam):
    """(adv f32 [T, N], returns f32 [T, N], A f64 [T, N]): the header's recurrence, float64, in its operation order"""
    r = np.asarray(rewards, dtype=np.float32).astype(np.float64)
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    nd = np.where(np.asarray(dones) != 0, 0.0, 1.0)
    T, N = r.shape
    A = np.zeros(N)
    out = np.zeros((T, N))
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * v[t + 1] * nd[t] - v[t]
        A = delta + gamma * lam * nd[t] * A
        out[t] = A
    return out.astype(np.float32), (out + v[:-1]).astype(np.float32), out


def gae_direct(rewards, values, dones, gamma, lam):
    """A f64 [T, N] without the recurrence: A_t = sum_{k >= t} (prod_{i = t}^{k - 1} gamma lam nd_i) delta_k"""
    r = np.asarray(rewards, dtype=np.float32).astype(np.float64)
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    nd = np.where(np.asarray(dones) != 0, 0.0, 1.0)
    T, N = r.shape
    delta = r + gamma * v[1:] * nd - v[:-1]
    out = np.zeros((T, N))
    for t in range(T):
        weight = np.ones(N)
        for k in range(t, T):
            out[t] += weight * delta[k]
            weight = weight * (gamma * lam * nd[k])
    return out
