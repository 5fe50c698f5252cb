"""A differentiable restatement of the policy's TreeLSTM forward (solution/nn/TreeLSTM.py), written functionally (no in-place
write into h / c, so autograd goes through every level), in torch, float64 by default.  tests/tree_lstm_torch.py detaches its
parameters and stays the forward's restatement; this one is the gradient's: pinned to the reference module's own autograd by
tests/test_tree_lstm_grad_golden.py, and what the GPU tests hold fl_tree_lstm_backward to.

Inputs as BatchedRailEnv.obs_policy() returns them (see tests/tree_lstm_torch.py); params: a mapping with the reference's
state_dict names whose tensors may require grad.  A child that was not computed before its parent's level reads as zero and so
gets no gradient; a child named by several edges gets the sum; padding nodes stay zero whatever gradient is given for them.
"""
import torch

PARAM_ORDER = ("W_iou.weight", "W_iou.bias", "U_iou.weight", "W_c.weight", "W_c.bias", "W_f.weight", "W_f.bias", "U_f.weight")


def tree_lstm(forest, adjacency, node_order, edge_order, p, dtype=torch.float64):
    """h of every node [B*A*N, 128], differentiable with respect to the tensors of p (which are used as they are: dtype `dtype`,
    on the inputs' device)"""
    B, A, N, F = forest.shape
    M = p["W_f.weight"].shape[0]
    dev = forest.device
    x = forest.reshape(-1, F).to(dtype)
    adj = adjacency.reshape(-1, 3)
    no = node_order.reshape(-1)
    eo = edge_order.reshape(-1)
    h = torch.zeros(B * A * N, M, dtype=dtype, device=dev)
    c = torch.zeros_like(h)
    top = int(no.max())
    for n in range(0, top + 1):
        nodes = (no == n).nonzero().flatten()
        if len(nodes) == 0:
            continue
        xn = x[nodes]
        iou = xn @ p["W_iou.weight"].T + p["W_iou.bias"]
        if n > 0:
            ch = adj[eo == n][:, 1].view(-1, 3)
            ok = ((no[ch] >= 0) & (no[ch] < n)).unsqueeze(-1).to(dtype)
            hk, ck = h[ch] * ok, c[ch] * ok                                            # [n, 3, M]
            iou = iou + hk.reshape(len(nodes), 3 * M) @ p["U_iou.weight"].T
            f = torch.sigmoid((xn @ p["W_f.weight"].T + p["W_f.bias"]).unsqueeze(1) + hk @ p["U_f.weight"].T)
            c_red = (f * ck).reshape(len(nodes), 3 * M) @ p["W_c.weight"].T + p["W_c.bias"]
        i, o, u = iou[:, :M], iou[:, M:2 * M], iou[:, 2 * M:]
        cn = torch.sigmoid(i) * torch.tanh(u)
        if n > 0:
            cn = cn + c_red
        c = c.index_copy(0, nodes, cn)
        h = h.index_copy(0, nodes, torch.sigmoid(o) * torch.tanh(cn))
    return h


def grads(x, params, R, roots, dtype=torch.float64):
    """the eight gradients (a dict, dtype `dtype`) of sum(R * h) over the roots (R [T, 128]) or over every node (R [T*N, 128]),
    on the device of the inputs x = (forest, adjacency, node_order, edge_order)"""
    dev = x[0].device
    N = x[0].shape[2]
    p = {k: params[k].detach().to(device=dev, dtype=dtype).clone().requires_grad_(True) for k in PARAM_ORDER}
    h = tree_lstm(*x, p, dtype)
    if roots:
        h = h.view(-1, N, h.shape[1])[:, 0]
    loss = (h * R.to(device=dev, dtype=dtype).view(h.shape)).sum()
    if not loss.requires_grad:                                   # a forest of nothing but padding: no node, every gradient zero
        return {k: torch.zeros_like(v) for k, v in p.items()}
    g = torch.autograd.grad(loss, [p[k] for k in PARAM_ORDER], allow_unused=True)
    return {k: (torch.zeros_like(p[k]) if v is None else v) for k, v in zip(PARAM_ORDER, g)}


def rel_errors(g, g64):
    """per parameter max |g - g64| / max |g64|; where g64 is identically zero: 0.0 if g is too, else inf"""
    out = {}
    for k in PARAM_ORDER:
        den = float(g64[k].abs().max())
        num = float((g[k].double() - g64[k]).abs().max())
        out[k] = num / den if den > 0 else (0.0 if num == 0 else float("inf"))
    return out
