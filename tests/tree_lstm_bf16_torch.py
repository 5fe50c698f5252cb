"""The emulation the tolerance of fl_tree_lstm_bf16's tests rests on: tests/tree_lstm_torch.py's tree_lstm with the operands of the
three recurrent products passed through bfloat16 (round to nearest even, .float().to(torch.bfloat16)) and back -- U_iou, U_f and
W_c once, h_k and f * c_k where they enter a product.  Everything else, the sums of those products included, is float64 (or
`dtype`): W_iou x, W_f x, the biases, the gates, h and c.  A node of height 0 has no recurrent product, so the emulation equals
the restatement there bit for bit.
"""
import torch


def bf16(t):
    """t rounded to bfloat16 and back, in t's dtype"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def tree_lstm(forest, adjacency, node_order, edge_order, params, dtype=torch.float64, with_c=False):
    """h of every node [B*A*N, 128] (and c, with_c=True), computed in `dtype` on the inputs' device"""
    dev = forest.device
    p = {k: v.detach().to(device=dev, dtype=dtype) for k, v in params.items()}
    u_iou, u_f, w_c = bf16(p["U_iou.weight"]), bf16(p["U_f.weight"]), bf16(p["W_c.weight"])
    B, A, N, F = forest.shape
    M = p["W_f.weight"].shape[0]
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
            e = adj[eo == n]
            par, ch = e[:, 0].view(-1, 3), e[:, 1].view(-1, 3)
            assert torch.equal(par, nodes.view(-1, 1).expand(-1, 3)), "a node of height %d without its three edges in order" % n
            ok = ((no[ch] >= 0) & (no[ch] < n)).unsqueeze(-1).to(dtype)
            hk, ck = bf16(h[ch] * ok), c[ch] * ok                                     # [n, 3, M]
            iou = iou + hk.reshape(len(nodes), 3 * M) @ u_iou.T
            f = torch.sigmoid((xn @ p["W_f.weight"].T + p["W_f.bias"]).unsqueeze(1) + hk @ u_f.T)
            c_red = bf16(f * ck).reshape(len(nodes), 3 * M) @ w_c.T + p["W_c.bias"]
        i, o, u = iou[:, :M], iou[:, M:2 * M], iou[:, 2 * M:]
        cn = torch.sigmoid(i) * torch.tanh(u)
        if n > 0:
            cn = cn + c_red
        c[nodes] = cn
        h[nodes] = torch.sigmoid(o) * torch.tanh(cn)
    return (h, c) if with_c else h
