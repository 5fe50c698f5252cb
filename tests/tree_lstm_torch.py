"""The project's own restatement of the policy's TreeLSTM forward (solution/nn/TreeLSTM.py), written from the math, level by
level, in torch (float64 by default).  Pinned to the reference's outputs by tests/test_tree_lstm_golden.py; the GPU tests compare
fl_tree_lstm with it where no fixture reaches, and tools/tree_lstm_bench.py times it as the masked-loop baseline.

Inputs as BatchedRailEnv.obs_policy() returns them (adjacency already modified): forest [B, A, N, 12], adjacency [B, A, N-1, 3]
(global node ids, negatives -2), node_order [B, A, N] (height, -2 padding), edge_order [B, A, N-1] (the parent's height).
params: a mapping with the reference's state_dict names.

  leaf (height 0)    iou = W_iou x + b_iou;  c = sigmoid(i) * tanh(u);  h = sigmoid(o) * tanh(c)
  height n > 0       children k1..k3 = the children of the node's three edges, in edge-list order
                     iou = W_iou x + b_iou + U_iou [h_k1 | h_k2 | h_k3];  f_j = sigmoid(W_f x + b_f + U_f h_kj)
                     c = sigmoid(i) * tanh(u) + W_c [f_1 c_k1 | f_2 c_k2 | f_3 c_k3] + b_c;  h = sigmoid(o) * tanh(c)
  padding            h = c = 0
"""
import torch


def triple_rule_violations(adjacency, node_order, edge_order):
    """trees [B, A] (bool) where a node of height n > 0 does not have its three edges one after another, in node order, inside
    its own tree -- the condition under which the reference's batch-wide pairing of level nodes and edge triples is per tree;
    also a node_order outside {-2} u [0, N-1], a real edge (of any order, 0 included) with its parent or child outside the tree,
    or an edge_order other than the parent's node_order: what include/flatland_hip.h says fl_tree_lstm counts"""
    B, A, N = node_order.shape
    no = node_order.reshape(B * A, N).cpu()
    eo = edge_order.reshape(B * A, N - 1).cpu()
    adj = adjacency.reshape(B * A, N - 1, 3).cpu()
    bad = torch.zeros(B * A, dtype=torch.bool)
    for t in range(B * A):
        base = t * N
        if not (((no[t] == -2) | ((no[t] >= 0) & (no[t] <= N - 1))).all()):
            bad[t] = True
            continue
        for n in range(1, int(no[t].max()) + 1 if (no[t] >= 0).any() else 1):
            nodes = (no[t] == n).nonzero().flatten() + base
            e = adj[t][eo[t] == n]
            if len(e) != 3 * len(nodes) or not torch.equal(e[:, 0], nodes.repeat_interleave(3)) or \
                    ((e[:, 1] < base) | (e[:, 1] >= base + N)).any():
                bad[t] = True
                break
        real = eo[t] != -2
        if not bad[t] and real.any():
            p, ch = adj[t][real, 0], adj[t][real, 1]
            if ((p < base) | (p >= base + N)).any() or not torch.equal(no[t][p - base], eo[t][real]):
                bad[t] = True
            elif ((ch < base) | (ch >= base + N)).any():      # "an index outside itself": on an edge of order 0 as well
                bad[t] = True
    return bad.view(B, A)


def tree_lstm(forest, adjacency, node_order, edge_order, params, dtype=torch.float64, with_c=False):
    """h of every node [B*A*N, 128] (and c, with_c=True), computed in `dtype` on the inputs' device"""
    dev = forest.device
    p = {k: v.detach().to(device=dev, dtype=dtype) for k, v in params.items()}
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
            # a child not computed before this level reads 0, as in the reference (zero-initialised, gathered before the writes)
            ok = ((no[ch] >= 0) & (no[ch] < n)).unsqueeze(-1).to(dtype)
            hk, ck = h[ch] * ok, c[ch] * ok                                            # [n, 3, M]
            iou = iou + hk.reshape(len(nodes), 3 * M) @ p["U_iou.weight"].T
            f = torch.sigmoid((xn @ p["W_f.weight"].T + p["W_f.bias"]).unsqueeze(1) + hk @ p["U_f.weight"].T)
            c_red = (f * ck).reshape(len(nodes), 3 * M) @ p["W_c.weight"].T + p["W_c.bias"]
        i, o, u = iou[:, :M], iou[:, M:2 * M], iou[:, 2 * M:]
        cn = torch.sigmoid(i) * torch.tanh(u)
        if n > 0:
            cn = cn + c_red
        c[nodes] = cn
        h[nodes] = torch.sigmoid(o) * torch.tanh(cn)
    return (h, c) if with_c else h


def seeded_params(seed, scale=1.0, names_shapes=None):
    """the goldens' weights: numpy.random.default_rng(seed), each parameter in state_dict order, uniform in +-scale/sqrt(fan_in),
    float32"""
    import numpy as np
    if names_shapes is None:
        names_shapes = [("W_iou.weight", (384, 12)), ("W_iou.bias", (384,)), ("U_iou.weight", (384, 384)),
                        ("W_c.weight", (128, 384)), ("W_c.bias", (128,)), ("W_f.weight", (128, 12)), ("W_f.bias", (128,)),
                        ("U_f.weight", (128, 128))]
    fan_in = {"W_iou": 12, "U_iou": 384, "W_c": 384, "W_f": 12, "U_f": 128}
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in names_shapes:
        bound = scale / np.sqrt(fan_in[name.split(".")[0]])
        out[name] = torch.from_numpy(rng.uniform(-bound, bound, size=shape).astype(np.float32))
    return out


def modify_adjacency(adjacency):
    """Network.modify_adjacency (solution/nn/net_tree.py:105-116) restated: int adjacency [B, A, E, 3] -> int64, parent / child
    offset by (b*A + a) * N, every negative entry -2"""
    adj = torch.as_tensor(adjacency).to(torch.int64).clone()
    B, A, E, _ = adj.shape
    N = E + 1
    adj[adj == -2] = -B * A * N
    off = (torch.arange(B * A, dtype=torch.int64, device=adj.device) * N).view(B, A, 1)
    adj[..., 0] += off
    adj[..., 1] += off
    adj[adj < 0] = -2
    return adj
