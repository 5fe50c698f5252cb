"""Synthetic forests in the policy's input format, for the TreeLSTM tests: deterministic (numpy.random.default_rng(seed)), numpy
and torch only, no GPU.  make(kind, T, N, seed, ...) returns what BatchedRailEnv.obs_policy() would hand the tree encoder for one
env of T agents: forest f32 [1, T, N, 12], adjacency i64 [1, T, N-1, 3] already modified (global node ids, negatives -2),
node_order i64 [1, T, N] (height, -2 padding), edge_order i64 [1, T, N-1] (the parent's height, -2 padding).

Kinds (every tree is padded to N nodes and N-1 edges; (N - 1) % 3 == 0):
  rand    random ternary trees: a random number of internal nodes, each expansion at a random leaf
  chain   the maximal number of internal nodes, (N - 1) / 3, on one path (heights 0 .. (N - 1) / 3)
  full    the largest complete ternary tree that fits (4, 13 or 40 nodes)
  perm    rand, node ids permuted (the root stays node 0); a level's parents in increasing node id, each parent's three edges one
          after another within its level; levels and padding edges interleaved in the edge list
  gaps    rand, the heights > 0 relabelled by a strictly increasing map into [1, N-1]; edge list interleaved as in perm
  flat    L height-0 nodes (nodes 0 .. L-1) without any edge, the rest padding; L an int or a sequence cycled over the trees
  lvl1    a tree with exactly m nodes of height 1 (m an int or a sequence cycled over the trees): the level populations of a
          group of trees can be set to a tile edge
  weird   perm, about 10 % of the children replaced by the parent itself and about 10 % by a random node of the same tree
          (padding, higher, or another parent's child): all of them legal, the first two kinds read as zero
  mixpad  kind `base` with every third tree (0, 3, ...) all padding, its root included

In the plain kinds the edge list holds the levels one after another, the root's first, then the padding.  The third adjacency
column is what modify_adjacency leaves of the action code: -2, 0, 1 for a parent's three edges.

Features: "gauss" = N(0, 3^2) on every node, padding included (a padding node's features must not matter), or
"fixture:NAME" = rows of o_forest of tests/golden/NAME.npz, sampled with replacement.
"""
import os

import numpy as np
import torch

KINDS = ("rand", "chain", "full", "perm", "gaps", "flat", "lvl1", "weird", "mixpad")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = 12


def _pick(v, t):
    return int(v[t % len(v)]) if hasattr(v, "__len__") else int(v)


def max_lvl1(N):
    """the largest m a lvl1 tree of N nodes can have"""
    kmax = (N - 1) // 3
    m = 0
    while (m + 1) + (m + 1) // 2 <= kmax:       # m + 1 nodes of height 1 need ceil(m / 2) internal nodes above them
        m += 1
    return m


def _topology(kind, N, rng, m=None):
    """children: {node: [c1, c2, c3]} over ids in creation order (the root is 0, a child's id is above its parent's)"""
    kmax = (N - 1) // 3
    children, leaves, nxt = {}, [0], 1

    def expand(p):
        nonlocal nxt
        leaves.remove(p)
        children[p] = [nxt, nxt + 1, nxt + 2]
        leaves.extend(children[p])
        nxt += 3

    if kind == "chain":
        for _ in range(kmax):
            expand(leaves[-1])
    elif kind == "full":
        size, depth = 1, 0
        while size + 3 ** (depth + 1) <= N:
            depth += 1
            size += 3 ** depth
        for _ in range((size - 1) // 3):
            expand(leaves[0])                                    # breadth first: the oldest leaf
    elif kind == "lvl1":
        if m > 0:
            top = m // 2                                         # ceil((m - 1) / 2) internal nodes give m or m + 1 leaf slots
            assert m + top <= kmax, "lvl1: %d nodes of height 1 do not fit in %d nodes" % (m, N)
            for _ in range(top):
                expand(leaves[0])
            for p in sorted(leaves)[-m:]:                        # at most one slot stays a leaf: every node above has height >= 2
                expand(p)
    else:
        for _ in range(int(rng.integers(0, kmax + 1))):
            expand(leaves[int(rng.integers(len(leaves)))])
    return children, nxt


def _tree(kind, N, rng, L=None, m=None):
    """one tree: node_order [N], edge_order [N-1], adjacency [N-1, 3] with tree-local ids (-2 = padding)"""
    E = N - 1
    no = np.full(N, -2, np.int64)
    eo = np.full(E, -2, np.int64)
    adj = np.full((E, 3), -2, np.int64)
    if kind == "flat":
        no[:L] = 0
        return no, eo, adj
    children, n_real = _topology(kind, N, rng, m)
    height = [0] * n_real
    for v in range(n_real - 1, -1, -1):                          # children have the larger ids
        if v in children:
            height[v] = 1 + max(height[c] for c in children[v])
    if kind == "lvl1":
        assert sum(h == 1 for h in height) == m
    if kind == "gaps":
        old = sorted(set(height) - {0})
        new = np.sort(rng.choice(np.arange(1, N), size=len(old), replace=False)) if old else []
        relabel = {0: 0, **{o: int(n) for o, n in zip(old, new)}}
        height = [relabel[h] for h in height]
    shuffled = kind in ("perm", "weird", "gaps")
    ids = np.arange(N)
    if kind in ("perm", "weird"):
        ids[1:] = 1 + rng.permutation(N - 1)
    for v in range(n_real):
        no[ids[v]] = height[v]
    levels = {}
    for p in children:
        levels.setdefault(height[p], []).append(p)
    seqs = []                                                    # per level, root's level first: its edges in the order required
    for n in sorted(levels, reverse=True):
        seqs.append([(n, ids[p], ids[c], j) for p in sorted(levels[n], key=lambda v: ids[v]) for j, c in enumerate(children[p])])
    order = [i for i, s in enumerate(seqs) for _ in s] + [-1] * (E - 3 * len(children))
    if shuffled:
        rng.shuffle(order)
    pos = [0] * len(seqs)
    for e, i in enumerate(order):
        if i < 0:
            continue
        n, p, c, j = seqs[i][pos[i]]
        pos[i] += 1
        if kind == "weird":
            r = rng.random()
            if r < 0.1:
                c = p
            elif r < 0.2:
                c = int(rng.integers(N))
        eo[e] = n
        adj[e] = (p, c, j - 1 if j else -2)
    return no, eo, adj


def features(spec, T, N, rng):
    if spec == "gauss":
        return (rng.normal(size=(T, N, F)) * 3).astype(np.float32)
    assert spec.startswith("fixture:"), spec
    fx = np.load(os.path.join(GOLD, spec[len("fixture:"):] + ".npz"))
    rows = np.ascontiguousarray(fx["o_forest"], dtype=np.float32).reshape(-1, F)
    return rows[rng.integers(0, len(rows), size=T * N)].reshape(T, N, F)


def structure(kind, T, N, seed, base="rand", L=None, m=None):
    """numpy, tree-local ids: node_order i64 [T, N], edge_order i64 [T, N-1], adjacency i64 [T, N-1, 3]"""
    assert kind in KINDS and base in KINDS and base != "mixpad", (kind, base)
    assert 4 <= N <= 64 and (N - 1) % 3 == 0, N
    rng = np.random.default_rng(seed)
    no = np.full((T, N), -2, np.int64)
    eo = np.full((T, N - 1), -2, np.int64)
    adj = np.full((T, N - 1, 3), -2, np.int64)
    for t in range(T):
        k = base if kind == "mixpad" else kind
        if kind == "mixpad" and t % 3 == 0:
            continue
        no[t], eo[t], adj[t] = _tree(k, N, rng, None if L is None else _pick(L, t), None if m is None else _pick(m, t))
    return no, eo, adj


def to_policy(x, no, eo, adj):
    """numpy per-tree arrays with tree-local ids -> the four torch tensors with a leading batch of 1 and global node ids"""
    T, N = no.shape
    adj = adj.copy()
    off = (np.arange(T, dtype=np.int64) * N).reshape(T, 1)
    for col in (0, 1):
        a = adj[:, :, col]
        adj[:, :, col] = np.where(a >= 0, a + off, -2)
    return (torch.from_numpy(np.ascontiguousarray(x)).view(1, T, N, F), torch.from_numpy(adj).view(1, T, N - 1, 3),
            torch.from_numpy(no.copy()).view(1, T, N), torch.from_numpy(eo.copy()).view(1, T, N - 1))


def make(kind, T, N, seed, feat="gauss", base="rand", L=None, m=None):
    no, eo, adj = structure(kind, T, N, seed, base, L, m)
    x = features(feat, T, N, np.random.default_rng([seed, 1]))
    return to_policy(x, no, eo, adj)


def level_populations(node_order, G):
    """{(group, height): nodes} of consecutive groups of G trees: what one workgroup of fl_tree_lstm finds on a level"""
    no = node_order.reshape(-1, node_order.shape[-1]).cpu().numpy()
    out = {}
    for g in range(0, len(no), G):
        v, c = np.unique(no[g:g + G][no[g:g + G] >= 0], return_counts=True)
        out.update({(g // G, int(a)): int(b) for a, b in zip(v, c)})
    return out


def spread(total, G):
    """G per-tree counts that add up to total, as even as possible"""
    return [total // G + (i < total % G) for i in range(G)]
