"""The policy network on the GPU: TreeLSTM (solution/nn/TreeLSTM.py) as one HIP launch (fl_tree_lstm), and Network
(solution/nn/net_tree.py) with everything after the tree encoder -- attribute MLP, three attention blocks over the agents of an
env, actor and critic heads -- and the actor's choice of an action (solution/plfActor.py:30-46) as fl_policy_head.

`TreeLSTM` has the reference module's submodules, parameter names and shapes, so a reference checkpoint loads unchanged, and it
takes the tensors BatchedRailEnv.obs_policy() returns (adjacency already modified) as they are.  The kernel reads the live
parameter tensors at every call: after load_state_dict or an in-place update the next forward uses the new values.

By default the encoder is inference only: the output comes through an autograd.Function whose backward raises NotImplementedError.
TreeLSTM(trainable=True) (or m.trainable = True) makes forward / roots differentiable with respect to the eight parameters: the
forward is the same kernel (every node, c kept), the backward is fl_tree_lstm_backward (include/flatland_train.h) for everything
that follows the tree order, then the parameter gradients as float32 matrix products over all nodes, in chunks of
BACKWARD_CHUNK_TREES trees added in order.  Two backward passes on the same inputs give the same bits.  The forest gets no
gradient.

The head is inference only by default too: its backward raises.  Network(trainable=True) (or net.trainable = True,
Network.from_module(m, trainable=True)) makes head / forward differentiable with respect to the 38 head parameters and the tree
embedding: the forward is fl_policy_head_forward_saved (include/flatland_policy_train.h: the inference kernels, every block's q k v
and attention output kept; the same bits), the backward fl_policy_head_backward for everything per row and per env, then the 38
parameter gradients as the same float32 block products, in chunks of whole envs of at most HEAD_BACKWARD_CHUNK_ROWS rows added in
order.  agents_attr gets no gradient.  With both switches set one loss.backward() through Network.forward trains all 46 parameters
without a torch eager op on the forward path; Network.forward_torch / head_torch stay the head through torch's eager ops.

TreeLSTM(precision="bf16") (or m.precision = "bf16", Network(precision="bf16")) is the encoder for rolling out a trained policy:
fl_tree_lstm_bf16 (include/flatland_policy_bf16.h) runs the three recurrent products U_iou h_k, U_f h_k and W_c (f * c_k) on the
bf16 matrix instruction with float32 sums; W x, the biases, the gates and h / c stay float32, a leaf is computed as before.  The
module packs the three matrices to bf16 on first use and again whenever one of them changed, so the promise above holds.  It is
inference only: with trainable set it runs under torch.no_grad() and raises under grad mode.  The head stays float32 under it.

Network(head_precision="bf16") (or net.head_precision = "bf16") is the same for the head: fl_policy_head_bf16
(include/flatland_policy_head_bf16.h) runs 16 of the head's 19 matrices -- everything but attr_embedding.0 and the two heads' last
layers -- and the attention's two products on the bf16 matrix instruction with float32 sums; biases, GELU, the softmax's maxima, exp
and sums stay float32, q k v are kept in bf16.  The module packs the 16 matrices on first use and again whenever one of them changed.
Inference only, as the encoder's.  A whole bf16 roll-out is Network(precision="bf16", head_precision="bf16").

TreeLSTM(param_grads="hip") / Network(param_grads="hip") (or the attribute param_grads of either, or from_module(m,
param_grads="hip")) take the parameter gradients from the library as well: fl_tree_lstm_param_grads and fl_policy_head_param_grads
(include/flatland_param_grads.h), one grouped MFMA kernel per chunk with _tn's summation order fixed in the kernel, so that the
gradients of a chunk are the same bits from call to call whatever the BLAS library does.  "torch", the default, is the products
below.  Network's value governs the head, its tree_lstm keeps its own; Network(param_grads="hip") sets both.

What PPO needs per step is here too (include/flatland_ppo.h): sample_actions / Network.rollout draw an action per agent with that
agent's own uniform number and return its log-probability and entropy (fl_policy_sample: the draw is fl_policy_head's "soft" draw,
so the reference's constant u reproduces Network.act); gae forms advantages and returns (fl_gae); ppo_loss is the clipped
surrogate with the value and entropy terms as an autograd.Function over fl_ppo_loss, so loss.backward() through
Network(trainable=True).forward runs no torch eager op between the HIP forward and the HIP backward.  The loop, the roll-out buffer
and the optimiser are the caller's.

Swap it into the reference's Network:  net.tree_lstm = TreeLSTM.from_module(net.tree_lstm)
or take the whole network:              net = Network.from_module(net)
"""
import torch
import torch.nn as nn

from . import hip_backend

IN_FEATURES = 12      # FeatureParserConfig.node_sz
OUT_FEATURES = 128    # NetworkConfig.tree_embedding_sz
PRECISIONS = ("f32", "bf16")
PARAM_GRADS = ("torch", "hip")
PARAM_ORDER = ("W_iou.weight", "W_iou.bias", "U_iou.weight", "W_c.weight", "W_c.bias", "W_f.weight", "W_f.bias", "U_f.weight")


class TreeLSTMViolation(ValueError):
    """check=True found trees that break the reference's grouping (their outputs are unspecified)."""


BACKWARD_CHUNK_TREES = 4096      # trees a fl_tree_lstm_backward launch: its per-node buffers and workspace are 8.2 KB a node
REDUCE_BLOCK = 256               # nodes a float32 partial product of a parameter gradient


def _tn(a, b):
    """a^T b over the rows, [n, p] x [n, q] -> [p, q], summed in a fixed order: whole blocks of REDUCE_BLOCK rows as one batched
    float32 product, the partial products added in float64, then the ragged rest.  Short blocks and the float64 sum keep the
    rounding of a sum over 10^5 nodes at that of one block: one long float32 product over all rows measured up to 3.6x the error
    of torch's own float32 autograd, which sums level by level"""
    n = a.shape[0]
    main = n - n % REDUCE_BLOCK
    out = None
    if main:
        out = torch.bmm(a[:main].view(-1, REDUCE_BLOCK, a.shape[1]).transpose(1, 2),
                        b[:main].view(-1, REDUCE_BLOCK, b.shape[1])).sum(0, dtype=torch.float64)
    if main < n:
        rest = torch.matmul(a[main:].t(), b[main:]).double()
        out = rest if out is None else out + rest
    return out.to(a.dtype)


def _colsum(a):
    """the sum over the rows, accumulated in float64"""
    return a.sum(0, dtype=torch.float64).to(a.dtype)


def tree_lstm_param_grads(x, node_order, h, da, dc, dg, q, child):
    """the eight parameter gradients, in PARAM_ORDER, from fl_tree_lstm_backward's per-node rows (include/flatland_train.h): x f32
    [n, 12], node_order i64 [n], h f32 [n, 128], da [n, 384], dc [n, 128], dg [n, 3, 128], q [n, 384], child i32 [n, 3] (ids into
    these very rows, -1 = read as zero)"""
    n = x.shape[0]
    zero = x.new_zeros(())
    x = torch.where((node_order >= 0).view(n, 1), x, zero)                   # (a padding node's features must not matter: 0 * nan)
    hk = torch.where((child >= 0).view(n, 3, 1), h[child.clamp(min=0).long()], zero)
    dgs = dg.sum(1)
    return (_tn(da, x), _colsum(da), _tn(da, hk.view(n, 3 * OUT_FEATURES)), _tn(dc, q),
            _colsum(torch.where((node_order >= 1).view(n, 1), dc, zero)), _tn(dgs, x), _colsum(dgs),
            _tn(dg.reshape(3 * n, OUT_FEATURES), hk.view(3 * n, OUT_FEATURES)))


class _TrainForward(torch.autograd.Function):
    """fl_tree_lstm on every node with c kept, fl_tree_lstm_backward + the parameter products behind it"""

    @staticmethod
    def forward(ctx, forest, adjacency, node_order, edge_order, roots_only, status, hip_grads, *weights):
        B, A, N = forest.shape[:3]
        T = B * A
        h = torch.empty((T * N, OUT_FEATURES), dtype=torch.float32, device=forest.device)
        c = torch.empty_like(h)
        hip_backend.tree_lstm(forest, adjacency, node_order, edge_order, weights, False, h, c, status=status)
        ctx.roots_only, ctx.hip_grads = roots_only, hip_grads
        ctx.save_for_backward(forest, adjacency, node_order, edge_order, h, c, *weights)
        return h.view(T, N, OUT_FEATURES)[:, 0].contiguous() if roots_only else h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        forest, adjacency, node_order, edge_order, h, c = ctx.saved_tensors[:6]
        weights = ctx.saved_tensors[6:]
        B, A, N = forest.shape[:3]
        T, M, dev = B * A, OUT_FEATURES, forest.device
        grad = grad.to(torch.float32).contiguous().view(T if ctx.roots_only else T * N, M)
        x, adj = forest.view(T, N, IN_FEATURES), adjacency.view(T, N - 1, 3)
        no, eo = node_order.view(T, N), edge_order.view(T, N - 1)
        hv, cv, gv = h.view(T, N, M), c.view(T, N, M), grad.view(T, -1, M)
        total = None
        for t0 in range(0, T, BACKWARD_CHUNK_TREES):
            t1 = min(T, t0 + BACKWARD_CHUNK_TREES)
            n = (t1 - t0) * N
            a = adj[t0:t1]
            if t0:                                                # node ids count from the chunk's first tree
                shift = torch.zeros(3, dtype=torch.int64, device=dev)
                shift[:2] = t0 * N
                a = torch.where(a >= 0, a - shift, a)
            da = torch.empty((n, 3 * M), dtype=torch.float32, device=dev)
            dc = torch.empty((n, M), dtype=torch.float32, device=dev)
            dg = torch.empty((n, 3, M), dtype=torch.float32, device=dev)
            q = torch.empty((n, 3 * M), dtype=torch.float32, device=dev)
            child = torch.empty((n, 3), dtype=torch.int32, device=dev)
            hc = hv[t0:t1].reshape(n, M)
            hip_backend.tree_lstm_backward(x[t0:t1], a, no[t0:t1], eo[t0:t1], weights, hc, cv[t0:t1].reshape(n, M),
                                           gv[t0:t1].reshape(-1, M), ctx.roots_only, da, dc, dg, q, child)
            grads = hip_backend.tree_lstm_param_grads if ctx.hip_grads else tree_lstm_param_grads
            part = grads(x[t0:t1].reshape(n, IN_FEATURES), no[t0:t1].reshape(n), hc, da, dc, dg, q, child)
            total = part if total is None else tuple(u + v for u, v in zip(total, part))
        need = ctx.needs_input_grad[7:]
        return (None,) * 7 + tuple(g if k else None for g, k in zip(total, need))


class _Forward(torch.autograd.Function):
    """the inference forward: fl_tree_lstm (packed None), or fl_tree_lstm_bf16 on the packed bf16 buffer"""

    @staticmethod
    def forward(ctx, forest, adjacency, node_order, edge_order, roots_only, status, packed, *weights):
        B, A, N = forest.shape[:3]
        T = B * A
        h = torch.empty((T if roots_only else T * N, OUT_FEATURES), dtype=torch.float32, device=forest.device)
        if packed is None:
            hip_backend.tree_lstm(forest, adjacency, node_order, edge_order, weights, roots_only, h, status=status)
        else:
            hip_backend.tree_lstm_bf16(forest, adjacency, node_order, edge_order, weights, packed, roots_only, h, status=status)
        ctx.bf16 = packed is not None
        return h

    @staticmethod
    def backward(ctx, *grads):
        if ctx.bf16:
            raise NotImplementedError("TreeLSTM (fl_tree_lstm_bf16) is inference only: no backward; training runs precision='f32'")
        raise NotImplementedError("TreeLSTM (fl_tree_lstm) is inference only: no backward")


def _precision(value, what="TreeLSTM: precision"):
    if value not in PRECISIONS:
        raise ValueError("%s must be 'f32' or 'bf16', got %r" % (what, value))
    return value


def _param_grads(value, what):
    if value not in PARAM_GRADS:
        raise ValueError("%s: param_grads must be 'torch' or 'hip', got %r" % (what, value))
    return value


def _switches(module, trainable, attr, precision, what):
    """the plain attributes TreeLSTM and Network share: trainable, the precision switch `attr` (`what` names it in a refusal) and
    _packed, the cache of _packed_bf16, empty"""
    module.trainable = bool(trainable)
    setattr(module, attr, _precision(precision, what))
    module._packed = {}


def _packed_bf16(module, pack, ws, matrices, device):
    """The bf16 buffer of the matrices ws[i], i in `matrices`, for torch's current stream, kept in module._packed as (device, stream)
    -> (what was packed, the buffer): packed by pack(ws, the old buffer or None) at the first use on that stream, and again when one
    of the matrices is another tensor (data_ptr) or was written in place (_version) since -- load_state_dict and an optimizer step
    both are; a write through `.data` bumps no version and is not seen (clear module._packed after one).  One buffer a stream,
    packed and read on that stream only, so no launch waits on another stream's."""
    key = tuple((ws[i].data_ptr(), ws[i]._version) for i in matrices)
    slot = (device, torch.cuda.current_stream(device).cuda_stream)
    have = module._packed.get(slot)
    if have is None or have[0] != key:
        module._packed[slot] = have = (key, pack(ws, None if have is None else have[1]))
    return have[1]


class TreeLSTM(nn.Module):
    """TreeLSTM(in_features=12, out_features=128) on fl_tree_lstm; forward(forest, adjacency, node_order, edge_order) returns
    h of every node, [B*A*N, 128] f32, as the reference does; roots(...) returns node 0 of every tree, [B, A, 128].
    trainable (a plain attribute, settable): False = inference only, backward raises; True = with grad mode on, forward and roots
    are differentiable with respect to the parameters (fl_tree_lstm_backward), their values the same bits as the inference path's.
    precision (a plain attribute, settable): "f32" = fl_tree_lstm; "bf16" = fl_tree_lstm_bf16, the recurrent products with bf16
    operands and float32 sums, inference only -- together with trainable it runs under torch.no_grad() and raises ValueError under
    grad mode (training stays float32: the backward recomputes float32 gates from the saved h / c).
    param_grads (a plain attribute, settable): "torch" = the eight parameter gradients as torch products (tree_lstm_param_grads);
    "hip" = fl_tree_lstm_param_grads, the same sums in one deterministic kernel."""

    def __init__(self, in_features=IN_FEATURES, out_features=OUT_FEATURES, trainable=False, precision="f32", param_grads="torch"):
        super().__init__()
        _switches(self, trainable, "precision", precision, "TreeLSTM: precision")
        self.param_grads = _param_grads(param_grads, "TreeLSTM")
        if (in_features, out_features) != (IN_FEATURES, OUT_FEATURES):
            raise ValueError("TreeLSTM: only in_features=%d, out_features=%d exist here, got %d, %d"
                             % (IN_FEATURES, OUT_FEATURES, in_features, out_features))
        self.in_features = in_features
        self.out_features = out_features
        self.W_iou = nn.Linear(in_features, 3 * out_features)
        self.U_iou = nn.Linear(3 * out_features, 3 * out_features, bias=False)
        self.W_c = nn.Linear(3 * out_features, out_features)
        self.W_f = nn.Linear(in_features, out_features)
        self.U_f = nn.Linear(out_features, out_features, bias=False)

    @classmethod
    def from_module(cls, m, trainable=False, precision="f32", param_grads="torch"):
        """a TreeLSTM that shares m's parameters (m: the reference's TreeLSTM or one of these)"""
        if (m.in_features, m.out_features) != (IN_FEATURES, OUT_FEATURES):
            raise ValueError("TreeLSTM.from_module: only in_features=%d, out_features=%d exist here, got %d, %d"
                             % (IN_FEATURES, OUT_FEATURES, m.in_features, m.out_features))
        obj = cls.__new__(cls)
        nn.Module.__init__(obj)
        obj.in_features, obj.out_features = m.in_features, m.out_features
        _switches(obj, trainable, "precision", precision, "TreeLSTM: precision")
        obj.param_grads = _param_grads(param_grads, "TreeLSTM")
        for name in ("W_iou", "U_iou", "W_c", "W_f", "U_f"):
            setattr(obj, name, getattr(m, name))
        return obj

    def _weights(self, device):
        sd = dict(self.named_parameters())
        ws = []
        for name in PARAM_ORDER:
            w = sd[name]
            if w.dtype != torch.float32 or w.device != device or not w.is_contiguous():
                raise TypeError("TreeLSTM: parameter %s must be a contiguous float32 tensor on %s (got %s on %s%s)"
                                % (name, device, w.dtype, w.device, "" if w.is_contiguous() else ", not contiguous"))
            ws.append(w)
        return ws

    @staticmethod
    def _check_inputs(forest, adjacency, node_order, edge_order):
        for name, x, dt in (("forest", forest, torch.float32), ("adjacency", adjacency, torch.int64),
                            ("node_order", node_order, torch.int64), ("edge_order", edge_order, torch.int64)):
            if not isinstance(x, torch.Tensor):
                raise TypeError("TreeLSTM: %s must be a tensor" % name)
            if x.dtype != dt:
                raise TypeError("TreeLSTM: %s must be %s, got %s" % (name, dt, x.dtype))
            if x.device.type != "cuda":
                raise TypeError("TreeLSTM: %s must be on a GPU, got %s" % (name, x.device))
            if x.device != forest.device:
                raise TypeError("TreeLSTM: %s is on %s, forest on %s" % (name, x.device, forest.device))
            if not x.is_contiguous():
                raise ValueError("TreeLSTM: %s must be contiguous" % name)
        if forest.dim() != 4 or forest.shape[3] != IN_FEATURES:
            raise ValueError("TreeLSTM: forest must be [B, A, N, %d], got %s" % (IN_FEATURES, tuple(forest.shape)))
        B, A, N = forest.shape[:3]
        for name, x, shape in (("adjacency", adjacency, (B, A, N - 1, 3)), ("node_order", node_order, (B, A, N)),
                               ("edge_order", edge_order, (B, A, N - 1))):
            if tuple(x.shape) != shape:
                raise ValueError("TreeLSTM: %s must be %s, got %s" % (name, shape, tuple(x.shape)))
        if B * A == 0:
            raise ValueError("TreeLSTM: no trees")
        if N < 4 or N > 64 or (N - 1) % 3:
            raise ValueError("TreeLSTM: %d nodes a tree: 4 <= N <= 64 and (N - 1) %% 3 == 0 are required (the reference pairs "
                             "each level's nodes with triples of its edges)" % N)

    def _run(self, forest, adjacency, node_order, edge_order, roots_only, check):
        bf16 = _precision(self.precision) == "bf16"
        train = self.trainable and torch.is_grad_enabled()
        if bf16 and train:
            raise ValueError("TreeLSTM: precision='bf16' is inference only (fl_tree_lstm_backward recomputes float32 gates): run it "
                             "under torch.no_grad(), or train with precision='f32'")
        self._check_inputs(forest, adjacency, node_order, edge_order)
        ws = self._weights(forest.device)
        status = torch.zeros(1, dtype=torch.int32, device=forest.device) if check else None
        if train and forest.requires_grad:
            raise ValueError("TreeLSTM: the forest gets no gradient (fl_tree_lstm_backward differentiates with respect to the "
                             "parameters only): detach it")
        if train:
            hip_grads = _param_grads(self.param_grads, "TreeLSTM") == "hip"
            out = _TrainForward.apply(forest, adjacency, node_order, edge_order, roots_only, status, hip_grads, *ws)
        else:                                        # U_iou, W_c and U_f (items 2, 3, 7) are the packed ones
            packed = _packed_bf16(self, hip_backend.tree_lstm_pack_bf16, ws, (2, 3, 7), forest.device) if bf16 else None
            out = _Forward.apply(forest, adjacency, node_order, edge_order, roots_only, status, packed, *ws)
        if check:
            bad = int(status.item())
            if bad:
                raise TreeLSTMViolation("TreeLSTM: %d tree(s) break the reference's grouping (every node of height n > 0 needs "
                                        "its three edges one after another, in node order, inside its own tree)" % bad)
        return out

    def forward(self, forest, adjacency, node_order, edge_order, check=False):
        """h of every node, [B*A*N, 128]; check=True reads the status word back (a host sync) and raises on violations"""
        return self._run(forest, adjacency, node_order, edge_order, False, check)

    def roots(self, forest, adjacency, node_order, edge_order, check=False):
        """h of node 0 of every tree, [B, A, 128]: what Network.forward keeps (net_tree.py:77-80), without the other nodes' output"""
        B, A = forest.shape[:2]
        return self._run(forest, adjacency, node_order, edge_order, True, check).view(B, A, OUT_FEATURES)


# ---------------------------------------------------------------------------------------------------------------- Network
AGENT_ATTR = 83       # FeatureParserConfig.agent_attr
HIDDEN = 128          # NetworkConfig.hidden_sz
EMBED = HIDDEN + OUT_FEATURES
HEADS = 4
ACTIONS = 5           # FeatureParserConfig.action_sz
U_REFERENCE = hip_backend.POLICY_U_REFERENCE
# the state_dict without tree_lstm.*, in state_dict order: the parameter list of fl_policy_head (include/flatland_policy.h)
HEAD_PARAM_ORDER = tuple(
    ["attr_embedding.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]
    + ["transformer.%d.%s" % (i, k) for i in range(3)
       for k in ("attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias",
                 "att_mlp.0.weight", "att_mlp.0.bias")]
    + ["%s.%d.%s" % (n, i, k) for n in ("actor_net", "critic_net") for i in (0, 2, 4) for k in ("weight", "bias")])


class Transformer(nn.Module):
    """one attention block: MultiheadAttention over the agents of an env (sequence = agents, batch = envs), then
    att_mlp = GELU(Linear([input | attention output])); no residual, no layer norm"""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.attention = nn.MultiheadAttention(embed_dim, num_heads)
        self.att_mlp = nn.Sequential(nn.Linear(2 * embed_dim, embed_dim), nn.GELU())

    def forward(self, x):
        seq = x.transpose(0, 1)                      # [A, B, E]
        out, _ = self.attention(seq, seq, seq, need_weights=False)
        return self.att_mlp(torch.cat([x, out.transpose(0, 1)], dim=-1))


def _mlp(sizes, last_act):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if last_act or i < len(sizes) - 2:
            layers.append(nn.GELU())
    return nn.Sequential(*layers)


class _Head(torch.autograd.Function):
    """the inference head: fl_policy_head (packed None), or fl_policy_head_bf16 on the packed bf16 buffer"""

    @staticmethod
    def forward(ctx, agents_attr, tree_embedding, valid_actions, mode, u, with_value, packed, *weights):
        B, A = agents_attr.shape[:2]
        dev = agents_attr.device
        logits = torch.empty((B, A, ACTIONS), dtype=torch.float32, device=dev)
        value = torch.empty((B,), dtype=torch.float32, device=dev) if with_value else None
        actions = torch.empty((B, A), dtype=torch.uint8, device=dev) if mode is not None else None
        if packed is None:
            hip_backend.policy_head(agents_attr, tree_embedding, weights, logits, value, valid_actions, actions, mode, u)
        else:
            hip_backend.policy_head_bf16(agents_attr, tree_embedding, weights, packed, logits, value, valid_actions, actions, mode, u)
        out = (logits,) + ((value,) if with_value else ()) + ((actions,) if actions is not None else ())
        if actions is not None:
            ctx.mark_non_differentiable(actions)
        ctx.bf16 = packed is not None
        return out

    @staticmethod
    def backward(ctx, *grads):
        if ctx.bf16:
            raise NotImplementedError("Network (fl_policy_head_bf16) is inference only: no backward; training runs head_precision='f32'")
        raise NotImplementedError("Network (fl_policy_head) is inference only: no backward; forward_torch is the path with autograd")


# (env, agent) rows a fl_policy_head_backward launch: saved forward + rows are 54.9 KB a row, 1.8 GB a chunk (8 192 rows measured
# 1.4x the unchunked forward at cfg5: 20 envs of 400 agents are one workgroup a CU and a launch tail per chunk)
HEAD_BACKWARD_CHUNK_ROWS = 32768


def head_chunks(B, A):
    """[(first env, env behind the last)]: the envs in order, in chunks of whole envs (the attention never crosses an env) of at most
    HEAD_BACKWARD_CHUNK_ROWS rows -- of one env where a single env has more"""
    per = max(1, HEAD_BACKWARD_CHUNK_ROWS // A)
    return [(e0, min(B, e0 + per)) for e0 in range(0, B, per)]


def policy_head_param_grads(attr, sv, rw, actor=True, critic=True):
    """the 38 parameter gradients, in HEAD_PARAM_ORDER, from fl_policy_head_backward's rows (include/flatland_policy_train.h): attr
    f32 [R, 83], sv / rw = hip_backend.policy_views of the saved forward / of the rows.  dW = sum over the rows of dZ^T X, db = sum of
    dZ (_tn, _colsum).  actor / critic False: that head's six are None (its rows were not written)."""
    def lin(dz, *xs):
        return [torch.cat([_tn(dz, x) for x in xs], dim=1) if len(xs) > 1 else _tn(dz, xs[0]), _colsum(dz)]
    out = lin(rw["attr.dz0"], attr) + lin(rw["attr.dz2"], rw["attr.h1"]) + lin(rw["attr.dz4"], rw["attr.h2"]) \
        + lin(rw["attr.dz6"], rw["attr.h3"])
    for i, y in enumerate(("emb", "y1", "y2")):
        out += lin(rw["dqkv%d" % i], sv[y]) + lin(rw["do%d" % i], sv["c%d" % i]) + lin(rw["dz%d" % i], sv[y], rw["o%d" % i])
    for name, n, on in (("actor", ACTIONS, actor), ("critic", 1, critic)):
        if on:
            out += lin(rw[name + ".dz0"], sv["emb"], sv["y3"]) + lin(rw[name + ".dz2"], rw[name + ".u1"]) \
                + lin(rw[name + ".dz4"][:, :n].contiguous(), rw[name + ".u2"])
        else:
            out += [None] * 6
    return out


def _aligned(t):
    """t, or a copy of it where a slice of whole envs does not start on 16 bytes"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _HeadTrain(torch.autograd.Function):
    """fl_policy_head_forward_saved per chunk of envs (with a mode: fl_policy_head's action choice behind it), and behind it
    fl_policy_head_backward + the parameter products, the chunks' gradients added in order"""

    @staticmethod
    def forward(ctx, agents_attr, tree_embedding, valid_actions, mode, u, with_value, hip_grads, *weights):
        B, A = agents_attr.shape[:2]
        dev = agents_attr.device
        chunks = head_chunks(B, A)
        ctx.hip_grads = hip_grads
        logits, values, saved = [], [], []
        for e0, e1 in chunks:
            lg = torch.empty((e1 - e0, A, ACTIONS), dtype=torch.float32, device=dev)
            va = torch.empty((e1 - e0,), dtype=torch.float32, device=dev) if with_value else None
            sv = torch.empty(hip_backend.policy_saved_floats(e1 - e0, A), dtype=torch.float32, device=dev)
            hip_backend.policy_head_forward_saved(_aligned(agents_attr[e0:e1]), tree_embedding[e0:e1], weights, lg, va, sv)
            logits.append(lg), values.append(va), saved.append(sv)
        logits = logits[0] if len(chunks) == 1 else torch.cat(logits)
        value = (values[0] if len(chunks) == 1 else torch.cat(values)) if with_value else None
        actions = None
        if mode is not None:                         # the choice is part of fl_policy_head's last kernel: that call once more
            actions = torch.empty((B, A), dtype=torch.uint8, device=dev)
            hip_backend.policy_head(agents_attr, tree_embedding, weights, torch.empty_like(logits), None, valid_actions, actions, mode, u)
            ctx.mark_non_differentiable(actions)
        ctx.chunks, ctx.n_saved, ctx.with_value = chunks, len(saved), with_value
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(agents_attr, tree_embedding, *saved, *weights)
        return (logits,) + ((value,) if with_value else ()) + ((actions,) if actions is not None else ())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logits, *more):
        agents_attr, tree_embedding = ctx.saved_tensors[:2]
        saved = ctx.saved_tensors[2:2 + ctx.n_saved]
        weights = ctx.saved_tensors[2 + ctx.n_saved:]
        B, A = agents_attr.shape[:2]
        dev = agents_attr.device
        g_value = more[0] if ctx.with_value else None
        nothing = (None,) * (7 + len(weights))
        if g_logits is None and g_value is None:
            return nothing
        if g_logits is not None:
            g_logits = g_logits.to(torch.float32).contiguous().view(B, A, ACTIONS)
        if g_value is not None:
            g_value = g_value.to(torch.float32).contiguous().view(B)
        total, gtree = None, []
        for (e0, e1), sv in zip(ctx.chunks, saved):
            R = (e1 - e0) * A
            attr = _aligned(agents_attr[e0:e1])
            rows = torch.empty(R * hip_backend.POLICY_ROW_FLOATS, dtype=torch.float32, device=dev)
            gt = torch.empty((e1 - e0, A, OUT_FEATURES), dtype=torch.float32, device=dev)
            hip_backend.policy_head_backward(attr, tree_embedding[e0:e1], weights, sv,
                                             None if g_logits is None else _aligned(g_logits[e0:e1]),
                                             None if g_value is None else _aligned(g_value[e0:e1]), gt, rows)
            if ctx.hip_grads:
                part = hip_backend.policy_head_param_grads(attr, sv, rows, g_logits is not None, g_value is not None)
            else:
                part = policy_head_param_grads(attr.view(R, AGENT_ATTR), hip_backend.policy_views(sv, hip_backend.POLICY_SAVED_LAYOUT, R),
                                               hip_backend.policy_views(rows, hip_backend.POLICY_ROWS_LAYOUT, R),
                                               g_logits is not None, g_value is not None)
            total = part if total is None else [None if v is None else w + v for w, v in zip(total, part)]
            gtree.append(gt)
        gtree = gtree[0] if len(gtree) == 1 else torch.cat(gtree)
        need = ctx.needs_input_grad
        return (None, gtree if need[1] else None) + (None,) * 5 + tuple(g if k else None for g, k in zip(total, need[7:]))


class Network(nn.Module):
    """The reference's Network (solution/nn/net_tree.py:32-103) with its submodule names and shapes, so load_state_dict of a
    reference checkpoint works unchanged; tree_lstm is this file's TreeLSTM, everything after it runs as fl_policy_head.
    trainable (a plain attribute, settable): False = the head is inference only, backward raises; True = with grad mode on, head
    and forward are differentiable with respect to the 38 head parameters and the tree embedding (fl_policy_head_forward_saved,
    fl_policy_head_backward), their values the same bits as the inference path's.  With tree_lstm.trainable set as well one
    loss.backward() trains all 46 parameters.
    precision: the tree encoder's (tree_lstm.precision, which stays settable): "bf16" = fl_tree_lstm_bf16 for roll-outs.  The head
    stays float32 under it.
    head_precision (a plain attribute, settable): "f32" = fl_policy_head; "bf16" = fl_policy_head_bf16 in head, forward and act: 16
    of the head's 19 matrices and the attention's products with bf16 operands and float32 sums, inference only -- together with
    trainable it runs under torch.no_grad() and raises ValueError under grad mode (training stays float32).
    param_grads (a plain attribute, settable): "torch" = the head's 38 parameter gradients as torch products
    (policy_head_param_grads); "hip" = fl_policy_head_param_grads.  It governs the head; tree_lstm.param_grads stays settable on its
    own, and the constructor's value sets both."""

    def __init__(self, trainable=False, precision="f32", head_precision="f32", param_grads="torch"):
        super().__init__()
        _switches(self, trainable, "head_precision", head_precision, "Network: head_precision")
        self.param_grads = _param_grads(param_grads, "Network")
        self.tree_lstm = TreeLSTM(IN_FEATURES, OUT_FEATURES, precision=precision, param_grads=param_grads)
        self.attr_embedding = _mlp((AGENT_ATTR, 2 * HIDDEN, 2 * HIDDEN, 2 * HIDDEN, HIDDEN), True)
        self.transformer = nn.Sequential(*[Transformer(EMBED, HEADS) for _ in range(3)])
        self.actor_net = _mlp((2 * EMBED, 2 * HIDDEN, HIDDEN, ACTIONS), False)
        self.critic_net = _mlp((2 * EMBED, 2 * HIDDEN, HIDDEN, 1), False)

    @classmethod
    def from_module(cls, m, trainable=False, precision=None, head_precision=None, param_grads=None):
        """a Network that shares m's parameters (m: the reference's Network or one of these); precision: the tree encoder's, None =
        m.tree_lstm's own ("f32" for the reference's); head_precision: None = m's own ("f32" for the reference's); param_grads: the
        head's and the encoder's, None = m's and m.tree_lstm's own ("torch" for the reference's)"""
        obj = cls.__new__(cls)
        nn.Module.__init__(obj)
        _switches(obj, trainable, "head_precision", getattr(m, "head_precision", "f32") if head_precision is None else head_precision,
                  "Network: head_precision")
        obj.param_grads = _param_grads(getattr(m, "param_grads", "torch") if param_grads is None else param_grads, "Network")
        obj.tree_lstm = TreeLSTM.from_module(m.tree_lstm, trainable=getattr(m.tree_lstm, "trainable", False),
                                             precision=getattr(m.tree_lstm, "precision", "f32") if precision is None else precision,
                                             param_grads=getattr(m.tree_lstm, "param_grads", "torch") if param_grads is None
                                             else param_grads)
        obj.attr_embedding = m.attr_embedding
        blocks = []
        for b in m.transformer:
            t = Transformer.__new__(Transformer)
            nn.Module.__init__(t)
            t.attention, t.att_mlp = b.attention, b.att_mlp
            blocks.append(t)
        obj.transformer = nn.Sequential(*blocks)
        obj.actor_net, obj.critic_net = m.actor_net, m.critic_net
        obj._head_weights(None)                      # the names and shapes are the ones the kernels take
        return obj

    def _head_weights(self, device):
        sd = dict(self.named_parameters())
        ref = dict(zip(HEAD_PARAM_ORDER, hip_backend.POLICY_HEAD_PARAM_SHAPES))
        ws = []
        for name in HEAD_PARAM_ORDER:
            if name not in sd or tuple(sd[name].shape) != ref[name]:
                raise ValueError("Network: parameter %s must have shape %s (got %s)"
                                 % (name, ref[name], tuple(sd[name].shape) if name in sd else None))
            w = sd[name]
            if device is not None and (w.dtype != torch.float32 or w.device != device or not w.is_contiguous()):
                raise TypeError("Network: parameter %s must be a contiguous float32 tensor on %s (got %s on %s%s)"
                                % (name, device, w.dtype, w.device, "" if w.is_contiguous() else ", not contiguous"))
            ws.append(w)
        return ws

    @staticmethod
    def _check_head_inputs(agents_attr, tree_embedding, valid_actions):
        for name, x, dt in (("agents_attr", agents_attr, torch.float32), ("tree_embedding", tree_embedding, torch.float32),
                            ("valid_actions", valid_actions, torch.uint8)):
            if x is None and name == "valid_actions":
                continue
            if not isinstance(x, torch.Tensor):
                raise TypeError("Network: %s must be a tensor" % name)
            if x.dtype != dt:
                raise TypeError("Network: %s must be %s, got %s" % (name, dt, x.dtype))
            if x.device.type != "cuda":
                raise TypeError("Network: %s must be on a GPU, got %s" % (name, x.device))
            if x.device != agents_attr.device:
                raise TypeError("Network: %s is on %s, agents_attr on %s" % (name, x.device, agents_attr.device))
            if not x.is_contiguous():
                raise ValueError("Network: %s must be contiguous" % name)
        if agents_attr.dim() != 3 or agents_attr.shape[2] != AGENT_ATTR:
            raise ValueError("Network: agents_attr must be [B, A, %d], got %s" % (AGENT_ATTR, tuple(agents_attr.shape)))
        B, A = agents_attr.shape[:2]
        if tuple(tree_embedding.shape) != (B, A, OUT_FEATURES):
            raise ValueError("Network: tree_embedding must be %s, got %s" % ((B, A, OUT_FEATURES), tuple(tree_embedding.shape)))
        if valid_actions is not None and tuple(valid_actions.shape) != (B, A, ACTIONS):
            raise ValueError("Network: valid_actions must be %s, got %s" % ((B, A, ACTIONS), tuple(valid_actions.shape)))
        if B == 0 or A == 0:
            raise ValueError("Network: no agents")
        if A > 1024:
            raise ValueError("Network: %d agents an env, at most 1024" % A)

    def head(self, agents_attr, tree_embedding, valid_actions=None, mode=None, u=None, value=True):
        """Everything after the tree encoder (fl_policy_head) on agents_attr f32 [B, A, 83] and tree_embedding f32 [B, A, 128] (what
        TreeLSTM.roots returns): ([logits [B, A, 5]], value [B]) as forward returns them (value=False: the critic is not run, value is
        None); with mode "soft" / "hard" and valid_actions u8 [B, A, 5] the actions u8 [B, A] come as a third item.  u: the uniform
        draw of "soft", None = the reference's constant (it seeds numpy with 42 before every draw).  With head_precision "bf16" the
        launches are fl_policy_head_bf16's."""
        if mode not in (None, "soft", "hard"):
            raise ValueError("Network: mode must be None, 'soft' or 'hard', got %r" % (mode,))
        if mode is not None and valid_actions is None:
            raise ValueError("Network: mode %r needs valid_actions" % mode)
        if u is not None and not 0.0 <= float(u) < 1.0:
            raise ValueError("Network: u must be in [0, 1), got %r" % (u,))
        bf16 = _precision(self.head_precision, "Network: head_precision") == "bf16"
        if bf16 and self.trainable and torch.is_grad_enabled():
            raise ValueError("Network: head_precision='bf16' is inference only (fl_policy_head_backward belongs to the float32 "
                             "forward): run it under torch.no_grad(), or train with head_precision='f32'")
        self._check_head_inputs(agents_attr, tree_embedding, valid_actions if mode is not None else None)
        ws = self._head_weights(agents_attr.device)
        train = self.trainable and torch.is_grad_enabled()
        if train and agents_attr.requires_grad:
            raise ValueError("Network: agents_attr gets no gradient (fl_policy_head_backward differentiates with respect to the "
                             "parameters and the tree embedding only): detach it")
        args = (agents_attr, tree_embedding, valid_actions if mode is not None else None, mode, u, bool(value))
        if train:
            out = list(_HeadTrain.apply(*args, _param_grads(self.param_grads, "Network") == "hip", *ws))
        else:
            packed = _packed_bf16(self, hip_backend.policy_head_pack_bf16, ws, hip_backend.POLICY_HEAD_BF16_MATRICES,
                                  agents_attr.device) if bf16 else None
            out = list(_Head.apply(*args, packed, *ws))
        logits = out.pop(0)
        val = out.pop(0) if value else None
        return ([logits], val) + ((out.pop(0),) if mode is not None else ())

    def forward(self, agents_attr, forest, adjacency, node_order, edge_order):
        """([logits [B, A, 5]], value [B]) as the reference's forward returns them.  The inputs are the tensors of
        BatchedRailEnv.obs_policy(): the adjacency is ALREADY MODIFIED (global node ids, negatives -2) -- the reference's forward
        modifies it itself (net_tree.py:75, 105-116), this one does not.  With trainable set the head's gradient on the tree
        embedding is the upstream of TreeLSTM.roots: with tree_lstm.trainable as well all 46 parameters get gradients, without it
        the encoder's output enters as a constant."""
        if self.trainable and not self.tree_lstm.trainable:
            with torch.no_grad():
                tree = self.tree_lstm.roots(forest, adjacency, node_order, edge_order)
        else:
            tree = self.tree_lstm.roots(forest, adjacency, node_order, edge_order)
        return self.head(agents_attr, tree)

    def act(self, agents_attr, forest, adjacency, node_order, edge_order, valid_actions, mode="soft", u=None):
        """the actions u8 [B, A] of Actor._choose_action per agent, on the device and ready for BatchedRailEnv.step(actions,
        filter_required=True); the inputs as for forward (adjacency already modified), valid_actions u8 [B, A, 5]"""
        if mode not in ("soft", "hard"):
            raise ValueError("Network.act: mode must be 'soft' or 'hard', got %r" % (mode,))
        with torch.no_grad():
            tree = self.tree_lstm.roots(forest, adjacency, node_order, edge_order)
            return self.head(agents_attr, tree, valid_actions, mode, u, value=False)[2]

    def rollout(self, agents_attr, forest, adjacency, node_order, edge_order, valid_actions, u=None, generator=None):
        """One on-policy step: forward and sample_actions under torch.no_grad(), with either precision of the encoder and of the
        head.  Returns (actions u8 [B, A] ready for BatchedRailEnv.step(actions, filter_required=True), logp f32 [B, A], entropy f32
        [B, A], value f32 [B], logits f32 [B, A, 5]); the inputs as for forward (adjacency already modified), valid_actions u8
        [B, A, 5]; u, generator: as for sample_actions (None: a uniform number per agent from torch's generator).  act stays the
        reference's draw."""
        with torch.no_grad():
            logits, value = self.forward(agents_attr, forest, adjacency, node_order, edge_order)
            actions, logp, entropy = sample_actions(logits[0], valid_actions, u, generator)
        return actions, logp, entropy, value, logits[0]

    def head_torch(self, agents_attr, tree_embedding):
        """head() through torch's eager ops on the same parameters, with autograd: ([logits], value)"""
        embedding = torch.cat([self.attr_embedding(agents_attr), tree_embedding], dim=2)
        both = torch.cat([embedding, self.transformer(embedding)], dim=-1)
        return [self.actor_net(both)], self.critic_net(both).mean(1).view(-1)

    def forward_torch(self, agents_attr, forest, adjacency, node_order, edge_order):
        """forward() with everything after the tree encoder in torch's eager ops: the path with autograd.  The tree encoder is
        fl_tree_lstm here as well: with tree_lstm.trainable set its parameters get gradients too (fl_tree_lstm_backward), so one
        call trains the whole network; without it its output enters as a constant.  The adjacency is already modified, as for
        forward."""
        if self.tree_lstm.trainable:
            tree = self.tree_lstm.roots(forest, adjacency, node_order, edge_order)
        else:
            with torch.no_grad():
                tree = self.tree_lstm.roots(forest, adjacency, node_order, edge_order)
        return self.head_torch(agents_attr, tree)


def _rows(name, t, like, dtype):
    """t as a contiguous tensor of dtype with like's leading shape (the rows), on like's device"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != like.device or tuple(t.shape) != tuple(like.shape[:-1]):
        raise ValueError("%s must be a %s tensor of shape %s on %s" % (name, dtype, tuple(like.shape[:-1]), like.device))
    return t.detach().contiguous()


def _check_logits(what, logits, valid_actions):
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device.type != "cuda" or logits.dim() < 1 \
            or logits.shape[-1] != ACTIONS or logits.numel() == 0:
        raise ValueError("%s: logits must be a float32 [..., %d] tensor on a GPU" % (what, ACTIONS))
    if not isinstance(valid_actions, torch.Tensor) or valid_actions.dtype != torch.uint8 or valid_actions.device != logits.device \
            or tuple(valid_actions.shape) != tuple(logits.shape):
        raise ValueError("%s: valid_actions must be a uint8 tensor of shape %s on %s" % (what, tuple(logits.shape), logits.device))


def sample_actions(logits, valid_actions, u=None, generator=None):
    """(actions u8 [B, A], logp f32 [B, A], entropy f32 [B, A]) of logits f32 [B, A, 5] under the mask valid_actions u8 [B, A, 5]
    (fl_policy_sample, include/flatland_ppo.h): the reference actor's soft draw per agent with that agent's own uniform number, the
    log-probability of the drawn action and the entropy of the masked softmax, both evaluated in float64.  u: a float64 [B, A] tensor
    in [0, 1), used as given; a Python float, that value for every agent (hip_backend.POLICY_U_REFERENCE reproduces mode "soft");
    None: torch.rand in float64 on the logits' device from `generator`.  No gradient flows through it."""
    _check_logits("sample_actions", logits, valid_actions)
    dev, shape = logits.device, tuple(logits.shape[:-1])
    if u is None:
        u = torch.rand(shape, dtype=torch.float64, device=dev, generator=generator)
    elif isinstance(u, torch.Tensor):
        u = _rows("sample_actions: u", u, logits, torch.float64)
    else:
        if not 0.0 <= float(u) < 1.0:
            raise ValueError("sample_actions: u must be in [0, 1), got %r" % (u,))
        u = torch.full(shape, float(u), dtype=torch.float64, device=dev)
    actions = torch.empty(shape, dtype=torch.uint8, device=dev)
    logp = torch.empty(shape, dtype=torch.float32, device=dev)
    entropy = torch.empty(shape, dtype=torch.float32, device=dev)
    hip_backend.policy_sample(logits.detach().contiguous(), valid_actions.contiguous(), u, actions, logp, entropy)
    return actions, logp, entropy


class _PpoLoss(torch.autograd.Function):
    """fl_ppo_loss: the loss with its gradients in one call; backward scales them by the upstream scalar on the device"""

    @staticmethod
    def forward(ctx, logits, value, valid_actions, actions, old_logp, advantages, returns, mask, clip, vf_coef, ent_coef):
        dev = logits.device
        grad_logits = torch.empty(logits.shape, dtype=torch.float32, device=dev)
        grad_value = None if value is None else torch.empty(value.shape, dtype=torch.float32, device=dev)
        stats = torch.empty(hip_backend.PPO_STATS, dtype=torch.float64, device=dev)
        hip_backend.ppo_loss(logits.detach().contiguous(), valid_actions, actions, old_logp, advantages, mask,
                             None if value is None else value.detach().contiguous(), returns, clip, vf_coef, ent_coef, grad_logits,
                             grad_value, stats)
        ctx.save_for_backward(grad_logits, grad_value)
        ctx.mark_non_differentiable(stats)
        return stats[3].clone(), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_stats):
        grad_logits, grad_value = ctx.saved_tensors
        g = g_loss.to(torch.float32)
        need = ctx.needs_input_grad
        return (grad_logits * g if need[0] else None, grad_value * g if grad_value is not None and need[1] else None) + (None,) * 9


def ppo_loss(logits, value, valid_actions, actions, old_logp, advantages, returns, mask=None, clip=0.2, vf_coef=0.5, ent_coef=0.01):
    """(loss, stats) of PPO's clipped surrogate with the value and entropy terms (fl_ppo_loss, include/flatland_ppo.h, which states
    the formulas): logits f32 [B, A, 5] and value f32 [B] as Network.forward returns them (value None, with returns None: no critic
    terms), valid_actions u8 [B, A, 5], actions u8 [B, A], old_logp f32 [B, A] and advantages f32 [B, A] of the roll-out, returns f32
    [B], mask u8 [B, A] or None (0 = the agent's step does not count).  loss: a 0-dim float64 tensor = stats[3]; loss.backward()
    hands the kernel's gradients, times the upstream scalar, to logits and value.  stats: the float64 [8] device tensor (L_pi, L_v,
    mean entropy, total, mean old_logp - logp, clipped share, counted rows, rows whose action is not valid)."""
    _check_logits("ppo_loss", logits, valid_actions)
    actions = _rows("ppo_loss: actions", actions, logits, torch.uint8)
    old_logp = _rows("ppo_loss: old_logp", old_logp, logits, torch.float32)
    advantages = _rows("ppo_loss: advantages", advantages, logits, torch.float32)
    if mask is not None:
        mask = _rows("ppo_loss: mask", mask, logits, torch.uint8)
    if (value is None) != (returns is None):
        raise ValueError("ppo_loss: value and returns are both given or both None")
    if value is not None:
        if not isinstance(value, torch.Tensor) or value.dtype != torch.float32 or value.device != logits.device or value.numel() == 0:
            raise ValueError("ppo_loss: value must be a float32 tensor on %s" % logits.device)
        if not isinstance(returns, torch.Tensor) or returns.dtype != torch.float32 or returns.device != logits.device \
                or tuple(returns.shape) != tuple(value.shape):
            raise ValueError("ppo_loss: returns must be a float32 tensor of shape %s on %s" % (tuple(value.shape), logits.device))
        returns = returns.detach().contiguous()
    for name, c in (("clip", clip), ("vf_coef", vf_coef), ("ent_coef", ent_coef)):
        if not float("-inf") < float(c) < float("inf") or (name == "clip" and float(c) < 0):
            raise ValueError("ppo_loss: %s must be finite%s, got %r" % (name, " and >= 0" if name == "clip" else "", c))
    return _PpoLoss.apply(logits, value, valid_actions.contiguous(), actions, old_logp, advantages, returns, mask, float(clip),
                          float(vf_coef), float(ent_coef))


def gae(rewards, values, dones, gamma=0.99, lam=0.95):
    """(advantages f32 [T, N], returns f32 [T, N]) of rewards f32 [T, N], values f32 [T + 1, N] (the last row bootstraps) and dones
    u8 [T, N] (non-zero: the episode of that column ended with step t) by generalised advantage estimation in float64 (fl_gae,
    include/flatland_ppo.h).  N is whatever the caller estimates per column: envs, or (env, agent) pairs."""
    if not isinstance(rewards, torch.Tensor) or rewards.dtype != torch.float32 or rewards.dim() != 2 or rewards.numel() == 0 \
            or rewards.device.type != "cuda":
        raise ValueError("gae: rewards must be a float32 [T, N] tensor on a GPU")
    T, N = rewards.shape
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.device != rewards.device \
            or tuple(values.shape) != (T + 1, N):
        raise ValueError("gae: values must be a float32 tensor of shape %s on %s" % ((T + 1, N), rewards.device))
    if not isinstance(dones, torch.Tensor) or dones.dtype != torch.uint8 or dones.device != rewards.device \
            or tuple(dones.shape) != (T, N):
        raise ValueError("gae: dones must be a uint8 tensor of shape %s on %s" % ((T, N), rewards.device))
    if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):
        raise ValueError("gae: gamma and lam must be in [0, 1], got %r and %r" % (gamma, lam))
    adv = torch.empty((T, N), dtype=torch.float32, device=rewards.device)
    ret = torch.empty((T, N), dtype=torch.float32, device=rewards.device)
    hip_backend.gae(rewards.detach().contiguous(), values.detach().contiguous(), dones.contiguous(), gamma, lam, adv, ret)
    return adv, ret
