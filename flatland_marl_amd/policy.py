"""The policy network's tree encoder on the GPU: TreeLSTM (solution/nn/TreeLSTM.py) as one HIP launch (fl_tree_lstm).

`TreeLSTM` has the reference module's submodules, parameter names and shapes, so a reference checkpoint loads unchanged, and it
takes the tensors BatchedRailEnv.obs_policy() returns (adjacency already modified) as they are.  The kernel reads the live
parameter tensors at every call: after load_state_dict or an in-place update the next forward uses the new values.  Inference
only: the output comes through an autograd.Function whose backward raises NotImplementedError.

Swap it into the reference's Network:  net.tree_lstm = TreeLSTM.from_module(net.tree_lstm)
"""
import torch
import torch.nn as nn

from . import hip_backend

IN_FEATURES = 12      # FeatureParserConfig.node_sz
OUT_FEATURES = 128    # NetworkConfig.tree_embedding_sz
PARAM_ORDER = ("W_iou.weight", "W_iou.bias", "U_iou.weight", "W_c.weight", "W_c.bias", "W_f.weight", "W_f.bias", "U_f.weight")


class TreeLSTMViolation(ValueError):
    """check=True found trees that break the reference's grouping (their outputs are unspecified)."""


class _Forward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, forest, adjacency, node_order, edge_order, roots_only, status, *weights):
        B, A, N = forest.shape[:3]
        T = B * A
        h = torch.empty((T if roots_only else T * N, OUT_FEATURES), dtype=torch.float32, device=forest.device)
        hip_backend.tree_lstm(forest, adjacency, node_order, edge_order, weights, roots_only, h, status=status)
        return h

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("TreeLSTM (fl_tree_lstm) is inference only: no backward")


class TreeLSTM(nn.Module):
    """TreeLSTM(in_features=12, out_features=128) on fl_tree_lstm; forward(forest, adjacency, node_order, edge_order) returns
    h of every node, [B*A*N, 128] f32, as the reference does; roots(...) returns node 0 of every tree, [B, A, 128]."""

    def __init__(self, in_features=IN_FEATURES, out_features=OUT_FEATURES):
        super().__init__()
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
    def from_module(cls, m):
        """a TreeLSTM that shares m's parameters (m: the reference's TreeLSTM or one of these)"""
        if (m.in_features, m.out_features) != (IN_FEATURES, OUT_FEATURES):
            raise ValueError("TreeLSTM.from_module: only in_features=%d, out_features=%d exist here, got %d, %d"
                             % (IN_FEATURES, OUT_FEATURES, m.in_features, m.out_features))
        obj = cls.__new__(cls)
        nn.Module.__init__(obj)
        obj.in_features, obj.out_features = m.in_features, m.out_features
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
        self._check_inputs(forest, adjacency, node_order, edge_order)
        ws = self._weights(forest.device)
        status = torch.zeros(1, dtype=torch.int32, device=forest.device) if check else None
        out = _Forward.apply(forest, adjacency, node_order, edge_order, roots_only, status, *ws)
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
