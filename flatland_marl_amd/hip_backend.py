"""ctypes binding of the C-ABI in include/flatland_hip.h (csrc/libflatland_hip.so) and the batched
tensor-level env on top of it.  torch is used for device buffers and streams only.

There is NO CPU fallback: every compute entry point fails loudly when the HIP library is missing or
no GPU is visible.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libflatland_hip.so")

FL_OK = 0
ERR_NAMES = {1: "FL_ERR_ARG", 2: "FL_ERR_HIP", 3: "FL_ERR_EPISODE_DONE", 4: "FL_ERR_STATE_SYNC",
             5: "FL_ERR_ZERO_TRANSITION", 6: "FL_ERR_CAPACITY"}
# the public headers' constants, restated (tests/test_cabi_headers.py holds each to its header); POLICY_SAVED_FLOATS and POLICY_ROW_FLOATS
# (FL_POLICY_HEAD_SAVED_FLOATS, FL_POLICY_HEAD_ROW_FLOATS) follow from the layout tables below
FL_STEP_AUTO_RESET, FL_STEP_FILTER_REQUIRED = 1, 2
FL_OBS_KEEP_TREE_ROWS = 1
ACTION_ABSENT = 255
STATE_COLS = 12
AUX_COLS = 4
PPO_STATS = 8
PARAM_GRADS_MAX_SLICES = 32
POLICY_HEAD_NPARAMS = 38
POLICY_SELECT = {None: 0, "soft": 1, "hard": 2}      # FL_POLICY_SELECT_NONE, _SOFT, _HARD
POLICY_U_REFERENCE = 0.3745401188473625      # numpy.random.RandomState(42).random_sample(): the reference seeds before every draw
# the 16 matrices fl_policy_head_pack_bf16 rounds, as indices into the 38 parameters, in the packed buffer's order
POLICY_HEAD_BF16_MATRICES = (2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 32, 34)
STATE_NAMES = ("row", "col", "dir", "state", "malf", "nmalf", "scount", "saved", "arrival",
               "old_row", "old_col", "old_dir")

vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
_cutils7 = [vp] * 7        # attr, forest, adjacency, node_order, edge_order, valid_actions, props
_tree3 = [i32, i32, vp]    # tree_max_depth, tree_pred_depth, tree_out
# header file name (include/) -> {name: (argtypes, restype)} of every function it declares, in the header's order
ABI = {
    "flatland_hip.h": {
        "fl_last_error": ([], C.c_char_p),
        "fl_version": ([], i32),
        "fl_device_count": ([], i32),
        "fl_create": ([i32, i32, i32, i32, i32, C.POINTER(vp)], i32),
        "fl_destroy": ([vp], None),
        "fl_set_stream": ([vp, vp], i32),
        "fl_sync": ([vp], i32),
        "fl_load_env": ([vp, i32] + [vp] * 7 + [i32, u64, i32, i32, vp, i32], i32),
        "fl_reserve": ([vp, i32, i32], i32),
        "fl_commit": ([vp], i32),
        "fl_set_rng": ([vp, vp, vp], i32),
        "fl_get_rng": ([vp, vp, vp], i32),
        "fl_reset": ([vp, vp, i32], i32),
        "fl_reset_dev": ([vp, vp, i32], i32),
        "fl_step": ([vp, vp, vp, vp, vp, i32], i32),
        "fl_step_synth": ([vp, u32, u32, i32, vp, vp, vp, i32], i32),
        "fl_step_obs": ([vp, vp, u32, u32, i32, vp, vp, vp, i32, i32, i32] + _cutils7 + _tree3, i32),
        "fl_obs_cutils_tree": ([vp, i32, i32] + _cutils7 + _tree3, i32),
        "fl_metrics": ([vp, vp, i32], i32),
        "fl_scores": ([vp, vp, i32], i32),
        "fl_check": ([vp], i32),
        "fl_obs_cutils": ([vp, i32, i32] + _cutils7, i32),
        "fl_obs_cutils_handles": ([vp, i32, i32, vp, i32] + _cutils7, i32),
        "fl_obs_cutils_policy": ([vp, i32, i32] + _cutils7, i32),
        "fl_obs_tree": ([vp, i32, i32, vp], i32),
        "fl_obs_tree_handles": ([vp, i32, i32, vp, i32, vp], i32),
        "fl_obs_global": ([vp, i32, i32, i32, vp, vp, vp], i32),
        "fl_obs_set_mode": ([vp, i32], i32),
        "fl_info": ([vp, vp, vp, vp, vp], i32),
        "fl_policy_pack": ([i32, i32, i32] + [vp] * 7, i32),
        "fl_tree_lstm_workspace_bytes": ([i32, i32, i32], C.c_size_t),
        "fl_tree_lstm": ([i32, i32] + [vp] * 12 + [i32, vp, vp, vp, vp, C.c_size_t, vp], i32),
        "fl_get_state": ([vp, vp, vp], i32),
        "fl_get_state_aux": ([vp, vp], i32),
        "fl_set_state": ([vp, vp, vp, vp, vp], i32),
        "fl_motion_check": ([i32, i32, vp, vp, vp, vp], i32),
        "fl_distance_map": ([vp, i32, C.POINTER(i32), vp, vp], i32),
        "fl_distance_map_rebuild": ([vp], i32),
        "fl_distance_map_rebuild_masked": ([vp, vp], i32),
        "fl_positions_map": ([vp, i32, vp], i32),
        "fl_algorithmic_bytes_per_agent_step": ([vp, i32, i32], C.c_double),
    },
    "flatland_policy.h": {
        "fl_policy_head_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head": ([i32, i32, vp, vp, C.POINTER(vp), vp, i32, C.c_double, vp, vp, vp, vp, C.c_size_t, vp], i32),
    },
    "flatland_train.h": {
        "fl_tree_lstm_backward_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_tree_lstm_backward": ([i32, i32] + [vp] * 15 + [i32] + [vp] * 7 + [C.c_size_t, vp], i32),
    },
    "flatland_policy_train.h": {
        "fl_policy_head_saved_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head_forward_saved": ([i32, i32, vp, vp, C.POINTER(vp), vp, vp, vp, C.c_size_t, vp], i32),
        "fl_policy_head_backward_rows_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head_backward_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head_backward": ([i32, i32, vp, vp, C.POINTER(vp), vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp], i32),
    },
    "flatland_predict.h": {
        "fl_predict": ([vp, i32, i32, i32, i32, vp, vp, vp], i32),
    },
    "flatland_wrappers.h": {
        "fl_action_space": ([vp, i32, i32, i32, vp, vp, vp, vp, vp, vp], i32),
        "fl_decision_cells": ([vp, i32, i32, vp], i32),
    },
    "flatland_policy_bf16.h": {
        "fl_tree_lstm_bf16_packed_bytes": ([], C.c_size_t),
        "fl_tree_lstm_pack_bf16": ([vp, vp, vp, vp, C.c_size_t, vp], i32),
        "fl_tree_lstm_bf16_workspace_bytes": ([i32, i32, i32], C.c_size_t),
        "fl_tree_lstm_bf16": ([i32, i32] + [vp] * 10 + [C.c_size_t, i32, vp, vp, vp, vp, C.c_size_t, vp], i32),
    },
    "flatland_policy_head_bf16.h": {
        "fl_policy_head_bf16_packed_bytes": ([], C.c_size_t),
        "fl_policy_head_pack_bf16": ([C.POINTER(vp), vp, C.c_size_t, vp], i32),
        "fl_policy_head_bf16_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head_bf16": ([i32, i32, vp, vp, C.POINTER(vp), vp, C.c_size_t, vp, i32, C.c_double, vp, vp, vp, vp, C.c_size_t, vp], i32),
    },
    "flatland_param_grads.h": {
        "fl_policy_head_param_grads_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_policy_head_param_grads": ([i32, i32, vp, vp, vp, i32, i32, C.POINTER(vp), i32, vp, C.c_size_t, vp], i32),
        "fl_tree_lstm_param_grads_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_tree_lstm_param_grads": ([i32] + [vp] * 8 + [C.POINTER(vp), i32, vp, C.c_size_t, vp], i32),
    },
    "flatland_ppo.h": {
        "fl_policy_sample": ([i32, vp, vp, vp, vp, vp, vp, vp], i32),
        "fl_ppo_loss_workspace_bytes": ([i32, i32], C.c_size_t),
        "fl_ppo_loss": ([i32, i32] + [vp] * 8 + [C.c_double] * 3 + [vp, vp, vp, vp, C.c_size_t, vp], i32),
        "fl_gae": ([i32, i32, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp], i32),
    },
}
# diagnostics the library exports beside the public headers
DEBUG_ABI = {
    "fl_debug_last_obs_class": ([vp, vp], i32),
    "fl_debug_last_obs_launch": ([vp, vp, i32], i32),
    # the host half of a handle alone (csrc/fl_static.h), no GPU needed: new(B, A, H, W), free, load (fl_load_env's arguments after the
    # handle), reserve, commit, read(name, env or -1, out, capacity in bytes) -> bytes
    "fl_debug_static_new": ([i32, i32, i32, i32], vp),
    "fl_debug_static_free": ([vp], None),
    "fl_debug_static_load": ([vp, i32] + [vp] * 7 + [i32, u64, i32, i32, vp, i32], i32),
    "fl_debug_static_reserve": ([vp, i32, i32], i32),
    "fl_debug_static_commit": ([vp], i32),
    "fl_debug_static_read": ([vp, C.c_char_p, i32, vp, C.c_longlong], C.c_longlong),
    # the library's copy of POLICY_SAVED_LAYOUT (table 0), POLICY_ROWS_LAYOUT (1) and POLICY_HEAD_PARAM_SHAPES (2), csrc/fl_policy_layout.h:
    # (table, entry or -1 for the count, name out, its capacity, a out, b out)
    "fl_debug_policy_layout": ([i32, i32, C.c_char_p, i32, C.POINTER(i32), C.POINTER(i32)], i32),
    # the launcher's table of environment switches (csrc/fl_obs_switches.h) as text, no GPU needed: (out, its capacity) -> bytes
    "fl_debug_obs_switches": ([C.c_char_p, i32], i32),
}
_lib = None


class FlatlandHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, code), msg))
        self.code = code


class EpisodeDoneError(FlatlandHipError):
    """RailEnv.step raises Exception("Episode is done, cannot call step()") (rail_env.py:508-509)."""


def build(force=False):
    env = dict(os.environ)
    if force:
        env["FORCE"] = "1"
    subprocess.check_call([os.path.join(HERE, "csrc", "build.sh")], env=env, stdout=subprocess.DEVNULL)
    return LIB_PATH


def symbols(header=None):
    """the names one header declares, in its order (None: those of all ten, in the table's order)"""
    return tuple(name for h in ([header] if header else ABI) for name in ABI[h])


def bind(L, groups=None):
    """argtypes and restype of every function of the groups (keys of ABI or "debug"; None: all of them) on the ctypes.CDLL L,
    which it returns.  No torch, no GPU."""
    for g in (*ABI, "debug") if groups is None else groups:
        for name, (args, res) in (DEBUG_ABI if g == "debug" else ABI[g]).items():
            fn = getattr(L, name, None)        # (a library from bench.py --lib or a tool's LIB_PATH may predate the newer ones)
            if fn is not None:
                fn.argtypes, fn.restype = args, res
    return L


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                "%s is missing: build it with flatland_marl_amd/csrc/build.sh (hipcc --offload-arch=gfx950); "
                "there is no CPU fallback" % LIB_PATH)
        # torch ships its own HIP runtime (same soname as /opt/rocm's): it has to be the one this process loads first,
        # otherwise torch.cuda finds no device once the library below has pulled in the system runtime
        import torch  # noqa: F401
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def _sym(name):
    """entry point `name` of the loaded library -- which may be an older build that does not have it yet"""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise FlatlandHipError(1, "the loaded library has no %s (an older build loaded through --lib?)" % name)
    return fn


def obs_switches():
    """the observation launcher's diagnostic environment switches, from the library's own table: {name: (kind, what it rules out)} with kind
    "flag" / "int" / "bytes" / "keys" and "nothing" / "bins" / "classes".  No GPU."""
    fn = _sym("fl_debug_obs_switches")
    buf = C.create_string_buffer(fn(None, 0))
    assert fn(buf, len(buf)) == len(buf)
    return {name: (kind, out) for name, kind, out in (ln.split() for ln in buf.value.decode().splitlines())}


def _chk(rc):
    if rc != FL_OK:
        msg = lib().fl_last_error().decode()
        if rc == 3:
            raise EpisodeDoneError(rc, msg)
        raise FlatlandHipError(rc, msg)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_tensors(what, dev, specs, torch_names=False):
    """The tensor checks of the policy wrappers.  specs: (name, tensor or None, dtype, minimum elements or None); a tensor that is
    given must be contiguous, of that dtype, on dev, and hold at least that many elements.  The message names the dtype as
    "float32", or with torch_names as "torch.float32"."""
    for name, o, dt, n in specs:
        if o is not None and (o.dtype != dt or o.device != dev or not o.is_contiguous() or (n is not None and o.numel() < n)):
            raise ValueError("%s: %s must be a contiguous %s tensor %son %s"
                             % (what, name, dt if torch_names else str(dt).replace("torch.", ""),
                                "" if n is None else "of at least %d elements " % n, dev))


def _call(fn, dev, workspace_bytes, *args):
    """fn(*args[, workspace, its bytes], stream) on torch's current stream of dev, with a workspace from torch's allocator
    (workspace_bytes None: the entry point takes none); raises on a refusal"""
    import torch
    with torch.cuda.device(dev):
        if workspace_bytes is not None:
            ws = torch.empty(max(workspace_bytes, 16), dtype=torch.uint8, device=dev)
            args += (ws.data_ptr(), ws.numel())
        _chk(fn(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def _opt(t):
    return None if t is None else t.data_ptr()


def malf_threshold(rate):
    """ceil((1 - exp(-rate)) * 2**53): `np_random.rand() < _malfunction_prob(rate)` as a 53-bit integer
    compare (malfunction_generators.py:24-33,46-53)."""
    if rate <= 0:
        return 0
    p = float(1 - np.exp(-rate))
    return int(math.ceil(p * 2.0 ** 53))


def motion_check(offsets, cur, nxt, device=0):
    """MotionCheck (agent_chains.py:19-236) on independent agent lists through the step kernel's conflict resolution
    (fl_motion_check): cur / nxt are cell ids or -1 (off the map); returns can_move as a bool array."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    cur = np.ascontiguousarray(cur, dtype=np.int32)
    nxt = np.ascontiguousarray(nxt, dtype=np.int32)
    out = np.zeros(max(len(cur), 1), dtype=np.uint8)
    _chk(lib().fl_motion_check(int(device), len(offsets) - 1, _p(offsets), _p(cur), _p(nxt), _p(out)))
    return out[:len(cur)].astype(bool)


def policy_pack(adjacency, node_order, edge_order, adj_out, no_out, eo_out):
    """int32 device tensors [B,A,E,3] / [B,A,E+1] / [B,A,E] -> int64 outputs (fl_policy_pack) on torch's current stream."""
    import torch
    B, A, E = adjacency.shape[:3]
    s = torch.cuda.current_stream(adjacency.device).cuda_stream
    _chk(lib().fl_policy_pack(B, A, E, adjacency.data_ptr(), node_order.data_ptr(), edge_order.data_ptr(),
                              adj_out.data_ptr(), no_out.data_ptr(), eo_out.data_ptr(), C.c_void_p(s)))


def tree_lstm(forest, adjacency, node_order, edge_order, weights, roots_only, h, c=None, status=None):
    """TreeLSTM.forward (fl_tree_lstm) on torch's current stream of the inputs' device, with a workspace from torch's allocator.
    forest f32 [..., N, 12], adjacency i64 [..., N-1, 3] (modified), node_order i64 [..., N], edge_order i64 [..., N-1], all
    contiguous on one device; weights = (W_iou.weight, W_iou.bias, U_iou.weight, W_c.weight, W_c.bias, W_f.weight, W_f.bias,
    U_f.weight), f32 contiguous; h (and c, if given) f32 [T*N, 128] or, roots_only, [T, 128]; status i32 [1] or None."""
    return _tree_lstm("tree_lstm", forest, adjacency, node_order, edge_order, weights, None, roots_only, h, c, status)


def _tree_lstm(what, forest, adjacency, node_order, edge_order, weights, packed, roots_only, h, c, status):
    """tree_lstm (packed None) and tree_lstm_bf16: fl_<what>"""
    import torch
    N = forest.shape[-2]
    T = forest.numel() // (N * 12)
    dev = forest.device
    fn = _sym("fl_" + what)
    bf16 = what == "tree_lstm_bf16"
    if bf16 and len(weights) != 8:
        raise ValueError("%s: %d weights, 8 expected" % (what, len(weights)))
    rows = (T if roots_only else T * N) * 128
    _check_tensors(what, dev, (("h", h, torch.float32, rows), ("c", c, torch.float32, rows)))
    if bf16:
        if packed.dtype != torch.uint8 or packed.device != dev or not packed.is_contiguous():
            raise ValueError("%s: packed must be a contiguous uint8 tensor on %s (tree_lstm_pack_bf16)" % (what, dev))
        mats = [weights[i].data_ptr() for i in (0, 1, 4, 5, 6)] + [packed.data_ptr(), packed.numel()]
    else:
        mats = [w.data_ptr() for w in weights]
    _call(fn, dev, _sym("fl_%s_workspace_bytes" % what)(T, N, int(roots_only)),
          T, N, forest.data_ptr(), adjacency.data_ptr(), node_order.data_ptr(), edge_order.data_ptr(), *mats, int(roots_only),
          h.data_ptr(), _opt(c), _opt(status))
    return h


def _pack_bf16(kind, dev, out, elements, *args):
    """The second half of tree_lstm_pack_bf16 and policy_head_pack_bf16 (kind "tree_lstm" / "policy_head"): out (None: a new
    buffer) and the call fl_<kind>_pack_bf16(*args, out, its bytes, stream).  elements: how many the matrices have together, where
    that is still to be compared with the buffer's size (None: checked already)"""
    import torch
    what = kind + "_pack_bf16"
    fn = _sym("fl_" + what)
    nbytes = _sym("fl_%s_bf16_packed_bytes" % kind)()
    if elements is not None and elements * 2 != nbytes:
        raise ValueError("%s: the 16 matrices must have %d elements together" % (what, nbytes // 2))
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _check_tensors(what, dev, [("out", out, torch.uint8, nbytes)])
    _call(fn, dev, None, *args, out.data_ptr(), out.numel())
    return out


def tree_lstm_pack_bf16(weights, out=None):
    """The three recurrent matrices rounded to bf16 in one buffer (fl_tree_lstm_pack_bf16, include/flatland_policy_bf16.h) on
    torch's current stream of the weights' device.  weights: the eight tensors tree_lstm takes, of which U_iou.weight, W_c.weight and
    U_f.weight (items 2, 3, 7) are read; out: a uint8 tensor of at least fl_tree_lstm_bf16_packed_bytes() bytes to pack into (None:
    a new one).  Returns the packed buffer: pack again after the weights changed."""
    import torch
    if len(weights) != 8:
        raise ValueError("tree_lstm_pack_bf16: %d weights, 8 expected" % len(weights))
    u_iou, w_c, u_f = weights[2], weights[3], weights[7]
    dev = u_iou.device
    for name, w, n in (("U_iou.weight", u_iou, 384 * 384), ("W_c.weight", w_c, 128 * 384), ("U_f.weight", u_f, 128 * 128)):
        if w.dtype != torch.float32 or w.device != dev or not w.is_contiguous() or w.numel() != n:
            raise ValueError("tree_lstm_pack_bf16: %s must be a contiguous float32 tensor of %d elements on %s" % (name, n, dev))
    return _pack_bf16("tree_lstm", dev, out, None, u_iou.data_ptr(), w_c.data_ptr(), u_f.data_ptr())


def tree_lstm_bf16(forest, adjacency, node_order, edge_order, weights, packed, roots_only, h, c=None, status=None):
    """TreeLSTM.forward with bf16 matrix operands in the three recurrent products (fl_tree_lstm_bf16,
    include/flatland_policy_bf16.h), for inference, on torch's current stream of the inputs' device, with a workspace from torch's
    allocator.  Inputs, weights (the eight of tree_lstm: the five float32 ones are read), h, c and status as for tree_lstm; packed:
    what tree_lstm_pack_bf16 made of the same weights."""
    return _tree_lstm("tree_lstm_bf16", forest, adjacency, node_order, edge_order, weights, packed, roots_only, h, c, status)


def tree_lstm_backward(forest, adjacency, node_order, edge_order, weights, h, c, grad_h, roots_only, da, dc, dg, q, child,
                       status=None):
    """The tree-ordered part of TreeLSTM's gradient (fl_tree_lstm_backward, include/flatland_train.h) on torch's current stream of
    the inputs' device, with a workspace from torch's allocator.  Inputs and weights as for tree_lstm; h, c f32 [T*N, 128] of every
    node from the forward; grad_h f32 [T*N, 128] or, roots_only, [T, 128].  Outputs, per node: da f32 [T*N, 384], dc f32
    [T*N, 128], dg f32 [T*N, 3, 128], q f32 [T*N, 384], child i32 [T*N, 3]; status i32 [1] or None.  No parameter gradient is
    written: policy.tree_lstm_param_grads forms them from these rows."""
    import torch
    N = forest.shape[-2]
    T = forest.numel() // (N * 12)
    fn = _sym("fl_tree_lstm_backward")
    dev = forest.device
    if len(weights) != 8:
        raise ValueError("tree_lstm_backward: %d weights, 8 expected" % len(weights))
    _check_tensors("tree_lstm_backward", dev,
                   [("forest", forest, torch.float32, None), ("adjacency", adjacency, torch.int64, None),
                    ("node_order", node_order, torch.int64, None), ("edge_order", edge_order, torch.int64, None)]
                   + [("weight %d" % i, w, torch.float32, None) for i, w in enumerate(weights)], torch_names=True)
    if adjacency.numel() != T * (N - 1) * 3 or node_order.numel() != T * N or edge_order.numel() != T * (N - 1):
        raise ValueError("tree_lstm_backward: index tensors of %d trees x %d nodes are expected" % (T, N))
    _check_tensors("tree_lstm_backward", dev,
                   (("h", h, torch.float32, T * N * 128), ("c", c, torch.float32, T * N * 128),
                    ("grad_h", grad_h, torch.float32, (T if roots_only else T * N) * 128),
                    ("da", da, torch.float32, T * N * 384), ("dc", dc, torch.float32, T * N * 128),
                    ("dg", dg, torch.float32, T * N * 384), ("q", q, torch.float32, T * N * 384),
                    ("child", child, torch.int32, T * N * 3)), torch_names=True)
    _call(fn, dev, _sym("fl_tree_lstm_backward_workspace_bytes")(T, N),
          T, N, forest.data_ptr(), adjacency.data_ptr(), node_order.data_ptr(), edge_order.data_ptr(),
          *[w.data_ptr() for w in weights], h.data_ptr(), c.data_ptr(), grad_h.data_ptr(), int(roots_only),
          da.data_ptr(), dc.data_ptr(), dg.data_ptr(), q.data_ptr(), child.data_ptr(), _opt(status))


def policy_head(agents_attr, tree_embedding, params, logits, value=None, valid_actions=None, actions=None, mode=None, u=None):
    """The policy network after its tree encoder and the actor's choice (fl_policy_head) on torch's current stream of the inputs'
    device, with a workspace from torch's allocator.  agents_attr f32 [B, A, 83], tree_embedding f32 [B, A, 128]; params = the 38
    tensors of include/flatland_policy.h in its order, f32 contiguous; logits f32 [B, A, 5]; value f32 [B] or None (the critic is
    not run); mode None / "soft" / "hard" with valid_actions u8 [B, A, 5] and actions u8 [B, A]; u None = the reference's constant."""
    return _policy_head("policy_head", agents_attr, tree_embedding, params, None, logits, value, valid_actions, actions, mode, u)


def _policy_head(what, agents_attr, tree_embedding, params, packed, logits, value, valid_actions, actions, mode, u):
    """policy_head (packed None) and policy_head_bf16: fl_<what>"""
    import torch
    B, A = agents_attr.shape[:2]
    fn = _sym("fl_" + what)
    if mode not in POLICY_SELECT:
        raise ValueError("%s: mode must be None, 'soft' or 'hard', got %r" % (what, mode))
    if len(params) != POLICY_HEAD_NPARAMS:
        raise ValueError("%s: %d parameters, %d expected" % (what, len(params), POLICY_HEAD_NPARAMS))
    dev = agents_attr.device
    _check_tensors(what, dev, (("logits", logits, torch.float32, B * A * 5), ("value", value, torch.float32, B),
                               ("valid_actions", valid_actions, torch.uint8, B * A * 5), ("actions", actions, torch.uint8, B * A)),
                   torch_names=True)
    bf16 = what == "policy_head_bf16"
    if bf16 and (packed.dtype != torch.uint8 or packed.device != dev or not packed.is_contiguous()):
        raise ValueError("%s: packed must be a contiguous uint8 tensor on %s (policy_head_pack_bf16)" % (what, dev))
    weights = [(vp * POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in params])] + ([packed.data_ptr(), packed.numel()] if bf16 else [])
    _call(fn, dev, _sym("fl_%s_workspace_bytes" % what)(B, A),
          B, A, agents_attr.data_ptr(), tree_embedding.data_ptr(), *weights, _opt(valid_actions), POLICY_SELECT[mode],
          POLICY_U_REFERENCE if u is None else float(u), logits.data_ptr(), _opt(value), _opt(actions))
    return logits


def policy_head_pack_bf16(weights, out=None):
    """The head's 16 bf16 matrices in one buffer (fl_policy_head_pack_bf16, include/flatland_policy_head_bf16.h) on torch's current
    stream of the weights' device.  weights: the 38 tensors policy_head takes, of which POLICY_HEAD_BF16_MATRICES are read; out: a
    uint8 tensor of at least fl_policy_head_bf16_packed_bytes() bytes to pack into (None: a new one).  Returns the packed buffer:
    pack again after the weights changed."""
    import torch
    if len(weights) != POLICY_HEAD_NPARAMS:
        raise ValueError("policy_head_pack_bf16: %d parameters, %d expected" % (len(weights), POLICY_HEAD_NPARAMS))
    dev = weights[POLICY_HEAD_BF16_MATRICES[0]].device
    for i in POLICY_HEAD_BF16_MATRICES:
        w = weights[i]
        if w.dtype != torch.float32 or w.device != dev or not w.is_contiguous() or w.dim() != 2:
            raise ValueError("policy_head_pack_bf16: parameter %d must be a contiguous float32 matrix on %s" % (i, dev))
    return _pack_bf16("policy_head", dev, out, sum(weights[i].numel() for i in POLICY_HEAD_BF16_MATRICES),
                      (vp * POLICY_HEAD_NPARAMS)(*[None if w is None else w.data_ptr() for w in weights]))


def policy_head_bf16(agents_attr, tree_embedding, params, packed, logits, value=None, valid_actions=None, actions=None, mode=None,
                     u=None):
    """policy_head with bf16 matrix operands in 16 of its 19 matrices (fl_policy_head_bf16, include/flatland_policy_head_bf16.h),
    for inference, on torch's current stream of the inputs' device, with a workspace from torch's allocator.  The arguments of
    policy_head; packed: what policy_head_pack_bf16 made of the same params."""
    return _policy_head("policy_head_bf16", agents_attr, tree_embedding, params, packed, logits, value, valid_actions, actions, mode, u)


# (name, floats a row) of the arrays of saved_dev and rows_dev, in their order (include/flatland_policy_train.h): array k of R rows
# starts at R * (the floats a row of the arrays before it)
POLICY_SAVED_LAYOUT = ((("emb", 256), ("y1", 256), ("y2", 256), ("y3", 256)) + tuple(("c%d" % i, 256) for i in range(3))
                       + tuple(("qkv%d" % i, 768) for i in range(3)) + (("val", 1),))
POLICY_ROWS_LAYOUT = ((("attr.dz0", 256), ("attr.dz2", 256), ("attr.dz4", 256), ("attr.dz6", 128), ("attr.h1", 256), ("attr.h2", 256),
                       ("attr.h3", 256))
                      + tuple(("%s%d" % (n, i), k) for i in range(3)
                              for n, k in (("dqkv", 768), ("do", 256), ("dz", 256), ("o", 256), ("dc", 256), ("dy", 256)))
                      + (("dy3", 256),)
                      + tuple(("%s.%s" % (h, n), k) for h, last in (("actor", 8), ("critic", 4))
                              for n, k in (("dz0", 256), ("dz2", 128), ("dz4", last), ("u1", 256), ("u2", 128))))
POLICY_SAVED_FLOATS = sum(k for _, k in POLICY_SAVED_LAYOUT)      # 4 097
POLICY_ROW_FLOATS = sum(k for _, k in POLICY_ROWS_LAYOUT)      # 9 612


def policy_views(buf, layout, R):
    """name -> the [R, n] view ([R] for n = 1) of every array of a float32 saved / rows buffer of R rows"""
    out, off = {}, 0
    for name, k in layout:
        v = buf[off * R:(off + k) * R]
        out[name] = v if k == 1 else v.view(R, k)
        off += k
    return out


def policy_saved_floats(B, A):
    """the float32 elements of a saved buffer of B envs x A agents (fl_policy_head_saved_bytes: whole 16 bytes)"""
    return _sym("fl_policy_head_saved_bytes")(B, A) // 4


def _policy_train_check(what, agents_attr, tree_embedding, params):
    import torch
    if len(params) != POLICY_HEAD_NPARAMS:
        raise ValueError("%s: %d parameters, %d expected" % (what, len(params), POLICY_HEAD_NPARAMS))
    dev = agents_attr.device
    B, A = agents_attr.shape[:2]
    _check_tensors(what, dev, [("agents_attr", agents_attr, torch.float32, B * A * 83),
                               ("tree_embedding", tree_embedding, torch.float32, B * A * 128)]
                   + [("parameter %d" % i, w, torch.float32, 1) for i, w in enumerate(params)])
    return B, A, dev


def policy_head_forward_saved(agents_attr, tree_embedding, params, logits, value, saved):
    """fl_policy_head without the action choice, keeping what the backward reads (fl_policy_head_forward_saved,
    include/flatland_policy_train.h) on torch's current stream of the inputs' device.  Inputs and params as for policy_head; logits
    f32 [B, A, 5]; value f32 [B] or None; saved: a float32 tensor of at least B * A * POLICY_SAVED_FLOATS elements."""
    import torch
    B, A, dev = _policy_train_check("policy_head_forward_saved", agents_attr, tree_embedding, params)
    _check_tensors("policy_head_forward_saved", dev, (("logits", logits, torch.float32, B * A * 5), ("value", value, torch.float32, B),
                                                      ("saved", saved, torch.float32, policy_saved_floats(B, A))))
    ptrs = (vp * POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in params])
    _call(_sym("fl_policy_head_forward_saved"), dev, None, B, A, agents_attr.data_ptr(), tree_embedding.data_ptr(), ptrs,
          logits.data_ptr(), _opt(value), saved.data_ptr(), saved.numel() * 4)
    return logits


def policy_head_backward(agents_attr, tree_embedding, params, saved, grad_logits, grad_value, grad_tree, rows):
    """The gradient of the policy head up to the sums over the rows (fl_policy_head_backward, include/flatland_policy_train.h) on
    torch's current stream of the inputs' device, with a workspace from torch's allocator.  saved: what policy_head_forward_saved
    left on the same inputs; grad_logits f32 [B, A, 5] or None; grad_value f32 [B] or None; grad_tree f32 [B, A, 128] (out); rows: a
    float32 tensor of at least B * A * POLICY_ROW_FLOATS elements (out).  No parameter gradient is written:
    policy.policy_head_param_grads forms them from the rows."""
    import torch
    B, A, dev = _policy_train_check("policy_head_backward", agents_attr, tree_embedding, params)
    _check_tensors("policy_head_backward", dev,
                   (("saved", saved, torch.float32, policy_saved_floats(B, A)), ("grad_logits", grad_logits, torch.float32, B * A * 5),
                    ("grad_value", grad_value, torch.float32, B), ("grad_tree", grad_tree, torch.float32, B * A * 128),
                    ("rows", rows, torch.float32, B * A * POLICY_ROW_FLOATS)))
    ptrs = (vp * POLICY_HEAD_NPARAMS)(*[w.data_ptr() for w in params])
    _call(_sym("fl_policy_head_backward"), dev, _sym("fl_policy_head_backward_workspace_bytes")(B, A),
          B, A, agents_attr.data_ptr(), tree_embedding.data_ptr(), ptrs, saved.data_ptr(), _opt(grad_logits), _opt(grad_value),
          grad_tree.data_ptr(), rows.data_ptr(), rows.numel() * 4)
    return grad_tree


# [out, in] of the 38 head parameters and of the encoder's 8, in the kernels' order (a bias: (out,))
POLICY_HEAD_PARAM_SHAPES = tuple(
    [s for o, k in ((256, 83), (256, 256), (256, 256), (128, 256)) for s in ((o, k), (o,))]
    + [s for _ in range(3) for o, k in ((768, 256), (256, 256), (256, 512)) for s in ((o, k), (o,))]
    + [s for last in (5, 1) for o, k in ((256, 512), (128, 256), (last, 128)) for s in ((o, k), (o,))])
TREE_LSTM_PARAM_SHAPES = ((384, 12), (384,), (384, 384), (128, 384), (128,), (128, 12), (128,), (128, 128))


def _param_grads_call(what, dev, rows, shapes, on, slices, workspace, *args):
    """fl_<what>(*args, grads, slices, workspace, its bytes, stream) with new output tensors of `shapes` (None where `on` is False)
    and the caller's workspace (a tensor of at least fl_<what>_workspace_bytes bytes) or one from torch's allocator"""
    import torch
    if not 0 <= slices <= PARAM_GRADS_MAX_SLICES:
        raise ValueError("%s: slices must be 0 (automatic) or in [1, %d], got %r" % (what, PARAM_GRADS_MAX_SLICES, slices))
    fn, need = _sym("fl_" + what), _sym("fl_%s_workspace_bytes" % what)(rows, slices)
    if workspace is not None and (workspace.device != dev or not workspace.is_contiguous()
                                  or workspace.numel() * workspace.element_size() < need):
        raise ValueError("%s: workspace must be a contiguous tensor of at least %d bytes on %s" % (what, need, dev))
    with torch.cuda.device(dev):
        grads = [torch.empty(s, dtype=torch.float32, device=dev) if k else None for s, k in zip(shapes, on)]
        if workspace is None and need:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ptrs = (vp * len(shapes))(*[_opt(g) for g in grads])
        _chk(fn(*args, ptrs, slices, _opt(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return grads


def policy_head_param_grads(agents_attr, saved, rows, actor=True, critic=True, slices=0, workspace=None):
    """The 38 gradients of the head's parameters (fl_policy_head_param_grads, include/flatland_param_grads.h) on torch's current
    stream of the inputs' device: agents_attr f32 [B, A, 83], saved / rows as policy_head_forward_saved / policy_head_backward left
    them for the same envs.  Returns a list of 38 new tensors in the parameters' order and shapes; actor / critic False: that head's
    six are None (its rows are not read).  slices: 0 = the library's choice, else the forced count; workspace: a tensor of at least
    fl_policy_head_param_grads_workspace_bytes(B * A, slices) bytes, None = from torch's allocator."""
    import torch
    B, A = agents_attr.shape[:2]
    dev = agents_attr.device
    _check_tensors("policy_head_param_grads", dev,
                   (("agents_attr", agents_attr, torch.float32, B * A * 83), ("saved", saved, torch.float32, policy_saved_floats(B, A)),
                    ("rows", rows, torch.float32, B * A * POLICY_ROW_FLOATS)))
    on = [True] * 26 + [bool(actor)] * 6 + [bool(critic)] * 6
    return _param_grads_call("policy_head_param_grads", dev, B * A, POLICY_HEAD_PARAM_SHAPES, on, int(slices), workspace,
                             B, A, agents_attr.data_ptr(), saved.data_ptr(), rows.data_ptr(), int(bool(actor)), int(bool(critic)))


def tree_lstm_param_grads(x, node_order, h, da, dc, dg, q, child, slices=0, workspace=None):
    """The 8 gradients of the tree encoder's parameters (fl_tree_lstm_param_grads, include/flatland_param_grads.h) on torch's
    current stream of the inputs' device: x f32 [n, 12], node_order i64 [n], h f32 [n, 128] and the rows tree_lstm_backward wrote
    for the same n nodes (da [n, 384], dc [n, 128], dg [n, 3, 128], q [n, 384], child i32 [n, 3]).  Returns a list of 8 new tensors
    in the parameters' order and shapes.  slices, workspace: as for policy_head_param_grads."""
    import torch
    n = node_order.numel()
    dev = x.device
    _check_tensors("tree_lstm_param_grads", dev,
                   (("x", x, torch.float32, n * 12), ("node_order", node_order, torch.int64, n), ("h", h, torch.float32, n * 128),
                    ("da", da, torch.float32, n * 384), ("dc", dc, torch.float32, n * 128), ("dg", dg, torch.float32, n * 384),
                    ("q", q, torch.float32, n * 384), ("child", child, torch.int32, n * 3)))
    return _param_grads_call("tree_lstm_param_grads", dev, n, TREE_LSTM_PARAM_SHAPES, [True] * 8, int(slices), workspace,
                             n, x.data_ptr(), node_order.data_ptr(), h.data_ptr(), da.data_ptr(), dc.data_ptr(), dg.data_ptr(),
                             q.data_ptr(), child.data_ptr())


def policy_sample(logits, valid_actions, u, actions, logp=None, entropy=None):
    """An action per (env, agent) row with that row's own uniform number, its log-probability and entropy (fl_policy_sample,
    include/flatland_ppo.h) on torch's current stream of the inputs' device.  logits f32 [..., 5], valid_actions u8 [..., 5], u f64
    [...] in [0, 1); actions u8 [...] (out), logp / entropy f32 [...] or None (out)."""
    import torch
    R = logits.numel() // 5
    dev = logits.device
    _check_tensors("policy_sample", dev, (("logits", logits, torch.float32, R * 5), ("valid_actions", valid_actions, torch.uint8, R * 5),
                                          ("u", u, torch.float64, R), ("actions", actions, torch.uint8, R),
                                          ("logp", logp, torch.float32, R), ("entropy", entropy, torch.float32, R)))
    _call(_sym("fl_policy_sample"), dev, None, R, logits.data_ptr(), valid_actions.data_ptr(), u.data_ptr(), actions.data_ptr(),
          _opt(logp), _opt(entropy))
    return actions


def ppo_loss(logits, valid_actions, actions, old_logp, advantages, mask, value, returns, clip, vf_coef, ent_coef, grad_logits,
             grad_value, stats):
    """The clipped-surrogate loss, its gradients and statistics (fl_ppo_loss, include/flatland_ppo.h) on torch's current stream of
    the inputs' device, with a workspace from torch's allocator.  logits f32 [R, 5], valid_actions u8 [R, 5], actions u8 [R],
    old_logp / advantages f32 [R], mask u8 [R] or None; value / returns f32 [B] and grad_value f32 [B] (out), or all three None;
    grad_logits f32 [R, 5] (out), stats f64 [8] (out)."""
    import torch
    R = logits.numel() // 5
    B = 0 if value is None else value.numel()
    dev = logits.device
    _check_tensors("ppo_loss", dev, (("logits", logits, torch.float32, R * 5), ("valid_actions", valid_actions, torch.uint8, R * 5),
                                     ("actions", actions, torch.uint8, R), ("old_logp", old_logp, torch.float32, R),
                                     ("advantages", advantages, torch.float32, R), ("mask", mask, torch.uint8, R),
                                     ("value", value, torch.float32, B), ("returns", returns, torch.float32, B),
                                     ("grad_logits", grad_logits, torch.float32, R * 5), ("grad_value", grad_value, torch.float32, B),
                                     ("stats", stats, torch.float64, PPO_STATS)))
    _call(_sym("fl_ppo_loss"), dev, _sym("fl_ppo_loss_workspace_bytes")(R, B), R, B, logits.data_ptr(), valid_actions.data_ptr(),
          actions.data_ptr(), old_logp.data_ptr(), advantages.data_ptr(), _opt(mask), _opt(value), _opt(returns), float(clip),
          float(vf_coef), float(ent_coef), grad_logits.data_ptr(), _opt(grad_value), stats.data_ptr())
    return stats


def gae(rewards, values, dones, gamma, lam, advantages, returns):
    """Generalised advantage estimation (fl_gae, include/flatland_ppo.h) on torch's current stream of the inputs' device: rewards
    f32 [T, N], values f32 [T + 1, N], dones u8 [T, N]; advantages / returns f32 [T, N] (out)."""
    import torch
    T, N = rewards.shape
    dev = rewards.device
    _check_tensors("gae", dev, (("rewards", rewards, torch.float32, T * N), ("values", values, torch.float32, (T + 1) * N),
                                ("dones", dones, torch.uint8, T * N), ("advantages", advantages, torch.float32, T * N),
                                ("returns", returns, torch.float32, T * N)))
    _call(_sym("fl_gae"), dev, None, T, N, rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), float(gamma), float(lam),
          advantages.data_ptr(), returns.data_ptr())
    return advantages, returns


class BatchedRailEnv:
    """B independent Flatland envs stepped in lock-step on one MI355X.

    `envs` is a list of B mappings with the static description of each env, as produced by the
    reference after reset(): grid u16[H,W], init_pos i32[A,2], init_dir i32[A], target i32[A,2],
    speed f64[A], earliest i32[A], latest i32[A], T, malf_rate, malf_min, malf_max, mt_key u32[624], mt_pos.
    All envs of one batch share (A, H, W).  reserve = (max unique targets, max rail cells) leaves room for maps loaded
    into the live batch later (replace_env); default: the largest env of `envs`.
    """

    def __init__(self, envs, device=0, max_nodes=31, pred_depth=500, reserve=None):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedRailEnv needs a HIP device (torch.cuda.is_available() is False); "
                               "the HIP path has no CPU fallback")
        L = lib()
        e0 = envs[0]
        self.B = len(envs)
        self.H, self.W = np.asarray(e0["grid"]).shape
        self.A = int(len(e0["init_dir"]))
        self.device = torch.device("cuda", device)
        self.max_nodes, self.pred_depth = max_nodes, pred_depth
        h = C.c_void_p()
        _chk(L.fl_create(self.B, self.A, self.H, self.W, device, C.byref(h)))
        self.h = h
        self.T = np.zeros(self.B, dtype=np.int32)
        if reserve is not None:
            _chk(L.fl_reserve(h, int(reserve[0]), int(reserve[1])))
        for b, e in enumerate(envs):
            self._load(b, e)
        with torch.cuda.device(self.device):
            _chk(L.fl_commit(h))
        B, A = self.B, self.A
        self.rewards = torch.zeros((B, A), dtype=torch.int32, device=self.device)
        self.dones = torch.zeros((B, A), dtype=torch.uint8, device=self.device)
        self.done_all = torch.zeros((B,), dtype=torch.uint8, device=self.device)
        self._obs = None                      # the cutils output tensors (made at the first use, dropped when max_nodes changes)
        self._tree = {}                       # (depth,) -> the upstream-tree tensor of that depth
        self._info = self._metrics = self._scores = self._pol = self._pol64 = None     # output tensors, made at the first use
        self._glob = {}                       # (dtype, b0, nb) -> obs_global's three tensors
        self._pred = {}                       # (max_depth, dtype, b0, nb) -> predictions' tensor, (max_depth, b0, nb) -> its two path tensors
        self._wrap = {}                       # (kind, ..., b0, nb) -> the tensors of the reduced action space (fl_action_space, fl_decision_cells)
        self.use_torch_stream()

    def _load(self, b, e):
        grid = np.ascontiguousarray(e["grid"], dtype=np.uint16)
        assert grid.shape == (self.H, self.W) and len(e["init_dir"]) == self.A
        a32 = lambda k: np.ascontiguousarray(e[k], dtype=np.int32)  # noqa: E731
        ip, idr, tg, ea, la = a32("init_pos"), a32("init_dir"), a32("target"), a32("earliest"), a32("latest")
        sp = np.ascontiguousarray(e["speed"], dtype=np.float64)
        key = np.ascontiguousarray(e["mt_key"], dtype=np.uint32)
        _chk(lib().fl_load_env(self.h, b, _p(grid), _p(ip), _p(idr), _p(tg), _p(sp), _p(ea), _p(la), int(e["T"]),
                               malf_threshold(float(e["malf_rate"])), int(e["malf_min"]), int(e["malf_max"]),
                               _p(key), int(e["mt_pos"])))
        self.T[b] = int(e["T"])

    def replace_env(self, b, env, commit=True):
        """RailEnv.reset(regenerate_rail=True, regenerate_schedule=True) for env b of the live batch (rail_env.py:288-320):
        a new map, new agents and a new RNG state; its distance maps and static tables are rebuilt on the GPU, its agents
        reset, the other envs keep running.  commit=False stages several replacements for one commit()."""
        self._load(b, env)
        if commit:
            self.commit()

    def commit(self):
        with self.torch.cuda.device(self.device):
            _chk(lib().fl_commit(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().fl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self):
        """enqueue on torch's current stream so torch ops and the kernels order naturally."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        _chk(lib().fl_set_stream(self.h, C.c_void_p(s)))

    # ---- dynamics
    def reset(self, mask=None, fresh=True):
        """mask: host array-like [B], a uint8 device tensor [B] (no host round trip), or None (= all envs)."""
        t = self.torch
        if isinstance(mask, t.Tensor) and mask.is_cuda:
            assert mask.dtype == t.uint8 and mask.numel() == self.B and mask.is_contiguous()
            _chk(lib().fl_reset_dev(self.h, mask.data_ptr(), int(fresh)))
            return
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        _chk(lib().fl_reset(self.h, None if m is None else _p(m), int(fresh)))

    def step(self, actions, auto_reset=False, filter_required=False):
        """actions: uint8 tensor [B, A] on the device (255 = agent not in the action dict).
        filter_required: ignore the actions of agents without action_required (eval_env.parse_actions)."""
        actions = self._actions(actions)
        _chk(lib().fl_step(self.h, actions.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr(), self.done_all.data_ptr(),
                           FL_STEP_AUTO_RESET * bool(auto_reset) | FL_STEP_FILTER_REQUIRED * bool(filter_required)))
        return self.rewards, self.dones, self.done_all

    def info(self):
        """get_info_dict as device tensors + evaluator scores of each env's last finished episode."""
        t = self.torch
        if self._info is None:
            B, A = self.B, self.A
            self._info = dict(action_required=t.zeros((B, A), dtype=t.uint8, device=self.device),
                              malfunction=t.zeros((B, A), dtype=t.int32, device=self.device),
                              state=t.zeros((B, A), dtype=t.uint8, device=self.device),
                              scores=t.zeros((B, 2), dtype=t.float64, device=self.device))
        i = self._info
        _chk(lib().fl_info(self.h, i["action_required"].data_ptr(), i["malfunction"].data_ptr(), i["state"].data_ptr(),
                           i["scores"].data_ptr()))
        return i

    def step_obs(self, actions=None, seed=0, stream_base=0, kind=0, auto_reset=False, filter_required=False, tree_depth=0,
                 tree_pred=30):
        """RailEnv.step() as the reference defines it: the tick AND the observations of the new state, one launch.
        actions None: the on-device synthetic stream (seed, stream_base, kind).  Returns (rewards, dones, done_all,
        cutils observation dict, upstream tree tensor or None)."""
        if actions is not None:
            actions = self._actions(actions)
        o = self._obs_buffers()
        tree = self._tree_buffer(tree_depth) if tree_depth > 0 else None
        _chk(lib().fl_step_obs(self.h, None if actions is None else actions.data_ptr(), int(seed), int(stream_base), int(kind),
                               self.rewards.data_ptr(), self.dones.data_ptr(), self.done_all.data_ptr(),
                               FL_STEP_AUTO_RESET * bool(auto_reset) | FL_STEP_FILTER_REQUIRED * bool(filter_required), self.max_nodes,
                               self.pred_depth, *self._cutils_ptrs(o), int(tree_depth), int(tree_pred), None if tree is None else tree.data_ptr()))
        return self.rewards, self.dones, self.done_all, o, tree

    def step_synth(self, seed, stream_base=0, kind=0, auto_reset=True):
        _chk(lib().fl_step_synth(self.h, int(seed), int(stream_base), int(kind), self.rewards.data_ptr(),
                                 self.dones.data_ptr(), self.done_all.data_ptr(), int(auto_reset)))
        return self.rewards, self.dones, self.done_all

    def metrics(self, reset=False):
        """int64[4] device tensor: (sum terminal rewards, arrived agents, agent-steps, finished episodes)."""
        if self._metrics is None:
            self._metrics = self.torch.zeros(4, dtype=self.torch.int64, device=self.device)
        _chk(lib().fl_metrics(self.h, self._metrics.data_ptr(), int(reset)))
        return self._metrics

    def scores(self, reset=False):
        """float64[3] device tensor: (sum of normalized rewards, sum of completion ratios, episodes) over the episodes finished
        since the counters were reset -- the evaluator's mean_normalized_reward / mean_percentage_complete as sums
        (flatland/evaluators/service.py:875-879, 900-913).  The episode count is the scores' own counter, reset with the sums
        (independent of metrics(reset=True))."""
        if self._scores is None:
            self._scores = self.torch.zeros(3, dtype=self.torch.float64, device=self.device)
        _chk(lib().fl_scores(self.h, self._scores.data_ptr(), int(reset)))
        return self._scores

    def check(self):
        _chk(lib().fl_check(self.h))

    def sync(self):
        _chk(lib().fl_sync(self.h))

    # ---- observations
    def _obs_buffers(self):
        if self._obs is None:
            t, B, A, N = self.torch, self.B, self.A, self.max_nodes
            dev = self.device
            self._obs = dict(
                agent_attr=t.zeros((B, A, 83), dtype=t.float32, device=dev),
                forest=t.zeros((B, A, N, 12), dtype=t.float32, device=dev),
                adjacency=t.zeros((B, A, N - 1, 3), dtype=t.int32, device=dev),
                node_order=t.zeros((B, A, N), dtype=t.int32, device=dev),
                edge_order=t.zeros((B, A, N - 1), dtype=t.int32, device=dev),
                valid_actions=t.zeros((B, A, 5), dtype=t.uint8, device=dev),
                props=t.zeros((B, A, 3), dtype=t.float64, device=dev))
        return self._obs

    def obs_outputs(self):
        """the flatland_cutils output tensors as the last observation call left them (obs_policy() returns five of the policy's
        inputs; valid_actions u8 [B, A, 5] and props are here), without a launch"""
        return self._obs_buffers()

    @staticmethod
    def _cutils_ptrs(o, index=None):
        """the seven flatland_cutils outputs as the C-ABI orders them; index: (adjacency, node_order, edge_order) tensors that take
        the place of o's (obs_policy's int64 ones)"""
        adj, no, eo = index if index is not None else (o["adjacency"], o["node_order"], o["edge_order"])
        return (o["agent_attr"].data_ptr(), o["forest"].data_ptr(), adj.data_ptr(), no.data_ptr(), eo.data_ptr(),
                o["valid_actions"].data_ptr(), o["props"].data_ptr())

    def _tree_buffer(self, depth):
        """the upstream-tree tensor of a depth: one object per depth, handed out by every call (see keep_tree_rows)"""
        key = (depth,)
        if key not in self._tree:
            n = (4 ** (depth + 1) - 1) // 3
            self._tree[key] = self.torch.zeros((self.B, self.A, n, 12), dtype=self.torch.float64, device=self.device)
        return self._tree[key]

    def _actions(self, actions):
        """a host array or a device tensor -> contiguous uint8 [B, A] on the device"""
        t = self.torch
        if not (isinstance(actions, t.Tensor) and actions.is_cuda):
            actions = t.as_tensor(np.ascontiguousarray(actions, dtype=np.uint8)).to(self.device)
        actions = actions.contiguous()
        assert actions.dtype == t.uint8 and actions.shape == (self.B, self.A)
        return actions

    def obs_cutils(self, handles=None):
        """flatland_cutils.TreeObsForRailEnv.get_many + get_properties for every agent of every env.  handles: get_many(handles)
        with a strict subset (a permutation of 0 .. n-1, the same list for every env; fl_obs_cutils_handles): the tensors still
        hold every agent's rows, the trees computed against the predictions of the listed agents only."""
        o = self._obs_buffers()
        if handles is not None:
            hs = np.ascontiguousarray(handles, dtype=np.int32)
            _chk(_sym("fl_obs_cutils_handles")(self.h, self.max_nodes, self.pred_depth, _p(hs), len(hs), *self._cutils_ptrs(o)))
        else:
            _chk(lib().fl_obs_cutils(self.h, self.max_nodes, self.pred_depth, *self._cutils_ptrs(o)))
        return o

    def obs_both(self, max_depth=2, pred_depth=30):
        """obs_cutils() and obs_tree(max_depth, pred_depth) in one launch; returns (cutils dict, tree tensor)."""
        o = self._obs_buffers()
        out = self._tree_buffer(max_depth)
        _chk(lib().fl_obs_cutils_tree(self.h, self.max_nodes, self.pred_depth, *self._cutils_ptrs(o), max_depth, pred_depth, out.data_ptr()))
        return o, out

    def keep_tree_rows(self, on=True):
        """FL_OBS_KEEP_TREE_ROWS: the upstream-tree tensor this object hands out is its own buffer, the same from call to call -- as long
        as the caller does not write into it, the builder only updates the rows that change (no -inf pre-fill of the slab per call).
        HAZARD: obs_tree / obs_both / step_obs hand out that very tensor; an in-place op on it (replacing -inf before a network, say) breaks
        the promise silently -- clone it first.  FL_OBS_KEEP_VERIFY=1 (environment, diagnostic) checks the promise before every such launch
        and latches an error for check() when a constant row is no longer -inf or a real row is."""
        _chk(_sym("fl_obs_set_mode")(self.h, FL_OBS_KEEP_TREE_ROWS if on else 0))

    def policy_inputs(self, obs=None):
        """(agents_attr f32[B,A,83], forest f32[B,A,N,12], adjacency i64[B,A,N-1,3], node_order i64[B,A,N],
        edge_order i64[B,A,N-1]) on the device, exactly what Network.forward consumes after its own
        modify_adjacency (solution/nn/net_tree.py:72-116); adjacency is already modified."""
        t = self.torch
        o = obs if obs is not None else self.obs_cutils()
        B, A, E = o["adjacency"].shape[:3]
        if self._pol is None or self._pol[2].shape[-1] != E:
            self._pol = (t.empty((B, A, E, 3), dtype=t.int64, device=self.device),
                         t.empty((B, A, E + 1), dtype=t.int64, device=self.device),
                         t.empty((B, A, E), dtype=t.int64, device=self.device))
        adj, no, eo = self._pol
        policy_pack(o["adjacency"], o["node_order"], o["edge_order"], adj, no, eo)
        return o["agent_attr"], o["forest"], adj, no, eo

    def obs_policy(self):
        """The consumer's call: the flatland_cutils observation with the index tensors as Network.forward takes them, ONE launch
        (fl_obs_cutils_policy) -- (agents_attr f32[B,A,83], forest f32[B,A,N,12], adjacency i64[B,A,N-1,3] already modified,
        node_order i64[B,A,N], edge_order i64[B,A,N-1]); valid_actions / props land in the obs_cutils() buffers.  Equal to
        policy_inputs(obs_cutils()) element for element."""
        t = self.torch
        o = self._obs_buffers()
        B, A, N = self.B, self.A, self.max_nodes
        if self._pol64 is None or self._pol64[1].shape[-1] != N:       # (max_nodes may be set anew by a builder's set_env)
            self._pol64 = (t.empty((B, A, N - 1, 3), dtype=t.int64, device=self.device), t.empty((B, A, N), dtype=t.int64, device=self.device),
                           t.empty((B, A, N - 1), dtype=t.int64, device=self.device))
        adj, no, eo = self._pol64
        _chk(_sym("fl_obs_cutils_policy")(self.h, self.max_nodes, self.pred_depth, *self._cutils_ptrs(o, self._pol64)))
        return o["agent_attr"], o["forest"], adj, no, eo

    def obs_tree(self, max_depth=2, pred_depth=30, handles=None):
        """upstream TreeObsForRailEnv(max_depth, ShortestPathPredictorForRailEnv(pred_depth)) as a dense tensor.  handles: get_many(handles)
        with a list (a permutation of 0 .. n-1, the same for every env; fl_obs_tree_handles): every agent's rows, the trees computed against
        the predictions of the listed agents only, by list position (observations.py:72-83, 337-366)."""
        out = self._tree_buffer(max_depth)
        if handles is not None:
            hs = np.ascontiguousarray(handles, dtype=np.int32)
            _chk(_sym("fl_obs_tree_handles")(self.h, max_depth, pred_depth, _p(hs), len(hs), out.data_ptr()))
        else:
            _chk(lib().fl_obs_tree(self.h, max_depth, pred_depth, out.data_ptr()))
        return out

    def _env_range(self, envs):
        """None -> every env; a range / slice of consecutive envs or a (start, stop) pair -> (b0, nb)"""
        if envs is None:
            return 0, self.B
        if isinstance(envs, (range, slice)):
            start, stop, step = envs.indices(self.B) if isinstance(envs, slice) else (envs.start, envs.stop, envs.step)
            if step != 1:
                raise ValueError("obs_global: envs has to be a run of consecutive envs, got %r" % (envs,))
        else:
            start, stop = (int(v) for v in envs)
        return int(start), int(stop) - int(start)

    def obs_global(self, dtype=None, envs=None, rail=True):
        """flatland.envs.observations.GlobalObsForRailEnv (observations.py:535-611) for every agent of the envs `envs` (None = all; a
        range / slice of consecutive envs or a (start, stop) pair), one launch (fl_obs_global): (rail [nb,H,W,16] or None when
        rail=False, agents_state [nb,A,H,W,5], targets [nb,A,H,W,2]) device tensors.  dtype torch.float64 (default: the reference's
        values) or torch.float32 (the same values cast).  The buffers are cached per (dtype, range) and rewritten by every call: the
        output is A times the map per env (4.8 GB in float64 for 1 024 envs of 80 agents on 35 x 30), so take big batches in ranges."""
        t = self.torch
        dtype = t.float64 if dtype is None else dtype
        if dtype not in (t.float64, t.float32):
            raise ValueError("obs_global: dtype has to be torch.float64 or torch.float32, got %r" % (dtype,))
        b0, nb = self._env_range(envs)
        if not (0 <= b0 and nb >= 1 and b0 + nb <= self.B):
            raise ValueError("obs_global: env range [%d, %d) is not inside [0, %d)" % (b0, b0 + nb, self.B))
        key = (dtype, b0, nb)
        if key not in self._glob:
            H, W, A, dev = self.H, self.W, self.A, self.device
            self._glob[key] = (t.empty((nb, H, W, 16), dtype=dtype, device=dev), t.empty((nb, A, H, W, 5), dtype=dtype, device=dev),
                               t.empty((nb, A, H, W, 2), dtype=dtype, device=dev))
        r, ast, tgt = self._glob[key]
        _chk(lib().fl_obs_global(self.h, b0, nb, 8 if dtype == t.float64 else 4, r.data_ptr() if rail else None, ast.data_ptr(),
                                 tgt.data_ptr()))
        return (r if rail else None), ast, tgt

    def predictions(self, max_depth=20, dtype=None, envs=None, paths=False):
        """flatland.envs.predictions.ShortestPathPredictorForRailEnv(max_depth).get() (predictions.py:97-180) for every agent of the
        envs `envs` (the forms obs_global takes), one launch (fl_predict): pred [nb, A, max_depth + 1, 5] with the rows (time, row, col,
        direction, action), dtype torch.float64 (default: the reference's) or torch.int32 (the same values).  paths=True: (pred,
        waypoints [nb, A, max_depth, 3] int32, length [nb, A] int32) -- get_shortest_paths(distance_map, max_depth)
        (rail_env_shortest_paths.py:203-274) as (row, col, direction) with -1 behind the path's length, length 0 = None.  The buffers
        are cached per (max_depth, dtype, range) and rewritten by every call."""
        t = self.torch
        dtype = t.float64 if dtype is None else dtype
        if dtype not in (t.float64, t.int32):
            raise ValueError("predictions: dtype has to be torch.float64 or torch.int32, got %r" % (dtype,))
        max_depth = int(max_depth)
        if not 1 <= max_depth <= 500:
            raise ValueError("predictions: max_depth has to be in 1 .. 500, got %d" % max_depth)
        b0, nb = self._env_range(envs)
        if not (0 <= b0 and nb >= 1 and b0 + nb <= self.B):
            raise ValueError("predictions: env range [%d, %d) is not inside [0, %d)" % (b0, b0 + nb, self.B))
        key = (max_depth, dtype, b0, nb)
        if key not in self._pred:
            self._pred[key] = t.empty((nb, self.A, max_depth + 1, 5), dtype=dtype, device=self.device)
        pred = self._pred[key]
        wp = ln = None
        if paths:
            pkey = (max_depth, b0, nb)
            if pkey not in self._pred:
                self._pred[pkey] = (t.empty((nb, self.A, max_depth, 3), dtype=t.int32, device=self.device),
                                    t.empty((nb, self.A), dtype=t.int32, device=self.device))
            wp, ln = self._pred[pkey]
        _chk(_sym("fl_predict")(self.h, b0, nb, max_depth, 0 if dtype == t.float64 else 1, pred.data_ptr(),
                                wp.data_ptr() if paths else None, ln.data_ptr() if paths else None))
        return (pred, wp, ln) if paths else pred

    # ---- the reduced action space of flatland/contrib/wrappers/flatland_wrappers.py
    def _wrap_range(self, who, envs):
        b0, nb = self._env_range(envs)
        if not (0 <= b0 and nb >= 1 and b0 + nb <= self.B):
            raise ValueError("%s: env range [%d, %d) is not inside [0, %d)" % (who, b0, b0 + nb, self.B))
        return b0, nb

    def _wrap_buffer(self, key, shape, dtype):
        if key not in self._wrap:
            self._wrap[key] = self.torch.empty(shape, dtype=dtype, device=self.device)
        return self._wrap[key]

    def _reduced(self, who, reduced, nb):
        """a host array or a device tensor -> contiguous uint8 [nb, A] on the device"""
        t = self.torch
        if not (isinstance(reduced, t.Tensor) and reduced.is_cuda):
            a = np.asarray(reduced)
            if a.dtype.kind not in "iub" or a.shape != (nb, self.A) or (a.size and (a.min() < 0 or a.max() > 255)):
                raise ValueError("%s: reduced has to hold integers 0 .. 255 of shape (%d, %d), got %s %r" % (who, nb, self.A, a.dtype, a.shape))
            reduced = t.as_tensor(np.ascontiguousarray(a, dtype=np.uint8)).to(self.device)
        if reduced.dtype != t.uint8 or tuple(reduced.shape) != (nb, self.A):
            raise ValueError("%s: reduced has to be a uint8 tensor of shape (%d, %d), got %s %r" % (who, nb, self.A, reduced.dtype, tuple(reduced.shape)))
        if reduced.device != self.device:
            raise ValueError("%s: reduced lies on %s, the batch on %s" % (who, reduced.device, self.device))
        return reduced.contiguous()

    def shortest_path_actions(self, dtype=None, envs=None):
        """possible_actions_sorted_by_distance(env, handle) (flatland_wrappers.py:14-56) for every agent of the envs `envs` (the forms
        obs_global takes), one launch (fl_action_space): (actions u8 [nb, A, 3] RailEnvActions, distance [nb, A, 3], count u8 [nb, A]).
        dtype torch.float64 (default: the reference's values, inf = unreachable) or torch.int32 (INT32_MAX = unreachable); behind
        `count` the slots hold action 0 and infinity.  The buffers are cached per (dtype, range) and rewritten by every call."""
        t = self.torch
        dtype = t.float64 if dtype is None else dtype
        if dtype not in (t.float64, t.int32):
            raise ValueError("shortest_path_actions: dtype has to be torch.float64 or torch.int32, got %r" % (dtype,))
        b0, nb = self._wrap_range("shortest_path_actions", envs)
        act = self._wrap_buffer(("sp_action", b0, nb), (nb, self.A, 3), t.uint8)
        dist = self._wrap_buffer(("sp_dist", dtype, b0, nb), (nb, self.A, 3), dtype)
        cnt = self._wrap_buffer(("sp_count", b0, nb), (nb, self.A), t.uint8)
        _chk(_sym("fl_action_space")(self.h, b0, nb, 0 if dtype == t.float64 else 1, act.data_ptr(), dist.data_ptr(), cnt.data_ptr(),
                                     None, None, None))
        return act, dist, cnt

    def on_decision_cell(self, envs=None):
        """SkipNoChoiceCellsWrapper.on_decision_cell(agent) (flatland_wrappers.py:197-198) for every agent of the envs `envs`: u8 [nb, A],
        1 = off the map or DONE, on its own start cell, on a switch or next to one (fl_action_space)"""
        b0, nb = self._wrap_range("on_decision_cell", envs)
        dec = self._wrap_buffer(("on_decision", b0, nb), (nb, self.A), self.torch.uint8)
        _chk(_sym("fl_action_space")(self.h, b0, nb, 0, None, None, None, dec.data_ptr(), None, None))
        return dec

    def decision_cells(self, envs=None):
        """find_all_cells_where_agent_can_choose(env) (flatland_wrappers.py:145-176) of the envs `envs`: u8 [nb, H, W], bit 0 = switch,
        bit 1 = neighbour of a switch (fl_decision_cells; the table is built with the env's static tables)"""
        b0, nb = self._wrap_range("decision_cells", envs)
        cells = self._wrap_buffer(("cells", b0, nb), (nb, self.H, self.W), self.torch.uint8)
        _chk(_sym("fl_decision_cells")(self.h, b0, nb, cells.data_ptr()))
        return cells

    def reduced_actions(self, reduced, envs=None):
        """ShortestPathActionWrapper.step's translation (flatland_wrappers.py:131-138) for the envs `envs`: reduced u8 [nb, A] with
        0 = do nothing, 1 = shortest path, 2 = second shortest path (3 = third where a list has three), 255 = agent not in the dict
        -> u8 [nb, A] RailEnvActions, what step() takes.  An entry the agent's list does not have gives 0 (the reference raises
        IndexError)."""
        b0, nb = self._wrap_range("reduced_actions", envs)
        reduced = self._reduced("reduced_actions", reduced, nb)
        out = self._wrap_buffer(("actions", b0, nb), (nb, self.A), self.torch.uint8)
        _chk(_sym("fl_action_space")(self.h, b0, nb, 0, None, None, None, None, reduced.data_ptr(), out.data_ptr()))
        return out

    def step_shortest_path(self, reduced, auto_reset=False, filter_required=False):
        """step(reduced_actions(reduced), ...): the translation and the tick back to back on the batch's stream, nothing in between"""
        return self.step(self.reduced_actions(reduced), auto_reset, filter_required)

    # ---- read-backs
    def state(self):
        st = np.zeros((self.B, self.A, STATE_COLS), dtype=np.int32)
        el = np.zeros(self.B, dtype=np.int32)
        _chk(lib().fl_get_state(self.h, _p(st), _p(el)))
        return st, el

    def state_aux(self):
        """int32[B, A, 4]: previous_state (-1 = None), in_malfunction signal of the last step, deadlocked, done."""
        aux = np.zeros((self.B, self.A, AUX_COLS), dtype=np.int32)
        _chk(lib().fl_get_state_aux(self.h, _p(aux)))
        return aux

    def set_state(self, state, aux=None, elapsed=None, done_all=None):
        """inject the dynamic agent state (fl_set_state): state int32[B, A, 12] as state() returns it."""
        state = np.ascontiguousarray(state, dtype=np.int32)
        assert state.shape == (self.B, self.A, STATE_COLS)
        if aux is not None:
            aux = np.ascontiguousarray(aux, dtype=np.int32)
            assert aux.shape == (self.B, self.A, AUX_COLS)
        if elapsed is not None:
            elapsed = np.ascontiguousarray(elapsed, dtype=np.int32)
            assert elapsed.shape == (self.B,)
        if done_all is not None:
            done_all = np.ascontiguousarray(done_all, dtype=np.uint8)
            assert done_all.shape == (self.B,)
        _chk(lib().fl_set_state(self.h, _p(state), None if aux is None else _p(aux), None if elapsed is None else _p(elapsed),
                                None if done_all is None else _p(done_all)))

    def rng_state(self):
        key = np.zeros((self.B, 624), dtype=np.uint32)
        pos = np.zeros(self.B, dtype=np.int32)
        _chk(lib().fl_get_rng(self.h, _p(key), _p(pos)))
        return key, pos

    def set_rng_state(self, key, pos):
        key = np.ascontiguousarray(key, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        assert key.shape == (self.B, 624) and pos.shape == (self.B,)
        _chk(lib().fl_set_rng(self.h, _p(key), _p(pos)))

    def distance_map(self, b):
        n = C.c_int(0)
        slot = np.zeros(self.A, dtype=np.int32)
        _chk(lib().fl_distance_map(self.h, b, C.byref(n), None, _p(slot)))
        dm = np.zeros((n.value, self.H, self.W, 4), dtype=np.uint16)
        _chk(lib().fl_distance_map(self.h, b, C.byref(n), _p(dm), _p(slot)))
        return dm, slot

    def rebuild_distance_maps(self, mask=None):
        """DistanceMap.reset() + _compute() on the GPU (asynchronous on the handle's stream) for every env, or for the
        envs with a non-zero entry in `mask` (uint8 device tensor [B], e.g. the done_all tensor of the last step)."""
        if mask is None:
            _chk(lib().fl_distance_map_rebuild(self.h))
        else:
            assert mask.is_cuda and mask.dtype == self.torch.uint8 and mask.numel() == self.B and mask.is_contiguous()
            _chk(lib().fl_distance_map_rebuild_masked(self.h, mask.data_ptr()))

    def positions_map(self, b):
        out = np.zeros((self.H, self.W), dtype=np.int32)
        _chk(lib().fl_positions_map(self.h, b, _p(out)))
        return out

    def last_obs_class(self):
        """diagnostic: (fixed launch class, split, envs on the class's body) of the last obs_both / step_obs launch -- class 0 = the
        runtime-carving kernel; split 1 = the class served only the envs that fit it, the others ran the runtime-carving body"""
        out = (C.c_int * 3)()
        _chk(_sym("fl_debug_last_obs_class")(self.h, out))
        return tuple(out)

    LAUNCH_FIELDS = ("mode", "var", "fix", "split", "fix2", "nt", "lds", "wl_bytes", "tab", "nh", "tmask", "dual", "items", "items_cap", "snext",
                     "partial", "bk_room", "own_filter", "fb", "raw", "wl_head", "bk", "tshift", "compact_t", "label")

    def last_obs_launch(self):
        """diagnostic: what the last observation launch of this handle ran, through any of obs_cutils / obs_policy / obs_both / obs_tree / step_obs
        -- a dict of LAUNCH_FIELDS: the kernel (k_obs<mode, var> of launch class `fix`, 0 = the runtime carving; split 1 / 2 = the class's split
        kernel, fix2 the second class of a split-2 kernel), threads and dynamic LDS bytes of the launch, the ObsOptions the launcher's preference
        walk accepted (wl_bytes .. wl_head) and what it derived from them (bk, tshift, compact_t; label = a handle subset).  mode -1: no launch yet."""
        out = (C.c_int * len(self.LAUNCH_FIELDS))()
        _chk(_sym("fl_debug_last_obs_launch")(self.h, out, len(out)))
        return dict(zip(self.LAUNCH_FIELDS, out))

    def algorithmic_bytes_per_agent_step(self, with_cutils_obs=True, tree_depth=0):
        return float(lib().fl_algorithmic_bytes_per_agent_step(self.h, int(with_cutils_obs), int(tree_depth)))


class MixedBatch:
    """Envs of DIFFERENT shapes stepped together: the reference's evaluator runs tests of different map sizes and agent counts
    back to back (solution/debug-environments/parameters_flatland_round_2_new.csv: 30x30 / 7 agents ... 158x158 / 425 agents).
    A C-ABI handle holds envs of one (A, H, W); this groups any list of env descriptions by shape into one handle per shape,
    each on a HIP stream of its own (kernels of different shapes overlap on the GPU), and keeps the caller's env order.

    env i lives in group `self.where[i][0]` at batch index `self.where[i][1]`; the per-group tensors are what BatchedRailEnv
    returns, `pick(i, tensors)` gives env i's slice of a per-group result list."""

    def __init__(self, envs, device=0, max_nodes=31, pred_depth=500):
        import torch
        self.torch = torch
        shapes, self.where = {}, []
        for e in envs:
            H, W = np.asarray(e["grid"]).shape
            key = (int(len(e["init_dir"])), int(H), int(W))
            g = shapes.setdefault(key, [])
            self.where.append((key, len(g)))
            g.append(e)
        self.keys = list(shapes)
        self.where = [(self.keys.index(k), b) for k, b in self.where]
        self.streams, self.groups = [], []
        for k in self.keys:
            s = torch.cuda.Stream(device=torch.device("cuda", device))
            with torch.cuda.stream(s):
                self.groups.append(BatchedRailEnv(shapes[k], device=device, max_nodes=max_nodes, pred_depth=pred_depth))
            self.streams.append(s)
        self.n = len(envs)

    def _on_streams(self, fn):
        """fn(k, group) enqueued on every group's own stream (the groups' kernels overlap); the CALLER's current stream then waits for
        all of them, so whatever the caller does next with the returned tensors -- a .cpu(), a torch op, its own kernels -- is ordered
        after the groups' work (the groups' streams are non-blocking: nothing orders them with the caller's stream otherwise)"""
        t = self.torch
        cur = t.cuda.current_stream(self.groups[0].device)
        out = []
        for k, (g, s) in enumerate(zip(self.groups, self.streams)):
            s.wait_stream(cur)                   # ... and the group's work after what the caller enqueued before (e.g. the actions' upload)
            with t.cuda.stream(s):
                out.append(fn(k, g))
        for s in self.streams:
            cur.wait_stream(s)
        return out

    def _each(self, fn):
        return self._on_streams(lambda k, g: fn(g))

    def pick(self, i, per_group):
        g, b = self.where[i]
        r = per_group[g]
        if isinstance(r, dict):
            return {k: v[b] for k, v in r.items()}
        if isinstance(r, tuple):
            return tuple(self.pick_one(x, b) for x in r)
        return r[b]

    @staticmethod
    def pick_one(x, b):
        return {k: v[b] for k, v in x.items()} if isinstance(x, dict) else (None if x is None else x[b])

    def step(self, actions, auto_reset=False, filter_required=False):
        """actions: one uint8 array [A_i] per env (255 = agent not in the dict), in the caller's env order"""
        per = [np.full((g.B, g.A), ACTION_ABSENT, dtype=np.uint8) for g in self.groups]
        for i, a in enumerate(actions):
            g, b = self.where[i]
            per[g][b] = np.asarray(a, dtype=np.uint8)
        return self._on_streams(lambda k, g: g.step(per[k], auto_reset=auto_reset, filter_required=filter_required))

    def _per_group(self, rows):
        per = [np.full((g.B, g.A), ACTION_ABSENT, dtype=np.uint8) for g in self.groups]
        for i, a in enumerate(rows):
            g, b = self.where[i]
            per[g][b] = np.asarray(a, dtype=np.uint8)
        return per

    def reduced_actions(self, reduced):
        """reduced: one uint8 array [A_i] per env in the caller's env order -> BatchedRailEnv.reduced_actions per shape group"""
        per = self._per_group(reduced)
        return self._on_streams(lambda k, g: g.reduced_actions(per[k]))

    def step_shortest_path(self, reduced, auto_reset=False, filter_required=False):
        """reduced as reduced_actions takes it; per group the translation and the tick on the group's stream"""
        per = self._per_group(reduced)
        return self._on_streams(lambda k, g: g.step_shortest_path(per[k], auto_reset=auto_reset, filter_required=filter_required))

    def stream_of(self, i):
        """stream id of env i in the on-device action stream of step_synth (groups in order, envs of a group consecutive)"""
        g, b = self.where[i]
        return sum(x.B for x in self.groups[:g]) + b

    def step_synth(self, seed, kind=0, auto_reset=True):
        """the on-device action stream; env i uses stream id stream_of(i)"""
        base = [sum(x.B for x in self.groups[:k]) for k in range(len(self.groups))]
        return self._on_streams(lambda k, g: g.step_synth(seed, base[k], kind, auto_reset=auto_reset))

    def obs_cutils(self):
        return self._each(lambda g: g.obs_cutils())

    def obs_both(self, max_depth=2, pred_depth=30):
        return self._each(lambda g: g.obs_both(max_depth, pred_depth))

    def obs_policy(self):
        """the consumer's call per group (fl_obs_cutils_policy): the adjacency of group k is offset over ITS (env, agent) flattening"""
        return self._each(lambda g: g.obs_policy())

    def obs_global(self, dtype=None, rail=True):
        """GlobalObsForRailEnv per group (fl_obs_global): one (rail, agents_state, targets) triple per shape group, its env axis in the
        group's batch order (pick(i, ...) gives env i's slices)"""
        return self._each(lambda g: g.obs_global(dtype, None, rail))

    def predictions(self, max_depth=20, dtype=None, paths=False):
        """ShortestPathPredictorForRailEnv(max_depth).get() per group (fl_predict): one result of BatchedRailEnv.predictions per shape
        group, its env axis in the group's batch order (pick(i, ...) gives env i's slices)"""
        return self._each(lambda g: g.predictions(max_depth, dtype, None, paths))

    def shortest_path_actions(self, dtype=None):
        """possible_actions_sorted_by_distance per group (fl_action_space): one result of BatchedRailEnv.shortest_path_actions per shape
        group, its env axis in the group's batch order (pick(i, ...) gives env i's slices)"""
        return self._each(lambda g: g.shortest_path_actions(dtype))

    def on_decision_cell(self):
        """SkipNoChoiceCellsWrapper.on_decision_cell per group"""
        return self._each(lambda g: g.on_decision_cell())

    def decision_cells(self):
        """find_all_cells_where_agent_can_choose per group (fl_decision_cells)"""
        return self._each(lambda g: g.decision_cells())

    def state(self, i):
        g, b = self.where[i]
        st, el = self.groups[g].state()
        return st[b], int(el[b])

    def metrics(self):
        """int64[4] on the host: the sums over all groups (what a multi-GPU harness all-reduces)"""
        return sum(m.cpu().numpy() for m in self._each(lambda g: g.metrics()))

    def check(self):
        for g in self.groups:
            g.check()

    def sync(self):
        for g in self.groups:
            g.sync()

    def close(self):
        for g in self.groups:
            g.close()
