// fl_tree_lstm.hip -- entry points of the policy's tree encoder: fl_tree_lstm (include/flatland_hip.h), its gradient
// fl_tree_lstm_backward (include/flatland_train.h) and the inference forward with bf16 matrix operands, fl_tree_lstm_bf16 with
// fl_tree_lstm_pack_bf16 (include/flatland_policy_bf16.h).  The checks (all before any HIP call) and the launches of the kernels in
// fl_tree_lstm.h, fl_tree_lstm_bwd.h and fl_tree_lstm_bf16.h.  No env handle: plain pointers and sizes.
#include <algorithm>

#include "../../include/flatland_hip.h"
#include "../../include/flatland_policy_bf16.h"
#include "../../include/flatland_train.h"
#include "fl_tree_lstm.h"
#include "fl_tree_lstm_bwd.h"
#include "fl_tree_lstm_bf16.h"
#include "fl_policy_host.h"

// sizes, then the pointers' NULLs and alignment in the table's order, then the workspace; `fn` names the caller in the message
static int ftl_check(const char *fn, int n_trees, int n_nodes, int roots_only, const FlPtr *tab, int n, size_t workspace_bytes,
                     size_t need) {
    if (n_trees <= 0 || n_nodes < 4 || n_nodes > FTL_MAX_N || n_trees > (INT32_MAX / FTL_MAX_N)) {
        fl_set_error("%s: bad sizes (n_trees %d, n_nodes %d; 1 <= n_trees, 4 <= n_nodes <= %d)", fn, n_trees, n_nodes, FTL_MAX_N);
        return FL_ERR_ARG;
    }
    if ((n_nodes - 1) % 3 != 0) {
        fl_set_error("%s: n_nodes %d: (n_nodes - 1) %% 3 != 0, the reference pairs every level's nodes with edge triples", fn, n_nodes);
        return FL_ERR_ARG;
    }
    if (roots_only != 0 && roots_only != 1) { fl_set_error("%s: roots_only must be 0 or 1", fn); return FL_ERR_ARG; }
    if (fl_check_ptrs(fn, tab, n) != FL_OK) return FL_ERR_ARG;
    char sizer[64];
    snprintf(sizer, sizeof sizer, "%s_workspace_bytes", fn);
    return fl_check_bytes(fn, "workspace", workspace_bytes, need, sizer);
}

static int ftl16_check_packed(const char *fn, size_t packed_bytes) {
    return fl_check_bytes(fn, "packed buffer", packed_bytes, fl_tree_lstm_bf16_packed_bytes(), "fl_tree_lstm_bf16_packed_bytes");
}

// the members both kernels take; G from the current device's CU count (looked up once a device)
static int ftl_trees(const char *fn, FtlTrees &a, int n_trees, int n_nodes, int roots_only, const float *forest,
                     const int64_t *adjacency, const int64_t *node_order, const int64_t *edge_order, const float *const (&w)[8],
                     int32_t *status) {
    static int n_cu[64];
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { fl_set_error("%s: hipGetDevice failed: %s", fn, hipGetErrorString(e)); return FL_ERR_HIP; }
    if (dev >= 0 && dev < 64 && n_cu[dev] == 0 &&
        hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cu[dev] = 0;
    a.T = n_trees; a.N = n_nodes; a.roots_only = roots_only;
    a.G = ftl_group(n_trees, dev >= 0 && dev < 64 ? n_cu[dev] : 0);
    a.forest = forest;
    a.adj = (const long long *)adjacency; a.no = (const long long *)node_order; a.eo = (const long long *)edge_order;
    a.w_iou = w[0]; a.b_iou = w[1]; a.u_iou = w[2]; a.w_c = w[3]; a.b_c = w[4]; a.w_f = w[5]; a.b_f = w[6]; a.u_f = w[7];
    a.status = (int *)status;
    return FL_OK;
}

// the outputs, and where a forward keeps every node's h and c: in the outputs themselves, or (roots_only, or no c) in the workspace
static void ftl_planes(FtlArgs &a, float *h_dev, float *c_dev, void *workspace_dev) {
    a.h_out = h_dev; a.c_out = c_dev;
    float *ws = (float *)workspace_dev;
    if (a.roots_only) { a.hbuf = ws; a.cbuf = ws + (size_t)a.T * a.N * FTL_M; }
    else { a.hbuf = h_dev; a.cbuf = c_dev ? c_dev : ws; }
}

size_t fl_tree_lstm_workspace_bytes(int n_trees, int n_nodes, int roots_only) {
    if (n_trees <= 0 || n_nodes <= 0) return 0;
    return (size_t)n_trees * n_nodes * FTL_M * sizeof(float) * (roots_only ? 2 : 1);
}

int fl_tree_lstm(int n_trees, int n_nodes, const float *forest_dev, const int64_t *adjacency_dev, const int64_t *node_order_dev,
                 const int64_t *edge_order_dev, const float *w_iou_dev, const float *b_iou_dev, const float *u_iou_dev,
                 const float *w_c_dev, const float *b_c_dev, const float *w_f_dev, const float *b_f_dev, const float *u_f_dev,
                 int roots_only, float *h_dev, float *c_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                 void *hip_stream) {
    const char *fn = "fl_tree_lstm";
    const FlPtr tab[] = {{forest_dev, "forest", 16}, {w_iou_dev, "w_iou", 16}, {b_iou_dev, "b_iou", 16}, {u_iou_dev, "u_iou", 16},
                          {w_c_dev, "w_c", 16}, {b_c_dev, "b_c", 16}, {w_f_dev, "w_f", 16}, {b_f_dev, "b_f", 16}, {u_f_dev, "u_f", 16},
                          {h_dev, "h", 16}, {workspace_dev, "workspace", 16},
                          {adjacency_dev, "adjacency", 8}, {node_order_dev, "node_order", 8}, {edge_order_dev, "edge_order", 8},
                          {c_dev, "c", 16, true}, {status_dev, "status", 4, true}};
    if (ftl_check(fn, n_trees, n_nodes, roots_only, tab, sizeof tab / sizeof tab[0], workspace_bytes,
                  fl_tree_lstm_workspace_bytes(n_trees, n_nodes, roots_only)) != FL_OK) return FL_ERR_ARG;
    FtlArgs a;
    const int rc = ftl_trees(fn, a, n_trees, n_nodes, roots_only, forest_dev, adjacency_dev, node_order_dev, edge_order_dev,
                             {w_iou_dev, b_iou_dev, u_iou_dev, w_c_dev, b_c_dev, w_f_dev, b_f_dev, u_f_dev}, status_dev);
    if (rc != FL_OK) return rc;
    ftl_planes(a, h_dev, c_dev, workspace_dev);
    fl_launch_tree_lstm(a, (hipStream_t)hip_stream);
    return fl_launched(fn);
}

size_t fl_tree_lstm_backward_workspace_bytes(int n_trees, int n_nodes) {
    if (n_trees <= 0 || n_nodes <= 0) return 0;
    return (size_t)n_trees * n_nodes * 6 * FTL_M * sizeof(float);
}

int fl_tree_lstm_backward(int n_trees, int n_nodes, const float *forest_dev, const int64_t *adjacency_dev,
                          const int64_t *node_order_dev, const int64_t *edge_order_dev, const float *w_iou_dev,
                          const float *b_iou_dev, const float *u_iou_dev, const float *w_c_dev, const float *b_c_dev,
                          const float *w_f_dev, const float *b_f_dev, const float *u_f_dev, const float *h_dev, const float *c_dev,
                          const float *grad_h_dev, int roots_only, float *da_dev, float *dc_dev, float *dg_dev, float *q_dev,
                          int32_t *child_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_tree_lstm_backward";
    const FlPtr tab[] = {{forest_dev, "forest", 16}, {w_iou_dev, "w_iou", 16}, {b_iou_dev, "b_iou", 16}, {u_iou_dev, "u_iou", 16},
                          {w_c_dev, "w_c", 16}, {b_c_dev, "b_c", 16}, {w_f_dev, "w_f", 16}, {b_f_dev, "b_f", 16}, {u_f_dev, "u_f", 16},
                          {h_dev, "h", 16}, {c_dev, "c", 16}, {grad_h_dev, "grad_h", 16}, {da_dev, "da", 16}, {dc_dev, "dc", 16},
                          {dg_dev, "dg", 16}, {q_dev, "q", 16}, {workspace_dev, "workspace", 16},
                          {adjacency_dev, "adjacency", 8}, {node_order_dev, "node_order", 8}, {edge_order_dev, "edge_order", 8},
                          {child_dev, "child", 4}, {status_dev, "status", 4, true}};
    if (ftl_check(fn, n_trees, n_nodes, roots_only, tab, sizeof tab / sizeof tab[0], workspace_bytes,
                  fl_tree_lstm_backward_workspace_bytes(n_trees, n_nodes)) != FL_OK) return FL_ERR_ARG;
    FtbArgs a;
    const int rc = ftl_trees(fn, a, n_trees, n_nodes, roots_only, forest_dev, adjacency_dev, node_order_dev, edge_order_dev,
                             {w_iou_dev, b_iou_dev, u_iou_dev, w_c_dev, b_c_dev, w_f_dev, b_f_dev, u_f_dev}, status_dev);
    if (rc != FL_OK) return rc;
    a.h = h_dev; a.c = c_dev; a.grad_h = grad_h_dev;
    a.da = da_dev; a.dc = dc_dev; a.dg = dg_dev; a.q = q_dev; a.child = (int *)child_dev;
    a.ghc = (float *)workspace_dev;
    a.gcc = a.ghc + (size_t)n_trees * n_nodes * 3 * FTL_M;
    fl_launch_tree_lstm_bwd(a, (hipStream_t)hip_stream);
    return fl_launched(fn);
}

size_t fl_tree_lstm_bf16_packed_bytes(void) { return (size_t)FTL16_PACKED * sizeof(__bf16); }

int fl_tree_lstm_pack_bf16(const float *u_iou_dev, const float *w_c_dev, const float *u_f_dev, void *packed_dev, size_t packed_bytes,
                           void *hip_stream) {
    const char *fn = "fl_tree_lstm_pack_bf16";
    const FlPtr tab[] = {{u_iou_dev, "u_iou", 16}, {w_c_dev, "w_c", 16}, {u_f_dev, "u_f", 16}, {packed_dev, "packed", 16}};
    if (fl_check_ptrs(fn, tab, 4) != FL_OK || ftl16_check_packed(fn, packed_bytes) != FL_OK) return FL_ERR_ARG;
    fl_launch_tree_lstm_pack_bf16(u_iou_dev, w_c_dev, u_f_dev, packed_dev, (hipStream_t)hip_stream);
    return fl_launched(fn);
}

size_t fl_tree_lstm_bf16_workspace_bytes(int n_trees, int n_nodes, int roots_only) {
    return fl_tree_lstm_workspace_bytes(n_trees, n_nodes, roots_only);
}

int fl_tree_lstm_bf16(int n_trees, int n_nodes, const float *forest_dev, const int64_t *adjacency_dev, const int64_t *node_order_dev,
                      const int64_t *edge_order_dev, const float *w_iou_dev, const float *b_iou_dev, const float *b_c_dev,
                      const float *w_f_dev, const float *b_f_dev, const void *packed_dev, size_t packed_bytes, int roots_only,
                      float *h_dev, float *c_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_tree_lstm_bf16";
    const FlPtr tab[] = {{forest_dev, "forest", 16}, {w_iou_dev, "w_iou", 16}, {b_iou_dev, "b_iou", 16}, {b_c_dev, "b_c", 16},
                          {w_f_dev, "w_f", 16}, {b_f_dev, "b_f", 16}, {packed_dev, "packed", 16},
                          {h_dev, "h", 16}, {workspace_dev, "workspace", 16},
                          {adjacency_dev, "adjacency", 8}, {node_order_dev, "node_order", 8}, {edge_order_dev, "edge_order", 8},
                          {c_dev, "c", 16, true}, {status_dev, "status", 4, true}};
    if (ftl_check(fn, n_trees, n_nodes, roots_only, tab, sizeof tab / sizeof tab[0], workspace_bytes,
                  fl_tree_lstm_bf16_workspace_bytes(n_trees, n_nodes, roots_only)) != FL_OK ||
        ftl16_check_packed(fn, packed_bytes) != FL_OK) return FL_ERR_ARG;
    Ftl16Args a;
    const int rc = ftl_trees(fn, a, n_trees, n_nodes, roots_only, forest_dev, adjacency_dev, node_order_dev, edge_order_dev,
                             {w_iou_dev, b_iou_dev, nullptr, nullptr, b_c_dev, w_f_dev, b_f_dev, nullptr}, status_dev);
    if (rc != FL_OK) return rc;
    a.packed = (const __bf16 *)packed_dev;
    ftl_planes(a, h_dev, c_dev, workspace_dev);
    fl_launch_tree_lstm_bf16(a, (hipStream_t)hip_stream);
    return fl_launched(fn);
}
