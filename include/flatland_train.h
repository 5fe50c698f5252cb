/* flatland_train.h -- training the policy's tree encoder on the GPU: the gradient of fl_tree_lstm.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose error codes and fl_last_error these use).
 *
 *   fl_tree_lstm_backward   what autograd computes through TreeLSTM.forward (solution/nn/TreeLSTM.py:33-154: forward's level
 *                           loop 33-56, _run_lstm's gathers, gates and index writes 58-154), the part that follows the tree order
 *
 * Sizes and inputs are fl_tree_lstm's (include/flatland_hip.h): in-features 12, hidden size 128, forest f32[T][N][12],
 * adjacency i64[T][N-1][3] already modified, node_order i64[T][N], edge_order i64[T][N-1], the eight weights in torch's own
 * layout, read as they are at every call.  Float32 end to end.
 *
 * Stateless: device pointers, one kernel launch enqueued on hip_stream, no host synchronisation, no allocation.
 *
 *   h_dev, c_dev   f32[T*N][128]  h and c of every node, as fl_tree_lstm returns them with roots_only = 0 and c_dev given.  The
 *                  gates are recomputed from them (in the forward's own order of operations), not stored by the forward.
 *   grad_h_dev     the gradient on h: f32[T*N][128], or with roots_only = 1 f32[T][128] for node 0 of every tree.  What is given
 *                  for a padding node is ignored.
 *
 * With i, o, u, f_j, the children k1..k3 and q = [f_1*c_k1 | f_2*c_k2 | f_3*c_k3] as in the forward, t = tanh(c), and Gh / Gc the
 * gradient on a node's h / c (the caller's plus what its parents hand down), per node:
 *   dc = Gc + Gh*o*(1 - t^2)     da = [dc*u*i*(1 - i) | Gh*t*o*(1 - o) | dc*i*(1 - u^2)]      (the gradient on W_iou x + b_iou + U_iou h)
 *   height > 0:  dq = W_c^T dc,  dg_j = dq_j*c_kj*f_j*(1 - f_j),  child kj: Gc += dq_j*f_j,  Gh += (U_iou^T da)[block j] + U_f^T dg_j
 * A child that read as zero in the forward (a height not below its parent's, a padding child, the parent itself) receives
 * nothing and counts as h = c = 0; a child named by several edges receives the sum.  The forest gets no gradient.
 *
 * Outputs, per node (rows of padding nodes are zero, ids -1; dg, q and ids of height-0 nodes as well):
 *   da_dev f32[T*N][384]   dc_dev f32[T*N][128]   dg_dev f32[T*N][3][128]   q_dev f32[T*N][384]
 *   child_dev i32[T*N][3]  the global node ids of k1..k3, -1 = read as zero
 * The eight parameter gradients are sums over the nodes of products of these rows (x = the node's features, hk = [h_k1|h_k2|h_k3]):
 *   dW_iou = sum da x^T   db_iou = sum da   dU_iou = sum da hk^T   dW_c = sum dc q^T   db_c = sum dc (height > 0 only)
 *   dW_f = sum (dg_1+dg_2+dg_3) x^T   db_f = sum (dg_1+dg_2+dg_3)   dU_f = sum_j sum dg_j h_kj^T
 * and are left to the caller (batch-wide matrix products); this call writes none of them.  fl_tree_lstm_param_grads of
 * include/flatland_param_grads.h forms them from these very rows.
 *
 * Deterministic: no float atomics, every address has one writer, a node adds its parents' hand-downs in increasing (parent id,
 * slot).  Two calls on the same inputs give the same bits.
 *
 * Trees are checked as fl_tree_lstm checks them: a violating tree adds 1 to *status_dev (if not NULL; the caller zeroes it) and
 * gets unspecified rows, but nothing is written outside its own rows.
 * workspace_dev: at least fl_tree_lstm_backward_workspace_bytes(n_trees, n_nodes) bytes (T*N*3072 B: the hand-downs of Gh and Gc
 * per child slot), 16-byte aligned.  With the outputs that is 8 204 B a node: run big batches in chunks of trees.
 *
 * FL_ERR_ARG before any HIP call: n_trees <= 0, n_nodes outside [4, 64], (n_nodes - 1) % 3 != 0, roots_only outside {0, 1}, a
 * NULL input / weight / h / c / grad_h / output / workspace, a float pointer not 16-byte aligned, an int64 pointer not 8-byte
 * aligned, child or status not 4-byte aligned, a short workspace.
 */
#ifndef FLATLAND_TRAIN_H
#define FLATLAND_TRAIN_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fl_tree_lstm_backward_workspace_bytes(int n_trees, int n_nodes);
int fl_tree_lstm_backward(int n_trees, int n_nodes, const float *forest_dev, const int64_t *adjacency_dev,
                          const int64_t *node_order_dev, const int64_t *edge_order_dev, const float *w_iou_dev,
                          const float *b_iou_dev, const float *u_iou_dev, const float *w_c_dev, const float *b_c_dev,
                          const float *w_f_dev, const float *b_f_dev, const float *u_f_dev, const float *h_dev, const float *c_dev,
                          const float *grad_h_dev, int roots_only, float *da_dev, float *dc_dev, float *dg_dev, float *q_dev,
                          int32_t *child_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
