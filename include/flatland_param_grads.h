/* flatland_param_grads.h -- the parameter gradients of the policy network on the GPU: the last step of training, the sums over
 * the rows that fl_policy_head_backward (include/flatland_policy_train.h) and fl_tree_lstm_backward (include/flatland_train.h)
 * leave.  Exported by libflatland_hip.so next to those headers (whose layouts these read, unchanged) and include/flatland_hip.h
 * (error codes, fl_last_error).
 *
 *   fl_policy_head_param_grads   the 38 gradients of the head's parameters from attr, the saved forward and the backward's rows
 *   fl_tree_lstm_param_grads     the 8 gradients of the tree encoder's parameters from x, node_order, h and the backward's rows
 *
 * Stateless: device pointers, everything enqueued on hip_stream (one launch; two with more than one slice), no host
 * synchronisation, no allocation.  Float32 inputs and outputs.  Each call OVERWRITES its outputs, it does not accumulate.
 *
 * ---- what is computed.  A weight's gradient is dW[p][q] = sum over the rows r of dZ[r][p] X[r][q], a bias's db[p] = sum_r dZ[r][p];
 * outputs have torch's own parameter shapes, [out][in].
 *
 * The head (R = n_envs * n_agents rows; grads[i] in the order of the 38 parameters of include/flatland_policy.h; dZ and X are the
 * arrays of rows_dev and saved_dev named in include/flatland_policy_train.h, which also lists these formulas):
 *     attr_embedding  .0: dZ = its dZ of layer 0, X = attr [R][83]    .2: layer 2, h1    .4: layer 4, h2    .6: layer 6, h3
 *     transformer.i   in_proj: dZ = dqkv_i, X = y_i (saved; y_0 = emb)    out_proj: dZ = do_i, X = c_i (saved)
 *                     att_mlp.0: dZ = dz_i, X = [y_i | o_i]
 *     actor_net / critic_net   .0: dZ = its dZ of layer 0, X = [emb | y_3] (saved)    .2: layer 2, u1
 *                     .4: the first 5 / 1 columns of its dZ of layer 4 (8 / 4 floats a row), X = u2
 * every weight followed by its bias, db = sum dZ of the same dZ.
 * actor = 0: the actor's six gradients (grads[26 .. 31]) are not written and may be NULL, its five arrays of rows_dev are not
 * read (fl_policy_head_backward with grad_logits NULL does not write them); critic = 0: the same for grads[32 .. 37].
 *
 * The encoder (n_rows = n_trees * n_nodes nodes; grads[i] in the order W_iou.weight, W_iou.bias, U_iou.weight, W_c.weight,
 * W_c.bias, W_f.weight, W_f.bias, U_f.weight; x_dev = the forest f32[n_rows][12], node_order_dev i64[n_rows], h_dev
 * f32[n_rows][128] of the forward, da, dc, dg, q, child as fl_tree_lstm_backward wrote them for the same nodes, child ids counting
 * from this call's first node):
 *     x' = x where node_order >= 0, else zero (a padding node's features never enter a sum, whatever they hold)
 *     hk_j = h[child[r][j]], zero where child[r][j] is outside [0, n_rows)
 *     dgs = (dg_1 + dg_2) + dg_3, added in float32 per node
 *     dW_iou = sum da x'^T   db_iou = sum da   dU_iou = sum da [hk_1 | hk_2 | hk_3]^T   dW_c = sum dc q^T
 *     db_c = sum dc over the nodes with node_order >= 1     dW_f = sum dgs x'^T   db_f = sum dgs
 *     dU_f = sum over the 3 n_rows pairs (r, j), in that order, of dg_j hk_j^T
 *
 * ---- summation order (the one policy._tn documents).  The rows of a sum go in blocks of 256.  A block's product is accumulated in
 * float32 by the matrix instruction (v_mfma_f32_32x32x2_f32: exact float32 products, rows taken two at a time in increasing
 * order); the blocks' results are added in float64 in block order; the last block is ragged.  A bias is the float64 sum of dZ: a
 * block's rows in row order, the blocks in block order.  The row range is cut into `slices` slices of ceil(blocks / slices) whole
 * blocks each (slices behind the last block are empty and contribute zero).  With one slice the float64 sums are rounded to
 * float32 and written.  With more, each slice writes its float64 sums to the workspace and a second launch adds the slices in
 * slice order, then rounds.
 *
 * Deterministic: no float atomics, every address has one writer per launch.  Two calls on the same inputs WITH THE SAME SLICE
 * COUNT give the same bits.  Different slice counts group the float64 additions differently: their results agree to rounding,
 * equal bits are not promised.
 *
 * ---- slices and workspace.  slices = 0: the library chooses from the row count, min(blocks, 2) for the head and min(blocks, 15)
 * for the encoder (the launch then has at most one workgroup per compute unit of an MI355X, which is what the kernel's registers
 * allow: 106 resp. 17 output tiles of 128 x 128 times the slices).  slices in [1, FL_PARAM_GRADS_MAX_SLICES] forces that count.  The workspace holds the float64
 * partials: nothing for one slice, else slices * 1 698 694 * 8 B for the head (13.6 MB a slice) and slices * 219 776 * 8 B for the
 * encoder (1.76 MB a slice); the two _workspace_bytes functions return that, with the count they would choose for slices = 0, and
 * 0 for n_rows <= 0 or slices outside [0, FL_PARAM_GRADS_MAX_SLICES].  workspace_dev may be NULL where they return 0.
 *
 * FL_ERR_ARG before any HIP call, nothing written: n_envs <= 0, n_agents outside [1, 1024], n_rows <= 0 or above 2^31 / 384,
 * slices outside [0, FL_PARAM_GRADS_MAX_SLICES], actor or critic outside {0, 1}, both zero, a NULL input, grads NULL, a NULL
 * gradient that is not switched off, a NULL workspace where bytes are needed, a short workspace, a float or workspace pointer not
 * 16-byte aligned, node_order not 8-byte aligned, child not 4-byte aligned.
 */
#ifndef FLATLAND_PARAM_GRADS_H
#define FLATLAND_PARAM_GRADS_H
#include "flatland_policy_train.h"
#include "flatland_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FL_PARAM_GRADS_MAX_SLICES 32
#define FL_PARAM_GRADS_BLOCK 256 /* rows a float32 partial product */

size_t fl_policy_head_param_grads_workspace_bytes(int n_rows, int slices);
int fl_policy_head_param_grads(int n_envs, int n_agents, const float *attr_dev, const void *saved_dev, const void *rows_dev,
                               int actor, int critic, float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes,
                               void *hip_stream);
size_t fl_tree_lstm_param_grads_workspace_bytes(int n_rows, int slices);
int fl_tree_lstm_param_grads(int n_rows, const float *x_dev, const int64_t *node_order_dev, const float *h_dev, const float *da_dev,
                             const float *dc_dev, const float *dg_dev, const float *q_dev, const int32_t *child_dev,
                             float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
