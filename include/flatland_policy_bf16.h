/* flatland_policy_bf16.h -- the policy's tree encoder for inference with bf16 matrix operands.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose error codes and fl_last_error this uses; a header of its own,
 * as flatland_policy.h, flatland_train.h and flatland_predict.h are, so that flatland_hip.h stays the list it was).
 *
 * fl_tree_lstm_bf16 is fl_tree_lstm (flatland_hip.h) with the three recurrent products -- U_iou [h_k1|h_k2|h_k3], U_f h_kj and
 * W_c [f_1*c_k1|f_2*c_k2|f_3*c_k3] -- on v_mfma_f32_32x32x16_bf16: their weights and their activations (h_k, f_j*c_kj) are rounded
 * to bf16, round to nearest even, the sums are float32.  W_iou x, W_f x, the biases, sigmoid / tanh and the h / c every level hands
 * to the next stay float32, so a node of height 0 sees no bf16 operand.  The same trees are accepted and the status word counts the
 * same trees; h and c are float32, padding nodes exactly 0, one writer per address, the same bits from run to run.  Inference only:
 * fl_tree_lstm_backward (flatland_train.h) recomputes float32 gates and belongs to fl_tree_lstm.
 *
 * fl_tree_lstm_bf16_packed_bytes(): the size of the packed weights, 425 984 bytes.
 * fl_tree_lstm_pack_bf16: rounds u_iou f32 [384][384], w_c f32 [128][384] and u_f f32 [128][128] (torch's [out][in] layout, on the
 *   device, 16-byte aligned) into packed_dev (16-byte aligned, packed_bytes >= fl_tree_lstm_bf16_packed_bytes()), one launch on
 *   hip_stream, no host synchronisation.  Layout: bf16 (the upper 16 bits of the rounded float32), the three matrices one after
 *   another -- U_iou at element 0, W_c at element 147 456, U_f at element 196 608 -- each in the order the kernel's wavefronts
 *   read it: a matrix W [R][K] as R / 32 blocks of 32 rows, a block as its K / 16 steps of the matrix instruction, a step as the 64
 *   lanes' operands of 8 elements, so that element 512 (b K / 16 + s) + 8 l + j of a matrix is W[32 b + (l & 31)][16 s + 8 (l >> 5) + j]
 *   (b < R / 32, s < K / 16, l < 64, j < 8).  Rounding is to nearest even as the hardware conversion does it: +-0, +-inf and
 *   subnormals keep their class, NaN stays NaN.  Call it again after the weights changed.
 * fl_tree_lstm_bf16_workspace_bytes(n_trees, n_nodes, roots_only): as fl_tree_lstm_workspace_bytes.
 * fl_tree_lstm_bf16: the arguments of fl_tree_lstm with packed_dev / packed_bytes in place of u_iou_dev, w_c_dev and u_f_dev;
 *   w_iou_dev f32 [384][12], b_iou_dev f32 [384], b_c_dev f32 [128], w_f_dev f32 [128][12], b_f_dev f32 [128].  The same checks,
 *   before any HIP call, with the same error codes (FL_ERR_ARG: sizes, (n_nodes - 1) % 3, roots_only, a NULL or misaligned
 *   pointer, a workspace or packed buffer that is too small); one launch on hip_stream, no host synchronisation. */
#ifndef FLATLAND_POLICY_BF16_H
#define FLATLAND_POLICY_BF16_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fl_tree_lstm_bf16_packed_bytes(void);
int fl_tree_lstm_pack_bf16(const float *u_iou_dev, const float *w_c_dev, const float *u_f_dev, void *packed_dev, size_t packed_bytes,
                           void *hip_stream);
size_t fl_tree_lstm_bf16_workspace_bytes(int n_trees, int n_nodes, int roots_only);
int fl_tree_lstm_bf16(int n_trees, int n_nodes, const float *forest_dev, const int64_t *adjacency_dev, const int64_t *node_order_dev,
                      const int64_t *edge_order_dev, const float *w_iou_dev, const float *b_iou_dev, const float *b_c_dev,
                      const float *w_f_dev, const float *b_f_dev, const void *packed_dev, size_t packed_bytes, int roots_only,
                      float *h_dev, float *c_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
