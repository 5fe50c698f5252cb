/* flatland_policy_head_bf16.h -- the policy network after its tree encoder for inference with bf16 matrix operands.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose error codes and fl_last_error this uses; a header of its own,
 * as flatland_policy.h and flatland_policy_bf16.h are, so that flatland_hip.h stays the list it was).
 *
 * fl_policy_head_bf16 is fl_policy_head (flatland_policy.h: the same arguments, outputs, action choice and launch structure -- 8
 * launches on hip_stream, 7 with value_dev NULL, no host synchronisation, no allocation) with 16 of its 19 matrices on
 * v_mfma_f32_32x32x16_bf16.  "bf16" = rounded to nearest even, the upper 16 bits of the rounded float32.
 *
 *   bf16 operands, float32 sums from zero, float32 bias added last, float32 GELU:
 *       attr_embedding.2 / .4 / .6, the three blocks' in_proj, out_proj and att_mlp.0, actor_net.0 / .2, critic_net.0 / .2.
 *       The weights are rounded by fl_policy_head_pack_bf16; an activation is rounded once, where the product reads it.
 *   exact float32, as in fl_policy_head:
 *       attr_embedding.0 (its inputs are raw attributes), actor_net.4 and critic_net.4 (they read the float32 GELU output).
 *   q, k, v are rounded to bf16 after the float32 bias and kept so in the workspace.
 *   attention: q k^T with bf16 operands and float32 sums; the row maxima and e = expf((s - max) / 8) float32; e rounded to bf16
 *       for e v; the row sum is the float32 sum of the ROUNDED e; the quotient last.  An output is a convex combination of the
 *       bf16 v rows up to float32 summation.
 *   One writer per address, no atomics: two calls give the same bits.  Inference only: fl_policy_head_backward
 *   (flatland_policy_train.h) belongs to the float32 forward.
 *
 * fl_policy_head_bf16_packed_bytes(): the size of the packed weights, 3 342 336 bytes.
 * fl_policy_head_pack_bf16: params = the HOST array of 38 device pointers of fl_policy_head; the 16 matrices above are read from it
 *   (16-byte aligned, torch's [out][in] layout) and rounded into packed_dev (16-byte aligned, packed_bytes >=
 *   fl_policy_head_bf16_packed_bytes()): one launch on hip_stream, no host synchronisation.  Call it again after the weights changed.
 *   Layout: the 16 matrices one after another in state_dict order, each in the order include/flatland_policy_bf16.h documents: a
 *   matrix W [R][K] as R / 32 blocks of 32 rows, a block as its K / 16 steps, a step as 64 lanes x 8 elements, so that element
 *   512 (b K / 16 + s) + 8 l + j of a matrix is W[32 b + (l & 31)][16 s + 8 (l >> 5) + j].  Element offsets:
 *          attr_embedding.2.weight [256][256]         0      attr_embedding.4.weight [256][256]     65 536
 *          attr_embedding.6.weight [128][256]   131 072
 *          transformer.i (i = 0 .. 2), at 163 840 + 393 216 i:
 *             attention.in_proj_weight [768][256]    +0      attention.out_proj.weight [256][256] +196 608
 *             att_mlp.0.weight [256][512]      +262 144
 *          actor_net.0.weight [256][512]      1 343 488      actor_net.2.weight [128][256]       1 474 560
 *          critic_net.0.weight [256][512]     1 507 328      critic_net.2.weight [128][256]      1 638 400      (end: 1 671 168)
 * fl_policy_head_bf16_workspace_bytes(n_envs, n_agents): R * 5636 bytes, R = n_envs * n_agents, rounded up to 16.
 * fl_policy_head_bf16: the arguments of fl_policy_head with packed_dev / packed_bytes behind params.  params is still read: the
 *   biases, attr_embedding.0.weight, actor_net.4.weight and critic_net.4.weight as float32.  The same checks before any HIP call with
 *   the same error codes, the messages prefixed fl_policy_head_bf16:, and FL_ERR_ARG for a NULL or misaligned packed_dev and a short
 *   packed buffer.
 *
 * The workspace after a call (R rows):
 *     emb, xa, xb, ao   f32 [R][256] each   at floats 0, 256 R, 512 R, 768 R   (the embedding, the outputs of blocks 0 and 1, the
 *                                                                               attention output of block 2)
 *     qkv               bf16 [R][768]       at byte 4096 R                      (q | k | v of block 2, row-major)
 *     val               f32 [R]             at byte 5632 R                      (the critic per agent; not written with value NULL)
 */
#ifndef FLATLAND_POLICY_HEAD_BF16_H
#define FLATLAND_POLICY_HEAD_BF16_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fl_policy_head_bf16_packed_bytes(void);
int fl_policy_head_pack_bf16(const float *const *params, void *packed_dev, size_t packed_bytes, void *hip_stream);
size_t fl_policy_head_bf16_workspace_bytes(int n_envs, int n_agents);
int fl_policy_head_bf16(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                        const void *packed_dev, size_t packed_bytes, const uint8_t *valid_actions_dev, int select, double u,
                        float *logits_dev, float *value_dev, uint8_t *actions_dev, void *workspace_dev, size_t workspace_bytes,
                        void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
