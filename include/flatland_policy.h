/* flatland_policy.h -- the policy network after its tree encoder and the actor's choice of an action, on the GPU.
 * Exported by libflatland_hip.so next to include/flatland_hip.h (whose error codes and fl_last_error these use).
 *
 *   fl_policy_head      Network.forward after tree_lstm (solution/nn/net_tree.py:82-103: attr_embedding, the three Transformer
 *                       blocks, actor_net, critic_net and its mean over the agents) and Actor._choose_action per agent
 *                       (solution/plfActor.py:30-46)
 *
 * Sizes are the solution's (solution/impl_config.py): agent_attr 83, hidden_sz 128, tree_embedding_sz 128 (embedding 256),
 * 4 heads of 64, 5 actions; other sizes do not exist here.  Float32 end to end.
 *
 * Stateless: device pointers, everything enqueued on hip_stream (8 kernel launches; 7 with value_dev NULL), no host
 * synchronisation, no allocation, nothing cached across calls -- the parameters are read as they are at every call.
 *
 *   attr_dev   f32[B][A][83]    agents_attr as fl_obs_cutils_policy writes it
 *   tree_dev   f32[B][A][128]   node 0 of every tree of fl_tree_lstm (roots_only = 1)
 *   params     a HOST array of FL_POLICY_HEAD_NPARAMS device pointers: the Network's state_dict without tree_lstm.*, in
 *              state_dict order, every tensor in torch's own layout ([out][in] row-major), contiguous:
 *                 0  attr_embedding.0.weight [256][83]     1  attr_embedding.0.bias [256]
 *                 2  attr_embedding.2.weight [256][256]    3  attr_embedding.2.bias [256]
 *                 4  attr_embedding.4.weight [256][256]    5  attr_embedding.4.bias [256]
 *                 6  attr_embedding.6.weight [128][256]    7  attr_embedding.6.bias [128]
 *                 8 + 6 i, i = 0 .. 2 (transformer.i.):
 *                    +0 attention.in_proj_weight [768][256] (rows q, k, v; head h = columns 64 h .. 64 h + 63 of each)
 *                    +1 attention.in_proj_bias [768]        +2 attention.out_proj.weight [256][256]
 *                    +3 attention.out_proj.bias [256]       +4 att_mlp.0.weight [256][512]     +5 att_mlp.0.bias [256]
 *                26  actor_net.0.weight [256][512]   27 actor_net.0.bias [256]    28 actor_net.2.weight [128][256]
 *                29  actor_net.2.bias [128]          30 actor_net.4.weight [5][128]   31 actor_net.4.bias [5]
 *                32  critic_net.0.weight [256][512]  33 critic_net.0.bias [256]   34 critic_net.2.weight [128][256]
 *                35  critic_net.2.bias [128]         36 critic_net.4.weight [1][128]  37 critic_net.4.bias [1]
 *   valid_actions_dev u8[B][A][5] (non-zero = valid) or NULL with select = 0
 *   logits_dev f32[B][A][5]; value_dev f32[B] (the mean of the critic over the env's agents, summed in a fixed order: two calls
 *              give the same bits) or NULL (critic_net is not run); actions_dev u8[B][A] or NULL with select = 0, ready for fl_step
 *
 * The attention runs over the agents of ONE env (the sequence) with the envs as the batch: no attention across envs, whatever
 * n_agents is; softmax over all n_agents keys, no mask, no dropout.  GELU is the exact (erf) form.
 *
 * select = 1 (soft): softmax of the valid actions' logits in float32 (as numpy on a float32 array), then numpy.random.choice's
 * inverse-CDF draw with the uniform number u: the float64 cumulative sum divided by its last element, searchsorted(u,
 * side = "right").  The reference seeds numpy with 42 before EVERY draw, so its u is the constant
 * RandomState(42).random_sample() = 0.3745401188473625 and its action a function of logits and mask.  An agent without a valid
 * action gets 0 (the reference draws from a mask of ones whose nonzero()[0] is five zeros).
 * select = 2 (hard): the first largest of those probabilities.  An agent without a valid action gets 0 HERE; the reference
 * raises IndexError there.
 *
 * workspace_dev: at least fl_policy_head_workspace_bytes(n_envs, n_agents) bytes, 16-byte aligned (B * A * 7172 bytes: the
 * embedding, two block outputs, the attention output, q k v, a critic value per agent).
 *
 * FL_ERR_ARG before any HIP call: n_envs <= 0, n_agents outside [1, 1024], a NULL attr / tree / params / parameter / logits /
 * workspace, a float pointer not 16-byte aligned, select outside 0 .. 2, select != 0 with a NULL mask or NULL actions, u outside
 * [0, 1), a short workspace.
 */
#ifndef FLATLAND_POLICY_H
#define FLATLAND_POLICY_H
#include "flatland_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FL_POLICY_HEAD_NPARAMS 38
#define FL_POLICY_SELECT_NONE 0
#define FL_POLICY_SELECT_SOFT 1
#define FL_POLICY_SELECT_HARD 2
#define FL_POLICY_U_REFERENCE 0.3745401188473625 /* numpy.random.RandomState(42).random_sample() */

size_t fl_policy_head_workspace_bytes(int n_envs, int n_agents);
int fl_policy_head(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                   const uint8_t *valid_actions_dev, int select, double u, float *logits_dev, float *value_dev,
                   uint8_t *actions_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
