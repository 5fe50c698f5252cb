/* flatland_ppo.h -- the per-step numerics of PPO on the GPU: a per-agent draw with its log-probability and entropy, generalised
 * advantage estimation, and the clipped-surrogate loss with its gradients on the logits and the value.
 * Exported by libflatland_hip.so next to include/flatland_policy.h (whose fl_policy_head makes the logits and whose
 * FL_POLICY_U_REFERENCE these use) and include/flatland_hip.h (error codes, fl_last_error).  The training loop, the roll-out buffer
 * and the optimiser stay with the caller.
 *
 *   fl_policy_sample   an action per row from its logits, its valid-action mask and its OWN uniform number; log pi(a), entropy
 *   fl_ppo_loss        L_pi + vf_coef L_v - ent_coef H over the counted rows; d/d logits, d/d value; eight statistics
 *   fl_gae             advantages and returns of T steps of N independent columns
 *
 * Stateless: device pointers only, everything enqueued on hip_stream (fl_policy_sample and fl_gae one kernel launch, fl_ppo_loss
 * three), no host synchronisation, no allocation, nothing cached across calls.  Float and double pointers are 16-byte aligned.
 * R = n_rows = the (env, agent) pairs, flattened; 5 actions.  No float atomics anywhere, one writer per address: two calls on
 * the same inputs give the same bits.
 *
 * Below, for one row: V = its valid actions (valid[j] != 0), x = its float32 logits, m = max over V of x.
 *
 * fl_policy_sample
 *   action_r  = Actor._choose_action's soft draw (solution/plfActor.py:30-46) with the row's u_r: the device function of
 *               fl_policy_head's select = 1, unchanged -- the float32 softmax over V as numpy computes it on a float32 array, the
 *               float64 cumulative sum divided by its last element, searchsorted(u_r, side = "right").  With every u_r equal to
 *               FL_POLICY_U_REFERENCE the actions are fl_policy_head's select = 1 actions bit for bit, and so the reference's.
 *   logp_r    = (x_a - m) - log sum_{j in V} exp(x_j - m)                          (a = action_r)
 *   entropy_r = - sum_{j in V} p_j logp_j,   p_j = exp(x_j - m) / sum_{k in V} exp(x_k - m)
 *   logp and entropy are evaluated in float64 from the float32 logits (the sums over V in ascending j) and rounded to float32
 *   once.  The draw's float32 probabilities and this float64 log-softmax differ by float32 roundings: logp_r is the log-probability
 *   of action_r under the float64 softmax, which is what fl_ppo_loss evaluates again.
 *   A row without a valid action: action 0 (as fl_policy_head), logp 0, entropy 0.  A row with one valid action: logp 0, entropy 0.
 *   u cannot be checked on the device: it is expected in [0, 1); u >= 1 yields the last valid action, a NaN the first.
 *   logp_dev / entropy_dev may be NULL (not written).
 *
 * fl_ppo_loss
 *   w_r = 1, unless mask_r == 0 (mask_dev NULL: no row is masked), or V is empty, or actions_r is not a valid action of the row
 *   (>= 5, or valid[actions_r] == 0).  stats[7] counts the rows that only the last reason excludes: mask_r != 0, V not empty, the
 *   action not valid.
 *   n     = sum_r w_r
 *   rho   = exp(logp_a - old_logp_r),  A = adv_r
 *   s     = min(rho A, clip(rho, 1 - eps, 1 + eps) A)
 *   L_pi  = - sum_r w_r s_r / n          Hbar = sum_r w_r H_r / n          (H_r = the row's entropy, as above)
 *   L_v   = 1/2 mean_b (v_b - R_b)^2 over the n_envs values, or 0 with value_dev NULL (then returns_dev and grad_value_dev are NULL
 *           too, n_envs is not used and may be 0)
 *   total = L_pi + vf_coef L_v - ent_coef Hbar
 *   The gradients of total:
 *     g_s              = rho A if (A >= 0 and rho <= 1 + eps) or (A < 0 and rho >= 1 - eps), else 0
 *     grad_logits[r][j] = (w_r / n) (- g_s (delta_{j,a} - p_j) + ent_coef p_j (logp_j + H_r))   for j in V, 0 for j not in V
 *     grad_value[b]    = vf_coef (v_b - R_b) / n_envs
 *   (these closed forms are torch's float64 autograd of the plain formula, torch.minimum's ties and clamp's inclusive bounds
 *   included).  n = 0: L_pi, Hbar, stats[4], stats[5] and every grad_logits are 0, no NaN; L_v and grad_value do not depend on n.
 *   stats (float64): [0] L_pi  [1] L_v  [2] Hbar  [3] total  [4] the mean over the counted rows of old_logp - logp_a
 *                    [5] the share of the counted rows with |rho - 1| > eps  [6] n  [7] rows excluded for an action that is not valid
 *   All per-row arithmetic is float64 with one rounding at each float32 store.  The sums are float64 in a fixed order: a workgroup
 *   of 256 rows (or values) in a fixed tree -- 64 lanes of a wavefront by cross-lane halving, the four wavefronts in order -- and the
 *   workgroups' sums by one workgroup whose lane t adds the sums of workgroups t, t + 256, ... in index order before the same tree.
 *   workspace_dev: at least fl_ppo_loss_workspace_bytes(n_rows, n_envs) bytes, 16-byte aligned; its contents before the call do not
 *   matter and mean nothing after it.  The byte function is monotone in both sizes, 0 for a size the call refuses, and with
 *   n_envs = 0 what a call without the value pointers needs (40 bytes per 256 rows or values, 8 per 256 rows up to 1024 times).
 *
 * fl_gae, per column, t from T - 1 down to 0, nd = 1 - (dones[t] != 0), A_T = 0:
 *   delta      = r_t + gamma * v_{t+1} * nd - v_t                     ((r_t + ((gamma v_{t+1}) nd)) - v_t)
 *   A_t        = delta + gamma * lam * nd * A_{t+1}                   (delta + (((gamma lam) nd) A_{t+1}))
 *   adv[t]     = f32(A_t),  returns[t] = f32(A_t + v_t)
 *   float64 throughout, in exactly that operation order, no contraction: a float64 evaluation in that order gives the same bits.
 *
 * FL_ERR_ARG before any HIP call:
 *   (a size is a count of rows, values or columns: 1 .. FL_PPO_MAX_ROWS)
 *   fl_policy_sample  n_rows <= 0; a NULL logits / valid / u / actions; a float or double pointer not 16-byte aligned
 *   fl_ppo_loss       n_rows <= 0; n_envs < 0, or 0 with a value pointer; a NULL logits / valid / actions / old_logp / adv /
 *                     grad_logits / stats / workspace; value, returns and grad_value not all three NULL or all three given; clip_eps,
 *                     vf_coef or ent_coef not finite, clip_eps < 0; a float or double pointer or the workspace not 16-byte aligned;
 *                     a short workspace
 *   fl_gae            n_steps <= 0 or n_cols <= 0; a NULL pointer; gamma or lam not finite or outside [0, 1]; a float pointer not
 *                     16-byte aligned
 */
#ifndef FLATLAND_PPO_H
#define FLATLAND_PPO_H
#include "flatland_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FL_PPO_STATS 8
#define FL_PPO_MAX_ROWS (1 << 28) /* the most rows, values and columns a call takes */

int fl_policy_sample(int n_rows, const float *logits_dev, const uint8_t *valid_dev, const double *u_dev, uint8_t *actions_dev,
                     float *logp_dev, float *entropy_dev, void *hip_stream);

size_t fl_ppo_loss_workspace_bytes(int n_rows, int n_envs);
int fl_ppo_loss(int n_rows, int n_envs, const float *logits_dev, const uint8_t *valid_dev, const uint8_t *actions_dev,
                const float *old_logp_dev, const float *adv_dev, const uint8_t *mask_dev, const float *value_dev,
                const float *returns_dev, double clip_eps, double vf_coef, double ent_coef, float *grad_logits_dev,
                float *grad_value_dev, double *stats_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream);

int fl_gae(int n_steps, int n_cols, const float *rewards_dev, const float *values_dev, const uint8_t *dones_dev, double gamma,
           double lam, float *adv_dev, float *returns_dev, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
