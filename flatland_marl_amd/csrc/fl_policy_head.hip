// fl_policy_head.hip -- entry points of include/flatland_policy.h and include/flatland_policy_train.h: the checks (all before any
// HIP call) and the launches of the kernels in fl_policy_head.h and fl_policy_head_bwd.h; behind them those of
// include/flatland_policy_head_bf16.h and fl_policy_head_bf16.h, and those of include/flatland_ppo.h and fl_ppo.h (whose draw is this
// unit's fph_choose).
#include <algorithm>
#include <cmath>

#include "../../include/flatland_policy.h"
#include "../../include/flatland_policy_train.h"
#include "../../include/flatland_policy_head_bf16.h"
#include "../../include/flatland_ppo.h"
#include "fl_policy_head.h"
#include "fl_policy_head_bf16.h"
#include "fl_policy_head_bwd.h"
#include "fl_policy_host.h"
#include "fl_ppo.h"

size_t fl_policy_head_workspace_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    const size_t R = (size_t)n_envs * n_agents;
    return (R * FPH_ROW_FLOATS * sizeof(float) + 15) / 16 * 16;
}

// sizes, NULLs and alignment of what the forward's entry points share; `fn` names the caller in the message
static int fph_check(const char *fn, int n_envs, int n_agents, const float *const *params, const FlPtr *tab, int n) {
    if (fph_check_sizes(fn, n_envs, n_agents) != FL_OK) return FL_ERR_ARG;
    if (!params) { fl_set_error("%s: params is NULL", fn); return FL_ERR_ARG; }
    if (fl_check_ptrs(fn, tab, n) != FL_OK) return FL_ERR_ARG;
    for (int i = 0; i < FPH_NPARAMS; i++)
        if (fl_check_param(fn, params, i) != FL_OK) return FL_ERR_ARG;
    return FL_OK;
}

// value, select, the mask, the actions and u of fl_policy_head and fl_policy_head_bf16
static int fph_check_choice(const char *fn, const float *value_dev, const uint8_t *valid_actions_dev, int select, double u,
                            const uint8_t *actions_dev) {
    const FlPtr value = {value_dev, "value", 16, true};
    if (fl_check_ptrs(fn, &value, 1) != FL_OK) return FL_ERR_ARG;
    if (select < 0 || select > 2) { fl_set_error("%s: select must be 0 (none), 1 (soft) or 2 (hard), got %d", fn, select); return FL_ERR_ARG; }
    if (select != 0 && (!valid_actions_dev || !actions_dev)) {
        fl_set_error("%s: select %d needs valid_actions and actions", fn, select);
        return FL_ERR_ARG;
    }
    if (!(u >= 0.0 && u < 1.0)) { fl_set_error("%s: u must be in [0, 1), got %g", fn, u); return FL_ERR_ARG; }
    return FL_OK;
}

// what the three forwards' arguments share; the caller places the arrays (emb, xa, xb, ao, qkv, val, y3)
static void fph_fill(FphArgs &a, int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                     const uint8_t *valid_actions_dev, int select, double u, float *logits_dev, float *value_dev, uint8_t *actions_dev) {
    a.B = n_envs; a.A = n_agents; a.R = n_envs * n_agents;
    a.select = select; a.u = u;
    a.attr = attr_dev; a.tree = tree_dev;
    for (int i = 0; i < FPH_NPARAMS; i++) a.p[i] = params[i];
    a.valid = valid_actions_dev; a.logits = logits_dev; a.value = value_dev; a.actions = actions_dev;
    a.ao = nullptr; a.qkv = nullptr; a.y3 = nullptr;
}

// emb, xa, xb = the first three [R][256] arrays of an inference workspace.  Returns the workspace as floats: the caller places the
// rest (ao, qkv, val) behind them
static float *fph_workspace(FphArgs &a, void *workspace_dev) {
    const size_t R = (size_t)a.R;
    float *f = (float *)workspace_dev;
    a.emb = f; a.xa = f + R * FPH_E; a.xb = f + 2 * R * FPH_E;
    return f;
}

// workgroups of the row-tile kernels (tiles of 32 rows) and of the attention kernels (an env's tiles of 32 agents, every env)
struct FphGrid { int tiles, qtiles; };
static FphGrid fph_grid(int n_envs, int n_agents) {
    return {(n_envs * n_agents + FPH_ROWS - 1) / FPH_ROWS, n_envs * ((n_agents + FPH_ROWS - 1) / FPH_ROWS)};
}

// more than 64 KiB of dynamic LDS needs the attribute
template <class K>
static int fph_allow_lds(const char *fn, K kernel, size_t bytes) {
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return FL_OK;
    fl_set_error("%s: hipFuncSetAttribute failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return FL_ERR_HIP;
}

// the forward's launches; block i's attention output goes to ao[i], its q k v are read from qkv[i]
static int fph_launch(const char *fn, FphArgs a, float *const (&ao)[3], float *const (&qkv)[3], hipStream_t s) {
    if (fph_allow_lds(fn, k_ph_embed, FPH_LDS_EMBED) != FL_OK || fph_allow_lds(fn, k_ph_block<false>, FPH_LDS_BLOCK) != FL_OK ||
        fph_allow_lds(fn, k_ph_block<true>, FPH_LDS_LAST) != FL_OK) return FL_ERR_HIP;
    const auto [tiles, qtiles] = fph_grid(a.B, a.A);
    a.qkv = qkv[0];
    hipLaunchKernelGGL(k_ph_embed, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_EMBED, s, a);
    const float *xin[3] = {a.emb, a.xa, a.xb};
    float *xout[3] = {a.xa, a.xb, nullptr};
    for (int blk = 0; blk < 3; blk++) {
        a.qkv = qkv[blk]; a.ao = ao[blk];
        hipLaunchKernelGGL(k_ph_attn, dim3(qtiles), dim3(FPH_THREADS), 0, s, a);
        if (blk < 2) {
            a.qkv = qkv[blk + 1];
            hipLaunchKernelGGL(k_ph_block<false>, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_BLOCK, s, a, blk, xin[blk], xout[blk]);
        } else {
            hipLaunchKernelGGL(k_ph_block<true>, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_LAST, s, a, blk, xin[blk], xout[blk]);
        }
    }
    if (a.value) hipLaunchKernelGGL(k_ph_value, dim3(a.B), dim3(64), 0, s, a);
    return fl_launched(fn);
}

int fl_policy_head(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                   const uint8_t *valid_actions_dev, int select, double u, float *logits_dev, float *value_dev,
                   uint8_t *actions_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_policy_head";
    const FlPtr tab[] = {{attr_dev, "attr", 16}, {tree_dev, "tree", 16}, {logits_dev, "logits", 16}, {workspace_dev, "workspace", 16}};
    if (fph_check(fn, n_envs, n_agents, params, tab, 4) != FL_OK ||
        fph_check_choice(fn, value_dev, valid_actions_dev, select, u, actions_dev) != FL_OK ||
        fl_check_bytes(fn, "workspace", workspace_bytes, fl_policy_head_workspace_bytes(n_envs, n_agents),
                       "fl_policy_head_workspace_bytes") != FL_OK) return FL_ERR_ARG;

    FphArgs a;
    fph_fill(a, n_envs, n_agents, attr_dev, tree_dev, params, valid_actions_dev, select, u, logits_dev, value_dev, actions_dev);
    float *ws = fph_workspace(a, workspace_dev);
    const size_t R = (size_t)a.R;
    a.val = ws + 7 * R * FPH_E;
    float *ao1 = ws + 3 * R * FPH_E, *qkv1 = ws + 4 * R * FPH_E;          // the three blocks share one array of each
    float *const ao[3] = {ao1, ao1, ao1}, *const qkv[3] = {qkv1, qkv1, qkv1};
    return fph_launch(fn, a, ao, qkv, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------------------------- training
size_t fl_policy_head_saved_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    const size_t R = (size_t)n_envs * n_agents;
    return (R * FPB_SAVED_FLOATS * sizeof(float) + 15) / 16 * 16;
}

size_t fl_policy_head_backward_rows_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    return (size_t)n_envs * n_agents * FPB_ROW_FLOATS * sizeof(float);
}

size_t fl_policy_head_backward_workspace_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    return (size_t)n_envs * n_agents * FPB_STATS * sizeof(float);
}

int fl_policy_head_forward_saved(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                                 float *logits_dev, float *value_dev, void *saved_dev, size_t saved_bytes, void *hip_stream) {
    const char *fn = "fl_policy_head_forward_saved";
    const FlPtr tab[] = {{attr_dev, "attr", 16}, {tree_dev, "tree", 16}, {logits_dev, "logits", 16}, {saved_dev, "saved", 16}};
    const FlPtr value = {value_dev, "value", 16, true};
    if (fph_check(fn, n_envs, n_agents, params, tab, 4) != FL_OK || fl_check_ptrs(fn, &value, 1) != FL_OK ||
        fl_check_bytes(fn, "saved buffer", saved_bytes, fl_policy_head_saved_bytes(n_envs, n_agents), "fl_policy_head_saved_bytes") != FL_OK)
        return FL_ERR_ARG;
    FphArgs a;
    fph_fill(a, n_envs, n_agents, attr_dev, tree_dev, params, nullptr, 0, 0.0, logits_dev, value_dev, nullptr);
    const auto sv = [&](int k) { return fpl_saved((float *)saved_dev, (size_t)a.R, k); };
    a.emb = sv(FPL_S_EMB); a.xa = sv(FPL_S_Y1); a.xb = sv(FPL_S_Y2); a.y3 = sv(FPL_S_Y3); a.val = sv(FPL_S_VAL);
    float *const ao[3] = {sv(FPL_S_C0), sv(FPL_S_C1), sv(FPL_S_C2)}, *const qkv[3] = {sv(FPL_S_QKV0), sv(FPL_S_QKV1), sv(FPL_S_QKV2)};
    return fph_launch(fn, a, ao, qkv, (hipStream_t)hip_stream);
}

// the backward's arguments: the saved arrays and the rows by name (fl_policy_layout.h)
static void fpb_fill(FpbArgs &a, int n_envs, int n_agents, const float *attr_dev, const float *const *params, const float *saved,
                     const float *grad_logits_dev, const float *grad_value_dev, float *grad_tree_dev, float *rows, float *stats) {
    a.B = n_envs; a.A = n_agents; a.R = n_envs * n_agents;
    a.attr = attr_dev;
    for (int i = 0; i < FPH_NPARAMS; i++) a.p[i] = params[i];
    a.gl = grad_logits_dev; a.gv = grad_value_dev; a.gtree = grad_tree_dev;
    a.stats = stats;
    const size_t R = (size_t)a.R;
    const auto sv = [&](int k) { return fpl_saved(saved, R, k); };
    const auto rw = [&](int k) { return fpl_rows(rows, R, k); };
    for (int i = 0; i < 4; i++) a.y[i] = sv(FPL_S_EMB + i);
    for (int i = 0; i < 3; i++) { a.ao[i] = sv(FPL_S_C0 + i); a.qkv[i] = sv(FPL_S_QKV0 + i); }
    for (int i = 0; i < 4; i++) a.a_dz[i] = rw(FPL_R_ATTR_DZ0 + i);
    for (int i = 0; i < 3; i++) a.a_h[i] = rw(FPL_R_ATTR_H1 + i);
    for (int i = 0; i < 3; i++) {
        const int b = i * FPL_R_PER_BLOCK;
        a.dqkv[i] = rw(FPL_R_DQKV0 + b); a.dout[i] = rw(FPL_R_DO0 + b); a.dz[i] = rw(FPL_R_DZ0 + b);
        a.o[i] = rw(FPL_R_O0 + b); a.dc[i] = rw(FPL_R_DC0 + b); a.dy[i] = rw(FPL_R_DY0 + b);
    }
    a.dy[3] = rw(FPL_R_DY3);
    for (int hd = 0; hd < 2; hd++) {
        const int h = hd * FPL_R_PER_HEAD;
        a.h_dz[hd][0] = rw(FPL_R_ACTOR_DZ0 + h); a.h_dz[hd][1] = rw(FPL_R_ACTOR_DZ2 + h); a.h_dz[hd][2] = rw(FPL_R_ACTOR_DZ4 + h);
        a.h_h[hd][0] = rw(FPL_R_ACTOR_U1 + h); a.h_h[hd][1] = rw(FPL_R_ACTOR_U2 + h);
    }
}

int fl_policy_head_backward(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                            const void *saved_dev, const float *grad_logits_dev, const float *grad_value_dev, float *grad_tree_dev,
                            void *rows_dev, size_t rows_bytes, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_policy_head_backward";
    const FlPtr tab[] = {{attr_dev, "attr", 16}, {tree_dev, "tree", 16}, {saved_dev, "saved", 16}, {grad_tree_dev, "grad_tree", 16},
                         {rows_dev, "rows", 16}, {workspace_dev, "workspace", 16}};
    const FlPtr grads[] = {{grad_logits_dev, "grad_logits", 16, true}, {grad_value_dev, "grad_value", 16, true}};
    if (fph_check(fn, n_envs, n_agents, params, tab, 6) != FL_OK) return FL_ERR_ARG;
    if (!grad_logits_dev && !grad_value_dev) { fl_set_error("%s: grad_logits and grad_value are both NULL", fn); return FL_ERR_ARG; }
    if (fl_check_ptrs(fn, grads, 2) != FL_OK ||
        fl_check_bytes(fn, "rows", rows_bytes, fl_policy_head_backward_rows_bytes(n_envs, n_agents),
                       "fl_policy_head_backward_rows_bytes") != FL_OK ||
        fl_check_bytes(fn, "workspace", workspace_bytes, fl_policy_head_backward_workspace_bytes(n_envs, n_agents),
                       "fl_policy_head_backward_workspace_bytes") != FL_OK) return FL_ERR_ARG;

    FpbArgs a;
    fpb_fill(a, n_envs, n_agents, attr_dev, params, (const float *)saved_dev, grad_logits_dev, grad_value_dev, grad_tree_dev,
             (float *)rows_dev, (float *)workspace_dev);

    hipStream_t s = (hipStream_t)hip_stream;
    if (fph_allow_lds(fn, k_pb_heads, FPB_LDS_HEADS) != FL_OK || fph_allow_lds(fn, k_pb_block, FPB_LDS_BLOCK) != FL_OK ||
        fph_allow_lds(fn, k_pb_inproj, FPB_LDS_INPROJ) != FL_OK || fph_allow_lds(fn, k_pb_attr, FPB_LDS_ATTR) != FL_OK) return FL_ERR_HIP;
    const auto [tiles, qtiles] = fph_grid(n_envs, n_agents);
    hipLaunchKernelGGL(k_pb_heads, dim3(tiles), dim3(FPH_THREADS), FPB_LDS_HEADS, s, a);
    for (int blk = 2; blk >= 0; blk--) {
        hipLaunchKernelGGL(k_pb_block, dim3(tiles), dim3(FPH_THREADS), FPB_LDS_BLOCK, s, a, blk);
        hipLaunchKernelGGL(k_pb_attn_q, dim3(qtiles), dim3(FPH_THREADS), 0, s, a, blk);
        hipLaunchKernelGGL(k_pb_attn_kv, dim3(qtiles), dim3(FPH_THREADS), 0, s, a, blk);
        hipLaunchKernelGGL(k_pb_inproj, dim3(tiles), dim3(FPH_THREADS), FPB_LDS_INPROJ, s, a, blk);
    }
    hipLaunchKernelGGL(k_pb_attr, dim3(tiles), dim3(FPH_THREADS), FPB_LDS_ATTR, s, a);
    return fl_launched(fn);
}

// ---------------------------------------------------------------------------------------------------------------- bf16 inference
size_t fl_policy_head_bf16_packed_bytes(void) { return (size_t)FPH16_PACKED * sizeof(__bf16); }

size_t fl_policy_head_bf16_workspace_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    const size_t R = (size_t)n_envs * n_agents;
    return (R * FPH16_ROW_BYTES + 15) / 16 * 16;
}

static_assert(fpl_bf16_param(FPH16_NMAT - 1) >= 0 && fpl_bf16_param(FPH16_NMAT) < 0, "the parameter table marks the 16 packed matrices");
static_assert(fpl_bf16_before(FPH16_NMAT) == FPH16_PACKED, "the pack kernel writes as many elements as fl_policy_head_bf16_packed_bytes counts");

static int fph16_check_packed(const char *fn, size_t packed_bytes) {
    return fl_check_bytes(fn, "packed buffer", packed_bytes, fl_policy_head_bf16_packed_bytes(), "fl_policy_head_bf16_packed_bytes");
}

int fl_policy_head_pack_bf16(const float *const *params, void *packed_dev, size_t packed_bytes, void *hip_stream) {
    const char *fn = "fl_policy_head_pack_bf16";
    if (!params) { fl_set_error("%s: params is NULL", fn); return FL_ERR_ARG; }
    for (int m = 0; m < FPH16_NMAT; m++)
        if (fl_check_param(fn, params, fpl_bf16_param(m)) != FL_OK) return FL_ERR_ARG;
    const FlPtr packed = {packed_dev, "packed", 16};
    if (fl_check_ptrs(fn, &packed, 1) != FL_OK || fph16_check_packed(fn, packed_bytes) != FL_OK) return FL_ERR_ARG;
    FlBf16Pack<FPH16_NMAT> a;
    int rows[FPH16_NMAT];
    for (int m = 0; m < FPH16_NMAT; m++) {
        const int i = fpl_bf16_param(m);
        a.src[m] = params[i]; a.K[m] = FPL_PARAMS[i].in; rows[m] = FPL_PARAMS[i].out;
    }
    fl_launch_bf16_pack(a, rows, packed_dev, (hipStream_t)hip_stream);                // (a.off[16] = FPH16_PACKED)
    return fl_launched(fn);
}

int fl_policy_head_bf16(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                        const void *packed_dev, size_t packed_bytes, const uint8_t *valid_actions_dev, int select, double u,
                        float *logits_dev, float *value_dev, uint8_t *actions_dev, void *workspace_dev, size_t workspace_bytes,
                        void *hip_stream) {
    const char *fn = "fl_policy_head_bf16";
    const FlPtr tab[] = {{attr_dev, "attr", 16}, {tree_dev, "tree", 16}, {logits_dev, "logits", 16}, {workspace_dev, "workspace", 16},
                         {packed_dev, "packed", 16}};
    if (fph_check(fn, n_envs, n_agents, params, tab, 5) != FL_OK ||
        fph_check_choice(fn, value_dev, valid_actions_dev, select, u, actions_dev) != FL_OK ||
        fl_check_bytes(fn, "workspace", workspace_bytes, fl_policy_head_bf16_workspace_bytes(n_envs, n_agents),
                       "fl_policy_head_bf16_workspace_bytes") != FL_OK ||
        fph16_check_packed(fn, packed_bytes) != FL_OK) return FL_ERR_ARG;

    Fph16Args a;
    fph_fill(a, n_envs, n_agents, attr_dev, tree_dev, params, valid_actions_dev, select, u, logits_dev, value_dev, actions_dev);
    float *ws = fph_workspace(a, workspace_dev);
    const size_t R = (size_t)a.R;
    a.ao = ws + 3 * R * FPH_E;
    a.qkv16 = (__bf16 *)(ws + 4 * R * FPH_E);
    a.val = (float *)(a.qkv16 + R * 3 * FPH_E);
    a.packed = (const __bf16 *)packed_dev;

    hipStream_t s = (hipStream_t)hip_stream;
    const auto [tiles, qtiles] = fph_grid(a.B, a.A);
    hipLaunchKernelGGL(k_ph16_embed, dim3(tiles), dim3(FPH_THREADS), 0, s, a);
    const float *xin[3] = {a.emb, a.xa, a.xb};
    float *xout[3] = {a.xa, a.xb, nullptr};
    for (int blk = 0; blk < 3; blk++) {
        hipLaunchKernelGGL(k_ph16_attn, dim3(qtiles), dim3(FPH_THREADS), 0, s, a);
        if (blk < 2) hipLaunchKernelGGL(k_ph16_block<false>, dim3(tiles), dim3(FPH_THREADS), 0, s, a, blk, xin[blk], xout[blk]);
        else hipLaunchKernelGGL(k_ph16_block<true>, dim3(tiles), dim3(FPH_THREADS), 0, s, a, blk, xin[blk], xout[blk]);
    }
    if (a.value) hipLaunchKernelGGL(k_ph_value, dim3(a.B), dim3(64), 0, s, (FphArgs)a);
    return fl_launched(fn);
}

// ---------------------------------------------------------------------------------------------------------------- PPO (include/flatland_ppo.h)
static int fpp_groups(int n) { return (n + FPP_THREADS - 1) / FPP_THREADS; }
static bool fpp_size(int n) { return n >= 1 && n <= FL_PPO_MAX_ROWS; }      // (a lane's row index and its strides stay inside an int)

// workgroups of k_ppo_rows (a workgroup takes 256 rows and 256 values) and of k_ppo_count
struct FppGrid { int groups, count_groups; };
static FppGrid fpp_grid(int n_rows, int n_envs) {
    const int row_groups = fpp_groups(n_rows), groups = n_envs > 0 ? std::max(row_groups, fpp_groups(n_envs)) : row_groups;
    return {groups, std::min(row_groups, FPP_COUNT_GROUPS)};
}

size_t fl_ppo_loss_workspace_bytes(int n_rows, int n_envs) {
    if (!fpp_size(n_rows) || (n_envs != 0 && !fpp_size(n_envs))) return 0;
    const auto [groups, count_groups] = fpp_grid(n_rows, n_envs);
    return ((size_t)groups * FPP_SUMS * sizeof(double) + (size_t)count_groups * 2 * sizeof(int) + 15) / 16 * 16;
}

int fl_policy_sample(int n_rows, const float *logits_dev, const uint8_t *valid_dev, const double *u_dev, uint8_t *actions_dev,
                     float *logp_dev, float *entropy_dev, void *hip_stream) {
    const char *fn = "fl_policy_sample";
    if (!fpp_size(n_rows)) { fl_set_error("%s: bad sizes (n_rows %d; 1 <= n_rows <= %d)", fn, n_rows, FL_PPO_MAX_ROWS); return FL_ERR_ARG; }
    const FlPtr tab[] = {{logits_dev, "logits", 16}, {valid_dev, "valid", 1}, {u_dev, "u", 16}, {actions_dev, "actions", 1},
                         {logp_dev, "logp", 16, true}, {entropy_dev, "entropy", 16, true}};
    if (fl_check_ptrs(fn, tab, 6) != FL_OK) return FL_ERR_ARG;
    hipLaunchKernelGGL(k_policy_sample, dim3(fpp_groups(n_rows)), dim3(FPP_THREADS), 0, (hipStream_t)hip_stream, n_rows, logits_dev,
                       valid_dev, u_dev, actions_dev, logp_dev, entropy_dev);
    return fl_launched(fn);
}

int fl_ppo_loss(int n_rows, int n_envs, const float *logits_dev, const uint8_t *valid_dev, const uint8_t *actions_dev,
                const float *old_logp_dev, const float *adv_dev, const uint8_t *mask_dev, const float *value_dev,
                const float *returns_dev, double clip_eps, double vf_coef, double ent_coef, float *grad_logits_dev,
                float *grad_value_dev, double *stats_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_ppo_loss";
    const int critic = (value_dev != nullptr) + (returns_dev != nullptr) + (grad_value_dev != nullptr);
    if (critic != 0 && critic != 3) {
        fl_set_error("%s: value, returns and grad_value are all three NULL or all three given (value %s, returns %s, grad_value %s)", fn,
                     value_dev ? "given" : "NULL", returns_dev ? "given" : "NULL", grad_value_dev ? "given" : "NULL");
        return FL_ERR_ARG;
    }
    if (!fpp_size(n_rows) || (n_envs != 0 && !fpp_size(n_envs)) || (n_envs == 0 && critic)) {
        fl_set_error("%s: bad sizes (n_rows %d, n_envs %d; 1 <= n_rows <= %d, 1 <= n_envs <= %d, n_envs 0 only without value, returns and "
                     "grad_value)", fn, n_rows, n_envs, FL_PPO_MAX_ROWS, FL_PPO_MAX_ROWS);
        return FL_ERR_ARG;
    }
    const FlPtr tab[] = {{logits_dev, "logits", 16}, {valid_dev, "valid", 1}, {actions_dev, "actions", 1}, {old_logp_dev, "old_logp", 16},
                         {adv_dev, "adv", 16}, {mask_dev, "mask", 1, true}, {value_dev, "value", 16, true},
                         {returns_dev, "returns", 16, true}, {grad_logits_dev, "grad_logits", 16}, {grad_value_dev, "grad_value", 16, true},
                         {stats_dev, "stats", 16}, {workspace_dev, "workspace", 16}};
    if (fl_check_ptrs(fn, tab, 12) != FL_OK) return FL_ERR_ARG;
    const struct { double v; const char *name; } coef[] = {{clip_eps, "clip_eps"}, {vf_coef, "vf_coef"}, {ent_coef, "ent_coef"}};
    for (const auto &c : coef)
        if (!std::isfinite(c.v)) { fl_set_error("%s: %s must be finite, got %g", fn, c.name, c.v); return FL_ERR_ARG; }
    if (clip_eps < 0.0) { fl_set_error("%s: clip_eps must be >= 0, got %g", fn, clip_eps); return FL_ERR_ARG; }
    const int n_values = critic ? n_envs : 0;
    if (fl_check_bytes(fn, "workspace", workspace_bytes, fl_ppo_loss_workspace_bytes(n_rows, n_values), "fl_ppo_loss_workspace_bytes") != FL_OK)
        return FL_ERR_ARG;

    FppLossArgs a;
    a.R = n_rows; a.B = n_values;
    const auto [groups, count_groups] = fpp_grid(n_rows, n_values);
    a.groups = groups; a.count_groups = count_groups;
    a.logits = logits_dev; a.valid = valid_dev; a.actions = actions_dev; a.mask = mask_dev;
    a.old_logp = old_logp_dev; a.adv = adv_dev; a.value = value_dev; a.returns = returns_dev;
    a.clip_eps = clip_eps; a.vf_coef = vf_coef; a.ent_coef = ent_coef;
    a.grad_logits = grad_logits_dev; a.grad_value = grad_value_dev; a.stats = stats_dev;
    a.sums = (double *)workspace_dev;
    a.counts = (int *)(a.sums + (size_t)groups * FPP_SUMS);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_ppo_count, dim3(count_groups), dim3(FPP_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_ppo_rows, dim3(groups), dim3(FPP_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_ppo_final, dim3(1), dim3(FPP_THREADS), 0, s, a);
    return fl_launched(fn);
}

int fl_gae(int n_steps, int n_cols, const float *rewards_dev, const float *values_dev, const uint8_t *dones_dev, double gamma,
           double lam, float *adv_dev, float *returns_dev, void *hip_stream) {
    const char *fn = "fl_gae";
    if (n_steps <= 0 || !fpp_size(n_cols)) {
        fl_set_error("%s: bad sizes (n_steps %d, n_cols %d; 1 <= n_steps, 1 <= n_cols <= %d)", fn, n_steps, n_cols, FL_PPO_MAX_ROWS);
        return FL_ERR_ARG;
    }
    const FlPtr tab[] = {{rewards_dev, "rewards", 16}, {values_dev, "values", 16}, {dones_dev, "dones", 1}, {adv_dev, "adv", 16},
                         {returns_dev, "returns", 16}};
    if (fl_check_ptrs(fn, tab, 5) != FL_OK) return FL_ERR_ARG;
    if (!(gamma >= 0.0 && gamma <= 1.0)) { fl_set_error("%s: gamma must be in [0, 1], got %g", fn, gamma); return FL_ERR_ARG; }
    if (!(lam >= 0.0 && lam <= 1.0)) { fl_set_error("%s: lam must be in [0, 1], got %g", fn, lam); return FL_ERR_ARG; }
    hipLaunchKernelGGL(k_gae, dim3(fpp_groups(n_cols)), dim3(FPP_THREADS), 0, (hipStream_t)hip_stream, n_steps, n_cols, rewards_dev,
                       values_dev, dones_dev, gamma, lam, adv_dev, returns_dev);
    return fl_launched(fn);
}
