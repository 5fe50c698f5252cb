// fl_policy_head.hip -- entry points of include/flatland_policy.h: the checks (all before any HIP call) and the launches of the
// kernels in fl_policy_head.h.
#include "../../include/flatland_policy.h"
#include "fl_policy_head.h"

size_t fl_policy_head_workspace_bytes(int n_envs, int n_agents) {
    if (n_envs <= 0 || n_agents <= 0) return 0;
    const size_t R = (size_t)n_envs * n_agents;
    return (R * FPH_ROW_FLOATS * sizeof(float) + 15) / 16 * 16;
}

int fl_policy_head(int n_envs, int n_agents, const float *attr_dev, const float *tree_dev, const float *const *params,
                   const uint8_t *valid_actions_dev, int select, double u, float *logits_dev, float *value_dev,
                   uint8_t *actions_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    if (n_envs <= 0 || n_agents < 1 || n_agents > FPH_MAX_A || (long long)n_envs * n_agents > INT32_MAX / (3 * FPH_E)) {
        fl_set_error("fl_policy_head: bad sizes (n_envs %d, n_agents %d; 1 <= n_envs, 1 <= n_agents <= %d)", n_envs, n_agents, FPH_MAX_A);
        return FL_ERR_ARG;
    }
    if (!params) { fl_set_error("fl_policy_head: params is NULL"); return FL_ERR_ARG; }
    const void *f16[] = {attr_dev, tree_dev, logits_dev, workspace_dev};
    const char *f16n[] = {"attr", "tree", "logits", "workspace"};
    for (int i = 0; i < 4; i++) {
        if (!f16[i]) { fl_set_error("fl_policy_head: %s is NULL", f16n[i]); return FL_ERR_ARG; }
        if ((uintptr_t)f16[i] % 16) { fl_set_error("fl_policy_head: %s is not 16-byte aligned", f16n[i]); return FL_ERR_ARG; }
    }
    for (int i = 0; i < FPH_NPARAMS; i++) {
        if (!params[i]) { fl_set_error("fl_policy_head: parameter %d is NULL", i); return FL_ERR_ARG; }
        if ((uintptr_t)params[i] % 16) { fl_set_error("fl_policy_head: parameter %d is not 16-byte aligned", i); return FL_ERR_ARG; }
    }
    if (value_dev && (uintptr_t)value_dev % 16) { fl_set_error("fl_policy_head: value is not 16-byte aligned"); return FL_ERR_ARG; }
    if (select < 0 || select > 2) { fl_set_error("fl_policy_head: select must be 0 (none), 1 (soft) or 2 (hard), got %d", select); return FL_ERR_ARG; }
    if (select != 0 && (!valid_actions_dev || !actions_dev)) {
        fl_set_error("fl_policy_head: select %d needs valid_actions and actions", select);
        return FL_ERR_ARG;
    }
    if (!(u >= 0.0 && u < 1.0)) { fl_set_error("fl_policy_head: u must be in [0, 1), got %g", u); return FL_ERR_ARG; }
    const size_t need = fl_policy_head_workspace_bytes(n_envs, n_agents);
    if (workspace_bytes < need) {
        fl_set_error("fl_policy_head: workspace of %zu bytes, %zu needed (fl_policy_head_workspace_bytes)", workspace_bytes, need);
        return FL_ERR_ARG;
    }

    FphArgs a;
    a.B = n_envs; a.A = n_agents; a.R = n_envs * n_agents;
    a.select = select; a.u = u;
    a.attr = attr_dev; a.tree = tree_dev;
    for (int i = 0; i < FPH_NPARAMS; i++) a.p[i] = params[i];
    a.valid = valid_actions_dev; a.logits = logits_dev; a.value = value_dev; a.actions = actions_dev;
    const size_t R = (size_t)a.R;
    float *ws = (float *)workspace_dev;
    a.emb = ws; a.xa = ws + R * FPH_E; a.xb = ws + 2 * R * FPH_E; a.ao = ws + 3 * R * FPH_E;
    a.qkv = ws + 4 * R * FPH_E; a.val = ws + 7 * R * FPH_E;

    hipStream_t s = (hipStream_t)hip_stream;
    // more than 64 KiB of dynamic LDS needs the attribute
    if (hipFuncSetAttribute((const void *)k_ph_embed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FPH_LDS_EMBED) != hipSuccess ||
        hipFuncSetAttribute((const void *)k_ph_block<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FPH_LDS_BLOCK) != hipSuccess ||
        hipFuncSetAttribute((const void *)k_ph_block<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FPH_LDS_LAST) != hipSuccess) {
        fl_set_error("fl_policy_head: hipFuncSetAttribute failed: %s", hipGetErrorString(hipGetLastError()));
        return FL_ERR_HIP;
    }
    const int tiles = (a.R + FPH_ROWS - 1) / FPH_ROWS;
    const int qtiles = n_envs * ((n_agents + FPH_ROWS - 1) / FPH_ROWS);
    hipLaunchKernelGGL(k_ph_embed, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_EMBED, s, a);
    const float *xin[3] = {a.emb, a.xa, a.xb};
    float *xout[3] = {a.xa, a.xb, nullptr};
    for (int blk = 0; blk < 3; blk++) {
        hipLaunchKernelGGL(k_ph_attn, dim3(qtiles), dim3(FPH_THREADS), 0, s, a);
        if (blk < 2) hipLaunchKernelGGL(k_ph_block<false>, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_BLOCK, s, a, blk, xin[blk], xout[blk]);
        else hipLaunchKernelGGL(k_ph_block<true>, dim3(tiles), dim3(FPH_THREADS), FPH_LDS_LAST, s, a, blk, xin[blk], xout[blk]);
    }
    if (value_dev) hipLaunchKernelGGL(k_ph_value, dim3(n_envs), dim3(64), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fl_set_error("fl_policy_head: launch failed: %s", hipGetErrorString(e)); return FL_ERR_HIP; }
    return FL_OK;
}
