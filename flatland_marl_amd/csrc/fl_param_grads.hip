// fl_param_grads.hip -- entry points of include/flatland_param_grads.h: the checks (all before any HIP call), the problem tables
// of the head's 19 and the encoder's 5 weight matrices and the launches of the kernels in fl_param_grads.h.
#include "../../include/flatland_param_grads.h"
#include "fl_param_grads.h"
#include "fl_policy_host.h"

static_assert(FL_PARAM_GRADS_MAX_SLICES == FPG_MAX_SLICES && FL_PARAM_GRADS_BLOCK == FPG_BLOCK, "the header's constants are the kernel's");

#define FPG_HEAD_AUTO 2          // slices = 0: at most this many for the head (106 tiles) ...
#define FPG_TREE_AUTO 15         // ... and for the encoder (17 tiles): at most 256 workgroups, one a compute unit (the kernel's registers)
                                 // (FPG_HEAD_DOUBLES, FPG_TREE_DOUBLES, the float64 partials of a slice: fl_policy_layout.h)

// a table under construction: problems in launch order, tiles and workspace offsets counted as they are added
struct FpgTable {
    FpgArgs a;
    int tiles;
    long long doubles;
    FpgTable() : tiles(0), doubles(0) { a.n = 0; }
    FpgProblem &add(int rows, const float *dz, int ldz, int P, const float *x0, int ldx0, int w0, float *out, float *bias) {
        FpgProblem &p = a.pr[a.n++];
        p.dz = dz; p.x0 = x0; p.x1 = nullptr; p.idx = nullptr; p.order = nullptr; p.out = out; p.bias = bias;
        p.rows = rows; p.ldz = ldz; p.P = P; p.terms = 1; p.term_stride = 0;
        p.ldx0 = ldx0; p.w0 = w0; p.ldx1 = 0; p.w1 = 0;
        p.idx_ld = 0; p.idx_rows = 0; p.x_min = FPG_NO_ORDER; p.b_min = FPG_NO_ORDER;
        p.ldo = w0;
        return p;
    }
    // after a problem's fields are final
    void place(FpgProblem &p) {
        const int Q = p.w0 + p.w1;
        p.tiles_q = (Q + FPG_TILE - 1) / FPG_TILE;
        p.tile0 = tiles;
        tiles += p.tiles_q * ((p.P + FPG_TILE - 1) / FPG_TILE);
        p.ws_off = doubles;
        doubles += (long long)p.P * (Q + (p.bias ? 1 : 0));
    }
    void second(FpgProblem &p, const float *x1, int ldx1, int w1) { p.x1 = x1; p.ldx1 = ldx1; p.w1 = w1; p.ldo = p.w0 + w1; }
};

static int fpg_slices(int n_rows, int slices, int automatic) {
    if (slices != 0) return slices;
    const int blocks = (n_rows + FPG_BLOCK - 1) / FPG_BLOCK;
    return blocks < automatic ? (blocks < 1 ? 1 : blocks) : automatic;
}

static size_t fpg_workspace_bytes(int n_rows, int slices, int automatic, long long doubles) {
    if (n_rows <= 0 || slices < 0 || slices > FPG_MAX_SLICES) return 0;
    const int s = fpg_slices(n_rows, slices, automatic);
    return s == 1 ? 0 : (size_t)s * doubles * sizeof(double);
}

size_t fl_policy_head_param_grads_workspace_bytes(int n_rows, int slices) {
    return fpg_workspace_bytes(n_rows, slices, FPG_HEAD_AUTO, FPG_HEAD_DOUBLES);
}

size_t fl_tree_lstm_param_grads_workspace_bytes(int n_rows, int slices) {
    return fpg_workspace_bytes(n_rows, slices, FPG_TREE_AUTO, FPG_TREE_DOUBLES);
}

// slices, grads and the workspace of both entry points; on[i]: gradient i is written
static int fpg_check_common(const char *fn, int slices, float *const *grads, const bool *on, int n_grads, void *workspace_dev,
                            size_t workspace_bytes, size_t need, const char *sizer) {
    if (slices < 0 || slices > FPG_MAX_SLICES) {
        fl_set_error("%s: slices must be 0 (automatic) or in [1, %d], got %d", fn, FPG_MAX_SLICES, slices);
        return FL_ERR_ARG;
    }
    if (!grads) { fl_set_error("%s: grads is NULL", fn); return FL_ERR_ARG; }
    for (int i = 0; i < n_grads; i++) {
        if (!on[i]) continue;
        char name[32];
        snprintf(name, sizeof name, "gradient %d", i);
        const FlPtr t = {grads[i], name, 16};
        if (fl_check_ptrs(fn, &t, 1) != FL_OK) return FL_ERR_ARG;
    }
    const FlPtr ws = {workspace_dev, "workspace", 16, need == 0};
    if (fl_check_ptrs(fn, &ws, 1) != FL_OK || fl_check_bytes(fn, "workspace", workspace_bytes, need, sizer) != FL_OK) return FL_ERR_ARG;
    return FL_OK;
}

static int fpg_launch(const char *fn, FpgTable &tb, int slices, void *workspace_dev, hipStream_t s) {
    tb.a.slices = slices;
    tb.a.ws_stride = tb.doubles;
    tb.a.ws = (double *)workspace_dev;
    hipLaunchKernelGGL(k_param_grads, dim3(tb.tiles, slices), dim3(FPG_THREADS), 0, s, tb.a);
    if (slices > 1) hipLaunchKernelGGL(k_param_grads_reduce, dim3(32, tb.a.n), dim3(FPG_THREADS), 0, s, tb.a);
    return fl_launched(fn);
}

// the head's 19 gradient problems in launch order (include/flatland_policy_train.h): dW of parameter `param` = sum over the rows of
// dZ^T [X0 | X1] and db of parameter `param` + 1 = sum dZ, where dZ is array dz of the rows and an X is attr, a saved array or an
// array of the rows.  padded: dZ's rows are wider than the layer (the last layers' 5 / 1 columns in rows of 8 / 4 floats)
struct FpgX { enum { NONE, ATTR, SAVED, ROWS } from; int k; };
struct FpgHeadProblem { int param, dz; FpgX x0, x1; bool padded; };
#define S(k) {FpgX::SAVED, FPL_S_##k}
#define R(k) {FpgX::ROWS, FPL_R_##k}
static constexpr FpgHeadProblem FPG_HEAD[19] = {
    {0, FPL_R_ATTR_DZ0, {FpgX::ATTR}}, {2, FPL_R_ATTR_DZ2, R(ATTR_H1)}, {4, FPL_R_ATTR_DZ4, R(ATTR_H2)}, {6, FPL_R_ATTR_DZ6, R(ATTR_H3)},
    {8, FPL_R_DQKV0, S(EMB)}, {10, FPL_R_DO0, S(C0)}, {12, FPL_R_DZ0, S(EMB), R(O0)},
    {14, FPL_R_DQKV1, S(Y1)}, {16, FPL_R_DO1, S(C1)}, {18, FPL_R_DZ1, S(Y1), R(O1)},
    {20, FPL_R_DQKV2, S(Y2)}, {22, FPL_R_DO2, S(C2)}, {24, FPL_R_DZ2, S(Y2), R(O2)},
    {26, FPL_R_ACTOR_DZ0, S(EMB), S(Y3)}, {28, FPL_R_ACTOR_DZ2, R(ACTOR_U1)}, {30, FPL_R_ACTOR_DZ4, R(ACTOR_U2), {}, true},
    {32, FPL_R_CRITIC_DZ0, S(EMB), S(Y3)}, {34, FPL_R_CRITIC_DZ2, R(CRITIC_U1)}, {36, FPL_R_CRITIC_DZ4, R(CRITIC_U2), {}, true},
};
#undef R
#undef S
constexpr int fpg_width(FpgX x) {
    return x.from == FpgX::ATTR ? FPH_ATTR : x.from == FpgX::SAVED ? FPL_SAVED[x.k].floats : x.from == FpgX::ROWS ? FPL_ROWS[x.k].floats : 0;
}
// every matrix once, in the parameters' order; [X0 | X1] as wide as the matrix; dZ as wide as the layer, or padded and said so
constexpr bool fpg_head_fits() {
    for (int n = 0; n < 19; n++) {
        const FpgHeadProblem &h = FPG_HEAD[n];
        const int out = FPL_PARAMS[h.param].out, ldz = FPL_ROWS[h.dz].floats;
        if (h.param != 2 * n || fpg_width(h.x0) + fpg_width(h.x1) != FPL_PARAMS[h.param].in || (h.padded ? ldz <= out : ldz != out)) return false;
    }
    return true;
}
static_assert(fpg_head_fits(), "the problems' arrays have the parameters' shapes");

int fl_policy_head_param_grads(int n_envs, int n_agents, const float *attr_dev, const void *saved_dev, const void *rows_dev,
                               int actor, int critic, float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes,
                               void *hip_stream) {
    const char *fn = "fl_policy_head_param_grads";
    if (fph_check_sizes(fn, n_envs, n_agents) != FL_OK) return FL_ERR_ARG;
    if ((actor != 0 && actor != 1) || (critic != 0 && critic != 1)) {
        fl_set_error("%s: actor and critic must be 0 or 1, got %d, %d", fn, actor, critic);
        return FL_ERR_ARG;
    }
    if (!actor && !critic) { fl_set_error("%s: actor and critic are both 0", fn); return FL_ERR_ARG; }
    const FlPtr tab[] = {{attr_dev, "attr", 16}, {saved_dev, "saved", 16}, {rows_dev, "rows", 16}};
    if (fl_check_ptrs(fn, tab, 3) != FL_OK) return FL_ERR_ARG;
    const int R = n_envs * n_agents;
    bool on[FPH_NPARAMS];
    for (int i = 0; i < FPH_NPARAMS; i++) on[i] = i < 26 || (i < 32 ? actor : critic);
    if (fpg_check_common(fn, slices, grads, on, FPH_NPARAMS, workspace_dev, workspace_bytes,
                         fl_policy_head_param_grads_workspace_bytes(R, slices), "fl_policy_head_param_grads_workspace_bytes") != FL_OK)
        return FL_ERR_ARG;

    FpgTable tb;
    const auto at = [&](FpgX x) -> const float * {
        return x.from == FpgX::ATTR ? attr_dev : x.from == FpgX::SAVED ? fpl_saved((const float *)saved_dev, (size_t)R, x.k)
                                                                       : fpl_rows((const float *)rows_dev, (size_t)R, x.k);
    };
    for (const FpgHeadProblem &h : FPG_HEAD) {
        if (!on[h.param]) continue;
        const FpgX dz = {FpgX::ROWS, h.dz};
        FpgProblem &p = tb.add(R, at(dz), fpg_width(dz), FPL_PARAMS[h.param].out, at(h.x0), fpg_width(h.x0), fpg_width(h.x0), grads[h.param],
                               grads[h.param + 1]);
        if (h.x1.from != FpgX::NONE) tb.second(p, at(h.x1), fpg_width(h.x1), fpg_width(h.x1));
        tb.place(p);
    }
    return fpg_launch(fn, tb, fpg_slices(R, slices, FPG_HEAD_AUTO), workspace_dev, (hipStream_t)hip_stream);
}

int fl_tree_lstm_param_grads(int n_rows, const float *x_dev, const int64_t *node_order_dev, const float *h_dev, const float *da_dev,
                             const float *dc_dev, const float *dg_dev, const float *q_dev, const int32_t *child_dev,
                             float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_tree_lstm_param_grads";
    constexpr int M = FTL_M, IN = FTL_F;
    if (n_rows <= 0 || n_rows > INT32_MAX / (3 * M)) {
        fl_set_error("%s: bad size (n_rows %d; 1 <= n_rows <= %d)", fn, n_rows, INT32_MAX / (3 * M));
        return FL_ERR_ARG;
    }
    const FlPtr tab[] = {{x_dev, "x", 16}, {node_order_dev, "node_order", 8}, {h_dev, "h", 16}, {da_dev, "da", 16}, {dc_dev, "dc", 16},
                         {dg_dev, "dg", 16}, {q_dev, "q", 16}, {child_dev, "child", 4}};
    if (fl_check_ptrs(fn, tab, 8) != FL_OK) return FL_ERR_ARG;
    const bool on[8] = {true, true, true, true, true, true, true, true};
    if (fpg_check_common(fn, slices, grads, on, 8, workspace_dev, workspace_bytes,
                         fl_tree_lstm_param_grads_workspace_bytes(n_rows, slices), "fl_tree_lstm_param_grads_workspace_bytes") != FL_OK)
        return FL_ERR_ARG;

    FpgTable tb;
    FpgProblem &wiou = tb.add(n_rows, da_dev, 3 * M, 3 * M, x_dev, IN, IN, grads[0], grads[1]);
    wiou.order = node_order_dev; wiou.x_min = 0;
    tb.place(wiou);
    for (int j = 0; j < 3; j++) {                      // dU_iou's columns of child j
        FpgProblem &u = tb.add(n_rows, da_dev, 3 * M, 3 * M, h_dev, M, M, grads[2] + j * M, nullptr);
        u.idx = child_dev + j; u.idx_ld = 3; u.idx_rows = n_rows; u.ldo = 3 * M;
        tb.place(u);
    }
    FpgProblem &wc = tb.add(n_rows, dc_dev, M, M, q_dev, 3 * M, 3 * M, grads[3], grads[4]);
    wc.order = node_order_dev; wc.b_min = 1;
    tb.place(wc);
    FpgProblem &wf = tb.add(n_rows, dg_dev, 3 * M, M, x_dev, IN, IN, grads[5], grads[6]);
    wf.terms = 3; wf.term_stride = M; wf.order = node_order_dev; wf.x_min = 0;
    tb.place(wf);
    FpgProblem &uf = tb.add(3 * n_rows, dg_dev, M, M, h_dev, M, M, grads[7], nullptr);       // the rows are the pairs (node, child slot)
    uf.idx = child_dev; uf.idx_ld = 1; uf.idx_rows = n_rows;
    tb.place(uf);
    return fpg_launch(fn, tb, fpg_slices(n_rows, slices, FPG_TREE_AUTO), workspace_dev, (hipStream_t)hip_stream);
}
