// fl_param_grads.hip -- entry points of include/flatland_param_grads.h: the checks (all before any HIP call), the problem tables
// of the head's 19 and the encoder's 5 weight matrices and the launches of the kernels in fl_param_grads.h.
#include "../../include/flatland_param_grads.h"
#include "fl_param_grads.h"
#include "fl_policy_host.h"

// the head's sizes (fl_policy_head.h; that header's kernels belong to another unit)
#define FPH_ATTR 83
#define FPH_H 128
#define FPH_E 256
#define FPH_ACT 5
#define FPH_NPARAMS 38
#define FPH_MAX_A 1024

static_assert(FL_PARAM_GRADS_MAX_SLICES == FPG_MAX_SLICES && FL_PARAM_GRADS_BLOCK == FPG_BLOCK, "the header's constants are the kernel's");

#define FPG_HEAD_AUTO 2          // slices = 0: at most this many for the head (106 tiles) ...
#define FPG_TREE_AUTO 15         // ... and for the encoder (17 tiles): at most 256 workgroups, one a compute unit (the kernel's registers)
#define FPG_HEAD_DOUBLES 1698694 // the float64 partials of a slice: sum of P * (Q + 1) over the head's matrices
#define FPG_TREE_DOUBLES 219776  // ... over the encoder's

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

int fl_policy_head_param_grads(int n_envs, int n_agents, const float *attr_dev, const void *saved_dev, const void *rows_dev,
                               int actor, int critic, float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes,
                               void *hip_stream) {
    const char *fn = "fl_policy_head_param_grads";
    if (n_envs <= 0 || n_agents < 1 || n_agents > FPH_MAX_A || (long long)n_envs * n_agents > INT32_MAX / (3 * FPH_E)) {
        fl_set_error("%s: bad sizes (n_envs %d, n_agents %d; 1 <= n_envs, 1 <= n_agents <= %d)", fn, n_envs, n_agents, FPH_MAX_A);
        return FL_ERR_ARG;
    }
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

    const size_t Rs = (size_t)R;
    const float *sv = (const float *)saved_dev, *rw = (const float *)rows_dev;
    const float *y[4], *c[3];
    for (int i = 0; i < 4; i++) y[i] = sv + i * Rs * FPH_E;
    for (int i = 0; i < 3; i++) c[i] = sv + (4 + i) * Rs * FPH_E;
    const auto take = [&](size_t n) { const float *q = rw; rw += Rs * n; return q; };      // the order of include/flatland_policy_train.h
    const float *a_dz[4], *a_h[3];
    for (int i = 0; i < 3; i++) a_dz[i] = take(FPH_E);
    a_dz[3] = take(FPH_H);
    for (int i = 0; i < 3; i++) a_h[i] = take(FPH_E);

    FpgTable tb;
    const float *a_x[4] = {attr_dev, a_h[0], a_h[1], a_h[2]};
    for (int i = 0; i < 4; i++)
        tb.place(tb.add(R, a_dz[i], i < 3 ? FPH_E : FPH_H, i < 3 ? FPH_E : FPH_H, a_x[i], i ? FPH_E : FPH_ATTR, i ? FPH_E : FPH_ATTR,
                        grads[2 * i], grads[2 * i + 1]));
    for (int i = 0; i < 3; i++) {
        const float *dqkv = take(3 * FPH_E), *dout = take(FPH_E), *dz = take(FPH_E), *o = take(FPH_E);
        take(FPH_E); take(FPH_E);                                                          // (dc_i, dy_i)
        float *const *g = grads + 8 + 6 * i;
        tb.place(tb.add(R, dqkv, 3 * FPH_E, 3 * FPH_E, y[i], FPH_E, FPH_E, g[0], g[1]));
        tb.place(tb.add(R, dout, FPH_E, FPH_E, c[i], FPH_E, FPH_E, g[2], g[3]));
        FpgProblem &m = tb.add(R, dz, FPH_E, FPH_E, y[i], FPH_E, FPH_E, g[4], g[5]);
        tb.second(m, o, FPH_E, FPH_E);
        tb.place(m);
    }
    take(FPH_E);                                                                           // (dy_3)
    for (int hd = 0; hd < 2; hd++) {
        const int last = hd ? 1 : FPH_ACT, last_ld = hd ? 4 : 8;
        const float *dz0 = take(FPH_E), *dz2 = take(FPH_H), *dz4 = take(last_ld), *u1 = take(FPH_E), *u2 = take(FPH_H);
        if (!(hd ? critic : actor)) continue;
        float *const *g = grads + 26 + 6 * hd;
        FpgProblem &m = tb.add(R, dz0, FPH_E, FPH_E, y[0], FPH_E, FPH_E, g[0], g[1]);
        tb.second(m, y[3], FPH_E, FPH_E);
        tb.place(m);
        tb.place(tb.add(R, dz2, FPH_H, FPH_H, u1, FPH_E, FPH_E, g[2], g[3]));
        tb.place(tb.add(R, dz4, last_ld, last, u2, FPH_H, FPH_H, g[4], g[5]));
    }
    return fpg_launch(fn, tb, fpg_slices(R, slices, FPG_HEAD_AUTO), workspace_dev, (hipStream_t)hip_stream);
}

int fl_tree_lstm_param_grads(int n_rows, const float *x_dev, const int64_t *node_order_dev, const float *h_dev, const float *da_dev,
                             const float *dc_dev, const float *dg_dev, const float *q_dev, const int32_t *child_dev,
                             float *const *grads, int slices, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "fl_tree_lstm_param_grads";
    constexpr int M = 128, IN = 12;
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
