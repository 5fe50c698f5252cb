// fl_tree_lstm_bwd.h -- the gradient of fl_tree_lstm.h's forward (autograd through solution/nn/TreeLSTM.py:33-154) for a whole
// batch of trees, one launch (gfx950): everything that depends on the tree order.  Included by fl_tree_lstm.hip, which holds its
// entry points fl_tree_lstm_backward / fl_tree_lstm_backward_workspace_bytes (include/flatland_train.h).
//
// Given h and c of every node (the forward's roots_only = 0 outputs) and Gh, the caller's gradient on h, per node of height n,
// with t = tanh(c) and Gh / Gc including what the node's parents hand down:
//   dc = Gc + Gh*o*(1 - t^2);  da_o = Gh*t*o*(1 - o);  da_i = dc*u*i*(1 - i);  da_u = dc*i*(1 - u^2)
//   n > 0:  dq = W_c^T dc;  dg_j = dq_j*c_kj*f_j*(1 - f_j);  Gc_kj += dq_j*f_j;  Gh_kj += (U_iou^T da)[block j] + U_f^T dg_j
// A child that read as zero in the forward (height not below the parent's, padding, the parent itself) receives nothing.
//
// Kernel: one workgroup (4 waves) per group of G consecutive trees, the forward's set-up (fl_tree_lstm.h's ftl_setup_tree and
// ftl_bucket: checks, status word, child table, nodes bucketed by height), then the levels top-down in tiles of 32 nodes.  Per
// tile the gates are recomputed from x and the children's saved h / c by the forward's own functions (ftl_stage, ftl_pre_iou,
// ftl_wfx, ftl_ufh, ftl_pre_f: one copy of the order of every sum, so i, o, u, f_j are the forward's bit for bit;
// c itself is read, not recomputed), then dc, da, dg_j, and the three transposed products as f32-input MFMA
// (v_mfma_f32_32x32x2_f32) with the tile's dc / da / dg_j staged in LDS over the consumed input tile: wave w takes columns
// 32w .. 32w+31 of each child slot, which are the hidden units whose f_j it holds in registers.  The weights are read in torch's
// [out][in] layout: a transposed product walks a weight's rows, a half-wave loads 128 contiguous bytes of one row a step.
//
// Determinism: no float atomics, one writer per address.  A parent writes what it hands to the child of its slot j into a slot
// of its OWN (workspace: hand-down of Gh and of Gc, [T*N][3][128] each); the set-up builds, per node, the list of (parent, slot)
// that name it, in increasing (parent id, slot), and the node sums them in that order when its level comes up -- a child shared
// by several edges gets the sum, as autograd gives it.  Which tile a node lands in does not matter: MFMA rows are independent.
//
// The kernel writes no parameter gradient.  Per node it leaves what the batch-wide products need: da [384], dc [128],
// dg_1..3 [3][128], q = [f_j*c_kj] [384], the three children's global node ids (-1 = read as zero); rows of padding nodes are
// zero (ids -1), dg and q of height-0 nodes too.
#pragma once
#include "fl_tree_lstm.h"

struct FtbArgs : FtlTrees {
    const float *h, *c;             // of every node, [T*N][M]
    const float *grad_h;            // [T*N][M], roots_only: [T][M]
    float *da, *dc, *dg, *q;        // [T*N][3M], [T*N][M], [T*N][3][M], [T*N][3M]
    int *child;                     // [T*N][3]
    float *ghc, *gcc;               // workspace: what (node, slot j) hands to its child's Gh / Gc, [T*N][3][M] each
};

// acc_j += A[row][k] * W[k][cj + col] over k in [0, K), K a multiple of 32: the transposed product (W row-major, ld floats a row)
template <int K>
__device__ __forceinline__ void ftb_gemm3t(const float *arow, const float *w, int ld, int c0, int c1, int c2, fl_f32x16 &a0,
                                           fl_f32x16 &a1, fl_f32x16 &a2, int hh) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 32) {
        float a[16];
        const int o = kc + 16 * hh;
        fl_ld16(arow + o, a);
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const float *wr = w + (size_t)(o + s) * ld;
            a0 = fl_mfma(a[s], wr[c0], a0);
            a1 = fl_mfma(a[s], wr[c1], a1);
            a2 = fl_mfma(a[s], wr[c2], a2);
        }
    }
}

template <int K>
__device__ __forceinline__ void ftb_gemm1t(const float *arow, const float *w, int ld, int c0, fl_f32x16 &a0, int hh) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 32) {
        float a[16];
        const int o = kc + 16 * hh;
        fl_ld16(arow + o, a);
#pragma unroll
        for (int s = 0; s < 16; s++) a0 = fl_mfma(a[s], w[(size_t)(o + s) * ld + c0], a0);
    }
}

__global__ void __launch_bounds__(FTL_THREADS) k_tree_lstm_bwd(FtbArgs p) {
    __shared__ __attribute__((aligned(16))) float s_x[FTL_ROWS * FTL_STRIDE];
    __shared__ FtlSetup s;                                   // (child: -1 = none or read as zero)
    __shared__ int s_top;
    __shared__ short s_pbeg[FTL_MAX_G * FTL_MAX_N];          // node -> its first entry of s_plist, and how many
    __shared__ short s_pnum[FTL_MAX_G * FTL_MAX_N];
    __shared__ short s_plist[FTL_MAX_G * FTL_MAX_N];         // (group-local parent) * 3 + slot of every edge that names the node
    __shared__ int s_rowg[FTL_ROWS], s_rown[FTL_ROWS], s_rowch[FTL_ROWS][3];   // tile row -> global id, group-local id, children

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, M = FTL_M;
    const int t0 = blockIdx.x * p.G;
    const int G = min(p.G, p.T - t0);

    // ---- set-up: one wave per tree (the forward's, then the children that read as zero are dropped and the parent lists built)
    ftl_setup_clear(s, G, N, tid);
    for (int tb = 0; tb < G; tb += 4) {
        const int tl = tb + wave;
        const bool act = tl < G;
        const int lv = ftl_setup_tree(p, s, t0, G, tl, lane, wave);
        // a child whose height is not below its parent's, or a padding child, read as zero: it gets nothing
        if (act && lane < N) {
            for (int j = 0; j < 3; j++) {
                const int ch = s.child[(tl * N + lane) * 3 + j];
                if (ch >= 0 && !ftl_child_read(s.lvl[tl * N + ch], lv)) s.child[(tl * N + lane) * 3 + j] = -1;
            }
        }
        __syncthreads();
        // the (parent, slot) entries that name node `lane`, in increasing (parent, slot): count, place by a prefix sum over the wave
        // (a tree has at most N - 1 entries: an edge fills at most one slot), fill
        int named = 0;
        if (act && lane < N)
            for (int e = 0; e < 3 * N; e++) named += s.child[tl * N * 3 + e] == lane;
        int incl = named;
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (act && lane < N) {
            const int beg = tl * N + incl - named;
            s_pbeg[tl * N + lane] = (short)beg;
            s_pnum[tl * N + lane] = (short)named;
            int k = 0;
            for (int e = 0; e < 3 * N; e++)
                if (s.child[tl * N * 3 + e] == lane) s_plist[beg + k++] = (short)(tl * N * 3 + e);
        }
        __syncthreads();
    }
    ftl_bucket(s, s_top, G, N, tid);
    // rows the level loop does not write: everything of a padding node, dg / q / children of a height-0 node
    {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const size_t g0 = (size_t)t0 * N;
        for (int i = tid; i < G * N * (3 * M / 4); i += FTL_THREADS) {
            const int node = i / (3 * M / 4), q = i % (3 * M / 4), lv = s.lvl[node];
            if (lv < 0) ((float4 *)p.da)[(g0 + node) * (3 * M / 4) + q] = z;
            if (lv <= 0) {
                ((float4 *)p.dg)[(g0 + node) * (3 * M / 4) + q] = z;
                ((float4 *)p.q)[(g0 + node) * (3 * M / 4) + q] = z;
            }
        }
        for (int i = tid; i < G * N * (M / 4); i += FTL_THREADS) {
            const int node = i / (M / 4), q = i % (M / 4);
            if (s.lvl[node] < 0) ((float4 *)p.dc)[(g0 + node) * (M / 4) + q] = z;
        }
        for (int i = tid; i < G * N * 3; i += FTL_THREADS)
            if (s.lvl[i / 3] <= 0) p.child[g0 * 3 + i] = -1;
    }
    __syncthreads();

    // ---- levels, top-down
    const int col = lane & 31, hh = lane >> 5, j0 = 32 * wave, cx = j0 + col;
    const size_t slot0 = (size_t)t0 * N * 3;                    // (group-local node) * 3 + slot -> its row of ghc / gcc
    for (int n = s_top; n >= 0; n--) {
        const int cnt = s.cnt[n], off = s.off[n];
        for (int r0 = 0; r0 < cnt; r0 += FTL_ROWS) {
            const int rows = min(FTL_ROWS, cnt - r0);
            if (tid < FTL_ROWS) {
                int g = -1, node = 0, cs[3] = {-1, -1, -1};
                if (tid < rows) {
                    node = s.list[off + r0 + tid];
                    const int tl = node / N;
                    g = (t0 + tl) * N + node % N;
                    if (n > 0) {
                        for (int j = 0; j < 3; j++) {
                            const int ch = s.child[node * 3 + j];
                            cs[j] = ch >= 0 ? (t0 + tl) * N + ch : -1;
                            p.child[(size_t)g * 3 + j] = cs[j];
                        }
                    }
                }
                s_rowg[tid] = g;
                s_rown[tid] = node;
                s_rowch[tid][0] = cs[0]; s_rowch[tid][1] = cs[1]; s_rowch[tid][2] = cs[2];
            }
            __syncthreads();
            ftl_stage(s_x, s_rowg, s_rowch, p.forest, p.h, n, tid);
            __syncthreads();

            const float *arow = &s_x[col * FTL_STRIDE];
            // i, o, u by the forward's function, then the bias as the forward adds it
            fl_f32x16 ai, ao, au;
            ftl_pre_iou(p, arow, n, j0, M + j0, 2 * M + j0, col, hh, ai, ao, au);
            const float bi = p.b_iou[cx], bo = p.b_iou[M + cx], bu = p.b_iou[2 * M + cx];
            float dai[16], dao[16], dau[16], dcc[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, hh);
                dai[r] = dao[r] = dau[r] = dcc[r] = 0.f;
                if (row < rows) {
                    const int g = s_rowg[row], node = s_rown[row];
                    float gh = p.roots_only ? (g % N == 0 ? p.grad_h[(size_t)(g / N) * M + cx] : 0.f) : p.grad_h[(size_t)g * M + cx];
                    float gc = 0.f;
                    const int beg = s_pbeg[node], num = s_pnum[node];
                    for (int k = 0; k < num; k++) {
                        const size_t at = (slot0 + s_plist[beg + k]) * M + cx;
                        gh += p.ghc[at];
                        gc += p.gcc[at];
                    }
                    const float ig = ftl_sigmoid(ai[r] + bi), og = ftl_sigmoid(ao[r] + bo), ug = tanhf(au[r] + bu);
                    const float t = tanhf(p.c[(size_t)g * M + cx]);
                    const float dc = gc + gh * og * (1.f - t * t);
                    dcc[r] = dc;
                    dao[r] = gh * t * og * (1.f - og);
                    dai[r] = dc * ug * ig * (1.f - ig);
                    dau[r] = dc * ig * (1.f - ug * ug);
                    p.dc[(size_t)g * M + cx] = dc;
                    p.da[(size_t)g * 3 * M + cx] = dai[r];
                    p.da[(size_t)g * 3 * M + M + cx] = dao[r];
                    p.da[(size_t)g * 3 * M + 2 * M + cx] = dau[r];
                }
            }
            if (n > 0) {
                // f_j by the forward's functions; q = f_j * c_kj goes out
                const fl_f32x16 wfx = ftl_wfx(p, arow, j0, col, hh);
                const float bf = p.b_f[cx];
                float fj[3][16];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const fl_f32x16 af = ftl_ufh(p, arow, j, j0, col, hh);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = fl_acc_row(r, hh);
                        fj[j][r] = ftl_sigmoid(ftl_pre_f(af[r], wfx[r], bf));
                        if (row < rows) {
                            const int ch = s_rowch[row][j];
                            const float cv = ch >= 0 ? p.c[(size_t)ch * M + cx] : 0.f;
                            p.q[(size_t)s_rowg[row] * 3 * M + j * M + cx] = fj[j][r] * cv;
                        }
                    }
                }
                __syncthreads();                                // every wave is done with the staged tile
#pragma unroll
                for (int r = 0; r < 16; r++) s_x[fl_acc_row(r, hh) * FTL_STRIDE + cx] = dcc[r];
                __syncthreads();
                // dq = W_c^T dc, columns j * M + cx: the units of f_j in this lane's registers
                fl_f32x16 q0 = {}, q1 = {}, q2 = {};
                ftb_gemm3t<FTL_M>(arow, p.w_c, 3 * M, cx, M + cx, 2 * M + cx, q0, q1, q2, hh);
                float dgj[3][16];
#pragma unroll
                for (int j = 0; j < 3; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = fl_acc_row(r, hh);
                        const float dq = j == 0 ? q0[r] : j == 1 ? q1[r] : q2[r];
                        dgj[j][r] = 0.f;
                        if (row < rows) {
                            const int g = s_rowg[row], ch = s_rowch[row][j];
                            const float cv = ch >= 0 ? p.c[(size_t)ch * M + cx] : 0.f;
                            const float f = fj[j][r];
                            dgj[j][r] = dq * cv * f * (1.f - f);
                            p.dg[(size_t)g * 3 * M + j * M + cx] = dgj[j][r];
                            p.gcc[((size_t)g * 3 + j) * M + cx] = dq * f;
                        }
                    }
                __syncthreads();                                // every wave is done with dc in LDS
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = fl_acc_row(r, hh);
                    s_x[row * FTL_STRIDE + cx] = dai[r];
                    s_x[row * FTL_STRIDE + M + cx] = dao[r];
                    s_x[row * FTL_STRIDE + 2 * M + cx] = dau[r];
                }
                __syncthreads();
                // what slot j hands to its child's Gh: (U_iou^T da)[j * M + cx] + (U_f^T dg_j)[cx]
                fl_f32x16 g0 = {}, g1 = {}, g2 = {};
                ftb_gemm3t<3 * FTL_M>(arow, p.u_iou, 3 * M, cx, M + cx, 2 * M + cx, g0, g1, g2, hh);
                __syncthreads();                                // every wave is done with da in LDS
#pragma unroll
                for (int j = 0; j < 3; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) s_x[fl_acc_row(r, hh) * FTL_STRIDE + j * M + cx] = dgj[j][r];
                __syncthreads();
                ftb_gemm1t<FTL_M>(arow, p.u_f, M, cx, g0, hh);
                ftb_gemm1t<FTL_M>(arow + M, p.u_f, M, cx, g1, hh);
                ftb_gemm1t<FTL_M>(arow + 2 * M, p.u_f, M, cx, g2, hh);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = fl_acc_row(r, hh);
                    if (row < rows) {
                        const size_t at = (size_t)s_rowg[row] * 3 * M + cx;
                        p.ghc[at] = g0[r];
                        p.ghc[at + M] = g1[r];
                        p.ghc[at + 2 * M] = g2[r];
                    }
                }
            }
            __syncthreads();                                    // the tile's hand-downs are visible; the LDS tile is free again
        }
    }
}

static inline void fl_launch_tree_lstm_bwd(const FtbArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_lstm_bwd, dim3((a.T + a.G - 1) / a.G), dim3(FTL_THREADS), 0, s, a);
}
