// fl_tree_lstm.h -- the policy's TreeLSTM forward (solution/nn/TreeLSTM.py:33-154) for a whole batch of trees, one launch
// (gfx950).  Included by fl_tree_lstm.hip, which holds its entry points fl_tree_lstm / fl_tree_lstm_workspace_bytes.  The set-up,
// the staging and the gate pre-activations are functions that the gradient's kernel (fl_tree_lstm_bwd.h) calls as well: both
// kernels accept the same trees and see the same gates because there is one copy of that code.
//
// Per tree t (nodes t*N .. t*N+N-1, node_order = height, -2 = padding), hidden size M = 128, in-features F = 12:
//   leaf (height 0)    iou = W_iou x + b_iou;  c = i*u;  h = o*tanh(c)        (i, o = sigmoid, u = tanh of the three thirds)
//   height n > 0       children k1..k3 = the children of the node's three edges, in edge-list order
//                      iou = W_iou x + b_iou + U_iou [h_k1 | h_k2 | h_k3];  f_j = sigmoid(W_f x + b_f + U_f h_kj)
//                      c = i*u + W_c [f_1*c_k1 | f_2*c_k2 | f_3*c_k3] + b_c;  h = o*tanh(c)
//   padding            h = c = 0
// A child whose height is not below its parent's (or a padding child) reads as 0: the reference gathers a level's children before
// it writes the level, from zero-initialised h / c.
//
// Kernel: one workgroup (4 waves) per group of G consecutive trees, no grid-wide synchronisation.  Set-up: one wave per tree
// checks it (indices inside the tree, edge_order = the parent's node_order, every node of height n > 0 the parent of the n-th
// level's edge triple of its own rank, node_order in {-2} u [0, N-1]; a violating tree adds 1 to the status word), fills the
// group's child table and buckets the group's nodes by height.  Then level by level, in tiles of 32 nodes: [x | h_k1 | h_k2 | h_k3]
// is staged in LDS (row stride 420 floats, = 4 mod 32: the 16 lanes of a ds_read_b128 phase hit distinct banks), and wave w
// computes hidden units 32w .. 32w+31 of the tile with f32-input MFMA (v_mfma_f32_32x32x2_f32, exact f32): i, o, u over
// K = 384 + 12 (U h from zero, then W x: see ftl_pre_iou), W_f x once and U_f h_kj for the three children, then f_j * c_kj
// goes to LDS (over the staged tile) and W_c runs over K = 384.  A wave's three iou accumulators hold the same hidden units, so the epilogue is in registers.  Weights are read
// in torch's [out][in] layout straight from global memory (L2): lane l of an MFMA step takes k = kc + 16 * (l >> 5) + s of
// chunk kc, so every lane loads 64 contiguous bytes of one weight row a chunk.  h and c of every node go to the output buffers
// or the workspace; the next level of the same workgroup reads them back after a barrier (workgroup-scope release / acquire).
#pragma once
#include "fl_internal.h"
#include "fl_mfma.h"
#include "fl_policy_layout.h"       // FTL_F, FTL_M

#define FTL_THREADS 256
#define FTL_ROWS 32                 // nodes a tile (the MFMA's 32 rows)
#define FTL_STRIDE 420              // floats a staged row: 12 + 3 * 128 = 396 used
#define FTL_MAX_G 16                // trees a workgroup
#define FTL_MAX_N 64                // nodes a tree (one lane per node in the set-up)

// what the forward's and the gradient's kernel both take: the forest, its order arrays, the weights, the status word
struct FtlTrees {
    int T, N, G, roots_only;
    const float *forest;
    const long long *adj, *no, *eo;
    const float *w_iou, *b_iou, *u_iou, *w_c, *b_c, *w_f, *b_f, *u_f;
    int *status;
};

struct FtlArgs : FtlTrees {
    float *h_out, *c_out;           // as the caller passed them (c_out may be NULL); roots_only: [T][M]
    float *hbuf, *cbuf;             // h / c of every node, [T*N][M] (the outputs or the workspace)
};

// a group's trees as the set-up leaves them.  The top level (ftl_bucket's s_top) is a word of its own beside it: as the last
// member it would leave the struct 4 bytes past a multiple of 16, and the padding after it would add 12 bytes of LDS a workgroup.
struct FtlSetup {
    short child[FTL_MAX_G * FTL_MAX_N * 3];     // tree-local child of (node, j), -1 = none
    short list[FTL_MAX_G * FTL_MAX_N];          // group-local node ids bucketed by height
    signed char lvl[FTL_MAX_G * FTL_MAX_N];     // height, -2 = padding (or an invalid node_order)
    int tmp[4][3][FTL_MAX_N];                   // per wave: node height, edge height, node rank of the tree in set-up
    int cnt[FTL_MAX_N], off[FTL_MAX_N], fill[FTL_MAX_N];
};

__device__ __forceinline__ float ftl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// acc += A[row][aoff + k] * W[wrow][k] over k in [0, K), K a multiple of 32; A = the staged tile row of this lane, W row-major
template <int K>
__device__ __forceinline__ void ftl_gemm1(const float *arow, const float *w0, fl_f32x16 &acc, int hh) {
#pragma unroll 2
    for (int kc = 0; kc < K; kc += 32) {
        float a[16], b[16];
        fl_ld16(arow + kc + 16 * hh, a);
        fl_ld16(w0 + kc + 16 * hh, b);
#pragma unroll
        for (int s = 0; s < 16; s++) acc = fl_mfma(a[s], b[s], acc);
    }
}

// the same for three weight rows at once (i, o, u of one hidden unit), sharing the A operand
template <int K>
__device__ __forceinline__ void ftl_gemm3(const float *arow, const float *w0, const float *w1, const float *w2, fl_f32x16 &c0,
                                          fl_f32x16 &c1, fl_f32x16 &c2, int hh) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 32) {
        float a[16], b0[16], b1[16], b2[16];
        const int o = kc + 16 * hh;
        fl_ld16(arow + o, a);
        fl_ld16(w0 + o, b0);
        fl_ld16(w1 + o, b1);
        fl_ld16(w2 + o, b2);
#pragma unroll
        for (int s = 0; s < 16; s++) {
            c0 = fl_mfma(a[s], b0[s], c0);
            c1 = fl_mfma(a[s], b1[s], c1);
            c2 = fl_mfma(a[s], b2[s], c2);
        }
    }
}

// the K = 12 products (W x): step s takes k = 2s + (l >> 5)
__device__ __forceinline__ void ftl_wx(const float *xrow, const float *w, int r0, int r1, int r2, int col,
                                       fl_f32x16 &c0, fl_f32x16 &c1, fl_f32x16 &c2, int nmat, int hh) {
#pragma unroll
    for (int s = 0; s < FTL_F / 2; s++) {
        const int k = 2 * s + hh;
        const float a = xrow[k];
        c0 = fl_mfma(a, w[(size_t)(r0 + col) * FTL_F + k], c0);
        if (nmat > 1) {
            c1 = fl_mfma(a, w[(size_t)(r1 + col) * FTL_F + k], c1);
            c2 = fl_mfma(a, w[(size_t)(r2 + col) * FTL_F + k], c2);
        }
    }
}

// ---- shared with the gradient's kernel: the set-up, the staging, the gate pre-activations

// before the set-up loop: no node counted, no child
__device__ __forceinline__ void ftl_setup_clear(FtlSetup &s, int G, int N, int tid) {
    for (int i = tid; i < FTL_MAX_N; i += FTL_THREADS) { s.cnt[i] = 0; s.fill[i] = 0; }
    for (int i = tid; i < G * N * 3; i += FTL_THREADS) s.child[i] = -1;
    __syncthreads();
}

// one iteration of the set-up loop, called by every thread (it has barriers): this wave checks tree tl of the group (tl >= G: none),
// fills its rows of the child table and of lvl and counts its nodes by height; a violating tree adds 1 to the status word.
// Returns the height of node `lane` (-2 = padding, invalid, or no such node).
__device__ __forceinline__ int ftl_setup_tree(const FtlTrees &p, FtlSetup &s, int t0, int G, int tl, int lane, int wave) {
    const int N = p.N, E = N - 1;
    const bool act = tl < G;
    const long long base = (long long)(t0 + tl) * N;
    int lv = -2, el = -2, pl = -1, cl = -1;
    bool bad = false;
    if (act && lane < N) {
        const long long raw = p.no[base + lane];
        if (raw == -2 || (raw >= 0 && raw <= N - 1)) lv = (int)raw;
        else bad = true;
    }
    if (act && lane < E) {
        const size_t e = (size_t)(t0 + tl) * E + lane;
        const long long raw = p.eo[e];
        if (raw != -2) {
            const long long pa = p.adj[e * 3], ch = p.adj[e * 3 + 1];
            if (raw < 0 || raw > N - 1 || pa < base || pa >= base + N || ch < base || ch >= base + N) bad = true;
            else { el = (int)raw; pl = (int)(pa - base); cl = (int)(ch - base); }
        }
    }
    if (act) {
        s.tmp[wave][0][lane] = lv;
        s.tmp[wave][1][lane] = el;
    }
    __syncthreads();
    int rank = 0, nsame = 0, esame = 0, erank = 0;
    if (act) {
        for (int v = 0; v < N; v++) {
            const int o = s.tmp[wave][0][v];
            nsame += o == lv;
            rank += (o == lv) & (v < lane);
        }
        for (int e = 0; e < E; e++) {
            const int o = s.tmp[wave][1][e];
            esame += o == lv;
            erank += (o == el) & (e < lane);
        }
        if (lane < N) s.tmp[wave][2][lane] = rank;
        if (lane < N && lv >= 1 && esame != 3 * nsame) bad = true;
    }
    __syncthreads();
    if (act) {
        if (lane < N) {
            s.lvl[tl * N + lane] = (signed char)lv;
            if (lv >= 0) atomicAdd(&s.cnt[lv], 1);
        }
        if (el >= 0) {
            if (s.tmp[wave][0][pl] != el) bad = true;
            else if (el >= 1) {
                if (s.tmp[wave][2][pl] != erank / 3) bad = true;
                else s.child[(tl * N + pl) * 3 + erank % 3] = (short)cl;
            }
        }
        const unsigned long long anybad = __ballot(bad);
        if (lane == 0 && anybad && p.status) atomicAdd(p.status, 1);
    }
    __syncthreads();
    return lv;
}

// after the set-up loop: the group's nodes bucketed by height (off, list; s_top = the highest level that has a node, -1 = none)
__device__ __forceinline__ void ftl_bucket(FtlSetup &s, int &s_top, int G, int N, int tid) {
    if (tid == 0) {
        int o = 0, top = -1;
        for (int n = 0; n < N; n++) { s.off[n] = o; o += s.cnt[n]; if (s.cnt[n]) top = n; }
        s_top = top;
    }
    __syncthreads();
    for (int i = tid; i < G * N; i += FTL_THREADS) {
        const int lv = s.lvl[i];
        if (lv >= 0) s.list[s.off[lv] + atomicAdd(&s.fill[lv], 1)] = (short)i;
    }
}

// a parent of height n reads a child of height cv; any other child (not below the parent, padding) reads as zero
__device__ __forceinline__ bool ftl_child_read(int cv, int n) { return cv >= 0 && cv < n; }

// stage [x | h_k1 | h_k2 | h_k3] of a tile of level n (float4 units: 3 + 3 * 32 a row); h = the plane that holds every node's h,
// rowg / rowch = a tile row's global node id and its children's (-1 = zero)
__device__ __forceinline__ void ftl_stage(float *s_x, const int *rowg, const int (*rowch)[3], const float *forest, const float *h,
                                          int n, int tid) {
    const int M = FTL_M;
    const int kq = n == 0 ? 3 : 3 + 3 * (M / 4);
    for (int i = tid; i < FTL_ROWS * kq; i += FTL_THREADS) {
        const int r = i / kq, q = i % kq;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int g = rowg[r];
        if (g >= 0) {
            if (q < 3) v = ((const float4 *)forest)[(size_t)g * 3 + q];
            else {
                const int j = (q - 3) / (M / 4), qq = (q - 3) % (M / 4);
                const int ch = rowch[r][j];
                if (ch >= 0) v = ((const float4 *)h)[(size_t)ch * (M / 4) + qq];
            }
        }
        *(float4 *)&s_x[r * FTL_STRIDE + 4 * q] = v;
    }
}

// i, o, u of one hidden unit before the bias, arow = this lane's row of the staged tile.  U h first, from zero, W x on top of
// it: every MFMA step rounds at the size of the running sum, and W x can be far larger than U h (the 192 steps of U h on top of
// W x cost up to 4x the error of a plain float32 forward).  r0, r1, r2 = the weight rows of the wave's first i, o, u unit
// (j0, M + j0, 2M + j0), as ftl_wx takes them: formed here from j0, the sums reassociate before inlining and both kernels end up
// with more registers (k_tree_lstm 198 -> 218 VGPRs and one workgroup a CU less, k_tree_lstm_bwd 241 -> 251)
__device__ __forceinline__ void ftl_pre_iou(const FtlTrees &p, const float *arow, int n, int r0, int r1, int r2, int col, int hh,
                                            fl_f32x16 &ai, fl_f32x16 &ao, fl_f32x16 &au) {
    const int M = FTL_M;
    const fl_f32x16 zero = {};
    ai = zero; ao = zero; au = zero;
    if (n > 0)
        ftl_gemm3<3 * FTL_M>(arow + FTL_F, p.u_iou + (size_t)(r0 + col) * 3 * M, p.u_iou + (size_t)(r1 + col) * 3 * M,
                             p.u_iou + (size_t)(r2 + col) * 3 * M, ai, ao, au, hh);
    ftl_wx(arow, p.w_iou, r0, r1, r2, col, ai, ao, au, 3, hh);
}

// W_f x of hidden unit j0 + col: the same for the three children, so the caller computes it once
__device__ __forceinline__ fl_f32x16 ftl_wfx(const FtlTrees &p, const float *arow, int j0, int col, int hh) {
    fl_f32x16 wfx = {}, dummy = {};
    ftl_wx(arow, p.w_f, j0, 0, 0, col, wfx, dummy, dummy, 1, hh);
    return wfx;
}

// U_f h_kj of hidden unit j0 + col, from zero as well
__device__ __forceinline__ fl_f32x16 ftl_ufh(const FtlTrees &p, const float *arow, int j, int j0, int col, int hh) {
    fl_f32x16 af = {};
    ftl_gemm1<FTL_M>(arow + FTL_F + j * FTL_M, p.u_f + (size_t)(j0 + col) * FTL_M, af, hh);
    return af;
}

// f_j before the sigmoid, one accumulator element: U_f h_kj and W_f x first, the bias last
__device__ __forceinline__ float ftl_pre_f(float ufh, float wfx, float bf) { return (ufh + wfx) + bf; }

__global__ void __launch_bounds__(FTL_THREADS) k_tree_lstm(FtlArgs p) {
    __shared__ __attribute__((aligned(16))) float s_x[FTL_ROWS * FTL_STRIDE];
    __shared__ FtlSetup s;
    __shared__ int s_top;
    __shared__ int s_rowg[FTL_ROWS], s_rowch[FTL_ROWS][3];   // tile row -> global node id, its children's global ids (-1 = zero)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, M = FTL_M;
    const int t0 = blockIdx.x * p.G;
    const int G = min(p.G, p.T - t0);

    // ---- set-up: one wave per tree
    ftl_setup_clear(s, G, N, tid);
    for (int tb = 0; tb < G; tb += 4) ftl_setup_tree(p, s, t0, G, tb + wave, lane, wave);
    ftl_bucket(s, s_top, G, N, tid);
    // padding nodes: h = c = 0 (every node's output, or the root's)
    if (!p.roots_only) {
        for (int i = tid; i < G * N * (M / 4); i += FTL_THREADS) {
            const int node = i / (M / 4), q = i % (M / 4);
            if (s.lvl[node] < 0) {
                const size_t g = (size_t)t0 * N + node;
                ((float4 *)p.h_out)[g * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.c_out) ((float4 *)p.c_out)[g * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    } else {
        for (int i = tid; i < G * (M / 4); i += FTL_THREADS) {
            const int tl = i / (M / 4), q = i % (M / 4);
            if (s.lvl[tl * N] < 0) {
                const size_t t = (size_t)t0 + tl;
                ((float4 *)p.h_out)[t * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.c_out) ((float4 *)p.c_out)[t * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __syncthreads();

    // ---- levels
    const int col = lane & 31, hh = lane >> 5, j0 = 32 * wave;
    const int top = s_top;
    for (int n = 0; n <= top; n++) {
        const int cnt = s.cnt[n], off = s.off[n];
        for (int r0 = 0; r0 < cnt; r0 += FTL_ROWS) {
            const int rows = min(FTL_ROWS, cnt - r0);
            if (tid < FTL_ROWS) {
                int g = -1, c0 = -1, c1 = -1, c2 = -1;
                if (tid < rows) {
                    const int node = s.list[off + r0 + tid], tl = node / N;
                    g = (t0 + tl) * N + node % N;
                    if (n > 0) {
                        int cs[3];
                        for (int j = 0; j < 3; j++) {
                            const int ch = s.child[node * 3 + j];
                            const int cv = ch >= 0 ? s.lvl[tl * N + ch] : -2;
                            cs[j] = ftl_child_read(cv, n) ? (t0 + tl) * N + ch : -1;
                        }
                        c0 = cs[0]; c1 = cs[1]; c2 = cs[2];
                    }
                }
                s_rowg[tid] = g;
                s_rowch[tid][0] = c0; s_rowch[tid][1] = c1; s_rowch[tid][2] = c2;
            }
            __syncthreads();
            ftl_stage(s_x, s_rowg, s_rowch, p.forest, p.hbuf, n, tid);
            __syncthreads();

            const float *arow = &s_x[col * FTL_STRIDE];         // this lane's A row (MFMA row = lane & 31)
            fl_f32x16 ai, ao, au;
            ftl_pre_iou(p, arow, n, j0, M + j0, 2 * M + j0, col, hh, ai, ao, au);
            const float bi = p.b_iou[j0 + col], bo = p.b_iou[M + j0 + col], bu = p.b_iou[2 * M + j0 + col];
            float iu[16], og[16], cc[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                iu[r] = ftl_sigmoid(ai[r] + bi) * tanhf(au[r] + bu);
                og[r] = ftl_sigmoid(ao[r] + bo);
                cc[r] = iu[r];
            }
            if (n > 0) {
                const fl_f32x16 wfx = ftl_wfx(p, arow, j0, col, hh);
                const float bf = p.b_f[j0 + col];
                float fc[3][16];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const fl_f32x16 af = ftl_ufh(p, arow, j, j0, col, hh);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = fl_acc_row(r, hh);
                        const int ch = s_rowch[row][j];
                        const float cv = ch >= 0 ? p.cbuf[(size_t)ch * M + j0 + col] : 0.f;
                        fc[j][r] = ftl_sigmoid(ftl_pre_f(af[r], wfx[r], bf)) * cv;
                    }
                }
                __syncthreads();                                // every wave is done with the staged tile
#pragma unroll
                for (int j = 0; j < 3; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = fl_acc_row(r, hh);
                        s_x[row * FTL_STRIDE + j * M + j0 + col] = fc[j][r];
                    }
                __syncthreads();
                fl_f32x16 ac = {};
                ftl_gemm1<3 * FTL_M>(arow, p.w_c + (size_t)(j0 + col) * 3 * M, ac, hh);
                const float bc = p.b_c[j0 + col];
#pragma unroll
                for (int r = 0; r < 16; r++) cc[r] = iu[r] + (ac[r] + bc);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, hh);
                if (row < rows) {
                    const int g = s_rowg[row];
                    const float hv = og[r] * tanhf(cc[r]);
                    p.hbuf[(size_t)g * M + j0 + col] = hv;
                    p.cbuf[(size_t)g * M + j0 + col] = cc[r];
                    if (p.roots_only && g % N == 0) {
                        p.h_out[(size_t)(g / N) * M + j0 + col] = hv;
                        if (p.c_out) p.c_out[(size_t)(g / N) * M + j0 + col] = cc[r];
                    }
                }
            }
            __syncthreads();                                    // the tile's h / c are visible; the LDS tile is free again
        }
    }
}

// trees a workgroup: about two workgroups a CU, at most FTL_MAX_G trees
static inline int ftl_group(int T, int n_cu) {
    const long long want = 2ll * (n_cu > 0 ? n_cu : 256);
    long long g = (T + want - 1) / want;
    return (int)std::max(1ll, std::min<long long>(g, FTL_MAX_G));
}

static inline void fl_launch_tree_lstm(const FtlArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_lstm, dim3((a.T + a.G - 1) / a.G), dim3(FTL_THREADS), 0, s, a);
}
