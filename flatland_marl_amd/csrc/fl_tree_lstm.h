// fl_tree_lstm.h -- the policy's TreeLSTM forward (solution/nn/TreeLSTM.py:33-154) for a whole batch of trees, one launch
// (gfx950).  Included by fl_host.hip, next to its entry points fl_tree_lstm / fl_tree_lstm_workspace_bytes.
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
// K = 384 + 12 (U h from zero, then W x: see the level loop), W_f x once and U_f h_kj for the three children, then f_j * c_kj
// goes to LDS (over the staged tile) and W_c runs over K = 384.  A wave's three iou accumulators hold the same hidden units, so the epilogue is in registers.  Weights are read
// in torch's [out][in] layout straight from global memory (L2): lane l of an MFMA step takes k = kc + 16 * (l >> 5) + s of
// chunk kc, so every lane loads 64 contiguous bytes of one weight row a chunk.  h and c of every node go to the output buffers
// or the workspace; the next level of the same workgroup reads them back after a barrier (workgroup-scope release / acquire).
#pragma once
#include "fl_internal.h"

#define FTL_F 12
#define FTL_M 128
#define FTL_THREADS 256
#define FTL_ROWS 32                 // nodes a tile (the MFMA's 32 rows)
#define FTL_STRIDE 420              // floats a staged row: 12 + 3 * 128 = 396 used
#define FTL_MAX_G 16                // trees a workgroup
#define FTL_MAX_N 64                // nodes a tree (one lane per node in the set-up)

typedef float ftl_f32x16 __attribute__((ext_vector_type(16)));

struct FtlArgs {
    int T, N, G, roots_only;
    const float *forest;
    const long long *adj, *no, *eo;
    const float *w_iou, *b_iou, *u_iou, *w_c, *b_c, *w_f, *b_f, *u_f;
    float *h_out, *c_out;           // as the caller passed them (c_out may be NULL); roots_only: [T][M]
    float *hbuf, *cbuf;             // h / c of every node, [T*N][M] (the outputs or the workspace)
    int *status;
};

__device__ __forceinline__ float ftl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ ftl_f32x16 ftl_mfma(float a, float b, ftl_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// acc += A[row][aoff + k] * W[wrow][k] over k in [0, K), K a multiple of 32; A = the staged tile row of this lane, W row-major
template <int K>
__device__ __forceinline__ void ftl_gemm1(const float *arow, const float *w0, ftl_f32x16 &acc, int hh) {
#pragma unroll 2
    for (int kc = 0; kc < K; kc += 32) {
        float a[16], b[16];
        const float4 *ap = (const float4 *)(arow + kc + 16 * hh), *bp = (const float4 *)(w0 + kc + 16 * hh);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4 av = ap[q], bv = bp[q];
            a[4 * q] = av.x; a[4 * q + 1] = av.y; a[4 * q + 2] = av.z; a[4 * q + 3] = av.w;
            b[4 * q] = bv.x; b[4 * q + 1] = bv.y; b[4 * q + 2] = bv.z; b[4 * q + 3] = bv.w;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) acc = ftl_mfma(a[s], b[s], acc);
    }
}

// the same for three weight rows at once (i, o, u of one hidden unit), sharing the A operand
template <int K>
__device__ __forceinline__ void ftl_gemm3(const float *arow, const float *w0, const float *w1, const float *w2, ftl_f32x16 &c0,
                                          ftl_f32x16 &c1, ftl_f32x16 &c2, int hh) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 32) {
        float a[16], b0[16], b1[16], b2[16];
        const int o = kc + 16 * hh;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4 av = ((const float4 *)(arow + o))[q];
            float4 v0 = ((const float4 *)(w0 + o))[q], v1 = ((const float4 *)(w1 + o))[q], v2 = ((const float4 *)(w2 + o))[q];
            a[4 * q] = av.x; a[4 * q + 1] = av.y; a[4 * q + 2] = av.z; a[4 * q + 3] = av.w;
            b0[4 * q] = v0.x; b0[4 * q + 1] = v0.y; b0[4 * q + 2] = v0.z; b0[4 * q + 3] = v0.w;
            b1[4 * q] = v1.x; b1[4 * q + 1] = v1.y; b1[4 * q + 2] = v1.z; b1[4 * q + 3] = v1.w;
            b2[4 * q] = v2.x; b2[4 * q + 1] = v2.y; b2[4 * q + 2] = v2.z; b2[4 * q + 3] = v2.w;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) {
            c0 = ftl_mfma(a[s], b0[s], c0);
            c1 = ftl_mfma(a[s], b1[s], c1);
            c2 = ftl_mfma(a[s], b2[s], c2);
        }
    }
}

// the K = 12 products (W x): step s takes k = 2s + (l >> 5)
__device__ __forceinline__ void ftl_wx(const float *xrow, const float *w, int r0, int r1, int r2, int col,
                                       ftl_f32x16 &c0, ftl_f32x16 &c1, ftl_f32x16 &c2, int nmat, int hh) {
#pragma unroll
    for (int s = 0; s < FTL_F / 2; s++) {
        const int k = 2 * s + hh;
        const float a = xrow[k];
        c0 = ftl_mfma(a, w[(size_t)(r0 + col) * FTL_F + k], c0);
        if (nmat > 1) {
            c1 = ftl_mfma(a, w[(size_t)(r1 + col) * FTL_F + k], c1);
            c2 = ftl_mfma(a, w[(size_t)(r2 + col) * FTL_F + k], c2);
        }
    }
}

__global__ void __launch_bounds__(FTL_THREADS) k_tree_lstm(FtlArgs p) {
    __shared__ __attribute__((aligned(16))) float s_x[FTL_ROWS * FTL_STRIDE];
    __shared__ short s_child[FTL_MAX_G * FTL_MAX_N * 3];     // tree-local child of (node, j), -1 = none
    __shared__ short s_list[FTL_MAX_G * FTL_MAX_N];          // group-local node ids bucketed by height
    __shared__ signed char s_lvl[FTL_MAX_G * FTL_MAX_N];     // height, -2 = padding (or an invalid node_order)
    __shared__ int s_tmp[4][3][FTL_MAX_N];                   // per wave: node height, edge height, node rank of the tree in set-up
    __shared__ int s_cnt[FTL_MAX_N], s_off[FTL_MAX_N], s_fill[FTL_MAX_N], s_top;
    __shared__ int s_rowg[FTL_ROWS], s_rowch[FTL_ROWS][3];   // tile row -> global node id, its children's global ids (-1 = zero)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, E = N - 1, M = FTL_M;
    const int t0 = blockIdx.x * p.G;
    const int G = min(p.G, p.T - t0);

    for (int i = tid; i < FTL_MAX_N; i += FTL_THREADS) { s_cnt[i] = 0; s_fill[i] = 0; }
    for (int i = tid; i < G * N * 3; i += FTL_THREADS) s_child[i] = -1;
    __syncthreads();

    // ---- set-up: one wave per tree
    for (int tb = 0; tb < G; tb += 4) {
        const int tl = tb + wave;
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
            s_tmp[wave][0][lane] = lv;
            s_tmp[wave][1][lane] = el;
        }
        __syncthreads();
        int rank = 0, nsame = 0, esame = 0, erank = 0;
        if (act) {
            for (int v = 0; v < N; v++) {
                const int o = s_tmp[wave][0][v];
                nsame += o == lv;
                rank += (o == lv) & (v < lane);
            }
            for (int e = 0; e < E; e++) {
                const int o = s_tmp[wave][1][e];
                esame += o == lv;
                erank += (o == el) & (e < lane);
            }
            if (lane < N) s_tmp[wave][2][lane] = rank;
            if (lane < N && lv >= 1 && esame != 3 * nsame) bad = true;
        }
        __syncthreads();
        if (act) {
            if (lane < N) {
                s_lvl[tl * N + lane] = (signed char)lv;
                if (lv >= 0) atomicAdd(&s_cnt[lv], 1);
            }
            if (el >= 0) {
                if (s_tmp[wave][0][pl] != el) bad = true;
                else if (el >= 1) {
                    if (s_tmp[wave][2][pl] != erank / 3) bad = true;
                    else s_child[(tl * N + pl) * 3 + erank % 3] = (short)cl;
                }
            }
            const unsigned long long anybad = __ballot(bad);
            if (lane == 0 && anybad && p.status) atomicAdd(p.status, 1);
        }
        __syncthreads();
    }
    if (tid == 0) {
        int o = 0, top = -1;
        for (int n = 0; n < N; n++) { s_off[n] = o; o += s_cnt[n]; if (s_cnt[n]) top = n; }
        s_top = top;
    }
    __syncthreads();
    for (int i = tid; i < G * N; i += FTL_THREADS) {
        const int lv = s_lvl[i];
        if (lv >= 0) s_list[s_off[lv] + atomicAdd(&s_fill[lv], 1)] = (short)i;
    }
    // padding nodes: h = c = 0 (every node's output, or the root's)
    if (!p.roots_only) {
        for (int i = tid; i < G * N * (M / 4); i += FTL_THREADS) {
            const int node = i / (M / 4), q = i % (M / 4);
            if (s_lvl[node] < 0) {
                const size_t g = (size_t)t0 * N + node;
                ((float4 *)p.h_out)[g * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.c_out) ((float4 *)p.c_out)[g * (M / 4) + q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    } else {
        for (int i = tid; i < G * (M / 4); i += FTL_THREADS) {
            const int tl = i / (M / 4), q = i % (M / 4);
            if (s_lvl[tl * N] < 0) {
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
        const int cnt = s_cnt[n], off = s_off[n];
        for (int r0 = 0; r0 < cnt; r0 += FTL_ROWS) {
            const int rows = min(FTL_ROWS, cnt - r0);
            if (tid < FTL_ROWS) {
                int g = -1, c0 = -1, c1 = -1, c2 = -1;
                if (tid < rows) {
                    const int node = s_list[off + r0 + tid], tl = node / N;
                    g = (t0 + tl) * N + node % N;
                    if (n > 0) {
                        int cs[3];
                        for (int j = 0; j < 3; j++) {
                            const int ch = s_child[node * 3 + j];
                            const int cv = ch >= 0 ? s_lvl[tl * N + ch] : -2;
                            cs[j] = (cv >= 0 && cv < n) ? (t0 + tl) * N + ch : -1;
                        }
                        c0 = cs[0]; c1 = cs[1]; c2 = cs[2];
                    }
                }
                s_rowg[tid] = g;
                s_rowch[tid][0] = c0; s_rowch[tid][1] = c1; s_rowch[tid][2] = c2;
            }
            __syncthreads();
            // stage [x | h_k1 | h_k2 | h_k3] (float4 units: 3 + 3 * 32 a row)
            const int kq = n == 0 ? 3 : 3 + 3 * (M / 4);
            for (int i = tid; i < FTL_ROWS * kq; i += FTL_THREADS) {
                const int r = i / kq, q = i % kq;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int g = s_rowg[r];
                if (g >= 0) {
                    if (q < 3) v = ((const float4 *)p.forest)[(size_t)g * 3 + q];
                    else {
                        const int j = (q - 3) / (M / 4), qq = (q - 3) % (M / 4);
                        const int ch = s_rowch[r][j];
                        if (ch >= 0) v = ((const float4 *)p.hbuf)[(size_t)ch * (M / 4) + qq];
                    }
                }
                *(float4 *)&s_x[r * FTL_STRIDE + 4 * q] = v;
            }
            __syncthreads();

            const float *arow = &s_x[col * FTL_STRIDE];         // this lane's A row (MFMA row = lane & 31)
            // U h first, from zero, W x on top of it: every MFMA step rounds at the size of the running sum, and W x can be far
            // larger than U h (the 192 steps of U h on top of W x cost up to 4x the error of a plain float32 forward)
            ftl_f32x16 ai = {}, ao = {}, au = {};
            if (n > 0)
                ftl_gemm3<3 * FTL_M>(arow + FTL_F, p.u_iou + (size_t)(j0 + col) * 3 * M, p.u_iou + (size_t)(M + j0 + col) * 3 * M,
                                     p.u_iou + (size_t)(2 * M + j0 + col) * 3 * M, ai, ao, au, hh);
            ftl_wx(arow, p.w_iou, j0, M + j0, 2 * M + j0, col, ai, ao, au, 3, hh);
            const float bi = p.b_iou[j0 + col], bo = p.b_iou[M + j0 + col], bu = p.b_iou[2 * M + j0 + col];
            float iu[16], og[16], cc[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                iu[r] = ftl_sigmoid(ai[r] + bi) * tanhf(au[r] + bu);
                og[r] = ftl_sigmoid(ao[r] + bo);
                cc[r] = iu[r];
            }
            if (n > 0) {
                ftl_f32x16 wfx = {}, dummy = {};
                ftl_wx(arow, p.w_f, j0, 0, 0, col, wfx, dummy, dummy, 1, hh);
                const float bf = p.b_f[j0 + col];
                float fc[3][16];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    ftl_f32x16 af = {};                          // (U_f h from zero as well; W_f x is added once, below)
                    ftl_gemm1<FTL_M>(arow + FTL_F + j * M, p.u_f + (size_t)(j0 + col) * M, af, hh);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                        const int ch = s_rowch[row][j];
                        const float cv = ch >= 0 ? p.cbuf[(size_t)ch * M + j0 + col] : 0.f;
                        fc[j][r] = ftl_sigmoid((af[r] + wfx[r]) + bf) * cv;
                    }
                }
                __syncthreads();                                // every wave is done with the staged tile
#pragma unroll
                for (int j = 0; j < 3; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                        s_x[row * FTL_STRIDE + j * M + j0 + col] = fc[j][r];
                    }
                __syncthreads();
                ftl_f32x16 ac = {};
                ftl_gemm1<3 * FTL_M>(arow, p.w_c + (size_t)(j0 + col) * 3 * M, ac, hh);
                const float bc = p.b_c[j0 + col];
#pragma unroll
                for (int r = 0; r < 16; r++) cc[r] = iu[r] + (ac[r] + bc);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
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
