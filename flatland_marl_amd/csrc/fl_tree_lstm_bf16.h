// fl_tree_lstm_bf16.h -- the TreeLSTM forward of fl_tree_lstm.h with the three recurrent products on the bf16 matrix instruction
// (gfx950), for inference.  Included by fl_tree_lstm.hip behind fl_tree_lstm.h, whose set-up (ftl_setup_clear, ftl_setup_tree,
// ftl_bucket, ftl_child_read), input products (ftl_wx, ftl_wfx), gate code (ftl_sigmoid, ftl_pre_f) and grouping (ftl_group) it
// calls: the same trees are accepted and counted, a leaf sees the same float32 arithmetic.
//
// What differs from k_tree_lstm: U_iou [h_k1|h_k2|h_k3], U_f h_kj and W_c [f_1*c_k1|f_2*c_k2|f_3*c_k3] run as
// v_mfma_f32_32x32x16_bf16 with a float32 accumulator.  The weights come rounded to bf16 (round to nearest even) from
// fl_tree_lstm_pack_bf16, in the order the kernel streams them (below); h_k is rounded when a tile is staged, f_j * c_kj when it is
// written over the tile.  W_iou x and W_f x (K = 12) stay exact float32 MFMA steps on top of the recurrent sum started from zero, as
// in ftl_pre_iou; biases, sigmoid / tanh and the h / c planes the next level reads stay float32.
//
// Tile: 32 nodes (FTL_ROWS), wave w computes hidden units 32w .. 32w+31, as in k_tree_lstm.  A staged row is [x f32 x 12 | h_k
// bf16 x 384] = 816 bytes = 204 dwords, with no padding: a ds_read_b128 is served in groups of 16 lanes whose rows (lane & 31) are
// a full set of residues mod 16, and a bank row has 16 slots of 16 bytes, so the 16 rows of a group hit 16 distinct slots when the
// stride in 16-byte slots is odd -- 816 / 16 = 51.  Lane l of a K = 16 step holds A[row l & 31][k = 8 (l >> 5) + j] and B[k][col
// l & 31], j = 0 .. 7: one 16-byte read of its LDS row and one of the packed weights a step.
//
// Packed weights (include/flatland_policy_bf16.h): a matrix W [R][K] is stored as R / 32 blocks of 32 rows; a block holds its K / 16
// steps one after another, a step the 64 lanes' operands one after another, 8 bf16 each: element j of lane l of step s of block b is
// W[32 b + (l & 31)][16 s + 8 (l >> 5) + j].  A wave's load of a step is 1 KB of consecutive bytes, eight whole 128-byte lines.  Read
// in torch's row-major layout instead (each lane 32 bytes of its own weight row a 32-k chunk, a quarter of 32 lines a load) the kernel
// measured 338 / 4 495 us at cfg2 / cfg3 against 297 / 4 083 us (profiles/tree_lstm_bf16_variants.json).
#pragma once
#include "fl_tree_lstm.h"

#define FTL16_XBYTES (FTL_F * 4)                        // the float32 features in front of a staged row
#define FTL16_STRIDE (FTL16_XBYTES + 3 * FTL_M * 2)     // bytes a staged row: 816
#define FTL16_U_IOU 0                                   // element offsets of the three matrices in the packed buffer
#define FTL16_W_C (3 * FTL_M * 3 * FTL_M)
#define FTL16_U_F (FTL16_W_C + FTL_M * 3 * FTL_M)
#define FTL16_PACKED (FTL16_U_F + FTL_M * FTL_M)        // 212 992 bf16 = 425 984 bytes
#define FTL16_STEP 512                                  // bf16 a packed step: 64 lanes x 8
#ifndef FTL16_UNROLL
#define FTL16_UNROLL 4                                  // K = 16 steps whose loads are issued together
#endif

struct Ftl16Args : FtlArgs {
    const __bf16 *packed;           // fl_tree_lstm_pack_bf16's buffer; u_iou, w_c, u_f of FtlTrees are NULL
};

// this lane's operands of step 0 of block `block` of a packed matrix of K columns
template <int K>
__device__ __forceinline__ const __bf16 *ftl16_block(const __bf16 *w, int block, int lane) {
    return w + (size_t)block * (K / 16) * FTL16_STEP + lane * 8;
}

// acc += A[row][k] * W[32 b + col][k] over k in [0, K), K a multiple of 16; arow = this lane's staged h_k / f*c_k row + 8 hh,
// wl = ftl16_block of the matrix
template <int K>
__device__ __forceinline__ void ftl16_gemm1(const __bf16 *arow, const __bf16 *wl, fl_f32x16 &acc) {
#pragma unroll FTL16_UNROLL
    for (int s = 0; s < K / 16; s++)
        acc = fl_mfma_bf16(*(const fl_bf16x8 *)(arow + 16 * s), *(const fl_bf16x8 *)(wl + s * FTL16_STEP), acc);
}

// the same for three blocks at once (i, o, u of one hidden unit), sharing the A operand
template <int K>
__device__ __forceinline__ void ftl16_gemm3(const __bf16 *arow, const __bf16 *w0, const __bf16 *w1, const __bf16 *w2, fl_f32x16 &c0,
                                            fl_f32x16 &c1, fl_f32x16 &c2) {
#pragma unroll FTL16_UNROLL
    for (int s = 0; s < K / 16; s++) {
        const fl_bf16x8 a = *(const fl_bf16x8 *)(arow + 16 * s);
        const fl_bf16x8 b0 = *(const fl_bf16x8 *)(w0 + s * FTL16_STEP), b1 = *(const fl_bf16x8 *)(w1 + s * FTL16_STEP),
                        b2 = *(const fl_bf16x8 *)(w2 + s * FTL16_STEP);
        c0 = fl_mfma_bf16(a, b0, c0);
        c1 = fl_mfma_bf16(a, b1, c1);
        c2 = fl_mfma_bf16(a, b2, c2);
    }
}

// stage [x | bf16(h_k1) | bf16(h_k2) | bf16(h_k3)] of a tile of level n in 16-byte units (3 of x, 16 a child); h = the float32 plane
// that holds every node's h, rowg / rowch = a tile row's global node id and its children's (-1 = zero)
__device__ __forceinline__ void ftl16_stage(unsigned char *s_t, const int *rowg, const int (*rowch)[3], const float *forest,
                                            const float *h, int n, int tid) {
    const int M = FTL_M;
    const int kq = n == 0 ? 3 : 3 + 3 * (M / 8);
    for (int i = tid; i < FTL_ROWS * kq; i += FTL_THREADS) {
        const int r = i / kq, q = i % kq;
        const int g = rowg[r];
        unsigned char *row = s_t + r * FTL16_STRIDE;
        if (q < 3) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g >= 0) v = ((const float4 *)forest)[(size_t)g * 3 + q];
            *(float4 *)(row + 16 * q) = v;
        } else {
            const int j = (q - 3) / (M / 8), qq = (q - 3) % (M / 8);
            const int ch = g >= 0 ? rowch[r][j] : -1;
            fl_bf16x8 o = {};
            if (ch >= 0) {
                const float4 a = ((const float4 *)h)[(size_t)ch * (M / 4) + 2 * qq], b = ((const float4 *)h)[(size_t)ch * (M / 4) + 2 * qq + 1];
                o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
                o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
            }
            *(fl_bf16x8 *)(row + 16 * q) = o;
        }
    }
}

__global__ void __launch_bounds__(FTL_THREADS) k_tree_lstm_bf16(Ftl16Args p) {
    __shared__ __attribute__((aligned(16))) unsigned char s_t[FTL_ROWS * FTL16_STRIDE];
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
    const __bf16 *u_iou = p.packed + FTL16_U_IOU, *w_c = p.packed + FTL16_W_C, *u_f = p.packed + FTL16_U_F;
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
            ftl16_stage(s_t, s_rowg, s_rowch, p.forest, p.hbuf, n, tid);
            __syncthreads();

            const float *xrow = (const float *)(s_t + col * FTL16_STRIDE);              // this lane's A row (MFMA row = lane & 31)
            const __bf16 *hrow = (const __bf16 *)(s_t + col * FTL16_STRIDE + FTL16_XBYTES) + 8 * hh;    // ... and its k half of a step
            const fl_f32x16 zero = {};
            fl_f32x16 ai = zero, ao = zero, au = zero;
            if (n > 0)          // the i, o, u rows of this wave's hidden units: blocks w, 4 + w, 8 + w of U_iou
                ftl16_gemm3<3 * FTL_M>(hrow, ftl16_block<3 * FTL_M>(u_iou, wave, lane), ftl16_block<3 * FTL_M>(u_iou, 4 + wave, lane),
                                       ftl16_block<3 * FTL_M>(u_iou, 8 + wave, lane), ai, ao, au);
            ftl_wx(xrow, p.w_iou, j0, M + j0, 2 * M + j0, col, ai, ao, au, 3, hh);       // exact float32, on top of U h
            const float bi = p.b_iou[j0 + col], bo = p.b_iou[M + j0 + col], bu = p.b_iou[2 * M + j0 + col];
            float iu[16], og[16], cc[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                iu[r] = ftl_sigmoid(ai[r] + bi) * tanhf(au[r] + bu);
                og[r] = ftl_sigmoid(ao[r] + bo);
                cc[r] = iu[r];
            }
            if (n > 0) {
                const fl_f32x16 wfx = ftl_wfx(p, xrow, j0, col, hh);
                const float bf = p.b_f[j0 + col];
                float fc[3][16];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    fl_f32x16 af = zero;
                    ftl16_gemm1<FTL_M>(hrow + j * M, ftl16_block<FTL_M>(u_f, wave, lane), af);
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
                        *(__bf16 *)(s_t + row * FTL16_STRIDE + FTL16_XBYTES + 2 * (j * M + j0 + col)) = (__bf16)fc[j][r];
                    }
                __syncthreads();
                fl_f32x16 ac = zero;
                ftl16_gemm1<3 * FTL_M>(hrow, ftl16_block<3 * FTL_M>(w_c, wave, lane), ac);
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

// fl_tree_lstm_pack_bf16: element i of the packed buffer = bf16(its source element), round to nearest even (v_cvt_pk_bf16_f32)
__global__ void __launch_bounds__(256) k_tree_lstm_pack_bf16(const float *u_iou, const float *w_c, const float *u_f, __bf16 *dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FTL16_PACKED) return;
    const float *src = i < FTL16_W_C ? u_iou : i < FTL16_U_F ? w_c : u_f;
    const int K = i < FTL16_U_F ? 3 * FTL_M : FTL_M;
    const int e = i - (i < FTL16_W_C ? FTL16_U_IOU : i < FTL16_U_F ? FTL16_W_C : FTL16_U_F);
    const int j = e & 7, l = (e >> 3) & 63, t = e / FTL16_STEP;
    const int step = t % (K / 16), block = t / (K / 16);
    dst[i] = (__bf16)src[(size_t)(32 * block + (l & 31)) * K + 16 * step + 8 * (l >> 5) + j];
}

static inline void fl_launch_tree_lstm_bf16(const Ftl16Args &a, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_lstm_bf16, dim3((a.T + a.G - 1) / a.G), dim3(FTL_THREADS), 0, s, a);
}

static inline void fl_launch_tree_lstm_pack_bf16(const float *u_iou, const float *w_c, const float *u_f, void *dst, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_lstm_pack_bf16, dim3((FTL16_PACKED + 255) / 256), dim3(256), 0, s, u_iou, w_c, u_f, (__bf16 *)dst);
}
