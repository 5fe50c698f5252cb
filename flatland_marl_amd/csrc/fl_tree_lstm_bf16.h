// fl_tree_lstm_bf16.h -- the TreeLSTM forward of fl_tree_lstm.h with the three recurrent products on the bf16 matrix instruction
// (gfx950), for inference.  Included by fl_tree_lstm.hip behind fl_tree_lstm.h, whose set-up (ftl_setup_clear, ftl_setup_tree,
// ftl_bucket, ftl_child_read), input products (ftl_wx, ftl_wfx), gate code (ftl_sigmoid, ftl_pre_f) and grouping (ftl_group) it
// calls: the same trees are accepted and counted, a leaf sees the same float32 arithmetic.
//
// What differs from k_tree_lstm: U_iou [h_k1|h_k2|h_k3], U_f h_kj and W_c [f_1*c_k1|f_2*c_k2|f_3*c_k3] run as
// v_mfma_f32_32x32x16_bf16 with a float32 accumulator.  The weights come rounded to bf16 (round to nearest even) from
// fl_tree_lstm_pack_bf16, in the order the kernel streams them (fl_bf16.h); h_k is rounded when a tile is staged, f_j * c_kj when it is
// written over the tile.  W_iou x and W_f x (K = 12) stay exact float32 MFMA steps on top of the recurrent sum started from zero, as
// in ftl_pre_iou; biases, sigmoid / tanh and the h / c planes the next level reads stay float32.
//
// Tile: 32 nodes (FTL_ROWS), wave w computes hidden units 32w .. 32w+31, as in k_tree_lstm.  A staged row is [x f32 x 12 | h_k
// bf16 x 384] = 816 bytes = 204 dwords, with no padding: a ds_read_b128 is served in groups of 16 lanes whose rows (lane & 31) are
// a full set of residues mod 16, and a bank row has 16 slots of 16 bytes, so the 16 rows of a group hit 16 distinct slots when the
// stride in 16-byte slots is odd -- 816 / 16 = 51.  What a lane holds of a K = 16 step: fl_bf16.h.
//
// Packed weights: fl_tree_lstm_pack_bf16's buffer holds U_iou, W_c and U_f one after another, each in the format of fl_bf16.h.
#pragma once
#include "fl_bf16.h"
#include "fl_tree_lstm.h"

#define FTL16_XBYTES (FTL_F * 4)                        // the float32 features in front of a staged row
#define FTL16_STRIDE (FTL16_XBYTES + 3 * FTL_M * 2)     // bytes a staged row: 816
#define FTL16_U_IOU 0                                   // element offsets of the three matrices in the packed buffer
#define FTL16_W_C (3 * FTL_M * 3 * FTL_M)
#define FTL16_U_F (FTL16_W_C + FTL_M * 3 * FTL_M)
#define FTL16_PACKED (FTL16_U_F + FTL_M * FTL_M)        // 212 992 bf16 = 425 984 bytes

struct Ftl16Args : FtlArgs {
    const __bf16 *packed;           // fl_tree_lstm_pack_bf16's buffer; u_iou, w_c, u_f of FtlTrees are NULL
};

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
                o = fl_bf16_round8(a, b);
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
            fl_f32x16 iou[3] = {zero, zero, zero};
            if (n > 0) {        // the i, o, u rows of this wave's hidden units: blocks w, 4 + w, 8 + w of U_iou
                const __bf16 *const ws[3] = {fl_bf16_block(u_iou, 3 * M, wave, lane), fl_bf16_block(u_iou, 3 * M, 4 + wave, lane),
                                             fl_bf16_block(u_iou, 3 * M, 8 + wave, lane)};
                fl_bf16_mm<3>(hrow, 3 * M / 16, ws, iou);
            }
            fl_f32x16 &ai = iou[0], &ao = iou[1], &au = iou[2];
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
                    fl_bf16_mm(hrow + j * M, M / 16, fl_bf16_block(u_f, M, wave, lane), af);
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
                fl_bf16_mm(hrow, 3 * M / 16, fl_bf16_block(w_c, 3 * M, wave, lane), ac);
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

static inline void fl_launch_tree_lstm_bf16(const Ftl16Args &a, hipStream_t s) {
    hipLaunchKernelGGL(k_tree_lstm_bf16, dim3((a.T + a.G - 1) / a.G), dim3(FTL_THREADS), 0, s, a);
}

// fl_tree_lstm_pack_bf16: the three matrices at FTL16_U_IOU, FTL16_W_C, FTL16_U_F
static inline void fl_launch_tree_lstm_pack_bf16(const float *u_iou, const float *w_c, const float *u_f, void *dst, hipStream_t s) {
    FlBf16Pack<3> a = {{u_iou, w_c, u_f}, {}, {3 * FTL_M, 3 * FTL_M, FTL_M}};
    fl_launch_bf16_pack(a, {3 * FTL_M, FTL_M, FTL_M}, dst, s);
}
