// fl_param_grads.h -- the parameter gradients of the policy network as one grouped kernel, float32 operands, gfx950.  Included by
// fl_param_grads.hip, which holds the entry points of include/flatland_param_grads.h; that header has the formulas, the summation
// order and the workspace.
//
// Every gradient is a sum over rows, G[p][q] = sum_r dZ[r][p] X[r][q] (a weight) or sum_r dZ[r][p] (a bias).  The host lists one
// FpgProblem per weight matrix (a matrix whose X is gathered through several index columns: one per column); k_param_grads runs them
// all in one launch, grid = (128 x 128 output tiles of all problems, row slices).
//
// A workgroup of 4 waves owns one output tile of one slice.  It stages 32 rows of dZ (128 columns) and of X (128 columns) in LDS
// (2 x 16 KB) and every wave takes a 64 x 64 quarter, four v_mfma_f32_32x32x2_f32 accumulators: the reduction runs over the rows,
// so lane l supplies dZ[r][p + (l & 31)] and X[r][q + (l & 31)] of row r = 2 k + (l >> 5), one ds_read_b32 each (32 consecutive
// floats a half wave: no bank conflict), and an element loaded from global memory serves 128 outputs (32 FLOP/B against 8 without
// the LDS tile).  The next step's rows are fetched into registers while the MFMAs of this step run.
//
// Summation order: the MFMA adds the rows of a block of FPG_BLOCK = 256 in float32; at the end of a block the accumulators are
// added to float64 ones and cleared, so a slice's blocks are added in float64 in block order; the last block is ragged.  A bias is
// summed in float64 throughout by the workgroups of the first column of tiles, from the dZ tile in LDS: a block's rows in row
// order, the blocks in block order.  With one slice the workgroup writes float32; with more it writes its float64 tile to the
// workspace and k_param_grads_reduce adds the slices in slice order.  No atomics, one writer an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_mfma.h"

#define FPG_TILE 128             // edge of a workgroup's output tile
#define FPG_KR 32                // rows a staging step
#define FPG_BLOCK 256            // rows a float32 partial product (policy.REDUCE_BLOCK)
#define FPG_THREADS 256
#define FPG_MAX_PROBLEMS 20
#define FPG_MAX_SLICES 32
#define FPG_NO_ORDER INT32_MIN   // x_min / b_min: no predicate

struct FpgProblem {
    const float *dz;             // [rows][ldz]; column p is dz[p] (+ dz[p + term_stride] + dz[p + 2 term_stride] with terms = 3, in float32)
    const float *x0, *x1;        // X = [x0 (w0 columns, ldx0 a row) | x1 (w1 columns)]; x1 NULL with w1 = 0
    const int32_t *idx;          // NULL, or row r of X is row idx[r * idx_ld] of x0 / x1; outside [0, idx_rows) reads as zero
    const int64_t *order;        // NULL, or node_order: X counts where order[r] >= x_min, the bias where order[r] >= b_min
    float *out, *bias;           // out[p * ldo + q]; bias[p] or NULL
    long long ws_off;            // doubles before this problem's [P][Q (+ 1 with a bias)] partial in a slice of the workspace
    int rows, ldz, P, terms, term_stride;
    int ldx0, w0, ldx1, w1;
    int idx_ld, idx_rows;
    int x_min, b_min;
    int ldo;
    int tile0, tiles_q;          // first tile of the grid's x, tiles along q
};

struct FpgArgs {
    FpgProblem pr[FPG_MAX_PROBLEMS];
    int n, slices;
    long long ws_stride;         // doubles a slice
    double *ws;
};

// A lane's share of the staging: four columns c .. c + 3 of four rows of dZ and of X a step.  The column is the lane's for the whole
// kernel, so what depends on it is decided once (FpgLaneZ, FpgLaneX); a row outside the problem is read at the last row and
// cleared by a select, so that the loads of a step are straight-line code and all in flight together.
struct FpgLaneZ {
    const float *p;              // dz + c, or dz where the lane has no column
    int n;                       // columns of the lane inside [0, P): 0 .. 4
    bool vec;                    // all four, 16-byte aligned: one float4 a term
};
struct FpgLaneX {
    const float *p[4];           // column c + j's first row (x0 or x1), x0 where the column is outside [0, Q)
    int ld[4];
    int n;                       // columns inside [0, Q)
    bool vec;                    // all four in one segment, 16-byte aligned
};

__device__ __forceinline__ FpgLaneZ fpg_lane_z(const FpgProblem &pr, int c) {
    FpgLaneZ z;
    z.n = min(max(pr.P - c, 0), 4);
    z.p = pr.dz + (z.n ? c : 0);
    z.vec = z.n == 4 && pr.ldz % 4 == 0;
    return z;
}

__device__ __forceinline__ FpgLaneX fpg_lane_x(const FpgProblem &pr, int c) {
    FpgLaneX x;
    const int Q = pr.w0 + pr.w1;
    x.n = min(max(Q - c, 0), 4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int cj = c + j;
        const bool second = cj >= pr.w0 && cj < Q;
        x.p[j] = cj >= Q ? pr.x0 : second ? pr.x1 + (cj - pr.w0) : pr.x0 + cj;
        x.ld[j] = second ? pr.ldx1 : pr.ldx0;
    }
    const bool one = c + 3 < pr.w0 || (c >= pr.w0 && c + 3 < Q);
    const int cc = c >= pr.w0 ? c - pr.w0 : c;
    x.vec = one && x.ld[0] % 4 == 0 && cc % 4 == 0;
    return x;
}

__device__ __forceinline__ float4 fpg_zero_unless(bool on, float4 v) {
    return make_float4(on ? v.x : 0.0f, on ? v.y : 0.0f, on ? v.z : 0.0f, on ? v.w : 0.0f);
}

// rows r0 + 8 i, i = 0 .. 3, of dZ
template <bool FULL>           // FULL: all four rows are inside the problem
__device__ __forceinline__ void fpg_fetch_z(const FpgProblem &pr, const FpgLaneZ &z, int r0, float4 (&out)[4]) {
    const int last = FULL ? INT32_MAX : pr.rows - 1;
    const bool three = pr.terms == 3;                          // (uniform; its branch stays outside the loops over the rows)
    if (z.vec && !three) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            out[i] = fpg_zero_unless(r0 + 8 * i <= last, *(const float4 *)(z.p + (size_t)min(r0 + 8 * i, last) * pr.ldz));
    } else if (z.vec) {
        float4 v[4], u[4], w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float *src = z.p + (size_t)min(r0 + 8 * i, last) * pr.ldz;
            v[i] = *(const float4 *)src;
            u[i] = *(const float4 *)(src + pr.term_stride);
            w[i] = *(const float4 *)(src + 2 * pr.term_stride);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            out[i] = fpg_zero_unless(r0 + 8 * i <= last, make_float4((v[i].x + u[i].x) + w[i].x, (v[i].y + u[i].y) + w[i].y,
                                                                      (v[i].z + u[i].z) + w[i].z, (v[i].w + u[i].w) + w[i].w));
    } else {                                                   // (a ragged edge: single floats, the terms read in any case)
        const int ts = three ? pr.term_stride : 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float *src = z.p + (size_t)min(r0 + 8 * i, last) * pr.ldz;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int jj = j < z.n ? j : 0;               // (a column outside reads the lane's first, or dz[0], and is cleared)
                const float t = src[jj], u = src[jj + ts], w = src[jj + 2 * ts];
                v[j] = j < z.n ? (three ? (t + u) + w : t) : 0.0f;
            }
            out[i] = fpg_zero_unless(r0 + 8 * i <= last, make_float4(v[0], v[1], v[2], v[3]));
        }
    }
}

// rows r0 + 8 i of X: gathered through idx, cleared where the node's order or its index says so
template <bool FULL>
__device__ __forceinline__ void fpg_fetch_x(const FpgProblem &pr, const FpgLaneX &x, int r0, float4 (&out)[4]) {
    const int last = FULL ? INT32_MAX : pr.rows - 1;
    int rr[4], k[4];
    int64_t o[4];
    bool on[4];
#pragma unroll
    for (int i = 0; i < 4; i++) rr[i] = min(r0 + 8 * i, last);
    if (pr.order) {                                            // (uniform branches around all four loads, the compares behind them)
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = pr.order[rr[i]];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = pr.x_min;
    }
    if (pr.idx) {
#pragma unroll
        for (int i = 0; i < 4; i++) k[i] = pr.idx[(size_t)rr[i] * pr.idx_ld];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) k[i] = rr[i];
    }
    const unsigned limit = pr.idx ? (unsigned)pr.idx_rows : (unsigned)pr.rows;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool inside = (unsigned)k[i] < limit;
        on[i] = (r0 + 8 * i <= last) & (o[i] >= (int64_t)pr.x_min) & inside;
        rr[i] = inside ? k[i] : 0;
    }
    if (x.vec) {
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = fpg_zero_unless(on[i], *(const float4 *)(x.p[0] + (size_t)rr[i] * x.ld[0]));
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float t = x.p[j][(size_t)rr[i] * x.ld[j]];
                v[j] = j < x.n ? t : 0.0f;
            }
            out[i] = fpg_zero_unless(on[i], make_float4(v[0], v[1], v[2], v[3]));
        }
    }
}

__global__ __launch_bounds__(FPG_THREADS) void k_param_grads(const FpgArgs a) {
    __shared__ __attribute__((aligned(16))) float zs[FPG_KR][FPG_TILE];
    __shared__ __attribute__((aligned(16))) float xs[FPG_KR][FPG_TILE];
    __shared__ int bflag[FPG_KR];
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), slice = blockIdx.y;
    const int col = l & 31, hh = l >> 5, wp = (w >> 1) * 64, wq = (w & 1) * 64;
    int pi = 0;
    while (pi + 1 < a.n && (int)blockIdx.x >= a.pr[pi + 1].tile0) pi++;
    const FpgProblem pr = a.pr[pi];
    const int tile = blockIdx.x - pr.tile0, p0 = tile / pr.tiles_q * FPG_TILE, q0 = tile % pr.tiles_q * FPG_TILE;
    const int P = pr.P, Q = pr.w0 + pr.w1;
    // the slice's blocks [b0, b1) and steps [s0, s1): a slice is a whole number of blocks, the last block may be ragged
    constexpr int SPB = FPG_BLOCK / FPG_KR;
    const int nblocks = (pr.rows + FPG_BLOCK - 1) / FPG_BLOCK, per = (nblocks + a.slices - 1) / a.slices;
    const int b0 = min(slice * per, nblocks), b1 = min(b0 + per, nblocks);
    const int s0 = b0 * SPB, s1 = min(b1 * SPB, (pr.rows + FPG_KR - 1) / FPG_KR);
    const bool with_bias = pr.bias != nullptr && q0 == 0 && t < FPG_TILE;       // (whole waves 0 and 1)
    const bool busy = p0 + wp < P && q0 + wq < Q;

    fl_f32x16 acc[2][2];
    double dacc[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[i][j][r] = 0.0f; dacc[i][j][r] = 0.0; }
    double bsum = 0.0, bblk = 0.0;

    // a thread's share of a step: rows (t >> 5) + 8 i, i = 0 .. 3, columns 4 (t & 31) .. + 3 of both tiles
    const int frow = t >> 5, fcol = 4 * (t & 31);
    float4 rz[4], rx[4];
    int rf = 0;
    const FpgLaneZ lz = fpg_lane_z(pr, p0 + fcol);
    const FpgLaneX lx = fpg_lane_x(pr, q0 + fcol);
    const bool flagged = pr.order != nullptr && pr.b_min != FPG_NO_ORDER;
    const auto fetch = [&](int s) {
        const int r0 = s * FPG_KR;
        if (r0 + FPG_KR <= pr.rows) {                          // (uniform: every step but a problem's last)
            fpg_fetch_z<true>(pr, lz, r0 + frow, rz);
            fpg_fetch_x<true>(pr, lx, r0 + frow, rx);
        } else {
            fpg_fetch_z<false>(pr, lz, r0 + frow, rz);
            fpg_fetch_x<false>(pr, lx, r0 + frow, rx);
        }
        if (t < FPG_KR) {
            const int r = min(r0 + t, pr.rows - 1);
            int64_t o = pr.b_min;
            if (flagged) o = pr.order[r];
            rf = (r0 + t < pr.rows) & (o >= (int64_t)pr.b_min);
        }
    };
    if (s0 < s1) fetch(s0);
#pragma unroll 1
    for (int s = s0; s < s1; s++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *(float4 *)&zs[frow + 8 * i][fcol] = rz[i];
            *(float4 *)&xs[frow + 8 * i][fcol] = rx[i];
        }
        if (t < FPG_KR) bflag[t] = rf;
        __syncthreads();
        if (s + 1 < s1) fetch(s + 1);
        if (busy)                                              // (a wave whose quarter lies outside the matrix has nothing to add)
#pragma unroll 4
        for (int k = 0; k < FPG_KR / 2; k++) {
            const int kr = 2 * k + hh;
            const float a0 = zs[kr][wp + col], a1 = zs[kr][wp + 32 + col];
            const float x0 = xs[kr][wq + col], x1 = xs[kr][wq + 32 + col];
            acc[0][0] = fl_mfma(a0, x0, acc[0][0]);
            acc[0][1] = fl_mfma(a0, x1, acc[0][1]);
            acc[1][0] = fl_mfma(a1, x0, acc[1][0]);
            acc[1][1] = fl_mfma(a1, x1, acc[1][1]);
        }
        if (with_bias && flagged) {
#pragma unroll 8
            for (int k = 0; k < FPG_KR; k++)
                bblk += bflag[k] ? (double)zs[k][t] : 0.0;
        } else if (with_bias) {                                // (rows behind the last are zero in the tile)
#pragma unroll 8
            for (int k = 0; k < FPG_KR; k++)
                bblk += (double)zs[k][t];
        }
        if ((s + 1) % SPB == 0 || s + 1 == s1) {        // the block's float32 sums join the float64 ones
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) { dacc[i][j][r] += (double)acc[i][j][r]; acc[i][j][r] = 0.0f; }
            bsum += bblk;
            bblk = 0.0;
        }
        __syncthreads();
    }

    const int Qb = Q + (pr.bias ? 1 : 0);
    double *ws = a.slices > 1 ? a.ws + (size_t)slice * a.ws_stride + pr.ws_off : nullptr;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int p = p0 + wp + 32 * i + fl_acc_row(r, hh), q = q0 + wq + 32 * j + col;
                if (p < P && q < Q) {
                    if (ws) ws[(size_t)p * Qb + q] = dacc[i][j][r];
                    else pr.out[(size_t)p * pr.ldo + q] = (float)dacc[i][j][r];
                }
            }
    if (with_bias && p0 + t < P) {
        if (ws) ws[(size_t)(p0 + t) * Qb + Q] = bsum;
        else pr.bias[p0 + t] = (float)bsum;
    }
}

// more than one slice: out = the slices' float64 partials added in slice order.  grid = (chunks of a problem's elements, problems)
__global__ __launch_bounds__(FPG_THREADS) void k_param_grads_reduce(const FpgArgs a) {
    const FpgProblem &pr = a.pr[blockIdx.y];
    const int Q = pr.w0 + pr.w1, Qb = Q + (pr.bias ? 1 : 0), n = pr.P * Qb;
    for (int e = blockIdx.x * FPG_THREADS + threadIdx.x; e < n; e += gridDim.x * FPG_THREADS) {
        const double *src = a.ws + pr.ws_off + e;
        double s = src[0];
        for (int k = 1; k < a.slices; k++) s += src[(size_t)k * a.ws_stride];
        const int p = e / Qb, q = e % Qb;
        if (q < Q) pr.out[(size_t)p * pr.ldo + q] = (float)s;
        else pr.bias[p] = (float)s;
    }
}
