// fl_policy_head_bwd.h -- the gradient of fl_policy_head (fl_policy_head.h) for a whole batch, float32, gfx950.  Included by
// fl_policy_head.hip, which holds the entry points of include/flatland_policy_train.h; that header has the formulas and the
// layout of the saved forward, of the rows and of the workspace.
//
// The same tiling as the forward: a workgroup of 4 waves takes 32 consecutive rows (which may straddle envs) and keeps a chain of
// layers in LDS tiles of row stride 260; the attention takes (env, tile of 32 agents) with a wave per head.  Run in reverse:
//   k_pb_heads          actor_net and critic_net: their first two layers again, then back -> d both = (d emb | dy_3)
//   per block 2, 1, 0:
//     k_pb_block        out_proj and att_mlp again, dz = dy_{i+1} g'(z), -> dy_i (att_mlp's half), do, dc
//     k_pb_attn_q       a workgroup per query tile: the softmax again (two passes, as the forward), D, dS, dq; keeps max, sum, D
//     k_pb_attn_kv      a workgroup per KEY tile that walks the query tiles in order: dk, dv (one writer, no atomics)
//     k_pb_inproj       dy_i += dqkv in_proj
//   k_pb_attr           the attribute MLP again and back; grad_tree = d emb[128:]
// = 1 + 3 * 4 + 1 = 14 launches on one stream.
//
// A forward layer is recomputed with fph_mm itself (the forward's order of operations, bias last), so a pre-activation has the
// forward's bits.  The lane that owns an element of a layer's output in the forward owns the same element of that layer's dZ in
// the backward (fph_mm and fpb_mmT give a wave the same 32 x 32 blocks), so g'(z) waits for its dZ in that element's slot of the
// rows, written and read back by the same lane.  dX = dZ W is the transposed product: lane l holds the A operand of row l & 31
// (16 contiguous floats of its dZ row in LDS) and column l & 31 of 16 weight rows (coalesced over the 32 lanes).
//
// From fl_policy_head.h: the coordinates (FphLane, FphRows, FphAttnTile), the attribute tile and first layer (fph_load_attr,
// fph_mm_attr) and the attention's pieces (fph_scores, fph_row_max / fph_row_sum, fph_ptile_mm).  Here: the transposed product
// fpb_mmT, a recomputed layer's and a dZ layer's write-back (fpb_fwd_out, fpb_bwd_out), and fpb_store2 for a transposed product
// that goes straight to the rows.
#pragma once
#include "fl_policy_head.h"

#define FPB_QSTRIDE 772             // LDS row stride of a [32][768] tile (4 mod 32, as 260)
#define FPB_STATS 12                // workspace floats a row: (max, sum, D) of the row's query in each of the 4 heads
                                    // (FPB_SAVED_FLOATS, FPB_ROW_FLOATS: fl_policy_layout.h)

struct FpbArgs {
    int B, A, R;
    const float *attr;
    const float *p[FPH_NPARAMS];
    const float *y[4], *ao[3], *qkv[3];                          // saved: y[0] = emb, y[1], y[2], y[3]; c_i; q k v of block i
    const float *gl, *gv;                                        // upstream (either may be NULL)
    float *gtree;
    float *a_dz[4], *a_h[3];                                     // rows: attribute MLP
    float *dqkv[3], *dout[3], *dz[3], *o[3], *dc[3], *dy[4];     // rows: blocks; dy[i] = gradient on y[i]
    float *h_dz[2][3], *h_h[2][2];                               // rows: actor (0), critic (1)
    float *stats;                                                // workspace
};

__device__ __forceinline__ float fpb_dgelu(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * (expf(-0.5f * z * z) * 0.39894228040143267794f);
}

// the wave's two blocks of a transposed product: acc[n] += dZ[row][j] * W[j][k0 + 32 n + col] over j in [0, J), J a multiple of
// 32: dz = the LDS tile of dZ (`stride` floats a row), w = W + k0, ld floats a row of W
__device__ __forceinline__ void fpb_mmT(const float *dz, int stride, int J, const float *w, int ld, fl_f32x16 (&acc)[2], const FphLane L) {
    constexpr int NB = 2;
    const float *dzrow = dz + L.col * stride, *const wc[NB] = {w + L.col, w + 32 + L.col};
#pragma unroll 1
    for (int jc = 0; jc < J; jc += 32) {
        const int o = jc + 16 * L.hh;
        float a[16], b[NB][16];
        fl_ld16(dzrow + o, a);
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int n = 0; n < NB; n++) b[n][s] = wc[n][(size_t)(o + s) * ld];
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int n = 0; n < NB; n++) acc[n] = fl_mfma(a[s], b[n][s], acc[n]);
    }
}

// a recomputed 256-wide layer, the wave's two blocks: z = acc + bias; GELU(z) -> the LDS tile and the rows' X; g'(z) -> the
// layer's dZ slot.  xg and slot point at the tile's first row (ld floats a row).
__device__ __forceinline__ void fpb_fwd_out(const fl_f32x16 (&acc)[2], const float *bias, float *lds, float *xg, float *slot, int ld, int rows,
                                            const FphLane L) {
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int c = 64 * L.wave + 32 * n + L.col;
        const float b = bias[c];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = fl_acc_row(r, L.hh);
            const float z = acc[n][r] + b, h = fph_gelu(z);
            lds[row * FPH_STRIDE + c] = h;
            if (row < rows) {
                xg[(size_t)row * ld + c] = h;
                slot[(size_t)row * ld + c] = fpb_dgelu(z);
            }
        }
    }
}

// dZ = acc * g'(z) (waiting in the slot) of the wave's two blocks -> the LDS tile and the slot; rows past the tile's last are zero in LDS
__device__ __forceinline__ void fpb_bwd_out(const fl_f32x16 (&acc)[2], float *lds, float *slot, int ld, int rows, const FphLane L) {
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int c = 64 * L.wave + 32 * n + L.col;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = fl_acc_row(r, L.hh);
            float d = 0.f;
            if (row < rows) {
                d = acc[n][r] * slot[(size_t)row * ld + c];
                slot[(size_t)row * ld + c] = d;
            }
            lds[row * FPH_STRIDE + c] = d;
        }
    }
}

// the wave's two blocks of a transposed product -> 64 columns of the global rows below `rows`, dst = the first of them in row 0
// (ld floats a row); add: added to what is there
__device__ __forceinline__ void fpb_store2(const fl_f32x16 (&acc)[2], float *dst, int ld, int rows, bool add, const FphLane L) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = fl_acc_row(r, L.hh);
        if (row < rows) {
            float *d = dst + (size_t)row * ld + L.col;
            d[0] = add ? d[0] + acc[0][r] : acc[0][r];
            d[32] = add ? d[32] + acc[1][r] : acc[1][r];
        }
    }
}

// ---- the heads: d both from the upstream gradients
__global__ void __launch_bounds__(FPH_THREADS) k_pb_heads(FpbArgs p) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    __shared__ float s_g[FPH_ROWS][8];
    float *te = s_f, *ty = s_f + FPH_ROWS * FPH_STRIDE, *t2 = s_f + 2 * FPH_ROWS * FPH_STRIDE, *t3 = s_f + 3 * FPH_ROWS * FPH_STRIDE;
    const FphLane L{};
    const FphRows T{p.R};

    fph_load_tile(te, 0, p.y[0] + (size_t)T.row0 * FPH_E, FPH_E, FPH_E / 4, T.rows, L);
    fph_load_tile(ty, 0, p.y[3] + (size_t)T.row0 * FPH_E, FPH_E, FPH_E / 4, T.rows, L);
    bool first = true;
#pragma unroll 1
    for (int hd = 0; hd < 2; hd++) {
        if (hd == 0 ? !p.gl : !p.gv) continue;
        const float *const *w = p.p + (hd ? FPH_P_CRITIC : FPH_P_ACTOR);
        const int nout = hd ? 1 : FPH_ACT, pad = hd ? 4 : 8;
        float *dz0 = p.h_dz[hd][0] + (size_t)T.row0 * FPH_E, *dz2 = p.h_dz[hd][1] + (size_t)T.row0 * FPH_H;
        {                                                        // the gradient on the last layer's output: the upstream itself
            const int r = L.tid >> 3, j = L.tid & 7;
            float v = 0.f;
            if (r < T.rows && j < nout) v = hd ? p.gv[(T.row0 + r) / p.A] / (float)p.A : p.gl[(size_t)(T.row0 + r) * FPH_ACT + j];
            s_g[r][j] = v;
            if (r < T.rows && j < pad) p.h_dz[hd][2][(size_t)(T.row0 + r) * pad + j] = v;
        }
        __syncthreads();
        {                                                        // layer 0 again: h1 -> t2 and the rows, g' -> dz0's slot
            fl_f32x16 acc[2] = {};
            fph_layer256(te, FPH_E, ty, FPH_E, w[0], acc, L);
            fpb_fwd_out(acc, w[1], t2, p.h_h[hd][0] + (size_t)T.row0 * FPH_E, dz0, FPH_E, T.rows, L);
        }
        __syncthreads();
        {                                                        // layer 2 again: h2 -> the rows; dz2 = (dz4 W4) g'(z2) -> t2[:, :128]
            const int f = 32 * L.wave + L.col;
            const float *const ws[1] = {w[2] + (size_t)f * FPH_E};
            fl_f32x16 acc[1] = {};
            fph_mm<1>(t2 + L.col * FPH_STRIDE, FPH_E, ws, acc, L);
            const float b = w[3][f];
            float w4[FPH_ACT];
            for (int j = 0; j < FPH_ACT; j++) w4[j] = j < nout ? w[4][(size_t)j * FPH_H + f] : 0.f;
            float *h2 = p.h_h[hd][1] + (size_t)T.row0 * FPH_H;
            __syncthreads();                                     // every wave has read h1
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, L.hh);
                const float z = acc[0][r] + b;
                float s = 0.f;
                for (int j = 0; j < FPH_ACT; j++) s += s_g[row][j] * w4[j];
                const float d = row < T.rows ? s * fpb_dgelu(z) : 0.f;
                t2[row * FPH_STRIDE + f] = d;
                if (row < T.rows) {
                    h2[(size_t)row * FPH_H + f] = fph_gelu(z);
                    dz2[(size_t)row * FPH_H + f] = d;
                }
            }
        }
        __syncthreads();
        {                                                        // dz0 = (dz2 W2) g'(z1) -> t3
            fl_f32x16 acc[2] = {};
            fpb_mmT(t2, FPH_STRIDE, FPH_H, w[2] + 64 * L.wave, FPH_E, acc, L);
            fpb_bwd_out(acc, t3, dz0, FPH_E, T.rows, L);
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < 2; t++) {                            // d both = dz0 W0: columns 0 .. 255 -> d emb, 256 .. 511 -> dy_3
            const int k0 = 32 * (4 * L.wave + 2 * t);
            fl_f32x16 acc[2] = {};
            fpb_mmT(t3, FPH_STRIDE, FPH_E, w[0] + k0, 2 * FPH_E, acc, L);
            float *dst = (k0 < FPH_E ? p.dy[0] + k0 : p.dy[3] + (k0 - FPH_E)) + (size_t)T.row0 * FPH_E;
            fpb_store2(acc, dst, FPH_E, T.rows, !first, L);       // the critic's after the actor's
        }
        __syncthreads();
        first = false;
    }
}

// ---- block i after its attention, backwards: dy_{i+1} -> dz, dy_i (att_mlp's half; block 0: added to the heads'), do, dc
__global__ void __launch_bounds__(FPH_THREADS) k_pb_block(FpbArgs p, int blk) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    float *bx = s_f, *ba = s_f + FPH_ROWS * FPH_STRIDE, *bz = s_f + 2 * FPH_ROWS * FPH_STRIDE;
    const FphLane L{};
    const FphRows T{p.R};
    const float *const *w = p.p + FPH_P_BLOCK + 6 * blk;
    const size_t t0 = (size_t)T.row0 * FPH_E;

    fph_load_tile(bx, 0, p.y[blk] + t0, FPH_E, FPH_E / 4, T.rows, L);
    fph_load_tile(ba, 0, p.ao[blk] + t0, FPH_E, FPH_E / 4, T.rows, L);
    __syncthreads();
    {                                                            // out_proj again: o -> ba and the rows
        fl_f32x16 acc[2] = {};
        fph_layer256(ba, FPH_E, nullptr, 0, w[2], acc, L);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int c = 64 * L.wave + 32 * n + L.col;
            const float b = w[3][c];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, L.hh);
                const float v = acc[n][r] + b;
                ba[row * FPH_STRIDE + c] = v;
                if (row < T.rows) p.o[blk][t0 + (size_t)row * FPH_E + c] = v;
            }
        }
    }
    __syncthreads();
    {                                                            // att_mlp again: dz = dy_{i+1} g'(z) -> bz and the rows
        fl_f32x16 acc[2] = {};
        fph_layer256(bx, FPH_E, ba, FPH_E, w[4], acc, L);
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int c = 64 * L.wave + 32 * n + L.col;
            const float b = w[5][c];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, L.hh);
                float d = 0.f;
                if (row < T.rows) {
                    d = p.dy[blk + 1][t0 + (size_t)row * FPH_E + c] * fpb_dgelu(acc[n][r] + b);
                    p.dz[blk][t0 + (size_t)row * FPH_E + c] = d;
                }
                bz[row * FPH_STRIDE + c] = d;
            }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < 2; t++) {                                // d [y | o] = dz W_m: waves 0, 1 -> dy_i, waves 2, 3 -> do (ba and the rows)
        const int k0 = 32 * (4 * L.wave + 2 * t);
        fl_f32x16 acc[2] = {};
        fpb_mmT(bz, FPH_STRIDE, FPH_E, w[4] + k0, 2 * FPH_E, acc, L);
        const bool left = k0 < FPH_E;
        const int c0 = left ? k0 : k0 - FPH_E;
        fpb_store2(acc, (left ? p.dy[blk] : p.dout[blk]) + t0 + c0, FPH_E, T.rows, left && blk == 0, L);     // y_0 = emb: after the heads' share
        if (!left) {                                             // do, zero past the tile's last row (o has been read: the barrier above)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = fl_acc_row(r, L.hh);
                ba[row * FPH_STRIDE + c0 + L.col] = row < T.rows ? acc[0][r] : 0.f;
                ba[row * FPH_STRIDE + c0 + 32 + L.col] = row < T.rows ? acc[1][r] : 0.f;
            }
        }
    }
    __syncthreads();
    {                                                            // dc = do W_o
        fl_f32x16 acc[2] = {};
        fpb_mmT(ba, FPH_STRIDE, FPH_E, w[2] + 64 * L.wave, FPH_E, acc, L);
        fpb_store2(acc, p.dc[blk] + t0 + 64 * L.wave, FPH_E, T.rows, false, L);
    }
}

// ---- attention of block i, backwards, the queries' side: workgroup = (env, tile of 32 queries), wave = head.  The forward's two
// passes over the keys (row maxima, then the sums of exp((s - max) / 8)), then two more with P = e / sum and dP = dC V^T:
// D = rowsum(P dP), then dS = P (dP - D) and dq = dS K / 8.  max, sum and D of every (query, head) stay in the workspace.
// D is summed from the very P and dP that dS is made of, not taken as rowsum(dC C): the two are equal in exact arithmetic, but
// only the first keeps sum_k dS = 0 to rounding, and dq = sum_k dS K cancels on that (uniform P over 1 024 keys: 36 x the
// error of torch's float32 softmax backward with rowsum(dC C), 1 x with this).
__global__ void __launch_bounds__(FPH_THREADS) k_pb_attn_q(FpbArgs p, int blk) {
    __shared__ __attribute__((aligned(16))) float s_p[FPH_HEADS][FPH_ROWS * FPH_PSTRIDE];
    const FphLane L{};
    const int A = p.A, head = L.wave;
    const FphAttnTile T{A};
    const float *qkv = p.qkv[blk] + T.base * (3 * FPH_E) + head * FPH_D;     // the head's q of the env's first agent; k at + 256, v at + 512
    float *sp = s_p[head];

    float qa[2][16], da[2][16];                                  // this lane's A operands: q and dC of row first + col
    {
        const size_t qi = (size_t)min(T.first + L.col, A - 1);
        const float *dcrow = p.dc[blk] + (T.base + qi) * FPH_E + head * FPH_D;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fl_ld16(qkv + qi * (3 * FPH_E) + 32 * c + 16 * L.hh, qa[c]);
            fl_ld16(dcrow + 32 * c + 16 * L.hh, da[c]);
        }
    }
    float mx[16], sum[16], D[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { mx[r] = -INFINITY; sum[r] = 0.f; D[r] = 0.f; }
    fl_f32x16 o0 = {}, o1 = {};

#pragma unroll 1
    for (int pass = 0; pass < 4; pass++) {
#pragma unroll 1
        for (int k0 = 0; k0 < A; k0 += 32) {
            const bool live = k0 + L.col < A;
            const float *krow = qkv + (size_t)min(k0 + L.col, A - 1) * (3 * FPH_E) + FPH_E;
            const fl_f32x16 s = fph_scores(qa, krow, L);
            if (pass == 0) {
                if (live) {
#pragma unroll
                    for (int r = 0; r < 16; r++) mx[r] = fmaxf(mx[r], s[r]);
                }
                continue;
            }
            if (pass == 1) {
#pragma unroll
                for (int r = 0; r < 16; r++) sum[r] += live ? expf((s[r] - mx[r]) * 0.125f) : 0.f;
                continue;
            }
            const fl_f32x16 dp = fph_scores(da, krow + FPH_E, L);       // dP = dC V^T
            if (pass == 2) {
#pragma unroll
                for (int r = 0; r < 16; r++) D[r] += live ? expf((s[r] - mx[r]) * 0.125f) / sum[r] * dp[r] : 0.f;
                continue;
            }
            __syncthreads();                                     // the previous chunk's dS has been read
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float pr = live ? expf((s[r] - mx[r]) * 0.125f) / sum[r] : 0.f;
                sp[fl_acc_row(r, L.hh) * FPH_PSTRIDE + L.col] = live ? pr * (dp[r] - D[r]) : 0.f;
            }
            __syncthreads();
            fph_ptile_mm(sp, qkv + FPH_E, 3 * FPH_E, k0, A, L, o0, o1);      // dS K
        }
        if (pass == 0) fph_row_max(mx);
        else if (pass == 1) fph_row_sum(sum);
        else if (pass == 2) fph_row_sum(D);
    }
    float *out = p.dqkv[blk] + T.base * (3 * FPH_E) + head * FPH_D;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int qi = T.first + fl_acc_row(r, L.hh);
        if (qi < A) {
            out[(size_t)qi * (3 * FPH_E) + L.col] = o0[r] * 0.125f;
            out[(size_t)qi * (3 * FPH_E) + 32 + L.col] = o1[r] * 0.125f;
            if (L.col == 0) {
                float *st = p.stats + (T.base + qi) * FPB_STATS + 3 * head;
                st[0] = mx[r]; st[1] = sum[r]; st[2] = D[r];
            }
        }
    }
}

// ---- the keys' side: workgroup = (env, tile of 32 KEYS), wave = head; the query tiles in increasing order.  Transposed tiles:
// rows = keys, columns = queries.  P^T = exp((k q^T - max_q) / 8) / sum_q, dP^T = V dC^T, dS^T = P^T (dP^T - D_q),
// dv = sum_q P^T dC, dk = sum_q dS^T Q / 8.
__global__ void __launch_bounds__(FPH_THREADS) k_pb_attn_kv(FpbArgs p, int blk) {
    __shared__ __attribute__((aligned(16))) float s_p[FPH_HEADS][2][FPH_ROWS * FPH_PSTRIDE];
    const FphLane L{};
    const int A = p.A, head = L.wave;
    const FphAttnTile T{A};
    const float *qkv = p.qkv[blk] + T.base * (3 * FPH_E) + head * FPH_D;
    const float *dc = p.dc[blk] + T.base * FPH_E + head * FPH_D;
    float *spp = s_p[head][0], *sps = s_p[head][1];

    float ka[2][16], va[2][16];                                  // this lane's A operands: k and v of key first + col
    {
        const float *krow = qkv + (size_t)min(T.first + L.col, A - 1) * (3 * FPH_E) + FPH_E;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            fl_ld16(krow + 32 * c + 16 * L.hh, ka[c]);
            fl_ld16(krow + FPH_E + 32 * c + 16 * L.hh, va[c]);
        }
    }
    fl_f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};
#pragma unroll 1
    for (int q0 = 0; q0 < A; q0 += 32) {
        const bool live = q0 + L.col < A;                        // this lane's query (column)
        const size_t qi = (size_t)min(q0 + L.col, A - 1);
        const float *qrow = qkv + qi * (3 * FPH_E), *dcrow = dc + qi * FPH_E;
        const float *st = p.stats + (T.base + qi) * FPB_STATS + 3 * head;
        const float mx = st[0], sum = st[1], D = st[2];
        fl_f32x16 s = {}, dp = {};                               // the two products in one loop, step by step (see below)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            float qb[16], db[16];
            fl_ld16(qrow + 32 * c + 16 * L.hh, qb);
            fl_ld16(dcrow + 32 * c + 16 * L.hh, db);
#pragma unroll
            for (int t = 0; t < 16; t++) { s = fl_mfma(ka[c][t], qb[t], s); dp = fl_mfma(va[c][t], db[t], dp); }
        }
        __syncthreads();                                         // the previous tile's P^T and dS^T have been read
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float pr = live ? expf((s[r] - mx) * 0.125f) / sum : 0.f;
            spp[fl_acc_row(r, L.hh) * FPH_PSTRIDE + L.col] = pr;
            sps[fl_acc_row(r, L.hh) * FPH_PSTRIDE + L.col] = live ? pr * (dp[r] - D) : 0.f;
        }
        __syncthreads();
        // P^T dC and dS^T Q likewise, not as two fph_ptile_mm (nor two fph_scores above): one after the other they compile to other
        // code, and the build that had them so took 3 % longer over the whole backward at 400 agents
        float pa[16], sa[16];
        fl_ld16(spp + L.col * FPH_PSTRIDE + 16 * L.hh, pa);
        fl_ld16(sps + L.col * FPH_PSTRIDE + 16 * L.hh, sa);
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int qq = q0 + 16 * L.hh + t;
            float c0 = 0.f, c1 = 0.f, x0 = 0.f, x1 = 0.f;
            if (qq < A) {
                const float *cr = dc + (size_t)qq * FPH_E, *qr = qkv + (size_t)qq * (3 * FPH_E);
                c0 = cr[L.col]; c1 = cr[32 + L.col]; x0 = qr[L.col]; x1 = qr[32 + L.col];
            }
            dv0 = fl_mfma(pa[t], c0, dv0); dv1 = fl_mfma(pa[t], c1, dv1);
            dk0 = fl_mfma(sa[t], x0, dk0); dk1 = fl_mfma(sa[t], x1, dk1);
        }
    }
    float *out = p.dqkv[blk] + T.base * (3 * FPH_E) + head * FPH_D;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ki = T.first + fl_acc_row(r, L.hh);
        if (ki < A) {
            float *o = out + (size_t)ki * (3 * FPH_E);
            o[FPH_E + L.col] = dk0[r] * 0.125f; o[FPH_E + 32 + L.col] = dk1[r] * 0.125f;
            o[2 * FPH_E + L.col] = dv0[r]; o[2 * FPH_E + 32 + L.col] = dv1[r];
        }
    }
}

// ---- dy_i += dqkv W_in (the third and last share of dy_i)
__global__ void __launch_bounds__(FPH_THREADS) k_pb_inproj(FpbArgs p, int blk) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    const FphLane L{};
    const FphRows T{p.R};
    const float *src = p.dqkv[blk] + (size_t)T.row0 * (3 * FPH_E);
    for (int i = L.tid; i < FPH_ROWS * (3 * FPH_E / 4); i += FPH_THREADS) {
        const int r = i / (3 * FPH_E / 4), q = i % (3 * FPH_E / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < T.rows) v = ((const float4 *)(src + (size_t)r * (3 * FPH_E)))[q];
        *(float4 *)&s_f[r * FPB_QSTRIDE + 4 * q] = v;
    }
    __syncthreads();
    const float *w = p.p[FPH_P_BLOCK + 6 * blk];
    fl_f32x16 acc[2] = {};
    fpb_mmT(s_f, FPB_QSTRIDE, 3 * FPH_E, w + 64 * L.wave, FPH_E, acc, L);
    fpb_store2(acc, p.dy[blk] + (size_t)T.row0 * FPH_E + 64 * L.wave, FPH_E, T.rows, true, L);
}

// ---- the attribute MLP again and backwards; grad_tree = d emb[128:]
__global__ void __launch_bounds__(FPH_THREADS) k_pb_attr(FpbArgs p) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    float *b0 = s_f, *b1 = s_f + FPH_ROWS * FPH_STRIDE;
    const FphLane L{};
    const FphRows T{p.R};
    const size_t t0 = (size_t)T.row0 * FPH_E;

    fph_load_attr(b0, FPH_STRIDE, p.attr, T, L);
    for (int i = L.tid; i < T.rows * (FPH_H / 4); i += FPH_THREADS) {
        const int r = i / (FPH_H / 4), q = i % (FPH_H / 4);
        ((float4 *)(p.gtree + (size_t)(T.row0 + r) * FPH_H))[q] = ((const float4 *)(p.dy[0] + t0 + (size_t)r * FPH_E + FPH_H))[q];
    }
    __syncthreads();
    const float *const *w = p.p + FPH_P_ATTR;
    {
        fl_f32x16 acc[2] = {};
        fph_mm_attr(b0 + L.col * FPH_STRIDE, w[0] + (size_t)(64 * L.wave + L.col) * FPH_ATTR, w[0] + (size_t)(64 * L.wave + 32 + L.col) * FPH_ATTR, acc, L);
        fpb_fwd_out(acc, w[1], b1, p.a_h[0] + t0, p.a_dz[0] + t0, FPH_E, T.rows, L);
    }
    __syncthreads();
    for (int l = 1; l <= 2; l++) {                               // 256 -> 256 twice: b1 -> b0 -> b1
        float *src = l == 1 ? b1 : b0, *dst = l == 1 ? b0 : b1;
        fl_f32x16 acc[2] = {};
        fph_layer256(src, FPH_E, nullptr, 0, w[2 * l], acc, L);
        fpb_fwd_out(acc, w[2 * l + 1], dst, p.a_h[l] + t0, p.a_dz[l] + t0, FPH_E, T.rows, L);
        __syncthreads();
    }
    {                                                            // 256 -> 128 again; dz6 = d emb[:128] g'(z6) -> b0[:, :128]
        const int f = 32 * L.wave + L.col;
        const float *const ws[1] = {w[6] + (size_t)f * FPH_E};
        fl_f32x16 acc[1] = {};
        fph_mm<1>(b1 + L.col * FPH_STRIDE, FPH_E, ws, acc, L);
        const float b = w[7][f];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = fl_acc_row(r, L.hh);
            float d = 0.f;
            if (row < T.rows) {
                d = p.dy[0][t0 + (size_t)row * FPH_E + f] * fpb_dgelu(acc[0][r] + b);
                p.a_dz[3][(size_t)(T.row0 + row) * FPH_H + f] = d;
            }
            b0[row * FPH_STRIDE + f] = d;
        }
    }
    __syncthreads();
    {                                                            // dz4 = (dz6 W6) g'(z4) -> b1
        fl_f32x16 acc[2] = {};
        fpb_mmT(b0, FPH_STRIDE, FPH_H, w[6] + 64 * L.wave, FPH_E, acc, L);
        fpb_bwd_out(acc, b1, p.a_dz[2] + t0, FPH_E, T.rows, L);
    }
    __syncthreads();
    for (int l = 2; l >= 1; l--) {                               // dz2 = (dz4 W4) g'(z2): b1 -> b0; dz0 = (dz2 W2) g'(z0): b0 -> b1
        float *src = l == 2 ? b1 : b0, *dst = l == 2 ? b0 : b1;
        fl_f32x16 acc[2] = {};
        fpb_mmT(src, FPH_STRIDE, FPH_E, w[2 * l] + 64 * L.wave, FPH_E, acc, L);
        fpb_bwd_out(acc, dst, p.a_dz[l - 1] + t0, FPH_E, T.rows, L);
        __syncthreads();
    }
}

#define FPB_LDS_HEADS (4 * FPH_ROWS * FPH_STRIDE * sizeof(float))
#define FPB_LDS_BLOCK (3 * FPH_ROWS * FPH_STRIDE * sizeof(float))
#define FPB_LDS_INPROJ (FPH_ROWS * FPB_QSTRIDE * sizeof(float))
#define FPB_LDS_ATTR (2 * FPH_ROWS * FPH_STRIDE * sizeof(float))
