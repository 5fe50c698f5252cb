// fl_policy_head.h -- the policy network after its tree encoder (solution/nn/net_tree.py:82-103) and the actor's choice of an
// action (solution/plfActor.py:30-46) for a whole batch, float32, gfx950.  Included by fl_policy_head.hip, which holds the entry
// points fl_policy_head / fl_policy_head_workspace_bytes (include/flatland_policy.h).
//
// Rows = the B*A (env, agent) pairs, flattened.  Everything but the attention is independent per row, so a workgroup (4 waves)
// takes a tile of 32 consecutive rows -- which may straddle envs -- and keeps a whole chain of layers in LDS:
//   k_ph_embed          attr MLP (83 -> 256 -> 256 -> 256 -> 128, GELU each) -> embedding [attr | tree] (256) -> q, k, v of block 1
//   k_ph_attn           softmax(q k^T / 8) v of one block: a workgroup per (env, tile of 32 queries), a wave per head
//   k_ph_block<false>   out_proj -> att_mlp = GELU(Linear [input | attention]) = the next block's input -> its q, k, v
//   k_ph_block<true>    out_proj -> att_mlp -> actor_net and critic_net on [embedding | att_mlp] -> logits, a row's critic value,
//                       the action
//   k_ph_value          mean of the critic values over the agents of an env, in a fixed order
// = embed, (attn, block) x 3 and value: 8 launches on one stream (7 without value).
//
// Products are f32-input MFMA (v_mfma_f32_32x32x2_f32, exact f32) as in fl_tree_lstm.h: a wave computes a block of 32 rows x
// 32 output features, lane l holds the A operand of row l & 31 and the weight row of feature l & 31, step s of a 32-wide chunk
// kc takes k = kc + 16 * (l >> 5) + s, so a lane reads 64 contiguous bytes of its weight row (torch's [out][in] layout, straight
// from global memory / L2) and of its LDS row a chunk (row stride 260 floats = 4 mod 32: conflict-free ds_read_b128).  Every sum
// starts from zero and takes the bias last.  A layer's results stay in registers until every wave has read the layer's input,
// so a layer may write over its own input.
//
// What the three policy-head headers share lives here: a thread's coordinates (FphLane), a kernel's row tile (FphRows) and
// attention tile (FphAttnTile), the attribute tile (fph_load_attr), the tail of the last block (fph_put_logits, fph_put_val,
// fph_act) and the float32 attention's pieces (fph_scores, fph_row_max / fph_row_sum, fph_ptile_mm), which fl_policy_head_bwd.h uses too.
#pragma once
#include "fl_internal.h"
#include "fl_mfma.h"
#include "fl_policy_layout.h"       // FPH_ATTR, FPH_H, FPH_E, FPH_ACT, FPH_NPARAMS, FPH_MAX_A

#define FPH_ATTR_PAD 96             // K of the first layer in LDS, zero filled
#define FPH_HEADS 4
#define FPH_D 64                    // head size
#define FPH_THREADS 256
#define FPH_ROWS 32
#define FPH_STRIDE 260
#define FPH_PSTRIDE 36              // a wave's tile of attention probabilities: 32 x 32, row stride 36
#define FPH_ROW_FLOATS (4 * FPH_E + 3 * FPH_E + 1)   // workspace floats a row: embedding, two block outputs, attention, q k v, value

// parameter indices: the Network's state_dict without tree_lstm.*, in state_dict order
enum {
    FPH_P_ATTR = 0,                 // attr_embedding.{0,2,4,6}.{weight,bias}
    FPH_P_BLOCK = 8,                // transformer.i: attention.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, att_mlp.0.weight, .bias
    FPH_P_ACTOR = 26,               // actor_net.{0,2,4}.{weight,bias}
    FPH_P_CRITIC = 32,              // critic_net.{0,2,4}.{weight,bias}
};

struct FphArgs {
    int B, A, R;                    // R = B * A rows
    int select;                     // 0 none, 1 soft, 2 hard
    double u;
    const float *attr, *tree;
    const float *p[FPH_NPARAMS];
    const unsigned char *valid;
    float *logits, *value;
    unsigned char *actions;
    float *emb, *xa, *xb, *ao, *qkv, *val;     // workspace: [R][256] x 4, [R][768], [R]
    float *y3;                                 // the third block's output [R][256], or NULL (inference): fl_policy_head_forward_saved
};

__device__ __forceinline__ float fph_gelu(float x) { return (x * 0.5f) * (1.0f + erff(x * 0.70710678118654752440f)); }

// The three coordinate structs are aggregates whose members initialise themselves: a kernel builds one in a line (`const FphLane
// L{};`, `const FphRows T{p.R};`, `const FphAttnTile T{p.A};`) and the helpers take them by value.  Not a constructor, not a
// reference: either keeps the struct in memory until the inliner has run, and the kernels then compile to other (measured:
// slower) code than with the plain ints that these replace; as written, a kernel that only swaps its ints for a struct compiles
// to the same instructions.
// a thread of a workgroup of 4 waves: its wave (the head, in the attention) and, for the MFMA, its row / column and k half (fl_mfma.h)
struct FphLane {
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
};

// the tile of 32 consecutive rows that workgroup blockIdx.x of a row-tile kernel takes: its first row and how many of R there are
struct FphRows {
    int R, row0 = blockIdx.x * FPH_ROWS, rows = min(FPH_ROWS, R - row0);
};

// the (env, tile of 32 queries or keys) of workgroup blockIdx.x of an attention kernel: first = the tile's first agent, base = the
// env's first row
struct FphAttnTile {
    int A, tiles = (A + FPH_ROWS - 1) / FPH_ROWS, env = blockIdx.x / tiles, first = (blockIdx.x % tiles) * FPH_ROWS;
    size_t base = (size_t)env * A;
};

// acc[b] += X[row][k] * W[j[b]][woff + k] over k in [0, K), K a multiple of 32: xrow = this lane's LDS row, w[b] = its weight row
template <int NB>
__device__ __forceinline__ void fph_mm(const float *xrow, int K, const float *const (&w)[NB], fl_f32x16 (&acc)[NB], const FphLane L) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 32) {
        float a[16], b[NB][16];
        const int o = kc + 16 * L.hh;
        fl_ld16(xrow + o, a);
#pragma unroll
        for (int n = 0; n < NB; n++) fl_ld16(w[n] + o, b[n]);
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int n = 0; n < NB; n++) acc[n] = fl_mfma(a[s], b[n][s], acc[n]);
    }
}

// the attribute tile of a row tile: 32 rows of `stride` floats, 83 attributes zero filled up to 96 (rows past the tile's last: zero)
__device__ __forceinline__ void fph_load_attr(float *dst, int stride, const float *attr, const FphRows T, const FphLane L) {
    for (int i = L.tid; i < FPH_ROWS * FPH_ATTR_PAD; i += FPH_THREADS) {
        const int r = i / FPH_ATTR_PAD, c = i % FPH_ATTR_PAD;
        dst[r * stride + c] = (r < T.rows && c < FPH_ATTR) ? attr[(size_t)(T.row0 + r) * FPH_ATTR + c] : 0.f;
    }
}

// the first layer over that tile, the wave's two blocks: xrow = this lane's row of the tile, w0 / w1 = its weight rows of 83 floats
// (no 16-byte alignment) in the two blocks
__device__ __forceinline__ void fph_mm_attr(const float *xrow, const float *w0, const float *w1, fl_f32x16 (&acc)[2], const FphLane L) {
#pragma unroll 1
    for (int kc = 0; kc < FPH_ATTR_PAD; kc += 32) {
        const int o = kc + 16 * L.hh;
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int k = o + s;
            const float a = xrow[k];
            const float b0 = k < FPH_ATTR ? w0[k] : 0.f, b1 = k < FPH_ATTR ? w1[k] : 0.f;
            acc[0] = fl_mfma(a, b0, acc[0]);
            acc[1] = fl_mfma(a, b1, acc[1]);
        }
    }
}

// (acc + bias[c0 + col]) [GELU] of one 32 x 32 block -> LDS columns c0 .. c0 + 31 (a 128-wide layer: c0 = 32 wave)
template <bool GELU>
__device__ __forceinline__ void fph_to_lds(const fl_f32x16 &acc, const float *bias, float *dst, int c0, const FphLane L) {
    const float b = bias[c0 + L.col];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float v = acc[r] + b;
        dst[fl_acc_row(r, L.hh) * FPH_STRIDE + c0 + L.col] = GELU ? fph_gelu(v) : v;
    }
}

// a 256-wide layer: the wave's two blocks, columns 64 wave .. 64 wave + 63
template <bool GELU>
__device__ __forceinline__ void fph_to_lds(const fl_f32x16 (&acc)[2], const float *bias, float *dst, const FphLane L) {
    fph_to_lds<GELU>(acc[0], bias, dst, 64 * L.wave, L);
    fph_to_lds<GELU>(acc[1], bias, dst, 64 * L.wave + 32, L);
}

// rows [0, rows) x 64 float4 of an LDS tile <-> global rows of ld floats (rows past `rows` read as zero)
__device__ __forceinline__ void fph_load_tile(float *dst, int c0, const float *src, int ld, int nq, int rows, const FphLane L) {
    for (int i = L.tid; i < FPH_ROWS * nq; i += FPH_THREADS) {
        const int r = i / nq, q = i % nq;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows) v = ((const float4 *)(src + (size_t)r * ld))[q];
        *(float4 *)&dst[r * FPH_STRIDE + c0 + 4 * q] = v;
    }
}

__device__ __forceinline__ void fph_store_tile(const float *src, float *dst, int rows, const FphLane L) {
    for (int i = L.tid; i < FPH_ROWS * (FPH_E / 4); i += FPH_THREADS) {
        const int r = i / (FPH_E / 4), q = i % (FPH_E / 4);
        if (r < rows) ((float4 *)(dst + (size_t)r * FPH_E))[q] = *(const float4 *)&src[r * FPH_STRIDE + 4 * q];
    }
}

// q, k, v of the next block: [rows][768] = X[32][256] in_proj^T + bias, straight to global memory (6 blocks a wave, in pairs)
__device__ __forceinline__ void fph_qkv(const float *x, const float *w, const float *bias, float *out, int rows, const FphLane L) {
    const int col = L.col;
#pragma unroll 1
    for (int pr = 0; pr < 3; pr++) {
        const int j0 = 32 * (6 * L.wave + 2 * pr), j1 = j0 + 32;
        const float *const ws[2] = {w + (size_t)(j0 + col) * FPH_E, w + (size_t)(j1 + col) * FPH_E};
        fl_f32x16 acc[2] = {};
        fph_mm<2>(x + col * FPH_STRIDE, FPH_E, ws, acc, L);
        const float b0 = bias[j0 + col], b1 = bias[j1 + col];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = fl_acc_row(r, L.hh);
            if (row < rows) {
                out[(size_t)row * (3 * FPH_E) + j0 + col] = acc[0][r] + b0;
                out[(size_t)row * (3 * FPH_E) + j1 + col] = acc[1][r] + b1;
            }
        }
    }
}

// Y[32][256] = [GELU](X0[32][K0] | X1[32][K1]) W^T + bias: the wave's two blocks, left in registers (bias and GELU: fph_to_lds)
__device__ __forceinline__ void fph_layer256(const float *x0, int K0, const float *x1, int K1, const float *w, fl_f32x16 (&acc)[2],
                                             const FphLane L) {
    const int ld = K0 + K1, j0 = 64 * L.wave, j1 = j0 + 32, col = L.col;
    const float *const ws[2] = {w + (size_t)(j0 + col) * ld, w + (size_t)(j1 + col) * ld};
    fph_mm<2>(x0 + col * FPH_STRIDE, K0, ws, acc, L);
    if (K1) {
        const float *const ws1[2] = {ws[0] + K0, ws[1] + K0};
        fph_mm<2>(x1 + col * FPH_STRIDE, K1, ws1, acc, L);
    }
}

// a head's last layer, 128 -> n_out (n_out <= 32), exact float32 on wave 0, the float32 and the bf16 head's: h = the hidden tile
// (`stride` floats a row); bias added
__device__ __forceinline__ void fph_head_out(const float *h, int stride, const float *w, const float *bias, int n_out, fl_f32x16 &out,
                                             const FphLane L) {
    if (L.wave != 0) return;
    const int j = min(L.col, n_out - 1);                         // (columns past n_out repeat the last feature and are dropped)
    const float *const ws[1] = {w + (size_t)j * FPH_H};
    fl_f32x16 acc[1] = {};
    fph_mm<1>(h + L.col * stride, FPH_H, ws, acc, L);
    const float b = bias[j];
#pragma unroll
    for (int r = 0; r < 16; r++) out[r] = acc[0][r] + b;
}

// a 512 -> 256 -> 128 -> n_out head (actor_net / critic_net) on [e | y]: the result of rows x n_out (n_out <= 32) in wave 0's acc
// registers, bias added; h is scratch.  Every wave calls it (barriers inside).
__device__ __forceinline__ void fph_head(const float *e, const float *y, float *h, const float *const *p, int n_out, fl_f32x16 &out,
                                         const FphLane L) {
    const int wave = L.wave, col = L.col;
    {
        fl_f32x16 acc[2] = {};
        fph_layer256(e, FPH_E, y, FPH_E, p[0], acc, L);
        __syncthreads();                                         // (h may still be read by the head before this one)
        fph_to_lds<true>(acc, p[1], h, L);
    }
    __syncthreads();
    {
        const float *const ws[1] = {p[2] + (size_t)(32 * wave + col) * FPH_E};
        fl_f32x16 acc[1] = {};
        fph_mm<1>(h + col * FPH_STRIDE, FPH_E, ws, acc, L);
        __syncthreads();
        fph_to_lds<true>(acc[0], p[3], h, 32 * wave, L);
    }
    __syncthreads();
    fph_head_out(h, FPH_STRIDE, p[4], p[5], n_out, out, L);
}

// Actor._choose_action (plfActor.py:30-46) on one agent's logits and valid-action mask.  The softmax over the valid logits in
// float32, as numpy computes it on a float32 array (max, exp, a sum from the left, the division).  soft: np.random.choice with
// the draw u: the float64 cumulative sum of p divided by its last element, searchsorted(u, side="right").  hard: the first
// largest p.  No valid action: 0.
__device__ __forceinline__ int fph_choose(const float *lg, const unsigned char *valid, int select, double u) {
    int idx[FPH_ACT], n = 0;
    float x[FPH_ACT];
    for (int a = 0; a < FPH_ACT; a++)
        if (valid[a]) { idx[n] = a; x[n] = lg[a]; n++; }
    if (n == 0) return 0;
    float m = x[0];
    for (int i = 1; i < n; i++) m = fmaxf(m, x[i]);
    float e[FPH_ACT], s = 0.f;
    for (int i = 0; i < n; i++) { e[i] = expf(x[i] - m); s = i ? s + e[i] : e[i]; }
    float pr[FPH_ACT];
    for (int i = 0; i < n; i++) pr[i] = e[i] / s;
    if (select == 2) {
        int best = 0;
        for (int i = 1; i < n; i++) if (pr[i] > pr[best]) best = i;
        return idx[best];
    }
    double cdf[FPH_ACT], c = 0.0;
    for (int i = 0; i < n; i++) { c = i ? c + (double)pr[i] : (double)pr[i]; cdf[i] = c; }
    int k = 0;
    for (int i = 0; i < n; i++) k += (cdf[i] / c) <= u;
    return idx[min(k, n - 1)];
}

// ---- attr MLP, embedding, q k v of the first block
__global__ void __launch_bounds__(FPH_THREADS) k_ph_embed(FphArgs p) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    float *b0 = s_f, *b1 = s_f + FPH_ROWS * FPH_STRIDE;
    const FphLane L{};
    const FphRows T{p.R};

    fph_load_attr(b0, FPH_STRIDE, p.attr, T, L);
    __syncthreads();
    const float *const *w = p.p + FPH_P_ATTR;
    {
        fl_f32x16 acc[2] = {};
        fph_mm_attr(b0 + L.col * FPH_STRIDE, w[0] + (size_t)(64 * L.wave + L.col) * FPH_ATTR, w[0] + (size_t)(64 * L.wave + 32 + L.col) * FPH_ATTR, acc, L);
        fph_to_lds<true>(acc, w[1], b1, L);
    }
    __syncthreads();
    for (int l = 1; l <= 2; l++) {                               // 256 -> 256 twice: b1 -> b0 -> b1
        float *src = l == 1 ? b1 : b0, *dst = l == 1 ? b0 : b1;
        fl_f32x16 acc[2] = {};
        fph_layer256(src, FPH_E, nullptr, 0, w[2 * l], acc, L);
        fph_to_lds<true>(acc, w[2 * l + 1], dst, L);
        __syncthreads();
    }
    {                                                            // 256 -> 128: b1 -> b0[:, :128]; the tree embedding beside it
        const float *const ws[1] = {w[6] + (size_t)(32 * L.wave + L.col) * FPH_E};
        fl_f32x16 acc[1] = {};
        fph_mm<1>(b1 + L.col * FPH_STRIDE, FPH_E, ws, acc, L);
        fph_to_lds<true>(acc[0], w[7], b0, 32 * L.wave, L);
        fph_load_tile(b0, FPH_H, p.tree + (size_t)T.row0 * FPH_H, FPH_H, FPH_H / 4, T.rows, L);
    }
    __syncthreads();
    fph_store_tile(b0, p.emb + (size_t)T.row0 * FPH_E, T.rows, L);
    fph_qkv(b0, p.p[FPH_P_BLOCK], p.p[FPH_P_BLOCK + 1], p.qkv + (size_t)T.row0 * (3 * FPH_E), T.rows, L);
}

// ---- the float32 attention's pieces, for k_ph_attn here and k_pb_attn_q / k_pb_attn_kv of fl_policy_head_bwd.h
// a chunk of scores, s = a b^T over a head's 64 features: a = this lane's row of A as fl_ld16 left it (2 chunks x the 16 of its k
// half), brow = the 64 features of this lane's column
__device__ __forceinline__ fl_f32x16 fph_scores(const float (&a)[2][16], const float *brow, const FphLane L) {
    fl_f32x16 s = {};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        float b[16];
        fl_ld16(brow + 32 * c + 16 * L.hh, b);
#pragma unroll
        for (int t = 0; t < 16; t++) s = fl_mfma(a[c][t], b[t], s);
    }
    return s;
}

// a row's maximum / sum over the 32 lanes that hold its columns (a butterfly: every lane ends with the same value)
__device__ __forceinline__ void fph_row_max(float (&v)[16]) {
#pragma unroll
    for (int r = 0; r < 16; r++)
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) v[r] = fmaxf(v[r], __shfl_xor(v[r], d, 64));
}

__device__ __forceinline__ void fph_row_sum(float (&v)[16]) {
#pragma unroll
    for (int r = 0; r < 16; r++)
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) v[r] = v[r] + __shfl_xor(v[r], d, 64);
}

// o0, o1 += P M: P = the wave's 32 x 32 tile in LDS (row stride 36), M = rows first .. first + 31 of a matrix of ld floats a row,
// its columns col and 32 + col; rows past A read as zero
__device__ __forceinline__ void fph_ptile_mm(const float *sp, const float *mat, int ld, int first, int A, const FphLane L, fl_f32x16 &o0,
                                             fl_f32x16 &o1) {
    float pa[16];
    fl_ld16(sp + L.col * FPH_PSTRIDE + 16 * L.hh, pa);
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const int i = first + 16 * L.hh + t;
        float v0 = 0.f, v1 = 0.f;
        if (i < A) {
            const float *row = mat + (size_t)i * ld;
            v0 = row[L.col]; v1 = row[32 + L.col];
        }
        o0 = fl_mfma(pa[t], v0, o0);
        o1 = fl_mfma(pa[t], v1, o1);
    }
}

// ---- attention of one block: workgroup = (env, tile of 32 queries), wave = head.  Two passes over the keys in chunks of 32: the
// row maxima of q k^T, then p = exp((s - max) / 8) (the scale 1/8 is a power of two: where it is applied does not change the
// rounding), its row sums and p v; the quotient last.  Keys past the env's last agent take no part.
__global__ void __launch_bounds__(FPH_THREADS) k_ph_attn(FphArgs p) {
    __shared__ __attribute__((aligned(16))) float s_p[FPH_HEADS][FPH_ROWS * FPH_PSTRIDE];
    const FphLane L{};
    const int A = p.A, head = L.wave;
    const FphAttnTile T{A};
    const float *qkv = p.qkv + T.base * (3 * FPH_E) + head * FPH_D;      // the head's q of the env's first agent; k at + 256, v at + 512
    float *sp = s_p[head];

    float qa[2][16];                                             // this lane's A operand: q of row first + col (the last one repeated past the env)
#pragma unroll
    for (int c = 0; c < 2; c++) fl_ld16(qkv + (size_t)min(T.first + L.col, A - 1) * (3 * FPH_E) + 32 * c + 16 * L.hh, qa[c]);
    float mx[16], sum[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { mx[r] = -INFINITY; sum[r] = 0.f; }
    fl_f32x16 o0 = {}, o1 = {};

#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
        for (int k0 = 0; k0 < A; k0 += 32) {
            const bool live = k0 + L.col < A;                     // this lane's key (score column)
            const fl_f32x16 s = fph_scores(qa, qkv + (size_t)min(k0 + L.col, A - 1) * (3 * FPH_E) + FPH_E, L);
            if (pass == 0) {
                if (live) {
#pragma unroll
                    for (int r = 0; r < 16; r++) mx[r] = fmaxf(mx[r], s[r]);
                }
                continue;
            }
            __syncthreads();                                     // the previous chunk's probabilities have been read
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float e = live ? expf((s[r] - mx[r]) * 0.125f) : 0.f;
                sum[r] += e;
                sp[fl_acc_row(r, L.hh) * FPH_PSTRIDE + L.col] = e;
            }
            __syncthreads();
            fph_ptile_mm(sp, qkv + 2 * FPH_E, 3 * FPH_E, k0, A, L, o0, o1);
        }
        if (pass == 0) fph_row_max(mx); else fph_row_sum(sum);
    }
    float *out = p.ao + T.base * FPH_E + head * FPH_D;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int qi = T.first + fl_acc_row(r, L.hh);
        if (qi < A) {
            out[(size_t)qi * FPH_E + L.col] = o0[r] / sum[r];
            out[(size_t)qi * FPH_E + 32 + L.col] = o1[r] / sum[r];
        }
    }
}

// the tail of the last block, float32 and bf16, in three pieces around the kernel's own calls of its head function (a function
// template that took the head as a callable compiled k_ph_block<true> to 97 VGPRs for 67 and one wave a SIMD less).
// wave 0's head output (fph_head) -> the logits in s_lg and in global memory
__device__ __forceinline__ void fph_put_logits(const fl_f32x16 &out, float (&s_lg)[FPH_ROWS][FPH_ACT + 1], float *logits, const FphRows T,
                                               const FphLane L) {
    if (L.wave != 0 || L.col >= FPH_ACT) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = fl_acc_row(r, L.hh);
        s_lg[row][L.col] = out[r];
        if (row < T.rows) logits[(size_t)(T.row0 + row) * FPH_ACT + L.col] = out[r];
    }
}

// ... of the critic -> the rows' values
__device__ __forceinline__ void fph_put_val(const fl_f32x16 &out, float *val, const FphRows T, const FphLane L) {
    if (L.wave != 0 || L.col != 0) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = fl_acc_row(r, L.hh);
        if (row < T.rows) val[T.row0 + row] = out[r];
    }
}

// the barrier behind the logits, then a thread a row chooses the action
__device__ __forceinline__ void fph_act(const float (&s_lg)[FPH_ROWS][FPH_ACT + 1], const FphArgs &p, const FphRows T, const FphLane L) {
    __syncthreads();
    if (p.select && L.tid < T.rows)
        p.actions[T.row0 + L.tid] = (unsigned char)fph_choose(s_lg[L.tid], p.valid + (size_t)(T.row0 + L.tid) * FPH_ACT, p.select, p.u);
}

// ---- the rest of a block per row tile; LAST: the heads and the action instead of the next block's q k v
template <bool LAST>
__global__ void __launch_bounds__(FPH_THREADS) k_ph_block(FphArgs p, int blk, const float *xin, float *xout) {
    extern __shared__ __attribute__((aligned(16))) float s_f[];
    __shared__ float s_lg[FPH_ROWS][FPH_ACT + 1];
    float *bx = s_f, *ba = s_f + FPH_ROWS * FPH_STRIDE, *bh = s_f + 2 * FPH_ROWS * FPH_STRIDE;     // (bh: LAST only)
    const FphLane L{};
    const FphRows T{p.R};
    const float *const *w = p.p + FPH_P_BLOCK + 6 * blk;
    const size_t t0 = (size_t)T.row0 * FPH_E;

    fph_load_tile(bx, 0, xin + t0, FPH_E, FPH_E / 4, T.rows, L);
    fph_load_tile(ba, 0, p.ao + t0, FPH_E, FPH_E / 4, T.rows, L);
    __syncthreads();
    {                                                            // out_proj, over the attention output
        fl_f32x16 acc[2] = {};
        fph_layer256(ba, FPH_E, nullptr, 0, w[2], acc, L);
        __syncthreads();
        fph_to_lds<false>(acc, w[3], ba, L);
    }
    __syncthreads();
    {                                                            // att_mlp on [input | attention], over the input
        fl_f32x16 acc[2] = {};
        fph_layer256(bx, FPH_E, ba, FPH_E, w[4], acc, L);
        __syncthreads();
        fph_to_lds<true>(acc, w[5], bx, L);
    }
    __syncthreads();
    if (!LAST) {
        fph_store_tile(bx, xout + t0, T.rows, L);
        fph_qkv(bx, w[6], w[7], p.qkv + (size_t)T.row0 * (3 * FPH_E), T.rows, L);
        return;
    }
    fph_load_tile(ba, 0, p.emb + t0, FPH_E, FPH_E / 4, T.rows, L);
    if (p.y3) fph_store_tile(bx, p.y3 + t0, T.rows, L);
    __syncthreads();
    fl_f32x16 out = {};
    fph_head(ba, bx, bh, p.p + FPH_P_ACTOR, FPH_ACT, out, L);
    fph_put_logits(out, s_lg, p.logits, T, L);
    if (p.value) {
        fph_head(ba, bx, bh, p.p + FPH_P_CRITIC, 1, out, L);
        fph_put_val(out, p.val, T, L);
    }
    fph_act(s_lg, p, T, L);
}

// ---- value[env] = mean of the env's critic values: a wave per env, lane l sums agents l, l + 64, ... in order, then a butterfly
__global__ void __launch_bounds__(64) k_ph_value(FphArgs p) {
    const int env = blockIdx.x, lane = threadIdx.x;
    const float *v = p.val + (size_t)env * p.A;
    float s = 0.f;
    for (int a = lane; a < p.A; a += 64) s += v[a];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) p.value[env] = s / (float)p.A;
}

#define FPH_LDS_EMBED (2 * FPH_ROWS * FPH_STRIDE * sizeof(float))
#define FPH_LDS_BLOCK (2 * FPH_ROWS * FPH_STRIDE * sizeof(float))
#define FPH_LDS_LAST (3 * FPH_ROWS * FPH_STRIDE * sizeof(float))
