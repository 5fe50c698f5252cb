// fl_policy_head_bf16.h -- the policy head of fl_policy_head.h with 16 of its 19 matrices on the bf16 matrix instruction
// (v_mfma_f32_32x32x16_bf16, gfx950), for inference.  Included by fl_policy_head.hip behind fl_policy_head.h, whose first layer
// (fph_load_attr, fph_mm_attr), float32 product (fph_mm), GELU (fph_gelu), a head's last layer (fph_head_out), the tail of the last
// block (fph_put_logits, fph_put_val, fph_act with the action choice fph_choose) and value kernel (k_ph_value) it calls, on that header's FphLane / FphRows /
// FphAttnTile coordinates.  The entry points are those of include/flatland_policy_head_bf16.h.
//
// Launches: k_ph16_embed, (k_ph16_attn, k_ph16_block) x 3, k_ph_value -- the structure of fl_policy_head.h, a workgroup of 4 waves
// on a tile of 32 rows, a wave per head in the attention.
//
// Where a value is bf16 (round to nearest even, as (__bf16)x converts) and where float32:
//   bf16 products, float32 sums from zero, float32 bias last, float32 GELU: attr_embedding.2 / .4 / .6, the three in_proj, out_proj
//     and att_mlp.0, actor_net.0 / .2, critic_net.0 / .2.  Their weights come packed and rounded from fl_policy_head_pack_bf16; an
//     activation is rounded once, when it is written to the LDS tile the product reads.
//   exact float32 MFMA as in fl_policy_head.h: attr_embedding.0 (K = 83, raw attributes) and actor_net.4 / critic_net.4, which read
//     the float32 GELU output of the layer before them.
//   q, k, v: rounded when in_proj writes them to the workspace after the float32 bias, bf16 [R][768] row-major, q | k | v.
//   emb, xa, xb, ao, val: float32 in the workspace; a tile rounds them when it stages them.
//   attention: S = q k^T on the bf16 instruction, the maxima and e = expf((s - max) / 8) float32, e rounded to bf16 for P V, the row
//     sum the float32 sum of the ROUNDED e (the values that multiply v), the quotient last: an output is a convex combination of
//     bf16 v rows up to float32 summation.
//
// LDS tiles are bytes: a bf16 row of 256 is 512 bytes = 32 slots of 16 bytes; a ds_read_b128 is conflict free when the row stride
// in 16-byte slots is odd (fl_tree_lstm_bf16.h), so rows are padded to 33 slots (528 bytes), the [x | a] rows of 512 to 65 (1040).
// What a lane holds of a K = 16 step, and the format of each of the 16 packed matrices: fl_bf16.h.
//
// The attention computes the scores TRANSPOSED, X = k q^T (A operand: 32 keys, B operand: the tile's 32 queries), so a lane holds
// one query's scores of 16 keys in its accumulator registers: the row maximum and the row sum are sums inside a lane and one
// exchange between the lane halves, and the rounded e are the A operand of P V as they are, with no trip through LDS -- registers
// 8 s .. 8 s + 7 are step s, whose element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3) of the chunk.
// The v operand: B of P V runs along the keys, B[key][d], and v is row-major along d.  Of the three ways (a transposed copy of the
// chunk in LDS, the transposing LDS read, a transposed second workspace region) this kernel stages the chunk transposed in LDS,
// vt[d][key]: the staging chooses each key's position, so the key order above -- which the transposing read does not produce --
// costs nothing, a lane's operand of a step is one 16-byte read (rows of 32 keys = 64 bytes, padded to 5 slots), and the
// workspace stays the documented one.  A wave stages its own head's chunk: 4 loads of 16 bytes (4 keys x 8 d) and 8 stores of 8
// bytes (4 keys of one d) a lane.
#pragma once
#include "fl_bf16.h"
#include "fl_policy_head.h"

#define FPH16_STRIDE 528                // bytes a staged bf16 row of 256: 33 slots
#define FPH16_STRIDE2 1040              // ... of 512 ([x | a], [emb | y]): 65 slots
#define FPH16_ASTRIDE 100               // floats a row of the float32 attribute tile (96 used): 4 mod 32
#define FPH16_HSTRIDE 132               // floats a row of a head's float32 hidden tile (128 used): 4 mod 32, 528 bytes
#define FPH16_VSTRIDE 80                // bytes a row of the transposed v chunk (32 keys): 5 slots
#define FPH16_NMAT 16
#define FPH16_ROW_BYTES (4 * FPH_E * 4 + 3 * FPH_E * 2 + 4)       // workspace bytes a row: 5636

// the 16 packed matrices in state_dict order: element offsets in the packed buffer
enum {
    FPH16_ATTR2 = 0, FPH16_ATTR4 = 65536, FPH16_ATTR6 = 131072,
    FPH16_BLOCK = 163840,               // + 393 216 blk: in_proj, out_proj (+ 196 608), att_mlp.0 (+ 262 144)
    FPH16_BLOCK_SIZE = 393216, FPH16_OUT_PROJ = 196608, FPH16_ATT_MLP = 262144,
    FPH16_ACTOR0 = 1343488, FPH16_ACTOR2 = 1474560, FPH16_CRITIC0 = 1507328, FPH16_CRITIC2 = 1638400,
    FPH16_PACKED = 1671168,             // bf16 elements: 3 342 336 bytes
};
// (literals, as the kernels use them: each is the running sum of out * in over the packed matrices of fl_policy_layout.h's table)
static_assert(FPH16_ATTR2 == fpl_bf16_before(0) && FPH16_ATTR4 == fpl_bf16_before(1) && FPH16_ATTR6 == fpl_bf16_before(2) &&
              FPH16_BLOCK == fpl_bf16_before(3) && FPH16_OUT_PROJ == fpl_bf16_before(4) - FPH16_BLOCK &&
              FPH16_ATT_MLP == fpl_bf16_before(5) - FPH16_BLOCK && FPH16_BLOCK_SIZE == fpl_bf16_before(6) - FPH16_BLOCK &&
              FPH16_ACTOR0 == fpl_bf16_before(12) && FPH16_ACTOR2 == fpl_bf16_before(13) && FPH16_CRITIC0 == fpl_bf16_before(14) &&
              FPH16_CRITIC2 == fpl_bf16_before(15), "the packed buffer's offsets (FPH16_PACKED: fl_policy_head.hip)");

struct Fph16Args : FphArgs {
    const __bf16 *packed;               // fl_policy_head_pack_bf16's buffer
    __bf16 *qkv16;                      // workspace: bf16 [R][768]; FphArgs::qkv is unused
};

// this lane's A row of a tile: row `col`, column c0, its k half of a step
__device__ __forceinline__ const __bf16 *fph16_arow(const unsigned char *tile, int stride, int c0, const FphLane L) {
    return (const __bf16 *)(tile + L.col * stride) + c0 + 8 * L.hh;
}

// a layer of 256 outputs: the wave's two blocks 2 wave, 2 wave + 1 of a packed matrix of K columns over a tile's columns c0 .. c0 + K
__device__ __forceinline__ void fph16_layer256(const unsigned char *tile, int stride, int c0, int K, const __bf16 *w, fl_f32x16 (&acc)[2],
                                               const FphLane L) {
    const __bf16 *const ws[2] = {fl_bf16_block(w, K, 2 * L.wave, L.lane), fl_bf16_block(w, K, 2 * L.wave + 1, L.lane)};
    fl_bf16_mm<2>(fph16_arow(tile, stride, c0, L), K / 16, ws, acc);
}

// (acc + bias) [GELU] of the 32 x 32 block of features j0 .. j0 + 31 of a layer: rounded to bf16 -> tile columns c0 + j0 ..; the
// float32 value -> g[row][j0 ..] of the rows below `rows` where g is given (g = the layer's first feature of row 0, ld floats a row)
template <bool GELU>
__device__ __forceinline__ void fph16_to_lds(const fl_f32x16 &acc, const float *bias, int j0, unsigned char *tile, int stride, int c0,
                                             const FphLane L, float *g = nullptr, int ld = 0, int rows = 0) {
    const float b = bias[j0 + L.col];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = fl_acc_row(r, L.hh);
        float v = acc[r] + b;
        if (GELU) v = fph_gelu(v);
        *((__bf16 *)(tile + row * stride) + c0 + j0 + L.col) = (__bf16)v;
        if (g && row < rows) g[(size_t)row * ld + j0 + L.col] = v;
    }
}

// a 256-wide layer: the wave's two blocks, features 64 wave .. 64 wave + 63
template <bool GELU>
__device__ __forceinline__ void fph16_to_lds(const fl_f32x16 (&acc)[2], const float *bias, unsigned char *tile, int stride, int c0,
                                             const FphLane L, float *g = nullptr, int ld = 0, int rows = 0) {
    fph16_to_lds<GELU>(acc[0], bias, 64 * L.wave, tile, stride, c0, L, g, ld, rows);
    fph16_to_lds<GELU>(acc[1], bias, 64 * L.wave + 32, tile, stride, c0, L, g, ld, rows);
}

// rows [0, rows) x n8 groups of 8 floats of global rows of ld floats -> bf16 columns c0 .. of a tile (rows past `rows`: zero); the
// float32 values are copied to copy[row][8 q ..] (ldc floats a row) where copy is given
__device__ __forceinline__ void fph16_load_tile(unsigned char *tile, int stride, int c0, const float *src, int ld, int n8, int rows, const FphLane L,
                                                float *copy = nullptr, int ldc = 0) {
    for (int i = L.tid; i < FPH_ROWS * n8; i += FPH_THREADS) {
        const int r = i / n8, q = i % n8;
        fl_bf16x8 o = {};
        if (r < rows) {
            const float4 a = ((const float4 *)(src + (size_t)r * ld))[2 * q], b = ((const float4 *)(src + (size_t)r * ld))[2 * q + 1];
            o = fl_bf16_round8(a, b);
            if (copy) {
                ((float4 *)(copy + (size_t)r * ldc))[2 * q] = a;
                ((float4 *)(copy + (size_t)r * ldc))[2 * q + 1] = b;
            }
        }
        *(fl_bf16x8 *)(tile + r * stride + 2 * (c0 + 8 * q)) = o;
    }
}

// q, k, v of the next block from a tile's columns c0 .. c0 + 255: bf16((X in_proj^T) + bias) -> out[rows][768] (6 blocks a wave, in pairs)
__device__ __forceinline__ void fph16_qkv(const unsigned char *tile, int stride, int c0, const __bf16 *w, const float *bias, __bf16 *out,
                                          int rows, const FphLane L) {
    const int col = L.col;
    const __bf16 *arow = fph16_arow(tile, stride, c0, L);
#pragma unroll 1
    for (int pr = 0; pr < 3; pr++) {
        const int b0 = 6 * L.wave + 2 * pr, j0 = 32 * b0, j1 = j0 + 32;
        const __bf16 *const ws[2] = {fl_bf16_block(w, FPH_E, b0, L.lane), fl_bf16_block(w, FPH_E, b0 + 1, L.lane)};
        fl_f32x16 acc[2] = {};
        fl_bf16_mm<2>(arow, FPH_E / 16, ws, acc);
        const float bb0 = bias[j0 + col], bb1 = bias[j1 + col];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = fl_acc_row(r, L.hh);
            if (row < rows) {
                out[(size_t)row * (3 * FPH_E) + j0 + col] = (__bf16)(acc[0][r] + bb0);
                out[(size_t)row * (3 * FPH_E) + j1 + col] = (__bf16)(acc[1][r] + bb1);
            }
        }
    }
}

// ---- attr MLP, embedding, q k v of the first block
__global__ void __launch_bounds__(FPH_THREADS) k_ph16_embed(Fph16Args p) {
    __shared__ __attribute__((aligned(16))) float s_attr[FPH_ROWS * FPH16_ASTRIDE];
    __shared__ __attribute__((aligned(16))) unsigned char s_t[2][FPH_ROWS * FPH16_STRIDE];
    const FphLane L{};
    const FphRows T{p.R};

    fph_load_attr(s_attr, FPH16_ASTRIDE, p.attr, T, L);
    __syncthreads();
    const float *const *w = p.p + FPH_P_ATTR;
    {                                                            // 83 -> 256, exact float32: -> tile 0
        fl_f32x16 acc[2] = {};
        fph_mm_attr(s_attr + L.col * FPH16_ASTRIDE, w[0] + (size_t)(64 * L.wave + L.col) * FPH_ATTR, w[0] + (size_t)(64 * L.wave + 32 + L.col) * FPH_ATTR, acc, L);
        fph16_to_lds<true>(acc, w[1], s_t[0], FPH16_STRIDE, 0, L);
    }
    __syncthreads();
    for (int l = 1; l <= 2; l++) {                               // 256 -> 256 twice: tile 0 -> 1 -> 0
        fl_f32x16 acc[2] = {};
        fph16_layer256(s_t[l - 1], FPH16_STRIDE, 0, FPH_E, p.packed + (l == 1 ? FPH16_ATTR2 : FPH16_ATTR4), acc, L);
        fph16_to_lds<true>(acc, w[2 * l + 1], s_t[l & 1], FPH16_STRIDE, 0, L);
        __syncthreads();
    }
    float *emb = p.emb + (size_t)T.row0 * FPH_E;
    {                                                            // 256 -> 128: tile 0 -> tile 1[:, :128] and emb; the tree embedding beside it
        fl_f32x16 acc = {};
        fl_bf16_mm(fph16_arow(s_t[0], FPH16_STRIDE, 0, L), FPH_E / 16, fl_bf16_block(p.packed + FPH16_ATTR6, FPH_E, L.wave, L.lane), acc);
        fph16_to_lds<true>(acc, w[7], 32 * L.wave, s_t[1], FPH16_STRIDE, 0, L, emb, FPH_E, T.rows);
        fph16_load_tile(s_t[1], FPH16_STRIDE, FPH_H, p.tree + (size_t)T.row0 * FPH_H, FPH_H, FPH_H / 8, T.rows, L, emb + FPH_H, FPH_E);
    }
    __syncthreads();
    fph16_qkv(s_t[1], FPH16_STRIDE, 0, p.packed + FPH16_BLOCK, p.p[FPH_P_BLOCK + 1], p.qkv16 + (size_t)T.row0 * (3 * FPH_E), T.rows, L);
}

// ---- attention of one block: workgroup = (env, tile of 32 queries), wave = head; see the head of this file.  Two passes over the
// keys in chunks of 32: the maxima, then e, its sums and e v.  Keys past the env's last agent take no part: their e and their v are 0.
__global__ void __launch_bounds__(FPH_THREADS) k_ph16_attn(Fph16Args p) {
    __shared__ __attribute__((aligned(16))) unsigned char s_vt[FPH_HEADS][FPH_D * FPH16_VSTRIDE];
    const FphLane L{};
    const int A = p.A, lane = L.lane, head = L.wave, col = L.col, hh = L.hh;
    const FphAttnTile T{A};
    const int q0 = T.first;
    const __bf16 *qkv = p.qkv16 + T.base * (3 * FPH_E);
    unsigned char *vt = s_vt[head];

    fl_bf16x8 qb[4];                                             // the B operand: q of query q0 + col (the last one repeated past the env)
    {
        const __bf16 *qrow = qkv + (size_t)min(q0 + col, A - 1) * (3 * FPH_E) + head * FPH_D + 8 * hh;
#pragma unroll
        for (int s = 0; s < 4; s++) qb[s] = *(const fl_bf16x8 *)(qrow + 16 * s);
    }
    // staging of v: this lane takes d = 8 slot .. 8 slot + 7 of keys 4 kq .. 4 kq + 3 of the chunk, which go to the positions
    // 4 quad .. 4 quad + 3 of a vt row: key 16 s + 4 t + b sits at 16 s + 8 (t & 1) + 4 (t >> 1) + b, the order of the A operand
    const int slot = lane & 7, kq = lane >> 3, quad = 4 * (kq >> 2) + 2 * (kq & 1) + ((kq & 3) >> 1);
    float mx = -INFINITY, sum = 0.f;
    fl_f32x16 o0 = {}, o1 = {};

#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
        for (int k0 = 0; k0 < A; k0 += 32) {
            const __bf16 *krow = qkv + (size_t)min(k0 + col, A - 1) * (3 * FPH_E) + FPH_E + head * FPH_D + 8 * hh;
            fl_f32x16 s = {};                                    // s[r] = q(query col) . k(key k0 + fl_acc_row(r, hh))
#pragma unroll
            for (int t = 0; t < 4; t++) s = fl_mfma_bf16(*(const fl_bf16x8 *)(krow + 16 * t), qb[t], s);
            if (pass == 0) {
#pragma unroll
                for (int r = 0; r < 16; r++)
                    if (k0 + fl_acc_row(r, hh) < A) mx = fmaxf(mx, s[r]);
                continue;
            }
            __syncthreads();                                     // the previous chunk's vt has been read
            {
                fl_bf16x8 v[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int key = k0 + 4 * kq + i;
                    const fl_bf16x8 zero = {};
                    v[i] = zero;
                    if (key < A) v[i] = *(const fl_bf16x8 *)(qkv + (size_t)key * (3 * FPH_E) + 2 * FPH_E + head * FPH_D + 8 * slot);
                }
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
                    const bf16x4 w = {v[0][e], v[1][e], v[2][e], v[3][e]};
                    *(bf16x4 *)(vt + (8 * slot + e) * FPH16_VSTRIDE + 8 * quad) = w;
                }
            }
            fl_bf16x8 pa[2];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool live = k0 + fl_acc_row(r, hh) < A;
                const __bf16 e = (__bf16)(live ? expf((s[r] - mx) * 0.125f) : 0.f);
                sum += (float)e;
                pa[r >> 3][r & 7] = e;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const fl_bf16x8 b0 = *(const fl_bf16x8 *)(vt + col * FPH16_VSTRIDE + 32 * t + 16 * hh);
                const fl_bf16x8 b1 = *(const fl_bf16x8 *)(vt + (32 + col) * FPH16_VSTRIDE + 32 * t + 16 * hh);
                o0 = fl_mfma_bf16(pa[t], b0, o0);
                o1 = fl_mfma_bf16(pa[t], b1, o1);
            }
        }
        // a query's maximum / sum: its two lanes (col, col + 32) hold the halves
        if (pass == 0) mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        else sum = sum + __shfl_xor(sum, 32, 64);
    }
    float *out = p.ao + T.base * FPH_E + head * FPH_D;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = fl_acc_row(r, hh), qi = q0 + row;
        const float sq = __shfl(sum, row, 64);                   // o[r] is query `row`'s, whose sum lane `row` holds
        if (qi < A) {
            out[(size_t)qi * FPH_E + col] = o0[r] / sq;
            out[(size_t)qi * FPH_E + 32 + col] = o1[r] / sq;
        }
    }
}

// a 512 -> 256 -> 128 -> n_out head on the tile [emb | y]: the first two layers bf16, the last float32 on the float32 GELU output;
// the result of rows x n_out in wave 0's registers, bias added.  h: 32 rows of 528 bytes, bf16 [256] then float32 [128].  Every
// wave calls it (barriers inside).
__device__ __forceinline__ void fph16_head(const unsigned char *tile, unsigned char *h, const __bf16 *w0, const __bf16 *w2, const float *const *p,
                                           int n_out, fl_f32x16 &out, const FphLane L) {
    const int wave = L.wave, col = L.col;
    {
        fl_f32x16 acc[2] = {};
        fph16_layer256(tile, FPH16_STRIDE2, 0, 2 * FPH_E, w0, acc, L);
        __syncthreads();                                         // (h may still be read by the head before this one)
        fph16_to_lds<true>(acc, p[1], h, FPH16_STRIDE, 0, L);
    }
    __syncthreads();
    float *hf = (float *)h;
    {
        fl_f32x16 acc = {};
        fl_bf16_mm(fph16_arow(h, FPH16_STRIDE, 0, L), FPH_E / 16, fl_bf16_block(w2, FPH_E, wave, L.lane), acc);
        __syncthreads();
        const float b = p[3][32 * wave + col];
#pragma unroll
        for (int r = 0; r < 16; r++) hf[fl_acc_row(r, L.hh) * FPH16_HSTRIDE + 32 * wave + col] = fph_gelu(acc[r] + b);
    }
    __syncthreads();
    fph_head_out(hf, FPH16_HSTRIDE, p[4], p[5], n_out, out, L);
}

// ---- the rest of a block per row tile; LAST: the heads and the action instead of the next block's q k v.  The tile is [x | a]:
// the block's input and its attention output, then [x | out_proj], then [x | y] (not LAST) or [emb | y] (LAST).
template <bool LAST>
__global__ void __launch_bounds__(FPH_THREADS) k_ph16_block(Fph16Args p, int blk, const float *xin, float *xout) {
    __shared__ __attribute__((aligned(16))) unsigned char s_t[FPH_ROWS * FPH16_STRIDE2];
    __shared__ __attribute__((aligned(16))) unsigned char s_h[LAST ? FPH_ROWS * FPH16_STRIDE : 16];
    __shared__ float s_lg[FPH_ROWS][FPH_ACT + 1];
    const FphLane L{};
    const FphRows T{p.R};
    const float *const *w = p.p + FPH_P_BLOCK + 6 * blk;
    const __bf16 *pk = p.packed + FPH16_BLOCK + (size_t)blk * FPH16_BLOCK_SIZE;
    const size_t t0 = (size_t)T.row0 * FPH_E;

    fph16_load_tile(s_t, FPH16_STRIDE2, 0, xin + t0, FPH_E, FPH_E / 8, T.rows, L);
    fph16_load_tile(s_t, FPH16_STRIDE2, FPH_E, p.ao + t0, FPH_E, FPH_E / 8, T.rows, L);
    __syncthreads();
    {                                                            // out_proj, over the attention output
        fl_f32x16 acc[2] = {};
        fph16_layer256(s_t, FPH16_STRIDE2, FPH_E, FPH_E, pk + FPH16_OUT_PROJ, acc, L);
        __syncthreads();
        fph16_to_lds<false>(acc, w[3], s_t, FPH16_STRIDE2, FPH_E, L);
    }
    __syncthreads();
    {                                                            // att_mlp on [input | attention], over the attention's half
        fl_f32x16 acc[2] = {};
        fph16_layer256(s_t, FPH16_STRIDE2, 0, 2 * FPH_E, pk + FPH16_ATT_MLP, acc, L);
        __syncthreads();
        fph16_to_lds<true>(acc, w[5], s_t, FPH16_STRIDE2, FPH_E, L, LAST ? nullptr : xout + t0, FPH_E, T.rows);
        if (LAST) fph16_load_tile(s_t, FPH16_STRIDE2, 0, p.emb + t0, FPH_E, FPH_E / 8, T.rows, L);
    }
    __syncthreads();
    if (!LAST) {
        fph16_qkv(s_t, FPH16_STRIDE2, FPH_E, pk + FPH16_BLOCK_SIZE, w[7], p.qkv16 + (size_t)T.row0 * (3 * FPH_E), T.rows, L);
        return;
    }
    fl_f32x16 out = {};
    fph16_head(s_t, s_h, p.packed + FPH16_ACTOR0, p.packed + FPH16_ACTOR2, p.p + FPH_P_ACTOR, FPH_ACT, out, L);
    fph_put_logits(out, s_lg, p.logits, T, L);
    if (p.value) {
        fph16_head(s_t, s_h, p.packed + FPH16_CRITIC0, p.packed + FPH16_CRITIC2, p.p + FPH_P_CRITIC, 1, out, L);
        fph_put_val(out, p.val, T, L);
    }
    fph_act(s_lg, p, T, L);
}
