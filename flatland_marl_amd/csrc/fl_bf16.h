// fl_bf16.h -- what the policy's bf16 kernels (fl_tree_lstm_bf16.h, fl_policy_head_bf16.h) share: the bf16 matrix instruction, the
// packed weight format, the product loop over it, the rounding of a tile's floats and the kernel that packs.  THE description of the
// packed format is the one below; the public headers (include/flatland_policy_bf16.h, include/flatland_policy_head_bf16.h) repeat
// it for their callers.
//
// The instruction (v_mfma_f32_32x32x16_bf16, float32 accumulator): lane l of a K = 16 step holds A[row l & 31][k = 8 (l >> 5) + j]
// and B[k = 8 (l >> 5) + j][column l & 31], j = 0 .. 7; the accumulator's rows are fl_acc_row's (fl_mfma.h).  A lane's operands of a
// step are one 16-byte read of its LDS row and one of the packed weights.
//
// Packed weights: a matrix W [R][K] (R a multiple of 32, K of 16) is stored as R / 32 blocks of 32 rows; a block holds its K / 16
// steps one after another, a step the 64 lanes' operands one after another, 8 bf16 each: element j of lane l of step s of block b is
// W[32 b + (l & 31)][16 s + 8 (l >> 5) + j] (fl_bf16_source).  A wave's load of a step is 1 KB of consecutive bytes, eight whole
// 128-byte lines.  Read in torch's row-major layout instead (each lane 32 bytes of its own weight row a 32-k chunk, a quarter of 32
// lines a load) the tree encoder measured 338 / 4 495 us at cfg2 / cfg3 against 297 / 4 083 us
// (profiles/tree_lstm_bf16_variants.json).  A packed buffer is several matrices, each in this format, one after another.
#pragma once
#include "fl_mfma.h"

typedef __bf16 fl_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ fl_f32x16 fl_mfma_bf16(fl_bf16x8 a, fl_bf16x8 b, fl_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

#define FL_BF16_STEP 512                // bf16 a packed step: 64 lanes x 8
#ifndef FL_BF16_UNROLL
#define FL_BF16_UNROLL 4                // K = 16 steps whose loads are issued together
#endif

// this lane's operands of step 0 of block `block` (32 rows of W = 32 output features) of a packed matrix of K columns
__device__ __forceinline__ const __bf16 *fl_bf16_block(const __bf16 *w, int K, int block, int lane) {
    return w + (size_t)block * (K / 16) * FL_BF16_STEP + lane * 8;
}

// acc[n] += A[row][k] * W_n[col][k] over `steps` K = 16 steps, the NB blocks sharing the A operand; arow = this lane's staged row
// + 8 (lane >> 5), w[n] = fl_bf16_block of block n.  A step's loads stand in front of its products: with each load next to its
// product the compiler waits for every load right behind its issue in k_tree_lstm_bf16's U_iou loop, and that launch measured 2.3
// to 3 % slower (profiles/README.md).  One block has a loop of its own below: passed as arrays of one it compiles to other code
// than a plain loop over one accumulator does.
template <int NB>
__device__ __forceinline__ void fl_bf16_mm(const __bf16 *arow, int steps, const __bf16 *const (&w)[NB], fl_f32x16 (&acc)[NB]) {
#pragma unroll FL_BF16_UNROLL
    for (int s = 0; s < steps; s++) {
        const fl_bf16x8 a = *(const fl_bf16x8 *)(arow + 16 * s);
        fl_bf16x8 b[NB];
#pragma unroll
        for (int n = 0; n < NB; n++) b[n] = *(const fl_bf16x8 *)(w[n] + s * FL_BF16_STEP);
#pragma unroll
        for (int n = 0; n < NB; n++) acc[n] = fl_mfma_bf16(a, b[n], acc[n]);
    }
}

// the same for one block (NB = 1)
__device__ __forceinline__ void fl_bf16_mm(const __bf16 *arow, int steps, const __bf16 *w, fl_f32x16 &acc) {
#pragma unroll FL_BF16_UNROLL
    for (int s = 0; s < steps; s++)
        acc = fl_mfma_bf16(*(const fl_bf16x8 *)(arow + 16 * s), *(const fl_bf16x8 *)(w + s * FL_BF16_STEP), acc);
}

// 8 consecutive floats -> bf16, round to nearest even, as (__bf16)x converts (v_cvt_pk_bf16_f32)
__device__ __forceinline__ fl_bf16x8 fl_bf16_round8(const float4 &a, const float4 &b) {
    fl_bf16x8 o;
    o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
    o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
    return o;
}

// element e of a packed matrix of K columns -> the index of its source element in the row-major W
__device__ __forceinline__ size_t fl_bf16_source(int e, int K) {
    const int j = e & 7, l = (e >> 3) & 63, t = e / FL_BF16_STEP;
    const int step = t % (K / 16), block = t / (K / 16);
    return (size_t)(32 * block + (l & 31)) * K + 16 * step + 8 * (l >> 5) + j;
}

// the N matrices of a packed buffer: matrix m is src[m] [rows][K[m]] and starts at element off[m]; off[N] = the buffer's elements
template <int N>
struct FlBf16Pack {
    const float *src[N];
    int off[N + 1];
    int K[N];
};

// element i of the packed buffer = bf16(its source element).  A template, so that the two units that launch it share no symbol.
template <int N>
__global__ void __launch_bounds__(256) k_bf16_pack(FlBf16Pack<N> a, __bf16 *dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.off[N]) return;
    int m = 0;
#pragma unroll
    for (int k = 1; k < N; k++)
        if (i >= a.off[k]) m = k;
    dst[i] = (__bf16)a.src[m][fl_bf16_source(i - a.off[m], a.K[m])];
}

// a.off[0 .. N] from the matrices' rows, then the launch
template <int N>
static inline void fl_launch_bf16_pack(FlBf16Pack<N> &a, const int (&rows)[N], void *dst, hipStream_t s) {
    a.off[0] = 0;
    for (int m = 0; m < N; m++) a.off[m + 1] = a.off[m] + rows[m] * a.K[m];
    hipLaunchKernelGGL(k_bf16_pack<N>, dim3((a.off[N] + 255) / 256), dim3(256), 0, s, a, (__bf16 *)dst);
}
