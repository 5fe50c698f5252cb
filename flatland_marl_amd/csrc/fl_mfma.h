// fl_mfma.h -- what the policy's kernels (fl_tree_lstm.h, fl_tree_lstm_bwd.h, fl_policy_head.h, fl_policy_head_bwd.h) share around
// the f32-input MFMA (v_mfma_f32_32x32x2_f32, exact f32): a wave computes 32 rows x 32 columns, lane l holds the A operand of row
// l & 31 and the B operand of column l & 31, step s of a 32-wide chunk kc takes k = kc + 16 * (l >> 5) + s.
#pragma once

typedef float fl_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ fl_f32x16 fl_mfma(float a, float b, fl_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// row of an accumulator register: lane l holds rows (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), r = 0 .. 15, of column l & 31 (the
// bf16 instruction of fl_bf16.h has the same accumulator)
__device__ __forceinline__ int fl_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// 16 consecutive floats (16-byte aligned) -> a[0 .. 15]: a lane's operands of one chunk.  Every product of those kernels unpacks with it.
__device__ __forceinline__ void fl_ld16(const float *src, float (&a)[16]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 v = ((const float4 *)src)[q];
        a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}
