// Shared device helpers of the split-bf16 kernels (conv_s2_bf16x3.hip, conv_wgrad_bf16x3.hip): an fp32 operand as the
// exact sum of three bf16 pieces, multiplied on the bf16 matrix cores.  Included inside each file's anonymous namespace, so it includes nothing itself:
// the file includes mfma_tile.h (f32x16) at file scope first.
#pragma once

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// two floats -> one dword of two round-to-nearest bf16 (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned pk) { return __builtin_bit_cast(float, pk << 16); }
__device__ __forceinline__ float bf16_hi(unsigned pk) { return __builtin_bit_cast(float, pk & 0xFFFF0000u); }

// a pair of floats -> its three bf16 pieces (exact three-way split): 11 VALU operations per pair
__device__ __forceinline__ void split2(float x0, float x1, unsigned& p1, unsigned& p2, unsigned& p3) {
    p1 = pack_bf16(x0, x1);
    const float r0 = x0 - bf16_lo(p1), r1 = x1 - bf16_hi(p1);
    p2 = pack_bf16(r0, r1);
    const float q0 = r0 - bf16_lo(p2), q1 = r1 - bf16_hi(p2);
    p3 = pack_bf16(q0, q1);
}

__device__ __forceinline__ f32x16 mma(const u32x4 a, const u32x4 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
