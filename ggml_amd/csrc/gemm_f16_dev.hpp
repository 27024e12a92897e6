// gemm_f16_dev.hpp — the 2-byte element of the matrix-core kernels on F16 / BF16 weights (gemm_f16.hip: k_gemm_f16<TN, BF>; moe_f16.hip: k_gemm_f16_ids<TN, BF>): its
// vectors, the rounding of four fp32 activations to it, and the matrix-core step on it.  Device code; kernel-library sources only.
#pragma once
#include "cdna4_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// the 2-byte element of a k_gemm_f16 instantiation: its vectors, and the matrix-core step on them
template <bool BF> struct f16_elem { typedef half_t e; typedef half4_t v4; typedef half8_t v8; };
template <> struct f16_elem<true> { typedef __bf16 e; typedef bf16x4_t v4; typedef bf16x8_t v8; };
// four activations of a stage, rounded to nearest even (GGML_FP32_TO_FP16 / ggml_compute_fp32_to_bf16: no subnormal flush); past K (`in` false) zeros
__device__ __forceinline__ void f16_round4(half4_t &h, const f32x4 &x, bool in) {
#pragma unroll
    for (int e = 0; e < 4; e++) h[e] = in ? (half_t)x[e] : (half_t)0.f;
}
__device__ __forceinline__ void f16_round4(bf16x4_t &h, const f32x4 &x, bool in) {      // as one vector: v_cvt_pk_bf16_f32 takes two values per instruction
    h = __builtin_convertvector(in ? x : f32x4{0.f, 0.f, 0.f, 0.f}, bf16x4_t);
}
__device__ __forceinline__ floatx16 f16_mfma(half8_t a, half8_t b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ floatx16 f16_mfma(bf16x8_t a, bf16x8_t b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
