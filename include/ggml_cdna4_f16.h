/* ggml_cdna4_f16.h — the route query of ggml_cdna4_op_mul_mat_f (include/ggml_cdna4.h) on F32 / F16 / BF16 weights; implemented in ggml_amd/csrc/gemm_f16.hip.
 * A header of its own, like ggml_cdna4_gguf.h: the ggml plug-in does not use it, so a plug-in built against ggml_cdna4.h stays current.
 *
 * ggml_cdna4_op_mul_mat_f with F16 src0 (src1 rounded to fp16 first, fp32 accumulation) runs on the matrix cores (k_gemm_f16) or, for 1 .. 8 activation rows,
 * on the weight-streaming k_gemv_f16, where K is a multiple of 8 and the data pointers and row / batch strides of src0 and src1 are multiples of 16 bytes;
 * every other call, and F32 weights, take one wave per output element (k_mul_mat_f).  CDNA4_F16_GEMM=0 in the environment keeps every call on that kernel.
 *
 * BF16 src0 (src0->type == 30, nb[0] == 2; F32 src1 and dst) is accepted by the same call under the same rules and takes the same routes on the bf16 forms of
 * those kernels: src1 is rounded to bf16 first (nearest even, no subnormal flush, NaN stays NaN: ggml_compute_fp32_to_bf16), the weights are used as stored,
 * accumulation is fp32.  (C-ABI only: the ggml plug-in does not offer BF16 MUL_MATs to this library.) */
#pragma once
#include "ggml_cdna4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the kernel ggml_cdna4_op_mul_mat_f(src0, src1, dst, ..) would take, read from the plan the call itself executes; needs no device (CDNA4_ASSUME_CUS names
 * the part): 0 the call is refused, 1 k_mul_mat_f, 2 k_gemv_f16, 3 k_gemm_f16 (BF16 src0: their bf16 forms) */
int ggml_cdna4_op_mul_mat_f_route(const ggml_cdna4_tensor * src0, const ggml_cdna4_tensor * src1, const ggml_cdna4_tensor * dst);

#ifdef __cplusplus
}
#endif
