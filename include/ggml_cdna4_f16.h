/* ggml_cdna4_f16.h — the route queries of the calls on F16 / BF16 weights: ggml_cdna4_mul_mat_id on F16 / BF16 expert stacks (further down), and
 * ggml_cdna4_op_mul_mat_f (include/ggml_cdna4.h) on F32 / F16 / BF16 weights; that one is implemented in ggml_amd/csrc/gemm_f16.hip.
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

/* MUL_MAT_ID on F16 / BF16 expert stacks (implemented in ggml_amd/csrc/moe_f16.hip).  ggml_cdna4_mul_mat_id (include/ggml_cdna4.h) accepts type 1 (F16) and
 * 30 (BF16) with its documented arguments; w_row_bytes is the byte stride of a row of K 2-byte weights.  b is rounded to the weights' format first (nearest even;
 * bf16: no subnormal flush, NaN stays NaN), the weights are used as stored, accumulation is fp32 in a fixed k order: two calls agree bit for bit.  Accepted where K is
 * a positive multiple of 8; as, w_row_bytes, w_expert_bytes, b and 4 * b_row_stride are multiples of 16; w_row_bytes <= 2^23; dst_row_stride >= M; and, as for the
 * quantized types, n_used % n_b == 0, b_tok_stride == n_b * b_row_stride, dst_tok_stride == n_used * dst_row_stride.  Everything else is refused with -1 and a message
 * naming the rule — there is no slower fall-back kernel.  A slot whose id lies outside [0, n_expert) stays unwritten.
 * Up to a crossover in n_tok * n_used (CDNA4_F16_MOE_GEMV_MAX in the environment overrides it) the call is one launch that needs no workspace (null is fine); above it
 * the ids are sorted on the device and ONE grouped matrix-core launch follows, which needs n_expert <= 1024 and a 256-byte-aligned workspace of
 * ggml_cdna4_mul_mat_id_workspace_size(type, ..) bytes: the row lists and tile tables only, there is no activation image (0 where K is not a positive multiple of 8 or
 * a count is not positive).  ggml_cdna4_mul_mat_id_prepared and ggml_cdna4_mul_mat_id_front_key answer -2 and 0 for these types.
 * (C-ABI only: the ggml plug-in does not offer F16 / BF16 MUL_MAT_IDs to this library.)
 *
 * The query: the kernel ggml_cdna4_mul_mat_id(type, .., workspace, workspace_bytes, stream) would take, read from the plan the call itself executes; needs no device:
 * 0 the call is refused (any other type included), 1 the per-column kernel (k_gemv_f16_ids; also an empty call, which launches nothing), 2 the grouped kernel
 * (k_moe_plan + k_gemm_f16_ids) */
int ggml_cdna4_mul_mat_id_f16_route(int type, const void * as, int64_t w_row_bytes, int64_t w_expert_bytes, const float * b, int64_t b_row_stride, int64_t b_tok_stride,
                                    const int32_t * ids, int64_t ids_tok_stride, float * dst, int64_t dst_row_stride, int64_t dst_tok_stride,
                                    int64_t M, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok, void * workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
