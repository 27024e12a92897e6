// gemm_f16_plan.hpp — the routing plan of ggml_cdna4_op_mul_mat_f (gemm_f16.hip): which kernel a MUL_MAT on F32 / F16 / BF16 weights takes and the launch geometry.
// f16_make_plan() is side-effect free — no launch, no error text; it reads the three tensor descriptors, the CU count and ONE env knob (CDNA4_F16_GEMM=0:
// the new kernels are off, for A/B timing) — so the call and ggml_cdna4_op_mul_mat_f_route read the SAME plan: the call executes it, the query reads `route`.
// Host-only; kernel-library sources only (like gemm_q_plan.hpp: not one of the files the ggml plug-in's checksum covers).
#pragma once
#include "../../include/ggml_cdna4.h"
#include "cdna4_common.h"
#include <stdlib.h>

enum f16_route {
    F16_REFUSED = 0,    // the call returns -1 with the message `err`
    F16_PLAIN = 1,      // k_mul_mat_f (ops.hip): one wave per output element; F32 weights, and whatever the kernels below cannot read
    F16_GEMV = 2,       // k_gemv_f16<nb> / k_gemv_bf16<nb>: 1 .. 8 activation rows, bound by the weight stream
    F16_GEMM = 3,       // k_gemm_f16<tn, bf>: the matrix cores
};                      // (the two 2-byte weight types route alike; for BF16 src0 a number names the bf16 instantiation)
struct f16_plan {
    int route; const char *err;
    bool empty;         // nothing to multiply: the call returns 0 without a launch
    int tn;             // F16_GEMM: activation rows per tile (32 / 128)
    bool y16;           // F16_GEMM: dst rows take 16-byte stores (its data pointer and strides are multiples of 16); otherwise 4-byte stores
    int nb;             // F16_GEMV: activation rows per work-group (1 / 2 / 4 / 8: N rounded up, the padding rows repeat the last one)
    unsigned gx, gy, gz;    // the grid (work-groups of 256 threads)
};

// k_mul_mat_f (ops.hip): one wave per output element of a MUL_MAT on F32 / F16 weights, any strides; the caller has validated the call
int cdna4_launch_mul_mat_f(const ggml_cdna4_tensor *a, const ggml_cdna4_tensor *b, const ggml_cdna4_tensor *d, hipStream_t st);

#define F16_GEMM_TM 128        // weight rows per tile of k_gemm_f16
#define F16_GEMV_ROWS 8         // weight rows per work-group of k_gemv_f16 (two per wave)
#define F16_GEMV_MAX_N 8        // the few-row / GEMM crossover (measured at [4096 x 4096])

inline f16_plan f16_make_plan(const ggml_cdna4_tensor *a, const ggml_cdna4_tensor *b, const ggml_cdna4_tensor *d, int cus) {
    f16_plan pl{};
    auto refuse = [&](const char *msg) { pl.route = F16_REFUSED; pl.err = msg; return pl; };
    if (!((a->type == CDNA4_F32 || a->type == CDNA4_F16 || a->type == CDNA4_BF16) && b->type == CDNA4_F32 && d->type == CDNA4_F32)) return refuse("mul_mat_f: F32/F16/BF16 x F32 only");
    if (!(a->ne[0] == b->ne[0] && d->ne[0] == a->ne[1] && d->ne[1] == b->ne[1] && d->ne[2] == b->ne[2] && d->ne[3] == b->ne[3])) return refuse("mul_mat_f: shape mismatch");
    if (!(a->ne[2] > 0 && a->ne[3] > 0 && b->ne[2] % a->ne[2] == 0 && b->ne[3] % a->ne[3] == 0)) return refuse("mul_mat_f: batch dims not broadcastable");
    if (!(a->nb[0] == (a->type == CDNA4_F32 ? 4 : 2) && b->nb[0] == 4)) return refuse("mul_mat_f: k must be the contiguous dimension");
    pl.route = F16_PLAIN;
    const int64_t M = d->ne[0], N = d->ne[1], K = a->ne[0], nbatch = d->ne[2] * d->ne[3];
    pl.empty = M * N * nbatch == 0;
    if (pl.empty || a->type == CDNA4_F32) return pl;
    const char *knob = getenv("CDNA4_F16_GEMM");
    if (knob && atoi(knob) == 0) return pl;
    // what the new kernels read: 16-byte chunks of eight weights (LDS-DMA / wave loads) and float4 activations; they write dst rows contiguous in m
    auto al16 = [](const ggml_cdna4_tensor *t) { return (((uintptr_t)t->data | (uintptr_t)t->nb[1] | (uintptr_t)t->nb[2] | (uintptr_t)t->nb[3]) & 15) == 0 && t->nb[1] > 0 && t->nb[2] >= 0 && t->nb[3] >= 0; };
    if (K <= 0 || K % 8 != 0 || !al16(a) || !al16(b) || d->nb[0] != 4 || d->nb[1] <= 0) return pl;
    // 32-bit offsets inside a tile (the LDS-DMA's lane offset), grid limits
    if (nbatch > 65535 || M > (int64_t)1 << 30 || N > (int64_t)1 << 30 || K > (int64_t)1 << 24 || a->nb[1] > (int64_t)1 << 23 || b->nb[1] > (int64_t)1 << 30 || d->nb[1] > (int64_t)1 << 40) return pl;
    if (N <= F16_GEMV_MAX_N) {
        pl.route = F16_GEMV;
        pl.nb = N <= 1 ? 1 : (N <= 2 ? 2 : (N <= 4 ? 4 : 8));
        pl.gx = (unsigned)((M + F16_GEMV_ROWS - 1) / F16_GEMV_ROWS); pl.gy = 1; pl.gz = (unsigned)nbatch;
        return pl;
    }
    const int64_t mt = (M + F16_GEMM_TM - 1) / F16_GEMM_TM;
    // 128-wide tiles reuse a weight tile four times as often, but only pay where they leave every CU a work-group (gpt-2's per-head products are twelve small GEMMs)
    pl.tn = (N <= 32 || mt * ((N + 127) / 128) * nbatch < (int64_t)(cus > 0 ? cus : 1)) ? 32 : 128;
    const int64_t nt = (N + pl.tn - 1) / pl.tn;
    if (nt > 65535) return pl;
    pl.route = F16_GEMM;
    pl.y16 = al16(d);
    pl.gx = (unsigned)mt; pl.gy = (unsigned)nt; pl.gz = (unsigned)nbatch;
    return pl;
}
