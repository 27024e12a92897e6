// mul_mat_id_plan.hpp — the routing plan of a MUL_MAT_ID (ggml_cdna4_mul_mat_id, its `prepared` twin and the front key): which launches a call takes, which weights
// they read and which view of the workspace they use.  mmid_make_plan() is side-effect free — no scratch, no launch, no error text, no fault status; it reads the call,
// the CU count, the env knobs and the (read-only) resident registry — so the calls and the key read the SAME plan: the calls execute it, the key reads a field.
// Kernel-library sources only (like gemm_q_plan.hpp: not one of the files the ggml plug-in's checksum covers).
#pragma once
#include "cdna4_kernels.h"

// a call as the C-ABI hands it over (include/ggml_cdna4.h: ggml_cdna4_mul_mat_id)
struct mmid_call {
    int type; const void *as; int64_t w_row_bytes, w_expert_bytes;
    const float *b; int64_t b_row_stride, b_tok_stride;
    const int32_t *ids; int64_t ids_tok_stride;
    float *dst; int64_t dst_row_stride, dst_tok_stride;
    int64_t M, K, n_expert, n_used, n_b, n_tok;
    void *workspace; size_t workspace_bytes;
};

enum mmid_kind {
    MMID_EMPTY,         // nothing to multiply: the call returns 0
    MMID_REFUSED,       // the call returns `rc` with the message `err`
    MMID_QUEUE,         // the work-queue form: k_moe_sk_front (unless the front is in place) + ONE persistent k_gemm_kq_sk (workspace: moe_sk_carve)
    MMID_TILES_MMQ,     // per tile (workspace: moe_carve): k_moe_plan + the int8 gather + the int8 matrix-core kernel (cdna4_launch_mmq_ids)
    MMID_TILES_T64,     // per tile: k_moe_plan + the fp16 gather + k_gemm_kq_t64<.., IDS> (cdna4_launch_gemm_t64_ids)
    MMID_TILES_KQ,      // per tile: k_moe_plan + the fp16 gather + k_gemm_q<.., IDS> (cdna4_launch_gemm_ids)
    MMID_GEMV_1,        // one token: ONE launch, the activation quantizer inside the GEMV (workspace untouched)
    MMID_GEMV,          // quantize (workspace: carve) + k_gemv_q over the (token, slot) columns
};
// k_gemm_kq_t64<.., IDS>: tile rows, whether the launch reads the planner's tile order / fragment tables, and the split it WANTS (2: the ticketed split, which the
// launcher takes only if it gets the scratch; the tables are off with it either way)
struct t64_ids_plan { int tm; bool tables; int splitk; };
t64_ids_plan t64_ids_make_plan(int M, int K, int img_rows);                                     // gemm_q_t64.hip, next to the measurements behind the rule
// (cdna4_launch_gemm_ids no longer forwards aligned Q4_K to cdna4_launch_gemm_t64_ids — the note above its declaration in cdna4_kernels.h is from before the plan: the plan
// names the terminal, and aligned Q4_K handed to cdna4_launch_gemm_ids would run k_gemm_q<Q4_K, .., WLDS, IDS>)
// k_gemm_q<.., IDS>: the expert matrices go through LDS (whole 16-byte superblocks, 16-byte aligned)
bool cdna4_gemm_ids_wlds(int type, const void *W, int64_t w_row_bytes, int64_t w_expert_bytes); // gemm_q_mfma.hip

struct mmid_plan {
    mmid_kind kind;
    int rc; const char *err;                    // MMID_REFUSED: -1 or -2 (no such form: the caller issues the full call) and the message; else 0 / nullptr
    int w_type; const uint8_t *W;               // what the kernel reads: the format as the kernel sees it (Q4_0R: the stack's resident image), its rows,
    int64_t w_row_bytes, w_expert_bytes;        // ... their stride and the experts'
    size_t ws_need;                             // bytes of the workspace view the kind names
    int64_t rows;                               // rows of the activation image: token order (MMID_QUEUE), expert-sorted with padding (MMID_TILES_*), n_tok * n_b (MMID_GEMV)
    int G; int64_t upt, ntile_cap; int cw[4];   // MMID_QUEUE: spans, units per tile, tile-record capacity, the planner's cost weights
    bool front_in_place;                        // MMID_QUEUE: k_moe_sk_front is not launched (the `prepared` twin)
    t64_ids_plan t64;                           // MMID_TILES_T64
    bool wlds;                                  // MMID_TILES_KQ
    uint32_t front_key;                         // what ggml_cdna4_mul_mat_id_front_key documents: non-zero only on MMID_QUEUE
};
mmid_plan mmid_make_plan(const mmid_call &c, bool front_in_place);                              // capi.hip
