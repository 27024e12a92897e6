// moe_f16_plan.hpp — the routing plan of ggml_cdna4_mul_mat_id on F16 / BF16 expert stacks (moe_f16.hip): which kernel the call takes, its tile width, its grid and
// the view of the workspace.  moe_f16_make_plan() is side-effect free — no launch, no scratch, no error text; it reads the call and two env knobs — so the call and
// ggml_cdna4_mul_mat_id_f16_route read the SAME plan: the call executes it, the query reads `route`.  (It does not depend on the CU count.)
// Host-only; kernel-library sources only (like gemm_f16_plan.hpp: not one of the files the ggml plug-in's checksum covers).
#pragma once
#include "gemm_f16_plan.hpp"
#include "mul_mat_id_plan.hpp"
#include <stdlib.h>

enum moe_f16_route {
    MOE_F16_REFUSED = 0,    // the call returns -1 with the message `err`
    MOE_F16_GEMV = 1,       // k_gemv_f16_ids<bf>: one (token, slot) column per work-group row, the expert id read on the device; no workspace
    MOE_F16_GEMM = 2,       // k_moe_plan + ONE k_gemm_f16_ids<tn, bf>: the matrix cores over the planner's tile table
};
// the workspace of route 2 — what k_moe_plan (quantize_act.hip) leaves: [img_src i32 R][img_dst i32 R][tile_expert | tile_order | tile_nfrag: 3 x i32 R / 128],
// R = image rows, an upper bound of sum_e ceil(cnt_e / 128) * 128.  No activation image: the GEMM gathers its rows from b.
struct moe_f16_view { size_t off_src, off_dst, off_tiles, total; int64_t img_rows; };
inline moe_f16_view moe_f16_carve(int64_t n_expert, int64_t n_used, int64_t n_tok) {
    const auto align256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    moe_f16_view v{};
    v.img_rows = (n_tok * n_used + 127) / 128 * 128 + 128 * n_expert;
    v.off_src = 0;
    v.off_dst = v.off_src + align256((size_t)v.img_rows * 4);
    v.off_tiles = v.off_dst + align256((size_t)v.img_rows * 4);
    v.total = v.off_tiles + align256((size_t)(v.img_rows / 128) * 4 * 3);
    return v;
}
// what ggml_cdna4_mul_mat_id_workspace_size answers for the two types
inline size_t moe_f16_workspace_size(int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok) {
    if (K <= 0 || K % 8 != 0 || n_expert <= 0 || n_used <= 0 || n_b <= 0 || n_tok <= 0) return 0;
    return moe_f16_carve(n_expert, n_used, n_tok).total;
}

// moe_f16.hip: ggml_cdna4_mul_mat_id on an F16 / BF16 expert stack, behind the call's fault-status check — plans, sets the error text of a refusal, launches
int cdna4_mul_mat_id_f16(const mmid_call &c, hipStream_t st);

struct moe_f16_plan {
    int route; const char *err;
    bool empty;             // nothing to multiply: the call returns 0 without a launch
    int tn;                 // MOE_F16_GEMM: image rows per work-group (32: one fragment of a tile record, 128: a whole record)
    bool y16;               // MOE_F16_GEMM: dst rows take 16-byte stores
    moe_f16_view ws;        // MOE_F16_GEMM
    unsigned gx, gy;        // the grid (work-groups of 256 threads)
};

// The per-column / grouped crossover in (token, slot) columns: n_tok * n_used <= this -> route 1.  CDNA4_F16_MOE_GEMV_MAX overrides it (A/B timing).
// Default 16, from profiles/r07/moe_f16.txt (8 experts x 2 used x 4096^2, uniform routing, us per call, route 1 | route 2): 8 columns 42 | 85 (F16), 42 | 81 (BF16);
// 16 columns 80 | 85, 80 | 81 — close to a tie —; 32 columns 159 | 86, 159 | 81.  Between 17 and 31 columns nothing was timed.
#define MOE_F16_GEMV_MAX 16
inline int64_t moe_f16_gemv_max() { const char *e = getenv("CDNA4_F16_MOE_GEMV_MAX"); return e ? atoll(e) : MOE_F16_GEMV_MAX; }

inline moe_f16_plan moe_f16_make_plan(const mmid_call &c) {
    moe_f16_plan pl{};
    auto refuse = [&](const char *msg) { pl.route = MOE_F16_REFUSED; pl.err = msg; return pl; };
    if (c.type != CDNA4_F16 && c.type != CDNA4_BF16) return refuse("mul_mat_id: unsupported weight type");
    pl.route = MOE_F16_GEMV;
    if (c.M <= 0 || c.n_tok <= 0 || c.n_used <= 0) { pl.empty = true; return pl; }
    if (c.K <= 0 || c.K % 8 != 0) return refuse("mul_mat_id: K must be a positive multiple of 8 for F16 / BF16 experts");
    if (c.n_expert <= 0) return refuse("mul_mat_id: n_expert must be positive");
    // the quantized call's own rules, with its messages (capi.hip: mmid_make_plan)
    if (c.n_b <= 0 || c.n_used % c.n_b) return refuse("mul_mat_id: n_used must be a multiple of b.ne[1]");
    if (c.dst_tok_stride != c.n_used * c.dst_row_stride) return refuse("mul_mat_id: dst must be contiguous over (slot, token)");
    if (c.b_tok_stride != c.n_b * c.b_row_stride) return refuse("mul_mat_id: b must be contiguous over (row, token)");
    // what the kernels read: 16-byte chunks of eight weights (LDS-DMA / wave loads) and float4 activations
    if (((uintptr_t)c.as | (uintptr_t)c.w_row_bytes | (uintptr_t)c.w_expert_bytes | (uintptr_t)c.b | (uintptr_t)(c.b_row_stride * 4)) & 15)
        return refuse("mul_mat_id: F16 / BF16 experts and b must be 16-byte aligned (pointers and strides)");
    if (c.b_row_stride < c.K) return refuse("mul_mat_id: b_row_stride < K");
    if (c.dst_row_stride < c.M) return refuse("mul_mat_id: dst_row_stride < M");
    // 32-bit row offsets inside a tile (the LDS-DMA's lane offset), as in f16_make_plan; int32 counters in k_moe_plan
    if (c.w_row_bytes < 2 * c.K || c.w_row_bytes > (int64_t)1 << 23 || c.w_expert_bytes < 0) return refuse("mul_mat_id: w_row_bytes must lie in [2 K, 2^23]");
    const int64_t pairs = c.n_tok * c.n_used;
    if (c.M > (int64_t)1 << 30 || c.n_tok > (int64_t)1 << 30 || c.n_used > (int64_t)1 << 30 || pairs > (int64_t)1 << 30) return refuse("mul_mat_id: too many rows or columns");
    if (pairs <= moe_f16_gemv_max() && pairs <= 65535) {
        pl.gx = (unsigned)((c.M + F16_GEMV_ROWS - 1) / F16_GEMV_ROWS); pl.gy = (unsigned)pairs;
        return pl;
    }
    if (c.n_expert > 1024) return refuse("mul_mat_id: more than 1024 F16 / BF16 experts above the per-column crossover");
    if (!c.workspace || ((uintptr_t)c.workspace & 255)) return refuse("mul_mat_id: workspace must be 256-byte aligned");
    pl.ws = moe_f16_carve(c.n_expert, c.n_used, c.n_tok);
    if (c.workspace_bytes < pl.ws.total) return refuse("mul_mat_id: workspace too small");
    // TN: a whole 128-row record per work-group.  The starting rule — 32-row fragments where pairs <= 32 * n_expert, the quantized path's threshold — lost where it was
    // timed (same table, TN 32 | TN 128: 128 columns, 16 rows per expert, 110 | 90 and 109 | 86; 1024 columns 128 | 110 and 126 | 105), so the fragment form is
    // reached through CDNA4_F16_MOE_TN=32 only (A/B timing, and the tests).  Not timed: more than 8 experts, the two forms against each other below 16 rows per expert.
    const char *tn_env = getenv("CDNA4_F16_MOE_TN");
    pl.tn = tn_env && atoi(tn_env) == 32 ? 32 : 128;
    const int64_t groups = ((c.M + F16_GEMM_TM - 1) / F16_GEMM_TM) * (pl.ws.img_rows / 128) * (pl.tn == 32 ? 4 : 1);
    if (groups > (int64_t)0x7FFFFFFF) return refuse("mul_mat_id: too many tiles for one launch");
    pl.route = MOE_F16_GEMM;
    pl.y16 = (((uintptr_t)c.dst | (uintptr_t)(c.dst_row_stride * 4)) & 15) == 0;
    pl.gx = (unsigned)groups; pl.gy = 1;
    return pl;
}
