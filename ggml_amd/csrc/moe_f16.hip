// moe_f16.hip — MUL_MAT_ID on F16 / BF16 expert stacks (F32 activations rounded to the weights' format first, fp32 accumulation: DESIGN 4.12 / 4.13 / 4.14), and the
// part of ggml_cdna4_mul_mat_id that serves them: plan (moe_f16_plan.hpp), execute.  Nothing here waits for another work-group, and nothing splits K: every output
// element is one column's own fp32 sum in a fixed k order, whatever place k_moe_plan's atomics gave its row.
//   k_gemv_f16_ids<BF>      one (token, slot) column per blockIdx.y, eight weight rows per work-group (two per wave).  The work-group reads its expert id from `ids` —
//                           an id outside [0, n_expert) ends it before any other load — and runs f16_gemv_stream (gemm_f16_dev.hpp) on that expert's rows against the
//                           ONE activation row tok * n_b + slot % n_b.
//   k_gemm_f16_ids<TN, BF>  k_moe_plan's tile table on the matrix cores: a work-group takes a 128 (M) x TN tile of ONE expert — TN 128: a whole 128-row tile record,
//                           TN 32: one of its four 32-row fragments — in the planner's order (fullest records first), the m index fastest, so that the work-groups in flight
//                           share one gathered activation tile in L2 and each weight tile is read once — and runs f16_gemm_tile (gemm_f16_dev.hpp) on it.  The activation
//                           rows are GATHERED — the tile's float4 loads go straight to b + img_src[row] * b_row_stride, no intermediate image.  Stores SCATTER: column n
//                           goes to dst + img_dst[row] * dst_row_stride; padding rows (img_src < 0) read the record's first row and are never stored.
#include "../../include/ggml_cdna4_f16.h"
#include "cdna4_common.h"
#include "cdna4_kernels.h"
#include "gemm_f16_dev.hpp"
#include "gemm_q_hw.h"
#include "moe_f16_plan.hpp"

struct moe_f16_args {
    const uint8_t *W; int64_t w_row_bytes, w_expert_bytes;                      // row m of expert e: W + e * w_expert_bytes + m * w_row_bytes, K 2-byte weights
    const float *X; int64_t x_row_stride;                                       // fp32 activation rows, stride in elements
    float *Y; int64_t y_row_stride;                                             // Y[(token, slot)][m], m contiguous
    const int32_t *ids; int64_t ids_tok_stride;                                 // k_gemv_f16_ids
    const int32_t *img_src, *img_dst, *tile_expert, *tile_order, *tile_nfrag;   // k_gemm_f16_ids: what k_moe_plan left (quantize_act.hip)
    int M, K, n_expert, n_used, n_b;
    int tiles_m, y16;                                                           // k_gemm_f16_ids: 128-row m tiles; dst rows take 16-byte stores
};

// ------------------------------------------------------------------------------------------------ route 1: one column per work-group row
template <bool BF>
__global__ __launch_bounds__(256) void k_gemv_f16_ids(const moe_f16_args p) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[F16_GEMV_LDS(1, BF)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.y, tok = col / p.n_used, slot = col % p.n_used;
    const int e = p.ids[(int64_t)tok * p.ids_tok_stride + slot];
    if (e < 0 || e >= p.n_expert) return;                                           // (work-group-uniform, before any barrier) the slot stays unwritten
    const int row0 = blockIdx.x * F16_GEMV_ROWS + wave * 2;                         // this wave's two weight rows (past M: row M - 1, not stored)
    const uint8_t *const we = p.W + (int64_t)e * p.w_expert_bytes;
    const uint8_t *const w0 = we + (int64_t)min(row0, p.M - 1) * p.w_row_bytes, *const w1 = we + (int64_t)min(row0 + 1, p.M - 1) * p.w_row_bytes;
    const float *const xrow = p.X + ((int64_t)tok * p.n_b + slot % p.n_b) * p.x_row_stride;      // slot u reads activation row u % n_b
    float s0[1], s1[1];
    f16_gemv_stream<1, BF>(s0, s1, smem, w0, w1, [&](int) __attribute__((always_inline)) { return xrow; }, p.K);
    if (lane == 0) {
        float *const yrow = p.Y + (int64_t)col * p.y_row_stride;
        if (row0 < p.M) yrow[row0] = s0[0];
        if (row0 + 1 < p.M) yrow[row0 + 1] = s1[0];
    }
}

// ------------------------------------------------------------------------------------------------ route 2: the planner's tiles on the matrix cores
template <int TN>
struct moe_f16_tile {                                   // what f16_gemm_tile asks: image rows n0 .. n0 + TN - 1 of a record with nfrag 32-row fragments, weight rows from m0
    const uint8_t *wb; int64_t w_nb1; int m0, M, y16;
    const moe_f16_args &p; int n0, nfrag, src_first;
    // image row -> row of b; a padding row (img_src < 0) reads the record's first row, which always holds one
    __device__ __forceinline__ const uint8_t *xrow(int r) const {
        const int src = p.img_src[n0 + r];
        return (const uint8_t *)(p.X + (int64_t)max(src < 0 ? src_first : src, 0) * p.x_row_stride);
    }
    // TN 128: the 32-row blocks that lie in fragments with rows
    __device__ __forceinline__ bool live(int b) const { return TN == 32 || b < nfrag; }
    // the column an image row names; a padding row names none
    __device__ __forceinline__ bool yrow(int c, float *&y) const {
        const int dcol = p.img_dst[n0 + c];
        y = p.Y + (int64_t)dcol * p.y_row_stride;
        return dcol >= 0;
    }
};
template <int TN, bool BF>
__global__ __launch_bounds__(256, 2) void k_gemm_f16_ids(const moe_f16_args p) {
    constexpr int FPT = 128 / TN;                       // work-groups per tile record (and m tile)
    __shared__ __attribute__((aligned(16))) uint8_t smem[F16_TILE_LDS(TN)];
    // the m index fastest, then (TN 32) the record's fragments, then the records in the planner's order: fullest first
    const int tile_m = (int)(blockIdx.x % (unsigned)p.tiles_m), j_rec = (int)(blockIdx.x / (unsigned)p.tiles_m);
    const int rec = __builtin_amdgcn_readfirstlane(p.tile_order[j_rec / FPT]), frag0 = j_rec % FPT;
    const int expert = __builtin_amdgcn_readfirstlane(p.tile_expert[rec]), nfrag = __builtin_amdgcn_readfirstlane(p.tile_nfrag[rec]);
    if (expert < 0 || frag0 * (TN / 32) >= nfrag) return;                           // (work-group-uniform, before any load or barrier) an unused record, an empty fragment
    const int m0 = tile_m * F16_GEMM_TM, n0 = rec * 128 + frag0 * TN;               // first weight row; first image row
    const moe_f16_tile<TN> t = {p.W + (int64_t)expert * p.w_expert_bytes + (int64_t)m0 * p.w_row_bytes, p.w_row_bytes, m0, p.M, p.y16, p, n0, nfrag, p.img_src[rec * 128]};
    f16_gemm_tile<TN, BF>(smem, t, p.K);
}

// ------------------------------------------------------------------------------------------------ host
static moe_f16_args moe_f16_args_of(const mmid_call &c) {
    moe_f16_args p{};
    p.W = (const uint8_t *)c.as; p.w_row_bytes = c.w_row_bytes; p.w_expert_bytes = c.w_expert_bytes;
    p.X = c.b; p.x_row_stride = c.b_row_stride;
    p.Y = c.dst; p.y_row_stride = c.dst_row_stride;
    p.ids = c.ids; p.ids_tok_stride = c.ids_tok_stride;
    p.M = (int)c.M; p.K = (int)c.K; p.n_expert = (int)c.n_expert; p.n_used = (int)c.n_used; p.n_b = (int)c.n_b;
    return p;
}

// ggml_cdna4_mul_mat_id on F16 / BF16 experts (capi.hip branches here behind its fault-status check): plan, execute
int cdna4_mul_mat_id_f16(const mmid_call &c, hipStream_t st) {
    const moe_f16_plan pl = moe_f16_make_plan(c);
    if (pl.route == MOE_F16_REFUSED) return cdna4_set_error_msg(pl.err);
    if (pl.empty) return 0;
    moe_f16_args p = moe_f16_args_of(c);
    const bool bf = c.type == CDNA4_BF16;
    const dim3 grid(pl.gx, pl.gy);
    if (pl.route == MOE_F16_GEMV) {
        if (bf) hipLaunchKernelGGL(k_gemv_f16_ids<true>, grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(k_gemv_f16_ids<false>, grid, dim3(256), 0, st, p);
        CDNA4_CHECK_LAUNCH();
        return 0;
    }
    uint8_t *const ws = (uint8_t *)c.workspace;
    int32_t *const img_src = (int32_t *)(ws + pl.ws.off_src), *const img_dst = (int32_t *)(ws + pl.ws.off_dst), *const tiles = (int32_t *)(ws + pl.ws.off_tiles);
    if (const int rc = cdna4_launch_moe_plan(c.ids, c.ids_tok_stride, (int)c.n_tok, (int)c.n_used, (int)c.n_b, (int)c.n_expert, (int)pl.ws.img_rows, img_src, img_dst, tiles, st)) return rc;
    const int ntile = (int)(pl.ws.img_rows / 128);
    p.img_src = img_src; p.img_dst = img_dst; p.tile_expert = tiles; p.tile_order = tiles + ntile; p.tile_nfrag = tiles + 2 * ntile;     // (k_moe_plan writes the three back to back)
    p.tiles_m = (int)((c.M + F16_GEMM_TM - 1) / F16_GEMM_TM); p.y16 = pl.y16 ? 1 : 0;
    if (pl.tn == 128) F16_LAUNCH(k_gemm_f16_ids, 128, bf, grid, st, p);
    else F16_LAUNCH(k_gemm_f16_ids, 32, bf, grid, st, p);
    CDNA4_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int ggml_cdna4_mul_mat_id_f16_route(int type, const void *as, int64_t w_row_bytes, int64_t w_expert_bytes, const float *b, int64_t b_row_stride, int64_t b_tok_stride,
                                    const int32_t *ids, int64_t ids_tok_stride, float *dst, int64_t dst_row_stride, int64_t dst_tok_stride,
                                    int64_t M, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok, void *workspace, size_t workspace_bytes) {
    const mmid_call c = {type, as, w_row_bytes, w_expert_bytes, b, b_row_stride, b_tok_stride, ids, ids_tok_stride, dst, dst_row_stride, dst_tok_stride, M, K, n_expert, n_used, n_b, n_tok, workspace, workspace_bytes};
    return moe_f16_make_plan(c).route;
}

}  // extern "C"
