// moe_f16.hip — MUL_MAT_ID on F16 / BF16 expert stacks (F32 activations rounded to the weights' format first, fp32 accumulation: DESIGN 4.12 / 4.13 / 4.14), and the
// part of ggml_cdna4_mul_mat_id that serves them: plan (moe_f16_plan.hpp), execute.  Nothing here waits for another work-group, and nothing splits K: every output
// element is one column's own fp32 sum in a fixed k order, whatever place k_moe_plan's atomics gave its row.
//   k_gemv_f16_ids<BF>      one (token, slot) column per blockIdx.y, eight weight rows per work-group (two per wave).  The work-group reads its expert id from `ids` —
//                           an id outside [0, n_expert) ends it before any other load — and streams that expert's rows in 16-byte lane chunks, eight loads in flight,
//                           against activation row tok * n_b + slot % n_b, rounded once into LDS (F16: kept as fp16; BF16: widened to fp32 in the two planes of k_gemv_bf16).
//   k_gemm_f16_ids<TN, BF>  k_moe_plan's tile table on the matrix cores: a work-group takes a 128 (M) x TN tile of ONE expert — TN 128: a whole 128-row tile record,
//                           TN 32: one of its four 32-row fragments — in the planner's order (fullest records first), the m index fastest, so that the work-groups in flight
//                           share one gathered activation tile in L2 and each weight tile is read once.  k_gemm_f16's stage structure: the weight tile goes by LDS-DMA
//                           into a three-slot swizzled ring, two stages ahead; the activation rows are GATHERED — float4 loads straight from b + img_src[row] *
//                           b_row_stride, no intermediate image — rounded behind the stage's MFMAs, one stage ahead.  Stores SCATTER: column n goes to dst + img_dst[row] *
//                           dst_row_stride; padding rows (img_src < 0) read the tile's first row and are never stored.
// LDS map of k_gemm_f16_ids, per ring slot: [128 weight rows x 64 B][TN activation rows x 64 B] (48 KB / 30 KB in all); a row holds its four 16-byte k-chunks at
// chunk ^ ((row >> 2) & 3), as in k_gemm_f16.
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
#define MOE_F16_KC 2048                                 // k per pass: the column's activations in LDS (fp16: 4 KB; bf16 widened to fp32: 8 KB)
template <bool BF>
__global__ __launch_bounds__(256) void k_gemv_f16_ids(const moe_f16_args p) {
    constexpr int NCH = MOE_F16_KC / 8;                                             // chunks (of eight k) per pass
    __shared__ __attribute__((aligned(16))) uint8_t smem[MOE_F16_KC * (BF ? 4 : 2)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.y, tok = col / p.n_used, slot = col % p.n_used;
    const int e = p.ids[(int64_t)tok * p.ids_tok_stride + slot];
    if (e < 0 || e >= p.n_expert) return;                                           // (work-group-uniform, before any barrier) the slot stays unwritten
    const int row0 = blockIdx.x * F16_GEMV_ROWS + wave * 2;                         // this wave's two weight rows (past M: row M - 1, not stored)
    const uint8_t *const we = p.W + (int64_t)e * p.w_expert_bytes;
    const uint8_t *const w0 = we + (int64_t)min(row0, p.M - 1) * p.w_row_bytes, *const w1 = we + (int64_t)min(row0 + 1, p.M - 1) * p.w_row_bytes;
    const float *const xrow = p.X + ((int64_t)tok * p.n_b + slot % p.n_b) * p.x_row_stride;      // slot u reads activation row u % n_b
    float acc0 = 0.f, acc1 = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += MOE_F16_KC) {
        const int kc = min(MOE_F16_KC, p.K - k0);
        if (k0) __syncthreads();
        // the column's activations of this pass, rounded once per work-group (nearest even; bf16: no subnormal flush, kept as fp32 in two planes — plane h holds
        // k 4 h .. 4 h + 3 of every 8-k chunk, so consecutive lanes read consecutive 16-byte pieces)
        for (int q = tid; q < kc / 4; q += 256) {
            const float4 v = *(const float4 *)(xrow + k0 + 4 * q);
            if constexpr (BF) {
                *(f32x4 *)(smem + ((q & 1) * NCH + (q >> 1)) * 16) = f32x4{(float)(__bf16)v.x, (float)(__bf16)v.y, (float)(__bf16)v.z, (float)(__bf16)v.w};
            } else {
                half4_t h; h[0] = (half_t)v.x; h[1] = (half_t)v.y; h[2] = (half_t)v.z; h[3] = (half_t)v.w;
                *(half4_t *)(smem + 8 * q) = h;
            }
        }
        __syncthreads();
        const int nch = kc / 8;                                                     // 16-byte chunks per row: lane l takes l, l + 64, ..
        for (int c = lane; c < nch; c += 256) {
            u32x4 wa[4], wc[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {                                           // all eight loads first; a chunk past the row reads chunk c again and is not used
                const int cc = c + 64 * j < nch ? c + 64 * j : c;
                wa[j] = ld_u32x4(w0 + (int64_t)(k0 + cc * 8) * 2); wc[j] = ld_u32x4(w1 + (int64_t)(k0 + cc * 8) * 2);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (c + 64 * j >= nch) break;
                if constexpr (BF) {
                    // a bf16 is the upper half of its fp32: dword d holds weight 2 d in its low half (a shift) and weight 2 d + 1 in its high half (a mask)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const f32x4 x = *(const f32x4 *)(smem + (h * NCH + c + 64 * j) * 16);
#pragma unroll
                        for (int d = 0; d < 2; d++) {
                            const uint32_t da = wa[j][2 * h + d], dc = wc[j][2 * h + d];
                            acc0 = fmaf(__builtin_bit_cast(float, da << 16), x[2 * d], acc0); acc0 = fmaf(__builtin_bit_cast(float, da & 0xFFFF0000u), x[2 * d + 1], acc0);
                            acc1 = fmaf(__builtin_bit_cast(float, dc << 16), x[2 * d], acc1); acc1 = fmaf(__builtin_bit_cast(float, dc & 0xFFFF0000u), x[2 * d + 1], acc1);
                        }
                    }
                } else {
                    const half8_t ha = __builtin_bit_cast(half8_t, wa[j]), hc = __builtin_bit_cast(half8_t, wc[j]);
                    const half8_t x = *(const half8_t *)(smem + (c + 64 * j) * 16);
#pragma unroll
                    for (int i = 0; i < 8; i++) { acc0 = fmaf((float)ha[i], (float)x[i], acc0); acc1 = fmaf((float)hc[i], (float)x[i], acc1); }
                }
            }
        }
    }
    const float s0 = wave_sum_dpp(acc0), s1 = wave_sum_dpp(acc1);
    if (lane == 0) {
        float *const yrow = p.Y + (int64_t)col * p.y_row_stride;
        if (row0 < p.M) yrow[row0] = s0;
        if (row0 + 1 < p.M) yrow[row0 + 1] = s1;
    }
}

// ------------------------------------------------------------------------------------------------ route 2: the planner's tiles on the matrix cores
#define MOE_F16_WST (F16_GEMM_TM * 64)                  // bytes of a weight stage: 128 rows x 32 halves
template <int TN, bool BF>
__global__ __launch_bounds__(256, 2) void k_gemm_f16_ids(const moe_f16_args p) {
    typedef typename f16_elem<BF>::v4 elem4_t; typedef typename f16_elem<BF>::v8 elem8_t;
    constexpr int XST = TN * 64, ST = MOE_F16_WST + XST, NST = 3;
    constexpr int NXL = TN / 32;                        // float4 loads per thread and stage
    constexpr int NBLK = TN == 128 ? 2 : 1;             // 32 x 32 blocks per wave and direction: a 64 x 64 / 32 x 32 wave tile
    constexpr int FPT = 128 / TN;                       // work-groups per tile record (and m tile)
    __shared__ __attribute__((aligned(16))) uint8_t smem[NST * ST];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the m index fastest, then (TN 32) the record's fragments, then the records in the planner's order: fullest first
    const int tile_m = (int)(blockIdx.x % (unsigned)p.tiles_m), j_rec = (int)(blockIdx.x / (unsigned)p.tiles_m);
    const int rec = __builtin_amdgcn_readfirstlane(p.tile_order[j_rec / FPT]), frag0 = j_rec % FPT;
    const int expert = __builtin_amdgcn_readfirstlane(p.tile_expert[rec]), nfrag = __builtin_amdgcn_readfirstlane(p.tile_nfrag[rec]);
    if (expert < 0 || frag0 * (TN / 32) >= nfrag) return;                           // (work-group-uniform, before any load or barrier) an unused record, an empty fragment
    const int m0 = tile_m * F16_GEMM_TM, n0 = rec * 128 + frag0 * TN;               // first weight row; first image row
    const uint8_t *const wb = p.W + (int64_t)expert * p.w_expert_bytes + (int64_t)m0 * p.w_row_bytes;
    const int K = p.K, nsteps = (K + 31) >> 5;
    const uint32_t lds0 = CDNA4_LDS_BASE(smem);

    // ---- the weight stage: eight 1 KB wave-pieces, two per wave.  LDS slot (16 bytes) q of a stage = row q / 4, stored chunk q % 4; rows past M read row M - 1
    uint32_t wrow[2]; int wchunk[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = (wave * 2 + i) * 64 + lane, r = q >> 2;
        wchunk[i] = (q & 3) ^ ((r >> 2) & 3);
        wrow[i] = (uint32_t)min(r, p.M - 1 - m0) * (uint32_t)p.w_row_bytes;
    }
    auto issue_w = [&](int s, int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int kc = 4 * s + wchunk[i];                                       // a chunk past K reads the row's first one: zero_tail() clears it
            const uint32_t voff = wrow[i] + (kc * 8 < K ? (uint32_t)kc * 16u : 0u);
            CDNA4_DMA16(voff, wb, lds0 + (uint32_t)(slot * ST + (wave * 2 + i) * 1024));
        }
    };
    // the chunks past K of the LAST stage, by the lane whose LDS-DMA wrote them and behind the wait for it: a stale NaN pattern times the other operand's zero is NaN
    auto zero_tail = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; i++)
            if ((4 * (nsteps - 1) + wchunk[i]) * 8 >= K) *(u32x4 *)(smem + slot * ST + (wave * 2 + i) * 1024 + 16 * lane) = u32x4{0u, 0u, 0u, 0u};
    };

    // ---- the activation stage: TN image rows x 32 k as float4 pieces, eight threads per row.  A thread resolves its rows ONCE: image row -> row of b; a padding row
    // (img_src < 0) reads the record's first row, which always holds one
    f32x4 xr[NXL]; const uint8_t *xrow[NXL]; int xlds[NXL];
    const int src_first = p.img_src[rec * 128];
#pragma unroll
    for (int i = 0; i < NXL; i++) {
        const int f = tid + 256 * i, r = f >> 3, kq = f & 7;
        const int src = p.img_src[n0 + r];
        xrow[i] = (const uint8_t *)(p.X + (int64_t)max(src < 0 ? src_first : src, 0) * p.x_row_stride);
        xlds[i] = MOE_F16_WST + r * 64 + (((kq >> 1) ^ ((r >> 2) & 3)) << 4) + (kq & 1) * 8;
    }
    auto xload = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NXL; i++) CDNA4_GLOAD16_PTR(xr[i], xrow[i] + (s * 32 + 4 * (tid & 7) < K ? s * 128 + 16 * (tid & 7) : 0));      // past K: the row's start, not used
    };
    auto xstore = [&](int s, int slot) __attribute__((always_inline)) {
        const bool in = s * 32 + 4 * (tid & 7) < K;
#pragma unroll
        for (int i = 0; i < NXL; i++) {
            elem4_t h;
            f16_round4(h, xr[i], in);
            *(elem4_t *)(smem + slot * ST + xlds[i]) = h;
        }
    };

    // ---- fragments: lane l holds row (l % 32) of a block, k 8 (l / 32) .. + 7 of a 16-k MFMA step
    const int wave_m = TN == 128 ? (wave & 1) * 64 : wave * 32, wave_n = TN == 128 ? (wave >> 1) * 64 : 0;
    const int frow = lane & 31, fsw = (frow >> 2) & 3, fh = lane >> 5;
    const int foff[2] = {frow * 64 + ((fh ^ fsw) << 4), frow * 64 + (((2 + fh) ^ fsw) << 4)};
    // TN 128: the wave's 32-row activation blocks that lie in fragments with rows (wave-uniform); no MFMA for the others
    bool live[NBLK];
#pragma unroll
    for (int bj = 0; bj < NBLK; bj++) live[bj] = TN == 32 || wave_n / 32 + bj < nfrag;
    floatx16 acc[NBLK][NBLK];
#pragma unroll
    for (int bi = 0; bi < NBLK; bi++)
#pragma unroll
        for (int bj = 0; bj < NBLK; bj++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[bi][bj][r] = 0.f;

    xload(0);
    issue_w(0, 0);
    if (nsteps > 1) { issue_w(1, 1); CDNA4_WAIT_VM(2); } else CDNA4_WAIT_VM(0);       // stage 0 of both operands has landed (stage 1's two pieces may fly)
#pragma unroll
    for (int i = 0; i < NXL; i++) CDNA4_WAIT_VM_TIED1(2, xr[i]);
    xstore(0, 0);
    if (nsteps == 1) zero_tail(0);

    int slot = 0;
    for (int s = 0; s < nsteps; s++) {
        const int slot1 = slot == 2 ? 0 : slot + 1, slot2 = slot1 == 2 ? 0 : slot1 + 1;
        // everyone's pieces of stage s are in LDS, and everyone is done reading stage s - 1 (slot2)
        CDNA4_WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool nx = s + 1 < nsteps, w2 = s + 2 < nsteps;
        if (nx) xload(s + 1);
        if (w2) issue_w(s + 2, slot2);
        const uint8_t *const ws = smem + slot * ST + wave_m * 64, *const xs = smem + slot * ST + MOE_F16_WST + wave_n * 64;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            elem8_t a[NBLK], b[NBLK];
#pragma unroll
            for (int bi = 0; bi < NBLK; bi++) a[bi] = *(const elem8_t *)(ws + bi * 2048 + foff[j]);
#pragma unroll
            for (int bj = 0; bj < NBLK; bj++) b[bj] = *(const elem8_t *)(xs + bj * 2048 + foff[j]);
#pragma unroll
            for (int bj = 0; bj < NBLK; bj++) {
                if (!live[bj]) continue;
#pragma unroll
                for (int bi = 0; bi < NBLK; bi++) acc[bi][bj] = f16_mfma(a[bi], b[bj], acc[bi][bj]);
            }
        }
        if (nx) {
            // the activation loads are older than stage s + 2's two pieces; behind vmcnt(2) stage s + 1's weight pieces (older still) have landed too
            if (w2) { CDNA4_WAIT_VM(2); } else { CDNA4_WAIT_VM(0); }
#pragma unroll
            for (int i = 0; i < NXL; i++) CDNA4_WAIT_VM_TIED1(2, xr[i]);
            xstore(s + 1, slot1);
            if (!w2) zero_tail(slot1);
        }
        slot = slot1;
    }

    // ---- store: accumulator values 4 g .. 4 g + 3 of a lane are rows m .. m + 3 of the column its image row names; a padding row names none
#pragma unroll
    for (int bj = 0; bj < NBLK; bj++) {
        if (!live[bj]) continue;
        const int dcol = p.img_dst[n0 + wave_n + 32 * bj + (lane & 31)];
        if (dcol < 0) continue;
        float *const yrow = p.Y + (int64_t)dcol * p.y_row_stride;
#pragma unroll
        for (int bi = 0; bi < NBLK; bi++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int m = m0 + wave_m + 32 * bi + 8 * g + 4 * fh;
                const floatx16 &c = acc[bi][bj];
                if (p.y16 && m + 3 < p.M) *(float4 *)(yrow + m) = make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
                else
#pragma unroll
                    for (int e = 0; e < 4; e++) if (m + e < p.M) yrow[m + e] = c[4 * g + e];
            }
    }
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
    if (bf) {
        if (pl.tn == 128) hipLaunchKernelGGL((k_gemm_f16_ids<128, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((k_gemm_f16_ids<32, true>), grid, dim3(256), 0, st, p);
    } else {
        if (pl.tn == 128) hipLaunchKernelGGL((k_gemm_f16_ids<128, false>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((k_gemm_f16_ids<32, false>), grid, dim3(256), 0, st, p);
    }
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
