// mmq_i8.hip — small batches (2 .. 64 activation rows) of the quantized MUL_MAT on the INT8 matrix cores.
//
// Between the one-row decode GEMV and the fp16 prefill GEMM there was nothing matrix-shaped: 2..8 rows ran the v_dot4_i32_i8 GEMV with eight
// columns per weight unit (27 us at 4096 x 14336 x 8 where one pass over the weights takes 10), 9..64 rows a mostly empty 128-row fp16 tile
// (31-35 us).  This kernel computes exactly what ggml_vec_dot_q4_K_q8_K computes (src/ggml-cpu/ggml-cpu-quants.c:5549-6194) — the INTEGER block
// dot products of the 4-bit weights with the Q8_K-quantized activations, then the fp32 scale products per superblock — but sixteen activation rows
// by sixteen weight rows by one 32-weight sub-block per instruction: v_mfma_i32_16x16x32_i8.  The integer sums are exact, so the result agrees
// with the GEMV units (and the CPU) to fp32 summation order, not to the fp16 rounding of the prefill GEMM.
//   reference dispatcher being replaced: ggml-cuda picks mul_mat_vec_q up to 8 columns and mmq above (src/ggml-cuda/ggml-cuda.cu:1844-1905, mmvq.cuh:3)
//
// MI355X mapping.  HBM-bound like the GEMV (each weight byte is read once); the matrix core only has to keep up.
//   * work-group = 16 weight rows, 8 waves; wave w takes the superblocks sb = w, w + 8, ... of those rows (the K split stays inside the
//     work-group: partial 16 x NB tiles meet in LDS at the end) — 256 work-groups at M = 4096, one per CU, like the one-launch decode kernel;
//   * MFMA operands: A = activations (rows = b), B = weights (columns = m).  Lane l supplies, for BOTH, row / column l % 16 and the eight
//     consecutive k of group l / 16 — so a lane holds the bytes of ITS weight row and decodes that row's 6-bit scales itself, and the
//     accumulator lane (column m = l % 16, rows b = 4 (l / 16) + i) needs nothing from other lanes on the weight side;
//   * weights come straight from global memory in that layout: per 64-weight group one 8-byte load per lane (low nibbles = sub-block 2g,
//     high = 2g + 1: two MFMAs per load), the 16-byte header once per superblock (the four lanes of a row load the same bytes: one L1 line);
//     the next superblock's loads are issued before the current one's arithmetic;
//   * activation side per superblock: eight 8-byte fragments per 16-column group, and per wave the sixteen columns' d and bsums pair sums staged
//     through a private LDS slot (lane (b, part) loads four bsums, adds them in pairs) for the minimum term sum_j m_j (bsums[2j] + bsums[2j+1]);
//   * per superblock and lane: sumi[i] = sum_j sc_j S_j[i] and summs[i] = sum_j m_j bs_j[i] in int32 (v_mad_i32_i24), then
//     acc[i] += (d dy_i) sumi[i] - (dmin dy_i) summs[i] in fp32 — the association of ggml_vec_dot_q4_K_q8_K's scalar body.
#include "cdna4_common.h"
#include "cdna4_formats.hpp"
#include "cdna4_kernels.h"
#include "epilogue.h"

typedef int intx4 __attribute__((ext_vector_type(4)));

struct mmq_args {
    const uint8_t *W; int64_t w_row_bytes;
    const int8_t *qs; const float *d; const int16_t *bsums;           // Q8_K activations (quantize_act.hip): [B][K], [B][K/256], [B][K/16]
    float *Y; int64_t y_row;                                          // Y[b * y_row + m]
    int M, K, B;
    cdna4_epilogue epi;
    // grouped MUL_MAT_ID (round 4): the activations are the EXPERT-SORTED image k_moe_plan lays out (every expert's run padded to 128 rows); blockIdx.y = a
    // chunk of 16 NCG image rows; tile_expert[row / 128] = its expert (-1: unused tile), row_dst[row] = the (token, slot) output row (-1: padding)
    const int32_t *tile_expert, *row_dst; int64_t w_expert_bytes;
};
// entry of every kernel: the grouped form re-bases the argument block onto its chunk and expert (work-group-uniform; false = nothing to do here)
template <int NCG> __device__ __forceinline__ bool mmq_ids_rebase(mmq_args &a, int d_per_row) {
    if (!a.tile_expert) return true;
    const int b0 = blockIdx.y * 16 * NCG;
    const int e = a.tile_expert[b0 >> 7];
    if (e < 0 || a.row_dst[b0] < 0) return false;                       // unused tile, or a chunk past the expert's run (runs are packed from the tile's start)
    a.W += (int64_t)e * a.w_expert_bytes;
    a.qs += (int64_t)b0 * a.K; a.d += (int64_t)b0 * d_per_row; if (a.bsums) a.bsums += (int64_t)b0 * (a.K / 16);
    a.row_dst += b0;
    a.B = min(a.B - b0, 16 * NCG);
    return true;
}
__device__ __forceinline__ void mmq_store(const mmq_args &a, float s, int m, int b) {
    if (a.row_dst) { const int pr = b < a.B ? a.row_dst[b] : -1; if (pr >= 0 && m < a.M) a.Y[(int64_t)pr * a.y_row + m] = s; }
    else if (b < a.B && m < a.M) a.Y[(int64_t)b * a.y_row + m] = epilogue_apply(a.epi, s, m, b);
}

__device__ __forceinline__ u32x2 ld_u32x2_a4(const void *p) { return *reinterpret_cast<const u32x2 *>(p); }
// 24-bit integer multiply (v_mul_i32_i24: full rate; the 32-bit v_mul_lo_u32 is a quarter of it) — both factors fit by construction here
#if defined(__HIPCC__)
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }
#else
static inline int mul24(int a, int b) { return a * b; }
#endif
__device__ __forceinline__ long as_i64(uint32_t lo, uint32_t hi) { return (long)(((uint64_t)hi << 32) | lo); }

// NCG column groups of 16 activation rows each (B <= 16 NCG); NW waves per work-group share the 16 weight rows and split the superblocks.
// Memory side (second version; the first loaded every MFMA operand straight into its lane — 8 bytes per lane, sixteen rows 32 bytes each per
// instruction — and was bound by the address coalescer: 25 us at 4096 x 14336 x 16): per superblock a wave fetches its slab with COALESCED 16-byte
// loads — the sixteen columns' 256 quants (4 instructions per column group), their bsums and d, the sixteen rows' 144-byte superblocks (3
// instructions) — one superblock AHEAD into registers, parks it in a private LDS area and reads the MFMA fragments from there (ds_read_b64, row
// strides 272 / 144 bytes: conflict-free).
// FIVE: Q5_K — the same superblock with 32 bytes of fifth bits behind the header (bit 2 gq of qh[l]: sub-block 2 gq's weight l, bit 2 gq + 1: sub-block
// 2 gq + 1's; src/ggml-quants.c:1482-1507): 176-byte rows, weights 0 .. 31 instead of 0 .. 15, everything else as Q4_K (ggml_vec_dot_q5_K_q8_K)
// What bounds it (round 6, profiles/r06/NOTES.md §3): the ACTIVATION traffic from the L2 — every 16-row work-group reads all B x K quantized activations, 59 MB at 16 rows of
// 4096 x 14336 beside 33 MB of weights, and a second column group costs as much again (11 -> 18 us).  Measured without effect on one box (mmq_prefetch_minmfma_ab.txt): the
// minimum term on the matrix core + byte-wise scale decode (loop VALU 201 -> 142) together with the weight slabs prefetched three superblocks ahead: 14.1-14.7 vs 14.0-14.4 us
// at 3-16 rows, 8.2 vs 7.9 at 4096^2 — not in the tree.  Fatter work-groups need a K split across work-groups, whose exchange cost what they saved (k_mmq_ks_q4_K, removed).
template <int NCG, int NW, bool FIVE = false>
__global__ __launch_bounds__(NW * 64) void k_mmq_q4_K(mmq_args a) {
    if (!mmq_ids_rebase<NCG>(a, a.K / 256)) return;
    constexpr int WB = FIVE ? 176 : 144, WP = WB / 16, NWI = (16 * WP + 63) / 64, QO = FIVE ? 48 : 16;
    constexpr int XROW = 272, XS = 16 * XROW, MS = 16 * 32, WSZ = 16 * WB;        // per wave: NCG x (quants | pair sums + d), then the weights
    constexpr int SLAB = NCG * (XS + MS) + WSZ;
    constexpr int SMEM = NW * SLAB > NW * NCG * 1024 ? NW * SLAB : NW * NCG * 1024;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) uint8_t smem[SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;                        // MFMA lane roles: row / column l % 16, k-group l / 16
    const int m0 = blockIdx.x * 16;
    const int nsb = a.K / 256;
    uint8_t *slab = smem + wave * SLAB;
    uint8_t *wl = slab + NCG * (XS + MS);

    float acc[NCG][4];
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[g][i] = 0.f;

    // ---- the slab of one superblock in registers: lane roles of the LOADS (coalesced), not of the MFMA
    struct Slab { u32x4 x[NCG][4]; u32x4 bs[NCG]; float dy[NCG]; u32x4 w[NWI]; };
    auto fetch = [&](int sb) __attribute__((always_inline)) {
        Slab r;
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {                                // piece i * 64 + lane: column 4 i + lane / 16, 16-byte chunk lane % 16
                const int b = min(g * 16 + 4 * i + (lane >> 4), a.B - 1);
                r.x[g][i] = ld_u32x4(a.qs + (int64_t)b * a.K + sb * 256 + (lane & 15) * 16);
            }
            const int bb = min(g * 16 + (lane >> 1), a.B - 1), bd = min(g * 16 + (lane & 15), a.B - 1);
            r.bs[g] = lane < 32 ? ld_u32x4(a.bsums + (int64_t)bb * (a.K / 16) + sb * 16 + (lane & 1) * 8) : u32x4{0, 0, 0, 0};
            r.dy[g] = a.d[(int64_t)bd * nsb + sb];
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) {                                  // piece i * 64 + lane of 16 WP: row piece / WP, chunk piece % WP
            const int pc = min(i * 64 + lane, 16 * WP - 1), row = pc / WP, c = pc - row * WP;
            r.w[i] = ld_u32x4(a.W + (int64_t)min(m0 + row, a.M - 1) * a.w_row_bytes + (int64_t)sb * WB + c * 16);
        }
        return r;
    };
    auto park = [&](const Slab &r) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(slab + g * (XS + MS) + (4 * i + (lane >> 4)) * XROW + (lane & 15) * 16) = r.x[g][i];
            if (lane < 32) {                                             // eight bsums -> four pair sums (bsums[2j] + bsums[2j+1]: what a sub-block's minimum multiplies)
                const uint32_t v[4] = {r.bs[g].x, r.bs[g].y, r.bs[g].z, r.bs[g].w};
                int ps[4];
#pragma unroll
                for (int t = 0; t < 4; t++) ps[t] = (int)(int16_t)(v[t] & 0xFFFF) + (int)(int16_t)(v[t] >> 16);
                *reinterpret_cast<u32x2 *>(slab + g * (XS + MS) + XS + (lane >> 1) * 32 + (lane & 1) * 8) =
                    u32x2{(uint32_t)(ps[0] & 0xFFFF) | ((uint32_t)ps[1] << 16), (uint32_t)(ps[2] & 0xFFFF) | ((uint32_t)ps[3] << 16)};
            }
            if (lane < 16) *reinterpret_cast<float *>(slab + g * (XS + MS) + XS + lane * 32 + 16) = r.dy[g];
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) if (i * 64 + lane < 16 * WP) *reinterpret_cast<u32x4 *>(wl + (i * 64 + lane) * 16) = r.w[i];
    };

    Slab cur{};
    if (wave < nsb) cur = fetch(wave);
    for (int sb = wave; sb < nsb; sb += NW) {
        CDNA4_WAVE_LDS_SYNC();                                           // the previous superblock's fragment reads are over
        park(cur);
        CDNA4_WAVE_LDS_SYNC();
        if (sb + NW < nsb) cur = fetch(sb + NW);                         // the next slab streams in under this one's arithmetic
        // ---- this lane's weight row (column col of the MFMA's B operand): header, scales and minima (get_scale_min_k4, ggml-quants.c:631-638)
        const u32x4 hdr = *reinterpret_cast<const u32x4 *>(wl + col * WB);
        u32x2 wq[4], qh = {0, 0};
#pragma unroll
        for (int gq = 0; gq < 4; gq++) wq[gq] = *reinterpret_cast<const u32x2 *>(wl + col * WB + QO + 32 * gq + 8 * grp);
        if constexpr (FIVE) qh = *reinterpret_cast<const u32x2 *>(wl + col * WB + 16 + 8 * grp);
        const float dw = h2f(hdr.x & 0xFFFF), dmin = h2f(hdr.x >> 16);
        int sc[8], mn[8];
#pragma unroll
        for (int j = 0; j < 8; j++) k4_scale_min_rt(hdr.y, hdr.z, hdr.w, j, sc[j], mn[j]);
#pragma unroll
        for (int g = 0; g < NCG; g++) {
            const uint8_t *xs = slab + g * (XS + MS) + col * XROW + 8 * grp;
            intx4 sumi = {0, 0, 0, 0};
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {                             // 64-weight group gq: sub-blocks 2 gq (low nibbles) and 2 gq + 1 (high)
                const u32x2 xl = *reinterpret_cast<const u32x2 *>(xs + 64 * gq), xh = *reinterpret_cast<const u32x2 *>(xs + 64 * gq + 32);
                const intx4 z = {0, 0, 0, 0};
                uint32_t l0 = wq[gq].x & 0x0F0F0F0Fu, l1 = wq[gq].y & 0x0F0F0F0Fu, h0 = (wq[gq].x >> 4) & 0x0F0F0F0Fu, h1 = (wq[gq].y >> 4) & 0x0F0F0F0Fu;
                if constexpr (FIVE) {
                    l0 |= ((qh.x >> (2 * gq)) & 0x01010101u) << 4; l1 |= ((qh.y >> (2 * gq)) & 0x01010101u) << 4;
                    h0 |= ((qh.x >> (2 * gq + 1)) & 0x01010101u) << 4; h1 |= ((qh.y >> (2 * gq + 1)) & 0x01010101u) << 4;
                }
                const intx4 sl = __builtin_amdgcn_mfma_i32_16x16x32_i8(as_i64(xl.x, xl.y), as_i64(l0, l1), z, 0, 0, 0);
                const intx4 sh = __builtin_amdgcn_mfma_i32_16x16x32_i8(as_i64(xh.x, xh.y), as_i64(h0, h1), z, 0, 0, 0);
                // |S| <= 32 * 31 * 127 and sc < 64: 24-bit multiplies (full rate; v_mul_lo_u32 is a quarter of it)
#pragma unroll
                for (int i = 0; i < 4; i++) sumi[i] += mul24(sc[2 * gq], sl[i]) + mul24(sc[2 * gq + 1], sh[i]);
            }
            // minimum term and the fp32 scale products: rows b = 4 grp + i of this column group
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint8_t *mb = slab + g * (XS + MS) + XS + (4 * grp + i) * 32;
                const u32x4 ps = *reinterpret_cast<const u32x4 *>(mb);
                const float dy = *reinterpret_cast<const float *>(mb + 16);
                const uint32_t pw[4] = {ps.x, ps.y, ps.z, ps.w};
                int summs = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) summs += mul24(mn[2 * j], (int)(int16_t)(pw[j] & 0xFFFF)) + mul24(mn[2 * j + 1], (int)(int16_t)(pw[j] >> 16));
                acc[g][i] += (dw * dy) * (float)sumi[i] - (dmin * dy) * (float)summs;
            }
        }
    }
    // ---- the waves' partial tiles meet in LDS: [wave][group][4][64 lanes]
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) red[((wave * NCG + g) * 4 + i) * 64 + lane] = acc[g][i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int g = 0; g < NCG; g++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < NW; w++) s += red[((w * NCG + g) * 4 + i) * 64 + lane];
                const int b = g * 16 + 4 * grp + i, m = m0 + col;
                mmq_store(a, s, m, b);
            }
    }
}

// ---- Q4_0 / Q8_0 weights: Q8_0 activations (d per 32-block on both sides, no minima): per block and MFMA acc += (d_w d_y) S, the association of
// ggml_vec_dot_q4_0_q8_0 / q8_0_q8_0's scalar bodies (src/ggml-cpu/ggml-cpu-quants.c:2293-2310, 3335-...).  Same staging: eight 18- / 34-byte blocks
// of a row are 144 / 272 contiguous bytes (16-byte aligned for K % 256 == 0); the quants of a block sit 2 bytes behind its d, so a lane's eight
// bytes are either 4-byte aligned (odd blocks) or straddle three dwords (even blocks: v_alignbit).
template <int TYPE, int NCG, int NW>
__global__ __launch_bounds__(NW * 64) void k_mmq_q8_0act(mmq_args a) {
    if (!mmq_ids_rebase<NCG>(a, a.K / 32)) return;
    constexpr int BB = TYPE == CDNA4_Q4_0 ? 18 : 34, WROW = 8 * BB, WP = WROW / 16;      // bytes per block, per 256 weights of a row; 16-byte pieces: 9 / 17
    constexpr int XROW = 272, XS = 16 * XROW, MS = 16 * 32, WSZ = 16 * WROW;
    constexpr int SLAB = NCG * (XS + MS) + WSZ, NWI = (16 * WP + 63) / 64;               // weight load instructions per slab: 3 / 5
    constexpr int SMEM = NW * SLAB > NW * NCG * 1024 ? NW * SLAB : NW * NCG * 1024;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) uint8_t smem[SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int m0 = blockIdx.x * 16;
    const int nsb = a.K / 256;
    uint8_t *slab = smem + wave * SLAB;
    uint8_t *wl = slab + NCG * (XS + MS);

    float acc[NCG][4];
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[g][i] = 0.f;

    struct Slab { u32x4 x[NCG][4]; u32x4 dy[NCG]; u32x4 w[NWI]; };
    auto fetch = [&](int sb) __attribute__((always_inline)) {
        Slab r;
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int b = min(g * 16 + 4 * i + (lane >> 4), a.B - 1);
                r.x[g][i] = ld_u32x4(a.qs + (int64_t)b * a.K + sb * 256 + (lane & 15) * 16);
            }
            const int bb = min(g * 16 + (lane >> 1), a.B - 1);                       // the column's eight block scales: 32 bytes, two lanes
            r.dy[g] = lane < 32 ? ld_u32x4(a.d + (int64_t)bb * (a.K / 32) + sb * 8 + (lane & 1) * 4) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) {
            const int pc = min(i * 64 + lane, 16 * WP - 1), row = pc / WP, c = pc - row * WP;
            r.w[i] = ld_u32x4(a.W + (int64_t)min(m0 + row, a.M - 1) * a.w_row_bytes + (int64_t)sb * WROW + c * 16);
        }
        return r;
    };
    auto park = [&](const Slab &r) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(slab + g * (XS + MS) + (4 * i + (lane >> 4)) * XROW + (lane & 15) * 16) = r.x[g][i];
            if (lane < 32) *reinterpret_cast<u32x4 *>(slab + g * (XS + MS) + XS + (lane >> 1) * 32 + (lane & 1) * 16) = r.dy[g];
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) if (i * 64 + lane < 16 * WP) *reinterpret_cast<u32x4 *>(wl + (i * 64 + lane) * 16) = r.w[i];
    };
    // eight bytes at a 2-byte-aligned LDS offset: two aligned dwords, or three and a 16-bit funnel shift
    auto ld8_a2 = [&](const uint8_t *p, int off) __attribute__((always_inline)) -> u32x2 {
        if ((off & 3) == 0) return u32x2{*reinterpret_cast<const uint32_t *>(p + off), *reinterpret_cast<const uint32_t *>(p + off + 4)};
        const uint32_t w0 = *reinterpret_cast<const uint32_t *>(p + off - 2), w1 = *reinterpret_cast<const uint32_t *>(p + off + 2), w2 = *reinterpret_cast<const uint32_t *>(p + off + 6);
        return u32x2{(w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16)};
    };

    Slab cur{};
    if (wave < nsb) cur = fetch(wave);
    for (int sb = wave; sb < nsb; sb += NW) {
        CDNA4_WAVE_LDS_SYNC();
        park(cur);
        CDNA4_WAVE_LDS_SYNC();
        if (sb + NW < nsb) cur = fetch(sb + NW);
        const uint8_t *wr = wl + col * WROW;
#pragma unroll
        for (int blk = 0; blk < 8; blk++) {
            const float dw = h2f(*reinterpret_cast<const uint16_t *>(wr + blk * BB));
            u32x2 wv;
            if constexpr (TYPE == CDNA4_Q4_0) {
                // nibble j low -> weight j, high -> weight j + 16 (src/ggml-quants.c:255-273): k-groups 0, 1 = low nibbles of bytes 0-7 / 8-15, groups 2, 3 = the high ones
                const int o0 = blk * BB + 2;                             // (blk * 18 + 2) % 4 is 2 for even blocks, 0 for odd ones: both forms, selected per lane by its group
                const u32x2 lo8 = ld8_a2(wr, o0), hi8 = ld8_a2(wr, o0 + 8);
                const u32x2 raw = (grp & 1) ? hi8 : lo8;
                const uint32_t sh = (grp & 2) ? 4u : 0u;
                uint32_t t0 = ((raw.x >> sh) & 0x0F0F0F0Fu) ^ 0x08080808u, t1 = ((raw.y >> sh) & 0x0F0F0F0Fu) ^ 0x08080808u;
                wv = u32x2{t0 | ((t0 & 0x08080808u) * 0x1Eu), t1 | ((t1 & 0x08080808u) * 0x1Eu)};        // q - 8 as int8 (see convert_w.hip: flip bit 3, extend the sign)
            } else {
                // one of the four 8-byte pieces of the block's 32 int8 (offset 2 + 8 grp): the offset's alignment depends on the lane's group — read both
                // candidates' dwords once (five aligned dwords cover bytes [blk BB, blk BB + 36) from the nearest 4-byte boundary) and select
                const int o = blk * BB + 2;
                const u32x2 p0 = ld8_a2(wr, o), p1 = ld8_a2(wr, o + 8), p2 = ld8_a2(wr, o + 16), p3 = ld8_a2(wr, o + 24);
                wv = grp == 0 ? p0 : (grp == 1 ? p1 : (grp == 2 ? p2 : p3));
            }
#pragma unroll
            for (int g = 0; g < NCG; g++) {
                const u32x2 xv = *reinterpret_cast<const u32x2 *>(slab + g * (XS + MS) + col * XROW + 32 * blk + 8 * grp);
                const intx4 z = {0, 0, 0, 0};
                const intx4 sv = __builtin_amdgcn_mfma_i32_16x16x32_i8(as_i64(xv.x, xv.y), as_i64(wv.x, wv.y), z, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float dy = *reinterpret_cast<const float *>(slab + g * (XS + MS) + XS + (4 * grp + i) * 32 + 4 * blk);
                    acc[g][i] += (float)sv[i] * (dw * dy);
                }
            }
        }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) red[((wave * NCG + g) * 4 + i) * 64 + lane] = acc[g][i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int g = 0; g < NCG; g++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < NW; w++) s += red[((w * NCG + g) * 4 + i) * 64 + lane];
                const int b = g * 16 + 4 * grp + i, m = m0 + col;
                mmq_store(a, s, m, b);
            }
    }
}

// ---- Q6_K weights (Q8_K activations): ggml_vec_dot_q6_K_q8_K (src/ggml-cpu/ggml-cpu-quants.c:6944-...): per 16-weight sub-block j the integer dot of
// (q6 - 32) with the activation quants, times the sub-block's int8 scale, summed over the superblock in int32, then x (d_w d_y) in fp32.
// Differences to the kernels above: (1) a superblock is 210 bytes (ql[128] qh[64] scales[16] d), 2-byte aligned only — the slab is fetched as the
// fourteen 16-byte ALIGNED pieces that cover each row's run (never touching a 16-byte line the run does not touch, so never a page the tensor does
// not own) and every field is read from LDS at its 2-byte-aligned place through aligned dwords and a funnel shift; (2) the scale changes every
// SIXTEEN weights, and the MFMA contracts 32: each 32-weight block is multiplied twice, with the other half's weight bytes zeroed (k-groups 0, 1 =
// the first sub-block, 2, 3 = the second) — 16 MFMAs per superblock and column group; the matrix core has the time; (3) q6 - 32 is built as a signed
// byte (flip bit 5, extend the sign: t | (t & 0x20) * 7), so there is no minimum term and the bsums are not read.
template <int NCG, int NW>
__global__ __launch_bounds__(NW * 64) void k_mmq_q6_K(mmq_args a) {
    if (!mmq_ids_rebase<NCG>(a, a.K / 256)) return;
    constexpr int WB = 210, NPC = 14, WROW = 240;                      // bytes per superblock; aligned pieces covering any 2-byte-aligned run of 210; LDS row slot
    constexpr int NWI = (16 * NPC + 63) / 64;                          // 4 load instructions per slab
    constexpr int XROW = 272, XS = 16 * XROW, MS = 16 * 32, WSZ = 16 * WROW;
    constexpr int SLAB = NCG * (XS + MS) + WSZ;
    constexpr int SMEM = NW * SLAB > NW * NCG * 1024 ? NW * SLAB : NW * NCG * 1024;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(16))) uint8_t smem[SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int m0 = blockIdx.x * 16;
    const int nsb = a.K / 256;
    uint8_t *slab = smem + wave * SLAB;
    uint8_t *wl = slab + NCG * (XS + MS);
    const uint8_t *wrow_g = a.W + (int64_t)min(m0 + col, a.M - 1) * a.w_row_bytes;     // this lane's weight row (MFMA role)

    float acc[NCG][4];
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[g][i] = 0.f;

    struct Slab { u32x4 x[NCG][4]; float dy[NCG]; u32x4 w[NWI]; };
    auto fetch = [&](int sb) __attribute__((always_inline)) {
        Slab r;
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int b = min(g * 16 + 4 * i + (lane >> 4), a.B - 1);
                r.x[g][i] = ld_u32x4(a.qs + (int64_t)b * a.K + sb * 256 + (lane & 15) * 16);
            }
            r.dy[g] = a.d[(int64_t)min(g * 16 + (lane & 15), a.B - 1) * nsb + sb];
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) {                                  // piece i * 64 + lane of 16 x 14: row piece / 14, aligned piece piece % 14 of that row's run
            const int pc = min(i * 64 + lane, 16 * NPC - 1), row = pc / NPC, c = pc - row * NPC;
            const uintptr_t start = (uintptr_t)(a.W + (int64_t)min(m0 + row, a.M - 1) * a.w_row_bytes + (int64_t)sb * WB);
            r.w[i] = ld_u32x4(reinterpret_cast<const uint8_t *>((start & ~(uintptr_t)15) + 16 * c));
        }
        return r;
    };
    auto park = [&](const Slab &r) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NCG; g++) {
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(slab + g * (XS + MS) + (4 * i + (lane >> 4)) * XROW + (lane & 15) * 16) = r.x[g][i];
            if (lane < 16) *reinterpret_cast<float *>(slab + g * (XS + MS) + XS + lane * 32 + 16) = r.dy[g];
        }
#pragma unroll
        for (int i = 0; i < NWI; i++) {
            const int pc = i * 64 + lane, row = pc / NPC, c = pc - row * NPC;
            if (pc < 16 * NPC) *reinterpret_cast<u32x4 *>(wl + row * WROW + c * 16) = r.w[i];
        }
    };
    auto ld8_a2 = [&](const uint8_t *p, int off) __attribute__((always_inline)) -> u32x2 {
        if ((off & 3) == 0) return u32x2{*reinterpret_cast<const uint32_t *>(p + off), *reinterpret_cast<const uint32_t *>(p + off + 4)};
        const uint32_t w0 = *reinterpret_cast<const uint32_t *>(p + off - 2), w1 = *reinterpret_cast<const uint32_t *>(p + off + 2), w2 = *reinterpret_cast<const uint32_t *>(p + off + 6);
        return u32x2{(w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16)};
    };

    Slab cur{};
    if (wave < nsb) cur = fetch(wave);
    for (int sb = wave; sb < nsb; sb += NW) {
        CDNA4_WAVE_LDS_SYNC();
        park(cur);
        CDNA4_WAVE_LDS_SYNC();
        if (sb + NW < nsb) cur = fetch(sb + NW);
        // this lane's row inside its slot: the run starts (address & 15) bytes into the first piece
        const int o = (int)((uintptr_t)(wrow_g + (int64_t)sb * WB) & 15);
        const uint8_t *wr = wl + col * WROW;
        const u32x2 s01 = ld8_a2(wr, o + 192), s23 = ld8_a2(wr, o + 200);              // the sixteen int8 sub-block scales
        const uint32_t scw[4] = {s01.x, s01.y, s23.x, s23.y};
        const uint32_t dword = (o & 3) == 0 ? *reinterpret_cast<const uint32_t *>(wr + o + 208) : *reinterpret_cast<const uint32_t *>(wr + o + 206) >> 16;
        const float dw = h2f(dword & 0xFFFF);
        intx4 sumi[NCG];
#pragma unroll
        for (int g = 0; g < NCG; g++) sumi[g] = intx4{0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < 2; n++) {                                    // 128-weight halves (dequantize_row_q6_K, src/ggml-quants.c:1690-1716)
            const u32x2 qh = ld8_a2(wr, o + 128 + 32 * n + 8 * grp);     // qh[l], l = 8 grp .. 8 grp + 7: two bits for each of the half's four 32-weight blocks
#pragma unroll
            for (int pp = 0; pp < 2; pp++) {
                const u32x2 ql = ld8_a2(wr, o + 64 * n + 32 * pp + 8 * grp);             // ql[32 pp + l]: low nibbles -> block pp, high nibbles -> block pp + 2
#pragma unroll
                for (int hi = 0; hi < 2; hi++) {
                    const int quad = pp + 2 * hi, jj = 4 * n + quad;     // 32-weight block jj of the superblock = sub-blocks 2 jj, 2 jj + 1
                    uint32_t v0 = ((ql.x >> (4 * hi)) & 0x0F0F0F0Fu) | (((qh.x >> (2 * quad)) & 0x03030303u) << 4);
                    uint32_t v1 = ((ql.y >> (4 * hi)) & 0x0F0F0F0Fu) | (((qh.y >> (2 * quad)) & 0x03030303u) << 4);
                    v0 ^= 0x20202020u; v1 ^= 0x20202020u;                // q6 - 32 as int8: flip bit 5 ...
                    v0 |= (v0 & 0x20202020u) * 7u; v1 |= (v1 & 0x20202020u) * 7u;       // ... and extend the sign (0x20 x 7 = 0xE0: no carry between bytes)
                    const uint32_t a0 = grp < 2 ? v0 : 0u, a1 = grp < 2 ? v1 : 0u, b0 = grp < 2 ? 0u : v0, b1 = grp < 2 ? 0u : v1;
                    const int sca = (int)(int8_t)((scw[jj >> 1] >> (16 * (jj & 1))) & 0xFF), scb = (int)(int8_t)((scw[jj >> 1] >> (16 * (jj & 1) + 8)) & 0xFF);
#pragma unroll
                    for (int g = 0; g < NCG; g++) {
                        const u32x2 xv = *reinterpret_cast<const u32x2 *>(slab + g * (XS + MS) + col * XROW + 32 * jj + 8 * grp);
                        const intx4 z = {0, 0, 0, 0};
                        const intx4 sa = __builtin_amdgcn_mfma_i32_16x16x32_i8(as_i64(xv.x, xv.y), as_i64(a0, a1), z, 0, 0, 0);
                        const intx4 sb2 = __builtin_amdgcn_mfma_i32_16x16x32_i8(as_i64(xv.x, xv.y), as_i64(b0, b1), z, 0, 0, 0);
                        // |S| <= 16 * 32 * 127 = 65,024 and |sc| <= 128: the products fit 24 bits (8,323,072 < 2^23)
#pragma unroll
                        for (int i = 0; i < 4; i++) sumi[g][i] += mul24(sca, sa[i]) + mul24(scb, sb2[i]);
                    }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < NCG; g++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float dy = *reinterpret_cast<const float *>(slab + g * (XS + MS) + XS + (4 * grp + i) * 32 + 16);
                acc[g][i] += (dw * dy) * (float)sumi[g][i];
            }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int g = 0; g < NCG; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) red[((wave * NCG + g) * 4 + i) * 64 + lane] = acc[g][i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int g = 0; g < NCG; g++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < NW; w++) s += red[((w * NCG + g) * 4 + i) * 64 + lane];
                const int b = g * 16 + 4 * grp + i, m = m0 + col;
                mmq_store(a, s, m, b);
            }
    }
}

// (Round 6 built a K-SLICED one-launch form for 2 .. 32 rows of Q4_K — 128-row work-groups that quantize their K slice of the activations themselves and meet through parked
//  partials + tickets, k_mmq_ks_q4_K, commit "small batches: ..." — 2e-7 from the oracle and BEHIND the two launches below at every size: 4096 x 14336 14.5-18.8 us against
//  13.8-14.3, 4096^2 8.3-10.0 against 7.9 (profiles/r06/batch_ks_final.txt): a work-group's life there is a chain fetch -> quantize -> barrier -> multiply -> park -> ticket ->
//  the last one's sum, with nothing to overlap it.  Removed.)
bool cdna4_mmq_supported(int type, int64_t M, int64_t K, int64_t B) {
    if (type == CDNA4_Q6_K && B > 32) return false;                   // (its three- and four-group forms spill: two accumulator sets per block pair)
    return cdna4_type_is_main5(type) && M > 0 && K >= 256 && K % 256 == 0 && B >= 2 && B <= 64;
}
template <int TYPE>
static void launch_q80act(const mmq_args &a, int ncg, dim3 grid, hipStream_t st) {
    if (ncg == 1) hipLaunchKernelGGL((k_mmq_q8_0act<TYPE, 1, 8>), grid, dim3(512), 0, st, a);
    else if (ncg == 2) hipLaunchKernelGGL((k_mmq_q8_0act<TYPE, 2, 8>), grid, dim3(512), 0, st, a);
    else if (ncg == 3) hipLaunchKernelGGL((k_mmq_q8_0act<TYPE, 3, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_mmq_q8_0act<TYPE, 4, 4>), grid, dim3(256), 0, st, a);
}
// grouped MUL_MAT_ID on the int8 matrix cores (round 4; VERDICT r3 "missing 4"): g.qs / g.d / g.bsums = the quantized EXPERT-SORTED image (g.ncol rows, a
// multiple of 128), one launch over (16 weight rows) x (32-row chunks of the image); chunks past an expert's run exit.  For few rows per expert — where the
// grouped fp16 GEMM multiplies 128-row tiles that are mostly padding — and on the CPU's own integer arithmetic (rel-L2 ~2e-7 instead of 3e-4).
bool cdna4_mmq_ids_supported(int type, int64_t K) {
    return cdna4_type_is_main5(type) && K >= 256 && K % 256 == 0;
}
int cdna4_launch_mmq_ids(const cdna4_gemv_args &g, const int32_t *tile_expert, const int32_t *row_dst, int64_t w_expert_bytes, hipStream_t st) {
    if (!cdna4_mmq_ids_supported(g.type, g.K) || g.ncol % 128 || !tile_expert || !row_dst) return cdna4_set_error_msg("mmq_ids: unsupported type / shape");
    if (((uintptr_t)g.W | (uintptr_t)g.w_row_bytes | (uintptr_t)w_expert_bytes) & (g.type == CDNA4_Q6_K ? 1 : 15)) return cdna4_set_error_msg("mmq_ids: expert matrices must be 16-byte aligned (Q6_K: 2-byte)");
    if (((uintptr_t)g.qs | (uintptr_t)g.d | (uintptr_t)g.bsums) & 15) return cdna4_set_error_msg("mmq_ids: quantized activations must be 16-byte aligned");
    if (g.M <= 0 || g.ncol <= 0) return 0;
    mmq_args a{};
    a.W = g.W; a.w_row_bytes = g.w_row_bytes; a.qs = g.qs; a.d = g.d; a.bsums = g.bsums; a.Y = g.Y; a.y_row = g.y_col_stride;
    a.M = g.M; a.K = g.K; a.B = g.ncol;
    a.tile_expert = tile_expert; a.row_dst = row_dst; a.w_expert_bytes = w_expert_bytes;
    const dim3 grid((g.M + 15) / 16, g.ncol / 32);
    if (g.type == CDNA4_Q4_0) hipLaunchKernelGGL((k_mmq_q8_0act<CDNA4_Q4_0, 2, 8>), grid, dim3(512), 0, st, a);
    else if (g.type == CDNA4_Q8_0) hipLaunchKernelGGL((k_mmq_q8_0act<CDNA4_Q8_0, 2, 8>), grid, dim3(512), 0, st, a);
    else if (g.type == CDNA4_Q6_K) hipLaunchKernelGGL((k_mmq_q6_K<2, 8>), grid, dim3(512), 0, st, a);
    else if (g.type == CDNA4_Q5_K) hipLaunchKernelGGL((k_mmq_q4_K<2, 8, true>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((k_mmq_q4_K<2, 8>), grid, dim3(512), 0, st, a);
    CDNA4_CHECK_LAUNCH();
    return 0;
}
// a.qs / a.d / a.bsums: the Q8_K (Q4_K) or Q8_0 (Q4_0 / Q8_0) workspace ggml_cdna4_prepare_act fills (path GEMV)
int cdna4_launch_mmq(const cdna4_gemv_args &g, hipStream_t st) {
    if (!cdna4_mmq_supported(g.type, g.M, g.K, g.ncol) || g.ids) return cdna4_set_error_msg("mmq: unsupported type / shape");
    if (((uintptr_t)g.W | (uintptr_t)g.w_row_bytes) & (g.type == CDNA4_Q6_K ? 1 : 15)) return cdna4_set_error_msg("mmq: weight rows must be 16-byte aligned (Q6_K: 2-byte)");
    if (((uintptr_t)g.qs | (uintptr_t)g.d) & 15) return cdna4_set_error_msg("mmq: quantized activations must be 16-byte aligned");
    if ((g.type == CDNA4_Q4_K || g.type == CDNA4_Q5_K) && ((uintptr_t)g.bsums & 15)) return cdna4_set_error_msg("mmq: quantized activations must be 16-byte aligned");
    mmq_args a{};
    a.W = g.W; a.w_row_bytes = g.w_row_bytes; a.qs = g.qs; a.d = g.d; a.bsums = g.bsums; a.Y = g.Y; a.y_row = g.y_col_stride;
    a.M = g.M; a.K = g.K; a.B = g.ncol; a.epi = g.epi;
    const dim3 grid((g.M + 15) / 16);
    const int ncg = (g.ncol + 15) / 16;
    if (g.type == CDNA4_Q4_0) launch_q80act<CDNA4_Q4_0>(a, ncg, grid, st);
    else if (g.type == CDNA4_Q8_0) launch_q80act<CDNA4_Q8_0>(a, ncg, grid, st);
    else if (g.type == CDNA4_Q6_K) {
        if (ncg == 1) hipLaunchKernelGGL((k_mmq_q6_K<1, 8>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((k_mmq_q6_K<2, 8>), grid, dim3(512), 0, st, a);
    }
    else if (g.type == CDNA4_Q5_K) {
        if (ncg == 1) hipLaunchKernelGGL((k_mmq_q4_K<1, 8, true>), grid, dim3(512), 0, st, a);
        else if (ncg == 2) hipLaunchKernelGGL((k_mmq_q4_K<2, 8, true>), grid, dim3(512), 0, st, a);
        else if (ncg == 3) hipLaunchKernelGGL((k_mmq_q4_K<3, 8, true>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((k_mmq_q4_K<4, 4, true>), grid, dim3(256), 0, st, a);
    }
    else if (ncg == 1) hipLaunchKernelGGL((k_mmq_q4_K<1, 8>), grid, dim3(512), 0, st, a);
    else if (ncg == 2) hipLaunchKernelGGL((k_mmq_q4_K<2, 8>), grid, dim3(512), 0, st, a);
    else if (ncg == 3) hipLaunchKernelGGL((k_mmq_q4_K<3, 8>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((k_mmq_q4_K<4, 4>), grid, dim3(256), 0, st, a);
    CDNA4_CHECK_LAUNCH();
    return 0;
}
