// gemm_f16_dev.hpp — what the kernels on F16 / BF16 weights share (gemm_f16.hip: k_gemm_f16, k_gemv_f16; moe_f16.hip: k_gemm_f16_ids, k_gemv_f16_ids):
//   f16_elem / f16_round4 / f16_mfma   the 2-byte element of the matrix-core kernels: its vectors, the rounding of four fp32 activations to it, the matrix-core step on it
//   f16_gemm_tile<TN, BF>              ONE 128 (M) x TN tile over the whole K on the matrix cores: stages, counted waits, ring, stores.  The kernel says where the tile lies
//   f16_gemv_stream<NB, BF>            TWO weight rows per wave streamed against NB activation rows: rounding into LDS, passes, wave sums.  The kernel stores them
// Device code; kernel-library sources only.
#pragma once
#include "cdna4_common.h"
#include "gemm_f16_plan.hpp"
#include "gemm_q_hw.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// the 2-byte element of a matrix-core instantiation: its vectors, and the matrix-core step on them
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

// host: the <V, BF> instantiation of the kernel template `kern` for a run-time bf, 256 threads per work-group
#define F16_LAUNCH(kern, V, bf, grid, st, p)                                          \
    do {                                                                              \
        if (bf) hipLaunchKernelGGL((kern<V, true>), grid, dim3(256), 0, st, p);       \
        else hipLaunchKernelGGL((kern<V, false>), grid, dim3(256), 0, st, p);         \
    } while (0)

// ------------------------------------------------------------------------------------------------ the matrix-core tile
// 128 x TN tile (TN 32 / 128), 256 threads, K step 32, v_mfma_f32_32x32x16_f16 (BF: .._bf16, same shape and accumulator layout) with the WEIGHTS as the A operand: a
// lane's four consecutive accumulator values are four consecutive m, and a dst row is contiguous in m — 16-byte stores.  The weight tile goes from its 2-byte rows
// straight into a three-slot LDS ring by LDS-DMA, two stages ahead; the activation tile goes through registers (float4 loads issued before a stage's MFMAs, rounded —
// BF: v_cvt_pk_bf16_f32 — and written behind them), one stage ahead.  One barrier per K step.
// LDS map, per ring slot: [128 weight rows x 64 B][TN activation rows x 64 B]; a row holds its four 16-byte k-chunks at chunk ^ ((row >> 2) & 3), so the sixteen lanes
// of a ds_read_b128 phase (rows r .. r + 15, one chunk) touch sixteen different 16-byte columns of the 256-byte bank window.
// `smem` is the kernel's own __shared__ array.  The tile object `t` answers where the tile lies:
//   t.wb, t.w_nb1, t.m0, t.M    row 0 of the weight tile, the row stride in bytes, the tile's first weight row and their number (rows past M read row M - 1, not stored)
//   t.xrow(r)                   the fp32 activation row of tile row r (always a readable one)
//   t.live(b)                   whether the tile's 32-row activation block b takes part (wave-uniform): no MFMA and no store for the others
//   t.yrow(c, y), t.y16         whether tile column c is stored, and then its dst row y; whether dst rows take 16-byte stores
#define F16_WST (F16_GEMM_TM * 64)                      // bytes of a weight stage: 128 rows x 32 halves
#define F16_TILE_LDS(TN) (3 * (F16_WST + (TN) * 64))    // the three ring slots: 48 KB / 30 KB
template <int TN, bool BF, typename TILE>
__device__ __forceinline__ void f16_gemm_tile(uint8_t (&smem)[F16_TILE_LDS(TN)], const TILE &t, const int K) {
    typedef typename f16_elem<BF>::v4 elem4_t; typedef typename f16_elem<BF>::v8 elem8_t;
    constexpr int ST = F16_WST + TN * 64;
    constexpr int NXL = TN / 32;                        // float4 loads per thread and stage
    constexpr int NBLK = TN == 128 ? 2 : 1;             // 32 x 32 blocks per wave and direction: a 64 x 64 / 32 x 32 wave tile
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *const wb = t.wb;
    const int nsteps = (K + 31) >> 5;
    const uint32_t lds0 = CDNA4_LDS_BASE(smem);

    // ---- the weight stage: eight 1 KB wave-pieces, two per wave.  LDS slot (16 bytes) q of a stage = row q / 4, stored chunk q % 4; rows past M read row M - 1
    uint32_t wrow[2]; int wchunk[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = (wave * 2 + i) * 64 + lane, r = q >> 2;
        wchunk[i] = (q & 3) ^ ((r >> 2) & 3);
        wrow[i] = (uint32_t)min(r, t.M - 1 - t.m0) * (uint32_t)t.w_nb1;
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

    // ---- the activation stage: TN rows x 32 k as float4 pieces, eight threads per row.  A thread resolves its rows ONCE
    f32x4 xr[NXL]; const uint8_t *xrow[NXL]; int xlds[NXL];
#pragma unroll
    for (int i = 0; i < NXL; i++) {
        const int f = tid + 256 * i, r = f >> 3, kq = f & 7;
        xrow[i] = t.xrow(r);
        xlds[i] = F16_WST + r * 64 + (((kq >> 1) ^ ((r >> 2) & 3)) << 4) + (kq & 1) * 8;
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
    bool live[NBLK];
#pragma unroll
    for (int bj = 0; bj < NBLK; bj++) live[bj] = t.live(wave_n / 32 + bj);
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
        const uint8_t *const ws = smem + slot * ST + wave_m * 64, *const xs = smem + slot * ST + F16_WST + wave_n * 64;
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

    // ---- store: accumulator values 4 g .. 4 g + 3 of a lane are rows m .. m + 3 of the dst row its tile column names
#pragma unroll
    for (int bj = 0; bj < NBLK; bj++) {
        if (!live[bj]) continue;
        float *yrow;
        if (!t.yrow(wave_n + 32 * bj + (lane & 31), yrow)) continue;
#pragma unroll
        for (int bi = 0; bi < NBLK; bi++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int m = t.m0 + wave_m + 32 * bi + 8 * g + 4 * fh;
                const floatx16 &c = acc[bi][bj];
                if (t.y16 && m + 3 < t.M) *(float4 *)(yrow + m) = make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
                else
#pragma unroll
                    for (int e = 0; e < 4; e++) if (m + e < t.M) yrow[m + e] = c[4 * g + e];
            }
    }
}

// ------------------------------------------------------------------------------------------------ the few-row stream
// A wave streams its TWO weight rows w0 / w1 (K 2-byte weights each) in 16-byte lane chunks (1 KB per wave load, eight loads in flight) against NB fp32 activation rows —
// xrow(n) names row n's — which the work-group (256 threads, all of them call this) rounds to the weights' format once into LDS, F16_GEMV_KC k per pass; fp32 FMAs in
// ascending k per lane, DPP wave sums (all 64 lanes active): s0[n] / s1[n] = row w0 / w1 times activation row n, in every lane.
// F16: the rows lie in LDS as fp16 (NB x 4 KB).  BF16: a bf16 is the upper half of its fp32, so a weight dword becomes two fp32 by a shift and a mask (once per chunk,
// shared by the NB rows), and the activations lie in LDS rounded to bf16 but already WIDENED to fp32 — the FMAs read them as they are.  Per activation row two planes of
// KC / 8 float4 — plane h holds k 4 h .. 4 h + 3 of every 8-k chunk, so the lanes of a wave (consecutive chunks) read consecutive 16-byte pieces: no bank conflict.  NB x 8 KB.
#define F16_GEMV_KC 2048                                                            // k per pass
#define F16_GEMV_LDS(NB, BF) ((NB) * F16_GEMV_KC * ((BF) ? 4 : 2))
template <int NB, bool BF, typename XROW>
__device__ __forceinline__ void f16_gemv_stream(float (&s0)[NB], float (&s1)[NB], uint8_t (&smem)[F16_GEMV_LDS(NB, BF)], const uint8_t *const w0, const uint8_t *const w1,
                                                const XROW xrow, const int K) {
    constexpr int NCH = F16_GEMV_KC / 8;                                            // chunks (of eight k) per pass
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int n = 0; n < NB; n++) s0[n] = s1[n] = 0.f;

    for (int k0 = 0; k0 < K; k0 += F16_GEMV_KC) {
        const int kc = min(F16_GEMV_KC, K - k0);
        if (k0) __syncthreads();
        // the NB activation rows of this pass, rounded once per work-group (nearest even; bf16: no subnormal flush, kept as fp32)
#pragma unroll
        for (int n = 0; n < NB; n++) {
            const float *const xr = xrow(n) + k0;
            for (int q = tid; q < kc / 4; q += 256) {
                const float4 v = *(const float4 *)(xr + 4 * q);
                if constexpr (BF) {
                    *(f32x4 *)(smem + ((n * 2 + (q & 1)) * NCH + (q >> 1)) * 16) = f32x4{(float)(__bf16)v.x, (float)(__bf16)v.y, (float)(__bf16)v.z, (float)(__bf16)v.w};
                } else {
                    half4_t h; h[0] = (half_t)v.x; h[1] = (half_t)v.y; h[2] = (half_t)v.z; h[3] = (half_t)v.w;
                    *(half4_t *)(smem + (n * F16_GEMV_KC + 4 * q) * 2) = h;
                }
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
                    // dword d holds weight 2 d in its low half (a shift) and weight 2 d + 1 in its high half (a mask)
                    float fa[8], fc[8];
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        fa[2 * d] = __builtin_bit_cast(float, wa[j][d] << 16); fa[2 * d + 1] = __builtin_bit_cast(float, wa[j][d] & 0xFFFF0000u);
                        fc[2 * d] = __builtin_bit_cast(float, wc[j][d] << 16); fc[2 * d + 1] = __builtin_bit_cast(float, wc[j][d] & 0xFFFF0000u);
                    }
#pragma unroll
                    for (int n = 0; n < NB; n++) {
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const f32x4 x = *(const f32x4 *)(smem + ((n * 2 + h) * NCH + c + 64 * j) * 16);
#pragma unroll
                            for (int e = 0; e < 4; e++) { s0[n] = fmaf(fa[4 * h + e], x[e], s0[n]); s1[n] = fmaf(fc[4 * h + e], x[e], s1[n]); }
                        }
                    }
                } else {
                    const half8_t ha = __builtin_bit_cast(half8_t, wa[j]), hc = __builtin_bit_cast(half8_t, wc[j]);
#pragma unroll
                    for (int n = 0; n < NB; n++) {
                        const half8_t x = *(const half8_t *)(smem + (n * F16_GEMV_KC + (c + 64 * j) * 8) * 2);
#pragma unroll
                        for (int e = 0; e < 8; e++) { s0[n] = fmaf((float)ha[e], (float)x[e], s0[n]); s1[n] = fmaf((float)hc[e], (float)x[e], s1[n]); }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NB; n++) { s0[n] = wave_sum_dpp(s0[n]); s1[n] = wave_sum_dpp(s1[n]); }
}
