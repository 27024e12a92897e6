// fattn.hip — GGML_OP_FLASH_ATTN_EXT for F16 K / V, semantics of ggml_compute_forward_flash_attn_ext_f16
// (src/ggml-cpu/ggml-cpu.c:10805-11016): per query row, online softmax over the keys of
//     s = scale * <fp16(q), k>  [-> softcap * tanh(s)]  + slope(head) * mask[q][kv]
// and the softmax-weighted sum of the value rows.  Head sizes 64 / 128 / 256.
//
// Everything is held in the accumulator layout of v_mfma_f32_32x32x16_f16 with the QUERY on the column (lane) axis:
//     S^T [32 kv x 32 q]  = K  [32 kv x hs]      . Q^T      A = 16-byte reads of K rows, B = fp16 Q held in registers
//     Vt  [32 kv x 32 d]  = V  [32 kv x 32 d]    . I        the matrix core as a transposer: A = 16-byte reads of V rows, B = 0/1 selection
//     O^T [32 d  x 32 q] += Vt^T[32 d x 32 kv]   . P^T      A = fp16(Vt) as it sits in the registers, B = fp16(P) as it sits in the registers
// Lane (q = lane % 32, h = lane / 32) holds accumulator rows rho(r, h) = (r & 3) + 8 (r >> 2) + 4 h, r = 0..15, of its column: the softmax
// statistics of a query row live in ONE lane pair (lane, lane ^ 32), rescaling O^T is a per-lane multiply, and the k-slots of the third
// product (8 h + j of step t <-> register 8 t + j) name the same key rho(8 t + j, h) on both operands because both came out of an
// accumulator whose rows are keys.  V is never gathered with 2-byte accesses (V x identity is exact: products with 1.0, sums with 0.0,
// fp32 -> fp16 of an fp16 value).  Precision: fp16 operands, fp32 statistics and accumulation (the CPU accumulates O in fp16 when V is
// F16: ours is the more accurate side).
//
// Two kernels share that arithmetic:
//   k_flash_attn_split  32 query rows per work-group (decode, small batches, prefill too small to fill the chip with 128-row tiles): the KEYS are split — over `nsplit` work-groups per
//                       query tile (so that a handful of heads still fills 256 CUs) and, inside a work-group, over its four waves (every
//                       fourth 32-key chunk).  K / V rows are read straight from HBM / L2 (each byte once per query tile).  The four
//                       waves' partial (max, sum, O) meet in LDS; with nsplit > 1 the work-group's partial goes to scratch and
//                       k_flash_attn_merge combines the splits in fixed order (no atomics: deterministic).
//   k_flash_attn_wide   128 query rows per work-group (prefill): every wave owns 32 query rows and ALL waves walk the same key chunks,
//                       staged once per work-group into LDS (coalesced 16-byte global loads into registers one chunk ahead, so the HBM
//                       latency hides behind the MFMAs of the current chunk), K / V traffic per query row a quarter of the split kernel's;
//                       the transposed V fragments are produced once per work-group (each wave transposes a quarter of the head
//                       dimension) and shared through LDS: 2 + hs / 16 ... MFMAs per wave and chunk instead of 3 hs / 16.
#include "../../include/ggml_cdna4.h"
#include "cdna4_common.h"
#include "cdna4_formats.hpp"
#include "cdna4_kernels.h"
#include "gemm_q_hw.h"
#include <math.h>
#include <algorithm>

void *cdna4_gemm_scratch(size_t bytes, int kind);      // gemm_q_mfma.hip: per-device scratch (kind 4 = partial results of the key split)
int cdna4_gemm_cu_count();

struct fattn_params {
    const char *q, *k, *v, *mask; float *dst;
    int64_t q_nb1, q_nb2, q_nb3, k_nb1, k_nb2, k_nb3, v_nb1, v_nb2, v_nb3, mask_nb1;       // bytes
    int n_q, n_head, n_kv, rk2, rk3, rv2, rv3;
    float scale, max_bias, logit_softcap, m0, m1; uint32_t n_head_log2;
    int mask_vec;                                  // mask rows are 16-byte aligned: whole chunks take the vector path of fa_softmax_step
    int nsplit, chunks_per_split;                  // key split over work-groups (k_flash_attn_split)
    int pack;                                      // k_flash_attn_split: query heads of one K / V head that share a 32-row tile (grouped-query decode), 1 = none
    float *part;                                   // nsplit > 1: [batch][head][q tile][split][(2 + HS) x 32] floats
};

__device__ __forceinline__ float fa_slope(const fattn_params &p, int head) {      // ggml-cpu.c:10902
    return p.max_bias > 0.0f ? ((uint32_t)head < p.n_head_log2 ? powf(p.m0, (float)(head + 1)) : powf(p.m1, (float)(2 * (head - (int)p.n_head_log2) + 1))) : 1.0f;
}
// this lane's query row as fp16 B fragments: Q[qi][16 s + 8 h + e]  (q_to_vec_dot = fp32 -> fp16 row, ggml-cpu.c:10929)
template <int NS> __device__ __forceinline__ void fa_load_q(const fattn_params &p, int qi, int head, int b3, int h, half8_t (&qf)[NS]) {
    const float *qrow = (const float *)(p.q + (int64_t)qi * p.q_nb1 + (int64_t)head * p.q_nb2 + (int64_t)b3 * p.q_nb3);
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int e = 0; e < 8; e++) qf[s][e] = (half_t)qrow[16 * s + 8 * h + e];
}
// selection operands of the transposing product: B[k-slot 8 h + j][column n] = (n == 16 u + 8 h + j)
__device__ __forceinline__ void fa_selectors(int n, int h, half8_t (&sel)[2]) {
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int j = 0; j < 8; j++) sel[u][j] = (n == 16 * u + 8 * h + j) ? (half_t)1.0f : (half_t)0.0f;
}
// one chunk's scores (accumulator layout) -> scale, softcap, mask; online-softmax update of (M, S); P as fp16 B fragments; returns the
// factor the O accumulator must be multiplied with.
// Everything behind the softcap lives in the LOG2 domain (scores, mask term and the running maximum M carry a factor log2(e)):
// e^(x - M) = 2^(x2 - M2) is then one v_exp_f32 per score instead of expf's range reduction, and scale * log2(e) is one constant.
// Accumulator register r = 4 g + j of lane (q, h) is key kv0 + 8 g + 4 h + j: the four mask values a register group needs are 8 contiguous
// bytes of this lane's mask row — read as such (whole chunks of a 16-byte aligned mask; fp16 -inf converts to -inf, no clamping), the conversion
// folded into the multiply-add.  Ragged chunks, unaligned masks and the softcap take the element-wise path.
__device__ __forceinline__ float fa_softmax_step(const fattn_params &p, floatx16 &s, int kv0, int h, const half_t *mrow, float slope2,
                                                 float &M, float &S, half8_t (&pf)[2]) {
    constexpr float LOG2E = 1.4426950408889634f;
    const bool whole = kv0 + 32 <= p.n_kv;                                      // wave-uniform
    if (whole && p.logit_softcap == 0.0f && (!mrow || p.mask_vec)) {
        const float c2 = p.scale * LOG2E;
        if (mrow) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const half4_t mv = *reinterpret_cast<const half4_t *>(mrow + kv0 + 8 * g + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; j++) s[4 * g + j] = __builtin_fmaf((float)mv[j], slope2, s[4 * g + j] * c2);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] *= c2;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int kv = kv0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float x = s[r] * p.scale;
            if (p.logit_softcap != 0.0f) x = p.logit_softcap * tanhf(x);
            x *= LOG2E;
            if (kv < p.n_kv) { if (mrow) x += slope2 * (float)mrow[kv]; } else x = -INFINITY;
            s[r] = x;
        }
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; r++) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float Mn = fmaxf(M, mx);
    // everything masked so far (Mn = -inf): subtract 0 instead — every 2^(-inf) below is 0 and (M, S, O) stay (-inf, 0, 0), as the CPU's
    // skipping of -inf entries leaves them (ggml-cpu.c:10935-10938); no (-inf) - (-inf) anywhere
    const float Ms = (Mn == -INFINITY) ? 0.0f : Mn;
    const float ms = __builtin_amdgcn_exp2f(M - Ms);
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float e = __builtin_amdgcn_exp2f(s[r] - Ms);
        sum += e; pf[r >> 3][r & 7] = (half_t)e;
    }
    sum += __shfl_xor(sum, 32);
    S = S * ms + sum; M = Mn;
    return ms;
}
// V /= S and the store: dst is [hs, n_head, n_q, batch] (the permute(0, 2, 1, 3) of ggml-cpu.c:11012); lane (q, h) holds d = 32 b + 8 g + 4 h + 0..3
template <int NB> __device__ __forceinline__ void fa_store(float *out, const floatx16 (&o)[NB], float inv, int h) {
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int g = 0; g < 4; g++)
            *reinterpret_cast<float4 *>(out + 32 * b + 8 * g + 4 * h) = make_float4(o[b][4 * g] * inv, o[b][4 * g + 1] * inv, o[b][4 * g + 2] * inv, o[b][4 * g + 3] * inv);
}

// Eight consecutive elements e0 .. e0 + 7 (e0 a multiple of 8) of a K / V row as an fp16 MFMA fragment.  F16 rows: 16 bytes as they lie.  Q8_0 / Q4_0
// rows — a quantized KV cache read by the decode kernel WITHOUT the fp16 copy the prefill path makes (VERDICT r2 "missing 5": one pass over 34 / 18
// bytes per 32 elements instead of a read of that, a write and a read of 64): fp16(to_float(element)), the rounding an F16 cache holding the
// dequantized values has (dequantize_row_q8_0 / _q4_0, src/ggml-quants.c:255-273, 367-377) — bit-identical to the converting path.  The eight quants sit 2 bytes
// behind their block's d: two aligned dwords, or three and a 16-bit funnel shift (rows are 4-byte aligned: 34 n / 18 n bytes with n even).
// Load and conversion are separate steps (fa_kv_load / fa_kv_cvt): the decode kernel requests a chunk's fragments one chunk ahead and keeps the RAW 16 bytes in the registers
// meanwhile — a conversion right behind the load would wait for it.  Raw form of a quantized fragment: x, y = its 8 quant bytes, w = the block's d in the low half,
// bit 17 = Q4_0's high nibbles.
template <int KVT> __device__ __forceinline__ u32x4 fa_kv_load(const char *row, int e0) {
    if constexpr (KVT == CDNA4_F16 || KVT == CDNA4_BF16) return *reinterpret_cast<const u32x4 *>(row + 2 * e0);
    else {
        constexpr int BB = KVT == CDNA4_Q8_0 ? 34 : 18;
        const char *blk = row + (e0 >> 5) * BB, *q = blk + 2 + (KVT == CDNA4_Q8_0 ? (e0 & 31) : (e0 & 15));      // Q4_0: element i < 16: low nibble of byte i, i >= 16: high nibble of byte i - 16
        u32x4 r;
        r.w = (uint32_t)*reinterpret_cast<const uint16_t *>(blk) | ((KVT == CDNA4_Q4_0 && (e0 & 16)) ? 0x20000u : 0u);
        // ONE 8-byte load at 2-byte alignment (global memory takes unaligned dword accesses on this target: hipcc emits global_load_dwordx2 for it) — the first form read two
        // or three aligned dwords behind a per-lane alignment branch and funnel-shifted them
        struct __attribute__((packed, aligned(2))) u64_a2 { uint64_t v; };
        const uint64_t b8 = reinterpret_cast<const u64_a2 *>(q)->v;
        r.x = (uint32_t)b8; r.y = (uint32_t)(b8 >> 32); r.z = 0;
        return r;
    }
}
template <int KVT> __device__ __forceinline__ half8_t fa_kv_cvt(u32x4 raw) {
    if constexpr (KVT == CDNA4_F16) return __builtin_bit_cast(half8_t, raw);
    else if constexpr (KVT == CDNA4_BF16) {                                 // bf16 -> fp32 (the 16 bits are the upper half) -> fp16: what k_q_to_f16_dense<BF16> writes
        const uint32_t ww[4] = {raw.x, raw.y, raw.z, raw.w};
        half8_t out;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float v = __builtin_bit_cast(float, (ww[j >> 1] >> (16 * (j & 1))) << 16);
            out[j] = (half_t)opaque_f32(v != v ? v : fminf(fmaxf(v, -65504.f), 65504.f));   // saturate at fp16's range (k_q_to_f16_dense<BF16> does the same)
        }
        return out;
    } else {
        // Round 6: the conversion in packed fp16 arithmetic.  A byte b in 0..255 under the exponent byte 0x64 is the fp16 number 1024 + b, EXACTLY; subtracting 1152 (Q8_0: b =
        // q + 128) or 1032 (Q4_0: b = the nibble) leaves the integer quant, exactly; times d (an fp16 number) is one exact product rounded once to fp16 — the value
        // fp16(fp32(d) * q) of the element-wise form it replaces (the fp32 product of an 11-bit and an 8-bit significand is exact), bit for bit, subnormals included.
        // 14 - 16 VALU per fragment instead of ~40.
        u32x2 w = {raw.x, raw.y};
        const half_t d = __builtin_bit_cast(half_t, (uint16_t)(raw.w & 0xFFFFu));
        const half2_t d2 = {d, d};
        half_t bias;
        if constexpr (KVT == CDNA4_Q8_0) { w.x ^= 0x80808080u; w.y ^= 0x80808080u; bias = (half_t)1152.0f; }
        else { const int sh = (raw.w & 0x20000u) ? 4 : 0; w.x = (w.x >> sh) & 0x0F0F0F0Fu; w.y = (w.y >> sh) & 0x0F0F0F0Fu; bias = (half_t)1032.0f; }
        const half2_t b2 = {bias, bias};
        half8_t out;
#pragma unroll
        for (int pr = 0; pr < 4; pr++) {                                // bytes 2 pr, 2 pr + 1 -> the two halves 0x64bb of one dword
            const uint32_t ww = pr < 2 ? w.x : w.y;
#if defined(__HIPCC__)
            const uint32_t hx = __builtin_amdgcn_perm(0x64646464u, ww, (pr & 1) ? 0x04030402u : 0x04010400u);
#else
            const uint32_t b01 = ww >> (16 * (pr & 1)), hx = (b01 & 0xFFu) | ((b01 & 0xFF00u) << 8) | 0x64006400u;
#endif
            const half2_t v = (__builtin_bit_cast(half2_t, hx) - b2) * d2;
            out[2 * pr] = v[0]; out[2 * pr + 1] = v[1];
        }
        return out;
    }
}

// ------------------------------------------------------------------------------------------------ key-split kernel (decode, <= 32 query rows per tile)
template <int HS, int KVT = CDNA4_F16>
__global__ __launch_bounds__(256, HS <= 128 ? 2 : 1) void k_flash_attn_split(const fattn_params p) {
    constexpr int NS = HS / 16, NB = HS / 32;                     // k-steps of Q.K, 32-wide blocks of the head dimension
    __shared__ float Os[HS * 32];                                 // one wave's O^T at a time: [d][q]
    __shared__ float Ms[32], Ss[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int qt = blockIdx.x / p.nsplit, split = blockIdx.x % p.nsplit;
    const int q0 = qt * 32, b3 = blockIdx.z;
    // Grouped-query decode (p.pack = n_head / n_head_kv > 1, n_q * pack <= 32): the tile's rows are (query row, head of the group) pairs, row n = query n / pack of head
    // blockIdx.y * pack + n % pack — the group's K / V rows are read ONCE for all of its heads (each head by itself read them again: pack times the cache traffic, and one
    // useful column of the 32 x 32 MFMA tile per head).  Otherwise row n is query q0 + n of head blockIdx.y.
    const int head = p.pack > 1 ? (int)blockIdx.y * p.pack + n % p.pack : (int)blockIdx.y;
    const int qrow = p.pack > 1 ? n / p.pack : q0 + n;
    const int qi = min(qrow, p.n_q - 1);                          // rows past the end repeat the last one and are not stored

    half8_t qf[NS], sel[2];
    fa_load_q<NS>(p, qi, head, b3, h, qf);
    fa_selectors(n, h, sel);
    const float slope2 = fa_slope(p, head) * 1.4426950408889634f;                 // log2 domain (fa_softmax_step)
    const char *kbase = p.k + (int64_t)(head / p.rk2) * p.k_nb2 + (int64_t)(b3 / p.rk3) * p.k_nb3;
    const char *vbase = p.v + (int64_t)(head / p.rv2) * p.v_nb2 + (int64_t)(b3 / p.rv3) * p.v_nb3;
    const half_t *mrow = p.mask ? (const half_t *)(p.mask + (int64_t)qi * p.mask_nb1) : nullptr;

    float M = -INFINITY, S = 0.0f;
    floatx16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;

    const int nchunk = (p.n_kv + 31) / 32;
    const int c_lo = split * p.chunks_per_split, c_hi = min(nchunk, c_lo + p.chunks_per_split);
    // The fragments of a chunk are requested ONE CHUNK AHEAD, into the registers the previous chunk's fragments have just left: K right behind the score products, V behind the
    // last P.V product — a chunk's loads have the rest of the step (K) or the next step's scores and softmax (V) to arrive, at no extra registers.  (First the loop issued each
    // fragment in front of its product: two exposed memory round trips per chunk; the F16 / Q8_0 / Q4_0 caches took 120 / 127 / 92 us at 32 K keys, within 30 % of each other in
    // TIME — bound by the dependent load -> use chain, not by bytes.)
    u32x4 kc[NS], vc[2 * NB];                                     // raw (fa_kv_load): converted where they are used
    auto load_k = [&](int c) __attribute__((always_inline)) {
        const char *kp = kbase + (int64_t)min(32 * c + n, p.n_kv - 1) * p.k_nb1;          // A row n of this lane = key 32 c + n (past the end: repeated, masked in the softmax)
#pragma unroll
        for (int st = 0; st < NS; st++) kc[st] = fa_kv_load<KVT>(kp, 16 * st + 8 * h);
    };
    auto load_v = [&](int c) __attribute__((always_inline)) {
        const char *vp = vbase + (int64_t)min(32 * c + n, p.n_kv - 1) * p.v_nb1;
#pragma unroll
        for (int u = 0; u < 2 * NB; u++) vc[u] = fa_kv_load<KVT>(vp, 16 * u + 8 * h);
    };
    if (c_lo + wave < c_hi) { load_k(c_lo + wave); load_v(c_lo + wave); }
    for (int c = c_lo + wave; c < c_hi; c += 4) {
        const int kv0 = 32 * c;
        floatx16 s;
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] = 0.0f;
#pragma unroll
        for (int st = 0; st < NS; st++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa_kv_cvt<KVT>(kc[st]), qf[st], s, 0, 0, 0);
        if (c + 4 < c_hi) load_k(c + 4);
        half8_t pf[2];
        const float ms = fa_softmax_step(p, s, kv0, h, mrow, slope2, M, S, pf);
        // O^T *= ms, skipped while no row of the wave moved its maximum (x 1.0 is exact).  ONE branch in front of the block loop: with the test
        // inside the loop hipcc (ROCm 7.2) branched on a stale SGPR pair for blocks 1..3 — wrong results on MI355X, invisible to the CPU emulation
        if (wave_any(ms != 1.0f)) {
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[b][r] *= ms;
        }
        // O^T = O^T * ms + Vt^T . P^T, one 32-wide block of the head dimension at a time
#pragma unroll
        for (int b = 0; b < NB; b++) {
            floatx16 vt;
#pragma unroll
            for (int r = 0; r < 16; r++) vt[r] = 0.0f;
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa_kv_cvt<KVT>(vc[2 * b]), sel[0], vt, 0, 0, 0);
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa_kv_cvt<KVT>(vc[2 * b + 1]), sel[1], vt, 0, 0, 0);
            half8_t vf[2];
#pragma unroll
            for (int r = 0; r < 16; r++) vf[r >> 3][r & 7] = (half_t)vt[r];
            o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0], pf[0], o[b], 0, 0, 0);
            o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1], pf[1], o[b], 0, 0, 0);
        }
        if (c + 4 < c_hi) load_v(c + 4);
    }

    // the four partial results meet: waves 1..3 hand theirs to wave 0 one after the other through LDS (same lane <-> element mapping on
    // both sides: Os[d][q], q = lane % 32 — conflict-free)
    for (int w = 1; w < 4; w++) {
        __syncthreads();
        if (wave == w) {
            if (h == 0) { Ms[n] = M; Ss[n] = S; }
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) Os[(32 * b + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + n] = o[b][r];
        }
        __syncthreads();
        if (wave == 0) {
            const float Mw = Ms[n], Sw = Ss[n], Mn = fmaxf(M, Mw);
            const float a0 = (M == -INFINITY) ? 0.0f : exp2f(M - Mn), aw = (Mw == -INFINITY) ? 0.0f : exp2f(Mw - Mn);      // (M in the log2 domain)
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[b][r] = o[b][r] * a0 + Os[(32 * b + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + n] * aw;
            S = S * a0 + Sw * aw; M = Mn;
        }
    }
    if (wave != 0 || qrow >= p.n_q) return;
    if (p.nsplit == 1) {
        fa_store<NB>(p.dst + (((int64_t)b3 * p.n_q + qrow) * p.n_head + head) * HS, o, 1.0f / S, h);
    } else {
        // this split's unnormalized (M, S, O) for k_flash_attn_merge: [.. head][tile][split][q][2 + HS] — the rows that exist, contiguous (grouped: one tile per head, row = query)
        float *pt = p.part + ((((int64_t)b3 * p.n_head + head) * gridDim.x + blockIdx.x) * 32 + (p.pack > 1 ? qrow : n)) * (HS + 4);
        if (h == 0) { pt[0] = M; pt[1] = S; }
        fa_store<NB>(pt + 4, o, 1.0f, h);
    }
}

// out[q][d] = sum_s O_s[q][d] e^(M_s - M*) / sum_s S_s e^(M_s - M*), splits in index order.  One work-group per (query tile, head, batch).
template <int HS>
__global__ __launch_bounds__(256) void k_flash_attn_merge(const fattn_params p) {
    const int qt = blockIdx.x, head = blockIdx.y, b3 = blockIdx.z;
    const float *base = p.part + (((int64_t)b3 * p.n_head + head) * (gridDim.x * p.nsplit) + (int64_t)qt * p.nsplit) * 32 * (HS + 4);
    for (int i = threadIdx.x; i < 32 * HS; i += 256) {
        const int q = i / HS, d = i % HS;
        if (qt * 32 + q >= p.n_q) break;
        float Mx = -INFINITY;
        for (int s = 0; s < p.nsplit; s++) Mx = fmaxf(Mx, base[((int64_t)s * 32 + q) * (HS + 4)]);
        float num = 0.0f, den = 0.0f;
        for (int s = 0; s < p.nsplit; s++) {
            const float *pt = base + ((int64_t)s * 32 + q) * (HS + 4);
            const float a = (pt[0] == -INFINITY) ? 0.0f : exp2f(pt[0] - Mx);      // (M in the log2 domain)
            num += pt[4 + d] * a; den += pt[1] * a;
        }
        p.dst[(((int64_t)b3 * p.n_q + (qt * 32 + q)) * p.n_head + head) * HS + d] = num * (1.0f / den);
    }
}

// The same for a handful of query rows (decode), one work-group per (query row, head, batch): k_flash_attn_merge gives a row's HS outputs to HS threads, each of which walks the
// splits twice with a dependent wait per load — 7 - 20 us of a 66 - 97 us decode call over 16 - 64 splits (rocprofv3, round 6).  Here the splits' (M, S) are fetched side by side
// into LDS, every thread derives the factors from there, and the 256 threads split the sum over the splits 256 / HS ways with four loads in flight each; the parts meet in LDS in
// part order, the splits inside a part in index order (deterministic).
template <int HS>
__global__ __launch_bounds__(256) void k_flash_attn_merge_rows(const fattn_params p) {
    constexpr int NP = 256 / HS;                                   // parts of the split range (HS 64: 4, 128: 2, 256: 1)
    __shared__ float sA[512], sS[512], sN[NP][HS];
    const int q = blockIdx.x, head = blockIdx.y, b3 = blockIdx.z, tid = threadIdx.x, d = tid % HS, part = tid / HS;
    const int qt = q >> 5, qr = q & 31, qtiles = (p.n_q + 31) >> 5;
    const float *base = p.part + ((((int64_t)b3 * p.n_head + head) * (qtiles * p.nsplit) + (int64_t)qt * p.nsplit) * 32 + qr) * (HS + 4);      // split s: + s * 32 * (HS + 4)
    const int64_t sstride = 32 * (HS + 4);
    for (int s = tid; s < p.nsplit; s += 256) { sA[s] = base[s * sstride]; sS[s] = base[s * sstride + 1]; }
    __syncthreads();
    float Mx = -INFINITY;
    for (int s = 0; s < p.nsplit; s++) Mx = fmaxf(Mx, sA[s]);
    float den = 0.0f;
    for (int s = 0; s < p.nsplit; s++) { const float a = (sA[s] == -INFINITY) ? 0.0f : exp2f(sA[s] - Mx); den += sS[s] * a; }      // (M in the log2 domain; every thread the same order)
    __syncthreads();
    for (int s = tid; s < p.nsplit; s += 256) sA[s] = (sA[s] == -INFINITY) ? 0.0f : exp2f(sA[s] - Mx);
    __syncthreads();
    const int per = (p.nsplit + NP - 1) / NP, s0 = part * per, s1 = min(p.nsplit, s0 + per);
    float num = 0.0f;
    int s = s0;
    for (; s + 4 <= s1; s += 4) {
        const float o0 = base[(s + 0) * sstride + 4 + d], o1 = base[(s + 1) * sstride + 4 + d], o2 = base[(s + 2) * sstride + 4 + d], o3 = base[(s + 3) * sstride + 4 + d];
        num += o0 * sA[s]; num += o1 * sA[s + 1]; num += o2 * sA[s + 2]; num += o3 * sA[s + 3];
    }
    for (; s < s1; s++) num += base[s * sstride + 4 + d] * sA[s];
    sN[part][d] = num;
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int pp = 1; pp < NP; pp++) num += sN[pp][d];
    p.dst[(((int64_t)b3 * p.n_q + q) * p.n_head + head) * HS + d] = num * (1.0f / den);
}

// ------------------------------------------------------------------------------------------------ wide kernel (prefill, 128 query rows per work-group)
template <int HS>
__global__ __launch_bounds__(256, HS <= 128 ? 2 : 1) void k_flash_attn_wide(const fattn_params p) {
    constexpr int NS = HS / 16, NB = HS / 32;
    constexpr int RS = (HS + 8) * 2;                              // bytes of a staged K / V row: 16 bytes of padding spread the rows over the banks
    constexpr int PIECES = 32 * HS / 8, PL = PIECES / 256;        // 16-byte pieces of one 32-row chunk, per thread
    __shared__ __attribute__((aligned(16))) uint8_t Ks[32 * RS], Vs[32 * RS];
    __shared__ __attribute__((aligned(16))) uint8_t Vt[NB * 2 * 64 * 16];     // transposed V as A fragments: [block][step][lane] x 16 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 128 + 32 * wave, head = blockIdx.y, b3 = blockIdx.z;
    const bool active = q0 < p.n_q;                               // a wave whose 32 rows are all past the end only helps with the staging
    const int qi = min(q0 + n, p.n_q - 1);

    half8_t qf[NS], sel[2];
    fa_load_q<NS>(p, qi, head, b3, h, qf);
    fa_selectors(n, h, sel);
    const float slope2 = fa_slope(p, head) * 1.4426950408889634f;                 // log2 domain (fa_softmax_step)
    const char *kbase = p.k + (int64_t)(head / p.rk2) * p.k_nb2 + (int64_t)(b3 / p.rk3) * p.k_nb3;
    const char *vbase = p.v + (int64_t)(head / p.rv2) * p.v_nb2 + (int64_t)(b3 / p.rv3) * p.v_nb3;
    const half_t *mrow = p.mask ? (const half_t *)(p.mask + (int64_t)qi * p.mask_nb1) : nullptr;

    float M = -INFINITY, S = 0.0f;
    floatx16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;

    // staging: piece pc = tid + 256 i of a chunk = (row pc / (HS / 8), 16-byte column pc % (HS / 8)): a wave reads whole rows, coalesced
    u32x4 kreg[PL], vreg[PL];
    auto fetch = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PL; i++) {
            const int pc = tid + 256 * i, row = pc / (HS / 8), col = pc % (HS / 8);
            const int64_t kr = min(32 * c + row, p.n_kv - 1);     // past the end: repeated, masked in the softmax
            kreg[i] = *reinterpret_cast<const u32x4 *>(kbase + kr * p.k_nb1 + 16 * col);
            vreg[i] = *reinterpret_cast<const u32x4 *>(vbase + kr * p.v_nb1 + 16 * col);
        }
    };
    const int nchunk = (p.n_kv + 31) / 32;
    fetch(0);
    for (int c = 0; c < nchunk; c++) {
        __syncthreads();                                          // every wave is done with the previous chunk's Ks / Vs / Vt
#pragma unroll
        for (int i = 0; i < PL; i++) {
            const int pc = tid + 256 * i, row = pc / (HS / 8), col = pc % (HS / 8);
            *reinterpret_cast<u32x4 *>(Ks + row * RS + 16 * col) = kreg[i];
            *reinterpret_cast<u32x4 *>(Vs + row * RS + 16 * col) = vreg[i];
        }
        __syncthreads();
        if (c + 1 < nchunk) fetch(c + 1);                         // in flight while this chunk is computed
        // this wave's share of the transposed V fragments (blocks wave, wave + 4, ..)
        for (int b = wave; b < NB; b += 4) {
            floatx16 vt;
#pragma unroll
            for (int r = 0; r < 16; r++) vt[r] = 0.0f;
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vs + n * RS + 64 * b + 16 * h), sel[0], vt, 0, 0, 0);
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vs + n * RS + 64 * b + 32 + 16 * h), sel[1], vt, 0, 0, 0);
            half8_t vf[2];
#pragma unroll
            for (int r = 0; r < 16; r++) vf[r >> 3][r & 7] = (half_t)vt[r];
            *reinterpret_cast<half8_t *>(Vt + ((b * 2 + 0) * 64 + lane) * 16) = vf[0];
            *reinterpret_cast<half8_t *>(Vt + ((b * 2 + 1) * 64 + lane) * 16) = vf[1];
        }
        half8_t pf[2];
        float ms = 1.0f;
        if (active) {
            floatx16 s;
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = 0.0f;
#pragma unroll
            for (int st = 0; st < NS; st++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Ks + n * RS + 32 * st + 16 * h), qf[st], s, 0, 0, 0);
            ms = fa_softmax_step(p, s, 32 * c, h, mrow, slope2, M, S, pf);
        }
        __syncthreads();                                          // Vt is complete
        if (active) {
            if (wave_any(ms != 1.0f)) {                                 // after the first chunks the running maximum rarely moves: x 1.0 skipped (exact; one branch, see above)
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++) o[b][r] *= ms;
            }
#pragma unroll
            for (int b = 0; b < NB; b++) {
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vt + ((b * 2 + 0) * 64 + lane) * 16), pf[0], o[b], 0, 0, 0);
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vt + ((b * 2 + 1) * 64 + lane) * 16), pf[1], o[b], 0, 0, 0);
            }
        }
    }
    if (q0 + n < p.n_q) fa_store<NB>(p.dst + (((int64_t)b3 * p.n_q + (q0 + n)) * p.n_head + head) * HS, o, 1.0f / S, h);
}

// ------------------------------------------------------------------------------------------------ wide kernel, 64-key chunks (head sizes 64 / 128)
// The same arithmetic as k_flash_attn_wide over TWO 32-key blocks per step: one online-softmax update (one maximum, one rescaling of O) and TWO
// barriers per 64 keys instead of three per 32 —
//   top of chunk c : the registers fetched during chunk c - 1 go to Ks / Vs (free: every wave has passed B2 of chunk c - 1, i.e. finished its
//                    score products and its share of the V transposition; only Vt may still be read, by the P.V products of chunk c - 1)
//   B1             : Ks / Vs of chunk c are visible, every wave is done with Vt of chunk c - 1
//                    K / V of chunk c + 1 are requested; this wave's (key block, head block) units are transposed into Vt; scores, softmax;
//                    the mask groups of chunk c + 1 are requested (their registers are free now)
//   B2             : Vt is complete                       P.V products
// The mask values of a whole chunk arrive a chunk ahead in registers (8 x 8 bytes per lane) like K / V do, so the softmax never waits for L2.
template <int NKB>
__device__ __forceinline__ float fa_softmax_blocks(const fattn_params &p, floatx16 (&s)[NKB], int kv0, int h, const half_t *mrow, float slope2, const half4_t (&mreg)[NKB * 4],
                                                   float &M, float &S, half8_t (&pf)[NKB * 2]) {
    constexpr float LOG2E = 1.4426950408889634f;
    const bool whole = kv0 + 32 * NKB <= p.n_kv;                                // wave-uniform
    if (whole && p.logit_softcap == 0.0f && (!mrow || p.mask_vec)) {           // (with a mask: exactly the condition under which the caller filled mreg)
        const float c2 = p.scale * LOG2E;
#pragma unroll
        for (int kb = 0; kb < NKB; kb++) {
            if (mrow) {
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int j = 0; j < 4; j++) s[kb][4 * g + j] = __builtin_fmaf((float)mreg[kb * 4 + g][j], slope2, s[kb][4 * g + j] * c2);
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) s[kb][r] *= c2;
            }
        }
    } else {
#pragma unroll
        for (int kb = 0; kb < NKB; kb++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int kv = kv0 + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * h;
                float x = s[kb][r] * p.scale;
                if (p.logit_softcap != 0.0f) x = p.logit_softcap * tanhf(x);
                x *= LOG2E;
                if (kv < p.n_kv) { if (mrow) x += slope2 * (float)mrow[kv]; } else x = -INFINITY;
                s[kb][r] = x;
            }
    }
    float mx = s[0][0];
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float Mn = fmaxf(M, mx);
    const float Ms = (Mn == -INFINITY) ? 0.0f : Mn;                             // (see fa_softmax_step)
    const float ms = __builtin_amdgcn_exp2f(M - Ms);
    float sum = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float e = __builtin_amdgcn_exp2f(s[kb][r] - Ms);
            sum += e; pf[kb * 2 + (r >> 3)][r & 7] = (half_t)e;
        }
    sum += __shfl_xor(sum, 32);
    S = S * ms + sum; M = Mn;
    return ms;
}

template <int HS>
__global__ __launch_bounds__(256, 2) void k_flash_attn_wide64(const fattn_params p) {
    constexpr int NS = HS / 16, NB = HS / 32, NKB = 2, CK = 32 * NKB;
    constexpr int RS = (HS + 8) * 2;                              // bytes of a staged K / V row (16 bytes of padding spread the rows over the banks)
    constexpr int PL = CK * HS / 8 / 256;                         // 16-byte pieces of one chunk per thread and matrix
    __shared__ __attribute__((aligned(16))) uint8_t Ks[CK * RS], Vs[CK * RS];
    __shared__ __attribute__((aligned(16))) uint8_t Vt[NB * NKB * 2 * 64 * 16];   // transposed V as A fragments: [head block][key block][k-step][lane] x 16 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 128 + 32 * wave, head = blockIdx.y, b3 = blockIdx.z;
    const bool active = q0 < p.n_q;                               // a wave whose 32 rows are all past the end only helps with the staging
    const int qi = min(q0 + n, p.n_q - 1);

    half8_t qf[NS], sel[2];
    fa_load_q<NS>(p, qi, head, b3, h, qf);
    fa_selectors(n, h, sel);
    const float slope2 = fa_slope(p, head) * 1.4426950408889634f;
    const char *kbase = p.k + (int64_t)(head / p.rk2) * p.k_nb2 + (int64_t)(b3 / p.rk3) * p.k_nb3;
    const char *vbase = p.v + (int64_t)(head / p.rv2) * p.v_nb2 + (int64_t)(b3 / p.rv3) * p.v_nb3;
    const half_t *mrow = p.mask ? (const half_t *)(p.mask + (int64_t)qi * p.mask_nb1) : nullptr;

    float M = -INFINITY, S = 0.0f;
    floatx16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;

    u32x4 kreg[PL], vreg[PL];
    half4_t mreg[NKB * 4] = {};
    auto fetch_kv = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PL; i++) {
            const int pc = tid + 256 * i, row = pc / (HS / 8), col = pc % (HS / 8);
            const int64_t kr = min(CK * c + row, p.n_kv - 1);     // past the end: repeated, masked in the softmax
            kreg[i] = *reinterpret_cast<const u32x4 *>(kbase + kr * p.k_nb1 + 16 * col);
            vreg[i] = *reinterpret_cast<const u32x4 *>(vbase + kr * p.v_nb1 + 16 * col);
        }
    };
    auto fetch_mask = [&](int c) __attribute__((always_inline)) {
        if (active && mrow && p.mask_vec && CK * c + CK <= p.n_kv) {   // (wave-uniform)
#pragma unroll
            for (int kb = 0; kb < NKB; kb++)
#pragma unroll
                for (int g = 0; g < 4; g++) mreg[kb * 4 + g] = *reinterpret_cast<const half4_t *>(mrow + CK * c + 32 * kb + 8 * g + 4 * h);
        }
    };
    const int nchunk = (p.n_kv + CK - 1) / CK;
    fetch_kv(0); fetch_mask(0);
    for (int c = 0; c < nchunk; c++) {
#pragma unroll
        for (int i = 0; i < PL; i++) {
            const int pc = tid + 256 * i, row = pc / (HS / 8), col = pc % (HS / 8);
            *reinterpret_cast<u32x4 *>(Ks + row * RS + 16 * col) = kreg[i];
            *reinterpret_cast<u32x4 *>(Vs + row * RS + 16 * col) = vreg[i];
        }
        __syncthreads();                                          // B1
        if (c + 1 < nchunk) fetch_kv(c + 1);                      // in flight while this chunk is computed
        for (int u = wave; u < NKB * NB; u += 4) {               // this wave's share of the transposed V fragments
            const int kb = u / NB, b = u % NB;
            floatx16 vt;
#pragma unroll
            for (int r = 0; r < 16; r++) vt[r] = 0.0f;
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vs + (32 * kb + n) * RS + 64 * b + 16 * h), sel[0], vt, 0, 0, 0);
            vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vs + (32 * kb + n) * RS + 64 * b + 32 + 16 * h), sel[1], vt, 0, 0, 0);
            half8_t vf[2];
#pragma unroll
            for (int r = 0; r < 16; r++) vf[r >> 3][r & 7] = (half_t)vt[r];
            *reinterpret_cast<half8_t *>(Vt + (((b * NKB + kb) * 2 + 0) * 64 + lane) * 16) = vf[0];
            *reinterpret_cast<half8_t *>(Vt + (((b * NKB + kb) * 2 + 1) * 64 + lane) * 16) = vf[1];
        }
        half8_t pf[NKB * 2];
        float ms = 1.0f;
        if (active) {
            floatx16 s[NKB];
#pragma unroll
            for (int kb = 0; kb < NKB; kb++) {
#pragma unroll
                for (int r = 0; r < 16; r++) s[kb][r] = 0.0f;
#pragma unroll
                for (int st = 0; st < NS; st++) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Ks + (32 * kb + n) * RS + 32 * st + 16 * h), qf[st], s[kb], 0, 0, 0);
            }
            ms = fa_softmax_blocks<NKB>(p, s, CK * c, h, mrow, slope2, mreg, M, S, pf);
        }
        if (c + 1 < nchunk) fetch_mask(c + 1);
        __syncthreads();                                          // B2
        if (active) {
            if (wave_any(ms != 1.0f)) {                             // (one branch in front of the block loop: see k_flash_attn_split)
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++) o[b][r] *= ms;
            }
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int kt = 0; kt < NKB * 2; kt++)
                    o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Vt + ((b * NKB * 2 + kt) * 64 + lane) * 16), pf[kt], o[b], 0, 0, 0);
        }
    }
    if (q0 + n < p.n_q) fa_store<NB>(p.dst + (((int64_t)b3 * p.n_q + (q0 + n)) * p.n_head + head) * HS, o, 1.0f / S, h);
}

// ------------------------------------------------------------------------------------------------ pipelined kernel (prefill, head sizes 64 / 128)
// NW waves x 32 query rows per work-group over 64-key chunks, the same accumulator-layout arithmetic as above, restructured around what the counters of the wide
// kernel said (round 6): it spent its LDS cycles on bank conflicts of the padded K rows, eight extra MFMAs per chunk on the V x identity transposition with an LDS
// round trip and a second barrier behind it, and its staging writes sat between the barriers.  Here
//   * K / V chunks are DOUBLE-buffered in LDS, fetched into registers right behind the barrier that ends a chunk (two chunks ahead of their use) and written to the
//     other buffer in the middle of the next chunk (between the softmax and the P.V products), when the loads have long landed: ONE barrier per chunk
//   * K rows are stored with their 16-byte slots XOR-swizzled by the row, so the four 16-lane groups of a ds_read_b128 fragment read (32 rows, one slot column) hit
//     16 distinct slots of the 256-byte bank row
//   * V is stored row-major (64-byte segments XOR-swizzled by the row) and read with gfx950's LDS transpose read, ds_read_b64_tr_b16: a 16-lane group hands in the
//     addresses of a [4 keys][16 d] block, 8 bytes per lane, and lane i receives column i — four keys of ITS head-dimension row, which is half an A fragment of the
//     third product (keys 16 kt + 4 h + 0..3 and 16 kt + 8 + 4 h + 0..3: the k-slot order P's accumulator registers already have).  No transposing MFMA, no Vt buffer.
//     (semantics pinned on the hardware by tools/microbench/tr16_probe.hip)
//   * the grid is one-dimensional and XCD-aware: work item (batch, head, query tile) w runs on XCD w / (items / 8), so the query tiles of a head share one L2
#if defined(__HIPCC__)
typedef __fp16 fa_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ half4_t fa_lds_tr16(const uint8_t *p) {
    return __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fa_fp16x4 *)(p)));
}
#else       // tools/emul: wave-collective — every lane posts its address; lane i of a 16-lane group takes element i % 4 of the lane 4 j + i / 4 for j = 0..3
static inline half4_t fa_lds_tr16(const uint8_t *p) {
    emu::WaveState &w = emu::my_wave();
    const int l = (int)(emu::t_threadIdx.x & 63), i = l & 15, g = l >> 4;
    memcpy(&w.A[l][0], &p, sizeof p);
    pthread_barrier_wait(&w.bar);
    half4_t r;
    for (int j = 0; j < 4; j++) { const uint8_t *a; memcpy(&a, &w.A[16 * g + 4 * j + (i >> 2)][0], sizeof a); r[j] = *reinterpret_cast<const half_t *>(a + 2 * (i & 3)); }
    pthread_barrier_wait(&w.bar);
    return r;
}
#endif

// value of the partner lane (lane ^ 32) combined with this lane's by a symmetric operation: v_permlane32_swap hands every lane BOTH halves' values
#if defined(__HIPCC__)
// (both results are pinned by an empty asm: hipcc 7.2 otherwise folds arithmetic on the PAIR of results as if they were one value — max(r0, r1) became r0, r0 + r1 became
// r0 + r0 in the ISA: 1e-2 errors on MI355X, invisible to the CPU emulation; tools/microbench/tr16_probe.hip checks the pinned form on the hardware)
__device__ __forceinline__ void fa_swap32(float v, float &lo, float &hi) {
    const uint32_t a = __builtin_bit_cast(uint32_t, v);
    const auto r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
    uint32_t r0 = r[0], r1 = r[1];
    asm volatile("" : "+v"(r0), "+v"(r1));
    lo = __builtin_bit_cast(float, r0); hi = __builtin_bit_cast(float, r1);           // lo: the value of lane l % 32, hi: of lane 32 + l % 32
}
__device__ __forceinline__ float fa_max_xor32(float v) { float lo, hi; fa_swap32(v, lo, hi); return fmaxf(lo, hi); }
__device__ __forceinline__ float fa_sum_xor32(float v) { float lo, hi; fa_swap32(v, lo, hi); return lo + hi; }
extern __shared__ __attribute__((aligned(16))) uint8_t fa_dyn_lds[];
#else
static inline float fa_max_xor32(float v) { return fmaxf(v, __shfl_xor(v, 32)); }
static inline float fa_sum_xor32(float v) { const float o = __shfl_xor(v, 32); return (emu::t_threadIdx.x & 32) ? o + v : v + o; }      // (lanes 0-31's value first, like the swap)
extern uint8_t fa_dyn_lds[];                                     // tools/emul: the harness defines it (a work-group is a process)
#endif

// online-softmax update of a WHOLE 64-key chunk without softcap, the scale folded into the exponent: with y = raw score (+ mask * slope / scale), c2 = scale * log2(e) > 0,
//     x2 = c2 y (the log2-domain score of fa_softmax_blocks),  max x2 = c2 max y,  2^(x2 - M) = v_exp_f32(fma(y, c2, -M))
// — per score one fma (mask, read as fp16: v_fma_mix), one max, one fma, one exp, one add, one conversion.  (M, S) stay in the log2 domain: a ragged last chunk goes
// through fa_softmax_blocks with the same running values.
template <int NKB, bool MASK>
__device__ __forceinline__ float fa_softmax_fast(floatx16 (&s)[NKB], const half4_t (&mreg)[NKB * 4], float c2, float mslope, float &M, float &S, half8_t (&pf)[NKB * 2]) {
    if constexpr (MASK) {
#pragma unroll
        for (int kb = 0; kb < NKB; kb++)
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int j = 0; j < 4; j++) s[kb][4 * g + j] = __builtin_fmaf((float)mreg[kb * 4 + g][j], mslope, s[kb][4 * g + j]);
    }
    float mx = s[0][0];
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
    mx = fa_max_xor32(mx);
    const float Mn = fmaxf(M, mx * c2);
    const float Ms = (Mn == -INFINITY) ? 0.0f : Mn;                             // (see fa_softmax_step)
    const float ms = __builtin_amdgcn_exp2f(M - Ms);
    float sum = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][r], c2, -Ms));
            sum += e; pf[kb * 2 + (r >> 3)][r & 7] = (half_t)e;
        }
    sum = fa_sum_xor32(sum);
    S = S * ms + sum; M = Mn;
    return ms;
}

// Which 64-key chunks does a query tile need at all?  A chunk whose mask entries are -inf for every row the tile's waves compute contributes P = 0, leaves (M, S) as they
// are and multiplies O by 2^0: skipping it is bit-neutral — and it is what the reference does entry by entry (`if (mv == -INFINITY) continue`, ggml-cpu.c:10935-10938).  Under
// a causal mask that is half of all chunks.  flags[tile][chunk] = 1 iff some entry of (the tile's rows) x (the chunk's keys) is not -inf; one work-group per (chunk, tile), which
// stops at the first such entry (a mask without -inf stretches costs one 16-byte load per lane).  Rows: the tile's own and — ragged last tile — the rows its waves take instead
// (k_flash_attn_pipe: the last 32).
__global__ __launch_bounds__(256) void k_fa_mask_flags(const fattn_params p, int tile_rows, int nchunk, uint8_t *flags) {
    __shared__ int any;
    const int tid = threadIdx.x, c = blockIdx.x, t = blockIdx.y;
    const int r_lo = min(t * tile_rows, max(p.n_q - 32, 0)), r_hi = min((t + 1) * tile_rows, p.n_q);
    if (tid == 0) any = 0;
    __syncthreads();
    const int col = 64 * c + 8 * (tid & 7);
    for (int r0 = r_lo; r0 < r_hi; r0 += 32) {
        const int r = r0 + (tid >> 3);
        bool mine = false;
        if (r < r_hi && col < p.n_kv) {
            const uint16_t *row = (const uint16_t *)(p.mask + (int64_t)r * p.mask_nb1) + col;
            if (col + 8 <= p.n_kv) {
                const u32x4 w = *reinterpret_cast<const u32x4 *>(row);
                mine = w.x != 0xFC00FC00u || w.y != 0xFC00FC00u || w.z != 0xFC00FC00u || w.w != 0xFC00FC00u;
            } else {
                for (int e = 0; col + e < p.n_kv; e++) mine = mine || row[e] != 0xFC00u;
            }
        }
        if (mine) any = 1;
        __syncthreads();
        if (any) break;                                             // (uniform: read behind the barrier)
    }
    if (tid == 0) flags[(int64_t)t * nchunk + c] = (uint8_t)(any != 0);
}

struct fa_true { static constexpr bool value = true; };
struct fa_false { static constexpr bool value = false; };
// MODE 0: no mask, no softcap, scale > 0; 1: the same with a 16-byte-aligned mask, staged through LDS (below); 2: everything else (fa_softmax_blocks on every chunk)
//
// Pipeline (round 6, second form — the counters of the first, register-staged form said: LDS conflict-free, but the matrix pipe 33 % busy in the steady state because a
// wave's scores -> softmax -> P.V chain ran strictly in sequence and the two waves of a SIMD, held in step by the barrier, were in the SAME phase most of the time):
//   * K / V / mask chunks travel by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write pass): requested at the top of a chunk into the buffer the last
//     barrier freed, waited for (vmcnt(0)) in front of the barrier that ends the chunk — a whole chunk of flight time.  The LDS image of a DMA piece is lane-linear, so the
//     swizzles are applied to the SOURCE address: the lane that fills LDS cell (row, s') fetches slot s' ^ swizzle(row) of that row.
//   * the scores run ONE chunk ahead of the softmax: chunk c's step issues the 16 MFMAs of S(c + 1) = K(c + 1) Q^T next to the VALU work of softmax(S(c)) — independent
//     instruction streams of one wave, which the matrix pipe and the VALU execute side by side — then P(c) V(c).  Two score accumulators alternate (the loop is unrolled
//     by two so that no register copies are needed); K is therefore staged a chunk ahead of V.
template <int HS, int NW, int MODE>
__global__ __launch_bounds__(64 * NW, 2) void k_flash_attn_pipe(const fattn_params p, int qtiles, int xcd_map, const uint8_t *flags) {
    constexpr int NS = HS / 16, NB = HS / 32, NKB = 2, CK = 64;
    constexpr int RB = HS * 2, SPR = HS / 8;                      // bytes / 16-byte slots of a K / V row
    constexpr int CB = CK * RB, NP = CB / 1024, PW = NP / NW;     // bytes of a chunk, 1 KB DMA pieces per chunk and matrix, pieces per wave
    static_assert(HS == 64 || HS == 128, "head sizes 64 / 128"); static_assert(PW >= 1 && NP % NW == 0, "DMA pieces");
    uint8_t *const smem = fa_dyn_lds;                             // K [2][CB] | V [2][CB] | MODE 1: mask [NW][2][32 rows x 128 B] | chunk list: count, ids (uint16 x 4096)
    constexpr int K_OFF = 0, V_OFF = 2 * CB, M_OFF = 4 * CB, L_OFF = 4 * CB + (MODE == 1 ? NW * 8192 : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n = lane & 31, h = lane >> 5;
    const uint32_t lds0 = CDNA4_LDS_BASE(smem);
    // work item of this work-group: consecutive items on one XCD (work-groups go to the XCDs round-robin)
    // (work-groups go to the XCDs round-robin: XCD x = blockIdx % 8 runs its slot-th item, slot = blockIdx / 8).  Without a mask an XCD takes whole heads (their K / V
    // are read from memory once); with one — the same mask tile for every head — it takes a quarter of the (batch, head) pairs x every second query tile, eight query
    // tiles of four heads at a time, so that K / V chunks AND mask chunks are each shared by several work-groups of the XCD's L2 while they stream
    // (first form: whole heads per XCD with a mask — 842 MB fetched beyond the L2 for 160 MB of operands, every mask request an L2 miss)
    int qt, hb;
    {
        const int nwg = (int)gridDim.x, hbs = nwg / qtiles, x = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
        if (xcd_map == 1 && (qtiles & 1) == 0 && (hbs & 3) == 0) {
            const int qh = qtiles >> 1, hq = hbs >> 2;             // query tiles / (batch, head) pairs of one XCD
            // query tiles of one parity per XCD, the LAST tile first: under a causal mask tile t walks t + 1 times as many chunks as tile 0 — halves of the tile range
            // per XCD left the upper half's XCDs with 2.8 times the work (255 us at 4096^2); late work-groups should be the short ones
            // (the dispatcher seems to stripe work-groups over a few queues per XCD before they find a free CU: tile heights that descend with the slot gave 256 us like the
            // unbalanced halves did.  The order below — 7 5 3 1 0 2 4 6 for eight tiles, rotated by the head — gives every residue class of the slot mod 2 / 4 the same work.)
            const int j = (slot % qh + slot / qh) % qh, rank = (qh & 1) ? j : (j < qh / 2 ? qh - 1 - 2 * j : 2 * (j - qh / 2));
            hb = (x >> 1) * hq + slot / qh; qt = 2 * rank + (x & 1);
        } else {
            const int w = (nwg & 7) == 0 ? x * (nwg >> 3) + slot : (int)blockIdx.x;
            qt = w % qtiles; hb = w / qtiles;
        }
    }
    // key split (p.nsplit > 1: grids below one work-group per CU — a prefill chunk of a few hundred rows against a long context): the (batch, head) axis of the map above carries the
    // split as its fastest part; split s walks chunks [s, s + 1) * chunks_per_split and leaves (M, S, O) unnormalized for k_flash_attn_pipe_merge
    const int split = p.nsplit > 1 ? hb % p.nsplit : 0;
    if (p.nsplit > 1) hb /= p.nsplit;
    const int head = hb % p.n_head, b3 = hb / p.n_head;
    // a wave whose 32 rows would reach past the end takes the LAST 32 rows instead (n_q >= 32 here): it recomputes rows another wave also computes — a row's result does
    // not depend on who computes it, both store the same bits — and nothing below has to clamp a query row
    const int q0 = min(qt * (32 * NW) + 32 * wave, p.n_q - 32);
    const int qi = q0 + n;

    half8_t qf[NS];
    fa_load_q<NS>(p, qi, head, b3, h, qf);
    const float slope2 = fa_slope(p, head) * 1.4426950408889634f;
    const float c2 = p.scale * 1.4426950408889634f, mslope = slope2 / c2;       // (MODE 0 / 1: p.scale > 0, no softcap)
    const uint8_t *kbase = (const uint8_t *)p.k + (int64_t)(head / p.rk2) * p.k_nb2 + (int64_t)(b3 / p.rk3) * p.k_nb3;
    const uint8_t *vbase = (const uint8_t *)p.v + (int64_t)(head / p.rv2) * p.v_nb2 + (int64_t)(b3 / p.rv3) * p.v_nb3;
    const half_t *mrow = p.mask ? (const half_t *)(p.mask + (int64_t)qi * p.mask_nb1) : nullptr;

    float M = -INFINITY, S = 0.0f;
    floatx16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;

    // row swizzles: K slot ^= ksw(row) (16 distinct slots over any 16 consecutive rows); V 64-byte segment ^= vsw(row) (the 4 rows of a transpose read land in 4 bank quarters);
    // mask slot ^= (row / 2) % 8 (8-byte reads of one slot column over 32 rows: 2-way, eight reads per chunk)
    auto ksw = [](int row) { return HS == 128 ? (row & 15) : ((row >> 1) & 7); };
    auto vsw = [](int row) { return HS == 128 ? (row & 3) : ((row >> 1) & 1); };
    // DMA piece j of a chunk = LDS cells 64 j .. 64 j + 63 (16 bytes each): lane l fills cell (row (64 j + l) / SPR, slot (64 j + l) % SPR); wave w moves pieces w, w + NW, ..
    // The source offsets of a whole chunk do not depend on the chunk: computed once.  A ragged last chunk clamps its rows (repeated rows, masked in the softmax).
    // One source offset per matrix: piece i of a wave lies DR = 64 NW / SPR rows behind piece i - 1, a multiple of 16, which every swizzle above ignores — the row
    // distance goes into the (scalar) base address.  The mask's four pieces: rows 8 i + l / 8, swizzle (row / 2) % 8 — pieces 0 / 2 and 1 / 3 share their offsets.
    constexpr int DR = 64 * NW / SPR;
    static_assert(PW == 1 || DR % 16 == 0, "piece stride vs swizzle period");
    auto kv_voff = [&](int i, bool is_v, int lim) __attribute__((always_inline)) {      // (32-bit arithmetic: the launcher checked 64 rows' worth of stride)
        const int j = wave + NW * i, cell = 64 * j + lane, row = cell / SPR, sp = cell % SPR;
        const int slot = is_v ? ((((sp >> 2) ^ vsw(row)) << 2) | (sp & 3)) : (sp ^ ksw(row));
        return (uint32_t)min(row, lim) * (uint32_t)(is_v ? p.v_nb1 : p.k_nb1) + (uint32_t)(16 * slot);
    };
    const uint32_t kvoff = kv_voff(0, false, CK - 1), vvoff = kv_voff(0, true, CK - 1);
    uint32_t moff[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int cell = 64 * i + lane, row = cell >> 3, sp = cell & 7;
        moff[i] = (uint32_t)(q0 + row) * (uint32_t)p.mask_nb1 + (uint32_t)(16 * (sp ^ ((row >> 1) & 7)));     // (the launcher checked n_q rows' worth of stride)
    }
    auto dma_kv = [&](int c, int buf, bool is_v, bool whole) __attribute__((always_inline)) {      // whole: the caller knows that chunk c is not the last one
        const int lim = p.n_kv - 1 - CK * c;                      // last valid row of the chunk
        const int64_t nb1 = is_v ? p.v_nb1 : p.k_nb1;
        const uint8_t *src = (is_v ? vbase : kbase) + (int64_t)(CK * c) * nb1;
        const uint32_t dst = lds0 + (is_v ? V_OFF : K_OFF) + buf * CB + 1024 * wave;
        if (whole || lim >= CK - 1) {
#pragma unroll
            for (int i = 0; i < PW; i++) CDNA4_DMA16(is_v ? vvoff : kvoff, src + (int64_t)(DR * i) * nb1, dst + 1024 * NW * i);
        } else {                                                  // ragged last chunk: rows past the end repeat the last one (masked in the softmax)
#pragma unroll
            for (int i = 0; i < PW; i++) { const uint32_t vo = kv_voff(i, is_v, lim); CDNA4_DMA16(vo, src, dst + 1024 * NW * i); }
        }
    };
    auto dma_mask = [&](int c, int buf) __attribute__((always_inline)) {      // chunk c's mask rows of this wave -> its buffer buf
        const uint8_t *src = (const uint8_t *)p.mask + 2 * (int64_t)(CK * c);
#pragma unroll
        for (int i = 0; i < 4; i++) CDNA4_DMA16(moff[i & 1], src + (int64_t)(16 * (i >> 1)) * p.mask_nb1, lds0 + M_OFF + wave * 8192 + buf * 4096 + 1024 * i);
    };
    // the same requests one piece at a time, for the hot step (whole chunks): op 0 .. NOPS - 1 = [MODE 1: the four mask pieces of chunk c + 1,] the PW K pieces of chunk
    // c + 2, the PW V pieces of chunk c + 1 — issued one per section of the score / softmax stretch instead of as a burst behind the barrier (eight pieces per wave
    // back to back, from all eight waves at once, cost the 4096^2 case 170 us: an LDS-DMA piece occupies the wave's issue for 60 - 185 cycles)
    constexpr int NOPS = (MODE == 1 ? 4 : 0) + 2 * PW;
    auto dma_op = [&](int op, int st, int ch1, int ch2) __attribute__((always_inline)) {      // step st; ch1 / ch2: the chunks of steps st + 1 / st + 2
        if (MODE == 1 && op < 4) {
            CDNA4_DMA16(moff[op & 1], (const uint8_t *)p.mask + 2 * (int64_t)(CK * ch1) + (int64_t)(16 * (op >> 1)) * p.mask_nb1, lds0 + M_OFF + wave * 8192 + ((st + 1) & 1) * 4096 + 1024 * op);
        } else {
            const int i = (op - (MODE == 1 ? 4 : 0)) % PW; const bool is_v = (op - (MODE == 1 ? 4 : 0)) >= PW;
            const int cc = is_v ? ch1 : ch2, buf = is_v ? (st + 1) & 1 : st & 1;
            const int64_t nb1 = is_v ? p.v_nb1 : p.k_nb1;
            CDNA4_DMA16(is_v ? vvoff : kvoff, (is_v ? vbase : kbase) + (int64_t)(CK * cc + DR * i) * nb1, lds0 + (is_v ? V_OFF : K_OFF) + buf * CB + 1024 * wave + 1024 * NW * i);
        }
    };
    // this lane's share of the operand addresses: K fragment (kb, st) = row 32 kb + n, slot 2 st + h; V transpose read (b, kt, u) = row 16 kt + 8 u + 4 h + i / 4,
    // bytes 64 b + 32 g1 + 8 (i % 4) .. + 7 of the row (i = lane % 16, g1 = (lane / 16) % 2)
    const int ti = lane & 15, g1 = (lane >> 4) & 1;
    const int krow = n * RB, kx = ksw(n);
    const int vrow = (4 * h + (ti >> 2)) * RB + 32 * g1 + 8 * (ti & 3), vx = vsw(4 * h + (ti >> 2));
    const uint8_t *const Mw = smem + M_OFF + wave * 8192 + n * 128;        // (+ 4096 for odd chunks)
    const int mx8 = (n >> 1) & 7;

    const int nchunk = (p.n_kv + CK - 1) / CK, nfast = MODE == 2 ? 0 : p.n_kv / CK;
    // the chunks this tile walks, in ascending order: all of them, or — with flags from k_fa_mask_flags — those that are not -inf throughout for every row of the tile.
    // The pipeline below counts STEPS i = 0 .. nlist - 1 (buffer parities follow i); the chunk of step i is cid(i).  Only the last entry can be the ragged chunk.
    uint16_t *const lst = reinterpret_cast<uint16_t *>(smem + L_OFF);
    if (wave == 0) {
        int count = 0;
        const int c_lo = split * p.chunks_per_split, c_hi = p.nsplit > 1 ? min(nchunk, c_lo + p.chunks_per_split) : nchunk;
        for (int base = c_lo; base < c_hi; base += 64) {
            const int c = base + lane;
            const bool keep = c < c_hi && (!flags || flags[(int64_t)qt * nchunk + c] != 0);
            const uint64_t bal = wave_ballot(keep);
            if (keep) lst[1 + count + __builtin_popcountll(bal & ((1ull << lane) - 1))] = (uint16_t)c;
            count += __builtin_popcountll(bal);
        }
        if (lane == 0) { if (count == 0) { lst[1] = (uint16_t)min(c_lo, nchunk - 1); count = 1; } lst[0] = (uint16_t)count; }      // (everything masked: one chunk alone gives what all of them would)
    }
    __syncthreads();
    const int nlist = __builtin_amdgcn_readfirstlane((int)lst[0]);
    auto cid = [&](int i) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane((int)lst[1 + i]); };
#ifdef FA_STAMP
    uint32_t stamp[6] = {};
#endif
    auto scores = [&](int c, floatx16 (&s)[NKB]) __attribute__((always_inline)) {
        const uint8_t *Kc = smem + K_OFF + (c & 1) * CB;
#pragma unroll
        for (int kb = 0; kb < NKB; kb++) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[kb][r] = 0.0f;
#pragma unroll
            for (int st = 0; st < NS; st++)
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8_t *>(Kc + 32 * kb * RB + krow + 16 * ((2 * st + h) ^ kx)), qf[st], s[kb], 0, 0, 0);
        }
    };
    // chunk c: [top] request K(c + 2), V(c + 1) into the buffers the last barrier freed; scores of chunk c + 1 next to the softmax of chunk c (sc -> P); request mask(c + 1);
    // O = O ms + V(c)^T P; all requests landed, barrier.  HOT: chunks c + 1, c + 2 exist and are not the last, chunk c is a whole chunk on the fast path — no branches around the MFMA / VALU mix.
    auto step = [&](int c, floatx16 (&sc)[NKB], floatx16 (&sn)[NKB], auto hot_tag) __attribute__((always_inline)) {      // c: the STEP; its chunk is ch0
        constexpr bool HOT = decltype(hot_tag)::value;
        const int ch0 = cid(c), ch1 = (HOT || c + 1 < nlist) ? cid(c + 1) : 0, ch2 = (HOT || c + 2 < nlist) ? cid(c + 2) : 0;      // the chunks of steps c, c + 1, c + 2
        const bool fast = HOT || ch0 < nfast;
        if constexpr (!HOT) {
            if (c + 2 < nlist) dma_kv(ch2, c & 1, false, false);
            if (c + 1 < nlist) dma_kv(ch1, (c + 1) & 1, true, false);
            if constexpr (MODE == 1) { if (c + 1 < nlist && ch1 < nfast) dma_mask(ch1, (c + 1) & 1); }       // (its buffer was last read by the softmax of step c - 1, in front of the last barrier)
        }
        half8_t pf[NKB * 2];
        float ms;
#ifdef FA_STAMP
        const uint64_t t0 = __builtin_amdgcn_s_memtime();
        uint64_t t1 = t0, t2 = t0, t3 = t0, t4 = t0;
#endif
        if constexpr (HOT) {
            // The issue order is written out: a wave issues in order, so what is to run beside an MFMA has to stand behind it in the instruction stream, and hipcc's
            // scheduler left to itself puts the 16 score MFMAs of chunk c + 1 in front of the whole softmax of chunk c.  Sixteen sections, fenced by sched_barrier(0):
            // section m = the K fragment read of MFMA m + 2, MFMA m, one slice of the softmax — slices 0..7 the mask term and the running maximum of four scores each,
            // then the row maximum and the factors, slices 8..15 exponent, sum and fp16 conversion of four scores each.
            const uint8_t *Kn = smem + K_OFF + ((c + 1) & 1) * CB + krow;
            auto kfrag = [&](int m) __attribute__((always_inline)) { return *reinterpret_cast<const half8_t *>(Kn + 32 * (m / NS) * RB + 16 * ((2 * (m % NS) + h) ^ kx)); };
            constexpr int NM = NKB * NS, SL = 32 / NM;              // MFMAs of a chunk's scores; scores per softmax slice of a half (HS 128: 16 MFMAs, 4 scores; HS 64: 8 MFMAs, 8 scores)
            constexpr int GS = 2 * SL / 4;                          // mask groups (four scores: one 8-byte read) per slice; requested one slice ahead
            half4_t mreg[NKB * 4] = {};
            auto mask_groups = [&](int sl) __attribute__((always_inline)) {
                if constexpr (MODE == 1) {
#pragma unroll
                    for (int g = GS * sl; g < GS * (sl + 1); g++) mreg[g] = *reinterpret_cast<const half4_t *>(Mw + (c & 1) * 4096 + 16 * (g ^ mx8) + 8 * h);
                }
            };
            constexpr int MPF = NM / 2;                             // mask groups requested this many slices ahead (all of them at the top: one slice ahead left every slice of
#pragma unroll                                                      // the first half waiting a full LDS round trip — 2,190 - 2,870 cycles for the half against 600 - 1,100 without a mask)
            for (int sl = 0; sl < MPF && sl < NM / 2; sl++) mask_groups(sl);
            half8_t kf[NM];
            kf[0] = kfrag(0); kf[1] = kfrag(1);
#pragma unroll
            for (int kb = 0; kb < NKB; kb++)
#pragma unroll
                for (int r = 0; r < 16; r++) sn[kb][r] = 0.0f;
            float mx = -INFINITY, Ms = 0.0f, sum = 0.0f;
            ms = 1.0f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < NM; m++) {
                if (m + 2 < NM) kf[m + 2] = kfrag(m + 2);
                sn[m / NS] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[m], qf[m % NS], sn[m / NS], 0, 0, 0);
#pragma unroll
                for (int op = m * NOPS / NM; op < (m + 1) * NOPS / NM; op++) dma_op(op, c, ch1, ch2);      // (NOPS requests spread evenly over the NM sections)
                if (m < NM / 2) {                                   // slice m of the first half: 2 SL scores
                    if (m + MPF < NM / 2) mask_groups(m + MPF);
#pragma unroll
                    for (int e = 2 * SL * m; e < 2 * SL * (m + 1); e++) {
                        const int kb = e >> 4, r = e & 15;
                        if constexpr (MODE == 1) sc[kb][r] = __builtin_fmaf((float)mreg[kb * 4 + (r >> 2)][r & 3], mslope, sc[kb][r]);
                        mx = fmaxf(mx, sc[kb][r]);
                    }
                    if (m == NM / 2 - 1) {
                        mx = fa_max_xor32(mx);
                        const float Mn = fmaxf(M, mx * c2);
                        Ms = (Mn == -INFINITY) ? 0.0f : Mn;             // (see fa_softmax_step)
                        ms = __builtin_amdgcn_exp2f(M - Ms);
                        M = Mn;
                    }
                } else {
#pragma unroll
                    for (int e = 2 * SL * (m - NM / 2); e < 2 * SL * (m - NM / 2 + 1); e++) {
                        const int kb = e >> 4, r = e & 15;
                        const float ex = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][r], c2, -Ms));
                        sum += ex; pf[kb * 2 + (r >> 3)][r & 7] = (half_t)ex;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#ifdef FA_STAMP
                if (m == NM / 2 - 1) t1 = __builtin_amdgcn_s_memtime();
#endif
            }
#ifdef FA_STAMP
            t2 = __builtin_amdgcn_s_memtime();
#endif
            sum = fa_sum_xor32(sum);
            S = S * ms + sum;
        } else {
            if (c + 1 < nlist) scores(c + 1, sn);
            half4_t mreg[NKB * 4] = {};
            if (fast) {
                if constexpr (MODE == 1) {
#pragma unroll
                    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
                        for (int g = 0; g < 4; g++) mreg[kb * 4 + g] = *reinterpret_cast<const half4_t *>(Mw + (c & 1) * 4096 + 16 * ((4 * kb + g) ^ mx8) + 8 * h);
                }
                ms = fa_softmax_fast<NKB, MODE == 1>(sc, mreg, c2, mslope, M, S, pf);
            } else {
                fattn_params pg = p; pg.mask_vec = 0;               // (element-wise path: mreg is not filled here)
                ms = fa_softmax_blocks<NKB>(pg, sc, CK * ch0, h, mrow, slope2, mreg, M, S, pf);
            }
        }
        const uint8_t *Vc = smem + V_OFF + (c & 1) * CB;
        if (wave_any(ms != 1.0f)) {                                 // (one branch in front of the block loop: see k_flash_attn_split)
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[b][r] *= ms;
        }
#pragma unroll
        for (int kt = 0; kt < NKB * 2; kt++)                        // (consecutive MFMAs on different accumulators)
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const uint8_t *va = Vc + 16 * kt * RB + vrow + 64 * (b ^ vx);
                const half4_t lo = fa_lds_tr16(va), hi = fa_lds_tr16(va + 8 * RB);
                const half8_t vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kt], o[b], 0, 0, 0);
            }
#ifdef FA_STAMP
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        t3 = __builtin_amdgcn_s_memtime();
#endif
        CDNA4_WAIT_VM(0);
#ifdef FA_STAMP
        t4 = __builtin_amdgcn_s_memtime();
#endif
        __syncthreads();                                          // everyone is done with K(c + 1)'s and V(c)'s reads; K(c + 2), V(c + 1), mask(c + 1) are in LDS
#ifdef FA_STAMP
        if (HOT) { const uint64_t t5 = __builtin_amdgcn_s_memtime(); stamp[0] += (uint32_t)(t1 - t0); stamp[1] += (uint32_t)(t2 - t1); stamp[2] += (uint32_t)(t3 - t2); stamp[3] += (uint32_t)(t4 - t3); stamp[4] += (uint32_t)(t5 - t4); stamp[5]++; }
#endif
    };

    dma_kv(cid(0), 0, false, false); dma_kv(cid(0), 0, true, false);
    if (nlist > 1) dma_kv(cid(1), 1, false, false);
    if constexpr (MODE == 1) { if (cid(0) < nfast) dma_mask(cid(0), 0); }
    CDNA4_WAIT_VM(0);
    __syncthreads();
    floatx16 sa[NKB], sb[NKB];
    scores(0, sa);
    __syncthreads();                                              // K(0) has been read by every wave: chunk 0's step may overwrite it with K(2)
    int c = 0;
    for (; c + 4 < nlist && nfast > 0; c += 2) { step(c, sa, sb, fa_true{}); step(c + 1, sb, sa, fa_true{}); }       // (steps c .. c + 3 are not the last: whole chunks)
    for (; c + 1 < nlist; c += 2) { step(c, sa, sb, fa_false{}); step(c + 1, sb, sa, fa_false{}); }
    if (c < nlist) step(c, sa, sb, fa_false{});
#ifdef FA_STAMP
    if ((blockIdx.x == 0 || blockIdx.x == 300) && lane == 0 && (wave == 0 || wave == 5))
        printf("FA_STAMP block %d wave %d hot steps %u: first half %u | second half %u | rescale + PV %u | vmcnt %u | barrier %u cycles per step\n", (int)blockIdx.x, wave, stamp[5],
               stamp[0] / stamp[5], stamp[1] / stamp[5], stamp[2] / stamp[5], stamp[3] / stamp[5], stamp[4] / stamp[5]);
#endif
    if (p.nsplit == 1) {
        fa_store<NB>(p.dst + (((int64_t)b3 * p.n_q + qi) * p.n_head + head) * HS, o, 1.0f / S, h);
    } else {                                                      // [batch][head][query row][split][M, S, -, -, O]
        float *pt = p.part + ((((int64_t)b3 * p.n_head + head) * p.n_q + qi) * p.nsplit + split) * (HS + 4);
        if (h == 0) { pt[0] = M; pt[1] = S; }
        fa_store<NB>(pt + 4, o, 1.0f, h);
    }
}
// out[q][d] = sum_s O_s[q][d] 2^(M_s - M*) / sum_s S_s 2^(M_s - M*), splits in index order (deterministic).  One work-group per (32 query rows, head, batch).
template <int HS>
__global__ __launch_bounds__(256) void k_flash_attn_pipe_merge(const fattn_params p) {
    const int q0 = 32 * blockIdx.x, head = blockIdx.y, b3 = blockIdx.z;
    for (int i = threadIdx.x; i < 32 * HS; i += 256) {
        const int q = q0 + i / HS, d = i % HS;
        if (q >= p.n_q) break;
        const float *base = p.part + (((int64_t)b3 * p.n_head + head) * p.n_q + q) * p.nsplit * (HS + 4);
        float Mx = -INFINITY;
        for (int s = 0; s < p.nsplit; s++) Mx = fmaxf(Mx, base[s * (HS + 4)]);
        float num = 0.0f, den = 0.0f;
        for (int s = 0; s < p.nsplit; s++) {
            const float *pt = base + s * (HS + 4);
            const float a = (pt[0] == -INFINITY) ? 0.0f : exp2f(pt[0] - Mx);      // (M in the log2 domain)
            num += pt[4 + d] * a; den += pt[1] * a;
        }
        p.dst[(((int64_t)b3 * p.n_q + q) * p.n_head + head) * HS + d] = num * (1.0f / den);
    }
}
template <int HS, int NW, int MODE> constexpr int k_flash_attn_pipe_lds() { return 4 * 64 * HS * 2 + (MODE == 1 ? NW * 8192 : 0) + 8192 + 16; }

#define NEED(cond, msg) do { if (!(cond)) return cdna4_set_error_msg(msg); } while (0)
typedef ggml_cdna4_tensor T4;

// the kernels exist for head sizes 64 / 128 / 256; any other head size up to 256 runs zero-padded to the next of them (copies, see below)
static inline bool fa_kernel_head_size(int64_t hs) { return hs == 64 || hs == 128 || hs == 256; }
extern "C" int ggml_cdna4_op_flash_attn_ext_supported(int64_t head_size, int kv_type) {
    if (head_size <= 0 || head_size > 256) return 0;
    return kv_type == CDNA4_F16 || kv_type == CDNA4_BF16 || (cdna4_to_f16_dense_supported(kv_type) && head_size % 32 == 0);
}
// ---- The launch plan: everything a call does after its argument checks — staging, kernel family and form, key split, merge, grids, LDS and scratch sizes.  fa_make_plan fills it from
// the descriptors alone: it reads its arguments, cdna4_gemm_cu_count() and the CDNA4_FA_* knobs, and allocates, launches and reports nothing; ggml_cdna4_op_flash_attn_ext executes it.
enum { FA_STAGE_NONE, FA_STAGE_COPY, FA_STAGE_PAD };                     // K / V read as they are | fp16 copy of the K / V that are not F16 | zero-padded copies of q, K, V and dst
enum { FA_PIPE, FA_WIDE, FA_SPLIT };                                     // k_flash_attn_pipe | k_flash_attn_wide64 / _wide | k_flash_attn_split
enum { FA_MERGE_NONE, FA_MERGE_TILES, FA_MERGE_ROWS, FA_MERGE_PIPE };    // - | k_flash_attn_merge | k_flash_attn_merge_rows | k_flash_attn_pipe_merge
struct fa_plan {
    int stage, family, kv_type, hs;                                      // kv_type, hs: the K / V type and head size the kernels see (behind the staging)
    int nw, mode, xcd_map; int64_t qtiles, items;                        // k_flash_attn_pipe: waves per work-group (32 query rows each), mode, XCD map, query tiles, work-groups
    int nsplit, chunks_per_split, chunk;                                 // key split over work-groups, in chunks of `chunk` keys; nsplit == 1: no kernel reads chunks_per_split (it covers all keys)
    int pack, mask_vec, merge, block, lds;                               // pack: k_flash_attn_split only (0 otherwise)
    dim3 grid, fgrid, mgrid; size_t part_bytes, flag_bytes;              // main / k_fa_mask_flags / merge grids; scratch of the partial results (nsplit > 1) and of the chunk flags (0: no flag pass)
};
// f(HS, NW, MODE) as integral constants for the forms of k_flash_attn_pipe that exist; false (f not called): there is none.  Only those are instantiated
// (head size 128 has no 2-wave form: its DMA pieces would straddle the K swizzle's period)
template <typename F> static inline bool fa_pipe_dispatch(int hs, int nw, int mode, F &&f) {
    bool hit = false;
    cdna4_dispatch(cdna4_types<64, 128>{}, hs, [&](auto HS) { cdna4_dispatch(cdna4_types<2, 4, 8>{}, nw, [&](auto NW) {
        if constexpr (HS.value == 64 || NW.value != 2) hit = cdna4_dispatch(cdna4_types<0, 1, 2>{}, mode, [&](auto MODE) { f(HS, NW, MODE); }); }); });
    return hit;
}
static bool fa_one_grid(int64_t wgs) { return wgs < (1ll << 31); }
static void fa_split_keys(fa_plan &pl, int64_t nc, int64_t want) { pl.chunks_per_split = (int)((nc + want - 1) / want); pl.nsplit = (int)((nc + pl.chunks_per_split - 1) / pl.chunks_per_split); }
// the descriptor of a staged copy of t: dense rows of n0 elements of `type` (F16 for K / V, F32 for q / dst); its address comes with the staging
static T4 fa_dense(T4 t, int type, int64_t n0) { t.data = nullptr; t.type = type; t.ne[0] = n0; t.nb[0] = type == CDNA4_F32 ? 4 : 2; for (int i = 1; i < 4; i++) t.nb[i] = t.nb[i - 1] * t.ne[i - 1]; return t; }
// the kernels of a call on the K / V they see (behind the staging) at the kernel head size D (q's, padded); exp2: no softcap and a positive scale (what the pipelined kernel's modes 0 / 1 need)
static fa_plan fa_plan_kernels(const T4 *q, const T4 *k, const T4 *v, const T4 *mask, bool exp2, int64_t D) {
    const auto n = [](int64_t x) { return std::max<int64_t>(x, 1); };      // (sizes the checks reject, or that leave nothing to do: the plan is total, nothing runs on it)
    const int64_t N = n(q->ne[1]), H = n(q->ne[2]), B3 = n(q->ne[3]), KV = n(k->ne[1]), rk2 = H / n(k->ne[2]), cus = cdna4_gemm_cu_count();
    const int kvt = k->type; fa_plan pl{}; pl.kv_type = kvt; pl.hs = (int)D; pl.block = 256; pl.nsplit = 1; pl.chunk = 32; pl.chunks_per_split = (int)((KV + 31) / 32);
    pl.mask_vec = mask && !(((uintptr_t)mask->data | (uintptr_t)mask->nb[1]) & 15);
    // head sizes 64 / 128 with an F16 K / V: the pipelined kernel on the largest query tile (256 / 128 / 64 rows) that still gives every CU a work-group
    // (CDNA4_FA_PIPE: measurement / test knob — 0 keeps the older kernels, 2 / 4 / 8 forces that many waves per work-group whatever the grid)
    // (beyond its 32-bit source offsets, its chunk list or one grid the call takes the older kernels below: never an error)
    const bool pipe_fits = KV <= 4095 * 64 && k->nb[1] < (1ll << 25) && v->nb[1] < (1ll << 25) && (!mask || (N + 16) * (int64_t)mask->nb[1] < (1ll << 32)) && fa_one_grid(((N + 63) / 64) * H * B3);
    if (kvt == CDNA4_F16 && (D == 64 || D == 128) && N > 32 && pipe_fits) {
        const char *e = getenv("CDNA4_FA_PIPE"), *es = getenv("CDNA4_FA_PIPE_SPLIT");
        const int64_t nc = (KV + 63) / 64;
        int nw = e ? atoi(e) : -1;
        int64_t split = 0;                                             // splits asked for (0: none considered); applied below only where a pipelined form is taken, so no other kernel's plan carries it
        if (nw < 0) {
            nw = 0;
            for (int w = 8; w >= (D == 128 ? 4 : 2) && !nw; w >>= 1)
                if (((N + 32 * w - 1) / (32 * w)) * H * B3 >= cus) nw = w;
            // below one work-group per CU: the smallest tile (128 rows at head size 128, 64 at 64) with the keys split over as many work-groups as fill the chip, each split at
            // least four chunks (CDNA4_FA_PIPE_SPLIT=0: off — then half a chip of 128-row tiles over a short key range, which still beat the key-split kernel: 25.8 against 28.8 us
            // at 512 x 512 x 32 heads)
            if (!nw && N >= 128 && !(es && atoi(es) == 0)) {
                const int w = D == 128 ? 4 : 2;
                const int64_t it = ((N + 32 * w - 1) / (32 * w)) * H * B3;
                int64_t want = (cus + it / 2) / it;
                static const int64_t split_min = getenv("CDNA4_FA_PIPE_SPLIT_MIN") ? atoll(getenv("CDNA4_FA_PIPE_SPLIT_MIN")) : 32;      // (A/B and test knob)
                if (want > nc / split_min) want = nc / split_min;              // (a split pays from about 32 chunks on: its partial results are written and merged — 512 x 4096 x 32 heads 150 -> 89 us with two splits of 32 chunks, 256 x 2048 46 -> 69 us with four of 8)
                if (want >= 2) { nw = w; split = want; }
            }
            if (!nw && D == 128 && KV <= 1024 && ((N + 127) / 128) * H * B3 >= cus / 2) nw = 4;
        }
        if (e && es && atoi(es) > 1) split = std::min<int64_t>(atoi(es), nc);      // (tests: a forced tile height with a forced key split)
        const int mode = (!exp2 || (mask && !pl.mask_vec)) ? 2 : (mask ? 1 : 0);
        if (fa_pipe_dispatch((int)D, nw, mode, [&](auto HS, auto NW, auto MODE) { pl.lds = k_flash_attn_pipe_lds<HS.value, NW.value, MODE.value>(); })) {
            pl.family = FA_PIPE; pl.nw = nw; pl.mode = mode; pl.block = 64 * nw; pl.chunk = 64;
            if (split) fa_split_keys(pl, nc, split);
            pl.qtiles = (N + 32 * nw - 1) / (32 * nw); pl.items = pl.qtiles * H * B3 * pl.nsplit; pl.grid = dim3((unsigned)pl.items);
            if (pl.nsplit > 1) { pl.part_bytes = (size_t)(B3 * H * N) * pl.nsplit * (D + 4) * 4 + 256; pl.merge = FA_MERGE_PIPE; pl.mgrid = dim3((unsigned)((N + 31) / 32), (unsigned)H, (unsigned)B3); }
            // chunks that are -inf throughout for a whole query tile are not walked (k_fa_mask_flags; bit-neutral): worth a pass over the mask from 2^20 entries on
            // (CDNA4_FA_NO_SKIP / CDNA4_FA_SKIP_MIN: A/B and test knobs)
            const int64_t skip_min = getenv("CDNA4_FA_SKIP_MIN") ? atoll(getenv("CDNA4_FA_SKIP_MIN")) : (1ll << 20);      // (tests: 0 takes the pass at any size)
            if (pl.mask_vec && N * KV >= skip_min && !getenv("CDNA4_FA_NO_SKIP")) { pl.flag_bytes = (size_t)(pl.qtiles * nc) + 256; pl.fgrid = dim3((unsigned)nc, (unsigned)pl.qtiles); }
            pl.xcd_map = getenv("CDNA4_FA_MAP") ? atoi(getenv("CDNA4_FA_MAP")) : (mask ? 1 : 0);     // (A/B knob; see the kernel)
            return pl;
        }
    }
    // prefill that fills the chip takes the 128-row kernels (128 query rows per work-group, K / V staged through LDS as fp16), everything else the key-split kernel
    // (CDNA4_FA_WIDE_MIN: measurement knob — the smallest number of 128-row work-groups that takes them; default: one per CU)
    static const int64_t min_wgs = getenv("CDNA4_FA_WIDE_MIN") ? atoll(getenv("CDNA4_FA_WIDE_MIN")) : 0;
    if (N > 32 && ((N + 127) / 128) * H * B3 >= (min_wgs > 0 ? min_wgs : cus)) { pl.family = FA_WIDE; pl.grid = dim3((unsigned)((N + 127) / 128), (unsigned)H, (unsigned)B3); return pl; }
    // decode / small batches: 32-row query tiles, the keys split over work-groups until the chip is full (one or two work-groups per CU, below), each split
    // >= 16 chunks
    // grouped-query decode: the heads of a K / V head in one tile (k_flash_attn_split; CDNA4_FA_NO_PACK: A/B knob)
    pl.family = FA_SPLIT; pl.pack = (rk2 > 1 && N * rk2 <= 32 && !getenv("CDNA4_FA_NO_PACK")) ? (int)rk2 : 1;
    const int64_t HT = pl.pack > 1 ? H / pl.pack : H;                // tiles along the head axis
    const int64_t nchunk = (KV + 31) / 32, qtiles = (N + 31) / 32, tiles = qtiles * HT * B3;
    // work-groups per CU the split aims at: ONE for F16 / BF16 rows (32 K keys x 32 heads 105.6 -> 99.2 us, grouped-query 8 K / V heads 60.6 -> 43.1: fewer partial results to
    // write, merge and wait for), TWO for quantized rows, whose conversion is VALU work a second resident work-group hides (Q8_0 88.6 against 108.8, Q4_0 66.7 against 81.4)
    static const int64_t wgs_knob = getenv("CDNA4_FA_SPLIT_WGS") ? atoll(getenv("CDNA4_FA_SPLIT_WGS")) : 0;      // (A/B knob)
    const int64_t wgs_per_cu = wgs_knob > 0 ? wgs_knob : (kvt == CDNA4_Q8_0 || kvt == CDNA4_Q4_0 ? 2 : 1);
    int64_t want = (wgs_per_cu * cus + tiles - 1) / tiles;
    { static const int64_t min_chunks = getenv("CDNA4_FA_SPLIT_MIN") ? atoll(getenv("CDNA4_FA_SPLIT_MIN")) : 16; if (want > nchunk / min_chunks) want = nchunk / min_chunks; }      // (each split at least 16 chunks — four per wave, which the one-chunk-ahead requests need to pay: 4 K keys x 32 heads 26.4 us at 8, 21.3 at 16, 25.4 at 32; CDNA4_FA_SPLIT_MIN: A/B knob)
    fa_split_keys(pl, nchunk, want < 1 ? 1 : want);
    pl.grid = dim3((unsigned)(qtiles * pl.nsplit), (unsigned)HT, (unsigned)B3);
    if (pl.nsplit > 1) {
        pl.part_bytes = (size_t)(qtiles * H * B3) * pl.nsplit * 32 * (D + 4) * 4 + 256;      // (per HEAD, also when the heads of a group share a tile)
        const bool rows = N <= 4 && pl.nsplit <= 512 && !getenv("CDNA4_FA_MERGE_OLD");      // a handful of rows: one work-group per row (CDNA4_FA_MERGE_OLD: A/B knob)
        pl.merge = rows ? FA_MERGE_ROWS : FA_MERGE_TILES; pl.mgrid = dim3((unsigned)(rows ? N : qtiles), (unsigned)H, (unsigned)B3);
    }
    return pl;
}
static fa_plan fa_make_plan(const T4 *q, const T4 *k, const T4 *v, const T4 *mask, bool exp2) {
    const int64_t D = q->ne[0], Dp = D <= 64 ? 64 : (D <= 128 ? 128 : 256); const bool pad = !fa_kernel_head_size(D);
    // a Q8_0 / Q4_0 / BF16 cache under the key-split kernel (decode, small batches): converted from the raw fragment bytes, no fp16 copy (fa_kv_load / fa_kv_cvt).  Only that kernel
    // reads a raw cache: a plan for the raw type that is any other kernel means the copy, and the kernels chosen for F16
    if (!pad && k->type == v->type && (k->type == CDNA4_Q8_0 || k->type == CDNA4_Q4_0 || k->type == CDNA4_BF16) && q->ne[1] < 128 && !getenv("CDNA4_FA_KV_COPY") &&      // (from 128 query rows on the F16 kernels' tiles and key split pay for the copy)
        !(((uintptr_t)k->data | (uintptr_t)v->data | (uintptr_t)k->nb[1] | (uintptr_t)k->nb[2] | (uintptr_t)k->nb[3] | (uintptr_t)v->nb[1] | (uintptr_t)v->nb[2] | (uintptr_t)v->nb[3]) & (k->type == CDNA4_BF16 ? 15 : 3))) {
        const fa_plan raw = fa_plan_kernels(q, k, v, mask, exp2, Dp);
        if (raw.family == FA_SPLIT) return raw;
    }
    const T4 ks = pad || k->type != CDNA4_F16 ? fa_dense(*k, CDNA4_F16, Dp) : *k, vs = pad || v->type != CDNA4_F16 ? fa_dense(*v, CDNA4_F16, Dp) : *v;
    fa_plan pl = fa_plan_kernels(q, &ks, &vs, mask, exp2, Dp);
    pl.stage = pad ? FA_STAGE_PAD : (k->type == CDNA4_F16 && v->type == CDNA4_F16 ? FA_STAGE_NONE : FA_STAGE_COPY);
    return pl;
}
// fills fattn_params and runs the kernel part of a plan: scratch, the optional flag pass, the main launch, the optional merge
static int fa_run(const fa_plan &pl, const T4 *q, const T4 *k, const T4 *v, const T4 *mask, const T4 *d, float scale, float max_bias, float logit_softcap, hipStream_t st) {
    const int64_t H = q->ne[2], B3 = q->ne[3];
    fattn_params p{};
    p.q = (const char *)q->data; p.k = (const char *)k->data; p.v = (const char *)v->data; p.mask = mask ? (const char *)mask->data : nullptr; p.dst = (float *)d->data;
    p.q_nb1 = q->nb[1]; p.q_nb2 = q->nb[2]; p.q_nb3 = q->nb[3];
    p.k_nb1 = k->nb[1]; p.k_nb2 = k->nb[2]; p.k_nb3 = k->nb[3]; p.v_nb1 = v->nb[1]; p.v_nb2 = v->nb[2]; p.v_nb3 = v->nb[3]; p.mask_nb1 = mask ? mask->nb[1] : 0;
    p.n_q = (int)q->ne[1]; p.n_head = (int)H; p.n_kv = (int)k->ne[1];
    p.rk2 = (int)(H / k->ne[2]); p.rk3 = (int)(B3 / k->ne[3]); p.rv2 = (int)(H / v->ne[2]); p.rv3 = (int)(B3 / v->ne[3]);
    // ggml-cpu.c:10876-10884
    p.scale = logit_softcap != 0.0f ? scale / logit_softcap : scale; p.max_bias = max_bias; p.logit_softcap = logit_softcap;
    p.n_head_log2 = 1u << (uint32_t)floorf(log2f((float)H));
    p.m0 = powf(2.0f, -(max_bias) / p.n_head_log2); p.m1 = powf(2.0f, -(max_bias / 2.0f) / p.n_head_log2);
    p.mask_vec = pl.mask_vec; p.nsplit = pl.nsplit; p.chunks_per_split = pl.chunks_per_split; p.pack = pl.pack;
    NEED(pl.family == FA_SPLIT || pl.kv_type == CDNA4_F16, "flash_attn_ext: the 128-row kernels take an F16 K / V");
    NEED(pl.family != FA_PIPE || fa_one_grid(pl.items), "flash_attn_ext: too many query tiles for one grid");      // (a forced key split: pipe_fits counted the tiles alone)
    if (pl.part_bytes) NEED(p.part = (float *)cdna4_gemm_scratch(pl.part_bytes, 4), "flash_attn_ext: cannot allocate the key-split scratch");
    uint8_t *flags = nullptr;
    if (pl.flag_bytes) {
        NEED(flags = (uint8_t *)cdna4_gemm_scratch(pl.flag_bytes, 11), "flash_attn_ext: cannot allocate the chunk flags");
        hipLaunchKernelGGL(k_fa_mask_flags, pl.fgrid, dim3(256), 0, st, p, 32 * pl.nw, (int)pl.fgrid.x, flags); CDNA4_CHECK_LAUNCH();
    }
    int rc = 0; bool hit = false; const dim3 block((unsigned)pl.block);
    if (pl.family == FA_PIPE) hit = fa_pipe_dispatch(pl.hs, pl.nw, pl.mode, [&](auto HS, auto NW, auto MODE) {
        if (pl.lds > 64 * 1024) rc = cdna4_raise_lds_limit<k_flash_attn_pipe<HS.value, NW.value, MODE.value>>(pl.lds, "flash_attn_ext: cannot raise the dynamic LDS limit");
        if (!rc) hipLaunchKernelGGL((k_flash_attn_pipe<HS.value, NW.value, MODE.value>), pl.grid, block, pl.lds, st, p, (int)pl.qtiles, pl.xcd_map, (const uint8_t *)flags);
    });
    else cdna4_dispatch(cdna4_types<64, 128, 256>{}, pl.hs, [&](auto HS) {
        // (128-row kernels — head sizes 64 / 128: 64-key chunks; 256: the 32-key-chunk kernel — its forms for the smaller heads were an A/B knob of round 3 and went in round 5)
        if (pl.family == FA_WIDE) { if constexpr (HS.value == 256) hipLaunchKernelGGL(k_flash_attn_wide<256>, pl.grid, block, 0, st, p); else hipLaunchKernelGGL(k_flash_attn_wide64<HS.value>, pl.grid, block, 0, st, p); hit = true; }
        else hit = cdna4_dispatch(cdna4_types<CDNA4_F16, CDNA4_BF16, CDNA4_Q8_0, CDNA4_Q4_0>{}, pl.kv_type, [&](auto KVT) { hipLaunchKernelGGL((k_flash_attn_split<HS.value, KVT.value>), pl.grid, block, 0, st, p); });
    });
    if (rc) return rc;
    NEED(hit, "flash_attn_ext: no kernel of this head size for this K / V type");      // (the checks leave none such: a plan that names no kernel must not pass for a result)
    CDNA4_CHECK_LAUNCH();
    if (pl.merge != FA_MERGE_NONE) cdna4_dispatch(cdna4_types<64, 128, 256>{}, pl.hs, [&](auto HS) {
        if (pl.merge == FA_MERGE_TILES) hipLaunchKernelGGL(k_flash_attn_merge<HS.value>, pl.mgrid, dim3(256), 0, st, p);
        else if (pl.merge == FA_MERGE_ROWS) hipLaunchKernelGGL(k_flash_attn_merge_rows<HS.value>, pl.mgrid, dim3(256), 0, st, p);
        else if constexpr (HS.value != 256) hipLaunchKernelGGL(k_flash_attn_pipe_merge<HS.value>, pl.mgrid, dim3(256), 0, st, p);
    });
    CDNA4_CHECK_LAUNCH();
    return 0;
}

// A BF16 K / V takes the same route (bf16 -> fp16: exact for |x| in [2^-14, 65504], the range a KV cache lives in; the CPU rounds q to bf16 instead,
// ggml-cpu.c:10929 with vec_dot_type BF16 — eight bits of mantissa — so ours is again the more accurate side).
// A quantized K / V (Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 — a quantized KV cache) is first written out as fp16 (to_float of every element rounded to
// fp16, dense [batch][head][n_kv][head_size] in library scratch: one pass over the cache), then the F16 kernels run on the copy.  The CPU
// instead quantizes q to the K type's vec_dot_type and takes integer dots (ggml-cpu.c:10921-10960); both are approximations of the same
// product, ours keeps q in fp16 like ggml-cuda's kernels do — inside the stock harness's gate, and closer to a float64 evaluation.
extern "C" int ggml_cdna4_op_flash_attn_ext(const T4 *q_in, const T4 *k_in, const T4 *v_in, const T4 *mask, const T4 *d_in,
                                            float scale, float max_bias, float logit_softcap, void *stream) {
    NEED(q_in && k_in && v_in && d_in, "flash_attn_ext: q, k, v and dst are required");
    // Head sizes without a kernel of their own (80, 96, 112, ...) run ZERO-PADDED to the next of 64 / 128 / 256: the padded components of q and k
    // add 0 to every score, the padded columns of v produce output columns that are dropped.  q, k, v are copied into padded scratch (k / v as
    // fp16), the result is computed into padded scratch and its first head_size columns copied out — four extra passes, all plain strided copies.
    const int64_t D = q_in->ne[0], N = q_in->ne[1], H = q_in->ne[2], B3 = q_in->ne[3];
    NEED(D > 0 && D <= 256, "flash_attn_ext: head size must be 1..256");
    const fa_plan pl = fa_make_plan(q_in, k_in, v_in, mask, logit_softcap == 0.0f && scale > 0.0f);      // (no side effects; the checks below ask what its staging asks)
    const bool pad = pl.stage == FA_STAGE_PAD; const int64_t Dp = pl.hs;      // (pl.hs: q's head size, padded — what k, v and dst are held to below)
    // the checks, on the descriptors the kernels will see: a staged tensor's is that of its copy, whose address comes with the staging below
    T4 kv[2] = {*k_in, *v_in}, qq = *q_in, dd = *d_in;
    const T4 *q = &qq, *k = &kv[0], *v = &kv[1], *d = &dd;
    bool staged[2];
    for (int i = 0; i < 2; i++) {
        T4 &t = kv[i];
        if (!(staged[i] = pl.stage != FA_STAGE_NONE && (t.type != CDNA4_F16 || pad))) continue;
        NEED(t.type == CDNA4_F16 || cdna4_to_f16_dense_supported(t.type), "flash_attn_ext: k / v must be F16, BF16 or Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0");
        NEED(t.ne[0] == D && (t.type == CDNA4_F16 || t.type == CDNA4_BF16 || D % 32 == 0) && t.ne[1] > 0 && t.ne[2] > 0 && t.ne[3] > 0, "flash_attn_ext: bad k / v shape");
        t = fa_dense(t, CDNA4_F16, Dp);
    }
    if (pad) {
        NEED(q->type == CDNA4_F32 && d->type == CDNA4_F32 && N > 0 && H > 0 && B3 > 0, "flash_attn_ext: F32 q / dst");
        NEED(d->ne[0] == D && d->ne[1] == H && d->ne[2] == N && d->ne[3] == B3, "flash_attn_ext: dst must be [head_size, n_head, n_q, batch]");
        qq = fa_dense(qq, CDNA4_F32, Dp); dd = fa_dense(dd, CDNA4_F32, Dp);
    }
    const int kvt = k->type;                                      // F16, or the raw BF16 / Q8_0 / Q4_0 of the key-split kernel
    const bool kvq = kvt == CDNA4_Q8_0 || kvt == CDNA4_Q4_0; const int64_t KV = k->ne[1];
    NEED(q->type == CDNA4_F32 && d->type == CDNA4_F32 && v->type == kvt && (kvt == CDNA4_F16 || kvt == CDNA4_BF16 || kvq), "flash_attn_ext: F32 q / dst and F16 k / v only");
    NEED(k->ne[0] == Dp && v->ne[0] == Dp && v->ne[1] == KV && k->ne[2] == v->ne[2] && k->ne[3] == v->ne[3], "flash_attn_ext: k / v shape mismatch");
    NEED(k->ne[2] > 0 && k->ne[3] > 0 && H % k->ne[2] == 0 && B3 % k->ne[3] == 0, "flash_attn_ext: heads / batch not broadcastable over k / v");
    NEED(d->ne[0] == Dp && d->ne[1] == H && d->ne[2] == N && d->ne[3] == B3, "flash_attn_ext: dst must be [head_size, n_head, n_q, batch]");
    NEED(d->nb[0] == 4 && d->nb[1] == 4 * Dp && d->nb[2] == d->nb[1] * H && d->nb[3] == d->nb[2] * N, "flash_attn_ext: dst must be contiguous");
    NEED(q->nb[0] == 4 && (kvq || (k->nb[0] == 2 && v->nb[0] == 2)), "flash_attn_ext: rows must be contiguous");
    NEED(!(((uintptr_t)k->data | (uintptr_t)v->data | (uintptr_t)d->data | (uintptr_t)k->nb[1] | (uintptr_t)k->nb[2] | (uintptr_t)k->nb[3] |
            (uintptr_t)v->nb[1] | (uintptr_t)v->nb[2] | (uintptr_t)v->nb[3]) & (kvq ? 3 : 15)) && !((uintptr_t)d->data & 15), "flash_attn_ext: k / v rows and dst must be 16-byte aligned");
    NEED(!(((uintptr_t)q->data | (uintptr_t)q->nb[1] | (uintptr_t)q->nb[2] | (uintptr_t)q->nb[3]) & 3), "flash_attn_ext: q must be 4-byte aligned");
    if (mask) {
        NEED(mask->type == CDNA4_F16 && mask->nb[0] == 2 && mask->ne[0] == KV && mask->ne[1] >= N && mask->ne[2] == 1 && mask->ne[3] == 1, "flash_attn_ext: mask must be F16 [n_kv, >= n_q]");
    } else NEED(max_bias == 0.0f, "flash_attn_ext: ALiBi needs a mask");
    if (N <= 0 || H <= 0 || B3 <= 0) return 0;
    NEED(KV > 0, "flash_attn_ext: no keys");
    NEED(H <= 65535 && B3 <= 65535, "flash_attn_ext: too many heads / batches for one grid");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 2; i++) {
        if (!staged[i]) continue;
        const T4 *src = i ? v_in : k_in; const size_t bytes = (size_t)(Dp * src->ne[1] * src->ne[2] * src->ne[3]) * 2;
        NEED(kv[i].data = cdna4_gemm_scratch(bytes + 256, 5 + i), "flash_attn_ext: cannot allocate the fp16 copy of k / v");
        if (pad && hipMemsetAsync(kv[i].data, 0, bytes, st) != hipSuccess) { (void)hipGetLastError(); return cdna4_set_error_msg("flash_attn_ext: memset failed"); }
        T4 c = kv[i]; c.ne[0] = D;                                     // head_size columns of rows Dp halves apart
        if (const int rc = src->type == CDNA4_F16 ? ggml_cdna4_op_cpy(src, &c, 0, stream) : cdna4_launch_to_f16_dense(src, kv[i].data, Dp, st)) return rc;
    }
    if (pad) {
        const size_t nel = (size_t)(Dp * N * H * B3);
        qq.data = cdna4_gemm_scratch(nel * 4 + 256, 7); dd.data = cdna4_gemm_scratch(nel * 4 + 256, 8);
        NEED(qq.data && dd.data, "flash_attn_ext: cannot allocate the padded q / dst");
        if (hipMemsetAsync(qq.data, 0, nel * 4, st) != hipSuccess) { (void)hipGetLastError(); return cdna4_set_error_msg("flash_attn_ext: memset failed"); }
        T4 c = qq; c.ne[0] = D;
        if (const int rc = ggml_cdna4_op_cpy(q_in, &c, 0, stream)) return rc;
    }
    const int rc = fa_run(pl, q, k, v, mask, d, scale, max_bias, logit_softcap, st);
    if (rc || !pad) return rc;
    T4 view = dd; view.ne[0] = D;                                      // the first head_size columns of every padded output row
    return ggml_cdna4_op_cpy(&view, d_in, 0, stream);
}
