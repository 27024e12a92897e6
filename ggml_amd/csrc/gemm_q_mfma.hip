// gemm_q_mfma.hip — batched prefill path: Y[b][m] = sum_k W[m][k] * X[b][k], W block-quantized, on the
// gfx950 matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate).
//
// Numerics ("parity mode"): X has already been quantized exactly like the reference CPU
// backend quantizes src1 (Q8_K / Q8_0, quantize_act.hip) and dequantized to fp16; weights are dequantized
// block-wise to fp16 with the reference formulas (dequantize_row_q4_K etc., src/ggml-quants.c:255,349,1280,
// 1482,1690).  Measured rel-L2 vs ggml-cpu ~3e-4 (gate 1e-3); vs the exact product it is ~4e-3 like the CPU.
//
// Structure (MI355X-first, not a port of src/ggml-cuda/mmq.cuh) — common to every kernel in this file:
//  * a wave owns 32 (or 64) weight rows for ALL activation rows of the tile, so every weight of the tile is dequantized by
//    exactly one lane, in registers, straight into the MFMA B operand — weights never exist as fp16 in LDS or HBM;
//  * k is consumed in a permuted order: MFMA A and B fragments only need to agree on which k each slot holds, so the
//    nibble unpack needs no byte shuffles (see chunk_of() and the pair-interleaved, k-panel-major fp16 image);
//  * packed weights and fp16 activations are staged through a 3-slot LDS ring (global_load_lds_dwordx4, 16-byte chunks
//    XOR-swizzled on the SOURCE address so the fragment ds_read_b128s are conflict-free); XCD-aware tile order.
// Kernels, oldest to newest (gemm_q_make_plan() picks; DESIGN.md 4.3 has the measurements):
//    k_gemm_q        4 waves, slice-per-barrier, per-lane weight loads, 128-wide activation tile — any format; K % 256 != 0, and (IDS) the grouped MUL_MAT_ID of Q5_K / Q6_K / Q4_0 / Q8_0
//    k_gemm_kq_w8    8 waves (two per SIMD), 128x128 tile, in-wave unpack/MFMA pipeline, split-K = 2 exchange — the shallow-K (< 3 superblocks per work-group) form of the next two
//    k_gemm_kq_w8p   + cross-stage software pipeline (barrier in the middle of the MFMA stream)   (Q5_K default)
//    k_gemm_kq_w12   + four LDS-DMA loader waves; they also re-lay Q4_0 / Q8_0 / Q6_K blocks while staging (Q4_K default)
//    (huge grids: k_gemm_kq_t64<.., 256> of gemm_q_t64.hip)
//    k_repack_*      16-byte-aligned re-layout of Q4_0 / Q8_0 / Q6_K into scratch (shallow-K fallback of the staged path)
#include "gemm_q_common.h"
#include "gemm_q_plan.hpp"
#include "mul_mat_id_plan.hpp"
#include "cdna4_formats.hpp"
#include <atomic>
#include <mutex>
#include "gemm_q_hw.h"
#include "quantize_dev.h"
#include "epilogue.h"

// repack kernels: one thread per 16-byte OUTPUT piece (coalesced stores; the 2-byte-aligned source bytes of a superblock
// are read by the 9 / 17 / 14 adjacent threads that build it)
__device__ __forceinline__ u32x4 ld16_a2(const uint8_t *p) { return u32x4{ld_u32_a2(p), ld_u32_a2(p + 4), ld_u32_a2(p + 8), ld_u32_a2(p + 12)}; }
__device__ __forceinline__ u32x4 fp16_d8(const uint8_t *src, int bstride) {           // the 8 block scales of a superblock
    uint32_t d[4];
#pragma unroll
    for (int b = 0; b < 4; b++) d[b] = (uint32_t)ld_u16(src + (2 * b) * bstride) | ((uint32_t)ld_u16(src + (2 * b + 1) * bstride) << 16);
    return u32x4{d[0], d[1], d[2], d[3]};
}
__global__ __launch_bounds__(256) void k_repack_q4_0(const uint8_t *__restrict__ W, int64_t w_row_bytes, int M, int nsb, uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)M * nsb * 9) return;
    const int pc = (int)(t % 9); const int64_t u = t / 9;
    const int row = (int)(u / nsb), sb = (int)(u % nsb);
    const uint8_t *src = W + (int64_t)row * w_row_bytes + (int64_t)sb * 8 * 18;
    u32x4 o;
    if (pc == 0) o = fp16_d8(src, 18);
    else {                                                             // piece (g, e): byte l = 16e + i of group g: low = blk 2g weight l, high = blk 2g+1 weight l
        const int g = (pc - 1) >> 1, e = (pc - 1) & 1;
        const u32x4 a = ld16_a2(src + (2 * g) * 18 + 2), c = ld16_a2(src + (2 * g + 1) * 18 + 2);
        const int sh = 4 * e;                                           // weights 0..15 = low nibbles, 16..31 = high nibbles of the 16 bytes
        o.x = ((a.x >> sh) & 0x0F0F0F0Fu) | (((c.x >> sh) & 0x0F0F0F0Fu) << 4); o.y = ((a.y >> sh) & 0x0F0F0F0Fu) | (((c.y >> sh) & 0x0F0F0F0Fu) << 4);
        o.z = ((a.z >> sh) & 0x0F0F0F0Fu) | (((c.z >> sh) & 0x0F0F0F0Fu) << 4); o.w = ((a.w >> sh) & 0x0F0F0F0Fu) | (((c.w >> sh) & 0x0F0F0F0Fu) << 4);
    }
    reinterpret_cast<u32x4 *>(out)[t] = o;
}
__global__ __launch_bounds__(256) void k_repack_q8_0(const uint8_t *__restrict__ W, int64_t w_row_bytes, int M, int nsb, uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)M * nsb * 17) return;
    const int pc = (int)(t % 17); const int64_t u = t / 17;
    const int row = (int)(u / nsb), sb = (int)(u % nsb);
    const uint8_t *src = W + (int64_t)row * w_row_bytes + (int64_t)sb * 8 * 34;
    reinterpret_cast<u32x4 *>(out)[t] = pc == 0 ? fp16_d8(src, 34) : ld16_a2(src + ((pc - 1) >> 1) * 34 + 2 + 16 * ((pc - 1) & 1));
}
__global__ __launch_bounds__(256) void k_repack_q6_K(const uint8_t *__restrict__ W, int64_t w_row_bytes, int M, int nsb, uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)M * nsb * 14) return;
    const int pc = (int)(t % 14); const int64_t u = t / 14;
    const int row = (int)(u / nsb), sb = (int)(u % nsb);
    const uint8_t *src = W + (int64_t)row * w_row_bytes + (int64_t)sb * 210;       // ql[128] qh[64] scales[16] d
    reinterpret_cast<u32x4 *>(out)[t] = pc == 0 ? u32x4{(uint32_t)ld_u16(src + 208), 0u, 0u, 0u} : (pc == 1 ? ld16_a2(src + 192) : ld16_a2(src + 16 * (pc - 2)));
}

// Q6_K -> Q6_K8 (cdna4_common.h; resident images only): piece 0 / 1 = the sixteen fp16 scales fp16(d * scales[i]), pieces 2 .. 17 = sixteen weights each, q - 32 as int8,
// in k order (weight 128 n + 32 quad + l: ql[64 n + 32 (quad & 1) + l] low / high nibble for quad < 2 / >= 2, bits 2 quad .. 2 quad + 1 of qh[32 n + l] — dequantize_row_q6_K,
// /root/reference/src/ggml-quants.c:1610-1640)
__global__ __launch_bounds__(256) void k_repack_q6_K8(const uint8_t *__restrict__ W, int64_t w_row_bytes, int M, int nsb, uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)M * nsb * 18) return;
    const int pc = (int)(t % 18); const int64_t u = t / 18;
    const int row = (int)(u / nsb), sb = (int)(u % nsb);
    const uint8_t *src = W + (int64_t)row * w_row_bytes + (int64_t)sb * 210;       // ql[128] qh[64] scales[16] d
    uint32_t o[4];
    if (pc < 2) {
        const float d = h2f(ld_u16(src + 208));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const half_t a = (half_t)(d * (float)(int8_t)src[192 + 8 * pc + 2 * i]), b = (half_t)(d * (float)(int8_t)src[192 + 8 * pc + 2 * i + 1]);
            o[i] = (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
        }
    } else {
        const int w0 = 16 * (pc - 2), n = w0 >> 7, quad = (w0 >> 5) & 3, l0 = w0 & 31;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int l = l0 + 4 * i + b;
                const uint32_t ql = src[64 * n + 32 * (quad & 1) + l], qh = src[128 + 32 * n + l];
                const int q = (int)(((quad < 2 ? ql : ql >> 4) & 0xFu) | (((qh >> (2 * quad)) & 3u) << 4)) - 32;
                v |= ((uint32_t)q & 0xFFu) << (8 * b);
            }
            o[i] = v;
        }
    }
    reinterpret_cast<u32x4 *>(out)[t] = u32x4{o[0], o[1], o[2], o[3]};
}

// ------------------------------------------------------------------------------------------------------------
void *cdna4_debug_trace = nullptr;   // profiling hook (ggml_cdna4_debug_trace): device buffer for k_gemm_kq_w8<.., true>


// IDS: the grouped MUL_MAT_ID form (see gemm_params: tile_expert / row_dst / w_expert_bytes) — activation tile tile_b of the expert-sorted image
// multiplies by expert tile_expert[tile_b]'s matrix, unused tiles exit, the store scatters through row_dst.  Serves the formats whose
// 128 x 128 LDS-DMA kernels have no grouped form yet (Q5_K / Q6_K / Q4_0 / Q8_0: per-lane loads of the ORIGINAL blocks, no re-layout).
template <int TYPE, int BNF, bool WLDS, bool IDS = false>
__global__ __launch_bounds__(256) void k_gemm_q(const gemm_params p) {
    constexpr int TB = 32 * BNF;                 // activation rows per tile
    constexpr int XS = TB * 128;                 // bytes of one X stage: TB rows x 64 halves
    constexpr int BLK = QT<TYPE>::BYTES;
    constexpr int WS = WLDS ? 128 * BLK : 0;     // bytes of one staged weight superblock panel (128 rows)
    constexpr int NP = BLK / 16;                 // 16-byte pieces per superblock (LDS path only)
    static_assert(!WLDS || (BLK % 16 == 0 && QT<TYPE>::KQ), "LDS weight staging needs 16-byte aligned superblocks");
    __shared__ __attribute__((aligned(16))) uint8_t smem[2 * XS + 2 * WS + 16];
    uint8_t *const Xs = smem, *const Ws = smem + 2 * XS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    // XCD-aware order: consecutive logical ids share the weight row-panel; blocks are dealt round-robin to the
    // 8 XCDs, so give each XCD a contiguous run of logical ids.
    const int nblk = gridDim.x;
    int L = blockIdx.x;
    if ((nblk & 7) == 0) L = (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3);
    const int tile_b = L % p.tiles_b; L /= p.tiles_b;
    const int ks = L % p.splitk, tile_m = L / p.splitk;
    const int m0 = tile_m * 128, b0 = tile_b * TB;
    const int ksteps = p.K / 64 / p.splitk;      // 64-k slices handled by this block
    const int kstep0 = ks * ksteps;

    int64_t wexp = 0;                                                   // byte offset of this tile's expert matrix
    if constexpr (IDS) {
        const int e = p.tile_expert[tile_b];
        if (e < 0) return;                                              // (work-group-uniform, before any barrier)
        wexp = (int64_t)e * p.w_expert_bytes;
    }
    const int mrow = min(m0 + wave * 32 + j, p.M - 1);
    const uint8_t *const wrow = p.W + wexp + (int64_t)mrow * p.w_row_bytes;

    floatx16 acc[BNF];
#pragma unroll
    for (int i = 0; i < BNF; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;

    // ---- staging helpers -------------------------------------------------------------------------------
    auto stage_x = [&](int step, int buf) {
        const int k0 = (kstep0 + step) * 64;
#pragma unroll
        for (int i = 0; i < BNF; i++) {
            const int pc = i * 256 + tid, row = pc >> 3, c = (pc & 7) ^ ((row >> 1) & 7);
            const int b = min(b0 + row, p.B - 1);
            glds16(p.xh + ((int64_t)(k0 >> 7) * p.B + b) * 128 + (k0 & 127) + c * 8, Xs + buf * XS + (i * 256 + wave * 64) * 16);
        }
    };
    auto stage_w = [&](int sb, int buf) {           // LDS path: the 128-row panel of superblock sb
        if (WLDS) {
#pragma unroll
            for (int i = 0; i < (2 * NP + 3) / 4; i++) {
                const int idx = wave + 4 * i;
                if (idx < 2 * NP) {
                    const int pc = idx * 64 + lane, row = pc / NP, c = pc % NP;
                    const int m = min(m0 + row, p.M - 1);
                    glds16(p.W + wexp + (int64_t)m * p.w_row_bytes + (int64_t)sb * BLK + c * 16, Ws + buf * WS + idx * 1024);
                }
            }
        }
    };

    const int xrow_off = j * 128, xswz = (j >> 1) & 7;
    auto compute = [&](const Raw<TYPE> &raw, int gsel, int buf) {
        half8_t wf[4];
        raw.frags(gsel, h, wf);
        const uint8_t *xs = Xs + buf * XS + xrow_off;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int coff = (chunk_of<TYPE>(kk, h) ^ xswz) << 4;
#pragma unroll
            for (int bf = 0; bf < BNF; bf++) {
                const half8_t xa = *reinterpret_cast<const half8_t *>(xs + bf * 32 * 128 + coff);
                acc[bf] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, wf[kk], acc[bf], 0, 0, 0);
            }
        }
    };

    // ---- main loop -------------------------------------------------------------------------------------
    if (QT<TYPE>::KQ) {
        const int sb0 = kstep0 >> 2, nsb = ksteps >> 2;
        stage_x(0, 0);
        stage_w(sb0, 0);
        CDNA4_WAIT_VM(0);
        __syncthreads();
        for (int s = 0; s < nsb; s++) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int step = 4 * s + g;
                if (step + 1 < ksteps) stage_x(step + 1, (step + 1) & 1);
                if (g == 0 && s + 1 < nsb) stage_w(sb0 + s + 1, (s + 1) & 1);
                Raw<TYPE> raw;
                if (WLDS) raw.load(Ws + (s & 1) * WS + (wave * 32 + j) * BLK, g, h);
                else raw.load(wrow + (int64_t)(sb0 + s) * BLK, g, h);
                compute(raw, g, step & 1);
                CDNA4_WAIT_VM(0);
                __syncthreads();
            }
        }
    } else {
        stage_x(0, 0);
        CDNA4_WAIT_VM(0);
        __syncthreads();
        for (int step = 0; step < ksteps; step++) {
            if (step + 1 < ksteps) stage_x(step + 1, (step + 1) & 1);
            Raw<TYPE> raw;
            raw.load(wrow + (int64_t)(2 * (kstep0 + step) + h) * BLK, 0, h);
            compute(raw, 0, step & 1);
            CDNA4_WAIT_VM(0);
            __syncthreads();
        }
    }

    // ---- epilogue: D[i][jcol]: lane holds column jcol = j (weight row m), rows i = (r&3) + 8*(r>>2) + 4*h ----
    const int m = m0 + wave * 32 + j;
    if (m < p.M) {
#pragma unroll
        for (int bf = 0; bf < BNF; bf++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int b = b0 + bf * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if constexpr (IDS) {                                    // image row -> (token, slot) output row; padding rows are not stored
                    const int pr = b < p.B ? p.row_dst[b] : -1;
                    if (pr >= 0) p.Y[(int64_t)pr * p.y_row + m] = acc[bf][r];
                } else if (b < p.B) {
                    float *dst = p.Y + (int64_t)b * p.y_row + m;
                    if (p.splitk > 1) unsafeAtomicAdd(dst, acc[bf][r]); else *dst = acc[bf][r];
                }
            }
    }
}


#include "gemm_kq_w8.inc"

#include "gemm_kq_w12.inc"

__global__ void k_zero_rows(float *Y, int64_t y_row, int M, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)M * B) Y[(i / M) * y_row + (i % M)] = 0.f;
}

bool cdna4_gemm_q_supported(int type, int64_t M, int64_t K, int64_t B) {
    if (M <= 0 || B <= 0) return false;
    switch (type) {
        case CDNA4_Q4_K: case CDNA4_Q5_K: case CDNA4_Q6_K: return K > 0 && K % 256 == 0;
        case CDNA4_Q4_0: case CDNA4_Q8_0: return K > 0 && K % 64 == 0;
        case CDNA4_Q5_0: case CDNA4_IQ4_NL: return K > 0 && K % 64 == 0;        // as Q8_0, after the exact re-encoding of convert_w.hip
        case CDNA4_Q4_1: case CDNA4_Q5_1: return K > 0 && K % 128 == 0;        // as Q8_0 with 2 K columns ([d q | m 1]) against a doubled activation image: whole 128-k panels
        case CDNA4_Q3_K: case CDNA4_Q2_K: return K > 0 && K % 256 == 0;     // as Q6_K (Q2_K: 2 K columns against a doubled activation image)
        // IQ4_XS has the same two-part form ([h part | l part], convert_w.hip).  Round 3 kept it off the GEMM by default because ~1 % of its outputs
        // differed between identical calls on MI355X; round 4 found the cause in the RE-ENCODING, not the GEMM: hipcc had reused the address VGPRs
        // of global loads still in flight (partial vmcnt waits) and the hardware then returned wrong bytes for the later loads (the
        // emulator cannot see it).  k_convert_iq4_xs_q6_K2 now waits for all four loads before the first use; byte-exact and bit-stable over 200
        // repeats on hardware (tests/test_gpu_widening.py).  CDNA4_IQ4_XS_GEMM=0 keeps every batch size on the int8-dot GEMV units.
        case CDNA4_IQ4_XS: { static const bool off = getenv("CDNA4_IQ4_XS_GEMM") && atoi(getenv("CDNA4_IQ4_XS_GEMM")) == 0; return !off && K > 0 && K % 256 == 0; }
    }
    return false;
}

template <int TYPE, int BNF, bool WLDS>
static int launch_variant(const cdna4_gemm_args &a, int splitk, hipStream_t st) {
    gemm_params p{}; p.trace = nullptr; p.partial = nullptr; p.flags = nullptr; p.sb_split = 0;
    p.W = a.W; p.w_row_bytes = a.w_row_bytes; p.xh = (const half_t *)a.xh; p.xh_row = a.xh_row_elems;
    p.Y = a.Y; p.y_row = a.y_row_elems; p.M = a.M; p.K = a.K; p.B = a.B; p.splitk = splitk;
    p.tiles_m = (a.M + 127) / 128; p.tiles_b = (a.B + 32 * BNF - 1) / (32 * BNF);
    if (splitk > 1) {
        const int64_t n = (int64_t)a.M * a.B;
        hipLaunchKernelGGL(k_zero_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.Y, a.y_row_elems, a.M, a.B);
    }
    hipLaunchKernelGGL((k_gemm_q<TYPE, BNF, WLDS>), dim3(p.tiles_m * p.tiles_b * splitk), dim3(256), 0, st, p);
    CDNA4_CHECK_LAUNCH();
    return 0;
}

// library-owned scratch for the split-K hand-off (partial tiles + flags), grown on demand like a BLAS workspace
// (one region per device; launches that use it are assumed to be stream-ordered on that device, as the plug-in's
// single-stream backend and the one-process-per-GPU bench are).
static void *g_scratch[192] = {nullptr}; static size_t g_scratch_bytes[192] = {0};
static std::mutex g_scratch_mu;                                     // the bookkeeping below, against host threads driving different devices; USE of an area stays stream-ordered per device
static std::atomic<uint64_t> g_scratch_generation{0};
uint64_t cdna4_scratch_generation() { return g_scratch_generation.load(); }
static void *get_scratch(size_t bytes, int kind = 0) {             // kind 0: split-K exchange buffers, 1: repacked weights, 2: exchange buffers of gemm_q_t64.hip (reader-reset flags), 3: re-encoded weights (convert_w.hip), 4: partial results of the key-split FLASH_ATTN_EXT (fattn.hip), 5 / 6: fp16 copies of a quantized (or head-size-padded) K / V in front of FLASH_ATTN_EXT, 7 / 8: its padded q / dst, 9: split-K exchange of gemm_q_lds.hip, 10: parked partial tiles + tickets of gemm_q_sk.hip, 11: chunk flags of FLASH_ATTN_EXT (fattn.hip: k_fa_mask_flags)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    dev += 16 * kind;
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    if (bytes <= g_scratch_bytes[dev]) return g_scratch[dev];
    g_scratch_generation++;                                          // captured launches hold the old address: see ggml_cdna4_scratch_generation()
    (void)hipDeviceSynchronize();
    if (g_scratch[dev]) (void)hipFree(g_scratch[dev]);
    g_scratch[dev] = nullptr; g_scratch_bytes[dev] = 0;
    const size_t want = (bytes + (4u << 20)) & ~(size_t)((1u << 20) - 1);
    void *ptr = nullptr;
    if (hipMalloc(&ptr, want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemset(ptr, 0, want) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(ptr); return nullptr; }
    // hipMemset runs on the NULL stream and returns at once: the caller's launches go to ITS stream, which need not wait for the NULL stream
    // (torch's side streams, the plug-in's non-blocking stream).  Without this wait the zero fill can land AFTER the first kernel wrote the
    // area — seen on MI355X as a first IQ4_XS prefill call 2e-2 from the oracle (its re-encoded weights partly zeroed), and it would equally
    // clear split-K flags under a running exchange.  Allocation is rare: wait here.
    (void)hipDeviceSynchronize();
    g_scratch[dev] = ptr; g_scratch_bytes[dev] = want;
    return ptr;
}
static int cu_count() {                                            // of the CURRENT device (cached per device)
    static int n[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) {
        // no device (the CPU test suite asking ggml_cdna4_mul_mat_route which kernel a shape would take): CDNA4_ASSUME_CUS names the part to answer for
        (void)hipGetLastError();
        static const int assumed = getenv("CDNA4_ASSUME_CUS") ? atoi(getenv("CDNA4_ASSUME_CUS")) : 1;
        return assumed > 0 ? assumed : 1;
    }
    if (!n[dev]) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev) == hipSuccess) n[dev] = pr.multiProcessorCount; else { (void)hipGetLastError(); n[dev] = 1; } }
    return n[dev];
}

void *cdna4_gemm_scratch(size_t bytes, int kind) { return get_scratch(bytes, kind); }

// ---- resident kernel-native images (round 5; the kernel-library half of the plug-in's CDNA4_Resident buffer type).  The formats that reach the matrix cores through an
// exact re-encoding (Q5_0 / IQ4_NL / Q4_1 / Q5_1 -> Q8_0, Q3_K / Q2_K / IQ4_XS -> Q6_K; convert_w.hip) were re-encoded PER CALL into library scratch (VERDICT r4 item 3,
// ADVICE r3 / r4).  A host that keeps a weight matrix resident can have the image built ONCE (ggml_cdna4_resident_image_register, capi.hip — built twice and compared
// byte for byte, so a re-encoding that is not bit-stable on this device is refused at load time instead of surfacing as a wrong product) and registers (base, image) here;
// every prefill route that needs the re-encoding then finds it by the weight pointer — whole matrices and row slices alike — and launches no conversion.  The reference
// has the same mechanism as a repacking buffer type: src/ggml-cpu/ggml-cpu-aarch64.cpp:4144-4172 (ggml_backend_cpu_aarch64_buffer_set_tensor repacks at load).
#include <map>
#include <shared_mutex>
namespace {
struct resident_entry { size_t bytes; const uint8_t *image; int type; int64_t M, K, row_bytes, image_row_bytes; };
std::map<uintptr_t, resident_entry> g_resident;
std::shared_mutex g_resident_mu;
std::atomic<int> g_resident_n{0};
}
// bytes of one image row: the exact re-encodings of convert_w.hip, and — Q4_0 — the 16-byte-aligned re-layout Q4_0R (eight fp16 scales + 128 bytes of nibbles in Q4_K's order per
// 256 weights: the SAME 144 bytes the source blocks take), which k_gemm_kq_t64 / k_gemm_r8 consume through LDS-DMA like Q4_K (0: no image for this type / K)
size_t cdna4_resident_image_row_bytes(int type, int64_t K) {
    if (type == CDNA4_Q4_0) return (K > 0 && K % 256 == 0) ? (size_t)(K / 256) * 144 : 0;
    if (type == CDNA4_Q8_0) return (K > 0 && K % 256 == 0) ? (size_t)(K / 256) * 272 : 0;          // Q8_0R: eight fp16 scales + the eight blocks' int8 (k_repack_q8_0)
    if (type == CDNA4_Q6_K) return (K > 0 && K % 256 == 0) ? (size_t)(K / 256) * 288 : 0;          // Q6_K8: sixteen fp16 scales (d multiplied in) + 256 int8 (k_repack_q6_K8)
    return K > 0 ? cdna4_convert_weights_bytes(type, 1, K) : 0;
}
// builds the image rows of M rows of W (re-encoding or re-layout) on `st`
int cdna4_resident_build(int type, const uint8_t *W, int64_t w_row_bytes, int64_t M, int64_t K, uint8_t *out, hipStream_t st) {
    if (type == CDNA4_Q4_0 || type == CDNA4_Q8_0 || type == CDNA4_Q6_K) {
        if (K % 256 || M <= 0) return cdna4_set_error_msg("resident_image: Q4_0 / Q8_0 rows must be whole 256-weight groups");
        const int nsb = (int)(K / 256);
        if (type == CDNA4_Q6_K) hipLaunchKernelGGL(k_repack_q6_K8, dim3((unsigned)((M * nsb * 18 + 255) / 256)), dim3(256), 0, st, W, w_row_bytes, (int)M, nsb, out);
        else if (type == CDNA4_Q4_0) hipLaunchKernelGGL(k_repack_q4_0, dim3((unsigned)((M * nsb * 9 + 255) / 256)), dim3(256), 0, st, W, w_row_bytes, (int)M, nsb, out);
        else hipLaunchKernelGGL(k_repack_q8_0, dim3((unsigned)((M * nsb * 17 + 255) / 256)), dim3(256), 0, st, W, w_row_bytes, (int)M, nsb, out);
        CDNA4_CHECK_LAUNCH();
        return 0;
    }
    return cdna4_launch_convert_weights(type, W, w_row_bytes, M, K, out, st);
}
int cdna4_resident_register(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, const void *image) {
    const size_t ib = cdna4_resident_image_row_bytes(type, K);
    if (!W || !image || M <= 0 || ib == 0 || w_row_bytes <= 0) return cdna4_set_error_msg("resident_image: bad arguments");
    std::unique_lock<std::shared_mutex> lock(g_resident_mu);
    g_resident[(uintptr_t)W] = resident_entry{(size_t)(M * w_row_bytes), (const uint8_t *)image, type, M, K, w_row_bytes, (int64_t)ib};
    g_resident_n.store((int)g_resident.size());
    g_scratch_generation++;                                          // a captured launch holds the route (image found or not) and the image's address: see ggml_cdna4_scratch_generation()
    return 0;
}
int cdna4_resident_unregister(const void *W) {
    std::unique_lock<std::shared_mutex> lock(g_resident_mu);
    const size_t n = g_resident.erase((uintptr_t)W);
    g_resident_n.store((int)g_resident.size());
    if (n) g_scratch_generation++;
    return n ? 0 : -1;
}
// the image rows of the M rows that start at W (a registered matrix or a row slice of one), or nullptr
const uint8_t *cdna4_resident_lookup(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K) {
    if (g_resident_n.load(std::memory_order_relaxed) == 0) return nullptr;
    std::shared_lock<std::shared_mutex> lock(g_resident_mu);
    auto it = g_resident.upper_bound((uintptr_t)W);
    if (it == g_resident.begin()) return nullptr;
    --it;
    const resident_entry &e = it->second;
    const uintptr_t off = (uintptr_t)W - it->first;
    if (off >= e.bytes || e.type != type || e.K != K || e.row_bytes != w_row_bytes || off % (uintptr_t)e.row_bytes) return nullptr;
    const int64_t row0 = (int64_t)(off / (uintptr_t)e.row_bytes);
    if (row0 + M > e.M) return nullptr;
    return e.image + row0 * e.image_row_bytes;
}
int cdna4_gemm_cu_count() { return cu_count(); }
// The exchanges that WAIT for a partner work-group (the one-launch step's grid barrier, the hand-off of k_gemm_kq_t64 / the 128 x 128-tile kernels, k_gemm_r8's
// reduce-scatter) are only correct while every work-group of the grid is resident at once — true when the caller owns the device, not when another process or stream holds
// CUs.  Round 6: the DEFAULT is "shared" — AUTO never chooses a waiting exchange: small grids take the ticketed split (the last work-group to arrive sums,
// nobody waits) or no split, the headline step is two launches; the reference's split work never waits on a co-resident block either (its stream-k partials are summed by a
// second launch, src/ggml-cuda/mmq.cuh:2796-2822).  A host that owns the device opts in: ggml_cdna4_set_shared_device(0) / GGML_CDNA4_OWNED_DEVICE=1 (bench.py does, and says
// so) — measured worth 1-2 % at the headline shape.  And a wait that runs into its bound is no longer silent: the work-group poisons its tile (NaN) AND sets the fault
// word below; the next ggml_cdna4_mul_mat* call / the plug-in's next graph_compute returns an error status, and the library switches itself to the shared mode.
static std::atomic<int> g_shared_device{-1};
int cdna4_gemm_shared_device() {
    int v = g_shared_device.load(std::memory_order_relaxed);
    if (v < 0) {
        v = 1;
        if (getenv("GGML_CDNA4_OWNED_DEVICE") && atoi(getenv("GGML_CDNA4_OWNED_DEVICE")) != 0) v = 0;
        if (getenv("GGML_CDNA4_SHARED_DEVICE")) v = atoi(getenv("GGML_CDNA4_SHARED_DEVICE")) != 0 ? 1 : 0;     // (the older knob, either way)
        g_shared_device.store(v, std::memory_order_relaxed);
    }
    return v;
}
int cdna4_gemm_set_shared_device(int shared) {
    const int old = cdna4_gemm_shared_device();
    g_shared_device.store(shared ? 1 : 0, std::memory_order_relaxed);
    if (old != (shared ? 1 : 0)) g_scratch_generation++;              // (the routes change: a host replaying captured launches re-captures)
    return old;
}
int cdna4_gemm_coresident_cus() { return cdna4_gemm_shared_device() ? 0 : cu_count(); }
// the fault word: four bytes of pinned, device-mapped host memory (portable: every device writes the same word); the kernels store to it at system scope, the host reads it
// like any variable.  nullptr where the allocation fails (the kernels then only poison their tile, as before).
static std::atomic<unsigned *> g_fault_host{nullptr};
static std::mutex g_fault_mu;
unsigned *cdna4_gemm_fault_word() {
    unsigned *h = g_fault_host.load(std::memory_order_acquire);
    if (!h) {
        std::lock_guard<std::mutex> lock(g_fault_mu);
        h = g_fault_host.load(std::memory_order_relaxed);
        if (!h) {
            void *ptr = nullptr;
            if (hipHostMalloc(&ptr, 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            for (int i = 0; i < 16; i++) ((volatile unsigned *)ptr)[i] = 0u;
            h = (unsigned *)ptr; g_fault_host.store(h, std::memory_order_release);
        }
    }
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (unsigned *)d;
}
int cdna4_gemm_take_fault(bool clear) {
    unsigned *h = g_fault_host.load(std::memory_order_acquire);
    if (!h) return 0;
    const unsigned v = clear ? __atomic_exchange_n(h, 0u, __ATOMIC_ACQ_REL) : __atomic_load_n(h, __ATOMIC_ACQUIRE);
    if (v && g_shared_device.exchange(1, std::memory_order_relaxed) != 1) g_scratch_generation++;      // never again on this process: the device is evidently not ours alone (captured launches hold the old routes: ggml_cdna4_scratch_generation moves)
    return (int)v;
}
static int co_cus() { return cdna4_gemm_coresident_cus(); }

// ---- The routing plan (gemm_q_plan.hpp; ADVICE r3: the tail predictor must not be a hand-kept copy of the routing): gemm_q_make_plan() below decides, side-effect free, which
// kernel a call takes, where its weights come from and the terminal's launch parameters; cdna4_launch_gemm_q() executes that plan, the queries read its fields.
// kernel ids (ggml_cdna4_mul_mat_route, include/ggml_cdna4.h): 10 k_gemm_kq_t64, 12 k_gemm_r8, 13 the 128 x 128-tile kernels (k_gemm_kq_w8 / _w8p / _w12), 14 the older per-lane-load
// kernel (k_gemm_q)

// experiment bits of k_gemm_kq_w12 (variant bits 16+), built in -DCDNA4_ABLATIONS libraries (tools/microbench) only: 1 = early table read (bit-identical, measured: no gain),
// 16.. = timing-only ablations
#ifdef CDNA4_ABLATIONS
#define W12_EXPS(X) X(1) X(2) X(4) X(6) X(16) X(32) X(64) X(128) X(256) X(96) X(224) X(480) X(288) X(512) X(544) X(992)
#else
#define W12_EXPS(X)
#endif
static bool w12_exp_built(int exp) {
#define W12_CASE(E) case E:
    switch (exp) { case 0: W12_EXPS(W12_CASE) return true; default: return false; }
#undef W12_CASE
}

// the 128 x 128-tile kernels on `type` (the kernel's own format: 100.. re-laid, 200.. staged): split, exchange and schedule for the chosen splitk / opt (65 k_gemm_kq_w12,
// 64 k_gemm_kq_w8p, else the schedule option of k_gemm_kq_w8).  a.splitk is the CALLER's (also behind a re-encoding): AUTO or explicit
static const char *w8_make_plan(int type, const cdna4_gemm_args &a, int splitk, int opt, int exp, w8_plan &w) {
    const int tiles_b = (a.B + 127) / 128, ntiles = ((a.M + 127) / 128) * tiles_b, total = a.K / 256;
    // split in two: AUTO (a.splitk <= 0) takes the TICKETED sum of gemm_w8_epilogue.inc (the last of a tile's two work-groups adds both partial tiles; nobody
    // waits, no co-residency assumed — round 4); an explicit splitk = 2 keeps the spinning hand-off where both halves of every tile are resident at once, and
    // falls back to a zero fill + fp32 atomics otherwise
    static const bool handoff_env = getenv("CDNA4_W8_HANDOFF") && atoi(getenv("CDNA4_W8_HANDOFF")) != 0;     // (A/B: the spinning hand-off for AUTO splits too)
    w.type = type; w.splitk = splitk; w.exp = exp; w.sb_split = 0; w.xchg_l2 = 0;
    w.ticketed = splitk == 2 && a.splitk <= 0 && (size_t)ntiles <= 8192 && !handoff_env;
    w.exchange = w.ticketed || (splitk == 2 && ntiles * 2 <= co_cus());
    if (w.exchange) {
        // the exchange is symmetric (each work-group exports half of its partial tile and finishes the other half): even split, the odd superblock to ks = 0
        const int split = (total + 1) / 2;
        w.sb_split = split < 1 ? 1 : (split > total - 1 ? total - 1 : split);
        // both work-groups of a tile share an XCD iff the XCD-aware remap is active (grid % 8 == 0) and each XCD's slice of the
        // tile order holds whole (tile_b x ks) groups; work-groups go to XCDs round-robin by blockIdx (the kernel verifies it)
        const int nb = ntiles * splitk;
        w.xchg_l2 = ((nb & 7) == 0 && ((nb >> 3) % (tiles_b * 2)) == 0) ? 1 : 0;
    }
    // the cross-stage pipeline is written for K ranges of >= 3 superblocks per work-group; shallower ones take schedule 20
    const int min_nsb = w.exchange ? (w.sb_split < total - w.sb_split ? w.sb_split : total - w.sb_split) : total / splitk;
    w.opt = ((opt == 64 || opt == 65) && min_nsb < 3) ? 20 : opt;
    // (what a type cannot reach is not instantiated: the re-laid formats (100..) never take the loader-wave kernel, the staged ones (200..) take nothing else — round 5: 9 kernels)
    if (type >= 100 && type < 200) { if (w.opt == 65) return "gemm_q: the re-laid formats run on k_gemm_kq_w8p / _w8"; }      // (any other option: k_gemm_kq_w8p, or schedule 20)
    else if (w.opt == 65) { if (type == CDNA4_Q4_K && !w12_exp_built(exp)) return "gemm_q: this k_gemm_kq_w12 experiment is not built"; }
    else if (type >= 200) return "gemm_q: staged formats run on the loader-wave kernel only";
    else if (w.opt != 64 && (w.opt & 31) != 20) return "gemm_q: of the 8-wave in-wave schedules only option 20 is built (variant 663)";
    return nullptr;
}

template <int TYPE>
static int launch_w8(const cdna4_gemm_args &a, const w8_plan &w, hipStream_t st) {
    gemm_params p{};
    p.W = a.W; p.w_row_bytes = a.w_row_bytes; p.xh = (const half_t *)a.xh; p.xh_row = a.xh_row_elems;
    p.Y = a.Y; p.y_row = a.y_row_elems; p.M = a.M; p.K = a.K; p.B = a.B; p.splitk = w.splitk;
    p.tiles_m = (a.M + 127) / 128; p.tiles_b = (a.B + 127) / 128;
    p.sb_split = w.sb_split; p.xchg_l2 = w.xchg_l2;
    const int ntiles = p.tiles_m * p.tiles_b;
    if (w.splitk == 1 || w.exchange) p.epi = a.epi;                       // gemm_w8_epilogue.inc applies it in the tile's store (not on the atomic-sum path)
    if (w.exchange) {
        // exchange slots after a FIXED 64-KB flag area (so that no shape's slots ever overlay another shape's flags).  A flag is
        // non-zero only between its writer's publication and its reader's reset inside one launch: no per-launch state on the
        // host, so the launch is graph-capturable once the scratch exists.
        const size_t pbytes = (size_t)ntiles * 128 * 128 * 4 * (w.ticketed ? 2 : 1), fbytes = 65536;      // hand-off: two half tiles per tile; ticketed: two whole ones
        char *sc = (char *)get_scratch(fbytes + pbytes);
        if (!sc) return cdna4_set_error_msg("gemm_q: cannot allocate split-K scratch");
        p.flags = (unsigned *)sc; p.partial = (float *)(sc + fbytes);
    } else if (w.splitk > 1) {
        const int64_t n = (int64_t)a.M * a.B;
        hipLaunchKernelGGL(k_zero_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.Y, a.y_row_elems, a.M, a.B);
    }
    p.trace = (unsigned long long *)cdna4_debug_trace;
    if (w.exchange && !w.ticketed) p.fault = cdna4_gemm_fault_word();     // (the waiting hand-off)
    p.tune = w.ticketed ? 2 : 0;      // bit1 = the ticketed split (gemm_w8_epilogue.inc); (bit0 = s_setprio 1 for the later-dispatched khalf-1 waves of k_gemm_kq_w8p: measured 26.31 vs 26.33 us, never enabled)
    const dim3 grid(ntiles * w.splitk);
    // (the s_memtime trace instantiations <.., TRACE = true> exist in the -DCDNA4_ABLATIONS library of tools/microbench only)
#ifdef CDNA4_ABLATIONS
#define W8_LAUNCH(O) do { if (p.trace) hipLaunchKernelGGL((k_gemm_kq_w8<TYPE, true, O>), grid, dim3(512), 0, st, p); \
                          else hipLaunchKernelGGL((k_gemm_kq_w8<TYPE, false, O>), grid, dim3(512), 0, st, p); } while (0)
#else
#define W8_LAUNCH(O) hipLaunchKernelGGL((k_gemm_kq_w8<TYPE, false, O>), grid, dim3(512), 0, st, p)
#endif
    // (w8_make_plan refused what is not instantiated for TYPE)
    if constexpr (TYPE < 100 || TYPE >= 200) if (w.opt == 65) {           // + loader waves
        if constexpr (TYPE == CDNA4_Q4_K) {
#define W12_EXP(E) case E: hipLaunchKernelGGL((k_gemm_kq_w12<TYPE, true, E>), grid, dim3(768), 0, st, p); CDNA4_CHECK_LAUNCH(); return 0;
            switch (w.exp) { W12_EXPS(W12_EXP) default: break; }
#undef W12_EXP
        }
        hipLaunchKernelGGL((k_gemm_kq_w12<TYPE, true>), grid, dim3(768), 0, st, p);
        CDNA4_CHECK_LAUNCH(); return 0;
    }
    if constexpr (TYPE < 200) {
        if (w.opt == 64) {                                                // cross-stage pipeline
#ifdef CDNA4_ABLATIONS
            if (p.trace) { hipLaunchKernelGGL((k_gemm_kq_w8p<TYPE, true>), grid, dim3(512), 0, st, p); CDNA4_CHECK_LAUNCH(); return 0; }
#endif
            hipLaunchKernelGGL((k_gemm_kq_w8p<TYPE, false>), grid, dim3(512), 0, st, p);
        } else W8_LAUNCH(20);                                             // the in-wave pipeline with the DMA pieces split over both phases (shallow-K fallback; repacked formats: their only other schedule)
#undef W8_LAUNCH
    }
    CDNA4_CHECK_LAUNCH();
    return 0;
}

static void plan_t64(gemm_q_plan &pl, const cdna4_gemm_args &k, int tm) {
    pl.k = k; pl.terminal = GQ_T64; pl.kernel = 10; pl.tail_in_store = true;
    pl.err = t64_make_plan(k, tm, k.splitk, pl.t64); pl.fuses_quantizer = pl.t64.fq;
}
static void plan_r8(gemm_q_plan &pl, const cdna4_gemm_args &k, int splitk) {
    pl.k = k; pl.terminal = GQ_R8; pl.kernel = 12; pl.tail_in_store = true;
    pl.err = r8_make_plan(k, splitk, pl.r8);
}
static void plan_w8(gemm_q_plan &pl, int type, const cdna4_gemm_args &k, int splitk, int opt, int exp = 0) {
    pl.k = k; pl.terminal = GQ_W8; pl.kernel = 13;
    pl.err = w8_make_plan(type, k, splitk, opt, exp, pl.w8); pl.tail_in_store = splitk == 1 || pl.w8.exchange;
}
// a resident kernel-native re-layout of the caller's rows (Q4_0R / Q8_0R / Q6_K8: cdna4_resident_*), 16-byte aligned: the arguments with it in W's place.  The image's
// activations are not Q4_K's: such a launch never carries the quantizer (xf = nullptr)
static bool resident_relayout(const cdna4_gemm_args &a, int image_type, int block_bytes, gemm_q_plan &pl, cdna4_gemm_args &r) {
    const uint8_t *img = cdna4_resident_lookup(a.type, a.W, a.w_row_bytes, a.M, a.K);
    if (!img || ((uintptr_t)img & 15)) return false;
    r = a; r.type = image_type; r.W = img; r.w_row_bytes = (int64_t)(a.K / 256) * block_bytes; r.xf = nullptr;
    pl.source = GQ_W_RESIDENT; pl.image = img;
    return true;
}

// the plan of a call on one of the five formats with kernels of their own.  registered: a.W are the caller's rows (they may have a resident image); false: re-encoded
// rows (a.W == nullptr: not there yet), which are 16-byte aligned and in no registry
template <int TYPE>
static void plan_type(const cdna4_gemm_args &a, bool registered, gemm_q_plan &pl) {
    constexpr bool CAN_LDS = QT<TYPE>::KQ && (QT<TYPE>::BYTES % 16 == 0);
    // variant (include/ggml_cdna4.h points here under this function's earlier name, launch_type()): bit0 = LDS weight staging (Q4_K/Q5_K only), bit1 = 128-wide activation tile, bit3 = the older
    // slice-per-barrier kernel instead of the pipelined one, bit4 = the 8-wave (two waves per SIMD) 128x128 kernel,
    // bits 5-9 = that kernel's schedule option OPT (see k_gemm_kq_w8; 20 = in-wave pipeline with the DMA pieces split over both phases),
    // bit11 = the cross-stage pipelined k_gemm_kq_w8p (the default),
    // bit12 = k_gemm_kq_w12 = w8p + four loader waves (the default for Q4_K).
    // 0 = auto: widest tile that the batch fills.
    int variant = a.variant;
    // (Q5_K on the loader-wave kernel: 31.0 vs 30.65 us — its larger Raw<> spills 32 B at 168 VGPRs — so it stays on k_gemm_kq_w8p)
    // Every batch the GEMM path is given (B > 8) takes the 128-wide activation tile and the 8-wave kernels: the 64-wide 4-wave kernels
    // put ONE work-group on every eighth CU at M = 4096 and have no K split — measured (Q4_K, MI355X) 31 us at 4096 x 4096 and 94 us
    // at 4096 x 14336 for every B in 9..64 against 21 / 47 us for B = 65 on a mostly empty 128-wide tile.
    if (variant <= 0) variant = 4 | (CAN_LDS ? 1 : 0) | 2 | (CAN_LDS ? (16 | (TYPE == CDNA4_Q4_K ? 4096 : 2048)) : 0);   // cross-stage pipeline; Q4_K: + loader waves (k_gemm_kq_w12: 168 VGPRs without spills only for this format)
    const bool wlds = (variant & 1) && CAN_LDS && ((((uintptr_t)a.W | (uintptr_t)a.w_row_bytes) & 15) == 0);
    const bool wide = (variant & 2) != 0;
    // split-K: K-quants split at superblock granularity, 32-block formats at 64-k slices
    const int kunits = QT<TYPE>::KQ ? a.K / 256 : a.K / 64;
    int splitk = a.splitk;
    bool uneven = false;                            // auto only: hand-off split of an odd superblock count (see below)
    if (splitk <= 0) {
        // auto: at most 2.  Two fp32 contributions added to a zeroed output are order-independent (a+b == b+a), so the
        // result stays deterministic; deeper splits (atomic sums of >2 terms) are opt-in only.
        const int tiles = ((a.M + 127) / 128) * ((a.B + (wide ? 127 : 63)) / (wide ? 128 : 64));
        if (variant & 16) splitk = (tiles * 2 <= cu_count() && kunits % 2 == 0 && kunits >= 4) ? 2 : 1;   // hand-off split: only if co-resident
        else splitk = 1;
        // An ODD number of superblocks — K = 11008 = 43 x 256, BASELINE configs[2] — also takes the hand-off split: its two
        // work-groups get sb_split / total - sb_split superblocks (22 / 21), which the exchange was written for (w8_make_plan:
        // sb_split).  Measured on MI355X (round-1 driver run): rel-L2 7.2e-7 vs the unsplit kernel, 59.7 vs 69.6 us.
        if ((variant & 16) && wlds && QT<TYPE>::KQ && tiles * 2 <= cu_count() && (kunits & 1) && kunits >= 7) { splitk = 2; uneven = true; }
    }
    if constexpr (TYPE == CDNA4_Q4_K) {
        // bit13 = k_gemm_kq_t64 (gemm_q_t64.hip: 64(m) x 128(b) wave tiles); bit14 / bit15 force its 128- / 256-row tile
        if (wlds && (variant & 8192)) return plan_t64(pl, a, (variant & 16384) ? 128 : ((variant & 32768) ? 256 : 0));
        // auto (round 2): k_gemm_kq_t64 for every prefill shape — 128-row tiles (hand-off split-K = 2 while both work-groups of a tile
        // are resident, uneven for odd superblock counts), 256-row tiles once the grid holds two of them per CU.  MI355X, same box, same
        // data: 4096x4096x512 24.25 vs 24.68 us on k_gemm_kq_w12, 4096x11008x512 50.95 vs 52.57, 8192x4096x512 37.1 vs 38.1,
        // 32768x8192x512 (256-row tiles) 239-243 vs 265.
        // auto (round 4): k_gemm_r8 (gemm_r8.inc: 32 x 256 wave tiles, half the unpack VALU per MFMA) where its 256 x 256 tiles fill the chip unsplit — 9-10 % ahead there
        if (wlds && a.variant <= 0 && a.splitk <= 0 && cdna4_gemm_r8_preferred(a)) return plan_r8(pl, a, 1);
        if (wlds && a.variant <= 0 && a.splitk <= 2) return plan_t64(pl, a, 0);      // (deeper, atomic splits: the older kernels below)
    }
    if constexpr (TYPE == CDNA4_Q5_K) {
        // round 4: k_gemm_r8 also unpacks Q5_K (its fifth bits cost 4-5 VALU per half2 pair: the format that gains most from one fragment meeting eight activation
        // fragments) — the same rule as Q4_K: grids of at least one 256 x 256 tile per CU, unsplit
        if (wlds && a.variant <= 0 && a.splitk <= 0 && cdna4_gemm_r8_preferred(a)) return plan_r8(pl, a, 1);
    }
    if (splitk < 1 || (kunits % splitk && !uneven)) { pl.err = "gemm_q: splitk must divide the number of K units"; return; }
    [[maybe_unused]] cdna4_gemm_args r;                                   // the arguments with an image / the re-laid rows in W's place
    if constexpr (TYPE == CDNA4_Q4_0) {
        // round 5: a RESIDENT Q4_0R image of this matrix (cdna4_resident_*: built once by the host / the CDNA4_Resident buffer type) puts Q4_0 on Q4_K's own kernels —
        // k_gemm_r8 where its tiles fill the chip, k_gemm_kq_t64 otherwise (256-row tiles, ticketed / deep splits, the tail in the store) — instead of the staging kernel
        if (registered && a.variant <= 0 && a.splitk <= 2 && a.K % 256 == 0 && resident_relayout(a, CDNA4_Q4_0R, 144, pl, r))
            return (a.splitk <= 0 && cdna4_gemm_r8_preferred(r)) ? plan_r8(pl, r, 1) : plan_t64(pl, r, 0);
    }
    if constexpr (TYPE == CDNA4_Q8_0 || TYPE == CDNA4_Q6_K) {
        // round 5: a resident Q8_0R / Q6_K8 image puts Q8_0 / Q6_K on k_gemm_r8 where its 256 x 256 tiles fill the chip (k_gemm_r8<Q8_0R | Q6_K8>: 64 raw bytes per row and K tile)
        if (registered && a.variant <= 0 && a.splitk <= 0 && a.K % 256 == 0 && resident_relayout(a, TYPE == CDNA4_Q8_0 ? CDNA4_Q8_0R : CDNA4_Q6_K8, TYPE == CDNA4_Q8_0 ? 272 : 288, pl, r)) {
            if (cdna4_gemm_r8_preferred(r)) return plan_r8(pl, r, 1);
            // smaller grids.  For Q4_K k_gemm_r8's co-resident split-K (2 / 4 / 8 work-groups per tile reduce-scatter their partial tiles) is level with or behind
            // k_gemm_kq_t64; Q8_0's alternative is the staging kernel, 35 % behind r8 per tile.  MI355X, one box, alternating, us per call, staging kernel -> r8
            // (profiles/r05/q80_r8_small.txt):   split in 2 (65 .. 128 tiles): 16384 x 8192 x 512 178 -> 139, 14336 x 4096 x 512 91 -> 71, 4096 x 4096 x 2048 103 -> 79;
            // split in 4 / 8 (<= 64 tiles): only long rows pay — 8192 x 8192 x 512 90.6 -> 83.7, 4096 x 14336 x 512 83.3 -> 77.3, but 8192 x 4096 x 512 48.7 -> 53.2,
            // 4096 x 4096 x 1024 49.2 -> 52.7, 4096 x 4096 x 512 31.0 -> 40.2.  One ragged round of at least 65 % of the CUs runs unsplit.
            const int nt256 = ((a.M + 255) / 256) * ((a.B + 255) / 256), cus = cu_count(), co = cdna4_gemm_coresident_cus();
            if (nt256 < cus && nt256 * 20 >= cus * 13) return plan_r8(pl, r, 1);
            if (nt256 * 2 <= co && a.K >= 1024 && (nt256 * 4 > co || a.K >= 8192)) return plan_r8(pl, r, 0);
            pl.source = GQ_W_GIVEN; pl.image = nullptr;                    // (the image goes unused: the routes below read the caller's rows)
        }
    }
    if constexpr (TYPE == CDNA4_Q4_0 || TYPE == CDNA4_Q8_0 || TYPE == CDNA4_Q6_K) {
        // 2-byte-aligned formats at prefill batch sizes, K in whole superblocks.  Preferred: no copy at all — the loader waves of k_gemm_kq_w12 read the original blocks and
        // re-lay them while staging (needs >= 3 superblocks of K per work-group, like the cross-stage pipeline itself).  Otherwise re-lay the weights into 16-byte-aligned
        // superblocks (scratch kind 1, per call: one extra read+write of W, ~5 us at 4096x4096) and run the LDS-DMA pipeline on that — 2.5-3x faster than the per-lane-load
        // kernel below, which stays for small batches and K % 256 != 0.
        constexpr int RT = TYPE == CDNA4_Q4_0 ? CDNA4_Q4_0R : (TYPE == CDNA4_Q8_0 ? CDNA4_Q8_0R : CDNA4_Q6_KR);
        constexpr int ST_ = TYPE == CDNA4_Q4_0 ? CDNA4_Q4_0S : (TYPE == CDNA4_Q8_0 ? CDNA4_Q8_0S : CDNA4_Q6_KS);
        if (a.variant <= 0 && a.K % 256 == 0) {
            // the auto split of both routes: in two where both work-groups of every tile fit the chip and each gets at least two superblocks
            const int nsb = a.K / 256, tiles = ((a.M + 127) / 128) * ((a.B + 127) / 128);
            const int sk = a.splitk > 0 ? a.splitk : ((tiles * 2 <= cu_count() && nsb % 2 == 0 && nsb >= 4) ? 2 : 1);
            if (nsb % sk == 0 && nsb / sk >= 3) return plan_w8(pl, ST_, a, sk, 65);
            if (nsb % sk) { pl.err = "gemm_q: splitk must divide the number of K units"; return; }
            r = a; r.W = nullptr; r.w_row_bytes = (int64_t)nsb * QT<RT>::BYTES;
            pl.source = GQ_W_RELAID;
            return plan_w8(pl, RT, r, sk, 64);
        }
    }
    if constexpr (CAN_LDS) {
        if (wlds && (variant & 16)) return plan_w8(pl, TYPE, a, splitk, (variant & 4096) ? 65 : ((variant & 2048) ? 64 : ((variant >> 5) & 31)), variant >> 16);
    }
    // the older kernel stores the plain product (k_epilogue behind it)
    // (round 5: the 4-wave pipelined k_gemm_kq_pipe and the 64-wide forms of k_gemm_q — explicit variants only since round 2 — are gone; bits 1 and 3 of a variant are ignored)
    pl.k = a; pl.terminal = GQ_KQ; pl.kernel = 14; pl.tail_in_store = false; pl.kq.wlds = wlds; pl.kq.splitk = splitk;
}


// grouped MUL_MAT_ID for Q5_K / Q6_K / Q4_0 / Q8_0: one launch of k_gemm_q<.., IDS> over (m tile) x (128-row activation tile of the expert-sorted
// image); a.B = image rows (a multiple of 128), a.Y rows indexed through row_dst.  (Which calls come here and which go to cdna4_launch_gemm_t64_ids: capi.hip, mmid_make_plan.)
template <int TYPE>
static int launch_ids(const cdna4_gemm_args &a, const int32_t *tile_expert, const int32_t *row_dst, int64_t w_expert_bytes, hipStream_t st) {
    gemm_params p{};
    p.W = a.W; p.w_row_bytes = a.w_row_bytes; p.xh = (const half_t *)a.xh; p.xh_row = a.xh_row_elems;
    p.Y = a.Y; p.y_row = a.y_row_elems; p.M = a.M; p.K = a.K; p.B = a.B; p.splitk = 1;
    p.tiles_m = (a.M + 127) / 128; p.tiles_b = a.B / 128;
    p.tile_expert = tile_expert; p.row_dst = row_dst; p.w_expert_bytes = w_expert_bytes;
    const dim3 grid(p.tiles_m * p.tiles_b);
    if constexpr (QT<TYPE>::KQ && (QT<TYPE>::BYTES % 16 == 0)) { if (cdna4_gemm_ids_wlds(TYPE, a.W, a.w_row_bytes, w_expert_bytes)) { hipLaunchKernelGGL((k_gemm_q<TYPE, 4, true, true>), grid, dim3(256), 0, st, p); CDNA4_CHECK_LAUNCH(); return 0; } }
    hipLaunchKernelGGL((k_gemm_q<TYPE, 4, false, true>), grid, dim3(256), 0, st, p);
    CDNA4_CHECK_LAUNCH();
    return 0;
}
// the expert matrices go through LDS: K-quants with whole 16-byte superblocks (Q4_K, Q5_K), 16-byte aligned
bool cdna4_gemm_ids_wlds(int type, const void *W, int64_t w_row_bytes, int64_t w_expert_bytes) {
    return cdna4_type_is_kq(type) && cdna4_type_bytes(type) % 16 == 0 && !(((uintptr_t)W | (uintptr_t)w_row_bytes | (uintptr_t)w_expert_bytes) & 15);
}
bool cdna4_gemm_ids_supported(int type, int64_t K) {
    const int64_t unit = cdna4_type_is_kq(type) ? 256 : 128;                              // (32-weight formats: whole 128-k panels of the image, whole 64-k slices)
    return cdna4_type_is_main5(type) && K >= unit && K % unit == 0;
}
int cdna4_launch_gemm_ids(const cdna4_gemm_args &a, const int32_t *tile_expert, const int32_t *row_dst, int64_t w_expert_bytes, hipStream_t st) {
    if (!cdna4_gemm_ids_supported(a.type, a.K) || a.B % 128) return cdna4_set_error_msg("gemm_ids: unsupported type / K, or image rows not a multiple of 128");
    if (((uintptr_t)a.xh & 15) || (((uintptr_t)a.W | (uintptr_t)a.w_row_bytes | (uintptr_t)w_expert_bytes) & 1)) return cdna4_set_error_msg("gemm_ids: misaligned operands");
    int rc = 0;
    if (cdna4_dispatch(cdna4_main5{}, a.type, [&](auto t) { rc = launch_ids<t.value>(a, tile_expert, row_dst, w_expert_bytes, st); })) return rc;
    return cdna4_set_error_msg("gemm_ids: unsupported weight type");
}

// the terminals of this file for weights that are (or were re-encoded as) TYPE: the 128 x 128-tile kernels on TYPE itself, on its staged or on its re-laid form, or k_gemm_q
template <int TYPE>
static int launch_planned(const cdna4_gemm_args &k, const gemm_q_plan &pl, hipStream_t st) {
    if (pl.terminal == GQ_W8) {
        if constexpr (TYPE == CDNA4_Q4_0 || TYPE == CDNA4_Q8_0 || TYPE == CDNA4_Q6_K) {
            constexpr int ST_ = TYPE == CDNA4_Q4_0 ? CDNA4_Q4_0S : (TYPE == CDNA4_Q8_0 ? CDNA4_Q8_0S : CDNA4_Q6_KS), RT = TYPE == CDNA4_Q4_0 ? CDNA4_Q4_0R : (TYPE == CDNA4_Q8_0 ? CDNA4_Q8_0R : CDNA4_Q6_KR);
            return pl.w8.type == ST_ ? launch_w8<ST_>(k, pl.w8, st) : launch_w8<RT>(k, pl.w8, st);
        } else return launch_w8<TYPE>(k, pl.w8, st);
    }
    if constexpr (QT<TYPE>::KQ && QT<TYPE>::BYTES % 16 == 0) { if (pl.kq.wlds) return launch_variant<TYPE, 4, true>(k, pl.kq.splitk, st); }
    return launch_variant<TYPE, 4, false>(k, pl.kq.splitk, st);
}

static const char *plan_call(const cdna4_gemm_args &a, gemm_q_plan &pl) {
    if (a.M <= 0 || a.B <= 0) return nullptr;                            // an empty product: nothing to launch
    if (!cdna4_gemm_q_supported(a.type, a.M, a.K, a.B)) return "gemm_q: unsupported type / shape";
    if ((uintptr_t)a.xh & 15) return "gemm_q: activation image must be 16-byte aligned";
    if (((uintptr_t)a.W | (uintptr_t)a.w_row_bytes) & 1) return "gemm_q: weight rows must be 2-byte aligned";
    if ((a.type == CDNA4_Q4_K || a.type == CDNA4_Q5_K) && (((uintptr_t)a.W | (uintptr_t)a.w_row_bytes) & 15)) return "gemm_q: Q4_K/Q5_K rows must be 16-byte aligned";
    if (cdna4_convert_weights_target(a.type) >= 0) {
        // no MFMA kernel of their own: re-encoded EXACTLY as Q8_0 / Q6_K (convert_w.hip) — a resident image built once at load (CDNA4_Resident buffers), or scratch per
        // call — and that format's plan.  Q5_0 / IQ4_NL / Q3_K: same shape.  Q4_1 / Q5_1 (scale part and minimum part side by side), Q2_K (scale part | minimum part) and
        // IQ4_XS (h part | l part): two column blocks, a.xh holds the activation image twice (capi.hip: prepare_act).  a.variant and a.splitk pass through to the target.
        pl.reencoded = true; pl.mid_type = cdna4_convert_weights_target(a.type); pl.kmul = cdna4_convert_weights_kmul(a.type);
        pl.image = cdna4_resident_lookup(a.type, a.W, a.w_row_bytes, a.M, a.K);
        pl.source = pl.image ? GQ_W_RESIDENT : GQ_W_REENCODED;
        cdna4_gemm_args c = a;
        c.type = pl.mid_type; c.W = pl.image; c.K = a.K * pl.kmul; c.xh_row_elems = c.K;
        pl.mid_row_bytes = c.w_row_bytes = c.type == CDNA4_Q8_0 ? (int64_t)(c.K / 32) * 34 : (int64_t)(c.K / 256) * 210;
        if (c.type == CDNA4_Q8_0) plan_type<CDNA4_Q8_0>(c, false, pl); else plan_type<CDNA4_Q6_K>(c, false, pl);
        return pl.err;
    }
    // variant bits 28 + 26 = k_gemm_r8 (gemm_q_lds.hip: in-register unpack, 32 x 256 wave tiles) explicitly (bits 16-24: ablation mask of -DCDNA4_ABLATIONS builds)
    if (a.variant > 0 && (a.variant & (1 << 28))) {
        if (!(a.variant & (1 << 26))) return "gemm_q: variant bit 28 without bit 26 named k_gemm_lds / k_gemm_w4, removed in round 5 (measured losses: profiles/r04/gemm_bench.txt)";
        plan_r8(pl, a, a.splitk);
        return pl.err;
    }
    if (!cdna4_dispatch(cdna4_main5{}, a.type, [&](auto t) { plan_type<t.value>(a, true, pl); })) return "gemm_q: unsupported weight type";
    return pl.err;
}
gemm_q_plan gemm_q_make_plan(const cdna4_gemm_args &a) {
    gemm_q_plan pl{};
    pl.source = GQ_W_GIVEN; pl.mid_type = a.type; pl.mid_row_bytes = a.w_row_bytes; pl.kmul = 1; pl.k = a;
    pl.err = plan_call(a, pl);
    if (pl.err) { pl.kernel = 0; pl.tail_in_store = pl.fuses_quantizer = false; }      // (a refused call: the queries answer "none")
    return pl;
}
// the three questions about the route cdna4_launch_gemm_q() takes for these arguments, read from its plan: does the kernel apply a.epi in its store, does it quantize a.xf
// itself, and which kernel is it (gemm_q_route_id: the ids above; + 100 behind an exact re-encoding; 11: k_gemm_kq_t64 with the quantizer inside; 0: none / refused)?
bool cdna4_gemm_q_fuses_quantizer(const cdna4_gemm_args &a) { return gemm_q_make_plan(a).fuses_quantizer; }
bool cdna4_gemm_q_fuses_tail(const cdna4_gemm_args &a) { return gemm_q_make_plan(a).tail_in_store; }
int cdna4_gemm_q_route(const cdna4_gemm_args &a) { return gemm_q_route_id(gemm_q_make_plan(a)); }

int cdna4_launch_gemm_q(const cdna4_gemm_args &a, hipStream_t st) {
    const gemm_q_plan pl = gemm_q_make_plan(a);
    if (pl.err) return cdna4_set_error_msg(pl.err);
    if (pl.terminal == GQ_NONE) return 0;
    const uint8_t *rows = pl.image ? pl.image : a.W;
    if (pl.reencoded && !pl.image) {
        uint8_t *cw = (uint8_t *)get_scratch(cdna4_convert_weights_bytes(a.type, a.M, a.K) + 256, 3);
        if (!cw) return cdna4_set_error_msg("gemm_q: cannot allocate the weight re-encoding scratch");
        if (const int rc = cdna4_launch_convert_weights(a.type, a.W, a.w_row_bytes, a.M, a.K, cw, st)) return rc;
        rows = cw;
    }
    if (pl.source == GQ_W_RELAID) {                                      // rows of mid_type -> 16-byte-aligned superblocks
        const int nsb = pl.k.K / 256;
        uint8_t *rw = (uint8_t *)get_scratch((size_t)a.M * pl.k.w_row_bytes + 256, 1);
        if (!rw) return cdna4_set_error_msg("gemm_q: cannot allocate the repack scratch");
        const dim3 grid((unsigned)(((int64_t)a.M * (pl.k.w_row_bytes / 16) + 255) / 256));
        if (pl.mid_type == CDNA4_Q4_0) hipLaunchKernelGGL(k_repack_q4_0, grid, dim3(256), 0, st, rows, pl.mid_row_bytes, a.M, nsb, rw);
        else if (pl.mid_type == CDNA4_Q8_0) hipLaunchKernelGGL(k_repack_q8_0, grid, dim3(256), 0, st, rows, pl.mid_row_bytes, a.M, nsb, rw);
        else hipLaunchKernelGGL(k_repack_q6_K, grid, dim3(256), 0, st, rows, pl.mid_row_bytes, a.M, nsb, rw);
        CDNA4_CHECK_LAUNCH();
        rows = rw;
    }
    cdna4_gemm_args k = pl.k; k.W = rows;
    if (pl.terminal == GQ_T64) return cdna4_run_gemm_t64(k, pl.t64, st);
    if (pl.terminal == GQ_R8) return cdna4_run_gemm_r8(k, pl.r8, st);
    int rc = 0;
    // (the five formats of cdna4_main5, in the order that keeps the kernels' order in the code object what it was before there was a plan)
    cdna4_dispatch(cdna4_types<CDNA4_Q4_K, CDNA4_Q5_K, CDNA4_Q4_0, CDNA4_Q6_K, CDNA4_Q8_0>{}, pl.mid_type, [&](auto t) { rc = launch_planned<t.value>(k, pl, st); });
    return rc;
}

