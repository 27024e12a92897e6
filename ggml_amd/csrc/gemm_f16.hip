// gemm_f16.hip — MUL_MAT on F16 / BF16 weights (F32 activations rounded to the weight's format first: vec_dot_type F16, ggml-cpu.c:7428-7605, and BF16,
// ggml-cpu.c:400-405; fp32 accumulation) on the matrix cores, and ggml_cdna4_op_mul_mat_f itself: validate, plan (gemm_f16_plan.hpp), execute.  Kernels beside
// k_mul_mat_f (ops.hip), which keeps F32 weights and every F16 / BF16 call these cannot read (K not a multiple of 8, src0 / src1 data or strides off 16 bytes):
//   k_gemm_f16<TN, BF>  128 x TN tiles (TN 32 / 128), K step 32, v_mfma_f32_32x32x16_f16 (BF: .._bf16, same shape and accumulator layout) with the WEIGHTS as the
//                   A operand: a lane's four consecutive accumulator values are four consecutive m, and a dst row is contiguous in m — 16-byte stores.  The weight
//                   tile goes from its 2-byte rows straight into a three-slot LDS ring by LDS-DMA, two stages ahead; the activation tile goes through registers
//                   (float4 loads issued before a stage's MFMAs, rounded — BF: v_cvt_pk_bf16_f32 — and written behind them), one stage ahead.  One barrier per K step.
//   k_gemv_f16<NB>  1 .. 8 activation rows: every wave streams TWO weight rows in 16-byte lane chunks (1 KB per wave load, eight loads in flight) against the NB
//                   activation rows, rounded to fp16 once per work-group into LDS.
//   k_gemv_bf16<NB> the same stream on bf16 rows with a loop of its own: a bf16 is the upper half of its fp32, so a weight dword becomes two fp32 by a shift and a mask
//                   (once per chunk, shared by the NB rows), and the activations lie in LDS rounded to bf16 but already WIDENED to fp32 — the FMAs read them as they are.
// LDS map of k_gemm_f16, per ring slot: [128 weight rows x 64 B][TN activation rows x 64 B]; a row holds its four 16-byte k-chunks at chunk ^ ((row >> 2) & 3),
// so the sixteen lanes of a ds_read_b128 phase (rows r .. r + 15, one chunk) touch sixteen different 16-byte columns of the 256-byte bank window.
#include "../../include/ggml_cdna4_f16.h"
#include "cdna4_common.h"
#include "cdna4_kernels.h"
#include "gemm_f16_dev.hpp"
#include "gemm_f16_plan.hpp"
#include "gemm_q_hw.h"

typedef ggml_cdna4_tensor T4;

struct f16_args {
    const uint8_t *W; int64_t w_nb1, w_nb2, w_nb3;      // fp16 / bf16 rows of K weights
    const uint8_t *X; int64_t x_nb1, x_nb2, x_nb3;      // fp32 rows of K activations
    uint8_t *Y; int64_t y_nb1, y_nb2, y_nb3;            // Y[n][m], m contiguous
    int M, N, K;
    int y16;                                            // k_gemm_f16: dst rows take 16-byte stores
    int ne2, r2, r3;                                    // dst batch (i2, i3) = (z % ne2, z / ne2) reads the weights of (i2 / r2, i3 / r3)
};

// ------------------------------------------------------------------------------------------------ the matrix-core GEMM
#define F16_WST (F16_GEMM_TM * 64)                      // bytes of a weight stage: 128 rows x 32 halves
template <int TN, bool BF>
__global__ __launch_bounds__(256, 2) void k_gemm_f16(const f16_args p) {
    typedef typename f16_elem<BF>::e elem_t; typedef typename f16_elem<BF>::v4 elem4_t; typedef typename f16_elem<BF>::v8 elem8_t;
    constexpr int XST = TN * 64, ST = F16_WST + XST, NST = 3;
    constexpr int NXL = TN / 32;                        // float4 loads per thread and stage
    constexpr int NBLK = TN == 128 ? 2 : 1;             // 32 x 32 blocks per wave and direction: a 64 x 64 / 32 x 32 wave tile
    __shared__ __attribute__((aligned(16))) uint8_t smem[NST * ST];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * F16_GEMM_TM, n0 = blockIdx.y * TN;
    const int i2 = (int)(blockIdx.z % (unsigned)p.ne2), i3 = (int)(blockIdx.z / (unsigned)p.ne2);
    const uint8_t *const wb = p.W + (int64_t)(i2 / p.r2) * p.w_nb2 + (int64_t)(i3 / p.r3) * p.w_nb3 + (int64_t)m0 * p.w_nb1;
    const uint8_t *const xb = p.X + (int64_t)i2 * p.x_nb2 + (int64_t)i3 * p.x_nb3;
    const int K = p.K, nsteps = (K + 31) >> 5;
    const uint32_t lds0 = CDNA4_LDS_BASE(smem);

    // ---- the weight stage: eight 1 KB wave-pieces, two per wave.  LDS slot (16 bytes) q of a stage = row q / 4, stored chunk q % 4; rows past M read row M - 1
    uint32_t wrow[2]; int wchunk[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = (wave * 2 + i) * 64 + lane, r = q >> 2;
        wchunk[i] = (q & 3) ^ ((r >> 2) & 3);
        wrow[i] = (uint32_t)min(r, p.M - 1 - m0) * (uint32_t)p.w_nb1;
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

    // ---- the activation stage: TN rows x 32 k as float4 pieces, eight threads per row; rows past N read row N - 1
    f32x4 xr[NXL]; const uint8_t *xrow[NXL]; int xlds[NXL];
#pragma unroll
    for (int i = 0; i < NXL; i++) {
        const int f = tid + 256 * i, r = f >> 3, kq = f & 7;
        xrow[i] = xb + (int64_t)min(n0 + r, p.N - 1) * p.x_nb1;
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
            for (int bi = 0; bi < NBLK; bi++)
#pragma unroll
                for (int bj = 0; bj < NBLK; bj++) acc[bi][bj] = f16_mfma(a[bi], b[bj], acc[bi][bj]);
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

    // ---- store: accumulator values 4 g .. 4 g + 3 of a lane are rows m .. m + 3 of column n
    uint8_t *const yb = p.Y + (int64_t)i2 * p.y_nb2 + (int64_t)i3 * p.y_nb3;
#pragma unroll
    for (int bj = 0; bj < NBLK; bj++) {
        const int n = n0 + wave_n + 32 * bj + (lane & 31);
        if (n >= p.N) continue;
        float *const yrow = (float *)(yb + (int64_t)n * p.y_nb1);
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

// ------------------------------------------------------------------------------------------------ 1 .. 8 activation rows
#define F16_GEMV_KC 2048                                // k per pass: NB rows of it as fp16 in LDS (NB x 4 KB)
template <int NB>
__global__ __launch_bounds__(256) void k_gemv_f16(const f16_args p) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[NB * F16_GEMV_KC * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * F16_GEMV_ROWS + wave * 2;                         // this wave's two weight rows (past M: row M - 1, not stored)
    const int i2 = (int)(blockIdx.z % (unsigned)p.ne2), i3 = (int)(blockIdx.z / (unsigned)p.ne2);
    const uint8_t *const wbat = p.W + (int64_t)(i2 / p.r2) * p.w_nb2 + (int64_t)(i3 / p.r3) * p.w_nb3;
    const uint8_t *const w0 = wbat + (int64_t)min(row0, p.M - 1) * p.w_nb1, *const w1 = wbat + (int64_t)min(row0 + 1, p.M - 1) * p.w_nb1;
    const uint8_t *const xb = p.X + (int64_t)i2 * p.x_nb2 + (int64_t)i3 * p.x_nb3;
    float acc0[NB], acc1[NB];
#pragma unroll
    for (int n = 0; n < NB; n++) acc0[n] = acc1[n] = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += F16_GEMV_KC) {
        const int kc = min(F16_GEMV_KC, p.K - k0);
        if (k0) __syncthreads();
        // the NB activation rows of this pass, rounded to fp16 (nearest even) once per work-group; a padding row repeats row N - 1
#pragma unroll
        for (int n = 0; n < NB; n++) {
            const float *const xr = (const float *)(xb + (int64_t)min(n, p.N - 1) * p.x_nb1) + k0;
            for (int q = tid; q < kc / 4; q += 256) {
                const float4 v = *(const float4 *)(xr + 4 * q);
                half4_t h; h[0] = (half_t)v.x; h[1] = (half_t)v.y; h[2] = (half_t)v.z; h[3] = (half_t)v.w;
                *(half4_t *)(smem + (n * F16_GEMV_KC + 4 * q) * 2) = h;
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
                const half8_t ha = __builtin_bit_cast(half8_t, wa[j]), hc = __builtin_bit_cast(half8_t, wc[j]);
#pragma unroll
                for (int n = 0; n < NB; n++) {
                    const half8_t x = *(const half8_t *)(smem + (n * F16_GEMV_KC + (c + 64 * j) * 8) * 2);
#pragma unroll
                    for (int e = 0; e < 8; e++) { acc0[n] = fmaf((float)ha[e], (float)x[e], acc0[n]); acc1[n] = fmaf((float)hc[e], (float)x[e], acc1[n]); }
                }
            }
        }
    }
    uint8_t *const yb = p.Y + (int64_t)i2 * p.y_nb2 + (int64_t)i3 * p.y_nb3;
#pragma unroll
    for (int n = 0; n < NB; n++) {
        const float s0 = wave_sum_dpp(acc0[n]), s1 = wave_sum_dpp(acc1[n]);
        if (lane == 0 && n < p.N) {
            float *const yrow = (float *)(yb + (int64_t)n * p.y_nb1);
            if (row0 < p.M) yrow[row0] = s0;
            if (row0 + 1 < p.M) yrow[row0 + 1] = s1;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 1 .. 8 activation rows, bf16 weights
// LDS, per activation row: two planes of KC / 8 float4 — plane h holds k 4 h .. 4 h + 3 of every 8-k chunk, so the lanes of a wave (consecutive chunks) read
// consecutive 16-byte pieces of a plane: no bank conflict.  NB x 8 KB.
template <int NB>
__global__ __launch_bounds__(256) void k_gemv_bf16(const f16_args p) {
    constexpr int NCH = F16_GEMV_KC / 8;                                            // chunks (of eight k) per pass
    __shared__ __attribute__((aligned(16))) uint8_t smem[NB * F16_GEMV_KC * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * F16_GEMV_ROWS + wave * 2;                         // this wave's two weight rows (past M: row M - 1, not stored)
    const int i2 = (int)(blockIdx.z % (unsigned)p.ne2), i3 = (int)(blockIdx.z / (unsigned)p.ne2);
    const uint8_t *const wbat = p.W + (int64_t)(i2 / p.r2) * p.w_nb2 + (int64_t)(i3 / p.r3) * p.w_nb3;
    const uint8_t *const w0 = wbat + (int64_t)min(row0, p.M - 1) * p.w_nb1, *const w1 = wbat + (int64_t)min(row0 + 1, p.M - 1) * p.w_nb1;
    const uint8_t *const xb = p.X + (int64_t)i2 * p.x_nb2 + (int64_t)i3 * p.x_nb3;
    float acc0[NB], acc1[NB];
#pragma unroll
    for (int n = 0; n < NB; n++) acc0[n] = acc1[n] = 0.f;

    for (int k0 = 0; k0 < p.K; k0 += F16_GEMV_KC) {
        const int kc = min(F16_GEMV_KC, p.K - k0);
        if (k0) __syncthreads();
        // the NB activation rows of this pass, rounded to bf16 (nearest even, no subnormal flush) once per work-group and kept as fp32; a padding row repeats row N - 1
#pragma unroll
        for (int n = 0; n < NB; n++) {
            const float *const xr = (const float *)(xb + (int64_t)min(n, p.N - 1) * p.x_nb1) + k0;
            for (int q = tid; q < kc / 4; q += 256) {
                const float4 v = *(const float4 *)(xr + 4 * q);
                *(f32x4 *)(smem + ((n * 2 + (q & 1)) * NCH + (q >> 1)) * 16) = f32x4{(float)(__bf16)v.x, (float)(__bf16)v.y, (float)(__bf16)v.z, (float)(__bf16)v.w};
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
                // a bf16 is the upper half of its fp32: dword d holds weight 2 d in its low half (a shift) and weight 2 d + 1 in its high half (a mask)
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
                        for (int e = 0; e < 4; e++) { acc0[n] = fmaf(fa[4 * h + e], x[e], acc0[n]); acc1[n] = fmaf(fc[4 * h + e], x[e], acc1[n]); }
                    }
                }
            }
        }
    }
    uint8_t *const yb = p.Y + (int64_t)i2 * p.y_nb2 + (int64_t)i3 * p.y_nb3;
#pragma unroll
    for (int n = 0; n < NB; n++) {
        const float s0 = wave_sum_dpp(acc0[n]), s1 = wave_sum_dpp(acc1[n]);
        if (lane == 0 && n < p.N) {
            float *const yrow = (float *)(yb + (int64_t)n * p.y_nb1);
            if (row0 < p.M) yrow[row0] = s0;
            if (row0 + 1 < p.M) yrow[row0 + 1] = s1;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
static int f16_cu_count() {                                        // of the current device; without one CDNA4_ASSUME_CUS names the part (the route query on the CPU)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        const int assumed = getenv("CDNA4_ASSUME_CUS") ? atoi(getenv("CDNA4_ASSUME_CUS")) : 1;
        return assumed > 0 ? assumed : 1;
    }
    static int n[16] = {0};
    if (dev < 0 || dev >= 16) return 1;
    if (!n[dev]) { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, dev) == hipSuccess) n[dev] = pr.multiProcessorCount; else { (void)hipGetLastError(); n[dev] = 1; } }
    return n[dev];
}

static int f16_run(const f16_plan &pl, const T4 *a, const T4 *b, const T4 *d, hipStream_t st) {
    f16_args p;
    p.W = (const uint8_t *)a->data; p.w_nb1 = a->nb[1]; p.w_nb2 = a->nb[2]; p.w_nb3 = a->nb[3];
    p.X = (const uint8_t *)b->data; p.x_nb1 = b->nb[1]; p.x_nb2 = b->nb[2]; p.x_nb3 = b->nb[3];
    p.Y = (uint8_t *)d->data; p.y_nb1 = d->nb[1]; p.y_nb2 = d->nb[2]; p.y_nb3 = d->nb[3];
    p.M = (int)d->ne[0]; p.N = (int)d->ne[1]; p.K = (int)a->ne[0];
    p.y16 = pl.y16 ? 1 : 0;
    p.ne2 = (int)d->ne[2]; p.r2 = (int)(b->ne[2] / a->ne[2]); p.r3 = (int)(b->ne[3] / a->ne[3]);
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    const bool bf = a->type == CDNA4_BF16;
    if (pl.route == F16_GEMM) {
        if (bf) {
            if (pl.tn == 128) hipLaunchKernelGGL((k_gemm_f16<128, true>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((k_gemm_f16<32, true>), grid, dim3(256), 0, st, p);
        } else {
            if (pl.tn == 128) hipLaunchKernelGGL((k_gemm_f16<128, false>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((k_gemm_f16<32, false>), grid, dim3(256), 0, st, p);
        }
    } else if (bf) {
        switch (pl.nb) {
            case 1: hipLaunchKernelGGL(k_gemv_bf16<1>, grid, dim3(256), 0, st, p); break;
            case 2: hipLaunchKernelGGL(k_gemv_bf16<2>, grid, dim3(256), 0, st, p); break;
            case 4: hipLaunchKernelGGL(k_gemv_bf16<4>, grid, dim3(256), 0, st, p); break;
            default: hipLaunchKernelGGL(k_gemv_bf16<8>, grid, dim3(256), 0, st, p); break;
        }
    } else {
        switch (pl.nb) {
            case 1: hipLaunchKernelGGL(k_gemv_f16<1>, grid, dim3(256), 0, st, p); break;
            case 2: hipLaunchKernelGGL(k_gemv_f16<2>, grid, dim3(256), 0, st, p); break;
            case 4: hipLaunchKernelGGL(k_gemv_f16<4>, grid, dim3(256), 0, st, p); break;
            default: hipLaunchKernelGGL(k_gemv_f16<8>, grid, dim3(256), 0, st, p); break;
        }
    }
    CDNA4_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int ggml_cdna4_op_mul_mat_f_route(const T4 *a, const T4 *b, const T4 *d) { return f16_make_plan(a, b, d, f16_cu_count()).route; }

int ggml_cdna4_op_mul_mat_f(const T4 *a, const T4 *b, const T4 *d, void *stream) {
    const f16_plan pl = f16_make_plan(a, b, d, f16_cu_count());
    if (pl.route == F16_REFUSED) return cdna4_set_error_msg(pl.err);
    if (pl.empty) return 0;
    if (pl.route == F16_PLAIN) return cdna4_launch_mul_mat_f(a, b, d, (hipStream_t)stream);
    return f16_run(pl, a, b, d, (hipStream_t)stream);
}

}  // extern "C"
