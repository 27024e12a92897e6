// gemm_f16.hip — MUL_MAT on F16 / BF16 weights (F32 activations rounded to the weight's format first: vec_dot_type F16, ggml-cpu.c:7428-7605, and BF16,
// ggml-cpu.c:400-405; fp32 accumulation) on the matrix cores, and ggml_cdna4_op_mul_mat_f itself: validate, plan (gemm_f16_plan.hpp), execute.  Kernels beside
// k_mul_mat_f (ops.hip), which keeps F32 weights and every F16 / BF16 call these cannot read (K not a multiple of 8, src0 / src1 data or strides off 16 bytes):
//   k_gemm_f16<TN, BF>  f16_gemm_tile (gemm_f16_dev.hpp) on the 128 x TN tile blockIdx.x / .y of batch blockIdx.z: rows past M read row M - 1, columns past N read row
//                       N - 1 of src1 and are not stored.
//   k_gemv_f16<NB, BF>  1 .. 8 activation rows: f16_gemv_stream (gemm_f16_dev.hpp), a wave on weight rows 8 blockIdx.x + 2 wave, + 1 against the NB first rows of
//                       src1 (a padding row repeats row N - 1 and is not stored).
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
struct f16_dense_tile {                                 // what f16_gemm_tile asks: tile (m0, n0) of one batch
    const uint8_t *wb; int64_t w_nb1; int m0, M, y16;
    const uint8_t *xb; int64_t x_nb1; uint8_t *yb; int64_t y_nb1; int n0, N;
    __device__ __forceinline__ const uint8_t *xrow(int r) const { return xb + (int64_t)min(n0 + r, N - 1) * x_nb1; }
    __device__ __forceinline__ constexpr bool live(int) const { return true; }
    __device__ __forceinline__ bool yrow(int c, float *&y) const { y = (float *)(yb + (int64_t)(n0 + c) * y_nb1); return n0 + c < N; }
};
template <int TN, bool BF>
__global__ __launch_bounds__(256, 2) void k_gemm_f16(const f16_args p) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[F16_TILE_LDS(TN)];
    const int m0 = blockIdx.x * F16_GEMM_TM, n0 = blockIdx.y * TN;
    const int i2 = (int)(blockIdx.z % (unsigned)p.ne2), i3 = (int)(blockIdx.z / (unsigned)p.ne2);
    const f16_dense_tile t = {p.W + (int64_t)(i2 / p.r2) * p.w_nb2 + (int64_t)(i3 / p.r3) * p.w_nb3 + (int64_t)m0 * p.w_nb1, p.w_nb1, m0, p.M, p.y16,
                              p.X + (int64_t)i2 * p.x_nb2 + (int64_t)i3 * p.x_nb3, p.x_nb1, p.Y + (int64_t)i2 * p.y_nb2 + (int64_t)i3 * p.y_nb3, p.y_nb1, n0, p.N};
    f16_gemm_tile<TN, BF>(smem, t, p.K);
}

// ------------------------------------------------------------------------------------------------ 1 .. 8 activation rows
template <int NB, bool BF>
__global__ __launch_bounds__(256) void k_gemv_f16(const f16_args p) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[F16_GEMV_LDS(NB, BF)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * F16_GEMV_ROWS + wave * 2;                         // this wave's two weight rows (past M: row M - 1, not stored)
    const int i2 = (int)(blockIdx.z % (unsigned)p.ne2), i3 = (int)(blockIdx.z / (unsigned)p.ne2);
    const uint8_t *const wbat = p.W + (int64_t)(i2 / p.r2) * p.w_nb2 + (int64_t)(i3 / p.r3) * p.w_nb3;
    const uint8_t *const w0 = wbat + (int64_t)min(row0, p.M - 1) * p.w_nb1, *const w1 = wbat + (int64_t)min(row0 + 1, p.M - 1) * p.w_nb1;
    const uint8_t *const xb = p.X + (int64_t)i2 * p.x_nb2 + (int64_t)i3 * p.x_nb3;
    float s0[NB], s1[NB];
    f16_gemv_stream<NB, BF>(s0, s1, smem, w0, w1, [&](int n) __attribute__((always_inline)) { return (const float *)(xb + (int64_t)min(n, p.N - 1) * p.x_nb1); }, p.K);
    uint8_t *const yb = p.Y + (int64_t)i2 * p.y_nb2 + (int64_t)i3 * p.y_nb3;
#pragma unroll
    for (int n = 0; n < NB; n++) {
        if (lane == 0 && n < p.N) {
            float *const yrow = (float *)(yb + (int64_t)n * p.y_nb1);
            if (row0 < p.M) yrow[row0] = s0[n];
            if (row0 + 1 < p.M) yrow[row0 + 1] = s1[n];
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
        if (pl.tn == 128) F16_LAUNCH(k_gemm_f16, 128, bf, grid, st, p);
        else F16_LAUNCH(k_gemm_f16, 32, bf, grid, st, p);
    } else {
        switch (pl.nb) {
            case 1: F16_LAUNCH(k_gemv_f16, 1, bf, grid, st, p); break;
            case 2: F16_LAUNCH(k_gemv_f16, 2, bf, grid, st, p); break;
            case 4: F16_LAUNCH(k_gemv_f16, 4, bf, grid, st, p); break;
            default: F16_LAUNCH(k_gemv_f16, 8, bf, grid, st, p); break;
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
