// capi.hip — the C-ABI of libcdna4_kernels.so (declared in include/ggml_cdna4.h).
#include "../../include/ggml_cdna4.h"
#include "cdna4_common.h"
#include "cdna4_formats.hpp"
#include "cdna4_kernels.h"
#include "gemm_q_plan.hpp"
#include "mul_mat_id_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

int cdna4_set_error(hipError_t e, const char *file, int line) {
    snprintf(g_err, sizeof g_err, "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
    return -1;
}
int cdna4_set_error_msg(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); return -1; }

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// Q5_0 / Q3_K / Q2_K: int8-dot GEMV units of gemv_q.hip for up to 8 activation rows, above that the Q8_0 / Q6_K MFMA GEMM on an exact
// re-encoding of the weights (convert_w.hip; Q2_K as [scale part | minimum part] against a doubled activation image)
// Q4_1 / Q5_1 (Q8_1 activations: s in the place of the bsums) and IQ4_NL: GEMV units; above 8 rows the Q8_0 GEMM on the re-encoding
// (Q4_1 / Q5_1 as [d q | m 1] against a doubled activation image, like Q2_K)
// (which types these are: cdna4_common.h — cdna4_type_qk() != 0 for the twelve accepted weight formats, cdna4_type_is_kq() for their superblock half)

// workspace carve: [qs int8 B*K][d f32 B*K/qka][bsums i16 B*K/16][xh f16 B*K]
struct ws_view { int8_t *qs; float *d; int16_t *bsums; void *xh; size_t total; };
static ws_view carve(int type, int64_t K, int64_t B, void *base) {
    ws_view v; uint8_t *p = (uint8_t *)base; size_t off = 0;
    const int64_t qka = cdna4_type_is_kq(type) ? 256 : 32;
    v.qs = (int8_t *)(p + off); off += align256((size_t)(B * K));
    v.d = (float *)(p + off); off += align256((size_t)(B * (K / qka)) * 4);
    v.bsums = (int16_t *)(p + off); off += align256((size_t)(B * (K / 16)) * 2);
    const int64_t kh = K * cdna4_convert_weights_kmul(type);       // Q2_K's GEMM reads the image twice in a row (convert_w.hip)
    v.xh = (void *)(p + off); off += align256((size_t)(B * ((kh + 127) / 128 * 128)) * 2) + 32768;    // whole 128-k panels; + slack: k_gemm_kq_t64 reads (and discards) up to 127 rows past a ragged last activation tile
    v.total = off;
    return v;
}

// workspace of the grouped MUL_MAT_ID path: [img_src i32 R][img_dst i32 R][tile_expert | tile_order | tile_nfrag: 3 x i32 R/128][xh f16 R x K (+ slack)], R = image rows =
// an upper bound of sum_e ceil(cnt_e / 128) * 128
struct moe_view { int32_t *img_src, *img_dst, *tile_expert; void *xh; int64_t img_rows; size_t total; };
static moe_view moe_carve(int64_t K, int64_t n_expert, int64_t n_used, int64_t n_tok, void *base) {
    moe_view v; uint8_t *p = (uint8_t *)base; size_t off = 0;
    const int64_t n_pairs = n_tok * n_used;
    v.img_rows = (n_pairs + 127) / 128 * 128 + 128 * n_expert;
    v.img_src = (int32_t *)(p + off); off += align256((size_t)v.img_rows * 4);
    v.img_dst = (int32_t *)(p + off); off += align256((size_t)v.img_rows * 4);
    v.tile_expert = (int32_t *)(p + off); off += align256((size_t)(v.img_rows / 128) * 4 * 3);     // [tile_expert | tile_order | tile_nfrag] (k_moe_plan writes all three)
    v.xh = (void *)(p + off); off += align256((size_t)v.img_rows * K * 2) + 32768;
    v.total = off;
    return v;
}

// the stream-k form of the grouped MUL_MAT_ID (round 6; quantize_act.hip: cdna4_launch_moe_sk_front, gemm_q_sk.hip): tile records, the spans, and the fp16 image of the
// n_tok * n_b activation rows in TOKEN order (the GEMM gathers a tile's rows itself: no per-pair copies, no padding rows)
struct moe_sk_view { int32_t *tile_rec, *wg_begin; void *xh; int64_t n_rows, ntile_cap; size_t total; };
static moe_sk_view moe_sk_carve(int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok, void *base) {
    moe_sk_view v; uint8_t *p = (uint8_t *)base; size_t off = 0;
    const int64_t n_pairs = n_tok * n_used;
    v.n_rows = n_tok * n_b;
    v.ntile_cap = (n_expert < n_pairs ? n_expert : n_pairs) + n_pairs / 128 + 1;          // >= sum_e ceil(cnt_e / 128)
    v.tile_rec = (int32_t *)(p + off); off += align256((size_t)v.ntile_cap * CDNA4_SK_REC * 4);
    v.wg_begin = (int32_t *)(p + off); off += align256((size_t)(1024 + 2) * 4);
    v.xh = (void *)(p + off); off += align256((size_t)v.n_rows * K * 2) + 32768;
    v.total = off;
    return v;
}
// may a MUL_MAT_ID of this type / K / expert count take the work-queue form?  (Q4_K experts, or Q4_0 experts in case their stack has a resident Q4_0R image: the plan
// and the workspace size both ask here)
static bool mmid_queue_shape(int type, int64_t K, int64_t n_expert) { return (type == CDNA4_Q4_K || type == CDNA4_Q4_0) && K % 256 == 0 && n_expert <= 1024; }

extern "C" {

int ggml_cdna4_api_version(void) { return GGML_CDNA4_API_VERSION; }
void ggml_cdna4_debug_trace(void *device_buffer) { cdna4_debug_trace = device_buffer; }
uint64_t ggml_cdna4_scratch_generation(void) { return cdna4_scratch_generation(); }
const char *ggml_cdna4_last_error(void) { return g_err; }
int ggml_cdna4_set_shared_device(int shared) { return cdna4_gemm_set_shared_device(shared); }
// a launch on a route that WAITS for co-resident work-groups (only chosen on an owned device) ran into its bound: its output tile(s) are NaN.  Never silent: the code the
// kernels stored (1 grid barrier, 2 / 4 hand-off, 3 reduce-scatter) comes back here, and the library has switched itself to the shared mode.
int ggml_cdna4_device_fault(int clear) { return cdna4_gemm_take_fault(clear != 0); }
// test hook: "another tenant" — work-groups that hold LDS (so that none of our 130-KB work-groups fits beside them) until the host releases them or the time is up
#ifndef CDNA4_HW_OVERRIDE
__global__ __launch_bounds__(64) void k_debug_occupy(const int *release, unsigned long long max_ticks, int lds_bytes) {
    extern __shared__ uint8_t occ_lds[];
    if (threadIdx.x == 0) occ_lds[lds_bytes - 1] = 1;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();        // 100 MHz
    while (__builtin_amdgcn_s_memrealtime() - t0 < max_ticks) {
        if (release && __hip_atomic_load(release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) break;
        __builtin_amdgcn_s_sleep(32);
    }
}
#endif
int ggml_cdna4_debug_occupy(int n_workgroups, int lds_kb, const int *release, int max_ms, void *stream) {
    if (n_workgroups <= 0 || lds_kb < 1 || lds_kb > 160 || max_ms < 0 || max_ms > 20000) return cdna4_set_error_msg("debug_occupy: 1 .. 160 KB of LDS, at most 20 s");
#ifndef CDNA4_HW_OVERRIDE
    if (lds_kb > 64 && hipFuncSetAttribute(reinterpret_cast<const void *>(k_debug_occupy), hipFuncAttributeMaxDynamicSharedMemorySize, lds_kb * 1024) != hipSuccess) { (void)hipGetLastError(); return cdna4_set_error_msg("debug_occupy: cannot raise the LDS limit"); }
    hipLaunchKernelGGL(k_debug_occupy, dim3(n_workgroups), dim3(64), lds_kb * 1024, (hipStream_t)stream, release, (unsigned long long)max_ms * 100000ull, lds_kb * 1024);
    CDNA4_CHECK_LAUNCH();
#endif
    return 0;
}
static int fault_status() {
    const int f = cdna4_gemm_take_fault(true);
    if (!f) return 0;
    snprintf(g_err, sizeof g_err, "an EARLIER launch waited for a co-resident work-group that never arrived (code %d): the device is not exclusively ours, that launch's output holds NaN tiles; "
                                  "the library now uses the non-waiting routes (ggml_cdna4_set_shared_device(1))", f);
    return -3;
}
int ggml_cdna4_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }
int ggml_cdna4_set_device(int device) { hipError_t e = hipSetDevice(device); return e == hipSuccess ? 0 : cdna4_set_error(e, __FILE__, __LINE__); }

size_t ggml_cdna4_row_size(int type, int64_t k) {
    if (type == CDNA4_F32) return (size_t)k * 4;
    if (type == CDNA4_F16) return (size_t)k * 2;
    const int qk = cdna4_type_qk(type);
    return qk && k % qk == 0 ? (size_t)(k / qk) * cdna4_type_bytes(type) : 0;
}

size_t ggml_cdna4_mul_mat_workspace_size(int type, int64_t K, int64_t n_act_rows) {
    if (!cdna4_type_qk(type) || K <= 0 || n_act_rows <= 0) return 0;
    return carve(type, K, n_act_rows, nullptr).total;
}

size_t ggml_cdna4_mul_mat_id_workspace_size(int type, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok) {
    if (!cdna4_type_qk(type) || K <= 0 || n_tok <= 0 || n_used <= 0 || n_b <= 0 || n_expert <= 0) return 0;
    const size_t plain = carve(type, K, n_tok * n_b, nullptr).total;
    if (!cdna4_gemm_ids_supported(type, K) || n_tok * n_used <= 32) return plain;
    size_t grouped = moe_carve(K, n_expert, n_used, n_tok, nullptr).total;
    // (the stream-k form's carve — Q4_K, and Q4_0 in case its stack has a resident image; M is not known here: its tables do not depend on it)
    if (mmid_queue_shape(type, K, n_expert)) { const size_t sk = moe_sk_carve(K, n_expert, n_used, n_b, n_tok, nullptr).total; if (sk > grouped) grouped = sk; }
    return grouped > plain ? grouped : plain;
}

// the public re-encodings keep the shape (Q2_K's two-part form needs the doubled activation image: library-internal)
static inline int public_convert_target(int type) {
    static const bool any = getenv("CDNA4_DIAG_CONVERT_ANY") && atoi(getenv("CDNA4_DIAG_CONVERT_ANY")) != 0;      // diagnosis only (scripts/gpu_diag_iq4xs2.py): the two-part forms too
    return (any || cdna4_convert_weights_kmul(type) == 1) ? cdna4_convert_weights_target(type) : -1;
}
int ggml_cdna4_convert_weights_target(int type) { return public_convert_target(type); }
size_t ggml_cdna4_convert_weights_size(int type, int64_t M, int64_t K) {
    if (public_convert_target(type) < 0 || M <= 0 || K <= 0 || ggml_cdna4_row_size(type, K) == 0) return 0;
    return cdna4_convert_weights_bytes(type, M, K);
}
int ggml_cdna4_convert_weights(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, void *out, void *stream) {
    if (public_convert_target(type) < 0) return cdna4_set_error_msg("convert_weights: no exact target format for this type");
    if (M <= 0) return 0;
    if (K <= 0 || ggml_cdna4_row_size(type, K) == 0) return cdna4_set_error_msg("convert_weights: K is not a whole number of blocks");
    if (!W || !out || w_row_bytes < (int64_t)ggml_cdna4_row_size(type, K)) return cdna4_set_error_msg("convert_weights: bad pointers or row stride");
    return cdna4_launch_convert_weights(type, (const uint8_t *)W, w_row_bytes, M, K, (uint8_t *)out, (hipStream_t)stream);
}

// ---- resident kernel-native images (see gemm_q_mfma.hip: cdna4_resident_*)
size_t ggml_cdna4_resident_image_size(int type, int64_t M, int64_t K) {
    if (M <= 0 || K <= 0 || ggml_cdna4_row_size(type, K) == 0) return 0;
    const size_t rb = cdna4_resident_image_row_bytes(type, K);
    return rb ? (size_t)M * rb + 256 : 0;                              // + slack: the kernels read whole 16-byte pieces
}
__global__ void k_count_diff16(const u32x4 *__restrict__ a, const u32x4 *__restrict__ b, int64_t n16, unsigned *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const u32x4 x = a[i], y = b[i];
    if (x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w) atomicAdd(out, 1u);
}
int ggml_cdna4_resident_image_register(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, void *image, int verify, void *stream) {
    const size_t need = ggml_cdna4_resident_image_size(type, M, K);
    if (need == 0) return cdna4_set_error_msg("resident_image: this type has no kernel-native image");
    if (!W || !image || w_row_bytes < (int64_t)ggml_cdna4_row_size(type, K) || ((uintptr_t)image & 255)) return cdna4_set_error_msg("resident_image: bad pointers, row stride or image alignment (256 bytes)");
    hipStream_t st = (hipStream_t)stream;
    int rc = cdna4_resident_build(type, (const uint8_t *)W, w_row_bytes, M, K, (uint8_t *)image, st);
    if (rc) return rc;
    if (verify) {
        // the re-encoding a second time, into library scratch, compared byte for byte: a conversion that is not bit-stable on this device (round 3 saw ~1 % of an IQ4_XS
        // product differ between identical calls; its cause was traced to the re-encoding kernel) is refused HERE, at load time
        const size_t bytes = (size_t)M * cdna4_resident_image_row_bytes(type, K), n16 = bytes / 16;
        uint8_t *again = (uint8_t *)cdna4_gemm_scratch(bytes + 512, 3);
        if (!again) return cdna4_set_error_msg("resident_image: cannot allocate the verification scratch");
        unsigned *cnt = (unsigned *)(again + ((bytes + 255) & ~(size_t)255));
        hipError_t e = hipMemsetAsync(cnt, 0, 4, st);
        if (e != hipSuccess) return cdna4_set_error(e, __FILE__, __LINE__);
        rc = cdna4_resident_build(type, (const uint8_t *)W, w_row_bytes, M, K, again, st);
        if (rc) return rc;
        if (n16) hipLaunchKernelGGL(k_count_diff16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (const u32x4 *)image, (const u32x4 *)again, (int64_t)n16, cnt);
        CDNA4_CHECK_LAUNCH();
        unsigned bad = 0;
        e = hipMemcpyAsync(&bad, cnt, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return cdna4_set_error(e, __FILE__, __LINE__);
        if (bad) { snprintf(g_err, sizeof g_err, "resident_image: two re-encodings of the same matrix differ in %u 16-byte pieces (type %d, %lld x %lld): image not registered", bad, type, (long long)M, (long long)K); return -1; }
    } else {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return cdna4_set_error(e, __FILE__, __LINE__);
    }
    return cdna4_resident_register(type, W, w_row_bytes, M, K, image);
}
int ggml_cdna4_resident_image_unregister(const void *W) { return cdna4_resident_unregister(W); }
int ggml_cdna4_resident_image_lookup(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, const void **image) {
    const uint8_t *r = cdna4_resident_lookup(type, W, w_row_bytes, M, K);
    if (image) *image = r;
    return r ? 1 : 0;
}

int ggml_cdna4_quantize_q8_K(const float *x, int64_t x_row_stride, int64_t K, int64_t B, int8_t *qs, float *d, int16_t *bsums, void *xh, void *stream) {
    if (((uintptr_t)x | (uintptr_t)(x_row_stride * 4)) & 15) return cdna4_set_error_msg("quantize_q8_K: x must be 16-byte aligned");
    if (qs && (!d || !bsums)) return cdna4_set_error_msg("quantize_q8_K: qs needs d and bsums");
    return cdna4_launch_quantize_q8_K(x, x_row_stride, K, B, qs, d, bsums, xh, (hipStream_t)stream);
}
int ggml_cdna4_quantize_q8_0(const float *x, int64_t x_row_stride, int64_t K, int64_t B, int8_t *qs, float *d, void *xh, int ref_rounding, void *stream) {
    if (((uintptr_t)x | (uintptr_t)(x_row_stride * 4)) & 15) return cdna4_set_error_msg("quantize_q8_0: x must be 16-byte aligned");
    if (qs && !d) return cdna4_set_error_msg("quantize_q8_0: qs needs d");
    return cdna4_launch_quantize_q8_0(x, x_row_stride, K, B, qs, d, xh, ref_rounding != 0, (hipStream_t)stream);
}

int ggml_cdna4_quantize_q8_1(const float *x, int64_t x_row_stride, int64_t K, int64_t B, int8_t *qs, float *d, float *s, void *xh, void *stream) {
    if (((uintptr_t)x | (uintptr_t)(x_row_stride * 4)) & 15) return cdna4_set_error_msg("quantize_q8_1: x must be 16-byte aligned");
    return cdna4_launch_quantize_q8_1(x, x_row_stride, K, B, qs, d, s, xh, false, (hipStream_t)stream);
}

// AUTO: one row -> the one-launch decode GEMV; 2 .. 64 rows of a format the int8 matrix-core kernel takes (mmq_i8.hip) -> that (an integer-dot
// path like the GEMV: PATH_GEMV family, workspace = the int8 SoA); above 8 rows otherwise, and above 64 always -> the fp16 MFMA GEMM
static bool use_mmq(int type, int64_t M, int64_t K, int64_t B) {
    static const bool off = getenv("CDNA4_NO_MMQ") && atoi(getenv("CDNA4_NO_MMQ")) != 0;
    static const int minb = getenv("CDNA4_MMQ_MINB") ? atoi(getenv("CDNA4_MMQ_MINB")) : 0, maxb = getenv("CDNA4_MMQ_MAXB") ? atoi(getenv("CDNA4_MMQ_MAXB")) : 0;   // measurement knobs
    if (off || !cdna4_mmq_supported(type, M, K, B)) return false;
    if (maxb > 0) return B >= (minb > 0 ? minb : 2) && B <= maxb;
    // Where it wins on MI355X — round 4: DEVICE time (HIP-graph replay of 40 calls, quantizer launch included; scripts/gpu_batch_sweep.py ->
    // profiles/r04/batch_sweep.txt: five formats x {4096^2, 4096 x 14336, 3072 x 768} x 2 .. 64 rows x {AUTO, kernel off, kernel forced}; round 3's sweep was
    // taken through a Python loop whose host time hid the differences below ~14 us).  us per call, int8 matrix cores vs the alternative:
    //   2 rows      GEMV everywhere (Q4_K 4096^2 4.8 vs 7.6)
    //   3 .. 4      GEMV unless the matrix is large: 4096^2 6.8 / 7.1 vs 7.8 / 7.9, 4096 x 14336 17.0 / 17.4 (GEMV) vs 13.8 / 14.0
    //   5 .. 8      the matrix cores EVERYWHERE: the 8-column GEMV forms take 11.2 / 11.5 us at 4096^2 (3072 x 768: 7.7 / 7.9) against 7.9 (5.9)      [new in round 4]
    //   9 .. 32     the matrix cores: 7.9 .. 11.0 vs 19.7 .. 20.6 on the fp16 GEMM at 4096^2; Q6_K 4096 x 14336 20.5 .. 27.9 vs 79
    //   33 .. 48    the matrix cores (not Q6_K: its three-group form spills): 4096^2 14.0 vs 21.1; 4096 x 14336 Q4_K 29.4 vs 31.4, Q4_0 40.1 vs 50.3, Q8_0 48.0 vs
    //               76.8, Q5_K 29.8 vs 63.6                                                                                                        [new in round 4]
    //   49 .. 64    small matrices (4096^2: 20.0 vs 21.0; 3072 x 768: 10.1 vs 13.7), and Q8_0 / Q5_K at any size (4096 x 14336: 59.9 vs 77.3, 48.3 vs 64.3); Q4_K / Q4_0
    //               on large matrices stay on the fp16 GEMM (49.0 vs 31.7, 52.8 vs 50.9)
    if (B >= 5 && B <= 48) return true;
    if (B >= 3 && B <= 4) return M * K >= ((int64_t)1 << 25);
    if (B >= 49) return M * K <= ((int64_t)1 << 24) || type == CDNA4_Q8_0 || type == CDNA4_Q5_K;
    return false;
}

int ggml_cdna4_prepare_act(int type, const float *X, int64_t x_row_stride, int64_t K, int64_t B, void *workspace, size_t workspace_bytes, int path, void *stream) {
    if (!cdna4_type_qk(type)) return cdna4_set_error_msg("prepare_act: unsupported weight type");
    if (B <= 0 || K <= 0) return 0;
    if (!workspace || ((uintptr_t)workspace & 255)) return cdna4_set_error_msg("prepare_act: workspace must be 256-byte aligned");
    const ws_view v = carve(type, K, B, workspace);
    if (workspace_bytes < v.total) return cdna4_set_error_msg("prepare_act: workspace too small");
    const bool want_i8 = path != GGML_CDNA4_PATH_GEMM, want_h = path != GGML_CDNA4_PATH_GEMV;
    if (cdna4_type_is_kq(type)) {
        const int rc = ggml_cdna4_quantize_q8_K(X, x_row_stride, K, B, want_i8 ? v.qs : nullptr, v.d, v.bsums, want_h ? v.xh : nullptr, stream);
        if (rc || !want_h || cdna4_convert_weights_kmul(type) == 1) return rc;
        // the image is k-panel-major ([K / 128][B][128] fp16): k-panels K / 128 .. 2 K / 128 - 1 of the doubled image are a copy of the first B K halves
        const hipError_t e = hipMemcpyAsync((char *)v.xh + (size_t)B * K * 2, v.xh, (size_t)B * K * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        return e == hipSuccess ? 0 : cdna4_set_error(e, __FILE__, __LINE__);
    }
    if (!cdna4_is_q81(type)) return ggml_cdna4_quantize_q8_0(X, x_row_stride, K, B, want_i8 ? v.qs : nullptr, v.d, want_h ? v.xh : nullptr, 0, stream);
    // Q4_1 / Q5_1: Q8_1 activations — s = fp16(d * sum q) per 32-block as fp32 where the K-quants keep their bsums (same byte count); the GEMM reads the
    // fp16 image twice in a row ([d q | m 1] weights): whole 128-k panels only (cdna4_gemm_q_supported)
    if (((uintptr_t)X | (uintptr_t)(x_row_stride * 4)) & 15) return cdna4_set_error_msg("quantize_q8_1: x must be 16-byte aligned");
    // GEMM image: [x~ | s e0] — the quantizer writes both halves (the second: the CPU's own fp16 s per 32-block against the weights' [d q | m e0]);
    // a ragged last panel has no GEMM form (cdna4_gemm_q_supported says so): then only the first half is written
    return cdna4_launch_quantize_q8_1(X, x_row_stride, K, B, want_i8 ? v.qs : nullptr, v.d, reinterpret_cast<float *>(v.bsums), want_h ? v.xh : nullptr,
                                      want_h && K % 128 == 0, (hipStream_t)stream);
}

static cdna4_gemm_args gemm_args_of(int type, const void *W, int64_t w_row_bytes, const void *xh, float *Y, int64_t y_row_stride, int64_t M, int64_t K, int64_t B,
                                    int gemm_variant, int splitk, const cdna4_epilogue &epi) {
    cdna4_gemm_args a{};
    a.type = type; a.W = (const uint8_t *)W; a.w_row_bytes = w_row_bytes; a.xh = xh; a.xh_row_elems = K;
    a.Y = Y; a.y_row_elems = y_row_stride; a.M = (int)M; a.K = (int)K; a.B = (int)B; a.variant = gemm_variant; a.splitk = splitk; a.epi = epi;
    return a;
}
// v: the quantized activations (ws_view{}: the kernel quantizes them itself); the MUL_MAT_ID callers add their ids with gemv_ids()
static cdna4_gemv_args gemv_args_of(int type, const void *W, int64_t w_row_bytes, const ws_view &v, float *Y, int64_t y_col_stride, int64_t M, int64_t K, int64_t ncol,
                                    const cdna4_epilogue &epi) {
    cdna4_gemv_args g{};
    g.type = type; g.W = (const uint8_t *)W; g.w_row_bytes = w_row_bytes; g.qs = v.qs; g.d = v.d; g.bsums = v.bsums;
    g.Y = Y; g.y_col_stride = y_col_stride; g.M = (int)M; g.K = (int)K; g.ncol = (int)ncol; g.epi = epi;
    return g;
}

// ---- The routing plan of a MUL_MAT: the ONE place that decides which kernel a call takes.  The calls launch what it says,
// the queries (route, image key, may_alias, the grouped call's admission) read its fields: change the routing here and nowhere else.
enum mm_kind {
    MM_NONE,            // not a supported call
    MM_REENCODE,        // an exact re-encoding of the weights (convert_w.hip), then the plan of `reencode_target`
    MM_GEMV_1,          // ONE launch: the activation quantizer inside the GEMV (workspace untouched)
    MM_GEMV_STAGED,     // quantize + GEMV with the columns staged in LDS
    MM_GEMV,            // quantize + k_gemv_q
    MM_MMQ,             // quantize + the int8 matrix-core kernel (mmq_i8.hip)
    MM_GEMM_1,          // ONE launch: the quantizer inside k_gemm_kq_t64 (which writes the image itself)
    MM_GEMM,            // quantize + the fp16 MFMA GEMM
};
struct mm_plan {
    mm_kind kind;
    int route_id;           // what ggml_cdna4_mul_mat_route documents
    uint32_t image_key;     // what ggml_cdna4_act_image_key documents
    bool tail_in_store;     // the launch applies the epilogue itself (otherwise k_epilogue follows it)
    int reencode_target;    // MM_REENCODE only, else -1
};
// Side-effect free.  X == nullptr: the image is already in the workspace (the `prepared` calls) — no re-encoding, no one-launch form, and the
// GEMV path launches the plain k_gemv_q, never the staged form.  An explicit PATH_GEMV keeps the v_dot4 units (tests compare the two).
static mm_plan plan_mul_mat(int type, const void *W, int64_t w_row_bytes, const float *X, int64_t x_row_stride, int64_t M, int64_t K, int64_t B,
                            int path, int gemm_variant, int splitk, const void *workspace) {
    mm_plan p = {MM_NONE, 0, 0, true, -1};
    if (!cdna4_type_qk(type) || M <= 0 || B <= 0 || K <= 0 || ggml_cdna4_row_size(type, K) == 0) return p;
    const bool autop = path == GGML_CDNA4_PATH_AUTO;
    // Formats with an exact same-shape re-encoding (Q5_0 / IQ4_NL -> Q8_0, Q3_K -> Q6_K) follow their TARGET format onto the int8 matrix-core kernel
    // where that one is chosen: its integer dots on Q8_0 activations are the CPU's own arithmetic for the source format (tests/test_gpu_widening.py).
    // From 9 rows up: below that the re-encoding pass (~2.5x the weight bytes) costs more than the staged GEMV it would replace.
    // The re-encoded rows are 16-byte aligned (library scratch, or a resident image).
    const int kmul = cdna4_convert_weights_kmul(type), tgt = cdna4_convert_weights_target(type);
    if (autop && X && kmul == 1 && tgt >= 0 && tgt != type && B >= 9 && use_mmq(tgt, M, K, B)) {
        p = plan_mul_mat(tgt, (const void *)(uintptr_t)256, (int64_t)ggml_cdna4_row_size(tgt, K), X, x_row_stride, M, K, B,
                         path, gemm_variant, splitk, workspace);
        p.kind = MM_REENCODE; p.route_id += 100; p.image_key = 0; p.reencode_target = tgt;       // (the image is the TARGET format's)
        return p;
    }
    const bool few = autop && use_mmq(type, M, K, B);                     // a batch size at which the int8 matrix cores win
    bool gemm = path == GGML_CDNA4_PATH_GEMM || (autop && !few && B > 8);
    if (gemm && !cdna4_gemm_q_supported(type, M, K, B)) {
        if (!autop) return p;
        gemm = false;
    }
    const uint32_t key = 1u | (cdna4_type_is_kq(type) ? 2u : 0u) | (cdna4_is_q81(type) ? 4u : 0u) | (kmul == 2 ? 8u : 0u);
    if (!gemm) {                                                          // the integer-dot family: the tail rides in the store
        // one launch while the redundant per-work-group quantization is cheap: B x K up to 32 K values, B rounded to the instantiated 2 / 4 / 8 columns
        const int64_t nbt = B <= 1 ? 1 : (B <= 2 ? 2 : (B <= 4 ? 4 : 8));
        const bool w_ok = !(((uintptr_t)W | (uintptr_t)w_row_bytes) & (type == CDNA4_Q6_K ? 1 : 15));
        const bool x_ok = X && !(((uintptr_t)X | (uintptr_t)(B > 1 ? x_row_stride * 4 : 0)) & 15);
        if (few && w_ok) { p.kind = MM_MMQ; p.route_id = 3; p.image_key = key; }
        else if (x_ok && cdna4_gemv_fused_supported(type, K, B) && (B == 1 || nbt * K <= 32768)) { p.kind = MM_GEMV_1; p.route_id = 1; }
        else { p.kind = X && cdna4_gemv_staged_supported(type, K, B) ? MM_GEMV_STAGED : MM_GEMV; p.route_id = 2; }
        return p;
    }
    // the GEMM side's single source of truth is the plan its launcher executes (gemm_q_plan.hpp): it sees W's alignment and resident image, the
    // image's alignment and, where the call hands its fp32 rows over next to a usable workspace, whether ONE launch does the whole step
    const void *xh = carve(type, K, B, (void *)workspace).xh;
    cdna4_gemm_args a = gemm_args_of(type, W, w_row_bytes, xh, nullptr, 0, M, K, B, gemm_variant, splitk, cdna4_epilogue{});
    if (X && workspace && !((uintptr_t)workspace & 255)) { a.xf = X; a.xf_row_elems = x_row_stride; }
    const gemm_q_plan g = gemm_q_make_plan(a);
    p.kind = g.fuses_quantizer ? MM_GEMM_1 : MM_GEMM;
    p.route_id = gemm_q_route_id(g); p.image_key = key | 16u; p.tail_in_store = g.tail_in_store;
    return p;
}
// the plan of the AUTO call on contiguous, 256-byte-aligned activations and workspace: what the queries answer from
static mm_plan plan_query(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, int64_t B) {
    return plan_mul_mat(type, W, w_row_bytes, (const float *)(uintptr_t)256, K, M, K, B, GGML_CDNA4_PATH_AUTO, 0, 0, (const void *)(uintptr_t)256);
}
static mm_plan plan_query(int type, int64_t M, int64_t K, int64_t B) {      // shape only: an aligned stand-in for W, contiguous rows
    return plan_query(type, (const void *)(uintptr_t)256, (int64_t)ggml_cdna4_row_size(type, K), M, K, B);
}

// X == nullptr: the `prepared` twins (the image is in the workspace).  epi: the MUL_MAT's tail
static int mul_mat_impl(int type, const void *W, int64_t w_row_bytes, const float *X, int64_t x_row_stride, float *Y, int64_t y_row_stride,
                        int64_t M, int64_t K, int64_t B, void *workspace, size_t workspace_bytes, int path, int gemm_variant, int splitk,
                        const cdna4_epilogue &epi, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!cdna4_type_qk(type)) return cdna4_set_error_msg("mul_mat: unsupported weight type");
    if (M <= 0 || B <= 0) return 0;
    if (K <= 0 || ggml_cdna4_row_size(type, K) == 0) return cdna4_set_error_msg("mul_mat: K is not a whole number of blocks");
    const mm_plan p = plan_mul_mat(type, W, w_row_bytes, X, x_row_stride, M, K, B, path, gemm_variant, splitk, workspace);
    if (p.kind == MM_NONE) return cdna4_set_error_msg("mul_mat: GEMM path does not support this shape");
    if (p.kind == MM_REENCODE) {
        // re-encode into scratch, then the target's own call: the same result as ggml_cdna4_convert_weights up front + ggml_cdna4_mul_mat on the target
        const int tgt = p.reencode_target;
        uint8_t *cw = const_cast<uint8_t *>(cdna4_resident_lookup(type, W, w_row_bytes, M, K));      // a resident image: no conversion launch
        if (!cw) {
            cw = (uint8_t *)cdna4_gemm_scratch(cdna4_convert_weights_bytes(type, M, K) + 256, 3);
            if (!cw) return cdna4_set_error_msg("mul_mat: cannot allocate the re-encoded weights");
            if (const int rc = cdna4_launch_convert_weights(type, (const uint8_t *)W, w_row_bytes, M, K, cw, st)) return rc;
        }
        return mul_mat_impl(tgt, cw, (int64_t)ggml_cdna4_row_size(tgt, K), X, x_row_stride, Y, y_row_stride, M, K, B, workspace, workspace_bytes,
                            path, gemm_variant, splitk, epi, stream);
    }
    if (p.kind == MM_GEMV_1) {                                            // decode with 1..8 activation rows
        const cdna4_gemv_args g = gemv_args_of(type, W, w_row_bytes, ws_view{}, Y, y_row_stride, M, K, B, epi);
        return B == 1 ? cdna4_launch_gemv_q_fused(g, X, st) : cdna4_launch_gemv_q_fused_n(g, X, x_row_stride, st);
    }
    const ws_view v = carve(type, K, B, workspace);
    if (!X || p.kind == MM_GEMM_1) {                                      // nothing to quantize in front of the launch
        if (workspace_bytes < v.total) return cdna4_set_error_msg("mul_mat: workspace too small");
    } else if (const int rc = ggml_cdna4_prepare_act(type, X, x_row_stride, K, B, workspace, workspace_bytes,
                                                     p.kind == MM_GEMM ? GGML_CDNA4_PATH_GEMM : GGML_CDNA4_PATH_GEMV, stream)) return rc;
    if (p.kind == MM_GEMM || p.kind == MM_GEMM_1) {
        cdna4_gemm_args a = gemm_args_of(type, W, w_row_bytes, v.xh, Y, y_row_stride, M, K, B, gemm_variant, splitk,
                                         p.tail_in_store ? epi : cdna4_epilogue{});
        // MM_GEMM_1: k_gemm_kq_t64<.., FQ> — every work-group quantizes its share of X into the image, a grid barrier, then the multiply (what
        // ggml_compute_forward_mul_mat does inside one op, ggml-cpu.c:7490-7509 + :7428-7605); same sums, same order as the two launches of MM_GEMM
        if (p.kind == MM_GEMM_1) { a.xf = X; a.xf_row_elems = x_row_stride; }
        const int rc = cdna4_launch_gemm_q(a, st);
        if (rc || p.tail_in_store) return rc;
        return cdna4_launch_epilogue(Y, y_row_stride, M, B, epi, st);      // the older GEMM kernels: one element-wise launch for the whole tail
    }
    const cdna4_gemv_args g = gemv_args_of(type, W, w_row_bytes, v, Y, y_row_stride, M, K, B, epi);
    if (p.kind == MM_MMQ) return cdna4_launch_mmq(g, st);                                 // 2..64 rows: int8 MFMA
    if (p.kind == MM_GEMV_STAGED) return cdna4_launch_gemv_q_staged(g, st);               // 2..8 rows: columns from LDS
    return cdna4_launch_gemv_q(g, st);
}
int ggml_cdna4_mul_mat(int type, const void *W, int64_t w_row_bytes, const float *X, int64_t x_row_stride, float *Y, int64_t y_row_stride,
                       int64_t M, int64_t K, int64_t B, void *workspace, size_t workspace_bytes, int path, int gemm_variant, int splitk, void *stream) {
    if (const int frc = fault_status()) return frc;
    return mul_mat_impl(type, W, w_row_bytes, X, x_row_stride, Y, y_row_stride, M, K, B, workspace, workspace_bytes, path, gemm_variant, splitk,
                        cdna4_epilogue{}, stream);
}
int ggml_cdna4_mul_mat_prepared(int type, const void *W, int64_t w_row_bytes, float *Y, int64_t y_row_stride, int64_t M, int64_t K, int64_t B,
                                const void *workspace, size_t workspace_bytes, int path, int gemm_variant, int splitk, void *stream) {
    if (const int frc = fault_status()) return frc;
    return mul_mat_impl(type, W, w_row_bytes, nullptr, 0, Y, y_row_stride, M, K, B, (void *)workspace, workspace_bytes, path, gemm_variant, splitk,
                        cdna4_epilogue{}, stream);
}
// n MUL_MATs of ONE activation row (B = 1) in ONE launch: wq / wk / wv, w_gate / w_up of a decoded token (round 6).  Matrices of one type and K; bias[i] may be null.
// Bit-identical to n ggml_cdna4_mul_mat[_fused] calls with B = 1 (the same kernel body per matrix).  Returns -2 where the call has no grouped form (the caller issues the
// separate calls): types outside the five headline formats, a K the one-launch decode does not take, misaligned rows.
int ggml_cdna4_mul_mat_group(int type, int n, const void *const *W, const int64_t *w_row_bytes, const int64_t *M, float *const *Y, const float *const *bias,
                             const float *X, int64_t K, void *stream) {
    if (const int frc = fault_status()) return frc;
    const char *why = nullptr;
    if (n < 1 || n > CDNA4_GEMV_GROUP_MAX || !W || !w_row_bytes || !M || !Y || !X) why = "mul_mat_group: 1 .. 4 matrices";
    else if (!cdna4_type_is_main5(type)) why = "mul_mat_group: no grouped form for this type";
    cdna4_gemv_group g{};
    g.K = (int)K;
    for (int i = 0; i < n && !why; i++) {
        const int w_mask = (type == CDNA4_Q4_K || type == CDNA4_Q5_K) ? 15 : 1;
        if (M[i] <= 0 || M[i] > 0x7fffffff || !W[i] || !Y[i] || (((uintptr_t)W[i] | (uintptr_t)w_row_bytes[i]) & w_mask)) why = "mul_mat_group: bad or misaligned matrix";
        else if (plan_mul_mat(type, W[i], w_row_bytes[i], X, K, M[i], K, 1, GGML_CDNA4_PATH_AUTO, 0, 0, nullptr).kind != MM_GEMV_1)
            why = "mul_mat_group: a matrix whose single call is not the one-launch GEMV (K, alignment)";
        g.W[i] = (const uint8_t *)W[i]; g.w_row_bytes[i] = w_row_bytes[i]; g.Y[i] = Y[i]; g.M[i] = (int)M[i]; g.bias[i] = bias ? bias[i] : nullptr;
    }
    if (why) { cdna4_set_error_msg(why); return -2; }
    return cdna4_launch_gemv_q_fused_grp(type, g, n, X, (hipStream_t)stream);
}
// the integer-dot kernels apply the tail where the element is reduced, and so do k_gemm_kq_t64 / k_gemm_r8 and the 128 x 128-tile kernels outside their
// atomic-sum split; the older MFMA GEMM kernels write the product first (k_epilogue behind them).  The call re-checks with the real pointers.
int ggml_cdna4_mul_mat_fused_residual_may_alias(int type, int64_t M, int64_t K, int64_t B) { return plan_query(type, M, K, B).tail_in_store ? 1 : 0; }
// the route of the AUTO call on the current device, host logic only (the numbers: include/ggml_cdna4.h; 11 = ONE launch, the quantizer inside k_gemm_kq_t64)
int ggml_cdna4_mul_mat_route(int type, int64_t M, int64_t K, int64_t B) { return plan_query(type, M, K, B).route_id; }
// the same for a concrete weight matrix: what the call on THIS matrix launches, given its alignment, row stride and resident image
int ggml_cdna4_mul_mat_route_of(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, int64_t B) {
    if (!W || w_row_bytes < (int64_t)ggml_cdna4_row_size(type, K)) return 0;
    return plan_query(type, W, w_row_bytes, M, K, B).route_id;
}
// the checks ggml_cdna4_mul_mat_fused and its pre-quantized twin (X == nullptr) share: 0, or the error status
static int fused_tail_ok(int type, const void *W, int64_t w_row_bytes, const float *X, int64_t x_row_stride, float *Y, int64_t y_row_stride,
                         int64_t M, int64_t K, int64_t B, int act, const float *residual, int64_t residual_row_stride, const void *workspace) {
    if (act != 0 && act != 1) return cdna4_set_error_msg("mul_mat_fused: act is 0 (none) or 1 (GELU)");
    if (residual && M > 0 && B > 0) {
        const char *r0 = (const char *)residual, *r1 = (const char *)(residual + (B - 1) * residual_row_stride + M);
        const char *y0 = (const char *)Y, *y1 = (const char *)(Y + (B - 1) * y_row_stride + M);
        const bool overlap = r0 < y1 && y0 < r1, exact = residual == Y && residual_row_stride == y_row_stride;
        // an exact alias needs the tail in the store: by the shape (what the query told the caller) and with these pointers (aligned rows)
        if (overlap && !(exact && plan_query(type, M, K, B).tail_in_store &&
                         plan_mul_mat(type, W, w_row_bytes, X, x_row_stride, M, K, B, GGML_CDNA4_PATH_AUTO, 0, 0, workspace).tail_in_store))
            return cdna4_set_error_msg("mul_mat_fused: residual overlaps Y (only an exact alias is allowed, and only where "
                                       "ggml_cdna4_mul_mat_fused_residual_may_alias says so)");
    }
    return 0;
}
int ggml_cdna4_mul_mat_fused(int type, const void *W, int64_t w_row_bytes, const float *X, int64_t x_row_stride, float *Y, int64_t y_row_stride,
                             int64_t M, int64_t K, int64_t B, const float *bias, int act, const float *residual, int64_t residual_row_stride,
                             void *workspace, size_t workspace_bytes, void *stream) {
    if (const int frc = fault_status()) return frc;
    if (const int rc = fused_tail_ok(type, W, w_row_bytes, X, x_row_stride, Y, y_row_stride, M, K, B, act, residual, residual_row_stride, workspace)) return rc;
    cdna4_epilogue e{}; e.bias = bias; e.resid = residual; e.resid_row_stride = residual_row_stride; e.act = act;
    return mul_mat_impl(type, W, w_row_bytes, X, x_row_stride, Y, y_row_stride, M, K, B, workspace, workspace_bytes, GGML_CDNA4_PATH_AUTO, 0, 0, e, stream);
}
// ---- the graph-level hand-off of quantized activations (round 5).  A transformer layer multiplies the SAME activations by several weight matrices
// (wq / wk / wv; w_gate / w_up): the CPU backend quantizes src1 once per MUL_MAT node (ggml-cpu.c:7490-7509) and so did every ggml_cdna4_mul_mat call.  A host that knows
// the activations have not changed since the previous call on this workspace asks for the key of the image each call leaves there; equal non-zero keys (and equal X, row
// stride, K, B) mean the second call can be ggml_cdna4_mul_mat_prepared[_fused] with path AUTO — the same kernels on the same image, bit-identical, one launch fewer.
//   0: the call leaves no reusable image (one-launch decode / few-row forms quantize inside the kernel; re-encoded formats on the int8 matrix cores use their target's image)
uint32_t ggml_cdna4_act_image_key(int type, int64_t M, int64_t K, int64_t B) { return plan_query(type, M, K, B).image_key; }
// the key of the call on a CONCRETE weight matrix: rows the int8 matrix-core kernel cannot read take a GEMV form, which names no image
uint32_t ggml_cdna4_act_image_key_of(int type, const void *W, int64_t w_row_bytes, int64_t M, int64_t K, int64_t B) {
    return plan_query(type, W, w_row_bytes, M, K, B).image_key;
}
// NORM / RMS_NORM [* gain] [+ shift] that ALSO leaves, in `workspace`, the activation image a following ggml_cdna4_mul_mat(type, .., X = dst, K = dst->ne[0], B = its rows)
// would build — for the calls whose ggml_cdna4_act_image_key is the K-quants' fp16 GEMM image (19): the MUL_MATs of dst then run ggml_cdna4_mul_mat_prepared[_fused] and
// the graph pays no quantizer launch for them at all.  dst's fp32 rows are written exactly as ggml_cdna4_op_norm_affine writes them; the image is bit-identical to
// ggml_cdna4_prepare_act's.  Rows of 256 .. 8192 values, dst rows contiguous ([B][K]).
static int norm_affine_act(const ggml_cdna4_tensor *src0, const ggml_cdna4_tensor *gain, const ggml_cdna4_tensor *shift, const ggml_cdna4_tensor *dst, float eps, int rms,
                           int type, void *workspace, size_t workspace_bytes, void *stream, bool kq);
int ggml_cdna4_op_norm_affine_q8_K(const ggml_cdna4_tensor *src0, const ggml_cdna4_tensor *gain, const ggml_cdna4_tensor *shift, const ggml_cdna4_tensor *dst, float eps, int rms,
                                   int type, void *workspace, size_t workspace_bytes, void *stream) {
    if (!cdna4_type_is_kq(type) || cdna4_convert_weights_kmul(type) != 1) return cdna4_set_error_msg("norm_q8_K: the image is the K-quants' (Q8_K activations, single image)");
    return norm_affine_act(src0, gain, shift, dst, eps, rms, type, workspace, workspace_bytes, stream, true);
}
// the same for the 32-block formats whose activations are Q8_0 (Q4_0 / Q8_0 / Q5_0 / IQ4_NL; ggml_cdna4_act_image_key == 17): the image of k_quantize_q8_0, bit for bit
int ggml_cdna4_op_norm_affine_q8_0(const ggml_cdna4_tensor *src0, const ggml_cdna4_tensor *gain, const ggml_cdna4_tensor *shift, const ggml_cdna4_tensor *dst, float eps, int rms,
                                   int type, void *workspace, size_t workspace_bytes, void *stream) {
    if (!cdna4_type_qk(type) || cdna4_type_is_kq(type) || cdna4_is_q81(type) || cdna4_convert_weights_kmul(type) != 1) return cdna4_set_error_msg("norm_q8_0: the image is the 32-block formats' (Q8_0 activations, single image)");
    return norm_affine_act(src0, gain, shift, dst, eps, rms, type, workspace, workspace_bytes, stream, false);
}
static int norm_affine_act(const ggml_cdna4_tensor *src0, const ggml_cdna4_tensor *gain, const ggml_cdna4_tensor *shift, const ggml_cdna4_tensor *dst, float eps, int rms,
                           int type, void *workspace, size_t workspace_bytes, void *stream, bool kq) {
    const int64_t K = dst->ne[0], B = dst->ne[1] * dst->ne[2] * dst->ne[3];
    if (K <= 0 || B <= 0 || K % (kq ? 256 : 32)) return cdna4_set_error_msg("norm + activation image: rows of whole blocks");
    if (dst->nb[1] != K * 4 || (dst->ne[2] > 1 && dst->nb[2] != dst->ne[1] * dst->nb[1]) || (dst->ne[3] > 1 && dst->nb[3] != dst->ne[2] * dst->nb[2])) return cdna4_set_error_msg("norm_q8_K: dst rows must be contiguous");
    if (!workspace || ((uintptr_t)workspace & 255)) return cdna4_set_error_msg("norm_q8_K: workspace must be 256-byte aligned");
    const ws_view v = carve(type, K, B, workspace);
    if (workspace_bytes < v.total) return cdna4_set_error_msg("norm_q8_K: workspace too small");
    return cdna4_launch_norm_affine_q8_K(src0, gain, shift, dst, eps, rms, v.xh, stream, kq ? 1 : 0);
}
// ggml_cdna4_mul_mat_fused on the image the previous call left in `workspace` (ggml_cdna4_act_image_key)
int ggml_cdna4_mul_mat_prepared_fused(int type, const void *W, int64_t w_row_bytes, float *Y, int64_t y_row_stride, int64_t M, int64_t K, int64_t B,
                                      const float *bias, int act, const float *residual, int64_t residual_row_stride,
                                      const void *workspace, size_t workspace_bytes, void *stream) {
    if (const int frc = fault_status()) return frc;
    if (const int rc = fused_tail_ok(type, W, w_row_bytes, nullptr, 0, Y, y_row_stride, M, K, B, act, residual, residual_row_stride, workspace)) return rc;
    if (!plan_query(type, M, K, B).image_key) return cdna4_set_error_msg("mul_mat_prepared_fused: a call of this shape has no prepared form (ggml_cdna4_act_image_key == 0)");
    cdna4_epilogue e{}; e.bias = bias; e.resid = residual; e.resid_row_stride = residual_row_stride; e.act = act;
    return mul_mat_impl(type, W, w_row_bytes, nullptr, 0, Y, y_row_stride, M, K, B, (void *)workspace, workspace_bytes, GGML_CDNA4_PATH_AUTO, 0, 0, e, stream);
}

}  // extern "C"

// ---- The routing plan of a MUL_MAT_ID (mul_mat_id_plan.hpp): the ONE place that decides which launches a call takes.  ggml_cdna4_mul_mat_id and its
// `prepared` twin execute it, ggml_cdna4_mul_mat_id_front_key reads its key: change the routing here and nowhere else.
struct mmid_knobs {                               // read once per process
    bool sk_off;                                  // CDNA4_MOE_SK=0: the per-tile launches instead of the work-queue form
    bool no_mmq_ids, mmq_ids_all;                 // CDNA4_NO_MMQ_IDS=1: no int8 matrix-core route; CDNA4_MMQ_IDS=2 (coverage / measurement): that route for Q4_K too, in front of the work queue
    // cost of one (tile, m-tile, superblock) unit by the tile's fragments in use (1 .. 4), relative.  FLAT, by measurement: the k loop is bound by its unpack /
    // issue work, which does not depend on the fragments — a tile with one fragment in use takes 1.78-1.91 us per superblock, a full one 1.86-1.92
    // (profiles/r06/moe_sk_trace_*.txt), with or without the activation DMA of the empty fragments; weights that call light tiles cheaper lost: 8 x 2 x 512 x 4096^2,
    // us per call, one box: 10,10,10,10 72.2 | 8,9,10,10 79.8 | 7,8,9,10 85.0 | 6,8,9,10 90.7 | 5,7,9,10 98.1 | 4,6,8,10 107.6 (CDNA4_SK_CW=a,b,c,d: measurement knob)
    int cw[4];
    mmid_knobs() : cw{10, 10, 10, 10} {
        const auto num = [](const char *e, int dflt) { return e ? atoi(e) : dflt; };
        sk_off = num(getenv("CDNA4_MOE_SK"), 1) == 0; no_mmq_ids = num(getenv("CDNA4_NO_MMQ_IDS"), 0) != 0; mmq_ids_all = num(getenv("CDNA4_MMQ_IDS"), 0) == 2;
        int t4[4]; const char *ev = getenv("CDNA4_SK_CW");
        if (ev && sscanf(ev, "%d,%d,%d,%d", &t4[0], &t4[1], &t4[2], &t4[3]) == 4 && t4[0] > 0 && t4[1] > 0 && t4[2] > 0 && t4[3] > 0 && t4[3] < 256) for (int i = 0; i < 4; i++) cw[i] = t4[i];
    }
};
static const char *const mmid_no_front = "mul_mat_id_prepared: a call of this shape leaves no front (ggml_cdna4_mul_mat_id_front_key == 0)";
mmid_plan mmid_make_plan(const mmid_call &c, bool front_in_place) {
    static const mmid_knobs knobs;
    mmid_plan p{};
    p.w_type = c.type; p.W = (const uint8_t *)c.as; p.w_row_bytes = c.w_row_bytes; p.w_expert_bytes = c.w_expert_bytes;
    const auto refuse = [&p](int rc, const char *msg) { p.kind = MMID_REFUSED; p.rc = rc; p.err = msg; return p; };
    const int type = c.type; const int64_t M = c.M, K = c.K, pairs = c.n_tok * c.n_used;
    const uintptr_t w_bits = (uintptr_t)c.as | (uintptr_t)c.w_row_bytes | (uintptr_t)c.w_expert_bytes, b_bits = (uintptr_t)c.b | (uintptr_t)(c.b_row_stride * 4);
    const bool kq = cdna4_type_is_kq(type), w16 = !(w_bits & 15), ws_ok = c.workspace && !((uintptr_t)c.workspace & 255);
    // prefill-sized mixture-of-experts batches: group the (token, slot) rows by expert on the device and run ONE MFMA GEMM launch over
    // the (expert, activation tile) table — every expert's weights are read once per m-tile instead of once per column
    // (ggml_compute_forward_mul_mat_id groups the same way on the host: ggml-cpu.c:7648-7781)
    const bool big = cdna4_type_qk(type) && M > 0 && K > 0 && c.n_tok > 0 && c.n_used > 0 && c.n_b > 0 && c.n_used % c.n_b == 0 && ggml_cdna4_row_size(type, K) != 0 &&
                     cdna4_gemm_ids_supported(type, K) && pairs > 32 && c.n_expert <= 1024 && !(w_bits & 1);
    // the resident Q4_0R image of a Q4_0 expert stack (ggml's 3-D expert tensor: the experts' rows back to back; found by the stack's pointer, like ggml_cdna4_mul_mat finds a
    // matrix's), or nullptr: with it the stack runs on Q4_K's grouped kernels (row stride (K / 256) * 144)
    const uint8_t *img = big && type == CDNA4_Q4_0 && K % 256 == 0 && c.w_expert_bytes == M * c.w_row_bytes ? cdna4_resident_lookup(CDNA4_Q4_0, c.as, c.w_row_bytes, M * c.n_expert, K) : nullptr;
    if ((uintptr_t)img & 15) img = nullptr;
    const auto reads_image = [&p, img, M, K] { p.w_type = CDNA4_Q4_0R; p.W = img; p.w_row_bytes = (K / 256) * 144; p.w_expert_bytes = M * p.w_row_bytes; };
    // Q4_K experts, and Q4_0 experts whose stack has a RESIDENT Q4_0R image: the work-queue (stream-k) form — TWO launches (planner + token-order quantizer; one persistent
    // grouped GEMM that gathers its rows), round 6.  By everything but b, the strides and the workspace pointer: what the key answers from
    const moe_sk_view sv = moe_sk_carve(K, c.n_expert, c.n_used, c.n_b, c.n_tok, nullptr);
    const bool queue = big && mmid_queue_shape(type, K, c.n_expert) && (img || (type == CDNA4_Q4_K && w16)) && !knobs.sk_off && !(knobs.mmq_ids_all && pairs <= 32 * c.n_expert) &&
                       cdna4_gemm_sk_supported(img ? CDNA4_Q4_0R : CDNA4_Q4_K, M, K, sv.n_rows, sv.ntile_cap) && c.workspace_bytes >= sv.total;
    if (front_in_place && !queue) return refuse(-2, mmid_no_front);
    if (!cdna4_type_qk(type)) return refuse(-1, "mul_mat_id: unsupported weight type");
    if (M <= 0 || c.n_tok <= 0 || c.n_used <= 0) { p.kind = MMID_EMPTY; return p; }
    if (K <= 0 || ggml_cdna4_row_size(type, K) == 0) return refuse(-1, "mul_mat_id: K is not a whole number of blocks");
    if (c.n_b <= 0 || c.n_used % c.n_b) return refuse(-1, "mul_mat_id: n_used must be a multiple of b.ne[1]");   // ggml_mul_mat_id: ids->ne[0] % b->ne[1] == 0 (src/ggml.c:2747); slot u reads row u % n_b
    if (c.dst_tok_stride != c.n_used * c.dst_row_stride) return refuse(-1, "mul_mat_id: dst must be contiguous over (slot, token)");
    if (c.b_tok_stride != c.n_b * c.b_row_stride) return refuse(-1, "mul_mat_id: b must be contiguous over (row, token)");
    const bool grouped = big && ws_ok && !(b_bits & 15);
    if (front_in_place && !grouped) return refuse(-2, "mul_mat_id_prepared: misaligned operands");
    if (grouped && queue) {
        p.kind = MMID_QUEUE; p.ws_need = sv.total; p.rows = sv.n_rows; p.ntile_cap = sv.ntile_cap; p.front_in_place = front_in_place;
        if (img) reads_image();
        p.G = cdna4_gemm_sk_spans(); p.upt = ((M + 127) / 128) * (K / 256);
        for (int i = 0; i < 4; i++) p.cw[i] = knobs.cw[i];
        p.front_key = 0x4D510000u | (img ? 2u : 1u);                    // (the image's activation class; the rest of what the front depends on is what the caller compares)
        return p;
    }
    const moe_view mv = moe_carve(K, c.n_expert, c.n_used, c.n_tok, nullptr);
    if (grouped && c.workspace_bytes >= mv.total && mv.img_rows * K * 2 < ((int64_t)1 << 31)) {      // (a workspace below that: the GEMV forms)
        p.ws_need = mv.total; p.rows = mv.img_rows;
        // few rows per expert (on average at most 32): the int8 matrix-core kernel over 32-row chunks of the same expert-sorted image — the CPU's own integer
        // block dots (ggml_compute_forward_mul_mat_id's vec_dot calls, ggml-cpu.c:7752-7776) instead of fp16 tiles that would be mostly padding.  The int8
        // image (quants, d, bsums) takes the place of the fp16 one in the workspace.  Where it wins (MI355X, one box, 8 experts x 2 used x 4096^2, us per call at
        // 32 / 64 / 128 tokens, profiles/r04/moe64_ab.txt): Q6_K 95 / 96 / 125 vs 158 / 158 / 160 and Q8_0 91 / 92 / 133 vs 144 / 144 / 147 on the grouped per-lane-load
        // GEMM these formats have; NOT Q4_K, whose grouped k_gemm_kq_t64 takes 45 / 46 / 51 against 82 / 83 / 115 (CDNA4_MMQ_IDS=2 forces it there: 2e-7 from the
        // oracle instead of 3e-4).  CDNA4_NO_MMQ_IDS=1 turns the route off.
        if (!knobs.no_mmq_ids && (type != CDNA4_Q4_K || knobs.mmq_ids_all) && pairs <= 32 * c.n_expert && cdna4_mmq_ids_supported(type, K) && !(w_bits & (type == CDNA4_Q6_K ? 1 : 15))) {
            p.kind = MMID_TILES_MMQ;
        } else if (img || (type == CDNA4_Q4_K && w16)) {                 // Q4_0 experts with a resident image of the whole stack: Q4_K's grouped kernel (round 5)
            p.kind = MMID_TILES_T64; p.t64 = t64_ids_make_plan((int)M, (int)K, (int)mv.img_rows);
            if (img) reads_image();
        } else {                                                          // Q5_K / Q6_K / Q4_0 / Q8_0, and Q4_K rows the 16-byte loads cannot take
            p.kind = MMID_TILES_KQ; p.wlds = cdna4_gemm_ids_wlds(type, c.as, c.w_row_bytes, c.w_expert_bytes);
        }
        return p;
    }
    // the GEMV forms, column c = (token, slot).  One token: one launch, the activation quantizer runs inside the GEMV
    const bool one = c.n_tok == 1 && c.n_used <= 65535 && cdna4_gemv_fused_supported(type, K, 1) && !(b_bits & 15);
    if (!one) {
        if (!ws_ok) return refuse(-1, "mul_mat_id: workspace must be 256-byte aligned");
        p.ws_need = carve(type, K, c.n_tok * c.n_b, nullptr).total; p.rows = c.n_tok * c.n_b;
        if (c.workspace_bytes < p.ws_need) return refuse(-1, "mul_mat_id: workspace too small");
        if (b_bits & 15) return refuse(-1, kq ? "quantize_q8_K: x must be 16-byte aligned" : (cdna4_is_q81(type) ? "quantize_q8_1: x must be 16-byte aligned" : "quantize_q8_0: x must be 16-byte aligned"));
    }
    // (what the activation quantizers and the GEMV launchers refuse, named here so that the call fails in front of its quantizer launch, not behind it.  The launchers
    //  remain the authority — ggml_cdna4_quantize_q8_* above, gemv_q.hip: cdna4_launch_gemv_q / _fused_ids, gemv_operands_ok — and keep their checks: these lines must MIRROR
    //  them, message for message; the property test over the call grid compares the plan's refusal with what the call answers)
    if (((uintptr_t)c.as | (uintptr_t)c.w_row_bytes | (uintptr_t)(one ? c.w_expert_bytes : 0)) & 1) return refuse(-1, "gemv_q: misaligned operands");
    if (!one && pairs > 65535) return refuse(-1, "gemv_q: too many MUL_MAT_ID columns");
    if ((type == CDNA4_Q4_K || type == CDNA4_Q5_K) && !w16) return refuse(-1, "gemv_q: Q4_K/Q5_K rows must be 16-byte aligned");
    p.kind = one ? MMID_GEMV_1 : MMID_GEMV;
    return p;
}

static int mul_mat_id_impl(const mmid_call &c, bool front_in_place, void *stream) {
    if (const int frc = fault_status()) return frc;
    const mmid_plan p = mmid_make_plan(c, front_in_place);
    if (p.kind == MMID_REFUSED) { cdna4_set_error_msg(p.err); return p.rc; }
    hipStream_t st = (hipStream_t)stream;
    const bool kq = cdna4_type_is_kq(c.type);
    // the MUL_MAT_ID columns of a GEMV launch
    const auto gemv_ids = [&c](cdna4_gemv_args g) {
        g.ids = c.ids; g.ids_tok_stride = c.ids_tok_stride; g.w_expert_bytes = c.w_expert_bytes; g.n_used = (int)c.n_used; g.n_b = (int)c.n_b; g.n_expert = (int)c.n_expert;
        return g;
    };
    switch (p.kind) {
    case MMID_QUEUE: {
        const moe_sk_view sv = moe_sk_carve(c.K, c.n_expert, c.n_used, c.n_b, c.n_tok, c.workspace);
        // (prepared: the front of an earlier call with the same b, ids and shape is in place)
        if (!p.front_in_place)
            if (const int rc = cdna4_launch_moe_sk_front(c.ids, c.ids_tok_stride, (int)c.n_tok, (int)c.n_used, (int)c.n_b, (int)c.n_expert, (int)p.ntile_cap, (int)p.upt, p.G, p.cw,
                                                         sv.tile_rec, sv.wg_begin, c.b, c.b_row_stride, c.K, p.w_type == CDNA4_Q4_K, sv.xh, st)) return rc;
        const cdna4_gemm_args a = gemm_args_of(p.w_type, p.W, p.w_row_bytes, sv.xh, c.dst, c.dst_row_stride, c.M, c.K, p.rows, 0, 0, cdna4_epilogue{});
        return cdna4_launch_gemm_sk(a, sv.tile_rec, sv.wg_begin, p.G, p.w_expert_bytes, st);
    }
    case MMID_TILES_MMQ: case MMID_TILES_T64: case MMID_TILES_KQ: {
        const moe_view mv = moe_carve(c.K, c.n_expert, c.n_used, c.n_tok, c.workspace);
        int rc = cdna4_launch_moe_plan(c.ids, c.ids_tok_stride, (int)c.n_tok, (int)c.n_used, (int)c.n_b, (int)c.n_expert, (int)mv.img_rows, mv.img_src, mv.img_dst, mv.tile_expert, st);
        if (rc) return rc;
        if (p.kind == MMID_TILES_MMQ) {
            ws_view iv{};                                                // the int8 image: [qs][d][bsums (K-quants)]
            iv.qs = (int8_t *)mv.xh;
            iv.d = (float *)((uint8_t *)mv.xh + align256((size_t)mv.img_rows * c.K));
            iv.bsums = kq ? (int16_t *)((uint8_t *)iv.d + align256((size_t)mv.img_rows * (c.K / 32) * 4)) : nullptr;
            rc = kq ? cdna4_launch_quantize_q8_K_gather_i8(c.b, c.b_row_stride, c.K, mv.img_rows, mv.img_src, iv.qs, iv.d, iv.bsums, st)
                    : cdna4_launch_quantize_q8_0_gather_i8(c.b, c.b_row_stride, c.K, mv.img_rows, mv.img_src, iv.qs, iv.d, st);
            if (rc) return rc;
            return cdna4_launch_mmq_ids(gemv_args_of(p.w_type, p.W, p.w_row_bytes, iv, c.dst, c.dst_row_stride, c.M, c.K, mv.img_rows, cdna4_epilogue{}), mv.tile_expert, mv.img_dst, p.w_expert_bytes, st);
        }
        rc = kq ? cdna4_launch_quantize_q8_K_gather(c.b, c.b_row_stride, c.K, mv.img_rows, mv.img_src, mv.xh, st)
                : cdna4_launch_quantize_q8_0_gather(c.b, c.b_row_stride, c.K, mv.img_rows, mv.img_src, mv.xh, st);
        if (rc) return rc;
        const cdna4_gemm_args a = gemm_args_of(p.w_type, p.W, p.w_row_bytes, mv.xh, c.dst, c.dst_row_stride, c.M, c.K, mv.img_rows, 0, 0, cdna4_epilogue{});
        return p.kind == MMID_TILES_T64 ? cdna4_launch_gemm_t64_ids(a, mv.tile_expert, mv.img_dst, p.w_expert_bytes, st) : cdna4_launch_gemm_ids(a, mv.tile_expert, mv.img_dst, p.w_expert_bytes, st);
    }
    case MMID_GEMV_1:
        return cdna4_launch_gemv_q_fused_ids(gemv_ids(gemv_args_of(c.type, c.as, c.w_row_bytes, ws_view{}, c.dst, c.dst_row_stride, c.M, c.K, c.n_used, cdna4_epilogue{})), c.b, c.b_row_stride, st);
    case MMID_GEMV: {
        const ws_view v = carve(c.type, c.K, p.rows, c.workspace);
        if (const int rc = ggml_cdna4_prepare_act(c.type, c.b, c.b_row_stride, c.K, p.rows, c.workspace, c.workspace_bytes, GGML_CDNA4_PATH_GEMV, stream)) return rc;
        return cdna4_launch_gemv_q(gemv_ids(gemv_args_of(c.type, c.as, c.w_row_bytes, v, c.dst, c.dst_row_stride, c.M, c.K, c.n_tok * c.n_used, cdna4_epilogue{})), st);
    }
    default: return 0;                                                   // MMID_EMPTY
    }
}

extern "C" {

int ggml_cdna4_mul_mat_id(int type, const void *as, int64_t w_row_bytes, int64_t w_expert_bytes, const float *b, int64_t b_row_stride, int64_t b_tok_stride,
                          const int32_t *ids, int64_t ids_tok_stride, float *dst, int64_t dst_row_stride, int64_t dst_tok_stride,
                          int64_t M, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok,
                          void *workspace, size_t workspace_bytes, void *stream) {
    const mmid_call c = {type, as, w_row_bytes, w_expert_bytes, b, b_row_stride, b_tok_stride, ids, ids_tok_stride, dst, dst_row_stride, dst_tok_stride, M, K, n_expert, n_used, n_b, n_tok, workspace, workspace_bytes};
    return mul_mat_id_impl(c, false, stream);
}
// MUL_MAT_IDs of ONE (b, ids) — a mixture-of-experts layer's w_up and w_gate stacks (llama.cpp build_moe_ffn) — share everything the first launch of the work-queue form makes:
// the sorted ids, the tile records, the spans, the quantized activations.  Non-zero: a ggml_cdna4_mul_mat_id of this call leaves that FRONT in its workspace, and
// ggml_cdna4_mul_mat_id_prepared with other expert weights of the same type / M / K, the same b, ids, strides and counts, on the untouched workspace multiplies it again
// (ONE launch instead of two, bit-identical to the full call).  The key of the plan of this call on aligned, contiguous stand-ins for the operands it is not given.
uint32_t ggml_cdna4_mul_mat_id_front_key(int type, const void *as, int64_t w_row_bytes, int64_t w_expert_bytes, int64_t M, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok, size_t workspace_bytes) {
    const mmid_call c = {type, as, w_row_bytes, w_expert_bytes, (const float *)(uintptr_t)256, K, n_b * K, nullptr, n_used, nullptr, M, n_used * M, M, K, n_expert, n_used, n_b, n_tok, (void *)(uintptr_t)256, workspace_bytes};
    return mmid_make_plan(c, false).front_key;
}
int ggml_cdna4_mul_mat_id_prepared(int type, const void *as, int64_t w_row_bytes, int64_t w_expert_bytes, const float *b, int64_t b_row_stride, int64_t b_tok_stride,
                                   const int32_t *ids, int64_t ids_tok_stride, float *dst, int64_t dst_row_stride, int64_t dst_tok_stride,
                                   int64_t M, int64_t K, int64_t n_expert, int64_t n_used, int64_t n_b, int64_t n_tok,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    const mmid_call c = {type, as, w_row_bytes, w_expert_bytes, b, b_row_stride, b_tok_stride, ids, ids_tok_stride, dst, dst_row_stride, dst_tok_stride, M, K, n_expert, n_used, n_b, n_tok, workspace, workspace_bytes};
    // (no front: answered in front of the fault status, like the key itself)
    if (!ggml_cdna4_mul_mat_id_front_key(type, as, w_row_bytes, w_expert_bytes, M, K, n_expert, n_used, n_b, n_tok, workspace_bytes)) { cdna4_set_error_msg(mmid_no_front); return -2; }
    return mul_mat_id_impl(c, true, stream);
}

}  // extern "C"
