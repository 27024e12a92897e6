// lib_emul_main.cpp — driver of the whole-library emulation build (lib_emul.h): calls the library's C-ABI like a host would.  Test infrastructure.
//   lib_emul mul_mat type M K B path w.bin x.bin y.bin          ggml_cdna4_mul_mat (path 0 = auto, 1 = GEMV, 2 = GEMM); w = M contiguous rows, x = [B][K] f32, y = [B][M]
//   lib_emul mul_mat_id type M K n_expert n_used n_b n_tok w.bin x.bin ids.bin y.bin
//   lib_emul plan < calls                                      the prefill GEMM's routing plans (gemm_q_plan.hpp), no kernel runs: see below
//   lib_emul plan_id < calls                                   MUL_MAT_ID's routing plans (mul_mat_id_plan.hpp), likewise
#include "lib_emul.h"
#include "../../include/ggml_cdna4.h"
#include "gemm_q_plan.hpp"
#include "mul_mat_id_plan.hpp"
#include <string>
int cdna4_set_error_msg(const char *msg);

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx;
dim3 g_gridDim, g_blockDim;
pthread_barrier_t g_wg_barrier;
WaveState *g_waves;
thread_local std::vector<Pending> t_vmq;
bool g_defer_dma = getenv("EMU_DEFER_DMA") && atoi(getenv("EMU_DEFER_DMA")) != 0;
size_t g_weaken = getenv("EMU_WEAKEN_WAITS") ? (size_t)atoi(getenv("EMU_WEAKEN_WAITS")) : 0;      // self-test of the counted waits: every wait tolerates this many more outstanding operations
}
__attribute__((aligned(16))) uint8_t smem[160 * 1024];             // the dynamic LDS of gemv_q.hip's kernels (a work-group is a process)
void *emu_shared_alloc(size_t n) {                                   // between two inaccessible pages, shared with the work-group processes
    const size_t pg = 4096, body = (n + pg - 1) / pg * pg;
    char *p = (char *)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) { perror("mmap"); exit(2); }
    mprotect(p, pg, PROT_NONE); mprotect(p + pg + body, pg, PROT_NONE);
    return p + pg + ((body - n) & ~(size_t)255);                     // 256-byte aligned like hipMalloc; the rear guard page at most 255 bytes away
}
static void *load(const char *path, size_t *n_out = nullptr) {
    FILE *f = fopen(path, "rb"); if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    void *p = emu_shared_alloc((size_t)n + 16); if (fread(p, 1, (size_t)n, f) != (size_t)n) exit(2); fclose(f);
    if (n_out) *n_out = (size_t)n;
    return p;
}
static void store(const char *path, const void *p, size_t n) { FILE *f = fopen(path, "wb"); fwrite(p, 1, n, f); fclose(f); }

int main(int argc, char **argv) {
    if (argc >= 10 && !strcmp(argv[1], "mul_mat")) {
        const int type = atoi(argv[2]); const int64_t M = atoll(argv[3]), K = atoll(argv[4]), B = atoll(argv[5]); const int path = atoi(argv[6]);
        size_t wn = 0; void *w = load(argv[7], &wn); float *x = (float *)load(argv[8]);
        float *y = (float *)emu_shared_alloc((size_t)(M * B) * 4);
        for (int64_t i = 0; i < M * B; i++) y[i] = -12345.f;
        const size_t wsn = ggml_cdna4_mul_mat_workspace_size(type, K, B);
        void *ws = emu_shared_alloc(wsn ? wsn : 256);
        // EMU_RESIDENT=1: with a resident kernel-native image of the weights registered first (built twice and compared, like a host does at load) where the type has one
        if (getenv("EMU_RESIDENT") && atoi(getenv("EMU_RESIDENT")) != 0) {
            const size_t in = ggml_cdna4_resident_image_size(type, M, K);
            if (in) {
                void *img = emu_shared_alloc(in);
                if (ggml_cdna4_resident_image_register(type, w, (int64_t)(wn / (size_t)M), M, K, img, 1, nullptr)) { fprintf(stderr, "resident_image_register: %s\n", ggml_cdna4_last_error()); return 1; }
                const int route = ggml_cdna4_mul_mat_route_of(type, w, (int64_t)(wn / (size_t)M), M, K, B);
                fprintf(stderr, "resident image registered: route %d\n", route);
                // EMU_DEFER_DMA=2: defer only on the kernels whose every wait is a counted vmcnt in the source (k_gemm_kq_t64 = 10, k_gemm_r8 = 12).  The staged forms of
                // k_gemm_kq_w12 rely on the compiler's own wait for their loader waves' register loads (everything older — the activation pieces — has landed with them):
                // the emulation completes plain loads at once and has no such wait to retire the deferred copies
                if (getenv("EMU_DEFER_DMA") && atoi(getenv("EMU_DEFER_DMA")) == 2 && route != 10 && route != 12) emu::g_defer_dma = false;
            }
        }
        else if (getenv("EMU_DEFER_DMA") && atoi(getenv("EMU_DEFER_DMA")) == 2) emu::g_defer_dma = false;
        const int rc = ggml_cdna4_mul_mat(type, w, (int64_t)(wn / (size_t)M), x, K, y, M, M, K, B, ws, wsn, path, 0, 0, nullptr);
        if (rc) { fprintf(stderr, "mul_mat: %s\n", ggml_cdna4_last_error()); return 1; }
        store(argv[9], y, (size_t)(M * B) * 4);
        return 0;
    }
    if (argc >= 13 && !strcmp(argv[1], "mul_mat_id")) {
        const int type = atoi(argv[2]); const int64_t M = atoll(argv[3]), K = atoll(argv[4]), NE = atoll(argv[5]), NU = atoll(argv[6]), NB = atoll(argv[7]), NT = atoll(argv[8]);
        size_t wn = 0; void *w = load(argv[9], &wn); float *x = (float *)load(argv[10]); int32_t *ids = (int32_t *)load(argv[11]);
        float *y = (float *)emu_shared_alloc((size_t)(M * NU * NT) * 4);
        for (int64_t i = 0; i < M * NU * NT; i++) y[i] = -12345.f;
        const size_t wsn = ggml_cdna4_mul_mat_id_workspace_size(type, K, NE, NU, NB, NT);
        void *ws = emu_shared_alloc(wsn ? wsn : 256);
        const int64_t rb = (int64_t)(wn / (size_t)(M * NE));
        if (getenv("EMU_RESIDENT") && atoi(getenv("EMU_RESIDENT")) != 0) {      // a resident image of the whole expert stack (M * NE rows)
            const size_t in = ggml_cdna4_resident_image_size(type, M * NE, K);
            if (in) {
                void *img = emu_shared_alloc(in);
                if (ggml_cdna4_resident_image_register(type, w, rb, M * NE, K, img, 1, nullptr)) { fprintf(stderr, "resident_image_register: %s\n", ggml_cdna4_last_error()); return 1; }
            }
        }
        const int rc = ggml_cdna4_mul_mat_id(type, w, rb, rb * M, x, K, NB * K, ids, NU, y, M, NU * M, M, K, NE, NU, NB, NT, ws, wsn, nullptr);
        if (rc) { fprintf(stderr, "mul_mat_id: %s\n", ggml_cdna4_last_error()); return 1; }
        store(argv[12], y, (size_t)(M * NU * NT) * 4);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        // one line per call read from stdin, "type M K B splitk variant w_offset xf image": the prefill GEMM's plan (gemm_q_make_plan) as field=value, made twice (`pure`: both
        // equal and ggml_cdna4_last_error untouched), then what cdna4_launch_gemm_q answers with every launch a no-op (rc, and the message behind `|`).  Operands are addresses
        // without memory behind them: W = 4096 + w_offset (image != 0: with a resident image registered for it), the activation image and — xf != 0 — the fp32 rows aligned
        setenv("EMU_NO_RUN", "1", 1);
        auto line_of = [](const gemm_q_plan &pl) {
            static const char *src[] = {"given", "resident", "reencoded", "relaid"}, *term[] = {"none", "t64", "r8", "w8", "kq"};
            const bool t = pl.terminal == GQ_T64, r = pl.terminal == GQ_R8, w = pl.terminal == GQ_W8, q = pl.terminal == GQ_KQ;
            const int tiles_w8 = ((pl.k.M + 127) / 128) * ((pl.k.B + 127) / 128);
            char b[512];
            snprintf(b, sizeof b, "ok=%d kernel=%d route=%d reenc=%d tail=%d fq=%d src=%s wtype=%d wrow=%lld kmul=%d term=%s tm=%d splitk=%d ntiles=%d ticketed=%d waits=%d zero=%d opt=%d sb_split=%d xchg_l2=%d",
                     !pl.err, pl.kernel, gemm_q_route_id(pl), (int)pl.reencoded, (int)pl.tail_in_store, (int)pl.fuses_quantizer, src[pl.source], w ? pl.w8.type : pl.k.type, (long long)pl.k.w_row_bytes, pl.kmul,
                     pl.err ? "none" : term[pl.terminal], t ? pl.t64.tm : (r ? pl.r8.tm : (w || q ? 128 : 0)), t ? pl.t64.splitk : (r ? pl.r8.splitk : (w ? pl.w8.splitk : (q ? pl.kq.splitk : 0))),
                     t ? pl.t64.ntiles : (r ? pl.r8.ntiles : (w || q ? tiles_w8 : 0)), t ? (int)pl.t64.ticketed2 : (w ? (int)pl.w8.ticketed : 0),
                     t ? (pl.t64.fq || (pl.t64.splitk == 2 && !pl.t64.ticketed2)) : (r ? pl.r8.splitk > 1 : (w ? pl.w8.exchange && !pl.w8.ticketed : 0)),
                     w ? (pl.w8.splitk > 1 && !pl.w8.exchange) : (q ? pl.kq.splitk > 1 : 0), w ? pl.w8.opt : 0, w ? pl.w8.sb_split : 0, w ? pl.w8.xchg_l2 : 0);
            return std::string(b);
        };
        char in[256];
        while (fgets(in, sizeof in, stdin)) {
            long long v[9] = {0};
            if (sscanf(in, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) < 6) continue;
            cdna4_gemm_args a{};
            a.type = (int)v[0]; a.M = (int)v[1]; a.K = (int)v[2]; a.B = (int)v[3]; a.splitk = (int)v[4]; a.variant = (int)v[5];
            a.W = (const uint8_t *)(uintptr_t)(4096 + v[6]); a.w_row_bytes = (int64_t)ggml_cdna4_row_size(a.type, a.K);
            a.xh = (const void *)(uintptr_t)(1 << 20); a.xh_row_elems = a.K; a.y_row_elems = a.M;
            if (v[7]) { a.xf = (const float *)(uintptr_t)(1 << 21); a.xf_row_elems = a.K; }
            if (v[8]) cdna4_resident_register(a.type, a.W, a.w_row_bytes, a.M, a.K, (const void *)(uintptr_t)(1 << 22));
            cdna4_set_error_msg("untouched");
            const std::string l1 = line_of(gemm_q_make_plan(a)), l2 = line_of(gemm_q_make_plan(a));
            const bool pure = l1 == l2 && !strcmp(ggml_cdna4_last_error(), "untouched");
            const gemm_q_plan pl = gemm_q_make_plan(a);
            const int rc = cdna4_launch_gemm_q(a, nullptr);
            printf("%s pure=%d plan_err=%d rc=%d | %s\n", l1.c_str(), (int)pure, (int)(pl.err != nullptr && !strcmp(pl.err, ggml_cdna4_last_error())), rc, rc ? ggml_cdna4_last_error() : "");
            if (v[8]) cdna4_resident_unregister(a.W);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "plan_id")) {
        // one line per call, "type M K n_expert n_used n_b n_tok as_offset b_offset ws_offset ws_bytes image prepared [dst_gap b_gap]": MUL_MAT_ID's plan (mmid_make_plan) as field=value, made
        // twice (`pure`), then what the call itself — ggml_cdna4_mul_mat_id, or its `prepared` twin — answers with every launch a no-op: rc, `plan_err` (the plan named the very
        // message the call failed with), the public front key, and the message behind `|`.  Operands are addresses without memory behind them, contiguous, at the given byte
        // offsets from aligned bases (the weights as `w=` are printed as an offset from their stack, or from the image); ws_bytes 0: what ggml_cdna4_mul_mat_id_workspace_size
        // says (printed as `size=`); image != 0: with a resident image of the stack registered; dst_gap / b_gap: elements between the tokens of dst / b
        setenv("EMU_NO_RUN", "1", 1);
        const uintptr_t as0 = (uintptr_t)1 << 40, img0 = (uintptr_t)2 << 40, b0 = (uintptr_t)3 << 40, ws0 = (uintptr_t)4 << 40, ids0 = (uintptr_t)5 << 40, dst0 = (uintptr_t)6 << 40;
        auto line_of = [&](const mmid_plan &made) {
            mmid_plan pl = made;                                        // (a refusal and an empty call name nothing else)
            if (made.kind == MMID_REFUSED || made.kind == MMID_EMPTY) { pl = mmid_plan{}; pl.kind = made.kind; pl.rc = made.rc; pl.W = (const uint8_t *)as0; }
            static const char *kind[] = {"empty", "refused", "queue", "tiles_mmq", "tiles_t64", "tiles_kq", "gemv_1", "gemv"};
            const bool q = pl.kind == MMID_QUEUE, t = pl.kind == MMID_TILES_T64;
            const uintptr_t w = (uintptr_t)pl.W;
            char b[512];
            snprintf(b, sizeof b, "kind=%s rc=%d wtype=%d w=%s%lld wrow=%lld wexp=%lld need=%zu rows=%lld G=%d upt=%lld cap=%lld cw=%d,%d,%d,%d front=%d tm=%d tables=%d split=%d wlds=%d key=%u",
                     kind[pl.kind], pl.rc, pl.w_type, w >= img0 ? "img+" : "as+", (long long)(w - (w >= img0 ? img0 : as0)), (long long)pl.w_row_bytes, (long long)pl.w_expert_bytes, pl.ws_need,
                     (long long)pl.rows, pl.G, (long long)pl.upt, (long long)pl.ntile_cap, pl.cw[0], pl.cw[1], pl.cw[2], pl.cw[3], q ? (pl.front_in_place ? 2 : 1) : 0,
                     t ? pl.t64.tm : 0, t ? (int)pl.t64.tables : 0, t ? pl.t64.splitk : 0, (int)pl.wlds, pl.front_key);
            return std::string(b);
        };
        char in[256];
        while (fgets(in, sizeof in, stdin)) {
            long long v[15] = {0};
            if (sscanf(in, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12, v + 13, v + 14) < 7) continue;
            mmid_call c{};
            c.type = (int)v[0]; c.M = v[1]; c.K = v[2]; c.n_expert = v[3]; c.n_used = v[4]; c.n_b = v[5]; c.n_tok = v[6];
            c.as = (const void *)(as0 + v[7]); c.w_row_bytes = (int64_t)ggml_cdna4_row_size(c.type, c.K); c.w_expert_bytes = c.M * c.w_row_bytes;
            c.b = (const float *)(b0 + v[8]); c.b_row_stride = c.K; c.b_tok_stride = c.n_b * c.K + v[14];
            c.ids = (const int32_t *)ids0; c.ids_tok_stride = c.n_used; c.dst = (float *)dst0; c.dst_row_stride = c.M; c.dst_tok_stride = c.n_used * c.M + v[13];
            const size_t size = ggml_cdna4_mul_mat_id_workspace_size(c.type, c.K, c.n_expert, c.n_used, c.n_b, c.n_tok);
            c.workspace = (void *)(ws0 + v[9]); c.workspace_bytes = v[10] ? (size_t)v[10] : size;
            const bool image = v[11] && !cdna4_resident_register(c.type, c.as, c.w_row_bytes, c.M * c.n_expert, c.K, (const void *)img0), prepared = v[12] != 0;
            cdna4_set_error_msg("untouched");
            const mmid_plan pl = mmid_make_plan(c, prepared);
            const std::string l1 = line_of(pl), l2 = line_of(mmid_make_plan(c, prepared));
            const bool pure = l1 == l2 && !strcmp(ggml_cdna4_last_error(), "untouched");
            const int rc = (prepared ? ggml_cdna4_mul_mat_id_prepared : ggml_cdna4_mul_mat_id)(c.type, c.as, c.w_row_bytes, c.w_expert_bytes, c.b, c.b_row_stride, c.b_tok_stride, c.ids, c.ids_tok_stride,
                c.dst, c.dst_row_stride, c.dst_tok_stride, c.M, c.K, c.n_expert, c.n_used, c.n_b, c.n_tok, c.workspace, c.workspace_bytes, nullptr);
            const std::string msg = rc ? ggml_cdna4_last_error() : "";
            const uint32_t key = ggml_cdna4_mul_mat_id_front_key(c.type, c.as, c.w_row_bytes, c.w_expert_bytes, c.M, c.K, c.n_expert, c.n_used, c.n_b, c.n_tok, c.workspace_bytes);
            printf("%s pure=%d size=%zu call_rc=%d plan_err=%d pubkey=%u | %s\n", l1.c_str(), (int)pure, size, rc, (int)(pl.err != nullptr && msg == pl.err), key, msg.c_str());
            if (image) cdna4_resident_unregister(c.as);
        }
        return 0;
    }
    fprintf(stderr, "usage: lib_emul mul_mat type M K B path w.bin x.bin y.bin | lib_emul mul_mat_id type M K n_expert n_used n_b n_tok w.bin x.bin ids.bin y.bin | lib_emul plan < calls | lib_emul plan_id < calls\n");
    return 2;
}
