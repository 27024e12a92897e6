// gemm_q_plan.hpp — the routing plan of the prefill GEMM (cdna4_launch_gemm_q): which kernel a call takes, where that kernel's weights come from and the
// launch parameters of the terminal.  gemm_q_make_plan() is side-effect free — no scratch, no launch, no error text; it reads the arguments, the CU counts, the
// shared-device mode, the env knobs and the (read-only) resident registry — so the call and every query read the SAME plan: the call executes it, the queries
// read a field.  Kernel-library sources only (like cdna4_formats.hpp: not one of the files the ggml plug-in's checksum covers).
#pragma once
#include "cdna4_kernels.h"

// k_gemm_kq_t64 (gemm_q_t64.hip): tile rows, split and whether the activation quantizer rides inside (`fq`)
struct t64_plan { int tm, splitk, ntiles; bool ticketed2, fq; };
// k_gemm_r8 (gemm_q_lds.hip): 256-row tiles; a split > 1 is the reduce-scatter between co-resident work-groups
struct r8_plan { int tm, splitk, ntiles; };
// the 128 x 128-tile kernels (gemm_q_mfma.hip): `type` the format the kernel is instantiated for (100.. re-laid, 200.. staged), `opt` 65 k_gemm_kq_w12 / 64 k_gemm_kq_w8p /
// 20 k_gemm_kq_w8 after the shallow-K demotion, `exp` the experiment bits of k_gemm_kq_w12.  exchange: the split in two meets in scratch (ticketed: the last to arrive sums,
// otherwise the waiting hand-off); a split without it zero-fills the output and sums with atomics (the tail is then not in the store)
struct w8_plan { int type, splitk, opt, exp; bool ticketed, exchange; int sb_split, xchg_l2; };
// the older per-lane-load kernel k_gemm_q: weights through LDS or not; a split zero-fills and sums with atomics
struct kq_plan { bool wlds; int splitk; };

// the sub-planners of the launchers that live in other files: nullptr, or the message the launcher refuses the call with
const char *t64_make_plan(const cdna4_gemm_args &a, int tm, int splitk, t64_plan &pl);          // tm 0 = choose / 128 / 256; splitk 0 = choose / 1 / 2 / 4 / 8
const char *r8_make_plan(const cdna4_gemm_args &a, int splitk, r8_plan &pl);                    // splitk 0 = choose
int cdna4_run_gemm_t64(const cdna4_gemm_args &a, const t64_plan &pl, hipStream_t st);
int cdna4_run_gemm_r8(const cdna4_gemm_args &a, const r8_plan &pl, hipStream_t st);

enum gq_source {
    GQ_W_GIVEN,         // the caller's rows
    GQ_W_RESIDENT,      // a resident image (`image`): the kernel-native re-layout of Q4_0 / Q8_0 / Q6_K, or the exact re-encoding of a format without a kernel of its own
    GQ_W_REENCODED,     // re-encoded per call into scratch kind 3 (convert_w.hip)
    GQ_W_RELAID,        // re-laid per call into scratch kind 1 (16-byte-aligned superblocks), from the caller's rows or from the re-encoded ones (`reencoded`)
};
enum gq_terminal { GQ_NONE, GQ_T64, GQ_R8, GQ_W8, GQ_KQ };
struct gemm_q_plan {
    const char *err;            // nullptr, or the message the call returns -1 with (nothing else of the plan is then meaningful)
    int kernel;                 // 10 k_gemm_kq_t64, 12 k_gemm_r8, 13 the 128 x 128-tile kernels, 14 k_gemm_q; 0: nothing to launch (an empty product)
    bool reencoded;             // the weights meet the kernel as their exact re-encoding (Q8_0 / Q6_K: `mid_type`)
    bool tail_in_store;         // the kernel applies a.epi in its store
    bool fuses_quantizer;       // the kernel quantizes a.xf itself (k_gemm_kq_t64<.., FQ>)
    gq_source source;
    const uint8_t *image;       // the resident rows: of the re-encoding (`reencoded`) or of the re-layout (GQ_W_RESIDENT); nullptr: none
    int mid_type;               // the format the terminal's rules were chosen for: a.type, or its re-encoding target
    int64_t mid_row_bytes;      // ... and its row bytes (what the re-layout pass of GQ_W_RELAID reads)
    int kmul;                  // k.K = a.K * kmul (2: a two-part re-encoding, the activation image is doubled)
    cdna4_gemm_args k;          // what the terminal is launched with: the caller's arguments with the kernel's weight type, row bytes and K; k.W == nullptr: the scratch rows
    gq_terminal terminal;
    t64_plan t64; r8_plan r8; w8_plan w8; kq_plan kq;      // the one `terminal` names
};
gemm_q_plan gemm_q_make_plan(const cdna4_gemm_args &a);                                          // gemm_q_mfma.hip
// what ggml_cdna4_mul_mat_route documents: 11 = k_gemm_kq_t64 with the activation quantizer inside (ONE launch), + 100 behind an exact re-encoding, 0: none
inline int gemm_q_route_id(const gemm_q_plan &pl) { return pl.kernel == 10 && pl.fuses_quantizer ? 11 : (pl.kernel ? pl.kernel + 100 * (int)pl.reencoded : 0); }
