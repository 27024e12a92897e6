"""Timing of ggml_cdna4_mul_mat_id on F16 / BF16 expert stacks (ggml_amd/csrc/moe_f16.hip): 8 experts x 2 used x [4096 x 4096], uniform routing, device events around
windows of calls, the two sides of every comparison alternating, median of three windows.

    python tools/microbench/moe_f16_bench.py [out.txt]

Three tables per weight type:
  * the per-column kernel (route 1) against the grouped one (route 2), both forced through CDNA4_F16_MOE_GEMV_MAX, for n_tok * n_used = 2 .. 32: the crossover's rows;
  * at 64 and 512 tokens, the grouped kernel on 32-row fragments against 128-row records (CDNA4_F16_MOE_TN);
  * at 512 tokens (128 rows per expert), the grouped call against eight ggml_cdna4_op_mul_mat_f calls of [4096 x 4096].[4096 x 128] on rows gathered beforehand
    (the gather is not timed): existing code doing the same flop with the host-side grouping for free.
Needs the GPU: no device, no numbers."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ggml_amd import native  # noqa: E402

M = K = 4096
NE, NU = 8, 2
ITERS = 200


def window(call, env):
    for k in ("CDNA4_F16_MOE_GEMV_MAX", "CDNA4_F16_MOE_TN"):
        os.environ.pop(k, None)
    os.environ.update(env)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def ab(side_a, side_b):
    """two (call, env) sides, windows alternating -> the medians of three, us per call"""
    t = [[], []]
    for _ in range(3):
        for i, (call, env) in enumerate((side_a, side_b)):
            t[i].append(window(call, env))
    return sorted(t[0])[1], sorted(t[1])[1]


def desc(t, type_, ne):
    d = native.Tensor()
    d.data = t.data_ptr(); d.type = type_; d.reserved = 0
    es = t.element_size()
    nb = [es, es * ne[0], es * ne[0] * ne[1], es * ne[0] * ne[1] * ne[2]]
    for i in range(4):
        d.ne[i] = ne[i]; d.nb[i] = nb[i]
    return d


def main():
    if not torch.cuda.is_available():
        sys.exit("moe_f16_bench: no GPU")
    L = native.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    for name, type_, dt in (("F16", 1, torch.float16), ("BF16", 30, torch.bfloat16)):
        w = (torch.randn((NE, M, K), device="cuda") * 0.05).to(dt)

        def grouped(nt):
            x, y = torch.randn((nt, 1, K), device="cuda"), torch.empty((nt, NU, M), device="cuda")
            tok, slot = torch.meshgrid(torch.arange(nt), torch.arange(NU), indexing="ij")
            ids = ((NU * tok + slot) % NE).to(torch.int32).cuda()                      # every expert gets n_tok * n_used / n_expert rows
            size = L.ggml_cdna4_mul_mat_id_workspace_size(type_, K, NE, NU, 1, nt)
            ws = torch.empty(size, dtype=torch.uint8, device="cuda")
            args = (type_, w.data_ptr(), 2 * K, 2 * K * M, x.data_ptr(), K, K, ids.data_ptr(), NU, y.data_ptr(), M, NU * M, M, K, NE, NU, 1, nt, ws.data_ptr(), size)

            def call():
                assert L.ggml_cdna4_mul_mat_id(*args, st) == 0, L.ggml_cdna4_last_error().decode()
            return call, (x, y, ids, ws)
        say("%s experts, %d x %d used x [%d x %d], us per call" % (name, NE, NU, M, K))
        say("%8s %8s %14s %14s" % ("n_tok", "columns", "route 1", "route 2"))
        for nt in (1, 2, 4, 8, 16):
            call, keep = grouped(nt)
            r1, r2 = ab((call, {"CDNA4_F16_MOE_GEMV_MAX": "1000000"}), (call, {"CDNA4_F16_MOE_GEMV_MAX": "0"}))
            say("%8d %8d %14.2f %14.2f" % (nt, nt * NU, r1, r2))
        say("%8s %8s %14s %14s" % ("n_tok", "columns", "TN 32", "TN 128"))
        for nt in (64, 512):
            call, keep = grouped(nt)
            t32, t128 = ab((call, {"CDNA4_F16_MOE_GEMV_MAX": "0", "CDNA4_F16_MOE_TN": "32"}), (call, {"CDNA4_F16_MOE_GEMV_MAX": "0", "CDNA4_F16_MOE_TN": "128"}))
            say("%8d %8d %14.2f %14.2f" % (nt, nt * NU, t32, t128))
        call, keep = grouped(512)
        rows = 512 * NU // NE
        xs, ys = torch.randn((NE, rows, K), device="cuda"), torch.empty((NE, rows, M), device="cuda")
        tri = [(desc(w[e], type_, (K, M, 1, 1)), desc(xs[e], 0, (K, rows, 1, 1)), desc(ys[e], 0, (M, rows, 1, 1))) for e in range(NE)]

        def dense():
            for a, b, d in tri:
                assert L.ggml_cdna4_op_mul_mat_f(C.byref(a), C.byref(b), C.byref(d), st) == 0, L.ggml_cdna4_last_error().decode()
        tg, td = ab((call, {}), (dense, {}))
        say("512 tokens: grouped call (default plan) %.2f | eight dense [%dx%d].[%dx%d] calls on gathered rows %.2f | grouped / dense %.3f" % (tg, M, K, K, rows, td, tg / td))
        say("")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
