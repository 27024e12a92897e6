"""A/B timing of ggml_cdna4_op_mul_mat_f on F16 / BF16 weights: CDNA4_F16_GEMM=0 (k_mul_mat_f, one wave per output element) against the default plan
(k_gemv_f16 / k_gemm_f16, ggml_amd/csrc/gemm_f16.hip), alternating the two per shape, device events around a batch of calls.

    python tools/microbench/f16_gemm_bench.py [--type f16|bf16|both] [out.txt]

--type both times the default plan of the two weight types against each other instead (windows alternating F16 / BF16, median of three): the table of DESIGN 4.13.

Columns: the route the plan takes, microseconds per call for both, the speed-up, and the new kernel's share of its roof — route 3: 2 M N K flop over the dense
fp16 MFMA peak (2516.6 TFLOP/s); route 2: the weight bytes (2 M K per weight batch) over the HBM peak (8 TB/s).  Needs the GPU: no device, no numbers."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ggml_amd import native  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 2516.6e12, 8.0e12
# (M, K, N, src0 batches, src1 batches)
SHAPES = [(4096, 4096, n, 1, 1) for n in (1, 2, 4, 8, 16, 32, 64, 512)] + [(32768, 8192, 512, 1, 1), (200, 64, 200, 12, 12), (1024, 64, 200, 12, 12), (64, 200, 200, 12, 12)]


def desc(t, type_, ne):
    d = native.Tensor()
    d.data = t.data_ptr(); d.type = type_; d.reserved = 0
    es = t.element_size()
    nb = [es, es * ne[0], es * ne[0] * ne[1], es * ne[0] * ne[1] * ne[2]]
    for i in range(4):
        d.ne[i] = ne[i]; d.nb[i] = nb[i]
    return d


def timed(L, a, b, d, knob, iters):
    if knob is None:
        os.environ.pop("CDNA4_F16_GEMM", None)
    else:
        os.environ["CDNA4_F16_GEMM"] = knob
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        assert L.ggml_cdna4_op_mul_mat_f(C.byref(a), C.byref(b), C.byref(d), st) == 0, L.ggml_cdna4_last_error().decode()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        L.ggml_cdna4_op_mul_mat_f(C.byref(a), C.byref(b), C.byref(d), st)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def both(L):
    """default plan, F16 against BF16 weights of the same shape: the two move the same bytes and issue the same MFMA count"""
    lines = ["%-28s %5s %12s %12s %10s" % ("[M x K] . [K x N] x batch", "route", "f16 us", "bf16 us", "bf16 / f16")]
    for m, k, n, ba, bb in SHAPES:
        w32 = torch.randn((ba, m, k), device="cuda") * 0.05
        x, y = torch.randn((bb, n, k), device="cuda"), torch.empty((bb, n, m), device="cuda")
        ws = [w32.half(), w32.bfloat16()]
        b, d = desc(x, 0, (k, n, bb, 1)), desc(y, 0, (m, n, bb, 1))
        a = [desc(ws[0], 1, (k, m, ba, 1)), desc(ws[1], 30, (k, m, ba, 1))]
        os.environ.pop("CDNA4_F16_GEMM", None)
        route = [L.ggml_cdna4_op_mul_mat_f_route(C.byref(t), C.byref(b), C.byref(d)) for t in a]
        assert route[0] == route[1], route
        t = [[], []]
        for _ in range(3):
            for i in (0, 1):
                t[i].append(timed(L, a[i], b, d, None, 200))
        f, g = sorted(t[0])[1], sorted(t[1])[1]
        lines.append("%-28s %5d %12.2f %12.2f %10.3f" % ("[%dx%d].[%dx%d]x%d" % (m, k, k, n, bb), route[0], f, g, g / f))
        print(lines[-1], flush=True)
    return lines


def main():
    if not torch.cuda.is_available():
        sys.exit("f16_gemm_bench: no GPU")
    L = native.lib()
    args = sys.argv[1:]
    wtype = args.pop(args.index("--type") + 1) if "--type" in args else "f16"
    args = [v for v in args if v != "--type"]
    lines = both(L) if wtype == "both" else ab(L, wtype)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


def ab(L, wtype):
    lines = ["%-28s %5s %12s %12s %8s %s" % ("[M x K] . [K x N] x batch", "route", "knob=0 us", "default us", "speed-up", "share of roof")]
    for m, k, n, ba, bb in SHAPES:
        w = torch.randn((ba, m, k), device="cuda") * 0.05
        w = w.bfloat16() if wtype == "bf16" else w.half()
        x = torch.randn((bb, n, k), device="cuda")
        y = torch.empty((bb, n, m), device="cuda")
        a, b, d = desc(w, 30 if wtype == "bf16" else 1, (k, m, ba, 1)), desc(x, 0, (k, n, bb, 1)), desc(y, 0, (m, n, bb, 1))
        os.environ.pop("CDNA4_F16_GEMM", None)
        route = L.ggml_cdna4_op_mul_mat_f_route(C.byref(a), C.byref(b), C.byref(d))
        flop = 2.0 * m * n * k * bb
        iters_new = 200
        iters_old = max(5, min(200, int(2e11 / flop)))             # the old kernel runs at a few TFLOP/s: keep its window near a tenth of a second
        t_old, t_new = [], []
        for _ in range(3):                                          # alternate the two; report the median
            t_old.append(timed(L, a, b, d, "0", iters_old)); t_new.append(timed(L, a, b, d, None, iters_new))
        o, nw = sorted(t_old)[1], sorted(t_new)[1]
        y_new = y.clone()
        timed(L, a, b, d, "0", 1)
        diff = ((y - y_new).abs().max() / y.abs().max()).item()
        share = ("%.3f of the 16-bit MFMA peak" % (flop / (nw * 1e-6) / PEAK_FLOPS)) if route == 3 else ("%.3f of HBM" % (2.0 * m * k * ba / (nw * 1e-6) / PEAK_BYTES)) if route == 2 else "-"
        lines.append("%-28s %5d %12.2f %12.2f %8.2f %s   (max |new - old| / max |old| = %.1e)" % ("[%dx%d].[%dx%d]x%d" % (m, k, k, n, bb), route, o, nw, o / nw, share, diff))
        print(lines[-1], flush=True)
    os.environ.pop("CDNA4_F16_GEMM", None)
    return lines


if __name__ == "__main__":
    main()
