"""-m gpu: ggml_cdna4_op_mul_mat_f on F16 weights (ggml_amd/csrc/gemm_f16.hip: k_gemm_f16 on the matrix cores, k_gemv_f16 for 1 .. 8 activation rows, k_mul_mat_f for
what they cannot read) against W.double() @ x.half().double().  Bound, elementwise: |y - ref| <= 2 K 2^-24 (|W| @ |x.half()|) — an fp16 x fp16 product is exact in fp32,
K fp32 additions in any order stay within (K - 1) 2^-24 of that sum of magnitudes, and the factor 2 covers the matrix core's undocumented internal rounding.  Every
case asserts its route through ggml_cdna4_op_mul_mat_f_route, so a silent fall-back fails.  The operands lie in NaN-filled buffers (row gaps, 64 bytes in front
and behind) and dst in a sentinel-filled one whose padding must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import refutil as R
from gpu_util import report, to_dev

pytestmark = pytest.mark.gpu
SENT = -12345.0


def _t4(ptr, type_, ne, nb):
    from ggml_amd import native
    d = native.Tensor()
    d.data = ptr; d.type = type_; d.reserved = 0
    for i in range(4):
        d.ne[i] = int(ne[i]); d.nb[i] = int(nb[i])
    return d


def _scatter(vals, nb, fill, dtype, off):
    """vals [n3][n2][n1][n0] placed at byte strides nb behind `off` bytes in a `fill`-ed buffer with 64 bytes to spare at the end"""
    es = np.dtype(dtype).itemsize
    idx = [np.arange(n).reshape([-1 if j == i else 1 for j in range(4)]) for i, n in enumerate(vals.shape)]      # axes (3, 2, 1, 0)
    pos = (off + idx[0] * nb[3] + idx[1] * nb[2] + idx[2] * nb[1] + idx[3] * nb[0]) // es
    buf = np.full(int(pos.max()) + 1 + 64 // es, fill, dtype)
    buf[pos] = vals
    return buf, pos


def _mul_mat(m, k, n, a23=(1, 1), b23=(1, 1), w_gap=0, x_gap=0, permuted=False, w_off=64):
    """-> (route, y [b3][b2][n][m], worst |y - ref| / bound); asserts finiteness, the bound and the untouched padding of dst"""
    from ggml_amd import native
    L = native.lib()
    rng = np.random.default_rng(m + 3 * k + 7 * n)
    w = rng.standard_normal((a23[1], a23[0], m, k)).astype(np.float16)
    x = (rng.standard_normal((b23[1], b23[0], n, k)) * 2).astype(np.float32)
    rb = 2 * k + w_gap
    wnb = [2, rb * a23[0], rb, rb * a23[0] * m] if permuted else [2, rb, rb * m, rb * m * a23[0]]       # permuted: memory order [a3][m][a2][k] (gpt-2's K view)
    xnb = [4, 4 * k + x_gap, (4 * k + x_gap) * n, (4 * k + x_gap) * n * b23[0]]
    ynb = [4, 4 * (m + 4), 4 * (m + 4) * n, 4 * (m + 4) * n * b23[0]]
    wbuf, _ = _scatter(w.view(np.uint16), wnb, 0x7E00, np.uint16, w_off)
    xbuf, _ = _scatter(x, xnb, np.nan, np.float32, 64)
    ybuf, ypos = _scatter(np.zeros((b23[1], b23[0], n, m), np.float32), ynb, SENT, np.float32, 64)
    ybuf[:] = SENT
    wd, xd, yd = to_dev(wbuf.view(np.int16)), to_dev(xbuf), to_dev(ybuf)
    a = _t4(wd.data_ptr() + w_off, R.F16, (k, m, a23[0], a23[1]), wnb)
    b = _t4(xd.data_ptr() + 64, R.F32, (k, n, b23[0], b23[1]), xnb)
    d = _t4(yd.data_ptr() + 64, R.F32, (m, n, b23[0], b23[1]), ynb)
    route = L.ggml_cdna4_op_mul_mat_f_route(C.byref(a), C.byref(b), C.byref(d))
    rc = L.ggml_cdna4_op_mul_mat_f(C.byref(a), C.byref(b), C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ggml_cdna4_last_error().decode()
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    y = out[ypos]
    mask = np.ones(out.shape, bool); mask[ypos] = False
    assert (out[mask] == SENT).all(), "dst padding overwritten"
    assert np.isfinite(y).all()
    w64, x64 = torch.from_numpy(w.astype(np.float64)), torch.from_numpy(x.astype(np.float16).astype(np.float64))
    i2 = np.arange(b23[0]) // (b23[0] // a23[0]); i3 = np.arange(b23[1]) // (b23[1] // a23[1])
    wt = w64[i3][:, i2].transpose(-1, -2)                                   # [b3][b2][k][m]
    ref, mag = (x64 @ wt).numpy(), (x64.abs() @ wt.abs()).numpy()
    ratio = float((np.abs(y - ref) / (2 * k * 2.0 ** -24 * mag + 1e-300)).max())
    report(test="mul_mat_f16", m=m, k=k, n=n, route=route, ratio=ratio)
    assert (np.abs(y - ref) <= 2 * k * 2.0 ** -24 * mag).all(), ratio
    return route, y, ratio


@pytest.mark.parametrize("m,k,n,kw", [
    (128, 32, 32, {}),                                                      # one tile, one step
    (130, 40, 33, dict(w_gap=16, x_gap=32)),                                # ragged M and N, K tail of 8, gaps between the rows of both operands
    (257, 1056, 129, {}),                                                   # 33 steps (the ring wraps), several tiles; on 256 CUs these few tiles are 32 wide
    (257, 1056, 129, dict(b23=(43, 1))),                                    # ... and 3 x 2 x 43 tiles of 128 fill them: the 128-wide kernel, weights broadcast
    (64, 64, 200, dict(a23=(2, 1), b23=(4, 2), permuted=True, x_gap=16)),   # r2 = 2, src0 a permuted view (nb1 > nb2), src1 rows strided
], ids=lambda v: "-".join(sorted(v)) if isinstance(v, dict) else str(v))
def test_f16_gemm_route(m, k, n, kw):
    assert _mul_mat(m, k, n, **kw)[0] == 3


@pytest.mark.parametrize("m,k", [(37, 24), (260, 2056)])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_f16_few_row_route(m, k, n):
    assert _mul_mat(m, k, n, w_gap=16 if n == 2 else 0, x_gap=16 if n == 3 else 0)[0] == 2


def test_f16_few_row_route_broadcasts_batches():
    assert _mul_mat(37, 520, 5, a23=(3, 1), b23=(6, 1))[0] == 2


@pytest.mark.parametrize("kw", [dict(k=36), dict(k=64, w_off=66)], ids=["k36", "src0+2"])
def test_f16_plain_route_is_the_old_kernel(kw, monkeypatch):
    """what the new kernels cannot read stays on k_mul_mat_f: correct, and the same bits as with the new kernels switched off"""
    kw = dict(kw); k = kw.pop("k")
    monkeypatch.delenv("CDNA4_F16_GEMM", raising=False)
    route, y, _ = _mul_mat(70, k, 20, **kw)
    monkeypatch.setenv("CDNA4_F16_GEMM", "0")
    route0, y0, _ = _mul_mat(70, k, 20, **kw)
    assert route == 1 and route0 == 1 and np.array_equal(y.view(np.uint32), y0.view(np.uint32))
