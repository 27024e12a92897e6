"""-m gpu: ggml_cdna4_op_mul_mat_f on BF16 weights (gemm_f16.hip: k_gemm_f16<.., bf16>, k_gemv_bf16; ops.hip: k_mul_mat_f<bf16>) against W.double() @ x.bfloat16().double().
Bound, elementwise, as for F16: |y - ref| <= 2 K 2^-24 (|W| @ |x_bf16|); a bf16 x bf16 product is exact in fp32.  Operands, dst and routes as in test_gpu_mul_mat_f16."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import report, to_dev
from test_gpu_mul_mat_f16 import SENT, _scatter, _t4

pytestmark = pytest.mark.gpu


def _mul_mat(m, k, n, a23=(1, 1), b23=(1, 1), w_gap=0, x_gap=0, permuted=False, w_off=64):
    from ggml_amd import native                             # -> (route, y [b3][b2][n][m]); asserts finiteness, the bound and the untouched padding of dst
    L = native.lib()
    g = torch.Generator().manual_seed(m + 3 * k + 7 * n)
    w, x = torch.randn((a23[1], a23[0], m, k), generator=g).bfloat16(), torch.randn((b23[1], b23[0], n, k), generator=g) * 2
    rb, xb = 2 * k + w_gap, 4 * k + x_gap
    wnb = [2, rb * a23[0], rb, rb * a23[0] * m] if permuted else [2, rb, rb * m, rb * m * a23[0]]       # permuted: memory order [a3][m][a2][k]
    xnb, ynb = [4, xb, xb * n, xb * n * b23[0]], [4, 4 * (m + 4), 4 * (m + 4) * n, 4 * (m + 4) * n * b23[0]]
    wbuf, xbuf = _scatter(w.view(torch.int16).numpy().view(np.uint16), wnb, 0x7FC0, np.uint16, w_off)[0], _scatter(x.numpy(), xnb, np.nan, np.float32, 64)[0]
    ybuf, ypos = _scatter(np.full((b23[1], b23[0], n, m), SENT, np.float32), ynb, SENT, np.float32, 64)
    wd, xd, yd = to_dev(wbuf.view(np.int16)), to_dev(xbuf), to_dev(ybuf)
    a, b, d = _t4(wd.data_ptr() + w_off, 30, (k, m, a23[0], a23[1]), wnb), _t4(xd.data_ptr() + 64, 0, (k, n, b23[0], b23[1]), xnb), _t4(yd.data_ptr() + 64, 0, (m, n, b23[0], b23[1]), ynb)
    route = L.ggml_cdna4_op_mul_mat_f_route(C.byref(a), C.byref(b), C.byref(d))
    assert L.ggml_cdna4_op_mul_mat_f(C.byref(a), C.byref(b), C.byref(d), torch.cuda.current_stream().cuda_stream) == 0, L.ggml_cdna4_last_error().decode()
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    y, mask = out[ypos], np.ones(out.shape, bool); mask[ypos] = False
    assert (out[mask] == SENT).all() and np.isfinite(y).all(), "dst padding overwritten, or a non-finite result"
    i2, i3 = np.arange(b23[0]) // (b23[0] // a23[0]), np.arange(b23[1]) // (b23[1] // a23[1])
    wt, x64 = w.double()[i3][:, i2].transpose(-1, -2), x.bfloat16().double()                          # wt [b3][b2][k][m]
    err, bound = np.abs(y - (x64 @ wt).numpy()), 2 * k * 2.0 ** -24 * (x64.abs() @ wt.abs()).numpy()
    report(test="mul_mat_bf16", m=m, k=k, n=n, route=route, ratio=float((err / (bound + 1e-300)).max()))
    assert (err <= bound).all()
    return route, y


@pytest.mark.parametrize("m,k,n,kw,want", [
    (128, 32, 32, {}, 3),                                                       # one tile, one step
    (130, 40, 33, dict(w_gap=16, x_gap=32), 3),                                 # ragged M and N, K tail of 8, gaps between the rows of both operands
    (257, 1056, 129, {}, 3),                                                    # 33 steps (the ring wraps); on 256 CUs these few tiles are 32 wide
    (257, 1056, 129, dict(b23=(43, 1)), 3),                                     # ... and 3 x 2 x 43 tiles of 128 fill them: the 128-wide kernel, weights broadcast
    (64, 64, 200, dict(a23=(2, 1), b23=(4, 2), permuted=True, x_gap=16), 3),    # r2 = 2, src0 a permuted view (nb1 > nb2), src1 rows strided
    (37, 520, 5, dict(a23=(3, 1), b23=(6, 1)), 2),                              # few rows, batches broadcast
    (70, 36, 20, {}, 1), (70, 64, 20, dict(w_off=66), 1),                       # what the bf16 kernels cannot read: K % 8, src0 at + 2 bytes
] + [(m, k, n, dict(w_gap=16 if n == 2 else 0, x_gap=16 if n == 3 else 0), 2) for m, k in [(37, 24), (260, 2056)] for n in (1, 2, 3, 8)],
    ids=lambda v: "-".join(sorted(v)) if isinstance(v, dict) else str(v))
def test_bf16_mul_mat(m, k, n, kw, want, monkeypatch):
    monkeypatch.delenv("CDNA4_F16_GEMM", raising=False)
    route, y = _mul_mat(m, k, n, **kw)
    assert route == want
    if want == 1:                                                               # ... k_mul_mat_f<bf16>: the same bits as with the bf16 kernels switched off
        monkeypatch.setenv("CDNA4_F16_GEMM", "0")
        route0, y0 = _mul_mat(m, k, n, **kw)
        assert route0 == 1 and np.array_equal(y.view(np.uint32), y0.view(np.uint32))
