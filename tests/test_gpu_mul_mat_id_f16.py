"""-m gpu: ggml_cdna4_mul_mat_id on F16 (type 1) and BF16 (type 30) expert stacks (ggml_amd/csrc/moe_f16.hip: k_gemv_f16_ids per column, k_moe_plan + k_gemm_f16_ids
grouped) against W_e.double() @ x_r.double(), x_r the activation row rounded to the weights' format.  Bound, elementwise, from DESIGN 4.12 / 4.13:
|y - ref| <= 2 K 2^-24 (|W_e| @ |x_r|).  Every case asserts its route through ggml_cdna4_mul_mat_id_f16_route.  The operands lie in NaN-filled buffers with gaps between
rows, experts and tokens, dst in a sentinel-filled one: its padding, and every slot whose id is out of range, must come back untouched."""
import numpy as np
import pytest
import torch

from gpu_util import report, to_dev

pytestmark = pytest.mark.gpu
SENT = -12345.0
# route, M, K, n_expert, n_used, n_b, n_tok, two ids out of range
CASES = [
    (1, 37, 24, 4, 2, 1, 1, False),
    (1, 260, 2056, 8, 4, 4, 2, True),           # second LDS pass; n_b == n_used
    (2, 128, 32, 2, 1, 1, 33, False),           # one step; 16-byte stores
    (2, 130, 40, 4, 2, 2, 40, True),            # ragged M; K tail of 8
    (2, 257, 1056, 3, 2, 1, 100, False),        # the ring wraps (33 steps); 128-row records: expert 0 holds 160 rows (a full record + one fragment), expert 1 none, expert 2 40
]


def _view(buf, off, shape, strides):
    """the elements at `strides` (in elements) behind `off` elements of a flat buffer, as a writable view"""
    return np.lib.stride_tricks.as_strided(buf[off:], shape, [s * buf.itemsize for s in strides])


def _ids(m, ne, nu, nt, bad):
    tok, slot = np.mgrid[0:nt, 0:nu]
    ids = (tok + 3 * slot) % ne
    if m == 257:
        ids = np.where(slot == 0, 0, np.where(tok < 40, 2, 0))
    ids = ids.astype(np.int32)
    if bad:
        ids[0, 1], ids[nt - 1, nu - 1] = -1, ne
    return ids


def _mul_mat_id(type_, want, m, k, ne, nu, nb, nt, bad):
    """-> y [n_tok][n_used][M]; asserts the route, the return code, the untouched padding and out-of-range slots, finiteness and the bound"""
    from ggml_amd import native
    L = native.lib()
    dt = torch.bfloat16 if type_ == 30 else torch.float16
    g = torch.Generator().manual_seed(m + 3 * k + 7 * nt)
    w, x = torch.randn((ne, m, k), generator=g).to(dt), torch.randn((nt, nb, k), generator=g) * 2
    ids = _ids(m, ne, nu, nt, bad)
    wrow, brow, drow = 2 * k + 16, k + 4, m + 4                                                 # bytes, elements, elements
    wexp = m * wrow + 32
    wbuf = np.full(32 + ne * wexp // 2 + 32, 0x7FC0 if type_ == 30 else 0x7E00, np.uint16)
    _view(wbuf, 32, (ne, m, k), (wexp // 2, wrow // 2, 1))[:] = w.view(torch.int16).numpy().view(np.uint16)
    xbuf = np.full(16 + nt * nb * brow + 16, np.nan, np.float32)
    _view(xbuf, 16, (nt, nb, k), (nb * brow, brow, 1))[:] = x.numpy()
    ibuf = np.full(nt * (nu + 1), -7, np.int32)
    _view(ibuf, 0, (nt, nu), (nu + 1, 1))[:] = ids
    ybuf = np.full(16 + nt * nu * drow + 16, SENT, np.float32)
    wd, xd, idd, yd = to_dev(wbuf.view(np.int16)), to_dev(xbuf), to_dev(ibuf), to_dev(ybuf)
    size = L.ggml_cdna4_mul_mat_id_workspace_size(type_, k, ne, nu, nb, nt)
    assert size > 0 and size % 256 == 0
    ws = torch.empty(size, dtype=torch.uint8, device="cuda")
    args = (type_, wd.data_ptr() + 64, wrow, wexp, xd.data_ptr() + 64, brow, nb * brow, idd.data_ptr(), nu + 1, yd.data_ptr() + 64, drow, nu * drow,
            m, k, ne, nu, nb, nt) + ((None, 0) if want == 1 else (ws.data_ptr(), size))          # the per-column route takes no workspace
    assert L.ggml_cdna4_mul_mat_id_f16_route(*args) == want
    assert L.ggml_cdna4_mul_mat_id(*args, torch.cuda.current_stream().cuda_stream) == 0, L.ggml_cdna4_last_error().decode()
    torch.cuda.synchronize()
    out = yd.cpu().numpy()
    y = _view(out, 16, (nt, nu, m), (nu * drow, drow, 1)).copy()
    valid = (ids >= 0) & (ids < ne)
    rest = out.copy()
    _view(rest, 16, (nt, nu, m), (nu * drow, drow, 1))[valid] = SENT
    assert (rest == SENT).all(), "dst padding or an out-of-range slot overwritten"
    assert np.isfinite(y[valid]).all()
    w64, xr = w.double(), x.to(dt).double().reshape(nt * nb, k)                                 # every expert times every rounded row: [row][expert][M]
    prod, mag = torch.einsum("emk,rk->rem", w64, xr).numpy(), torch.einsum("emk,rk->rem", w64.abs(), xr.abs()).numpy()
    tok, slot = np.mgrid[0:nt, 0:nu]
    pick = (tok * nb + slot % nb, np.where(valid, ids, 0))                                      # slot u reads activation row u % n_b
    err, bound = np.abs(y - prod[pick]), 2 * k * 2.0 ** -24 * mag[pick]
    report(test="mul_mat_id_f16", type=type_, m=m, k=k, n_tok=nt, route=want, ratio=float((err[valid] / (bound[valid] + 1e-300)).max()))
    assert (err[valid] <= bound[valid]).all()
    return y


@pytest.mark.parametrize("type_", [1, 30], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "r%d-%dx%d-%dtok" % (c[0], c[1], c[2], c[6]))
def test_mul_mat_id_f16(type_, case, monkeypatch):
    monkeypatch.delenv("CDNA4_F16_MOE_GEMV_MAX", raising=False)
    monkeypatch.delenv("CDNA4_F16_MOE_TN", raising=False)
    y = _mul_mat_id(type_, *case)
    if case[1] == 257:                                                                          # no output depends on the place the planner's atomics gave its row
        assert np.array_equal(y.view(np.uint32), _mul_mat_id(type_, *case).view(np.uint32))


@pytest.mark.parametrize("type_", [1, 30], ids=["f16", "bf16"])
def test_mul_mat_id_f16_on_32_row_fragments(type_, monkeypatch):
    """k_gemm_f16_ids<32, ..>, which the plan takes under CDNA4_F16_MOE_TN=32 only: a fragment per work-group, empty fragments end before their first load"""
    monkeypatch.setenv("CDNA4_F16_MOE_TN", "32")
    for case in CASES[3:]:
        _mul_mat_id(type_, *case)
