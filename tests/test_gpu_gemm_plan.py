"""-m gpu: every terminal the prefill GEMM's routing plan (ggml_amd/csrc/gemm_q_plan.hpp) can name, at the smallest shape that reaches it on a 256-CU part — the call executes
the plan the route query reads.  Through the C-ABI: the route id where the call is AUTO (up to 64 activation rows AUTO is the int8 matrix-core
kernel, so the 64-row shapes ask for the GEMM path and have a 65-row AUTO twin), the product against the CPU oracle (the bar of tests/test_gpu_parity.py for the fp16 MFMA
GEMM path: rel-L2 < 1e-3; rows sampled where the matrix is large), and ggml_cdna4_mul_mat_fused == ggml_cdna4_mul_mat + bias bit for bit on the routes whose tail is in the store."""
import numpy as np
import pytest
import torch

import refutil as R

pytestmark = pytest.mark.gpu
TOL_GEMM = 1e-3                                                          # tests/test_gpu_parity.py
PATH_AUTO, PATH_GEMM = 0, 2

# (name, type, M, K, B, path, splitk, owned device, route id the AUTO query names (None: the call is not AUTO), tail in the store)
CASES = [
    ("q4_K t64 ticketed split in two", R.Q4_K, 256, 512, 64, PATH_GEMM, 0, False, None, True),          # (64 rows: AUTO is the int8 matrix cores; the GEMM path is asked for)
    ("q4_K t64 deep split 8", R.Q4_K, 128, 4096, 16, PATH_GEMM, 0, False, None, True),
    ("q4_K r8 whole rounds", R.Q4_K, 4096, 512, 4096, PATH_AUTO, 0, False, 12, True),
    ("q4_K t64 one launch, owned device", R.Q4_K, 4096, 4096, 512, PATH_AUTO, 0, True, 11, True),
    ("q5_K 128x128 ticketed", R.Q5_K, 256, 1024, 64, PATH_GEMM, 0, False, None, True),
    ("q5_K 128x128 split 4: zero fill + atomics", R.Q5_K, 256, 1024, 64, PATH_GEMM, 4, False, None, False),
    ("q8_0 staged w12", R.Q8_0, 256, 768, 64, PATH_GEMM, 0, False, None, True),
    ("q8_0 re-layout + w8", R.Q8_0, 256, 256, 64, PATH_GEMM, 0, False, None, True),
    ("q8_0 older kernel", R.Q8_0, 256, 320, 64, PATH_GEMM, 0, False, None, False),
    ("q5_0 re-encoded, staged w12", R.Q5_0, 256, 768, 64, PATH_GEMM, 0, False, None, True),
    ("q8_0 staged w12, AUTO", R.Q8_0, 256, 768, 65, PATH_AUTO, 0, False, 13, True),
    ("q8_0 older kernel, AUTO", R.Q8_0, 256, 320, 65, PATH_AUTO, 0, False, 14, False),
    ("q5_0 re-encoded, AUTO", R.Q5_0, 256, 768, 65, PATH_AUTO, 0, False, 113, True),
    ("q4_K t64, AUTO", R.Q4_K, 256, 512, 65, PATH_AUTO, 0, False, 10, True),
    ("q5_K 128x128 ticketed, AUTO", R.Q5_K, 256, 1024, 65, PATH_AUTO, 0, False, 13, True),
    ("q8_0 re-layout + w8, AUTO", R.Q8_0, 256, 256, 65, PATH_AUTO, 0, False, 13, True),
]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from ggml_amd import native
    return native.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name,t,m,k,b,path,splitk,owned,route,tail", CASES, ids=[c[0] for c in CASES])
def test_the_call_executes_the_plan_the_queries_read(L, name, t, m, k, b, path, splitk, owned, route, tail):
    st = torch.cuda.current_stream().cuda_stream
    w = R.random_weights(t, m, k, seed=m + k + b)
    rng = np.random.default_rng(b)
    x = rng.uniform(-1, 1, (b, k)).astype(np.float32)
    bias = rng.standard_normal(m).astype(np.float32)
    wd, xd, bd = _dev(w), _dev(x), _dev(bias)
    rb = R.row_size(t, k)
    nws = L.ggml_cdna4_mul_mat_workspace_size(int(t), k, b)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device="cuda")
    y = torch.full((b, m), 7.0, dtype=torch.float32, device="cuda"); yf = torch.full((b, m), 9.0, dtype=torch.float32, device="cuda")
    old = L.ggml_cdna4_set_shared_device(0 if owned else 1)
    try:
        if route is not None:
            assert L.ggml_cdna4_mul_mat_route(int(t), m, k, b) == route
            assert L.ggml_cdna4_mul_mat_fused_residual_may_alias(int(t), m, k, b) == int(tail)
        rc = L.ggml_cdna4_mul_mat(int(t), wd.data_ptr(), rb, xd.data_ptr(), k, y.data_ptr(), m, m, k, b, ws.data_ptr(), ws.numel(), path, 0, splitk, st)
        assert rc == 0, L.ggml_cdna4_last_error()
        if route is not None and tail:                                  # the fused entry point is AUTO: the same route, with the bias added in the kernel's store
            rc = L.ggml_cdna4_mul_mat_fused(int(t), wd.data_ptr(), rb, xd.data_ptr(), k, yf.data_ptr(), m, m, k, b, bd.data_ptr(), 0, None, 0, ws.data_ptr(), ws.numel(), st)
            assert rc == 0, L.ggml_cdna4_last_error()
        torch.cuda.synchronize()
    finally:
        L.ggml_cdna4_set_shared_device(old)
    yh = y.cpu().numpy()
    assert np.isfinite(yh).all()
    rows = np.arange(m) if m <= 256 else np.random.default_rng(0).choice(m, 64, replace=False)
    wsub = np.concatenate([w[r * rb:(r + 1) * rb] for r in rows])
    e = R.rel_l2(yh[:, rows], R.o_mul_mat(t, wsub, x, len(rows), k))
    print("%s: rel-L2 vs the oracle %.3e" % (name, e))
    assert e < TOL_GEMM, (name, e)
    if route is not None and tail:
        assert np.array_equal(yf.cpu().numpy().view(np.uint32), (y + bd).cpu().numpy().view(np.uint32)), name
