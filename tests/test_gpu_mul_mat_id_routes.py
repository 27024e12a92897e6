"""-m gpu: the MUL_MAT_ID routing plan (ggml_amd/csrc/mul_mat_id_plan.hpp) at the calls where it changes its mind and no other GPU test stands: 4 experts x 2 used x
[130 x 256] (one ragged m-tile), 16 tokens (32 pairs: quantize + GEMV) against 17 (34: grouped); Q4_K's expert stack 16-byte aligned (the work queue) and shifted by 2 bytes
(k_gemm_q<Q4_K, IDS>, per-lane loads); Q6_K / Q8_0 at 17 tokens (the int8 matrix cores); one expert with 33 rows on k_gemm_q<.., IDS> with (Q5_K) and without (Q6_K) the
weights through LDS; a Q4_0 stack with a registered image at 17 tokens (the work queue on Q4_0R, in front of the int8 route); one token; and, in a fresh child process with
CDNA4_MOE_SK=0, the per-tile k_gemm_kq_t64<Q4_K, 128 | 256, IDS>.  Every cell against the oracle's MUL_MAT_ID under the bound the existing test of its kernel uses
(tests/test_gpu_parity.py: 1e-3 on the fp16 matrix-core GEMMs, 1e-5 on the integer-dot kernels); where the call leaves a front, the `prepared` call on a second stack is
bit-identical to its full call; with b shifted by 4 bytes the `prepared` call answers -2 and the one-token call -1, and neither writes dst."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refutil as R
from test_gpu_cabi_ops import L, _dev, _ok, _st      # noqa: F401  (the fixture + helpers)

pytestmark = pytest.mark.gpu
TOL_GEMV, TOL_GEMM = 1e-5, 1e-3                      # (tests/test_gpu_parity.py)
M, K, SENT = 130, 256, -77.0


@functools.lru_cache(maxsize=None)
def _problem(t, n_expert, n_used, n_tok, m=M, k=K):
    """two expert stacks, activations (n_b = 1), ids and the oracle's results — made once per cell, read-only"""
    rng = np.random.default_rng(int(t) * 1000 + n_expert * 100 + n_tok)
    w1, w2 = R.random_weights(t, n_expert * m, k, seed=5), R.random_weights(t, n_expert * m, k, seed=6)
    x = rng.uniform(-1, 1, (n_tok, 1, k)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    out = (w1, w2, x, ids, R.o_mul_mat_id(t, w1, x, ids, m, k, n_expert))
    for a in out:
        a.setflags(write=False)
    return out


def _shifted(a, nbytes):
    """a's bytes on the device, `nbytes` past a 256-byte boundary: (the tensor that owns them, the address)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 256, dtype=torch.uint8, device="cuda")
    buf[nbytes:nbytes + raw.size] = torch.from_numpy(np.array(raw)).cuda()
    return buf, buf.data_ptr() + nbytes


def _call(L, fn, t, w_ptr, x_ptr, idd, y, n_expert, n_used, n_tok, ws, m=M, k=K):
    rb = R.row_size(t, k)
    return fn(int(t), w_ptr, rb, m * rb, x_ptr, k, k, idd.data_ptr(), n_used, y.data_ptr(), m, n_used * m, m, k, n_expert, n_used, 1, n_tok, ws.data_ptr(), ws.numel(), _st())


def _key(L, t, w_ptr, n_expert, n_used, n_tok, nws, m=M, k=K):
    rb = R.row_size(t, k)
    return L.ggml_cdna4_mul_mat_id_front_key(int(t), w_ptr, rb, m * rb, m, k, n_expert, n_used, 1, n_tok, nws)


CELLS = [  # (id, type, n_expert, n_used, n_tok, shift of the stack, image, bound, leaves a front)
    ("q4_K-32-pairs-gemv", R.Q4_K, 4, 2, 16, 0, False, TOL_GEMV, False),
    ("q4_K-34-pairs-queue", R.Q4_K, 4, 2, 17, 0, False, TOL_GEMM, True),
    ("q4_K-34-pairs-shifted", R.Q4_K, 4, 2, 17, 2, False, TOL_GEMM, False),
    ("q6_K-34-pairs-int8", R.Q6_K, 4, 2, 17, 0, False, TOL_GEMV, False),
    ("q8_0-34-pairs-int8", R.Q8_0, 4, 2, 17, 0, False, TOL_GEMV, False),
    ("q5_K-one-expert-33", R.Q5_K, 1, 1, 33, 0, False, TOL_GEMM, False),
    ("q6_K-one-expert-33", R.Q6_K, 1, 1, 33, 0, False, TOL_GEMM, False),
    ("q4_0-image-34-pairs-queue", R.Q4_0, 4, 2, 17, 0, True, TOL_GEMM, True),
    ("q4_K-one-token", R.Q4_K, 4, 2, 1, 0, False, TOL_GEMV, False),
]


@pytest.mark.parametrize("cell,t,n_expert,n_used,n_tok,shift,image,tol,front", CELLS, ids=[c[0] for c in CELLS])
def test_route_agrees_with_the_oracle_and_its_front_serves_a_second_stack(L, cell, t, n_expert, n_used, n_tok, shift, image, tol, front):
    if shift and os.environ.get("CDNA4_TESTS_ON_EMULATOR") == "1":
        pytest.skip("k_gemm_q's 16-byte loads of a 2-byte-aligned block: the host build's aligned vector move traps (every byte is inside the stack: checked with a byte-wise load)")
    w1, w2, x, ids, yo = _problem(t, n_expert, n_used, n_tok)
    (b1, p1), (b2, p2), xd, idd = _shifted(w1, shift), _shifted(w2, shift), _dev(x), _dev(ids)
    nws = L.ggml_cdna4_mul_mat_id_workspace_size(int(t), K, n_expert, n_used, 1, n_tok)
    ws = torch.zeros(max(nws, 256), dtype=torch.uint8, device="cuda")
    imgs = []
    try:
        if image:
            for p in (p1, p2):
                imgs.append(torch.empty(L.ggml_cdna4_resident_image_size(int(t), n_expert * M, K), dtype=torch.uint8, device="cuda"))
                _ok(L, L.ggml_cdna4_resident_image_register(int(t), p, R.row_size(t, K), n_expert * M, K, imgs[-1].data_ptr(), 1, None))
        key = _key(L, t, p1, n_expert, n_used, n_tok, nws)
        assert (key != 0) == front and key == _key(L, t, p2, n_expert, n_used, n_tok, nws)
        y1, y2, y2_full = (torch.full((n_tok, n_used, M), SENT, dtype=torch.float32, device="cuda") for _ in range(3))
        _ok(L, _call(L, L.ggml_cdna4_mul_mat_id, t, p2, xd.data_ptr(), idd, y2_full, n_expert, n_used, n_tok, ws))
        ws.zero_()
        _ok(L, _call(L, L.ggml_cdna4_mul_mat_id, t, p1, xd.data_ptr(), idd, y1, n_expert, n_used, n_tok, ws))
        rc = _call(L, L.ggml_cdna4_mul_mat_id_prepared, t, p2, xd.data_ptr(), idd, y2, n_expert, n_used, n_tok, ws)
        torch.cuda.synchronize()
        e = R.rel_l2(y1.cpu().numpy(), yo)
        print("mul_mat_id_routes:", json.dumps(dict(cell=cell, rel_l2=e, key=key, prepared_rc=rc)))
        assert np.isfinite(y1.cpu().numpy()).all() and e < tol, e
        if front:
            assert rc == 0, L.ggml_cdna4_last_error().decode()
            assert torch.equal(y2.view(torch.int32), y2_full.view(torch.int32)) and not torch.equal(y1.view(torch.int32), y2.view(torch.int32))
        else:
            assert rc == -2 and bool((y2 == SENT).all())
    finally:
        if image:
            for p in (p1, p2)[:len(imgs)]:
                L.ggml_cdna4_resident_image_unregister(p)


def test_b_shifted_by_four_bytes_is_refused_and_dst_stays_untouched(L):
    """the `prepared` twin of a call that leaves a front: -2 (the caller issues the full call); one token: no one-launch form, and the quantizer of the GEMV form refuses the row (-1)"""
    t, n_expert, n_used = R.Q4_K, 4, 2
    for n_tok, fn, want, msg in ((17, L.ggml_cdna4_mul_mat_id_prepared, -2, "mul_mat_id_prepared: misaligned operands"), (1, L.ggml_cdna4_mul_mat_id, -1, "quantize_q8_K: x must be 16-byte aligned")):
        w1, _, x, ids, _ = _problem(t, n_expert, n_used, n_tok)
        (bw, pw), (bx, px), idd = _shifted(w1, 0), _shifted(x, 4), _dev(ids)
        nws = L.ggml_cdna4_mul_mat_id_workspace_size(int(t), K, n_expert, n_used, 1, n_tok)
        ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
        assert (_key(L, t, pw, n_expert, n_used, n_tok, nws) != 0) == (n_tok == 17)          # (the key is asked without b)
        y = torch.full((n_tok, n_used, M), SENT, dtype=torch.float32, device="cuda")
        assert _call(L, fn, t, pw, px, idd, y, n_expert, n_used, n_tok, ws) == want and L.ggml_cdna4_last_error().decode() == msg
        torch.cuda.synchronize()
        assert bool((y == SENT).all())


def _per_tile_cases(L):
    """(this process runs with CDNA4_MOE_SK=0) Q4_K on the per-tile k_gemm_kq_t64<.., IDS>: 34 pairs of [130 x 256] experts (128-row tiles with the planner's tile tables) and
    640 pairs of eight [4096 x 256] experts (thirteen activation tiles x sixteen 256-row m-tiles = 208 on 256 CUs: above 3/4 of a tile per CU, the 256-row form) -> rel-L2 vs the oracle, front key"""
    out = []
    for n_expert, n_used, n_tok, m in ((4, 2, 17, M), (8, 2, 320, 4096)):
        w1, _, x, ids, yo = _problem(R.Q4_K, n_expert, n_used, n_tok, m)
        wd, xd, idd = _dev(w1), _dev(x), _dev(ids)
        nws = L.ggml_cdna4_mul_mat_id_workspace_size(int(R.Q4_K), K, n_expert, n_used, 1, n_tok)
        ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
        y = torch.full((n_tok, n_used, m), SENT, dtype=torch.float32, device="cuda")
        _ok(L, _call(L, L.ggml_cdna4_mul_mat_id, R.Q4_K, wd.data_ptr(), xd.data_ptr(), idd, y, n_expert, n_used, n_tok, ws, m=m))
        torch.cuda.synchronize()
        yn = y.cpu().numpy()
        out.append(dict(m=m, n_tok=n_tok, key=_key(L, R.Q4_K, wd.data_ptr(), n_expert, n_used, n_tok, nws, m=m), finite=bool(np.isfinite(yn).all()), rel_l2=R.rel_l2(yn, yo)))
    return out


def test_per_tile_grouped_kernel_of_q4_K_without_the_work_queue(L):
    """CDNA4_MOE_SK=0 (read once per process) in ONE fresh child: no front key, and both tile forms of k_gemm_kq_t64<Q4_K, .., IDS> within the GEMM bar of the oracle"""
    if os.environ.get("CDNA4_TESTS_ON_EMULATOR") == "1":
        pytest.skip("the knob is read once per process: a child with the GPU's library")
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_mul_mat_id_routes as T\nfrom ggml_amd import native\nprint(json.dumps(T._per_tile_cases(native.lib())))\n") % (R.ROOT, os.path.join(R.ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, CDNA4_MOE_SK="0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    recs = json.loads(r.stdout.strip().splitlines()[-1])
    print("mul_mat_id_routes:", json.dumps(recs))
    assert len(recs) == 2
    for rec in recs:
        assert rec["key"] == 0 and rec["finite"] and rec["rel_l2"] < TOL_GEMM, rec
