"""ggml_cdna4_op_mul_mat_f_route: the kernel a MUL_MAT on F32 / F16 weights takes, read from the plan the call itself executes (ggml_amd/csrc/gemm_f16_plan.hpp) without a
device (CDNA4_ASSUME_CUS names the part): 0 refused, 1 k_mul_mat_f, 2 k_gemv_f16, 3 k_gemm_f16; CDNA4_F16_GEMM=0 keeps every accepted call on 1."""
import json
import os
import subprocess
import sys

import pytest

import refutil as R

# name -> (src0 type, M, K, N, src0 pointer offset, src0 nb1 - 2 K, src1 K - K, src0 ne2, src1 ne2), expected route
CASES = {
    "n1": ((1, 4096, 4096, 1, 0, 0, 0, 1, 1), 2), "n8": ((1, 4096, 4096, 8, 0, 0, 0, 1, 1), 2), "n512": ((1, 4096, 4096, 512, 0, 0, 0, 1, 1), 3),
    "k36": ((1, 4096, 36, 64, 0, 0, 0, 1, 1), 1), "src0+2": ((1, 4096, 4096, 64, 2, 0, 0, 1, 1), 1), "nb1+2": ((1, 4096, 4096, 64, 0, 2, 0, 1, 1), 1),
    "f32": ((0, 4096, 4096, 64, 0, 0, 0, 1, 1), 1), "ne0": ((1, 4096, 4096, 64, 0, 0, 8, 1, 1), 0), "batch": ((1, 4096, 4096, 64, 0, 0, 0, 2, 3), 0),
    "broadcast": ((1, 64, 64, 200, 0, 0, 0, 2, 4), 3),
}
CODE = r"""
import ctypes as C, json, sys
class T(C.Structure):
    _fields_ = [("data", C.c_void_p), ("type", C.c_int32), ("reserved", C.c_int32), ("ne", C.c_int64 * 4), ("nb", C.c_int64 * 4)]
L = C.CDLL(sys.argv[1])
f = L.ggml_cdna4_op_mul_mat_f_route; f.restype = C.c_int; f.argtypes = [C.c_void_p] * 3
def t4(ptr, type_, es, ne, nb1):
    t = T(); t.data = ptr; t.type = type_
    t.ne[:] = ne; t.nb[:] = [es, nb1, nb1 * ne[1], nb1 * ne[1] * ne[2]]
    return t
out = {}
for name, (t, m, k, n, off, gap, dk, a2, b2) in json.loads(sys.argv[2]).items():
    es = 2 if t == 1 else 4
    a, b, d = t4(0x10000 + off, t, es, (k, m, a2, 1), es * k + gap), t4(0x20000, 0, 4, (k + dk, n, b2, 1), 4 * (k + dk)), t4(0x30000, 0, 4, (m, n, b2, 1), 4 * m)
    out[name] = f(C.byref(a), C.byref(b), C.byref(d))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def routes():
    import __graft_entry__ as g
    g.build()

    def run(**env):
        r = subprocess.run([sys.executable, "-c", CODE, os.path.join(R.ROOT, "ggml_amd", "lib", "libcdna4_kernels.so"), json.dumps({k: v[0] for k, v in CASES.items()})],
                           capture_output=True, text=True, timeout=120,
                           env=dict({k: v for k, v in os.environ.items() if k != "CDNA4_F16_GEMM"}, CDNA4_ASSUME_CUS="256", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", **env))
        assert r.returncode == 0, r.stderr[-800:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    return run(), run(CDNA4_F16_GEMM="0")


@pytest.mark.parametrize("name", list(CASES))
def test_f16_route(routes, name):
    want = CASES[name][1]
    assert routes[0][name] == want
    assert routes[1][name] == min(want, 1)                 # the knob: k_mul_mat_f wherever a new kernel would run; a refused call stays refused
