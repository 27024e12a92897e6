"""ggml_cdna4_mul_mat_id_f16_route: the kernel a MUL_MAT_ID on F16 / BF16 experts takes, read from the plan the call itself executes (ggml_amd/csrc/moe_f16_plan.hpp)
without a device: 0 refused, 1 the per-column kernel, 2 the grouped kernel; and the workspace the grouped route asks for."""
import json
import os
import subprocess
import sys

import pytest

import refutil as R

XOVER = 16      # the per-column / grouped crossover in (token, slot) columns (moe_f16_plan.hpp: MOE_F16_GEMV_MAX)
# name -> (type, K, n_expert, n_used, n_tok, `as` offset, workspace bytes: -1 the published size, else that many), expected route
CASES = {
    "f16-below": ((1, 4096, 8, 2, XOVER // 2, 0, -1), 1), "f16-above": ((1, 4096, 8, 2, XOVER // 2 + 1, 0, -1), 2),
    "bf16-below": ((30, 4096, 8, 2, XOVER // 2, 0, 0), 1), "bf16-above": ((30, 4096, 8, 2, XOVER // 2 + 1, 0, -1), 2),
    "k36": ((1, 36, 8, 2, 4, 0, -1), 0), "as+2": ((1, 4096, 8, 2, 4, 2, -1), 0), "ws-small": ((30, 4096, 8, 2, 64, 0, 1024), 0),
    "1025-above": ((1, 4096, 1025, 2, 64, 0, -1), 0), "1025-below": ((1, 4096, 1025, 2, 4, 0, -1), 1), "f32": ((0, 4096, 8, 2, 4, 0, -1), 0),
}
CODE = r"""
import ctypes as C, json, sys
L = C.CDLL(sys.argv[1])
i64, vp = C.c_int64, C.c_void_p
f = L.ggml_cdna4_mul_mat_id_f16_route; f.restype = C.c_int; f.argtypes = [C.c_int, vp, i64, i64, vp, i64, i64, vp, i64, vp, i64, i64] + [i64] * 6 + [vp, C.c_size_t]
s = L.ggml_cdna4_mul_mat_id_workspace_size; s.restype = C.c_size_t; s.argtypes = [C.c_int] + [i64] * 5
out, m = {}, 4096
for name, (t, k, ne, nu, nt, off, ws) in json.loads(sys.argv[2]).items():
    size = s(t, k, ne, nu, 1, nt)
    out[name] = [f(t, 0x100000 + off, 2 * k, 2 * k * m, 0x200000, k, k, 0x300000, nu, 0x400000, m, nu * m, m, k, ne, nu, 1, nt, 0x500000, size if ws < 0 else ws), size]
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def answers():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CODE, os.path.join(R.ROOT, "ggml_amd", "lib", "libcdna4_kernels.so"), json.dumps({k: v[0] for k, v in CASES.items()})],
                       capture_output=True, text=True, timeout=120,
                       env=dict({k: v for k, v in os.environ.items() if not k.startswith("CDNA4_F16_MOE")}, CDNA4_ASSUME_CUS="256", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stderr[-800:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(CASES))
def test_moe_f16_route(answers, name):
    route, size = answers[name]
    assert route == CASES[name][1]
    if CASES[name][0][0] in (1, 30) and CASES[name][0][1] % 8 == 0:         # the planner's row lists and tile tables, whichever route the call takes
        assert size > 0 and size % 256 == 0
