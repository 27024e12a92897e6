"""ggml_cdna4_op_mul_mat_f_route on BF16 weights (type 30), without a device (CDNA4_ASSUME_CUS names the part): the plan of gemm_f16_plan.hpp routes them like F16 —
0 refused, 1 k_mul_mat_f<bf16>, 2 k_gemv_bf16, 3 k_gemm_f16<.., bf16>; CDNA4_F16_GEMM=0 keeps every accepted call on 1."""
import json
import os
import subprocess
import sys

import pytest

import refutil as R
import test_f16_plan as F

# name -> (src0 type, M, K, N, src0 pointer offset, src0 nb1 - 2 K, src1 K - K, src0 ne2, src1 ne2), expected route
CASES = {"n1": ((30, 4096, 4096, 1, 0, 0, 0, 1, 1), 2), "n8": ((30, 4096, 4096, 8, 0, 0, 0, 1, 1), 2), "n512": ((30, 4096, 4096, 512, 0, 0, 0, 1, 1), 3),
         "k36": ((30, 4096, 36, 64, 0, 0, 0, 1, 1), 1), "src0+2": ((30, 4096, 4096, 64, 2, 0, 0, 1, 1), 1), "nb1+2": ((30, 4096, 4096, 64, 0, 2, 0, 1, 1), 1),
         "ne0": ((30, 4096, 4096, 64, 0, 0, 8, 1, 1), 0), "batch": ((30, 4096, 4096, 64, 0, 0, 0, 2, 3), 0), "broadcast": ((30, 64, 64, 200, 0, 0, 0, 2, 4), 3)}
CODE = F.CODE.replace("es = 2 if t == 1 else 4", "es = 4 if t == 0 else 2")      # test_f16_plan's child process, told that type 30 has 2-byte elements too


@pytest.mark.parametrize("knob", [None, "0"])
def test_bf16_routes(knob):
    import __graft_entry__ as g
    g.build()
    env = dict({k: v for k, v in os.environ.items() if k != "CDNA4_F16_GEMM"}, CDNA4_ASSUME_CUS="256", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", CODE, os.path.join(R.ROOT, "ggml_amd", "lib", "libcdna4_kernels.so"), json.dumps({k: v[0] for k, v in CASES.items()})],
                       capture_output=True, text=True, timeout=120, env=env if knob is None else dict(env, CDNA4_F16_GEMM=knob))
    assert r.returncode == 0, r.stderr[-800:]
    # the knob: route 1 wherever a bf16 kernel would run; a refused call stays refused
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {k: v[1] if knob is None else min(v[1], 1) for k, v in CASES.items()}
