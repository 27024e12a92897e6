"""-m gpu: the plug-in's scheduler-facing surface through ggml's public API (oracle/split_harness.cpp, compiled against the
reference headers): ggml_backend_split_buffer_type via get_proc_address, whole-tensor scatter / gather, the multi-shard MUL_MAT
(on a one-GPU box the shards all sit on device 0: GGML_CDNA4_SPLIT_SELF), async tensor copies between two backends with events,
the pinned host buffer type, and the capability bits — each result against the reference CPU backend on identical data."""
import json
import os
import subprocess

import pytest
import torch

import refutil as R

pytestmark = pytest.mark.gpu
PLUGIN = os.path.join(R.ROOT, "ggml_amd", "lib", "libggml-cdna4.so")
EXE = os.path.join(R.REF_DIR, "split_harness")


def _run(type_, m, k, b, shards):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    if not os.path.exists(EXE):
        pytest.fail("prebuilt oracle/_ref/split_harness missing from the snapshot")
    env = dict(os.environ, GGML_CDNA4_STATS="1")
    if shards:
        env["GGML_CDNA4_SPLIT_SELF"] = str(shards)
    r = subprocess.run([EXE, PLUGIN, type_, str(m), str(k), str(b)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    import re
    j["graph_captures_replays"] = [[int(a), int(b)] for a, b in re.findall(r"(\d+) HIP-graph captures, (\d+) replays", r.stderr)]
    j["ksplit_rccl_sums"] = [[int(a), int(b)] for a, b in re.findall(r"K-split MUL_MAT: (\d+) RCCL all-reduces, (\d+) in-order sums", r.stderr)]
    with open(R.out_path("split_report.jsonl"), "a") as f:
        f.write(json.dumps(dict(j, shards=shards)) + "\n")
    return j


@pytest.mark.parametrize("shards", [0, 2, 8])
@pytest.mark.parametrize("type_,m,k,b", [("q4_K", 4096, 4096, 512), ("q4_K", 1000, 2048, 1), ("q4_0", 2048, 1024, 33), ("q6_K", 640, 512, 7), ("q8_0", 300, 256, 130), ("q5_K", 4096, 1024, 64)])
def test_split_buffer_type_mul_mat(type_, m, k, b, shards):
    j = _run(type_, m, k, b, shards)
    assert j["set_get_roundtrip"] is True
    assert j["split_vs_cpu_rel_l2"] < (1e-3 if b > 8 else 1e-5), j
    assert j["split_vs_plain_rel_l2"] < 2e-6 or b <= 8, j            # same kernels on row sub-ranges: at most a different K split
    assert j["async_ok"] is True and j["host_buffer_ok"] is True
    assert j["caps_async"] is True and j["caps_host_buffer"] is True and j["caps_events"] is True


@pytest.mark.parametrize("shards,rccl", [(0, "1"), (0, "0"), (2, "1"), (8, "1"), (3, "1")])
@pytest.mark.parametrize("type_,m,k,b", [("q4_K", 4096, 4096, 512), ("q4_K", 1000, 2048, 1), ("q4_0", 2048, 1024, 33), ("q6_K", 640, 512, 7), ("q8_0", 300, 256, 130), ("q5_K", 4096, 1024, 64)])
def test_ksplit_buffer_type_mul_mat(type_, m, k, b, shards, rccl):
    """the K-split buffer type ("ggml_backend_cdna4_ksplit_buffer_type": the north star's all-reduce variant): columns [klo, khi) of
    every row per shard (2-D scatter / gather of byte ranges of the block rows: whole-tensor round trip), one ggml_cdna4_mul_mat per shard on ITS slice of
    the activations, the partial [B][M] outputs summed — by the RCCL all-reduce when every device holds a shard (shards = 0 on a one-GPU box: a
    communicator of one rank, the plumbing a node would run; rccl = "0": the peer-copy + ggml_cdna4_sum_partials fall-back), by the in-order sum where the
    shards share the device (2 / 8 / 3 slices; 3 does not divide the superblock count evenly; K = 256 leaves all but one shard empty).  Against the
    CPU backend and the unsplit product; deterministic."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    env_before = os.environ.get("GGML_CDNA4_KSPLIT_RCCL")
    os.environ["GGML_CDNA4_KSPLIT_RCCL"] = rccl
    try:
        j = _run(type_, m, k, b, shards)
    finally:
        if env_before is None:
            os.environ.pop("GGML_CDNA4_KSPLIT_RCCL", None)
        else:
            os.environ["GGML_CDNA4_KSPLIT_RCCL"] = env_before
    red = j["ksplit_rccl_sums"]
    assert red and sum(a + b for a, b in red) >= 4, j                 # two graphs x two computes went through the K-split path
    if shards == 0 and rccl == "1":
        assert sum(a for a, _ in red) >= 4 and sum(b for _, b in red) == 0, j      # the RCCL communicator did the reduction (one rank on this box)
    else:
        assert sum(a for a, _ in red) == 0, j
    assert j["ksplit_set_get_roundtrip"] is True and j["ksplit_deterministic"] is True, j
    assert 0 <= j["ksplit_vs_cpu_rel_l2"] < (1e-3 if b > 8 else 1e-5), j
    assert j["ksplit_vs_plain_rel_l2"] < (5e-4 if b > 8 else 2e-6), j   # GEMM path: per-shard fp16 rounding of other partial sums; GEMV: fp32 order only


@pytest.mark.parametrize("type_", ["q4_K", "q4_0", "q6_K"])
def test_unchanged_graph_is_replayed_from_a_hip_graph(type_):
    """an MLP block (NORM, MUL, ADD, MUL_MAT, ADD, GELU, MUL_MAT, ADD, ADD) computed six times with changing inputs, for 1 and for 96
    activation rows: the second appearance of the unchanged graph is captured (fused chains, the one-launch GEMV, the MFMA GEMM with its
    split-K hand-off whose flags are reset by their readers), the remaining four are replays; every result matches the CPU backend and
    input A replayed == input A computed eagerly, bit for bit.  VERDICT r1 item 6 (capture a split into a HIP graph)."""
    j = _run(type_, 512, 512, 16, 0)
    assert j["graph_replay_ok"] is True, j
    assert j["graph_replay_worst_rel_l2"] < 1e-2
    caps = j["graph_captures_replays"]
    # first backend: 2 captures (1 row, 96 rows) + 2 x 5 launches of the captured graphs, then two graphs (2 rows, 160 rows) taking
    # turns three times, as the splits of a ggml_backend_sched graph do: each keeps its own slot — 2 more captures, 2 x 2 launches
    assert [4, 14] in caps, caps
    # second backend: a captured 96-row graph, ONE eager run of an 8192-row graph that moves the backend's workspace and the library's
    # split-K scratch, then the small graph three more times: its cached exec holds stale addresses, so it must be dropped and the graph
    # captured again (at once: it has run before, nothing is left to size), then replayed twice — 2 captures, 2 + 3 launches — with
    # results identical to the first run (checked by the harness)
    assert [2, 5] in caps, caps
