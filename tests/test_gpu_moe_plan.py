"""-m gpu: the grouped MUL_MAT_ID prefill in its stream-k form (k_moe_sk_front: moe_sk_plan + the token-order quantizer; k_gemm_kq_sk) where the other tests never go:
planner jobs of several ROUNDS (with a partial last one, and the round sizes of 257+ experts), an expert with more rows than 16 bits count, skewed routing (everything to
one expert, most experts empty, no valid id at all, negative ids), ids with a token stride wider than n_used, tiles cut by span boundaries at small shapes (the second
parking slot, three and more parts), the full-size shape against the oracle over the WHOLE matrix, and spans that touch more tile records than the kernel's LDS window holds.

Expected values without a full-size oracle run: the activations are D distinct base rows, token i = base row i % D times 2**s_i (s_i cycles over -3 .. 3).  A power of two
goes through quantize_row_q8_K / quantize_row_q8_0, the fp16 image and the fp32 sums exactly, so expected[i, slot] = table[i % D, ids[i, slot]] * 2**s_i with table = the
oracle's MUL_MAT_ID of the D base rows with every expert selected (one oracle call of D * n_expert rows); test_scaled_rows_of_the_table_are_the_oracles_bits (CPU) checks
that bit for bit for Q4_K, Q4_0 and Q8_0 — it holds for all three, no format needed its scales dropped.

The plan is read back from the workspace (a mirror of moe_sk_carve, capi.hip) and compared with a numpy stable counting sort; what a case exists for (rounds > 1, parking
slot 1, parts >= 3, tiles per span > 8, zero tiles) is asserted from that read-back through a model of k_gemm_kq_sk's span walk, so that a case which stops reaching its path
fails.  "A first part in slot 1" is the geometric half of "the keeper reads slot 1": every keeper other than that first part's own span reads it there (who arrives last is a
race the result must not depend on)."""
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
from test_gpu_moe_front import _args

gpu = pytest.mark.gpu
TOL_GEMM = 1e-3
SENT = -77.0
REC, TR = 260, 128
ON_EMULATOR = os.environ.get("CDNA4_TESTS_ON_EMULATOR") == "1"


def _report(**kw):
    print("moe_plan:", json.dumps(kw))
    with open(R.out_path("moe_plan_report.jsonl"), "a") as f:
        f.write(json.dumps(kw) + "\n")


# ------------------------------------------------------------------------------------------------ inputs and expected values
@functools.lru_cache(maxsize=None)
def _problem(t, n_expert, m, k, D=61):
    """weights, the D base rows and the oracle's table [D][n_expert][m] — made once per (format, shape), shared and read-only"""
    w = R.random_weights(t, n_expert * m, k, seed=5)
    base = np.random.default_rng(D * 1000 + k).uniform(-1, 1, (D, k)).astype(np.float32)
    table = R.o_mul_mat_id(t, w, base[:, None, :], np.tile(np.arange(n_expert, dtype=np.int32), (D, 1)), m, k, n_expert)
    for a in (w, base, table):
        a.setflags(write=False)
    return w, base, table


def _scales(n_tok):
    return np.exp2((np.arange(n_tok) % 7 - 3).astype(np.float32))


def _acts(base, n_tok):
    return (base[np.arange(n_tok) % len(base)] * _scales(n_tok)[:, None])[:, None, :].astype(np.float32)      # [n_tok][n_b = 1][k]


def _expected(table, ids):
    n_tok, n_expert = len(ids), table.shape[1]
    valid = (ids >= 0) & (ids < n_expert)
    exp = table[(np.arange(n_tok) % len(table))[:, None], np.clip(ids, 0, n_expert - 1)] * _scales(n_tok)[:, None, None]
    exp[~valid] = SENT
    return exp.astype(np.float32), valid


def _mmid(L, t, wd, xd, idd, ids_tok_stride, n_expert, n_used, n_tok, m, k, ws=None):
    """one ggml_cdna4_mul_mat_id (n_b = 1) into a sentinel-filled buffer -> (y, workspace, front key)"""
    rb = R.row_size(t, k)
    if ws is None:
        # (zero-filled: whatever a wrong plan leaves unwritten then reads activation row 0 and stores to pair 0 — inside the buffers)
        ws = torch.zeros(L.ggml_cdna4_mul_mat_id_workspace_size(int(t), k, n_expert, n_used, 1, n_tok), dtype=torch.uint8, device="cuda")
    y = torch.full((n_tok, n_used, m), SENT, dtype=torch.float32, device="cuda")
    a = list(_args(t, wd, rb, m, xd, k, idd, y, n_expert, n_used, 1, n_tok, ws)); a[8] = ids_tok_stride
    key = L.ggml_cdna4_mul_mat_id_front_key(int(t), wd.data_ptr(), rb, m * rb, m, k, n_expert, n_used, 1, n_tok, ws.numel())
    _ok(L, L.ggml_cdna4_mul_mat_id(*a))
    torch.cuda.synchronize()
    return y, ws, key


_LAST = {}


def _compare(case, y, exp, valid):
    """full matrix: finite, the slots of ids out of range untouched, the rest within the GEMM bar of the oracle"""
    yn = np.array(y.cpu().numpy())
    e = R.rel_l2(yn[valid], exp[valid]) if valid.any() else 0.0
    _report(case=case, rel_l2=e, rows=int(valid.sum()))
    _LAST["rel_l2"] = e
    assert np.isfinite(yn).all()
    assert (yn[~valid] == SENT).all()
    assert e < TOL_GEMM, e
    return yn


def _same_inputs_same_bits(yn, ids):
    """K = 256: every tile is whole, an output row is a function of (expert, activation row) alone — pairs with the same expert, base row and scale hold the same bits"""
    n_tok, D = len(ids), 61
    key = ids[:, 0].astype(np.int64) * (7 * D) + np.arange(n_tok) % (7 * D)
    order = np.argsort(key, kind="stable"); ks = key[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    rep = order[np.maximum.accumulate(np.where(first, np.arange(n_tok), 0))]
    assert (~first).sum() > 0
    yb = yn[:, 0].view(np.int32)
    assert np.array_equal(yb[order], yb[rep])


# ------------------------------------------------------------------------------------------------ the plan, read back
def _spans_of_device():
    if os.environ.get("CDNA4_SK_SPANS", "0") not in ("", "0"):
        return min(int(os.environ["CDNA4_SK_SPANS"]), 1024)
    if ON_EMULATOR:
        return int(os.environ.get("EMU_CUS", "256"))
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 1024)


def _round_pairs(n_expert):
    """pairs per round of moe_sk_plan: CH * 64, CH = clamp(4096 / n_expert, 4 .. 16) rounded down to a multiple of 4"""
    ch = 4096 // n_expert
    return 64 * (16 if ch > 16 else 4 if ch < 4 else ch & ~3)


def _read_plan(ws, ids, n_expert, m, k):
    """(tile records [ntl][260], wg_begin[G + 2], G, units per tile, rows per expert) — a mirror of moe_sk_carve; checks itself against the ids first"""
    pairs = ids.size
    cap = min(n_expert, pairs) + pairs // 128 + 1
    off = (cap * REC * 4 + 255) // 256 * 256
    raw = np.array(ws[:off + 1026 * 4].cpu().numpy())
    rec, wb = raw[:cap * REC * 4].view(np.int32).reshape(cap, REC), raw[off:off + 1026 * 4].view(np.int32)
    G, upt = _spans_of_device(), (m + 127) // 128 * (k // 256)
    flat = ids.reshape(-1)
    cnt = np.bincount(flat[(flat >= 0) & (flat < n_expert)], minlength=n_expert)
    ntl = int(((cnt + TR - 1) // TR).sum())
    assert wb[0] == 0 and wb[G] == ntl * upt and wb[G + 1] == ntl, (wb[0], wb[G], wb[G + 1], ntl, upt, G)
    return rec[:ntl], wb[:G + 2], G, upt, cnt


def _check_plan(rec, wb, G, ids, n_expert, cnt, n_b=1):
    """against a stable counting sort of the ids: tile headers in expert order; an expert's dst entries, concatenated, are its pairs in increasing order; src = the pair's
    activation row; a pair with an id out of range appears nowhere; wg_begin non-decreasing"""
    n_used, flat = ids.shape[1], ids.reshape(-1)
    t, seen = 0, []
    for e in np.nonzero(cnt)[0]:
        pe = np.nonzero(flat == e)[0]
        for idx in range((cnt[e] + TR - 1) // TR):
            rows = min(TR, cnt[e] - TR * idx)
            assert tuple(rec[t, :4]) == (e, rows, idx, (rows + 31) // 32), (t, rec[t, :4])
            want = pe[TR * idx:TR * idx + rows]
            assert np.array_equal(rec[t, 4 + TR:4 + TR + rows], want), (t, e, idx)
            assert np.array_equal(rec[t, 4:4 + rows], want // n_used * n_b + want % n_used % n_b), (t, e, idx)
            seen.append(want); t += 1
    assert t == len(rec)
    seen = np.concatenate(seen) if seen else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(seen), np.nonzero((flat >= 0) & (flat < n_expert))[0])
    assert (np.diff(wb[:G + 1]) >= 0).all()


def _walk(wb, G, upt, nsb):
    """k_gemm_kq_sk's walk of its span, per work-group: segments that park in slot 1, the most parts of a cut tile, cut tiles whose FIRST part lies in slot 1 (what any other
    keeper reads with sl == 1), the most tiles one span touches, cut segments behind the 8th tile of their span (after a reload of the record window)"""
    c = dict(spans=0, slot1=0, nparts=1, first_in_slot1=0, tiles=0, cut_behind_window=0)
    for w in range(G):
        ub, ue = int(wb[w]), int(wb[w + 1])
        if ub >= ue:
            continue
        c["spans"] += 1; c["tiles"] = max(c["tiles"], (ue - 1) // upt - ub // upt + 1)
        u = ub
        while u < ue:
            sb0 = u % upt % nsb
            n = min(nsb - sb0, ue - u)
            if n != nsb:
                u0, p0, wl = u - sb0, w, w
                while wb[p0] > u0: p0 -= 1
                while wb[wl + 1] < u0 + nsb: wl += 1
                c["nparts"] = max(c["nparts"], wl - p0 + 1)
                c["slot1"] += u != ub
                c["first_in_slot1"] += p0 == w and wb[p0] < u0
                c["cut_behind_window"] += u // upt - ub // upt >= 8
            u += n
    return {a: int(b) for a, b in c.items()}


def _run_case(L, case, t, ids, n_expert, m, k, D=61, wd=None, ids_dev=None, stride=None, ws=None):
    """the call, the full-matrix compare, and — when it took the stream-k form — the plan invariants -> (y on the host, key, span classification or None)"""
    w, base, table = _problem(t, n_expert, m, k, D)
    n_tok, n_used = ids.shape
    wd = _dev(w) if wd is None else wd
    y, ws, key = _mmid(L, t, wd, _dev(_acts(base, n_tok)), _dev(ids) if ids_dev is None else ids_dev, stride or n_used, n_expert, n_used, n_tok, m, k, ws)
    cls = None
    if key != 0:
        rec, wb, G, upt, cnt = _read_plan(ws, ids, n_expert, m, k)
        _check_plan(rec, wb, G, ids, n_expert, cnt)
        cls = _walk(wb, G, upt, k // 256)
        cls["ntl"] = len(rec)
    yn = _compare(case, y, *_expected(table, ids))
    return yn, key, cls, ws


# ------------------------------------------------------------------------------------------------ CPU: the table is exact
def test_scaled_rows_of_the_table_are_the_oracles_bits():
    """(no GPU) ~200 random (token, expert) pairs: the oracle's MUL_MAT_ID of the scaled row equals table[i % D, e] * 2**s_i bit for bit — Q4_K (Q8_K activations), Q4_0 and
    Q8_0 (Q8_0 activations)"""
    n_expert, m, k, n = 8, 128, 256, 200
    rng = np.random.default_rng(11)
    tok, e = rng.integers(0, 70000, n), rng.integers(0, n_expert, (n, 1)).astype(np.int32)
    for t in (R.Q4_K, R.Q4_0, R.Q8_0):
        w, base, table = _problem(t, n_expert, m, k)
        x = (base[tok % 61] * np.exp2((tok % 7 - 3).astype(np.float32))[:, None])[:, None, :].astype(np.float32)
        direct = R.o_mul_mat_id(t, w, x, e, m, k, n_expert)
        derived = (table[tok % 61, e[:, 0]] * np.exp2((tok % 7 - 3).astype(np.float32))[:, None])[:, None, :].astype(np.float32)
        assert np.array_equal(direct.view(np.int32), derived.view(np.int32)), t


# ------------------------------------------------------------------------------------------------ 1, 2: several rounds
@gpu
@pytest.mark.parametrize("n_tok,holes", [(1025, False), (2500, False), (1025, True)], ids=["1025", "2500", "1025-holes"])
def test_planner_runs_several_rounds_with_a_partial_last_one(L, n_tok, holes):
    """8 experts, one used: 1024-pair rounds — 1025 pairs are one pair over, 2500 are two rounds and a part; `holes`: every 19th id out of range (-1, n_expert, n_expert + 7)"""
    n_expert, m, k = 8, 128, 256
    ids = np.random.default_rng(n_tok).integers(0, n_expert, (n_tok, 1)).astype(np.int32)
    if holes:
        ids[::19, 0] = np.resize(np.array([-1, n_expert, n_expert + 7], np.int32), len(ids[::19]))
    assert n_tok > _round_pairs(n_expert) and n_tok % _round_pairs(n_expert)
    yn, key, cls, _ = _run_case(L, "1:%d%s" % (n_tok, "-holes" if holes else ""), R.Q4_K, ids, n_expert, m, k)
    assert key != 0
    if not holes:
        _same_inputs_same_bits(yn, ids)


@gpu
@pytest.mark.parametrize("n_expert,n_used,n_tok,round_pairs", [(300, 2, 500, 768), (1024, 1, 700, 256)], ids=["300-2-500", "1024-1-700"])
def test_planner_rounds_of_many_experts(L, n_expert, n_used, n_tok, round_pairs):
    """CH = 12 (300 experts: 768-pair rounds, two of them) and CH = 4 (1024 experts: 256-pair rounds, three); most experts empty or holding one to three rows"""
    m, k = 32, 256
    rng = np.random.default_rng(n_expert)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    assert _round_pairs(n_expert) == round_pairs and ids.size > round_pairs
    cnt = np.bincount(ids.reshape(-1), minlength=n_expert)
    assert ((cnt >= 0) & (cnt <= 3)).mean() > 0.5 and (cnt == 0).any()
    _, key, cls, _ = _run_case(L, "2:%d" % n_expert, R.Q4_K, ids, n_expert, m, k)
    assert key != 0 and cls["ntl"] == int((cnt > 0).sum())


# ------------------------------------------------------------------------------------------------ 3: everything to one expert
@gpu
@pytest.mark.parametrize("fmt,target", [("q4_K", 0), ("q4_K", 3), ("q4_K", 7), ("q8_0", 3), ("q4_0r", 3)])
def test_every_pair_to_one_expert(L, fmt, target):
    """1100 pairs to expert 0 / 3 / 7 of 8: nine tiles of one expert, the others empty, two rounds with one key per chunk.  q8_0: the same ids through the other planner
    (k_moe_plan, the per-tile route); q4_0r: Q4_0 experts with a resident Q4_0R image of the stack, on the stream-k form"""
    from ggml_amd import native
    n_expert, n_tok, m, k = 8, 1100, 128, 256
    t = {"q4_K": R.Q4_K, "q8_0": R.Q8_0, "q4_0r": R.Q4_0}[fmt]
    ids = np.full((n_tok, 1), target, np.int32)
    wd = _dev(_problem(t, n_expert, m, k)[0])
    if fmt == "q4_0r":
        img = torch.empty(L.ggml_cdna4_resident_image_size(int(t), n_expert * m, k), dtype=torch.uint8, device="cuda")
        native.check(L.ggml_cdna4_resident_image_register(int(t), wd.data_ptr(), R.row_size(t, k), n_expert * m, k, img.data_ptr(), 1, None))
    try:
        yn, key, cls, _ = _run_case(L, "3:%s-%d" % (fmt, target), t, ids, n_expert, m, k, wd=wd)
    finally:
        if fmt == "q4_0r":
            assert L.ggml_cdna4_resident_image_unregister(wd.data_ptr()) == 0
    assert (key != 0) == (fmt != "q8_0")
    if key:
        assert cls["ntl"] == 9 and n_tok > _round_pairs(n_expert)
    _same_inputs_same_bits(yn, ids)


# ------------------------------------------------------------------------------------------------ 4: a rank beyond 16 bits
@gpu
@pytest.mark.parametrize("fmt,n_tok", [("q4_K", 65736), ("q4_K", 66000), ("q8_0", 65736)])
def test_an_expert_with_more_rows_than_16_bits_count(L, fmt, n_tok):
    """two experts, 200 tokens spread through the batch to expert 0, the rest to expert 1: 65536 rows (ranks up to 65535, the last value 16 bits hold) and 65800 rows (ranks
    beyond: before the fix of moe_sk_plan's table — running totals in 16 bits — those rows landed in expert 1's first tiles, status 0).  Full matrix, and the first and
    last 512 pairs of expert 1 row by row.  q8_0: the per-tile route's planner with the same ids"""
    n_expert, m, k = 2, 64, 256
    t = R.Q4_K if fmt == "q4_K" else R.Q8_0
    ids = np.ones((n_tok, 1), np.int32)
    ids[np.linspace(5, n_tok - 7, 200).astype(np.int64), 0] = 0
    assert (ids == 0).sum() == 200
    yn, key, cls, _ = _run_case(L, "4:%s-%d" % (fmt, n_tok), t, ids, n_expert, m, k)
    exp, _ = _expected(_problem(t, n_expert, m, k)[2], ids)
    pe = np.nonzero(ids[:, 0] == 1)[0]
    rows = np.r_[pe[:512], pe[-512:]]
    err = np.linalg.norm((yn[rows, 0] - exp[rows, 0]).astype(np.float64), axis=1) / np.linalg.norm(exp[rows, 0].astype(np.float64), axis=1)
    _report(case="4:%s-%d rows" % (fmt, n_tok), worst_row=float(err.max()))
    assert (err <= TOL_GEMM).all(), (rows[err > TOL_GEMM][:8], err.max())


# ------------------------------------------------------------------------------------------------ 5: no valid id
@gpu
def test_no_valid_id_plans_no_tile_and_writes_nothing(L):
    n_expert, n_used, n_tok, m, k = 4, 2, 40, 128, 512
    rng = np.random.default_rng(5)
    ids = rng.choice(np.array([-1, n_expert, n_expert + 7], np.int32), (n_tok, n_used))
    yn, key, cls, ws = _run_case(L, "5:none", R.Q4_K, ids, n_expert, m, k)
    assert key != 0 and cls["ntl"] == 0 and cls["spans"] == 0 and (yn == SENT).all()
    ids2 = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    _, key, cls, _ = _run_case(L, "5:then-valid", R.Q4_K, ids2, n_expert, m, k, ws=ws)
    assert key != 0 and cls["ntl"] == 4


# ------------------------------------------------------------------------------------------------ 6: strided ids
@gpu
@pytest.mark.parametrize("n_used", [1, 2])
def test_ids_with_a_wider_token_stride(L, n_used):
    """ids = the first column(s) of an (n_tok, 8) tensor, as llama.cpp passes a view of the argsort (the other columns hold ids out of range): bit-identical to contiguous ids"""
    n_expert, n_tok, m, k = 8, 1025, 128, 256
    rng = np.random.default_rng(6)
    wide = np.full((n_tok, 8), 99, np.int32)
    wide[:, :n_used] = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)])
    ids = np.ascontiguousarray(wide[:, :n_used])
    wd = _dev(_problem(R.Q4_K, n_expert, m, k)[0])
    y_c, key_c, _, _ = _run_case(L, "6:contiguous-%d" % n_used, R.Q4_K, ids, n_expert, m, k, wd=wd)
    y_w, key_w, _, _ = _run_case(L, "6:stride8-%d" % n_used, R.Q4_K, ids, n_expert, m, k, wd=wd, ids_dev=_dev(wide), stride=8)
    assert key_c != 0 and key_w != 0 and ids.size > _round_pairs(n_expert)
    assert np.array_equal(y_c.view(np.int32), y_w.view(np.int32))


# ------------------------------------------------------------------------------------------------ 7: cut tiles at small shapes
@gpu
@pytest.mark.parametrize("name,n_expert,n_used,counts,m,k,nparts", [("a", 3, 1, (200, 0, 100), 128, 768, 2), ("b", 2, 1, (129, 1), 128, 3840, 8), ("c", 4, 4, None, 300, 1280, 3)])
def test_cut_tiles_use_the_second_parking_slot_and_many_parts(L, name, n_expert, n_used, counts, m, k, nparts):
    """small jobs use fewer spans than any device has CUs (about two superblocks each), so the geometry does not depend on the device: a span that ends one tile and begins
    another (its second segment parks in slot 1, the keeper finds that first part there), and tiles of 2 / 8 / 3 parts"""
    rng = np.random.default_rng(7)
    if counts is None:
        ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(33)]).astype(np.int32)
    else:
        ids = rng.permutation(np.repeat(np.arange(n_expert, dtype=np.int32), counts))[:, None]
    _, key, cls, _ = _run_case(L, "7:" + name, R.Q4_K, ids, n_expert, m, k)
    _report(case="7:" + name, **cls)
    assert key != 0 and cls["slot1"] >= 1 and cls["first_in_slot1"] >= 1 and cls["nparts"] >= nparts, cls


# ------------------------------------------------------------------------------------------------ 8: the full-size shape, whole matrix
@gpu
def test_full_size_prefill_over_the_whole_matrix(L):
    """8 experts x 2 used x 512 tokens x 4096^2 (what test_mul_mat_id_grouped_prefill samples 24 tokens of): every output row against the oracle's table (D = 16), and 20
    repeated calls bit-equal to the first"""
    n_expert, n_used, n_tok, m, k, D = 8, 2, 512, 4096, 4096, 16
    rng = np.random.default_rng(8)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tok)]).astype(np.int32)
    w, base, _ = _problem(R.Q4_K, n_expert, m, k, D)
    wd, xd, idd = _dev(w), _dev(_acts(base, n_tok)), _dev(ids)
    yn, key, cls, ws = _run_case(L, "8:full", R.Q4_K, ids, n_expert, m, k, D=D, wd=wd)
    _report(case="8:full", **cls)
    assert key != 0 and cls["nparts"] >= 2
    y0 = _dev(yn)
    for _ in range(20):
        y, _, _ = _mmid(L, R.Q4_K, wd, xd, idd, n_used, n_expert, n_used, n_tok, m, k, ws)
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the record window (NWIN = 8 tile records in LDS)
def _window_case(L, k):
    """8 experts x 640 tokens, M 128: 40 full tiles -> {rel_l2, finite, span classification} (run with 4 spans at K 256 and 3 spans at K 768)"""
    n_expert, m = 8, 128
    ids = (np.arange(640 * n_expert, dtype=np.int32) % n_expert)[:, None]
    _, key, cls, _ = _run_case(L, "window:%d" % k, R.Q4_K, ids, n_expert, m, k)
    return dict(key=key, rel_l2=_LAST["rel_l2"], **cls)


@gpu
@pytest.mark.parametrize("k,spans", [(256, 4), (768, 3)])
def test_spans_longer_than_the_record_window(L, k, spans):
    """CDNA4_SK_SPANS (read once per process) in ONE fresh child per shape: 40 tiles over 4 spans — ten tiles each, the window of 8 reloads; over 3 spans with three
    superblocks per tile a cut tile is the 14th of its span, behind a reload.  (On the emulator the CU count stands in for the knob: EMU_CUS, no child.)"""
    if ON_EMULATOR:
        if int(os.environ.get("EMU_CUS", "256")) != spans:
            pytest.skip("needs EMU_CUS=%d (tests/test_gpu_tests_on_the_emulator.py sets it)" % spans)
        rec = _window_case(L, k)
    else:
        code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import test_gpu_moe_plan as T\nfrom ggml_amd import native\nprint(json.dumps(T._window_case(native.lib(), %d)))\n") % (R.ROOT, os.path.join(R.ROOT, "tests"), k)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, CDNA4_SK_SPANS=str(spans)))
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        rec = json.loads(r.stdout.strip().splitlines()[-1])
    _report(case="window:%d-%d" % (k, spans), **rec)
    assert rec["key"] != 0 and rec["ntl"] == 40 and rec["spans"] == spans and rec["rel_l2"] < TOL_GEMM, rec
    if k == 256:
        assert rec["tiles"] >= 9, rec
    else:
        assert rec["cut_behind_window"] >= 1, rec
