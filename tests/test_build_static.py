"""Static properties of the compiled gfx950 kernels that the performance of the hot path depends on, checked from the
assembly hipcc emits (no GPU needed): the shipped kernels must not spill to scratch, the 12-wave kernel must fit three waves
per SIMD, and no work-group may ask for more than the CU's 160 KB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module", autouse=True)
def _emulators_built_in_parallel():
    """the CPU emulators (tools/emul) are built on demand by their check modules, one after the other; on a fresh checkout that is most of this
    file's run time, so build all of them here at once (each build is a no-op when its binary is newer than its sources)"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        return
    import importlib.util
    from concurrent.futures import ThreadPoolExecutor

    def mod(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "emul", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    jobs = [lambda: mod("emul_check").build("w12"), lambda: mod("emul_check").build("w8"), lambda: mod("emul_check").build("t64")]
    jobs += [mod(n).build for n in ("gemv_emul_check", "quant_emul_check", "convert_emul_check", "deq_emul_check", "fattn_emul_check", "lib_emul_check")]
    with ThreadPoolExecutor(max_workers=9) as ex:
        for f in [ex.submit(j) for j in jobs]:
            try:
                f.result()
            except Exception:  # noqa: BLE001 — the test that needs this emulator reports the build error
                pass


def _isa_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_manifest", os.path.join(ROOT, "tools", "isa_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gemm_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return _isa_tool().asm_of("gemm_q_mfma.hip")          # (cached compile shared with the manifest check: tools/isa_manifest.py)


def _prop(asm, kernel, name):                                        # (plain finds: the assembly of one source is tens of MB)
    key = ".set %s.%s, " % (kernel, name)
    i = asm.find(key)
    assert i >= 0, "kernel %s not found in the assembly" % kernel
    return int(re.match(r"\d+", asm[i + len(key):i + len(key) + 16]).group(0))


def _loops(body):
    """the depth-1 loops of a kernel body: from each loop header to the first s_cbranch_scc1 behind it (plain finds: a lazy DOTALL regex is quadratic on a chunk without one)"""
    out = []
    for chunk in body.split("Loop Header: Depth=1")[1:]:
        j = chunk.find("s_cbranch_scc1")
        if j >= 0:
            out.append(chunk[:j + len("s_cbranch_scc1")])
    return out


def _lds(asm, kernel):
    i = asm.find(".amdhsa_kernel %s\n" % kernel)
    assert i >= 0, kernel
    key = ".amdhsa_group_segment_fixed_size "
    j = asm.index(key, i)
    return int(re.match(r"\d+", asm[j + len(key):j + len(key) + 16]).group(0))


# mangled names: k_gemm_kq_w12<Q4_K, true, 0>, k_gemm_kq_w8p<Q5_K, false>, k_gemm_kq_w8<Q4_K, false, 20>
SHIPPED = [
    "_Z13k_gemm_kq_w12ILi12ELb1ELi0EEv11gemm_params",
    "_Z13k_gemm_kq_w8pILi13ELb0EEv11gemm_params",
    "_Z13k_gemm_kq_w8pILi12ELb0EEv11gemm_params",
    "_Z12k_gemm_kq_w8ILi12ELb0ELi20EEv11gemm_params",
]


@pytest.mark.parametrize("kernel", SHIPPED)
def test_shipped_gemm_kernels_do_not_spill(gemm_asm, kernel):
    assert _prop(gemm_asm, kernel, "private_seg_size") == 0
    assert _lds(gemm_asm, kernel) <= 160 * 1024


def test_64x128_wave_tile_kernel_resources(tmp_path):
    """gemm_q_t64.hip: 8 waves = 2 per SIMD -> at most 256 registers; no scratch access inside the main loop (the 256-row form
    parks one float4 in scratch in its EPILOGUE, which costs nothing); ring + reduction area within 160 KB of LDS"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    asm = _isa_tool().asm_of("gemm_q_t64.hip")

    def body_of(k):                                                     # (a 24-MB text: plain finds, not a DOTALL regex per kernel)
        i = asm.index("\n" + k + ":")
        return asm[i + 1:asm.index("\n.Lfunc_end", i)]
    # the plain product (TAIL = false; the tail-carrying twin shares the main loop) and — round 5 — the one-launch step that carries the activation quantizer and the
    # grid barrier in its prologue (FQ = true): the loop must be the same loop, in particular without a scratch access in it (a spill there would also break the
    # kernel's counted vmcnt waits, which assume that LDS-DMA is the only vector-memory traffic of the loop)
    # (type 102 = Q4_0R, round 5: Q4_0 through its resident 16-byte-aligned image — the same loop with a two-instruction constant step)
    for ty, tm, fq, max_scratch in ((12, 128, 0, 0), (12, 256, 0, 128), (12, 128, 1, 0), (102, 128, 0, 0), (102, 256, 0, 128)):
        k = "_Z13k_gemm_kq_t64ILi%dELi%dELb0ELi0ELb0ELb%dEEv11gemm_params" % (ty, tm, fq)
        assert _prop(asm, k, "num_vgpr") + _prop(asm, k, "num_agpr") <= 256
        assert _prop(asm, k, "private_seg_size") <= max_scratch
        assert _lds(asm, k) <= 160 * 1024
        body = body_of(k)
        # the steady-state stage pairs — one copy of the loop for the four loader waves, one for the others: no scratch access inside
        # (the 256-row form parks a few loader-only address registers in scratch AROUND the loops), 32 / 64 MFMAs each
        # (a loop = from its header to the first backward branch BEFORE the next loop's header: the quantizer's rolled loop in the FQ prologue ends in another branch form)
        loops = _loops(body)
        main = [lp for lp in loops if lp.count("v_mfma_f32_32x32x16_f16") == (32 if tm == 128 else 64)]
        assert len(main) == 2 and all("scratch_" not in lp for lp in main)
        assert sorted(lp.count("global_load_lds_dwordx4") for lp in main)[0] == 0        # the non-loader copy issues no LDS-DMA at all
    # the grouped MUL_MAT_ID instantiations (IDS; Q4_K and — round 5 — Q4_0R on a resident image of the expert stack): no scratch access in any loop that issues MFMAs
    for ty in (12, 102):
        for tm in (128, 256):
            k = "_Z13k_gemm_kq_t64ILi%dELi%dELb1ELi0ELb0ELb0EEv11gemm_params" % (ty, tm)
            assert _prop(asm, k, "num_vgpr") + _prop(asm, k, "num_agpr") <= 256 and _lds(asm, k) <= 160 * 1024
            body = body_of(k)
            loops = _loops(body)
            mf = [lp for lp in loops if "v_mfma_f32_32x32x16_f16" in lp]
            assert len(mf) >= 2 and all("scratch_" not in lp for lp in mf), k
    # nothing in this file loads into registers asynchronously: round 2's first version did (superblock headers, inline-asm
    # global_load_dwordx4 waited for a stage later) and hipcc copied the in-flight registers before the wait — one wave in a few
    # thousand got garbage constants on the GPU, invisibly to the CPU emulator.  Headers go through LDS (DMA) now.
    # (round 5: the one-launch step's prologue loads the fp32 activations into registers — compiler-issued, compiler-counted loads in front of the grid barrier, never
    #  beside the loop's hand-counted LDS-DMA: every one of them precedes the kernel's first MFMA; the kernels without the quantizer still have none)
    for name in sorted(set(re.findall(r"^(_Z13k_gemm_kq_t64\w+):", asm, re.M))):
        kbody = body_of(name)
        regloads = [m.start() for m in re.finditer(r"global_load_dwordx[24] v", kbody)]
        if name.endswith("ELb1EEv11gemm_params"):
            assert regloads and max(regloads) < kbody.index("v_mfma_f32_32x32x16_f16"), name
        else:
            assert not regloads, name


@pytest.mark.parametrize("m,k,b,splitk,tm", [(128, 256, 128, 1, 128), (300, 1536, 200, 1, 128), (300, 1536, 200, 1, 256), (513, 1024, 129, 2, 128),
                                             (256, 1792, 128, 2, 128), (512, 1792, 200, 2, 256), (200, 256, 100, 1, 256),
                                             (200, 2304, 40, 4, 128), (128, 4352, 9, 8, 128), (300, 2048, 130, 8, 128)])      # deep split: 9 / 17 / 8 superblocks over 4 / 8 / 8 work-groups
def test_64x128_wave_tile_kernel_source_on_the_cpu(m, k, b, splitk, tm):
    """tools/emul/t64_emul: the source of k_gemm_kq_t64 executed on the CPU against a direct fp16 product — both tile heights,
    ragged edges, one-superblock K ranges, even and uneven hand-off splits (the harness also checks that every exchange flag
    was reset by its reader) — with the LDS-DMA landing immediately and as late as the counted waits allow"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for defer in (False, True):
        assert mod.run(m, k, b, seed=m + k, timeout=900, splitk=splitk, kernel="t64", exp=tm, defer_dma=defer) < 1e-6


@pytest.mark.parametrize("m,k,b,e", [(128, 512, 384, 2), (256, 1024, 512, 3)])
def test_grouped_mul_mat_id_kernel_source_on_the_cpu(m, k, b, e):
    """k_gemm_kq_t64<Q4_K, 128, IDS> (the grouped MUL_MAT_ID launch): per-tile expert matrices, an unused tile whose work-groups exit, padding
    rows that are not stored, output rows scattered through row_dst — against the per-expert fp16 product, DMA landing immediately and late"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for defer in (False, True):
        err, untouched = mod.run_ids(m, k, b, e, seed=m + e, defer_dma=defer)
        assert err < 1e-6 and untouched


def test_64x128_wave_tile_kernel_counted_waits_are_tight(monkeypatch):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setenv("EMU_WEAKEN_WAITS", "1")
    assert mod.run(300, 1536, 200, seed=3, timeout=900, splitk=1, kernel="t64", exp=128, defer_dma=True) > 1e-3


def test_loader_wave_kernel_fits_three_waves_per_simd(gemm_asm):
    # 12 waves per work-group = 3 per SIMD: 512 registers / 3, allocation granule 8
    for k in ("_Z13k_gemm_kq_w12ILi12ELb1ELi0EEv11gemm_params", "_Z13k_gemm_kq_w12ILi202ELb1ELi0EEv11gemm_params",
              "_Z13k_gemm_kq_w12ILi208ELb1ELi0EEv11gemm_params", "_Z13k_gemm_kq_w12ILi214ELb1ELi0EEv11gemm_params"):
        assert _prop(gemm_asm, k, "num_vgpr") + _prop(gemm_asm, k, "num_agpr") <= 168


def test_two_waves_per_simd_kernels_fit_256_registers(gemm_asm):
    for k in SHIPPED[1:]:
        assert _prop(gemm_asm, k, "num_vgpr") + _prop(gemm_asm, k, "num_agpr") <= 256


@pytest.mark.parametrize("m,k,b,splitk,exp,l2", [(300, 1536, 200, 1, 0, 1), (256, 2048, 128, 2, 0, 1), (256, 2048, 128, 2, 0, 0), (256, 1024, 128, 1, 100, 1),
                                              (256, 1792, 128, 2, 0, 1), (300, 2304, 200, 2, 0, 0),          # ODD superblock counts: uneven 4 / 3 and 5 / 4 hand-off splits (the default route for odd counts)
                                              (513, 3072, 129, 2, 1, 1), (513, 3072, 129, 2, 2, 0), (300, 1536, 200, 1, 4, 1), (256, 2048, 128, 2, 6, 1)])
def test_shipped_12_wave_kernel_source_and_its_candidates_on_the_cpu(m, k, b, splitk, exp, l2):
    """tools/emul/w12_emul: the source of k_gemm_kq_w12 (+ the shared epilogue) executed on the CPU.  exp 0 is the shipped
    kernel (GPU-verified: this checks the emulator against it), 100 the variant without the loaders' scale table, 1 / 2 / 4 / 6
    the candidates kept in ablation builds (early table read, balanced epilogue, stores from registers, both): each must give
    the shipped kernel's result BIT FOR BIT, through both exchange transports"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    err, y = mod.run(m, k, b, seed=5, timeout=600, splitk=splitk, kernel="w12", exp=exp, xchg_l2=l2, return_y=True)
    assert err < 1e-6
    if exp != 0:
        _, y0 = mod.run(m, k, b, seed=5, timeout=600, splitk=splitk, kernel="w12", exp=0, xchg_l2=1, return_y=True)
        assert np.array_equal(y, y0)


@pytest.mark.parametrize("kernel,m,k,b,splitk,exp", [("w12", 300, 1536, 200, 1, 0), ("w12", 256, 2048, 128, 2, 0)])
def test_counted_vmcnt_waits_are_sufficient_and_tight(kernel, m, k, b, splitk, exp, monkeypatch):
    """EMU_DEFER_DMA=1: every LDS-DMA copy lands as LATE as the hardware permits — only when an s_waitcnt vmcnt(n) of the issuing
    wave retires it, in order — so a missing or too-weak wait leaves stale bytes in LDS.  Both kernels pass as written, and fail
    as soon as every wait tolerates one more outstanding operation (the self-test of this check)"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(m, k, b, seed=3, timeout=600, splitk=splitk, kernel=kernel, exp=exp, defer_dma=True) < 1e-6
    monkeypatch.setenv("EMU_WEAKEN_WAITS", "1")
    assert mod.run(m, k, b, seed=3, timeout=600, splitk=splitk, kernel=kernel, exp=exp, defer_dma=True) > 1e-3


def test_no_out_of_bounds_access_at_the_shape_that_faulted_on_the_gpu(tmp_path):
    """DESIGN.md 4.3, open issue: a gemm_bench process at 8192 x 8192 x 512 died with a GPU fault.  The emulator places every
    global buffer between inaccessible pages; the first and the last work-group of the shipped kernel at that shape (64 stages
    each, full-size W / activation image / Y) run without touching them"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    M, K, B = 8192, 8192, 512
    rng = np.random.default_rng(0)
    nb = M * K // 256
    w = rng.integers(0, 256, (nb, 144), dtype=np.uint8)
    w[:, 0:2] = rng.uniform(0.001, 0.004, nb).astype(np.float16).view(np.uint8).reshape(nb, 2)
    w[:, 2:4] = rng.uniform(0.01, 0.03, nb).astype(np.float16).view(np.uint8).reshape(nb, 2)
    w.tofile(str(tmp_path / "w.bin"))
    rng.uniform(-1, 1, (K // 128, B, 128)).astype(np.float16).tofile(str(tmp_path / "xh.bin"))
    exe = mod.build("w12")
    for blocks in ("0:1", "255:256"):
        r = subprocess.run([exe, str(M), str(K), str(B), str(tmp_path / "w.bin"), str(tmp_path / "xh.bin"), str(tmp_path / "y.bin"), "1", "0", "1"],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, EMU_BLOCKS=blocks))
        if r.returncode == 77:
            pytest.skip("the environment cannot host the emulation (process / thread limits)")
        assert r.returncode == 0, (blocks, r.stderr[-300:])
    y = np.fromfile(str(tmp_path / "y.bin"), np.float32).reshape(B, M)
    assert np.isfinite(y[-128:, -128:]).all() and not (y[-128:, -128:] == -12345.0).any()      # the last work-group's tile was written


def _reads_before_wait(asm, kernel):
    """inline-asm register loads (global_load_dwordx4 into VGPRs) whose destination is read by ANY later instruction before
    the next s_waitcnt vmcnt — the compiler treats an asm output as available at once, the hardware does not interlock"""
    m = re.search(r"^%s:.*?^\.Lfunc_end" % re.escape(kernel), asm, re.S | re.M)
    assert m, kernel
    lines = [ln.split(";")[0].rstrip() for ln in m.group(0).split("\n") if ln.strip() and not ln.strip().startswith(";")]
    n, bad = 0, []
    for i, ln in enumerate(lines):
        mm = re.match(r"\s*global_load_dwordx4 v\[(\d+):(\d+)\], v", ln)
        if not mm:
            continue
        n += 1
        regs = set(range(int(mm.group(1)), int(mm.group(2)) + 1))
        for t in lines[i + 1:i + 400]:
            if "s_waitcnt" in t and "vmcnt" in t:
                break
            parts = t.split(None, 1)
            if len(parts) < 2:
                continue
            ops = [x.strip() for x in parts[1].split(",")]
            srcs = ops if parts[0].startswith(("global_load_lds", "s_", "ds_write", "global_store", "buffer_store")) else ops[1:]
            used = set()
            for x in srcs:
                for a, b in re.findall(r"v\[(\d+):(\d+)\]", x):
                    used |= set(range(int(a), int(b) + 1))
                used |= {int(a) for a in re.findall(r"\bv(\d+)\b", x)}
            if used & regs:
                bad.append((ln.strip(), t.strip()))
                break
    return n, bad


def test_asynchronous_register_loads_are_not_read_before_their_wait(gemm_asm):
    """k_gemm_kq_w12's loader waves load superblock headers into registers with inline asm and wait for them later with a
    vmcnt wait tied to those registers.  Nothing stops the compiler from copying the registers in between (it did, in a first
    cut of the experimental kernel); the shipped binary must be free of such reads"""
    ks = re.findall(r"^(_Z13k_gemm_kq_w12ILi\d+ELb1ELi0EEv11gemm_params):", gemm_asm, re.M)
    assert len(ks) >= 4, ks                                    # Q4_K and the three staged forms (Q4_0, Q8_0, Q6_K re-laid by the loader waves)
    for k in ks:
        n, bad = _reads_before_wait(gemm_asm, k)
        assert n > 0 and not bad, (k, bad[:3])


@pytest.mark.parametrize("ncol", [2, 3, 8])
@pytest.mark.parametrize("t", [12, 13, 14, 2, 8])
def test_small_batch_decode_kernel_source_on_the_cpu(t, ncol):
    """tools/emul/gemv_emul: k_gemv_q_fused<.., NB> for 2..8 activation rows in ONE launch (every work-group quantizes the rows into
    LDS — bit-exact quantizer bodies — and each weight unit meets all columns from there), the five main formats, against the oracle;
    3 rows run the 4-column instantiation with its padding column repeating the last row"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemv_emul_check", os.path.join(ROOT, "tools", "emul", "gemv_emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(t, 37, 2048, seed=t + ncol, ncol=ncol) < 1e-5
    # ... and the form that is handed pre-quantized rows (one quantize launch for all work-groups) and only copies them into LDS
    assert mod.run_cols(t, 37, 2048, ncol, seed=t + ncol, staged=True) < 1e-5


@pytest.mark.parametrize("cfg", [0, 1])                       # 4 waves x 1 row, 8 waves x 2 rows (the M >= 4096 default)
@pytest.mark.parametrize("t", [12, 13, 14, 2, 8, 6, 10, 11, 3, 7, 20, 23])  # Q4_K, Q5_K, Q6_K, Q4_0, Q8_0, Q5_0, Q2_K, Q3_K, Q4_1, Q5_1 (in-launch Q8_1 quantizer), IQ4_NL, IQ4_XS
def test_decode_kernel_source_on_the_cpu(t, cfg):
    """tools/emul/gemv_emul: the source of the one-launch decode step (k_gemv_q_fused: in-kernel Q8_K / Q8_0 activation quantizer,
    int8 dots, wave reduction) executed on the CPU against the oracle's MUL_MAT — a GPU-free regression check of the B = 1 path"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemv_emul_check", os.path.join(ROOT, "tools", "emul", "gemv_emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(t, 37, 2048, seed=t + cfg, env={"CDNA4_FUSED_CFG": str(cfg)}) < 1e-5


@pytest.mark.parametrize("k", [2048, 12288])                  # one round of 64 units / three rounds (the register sets trade places twice)
@pytest.mark.parametrize("t", [12, 13, 14, 2, 10, 11, 23])    # the formats whose launcher can choose 16 waves x 1 row (K-quants and Q4_0)
@pytest.mark.parametrize("cfg", [4, 1, 3])                    # 16 x 1 (round 5), 8 x 2 (swapped loop), 8 x 1 (copying loop)
def test_decode_kernel_configurations_on_the_cpu(t, cfg, k):
    """round 5's decode configurations: 1024-thread work-groups with one row per wave, and the two forms of the multi-round loop (alternating register sets / copies),
    on rows of one and of three rounds — the kernel's source against the oracle's MUL_MAT"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    if k > 2048 and t not in (12, 14, 2):
        pytest.skip("the long rows: three formats are enough (emulation time)")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemv_emul_check", os.path.join(ROOT, "tools", "emul", "gemv_emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(t, 19, k, seed=t + cfg, env={"CDNA4_FUSED_CFG": str(cfg)}) < 1e-5


@pytest.mark.parametrize("kern,wtype,m,k,b,splitk", [(20, 12, 300, 1536, 200, 1), (20, 12, 256, 2048, 128, 2), (64, 12, 300, 1536, 200, 1), (64, 13, 256, 2048, 128, 2),
                                                     (64, 13, 300, 1536, 200, 1), (20, 13, 300, 512, 200, 1), (1064, 12, 256, 2048, 128, 2), (64, 13, 256, 1792, 128, 2)])
def test_8_wave_kernel_sources_on_the_cpu(kern, wtype, m, k, b, splitk):
    """tools/emul/w8_emul: k_gemm_kq_w8 (schedule 20: the shallow-K fallback and the kernel of the repacked formats) and
    k_gemm_kq_w8p (64: Q5_K's default; 1064: its TRACE build), Q4_K and Q5_K weights, executed on the CPU — with the LDS-DMA
    landing immediately and as late as the counted waits allow"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("emul_check", os.path.join(ROOT, "tools", "emul", "emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for defer in (False, True):
        assert mod.run(m, k, b, seed=m + k, timeout=600, splitk=splitk, kernel="w8", exp=kern, wtype=wtype, defer_dma=defer) < 1e-6


@pytest.mark.parametrize("kind,k,b,dist", [(0, 4096, 8, "uniform"), (0, 2048, 32, "ties"), (1, 4096, 8, "uniform"), (1, 1024, 32, "ties"), (2, 1024, 32, "ties"),
                                           (3, 2048, 8, "uniform"), (3, 1024, 16, "ties")])       # 3 = Q8_1 (k_quantize_q8_1: d, s = fp16(d * sum q), quants, image)
def test_activation_quantizer_sources_on_the_cpu_bit_exact(kind, k, b, dist):
    """tools/emul/quant_emul: k_quantize_q8_K / k_quantize_q8_0 (AVX2 and _ref roundings) executed on the CPU equal the oracle's
    quantize_row_q8_K / _q8_0 bit for bit — quants, scales, bsums — and their fp16 activation image equals fp16(d*q) in the
    panel-major, pair-interleaved layout; all-zero blocks, a negative maximum and exact .5 ties included"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("quant_emul_check", os.path.join(ROOT, "tools", "emul", "quant_emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(kind, k, b, dist=dist, seed=kind + k)


@pytest.mark.parametrize("t", [12, 13, 14, 2, 8, 6, 10, 11, 3, 7, 20, 23])
def test_multi_column_gemv_source_on_the_cpu(t):
    """tools/emul/gemv_emul: k_gemv_q (2 <= B <= 8 columns share one pass over the weights) on activations quantized by the
    oracle, against the oracle's MUL_MAT"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gemv_emul_check", os.path.join(ROOT, "tools", "emul", "gemv_emul_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run_cols(t, 33, 2048, 3, seed=t) < 1e-5
    assert mod.run_cols(t, 16, 1024, 8, seed=t + 1) < 1e-5


def _emul_module(name):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("ROCm clang not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "emul", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("wtype", [2, 8, 14])         # ggml type ids: Q4_0, Q8_0, Q6_K
def test_r8_on_the_resident_relayouts_counted_waits_are_sufficient_and_tight(wtype):
    """k_gemm_r8<Q4_0R | Q8_0R | Q6_K8> (round 5) on the CPU with every LDS-DMA copy performed as LATE as its counted vmcnt wait allows: correct (Q8_0R issues TWO raw pieces per K
    tile, so the loop's wait tolerates two outstanding operations instead of one); with every wait weakened by one the result is wrong — the waits are not slack.  Also the
    reduce-scatter split in two and a ragged tile."""
    mod = _emul_module("emul_check")
    assert mod.run_relayout(300, 1280, 200, wtype, defer_dma=True) < 1e-6
    assert mod.run_relayout(256, 1024, 256, wtype, splitk=2, defer_dma=True) < 1e-6
    assert mod.run_relayout(256, 768, 256, wtype, defer_dma=True, weaken=1) > 1e-2


@pytest.mark.parametrize("t,m,k", [(6, 8, 1024), (6, 33, 64), (11, 8, 1024), (11, 33, 512), (10, 8, 1024), (10, 33, 512), (10, 5, 256),
                                   (20, 8, 1024), (20, 33, 64), (3, 8, 1024), (3, 33, 128), (7, 8, 1024), (7, 33, 128), (23, 8, 1024), (23, 33, 256)])
def test_weight_reencoding_sources_on_the_cpu_are_exact(t, m, k):
    """tools/emul/convert_emul: k_convert_q5_0_q8_0 / k_convert_q3_K_q6_K / k_convert_q2_K_q6_K2 (the prefill route of Q5_0 / Q3_K / Q2_K)
    executed on the CPU: the oracle's dequantize_row of the re-encoded matrix equals its dequantize_row of the source bit for bit, on fully
    random block bytes; for Q2_K the sum of its two parts (scale part + minimum part, 2 K columns) equals it value for value.  Likewise IQ4_NL -> Q8_0
    (k_convert_iq4_nl_q8_0), Q4_1 / Q5_1 -> [d q | m 1] in Q8_0 (k_convert_q41_q8_0x2: the sum of the two parts bit for bit) and IQ4_XS -> [h part | l part]
    in Q6_K (k_convert_iq4_xs_q6_K2: value for value)"""
    assert _emul_module("convert_emul_check").run(t, m, k, seed=t + k)


@pytest.mark.parametrize("t", [2, 3, 6, 7, 8])
def test_fp16_copy_of_a_quantized_kv_source_on_the_cpu_bit_exact(t):
    """tools/emul/deq_emul f16: k_q_to_f16_dense (the pass in front of FLASH_ATTN_EXT when K / V arrive quantized) on strided rows equals
    fp16(oracle to_float) bit for bit, densely packed"""
    assert _emul_module("deq_emul_check").run_f16(t, 128, seed=t) and _emul_module("deq_emul_check").run_f16(t, 64, nrows=4, gap=0, seed=t + 1)


@pytest.mark.parametrize("t", [2, 8, 3, 6, 7])
def test_cpy_quantizer_sources_on_the_cpu_byte_exact(t):
    """tools/emul/deq_emul cpyq: ggml_cdna4_op_cpy F32 -> Q4_0 / Q8_0 / Q4_1 / Q5_0 / Q5_1 (k_cpy_f32_to_q, k_cpy_f32_to_q45) executed on the CPU equals the
    oracle's quantize_row_*_ref byte for byte (all-zero, constant and negative-maximum blocks included)"""
    mod = _emul_module("deq_emul_check")
    assert mod.run_cpyq(t, seed=t) and mod.run_cpyq(t, 512, 7, "normal", seed=t + 1)


@pytest.mark.parametrize("t", [2, 3, 6, 7, 8, 10, 11, 12, 13, 14, 20, 23])
def test_to_float_sources_on_the_cpu_bit_exact(t):
    """tools/emul/deq_emul: deq_elem of ops.hip (dequantize_row, GET_ROWS, CPY -> F32) executed on the CPU equals the oracle's dequantize_row_*
    bit for bit for all twelve block formats, on fully random block bytes"""
    assert _emul_module("deq_emul_check").run(t, 32 * 256 if t > 9 else 32 * 24, seed=t)


FATTN_EMUL_CASES = [dict(D=64, n_q=5, n_head=2, n_kv=96), dict(D=128, n_q=35, n_head=4, n_kv=200, n_head_kv=2, max_bias=8.0), dict(D=128, n_q=35, n_head=4, n_kv=200, n_head_kv=2, max_bias=8.0, cus=2),
                    dict(D=128, n_q=3, n_head=2, n_kv=64, softcap=10.0), dict(D=256, n_q=33, n_head=2, n_kv=130, n_head_kv=1, mask=False, cus=1),
                    dict(D=64, n_q=1, n_head=3, n_kv=517, inf_every=7), dict(D=128, n_q=40, n_head=2, n_kv=300, n_batch=2, permuted=True, cus=4),
                    dict(D=64, n_q=32, n_head=2, n_kv=31), dict(D=256, n_q=1, n_head=2, n_kv=1024, max_bias=8.0, inf_every=5), dict(D=128, n_q=2, n_head=2, n_kv=2048, inf_every=3),
                    dict(D=64, n_q=130, n_head=2, n_kv=257, inf_every=4), dict(D=64, n_q=130, n_head=2, n_kv=256, inf_every=4, cus=2),
                    dict(D=64, n_q=70, n_head=2, n_kv=1024, inf_every=4, max_bias=8.0), dict(D=256, n_q=200, n_head=1, n_kv=96, n_batch=2, cus=2),
                    dict(D=128, n_q=512, n_head=2, n_kv=512, n_head_kv=1, cus=8, inf_every=3)]


@pytest.mark.parametrize("kw", FATTN_EMUL_CASES)
def test_flash_attn_source_on_the_cpu(kw):
    """tools/emul/fattn_emul: k_flash_attn_split (+ k_flash_attn_merge when the keys are split over work-groups: the n_kv >= 512 cases; one or
    several 32-row query tiles) and k_flash_attn_wide (the `cus` cases — chosen when 128-row tiles fill the chip: K / V chunks and the
    transposed V fragments shared through LDS); masks on the vector path (16-byte aligned rows, transposed by the matrix core, -inf
    included) and on the element path (n_kv not a multiple of 8, ragged last chunk) — S^T = K.Q^T, V transposed on the matrix
    core, O^T += Vt^T.P^T — executed on the CPU with the MFMA emulated lane for lane: <= 5e-4 from a float64 evaluation of the operator, <= 6e-3 from the
    oracle (whose FP16 accumulator — the reference's, ggml-cpu.c:10960-10974 — is the larger part of that distance).  Grouped-query heads,
    ALiBi, softcap, no mask, -inf mask entries incl. a fully masked stretch, batches, permuted operands, ragged n_q / n_kv."""
    r = _emul_module("fattn_emul_check").run(**kw)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 5e-4 and r[1] < 6e-3, r


@pytest.mark.parametrize("t,kw", [(8, dict(D=64, n_q=5, n_head=2, n_kv=96)), (2, dict(D=128, n_q=3, n_head=4, n_kv=70, n_head_kv=2, permuted=True)),
                                  (3, dict(D=256, n_q=40, n_head=2, n_kv=200, cus=1)), (6, dict(D=128, n_q=1, n_head=4, n_kv=1024, n_head_kv=1)), (7, dict(D=64, n_q=33, n_head=2, n_kv=130))])
def test_flash_attn_on_a_quantized_kv_end_to_end_on_the_cpu(t, kw):
    """tools/emul/fattn_emul with a block-quantized K / V: ggml_cdna4_op_flash_attn_ext's own host code (scratch, descriptors), the conversion pass
    k_q_to_f16_dense and the F16 kernels, all from source on the CPU — <= 5e-4 from a float64 evaluation on the dequantized K / V and bit-identical
    to the F16 path on a cache that holds fp16(to_float(K)), fp16(to_float(V)); strided (permuted) rows, grouped-query heads, both kernels"""
    r = _emul_module("fattn_emul_check").run_quantized(t, seed=t, **kw)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 5e-4 and r[1] is True, r


@pytest.mark.parametrize("kw", [dict(D=80, n_q=5, n_head=2, n_kv=96), dict(D=80, n_q=35, n_head=4, n_kv=200, n_head_kv=2, max_bias=8.0, cus=2), dict(D=80, n_q=3, n_head=2, n_kv=70, permuted=True, n_batch=2),
                                dict(D=96, n_q=33, n_head=2, n_kv=130, mask=False), dict(D=112, n_q=1, n_head=3, n_kv=517, inf_every=7), dict(D=40, n_q=4, n_head=2, n_kv=64), dict(D=200, n_q=7, n_head=2, n_kv=90)])
def test_flash_attn_padded_head_sizes_end_to_end_on_the_cpu(kw):
    """head sizes without a kernel of their own (80 — the stock harness's —, 96, 112, 40, 200) run zero-padded to 64 / 128 / 256: the op's host code
    (padded copies of q / k / v, the result copied back) and the kernels from source on the CPU, same bars as the native head sizes"""
    r = _emul_module("fattn_emul_check").run(**kw)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 5e-4 and r[1] < 6e-3, r


def test_flash_attn_padded_head_size_with_a_quantized_kv_on_the_cpu():
    mod = _emul_module("fattn_emul_check")
    for t, D in ((8, 96), (2, 96), (7, 160)):
        r = mod.run_quantized(t, D, 5, 2, 96, seed=t)
        if r is None:
            pytest.skip("the environment cannot host the emulation")
        assert r[0] < 5e-4 and r[1] is True, (t, D, r)


# FLASH_ATTN_EXT launch plans (fattn.hip's fa_make_plan through `fattn_emul plan`).  Shape: "D n_q n_head n_batch n_kv n_head_kv kv_type mask softcap max_bias" (kv_type: 1 F16, 30 BF16,
# 8 Q8_0, 2 Q4_0, 3 Q4_1; mask: 0 none, 1 rows 16-byte aligned, 2 at a 2-byte offset), 256 CUs.  The expected values are what the launcher did BEFORE it had a plan: recorded from
# its launches (kernel, grids, LDS bytes, scratch sizes, fattn_params) with the launch calls replaced by prints — not taken from fa_make_plan.
FATTN_PLAN_TABLE = [
    # the pipelined kernel: 8 / 4 waves at head size 128, 8 / 4 / 2 at 64; modes 0 (no mask) / 1 (aligned mask) / 2 (softcap, unaligned mask); the flag pass from 2^20 mask entries on
    ("128 4096 32 1 4096 32 1 1 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=8 mode=1 map=1 nsplit=1 chunks_per_split=128 pack=0 merge=none grid=512,1,1 block=512 lds=139280 mgrid=1,1,1 fgrid=64,16,1 part_bytes=0 flag_bytes=1280"),
    ("128 4096 32 1 4096 32 1 0 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=8 mode=0 map=0 nsplit=1 chunks_per_split=128 pack=0 merge=none grid=512,1,1 block=512 lds=73744 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("128 1024 32 1 1024 32 1 1 30 0", "stage=none family=pipe kv_type=1 hs=128 nw=4 mode=2 map=1 nsplit=1 chunks_per_split=32 pack=0 merge=none grid=256,1,1 block=256 lds=73744 mgrid=1,1,1 fgrid=16,8,1 part_bytes=0 flag_bytes=384"),
    ("128 1024 32 1 1024 8 1 2 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=4 mode=2 map=1 nsplit=1 chunks_per_split=32 pack=0 merge=none grid=256,1,1 block=256 lds=73744 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("64 4096 32 1 4096 32 1 1 0 0", "stage=none family=pipe kv_type=1 hs=64 nw=8 mode=1 map=1 nsplit=1 chunks_per_split=128 pack=0 merge=none grid=512,1,1 block=512 lds=106512 mgrid=1,1,1 fgrid=64,16,1 part_bytes=0 flag_bytes=1280"),
    ("64 1024 32 1 2048 32 1 0 0 0", "stage=none family=pipe kv_type=1 hs=64 nw=4 mode=0 map=0 nsplit=1 chunks_per_split=64 pack=0 merge=none grid=256,1,1 block=256 lds=40976 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("64 512 32 1 512 32 1 1 0 0", "stage=none family=pipe kv_type=1 hs=64 nw=2 mode=1 map=1 nsplit=1 chunks_per_split=16 pack=0 merge=none grid=256,1,1 block=128 lds=57360 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("64 512 32 1 512 32 1 0 30 0", "stage=none family=pipe kv_type=1 hs=64 nw=2 mode=2 map=0 nsplit=1 chunks_per_split=16 pack=0 merge=none grid=256,1,1 block=128 lds=40976 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("128 1024 16 2 2048 16 1 1 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=4 mode=1 map=1 nsplit=1 chunks_per_split=64 pack=0 merge=none grid=256,1,1 block=256 lds=106512 mgrid=1,1,1 fgrid=32,8,1 part_bytes=0 flag_bytes=512"),
    # below one work-group per CU: the smallest tile with the keys split in two (512 x 4096 x 32 heads; its head size 64 twin)
    ("128 512 32 1 4096 32 1 1 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=4 mode=1 map=1 nsplit=2 chunks_per_split=32 pack=0 merge=pipe grid=256,1,1 block=256 lds=106512 mgrid=16,32,1 fgrid=64,4,1 part_bytes=17301760 flag_bytes=512"),
    ("64 256 32 1 4096 32 1 0 0 0", "stage=none family=pipe kv_type=1 hs=64 nw=2 mode=0 map=0 nsplit=2 chunks_per_split=32 pack=0 merge=pipe grid=256,1,1 block=128 lds=40976 mgrid=8,32,1 fgrid=1,1,1 part_bytes=4456704 flag_bytes=0"),
    # KV <= 1024 at head size 128: half a chip of 128-row tiles still takes the pipelined kernel; a quarter does not
    ("128 512 32 1 1024 32 1 1 0 0", "stage=none family=pipe kv_type=1 hs=128 nw=4 mode=1 map=1 nsplit=1 chunks_per_split=32 pack=0 merge=none grid=128,1,1 block=256 lds=106512 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("128 512 16 1 1024 16 1 1 0 0", "stage=none family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=1 chunks_per_split=32 pack=1 merge=none grid=16,16,1 block=256 lds=0 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    # head size 256: prefill that fills the chip on the 128-row kernel, smaller prefill on the key-split kernel
    ("256 1024 32 1 1024 32 1 1 0 0", "stage=none family=wide kv_type=1 hs=256 nw=0 mode=0 map=0 nsplit=1 chunks_per_split=32 pack=0 merge=none grid=8,32,1 block=256 lds=0 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("256 512 8 1 1024 8 1 1 0 0", "stage=none family=split kv_type=1 hs=256 nw=0 mode=0 map=0 nsplit=2 chunks_per_split=16 pack=1 merge=tiles grid=32,8,1 block=256 lds=0 mgrid=16,8,1 fgrid=1,1,1 part_bytes=8519936 flag_bytes=0"),
    ("64 33 1 1 4096 1 1 1 0 0", "stage=none family=split kv_type=1 hs=64 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=16 pack=1 merge=tiles grid=16,1,1 block=256 lds=0 mgrid=2,1,1 fgrid=1,1,1 part_bytes=139520 flag_bytes=0"),
    # one-row decode, without and with grouped-query packing; the row merge up to 4 rows, the tile merge from 5
    ("128 1 32 1 4096 32 1 1 0 0", "stage=none family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=16 pack=1 merge=rows grid=8,32,1 block=256 lds=0 mgrid=1,32,1 fgrid=1,1,1 part_bytes=4325632 flag_bytes=0"),
    ("128 1 32 1 4096 4 1 1 0 0", "stage=none family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=16 pack=8 merge=rows grid=8,4,1 block=256 lds=0 mgrid=1,32,1 fgrid=1,1,1 part_bytes=4325632 flag_bytes=0"),
    ("128 4 32 1 32768 32 1 1 0 0", "stage=none family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=128 pack=1 merge=rows grid=8,32,1 block=256 lds=0 mgrid=4,32,1 fgrid=1,1,1 part_bytes=4325632 flag_bytes=0"),
    ("128 5 32 1 32768 32 1 1 0 0", "stage=none family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=128 pack=1 merge=tiles grid=8,32,1 block=256 lds=0 mgrid=1,32,1 fgrid=1,1,1 part_bytes=4325632 flag_bytes=0"),
    # a Q8_0 cache: raw under the key-split kernel at 64 query rows, copied to fp16 at 128; Q4_0 (two work-groups per CU) and BF16 decode raw; Q4_1 has no raw form
    ("128 64 8 1 4096 8 8 1 0 0", "stage=none family=split kv_type=8 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=16 pack=1 merge=tiles grid=16,8,1 block=256 lds=0 mgrid=2,8,1 fgrid=1,1,1 part_bytes=2162944 flag_bytes=0"),
    ("128 128 8 1 4096 8 8 1 0 0", "stage=copy family=pipe kv_type=1 hs=128 nw=4 mode=1 map=1 nsplit=2 chunks_per_split=32 pack=0 merge=pipe grid=16,1,1 block=256 lds=106512 mgrid=4,8,1 fgrid=1,1,1 part_bytes=1081600 flag_bytes=0"),
    ("128 1 32 1 4096 8 2 1 0 0", "stage=none family=split kv_type=2 hs=128 nw=0 mode=0 map=0 nsplit=8 chunks_per_split=16 pack=4 merge=rows grid=8,8,1 block=256 lds=0 mgrid=1,32,1 fgrid=1,1,1 part_bytes=4325632 flag_bytes=0"),
    ("64 1 8 1 8192 8 30 0 0 0", "stage=none family=split kv_type=30 hs=64 nw=0 mode=0 map=0 nsplit=16 chunks_per_split=16 pack=1 merge=rows grid=16,8,1 block=256 lds=0 mgrid=1,8,1 fgrid=1,1,1 part_bytes=1114368 flag_bytes=0"),
    ("64 1 8 1 1024 8 3 1 0 8", "stage=copy family=split kv_type=1 hs=64 nw=0 mode=0 map=0 nsplit=2 chunks_per_split=16 pack=1 merge=rows grid=2,8,1 block=256 lds=0 mgrid=1,8,1 fgrid=1,1,1 part_bytes=139520 flag_bytes=0"),
    # padded head sizes (80, and 96 with a Q8_0 cache): the head size 128 kernels on zero-padded copies
    ("80 64 8 1 512 8 1 1 0 0", "stage=pad family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=1 chunks_per_split=16 pack=1 merge=none grid=2,8,1 block=256 lds=0 mgrid=1,1,1 fgrid=1,1,1 part_bytes=0 flag_bytes=0"),
    ("96 1 8 1 1024 8 8 1 0 0", "stage=pad family=split kv_type=1 hs=128 nw=0 mode=0 map=0 nsplit=2 chunks_per_split=16 pack=1 merge=rows grid=2,8,1 block=256 lds=0 mgrid=1,8,1 fgrid=1,1,1 part_bytes=270592 flag_bytes=0"),
]


def test_flash_attn_launch_plans_of_a_table_of_shapes():
    """every routing rule of FLASH_ATTN_EXT at a shape that takes it, with the whole plan the call must get (see FATTN_PLAN_TABLE): staging, kernel family and form, key split,
    packing, merge kernel, grids, block, dynamic LDS, scratch bytes.  One process, plans only."""
    plans = _emul_module("fattn_emul_check").plan([tuple(s.split()) for s, _ in FATTN_PLAN_TABLE])
    for (shape, want), p in zip(FATTN_PLAN_TABLE, plans):
        assert re.sub(r" chunk=\d+", "", p["line"]) == want, shape
        assert p["chunk"] == (64 if p["family"] == "pipe" else 32), shape        # keys per chunk of chunks_per_split: the kernels' own constants


@pytest.mark.parametrize("cus,env", [(256, {}), (8, {}), (256, {"CDNA4_FA_PIPE": "2", "CDNA4_FA_PIPE_SPLIT": "3"}), (256, {"CDNA4_FA_PIPE": "4", "CDNA4_FA_PIPE_SPLIT": "3", "CDNA4_FA_SKIP_MIN": "0"})])
def test_flash_attn_launch_plan_properties(cus, env):
    """what holds for the plan of ANY call, over a grid of some thousand shapes (and under the forced-tile / forced-split knobs, where CDNA4_FA_PIPE=2 names a tile height head
    size 128 does not have): which kernel may read which K / V, a key split that covers the keys exactly, scratch and merge exactly with a split, LDS and grid limits"""
    shapes = [(D, nq, h, 1, kv, hk, t, m, sc, 0) for D in (64, 80, 128, 256) for nq in (1, 4, 5, 32, 33, 127, 128, 512, 4096) for kv in (96, 1024, 4096, 32768)
              for h, hk in ((1, 1), (8, 1), (32, 32)) for t in (1, 30, 8, 2, 3) for m, sc in ((0, 0), (1, 0), (2, 0), (1, 30)) if D % 32 == 0 or t in (1, 30)]
    shapes += [(128, nq, 1, 1, 1 << 20, 1, t, 1, 0, 0) for nq in (1, 4, 5) for t in (1, 2)]      # (a million keys under one head: more than 512 splits on a chip of 2048 CUs, below)
    assert len(shapes) > 5000
    plans = _emul_module("fattn_emul_check").plan(shapes, cus=cus, env=env) + _emul_module("fattn_emul_check").plan(shapes[-6:], cus=2048, env=env)
    seen = set()
    for s, p in zip(shapes + shapes[-6:], plans):
        D, nq, kv, t = s[0], s[1], s[4], s[6]
        why = (s, p["line"])
        seen.add((p["family"], p["stage"], p["merge"], p["nw"], p["nsplit"] > 512))
        assert (p["stage"] == "pad") == (D == 80) and p["hs"] == (128 if D == 80 else D), why
        if p["family"] == "pipe":
            assert p["kv_type"] == 1 and p["hs"] in (64, 128) and nq > 32 and p["nw"] in ((2, 4, 8) if p["hs"] == 64 else (4, 8)) and p["block"] == 64 * p["nw"], why
        assert p["kv_type"] in (1, t), why
        if p["kv_type"] != 1:                                            # a raw BF16 / Q8_0 / Q4_0 cache: the key-split kernel alone reads it, and only below 128 query rows
            assert p["family"] == "split" and nq < 128 and p["stage"] == "none" and t in (30, 8, 2), why
        assert (p["stage"] == "copy") == (D != 80 and t != 1 and p["kv_type"] == 1), why
        nchunk = -(-kv // p["chunk"])
        assert p["nsplit"] >= 1 and (p["nsplit"] - 1) * p["chunks_per_split"] < nchunk <= p["nsplit"] * p["chunks_per_split"], why
        if p["family"] == "wide":
            assert p["nsplit"] == 1 and p["kv_type"] == 1, why
        assert (p["part_bytes"] > 0) == (p["nsplit"] > 1) == (p["merge"] != "none"), why
        assert (p["merge"] == "pipe") == (p["family"] == "pipe" and p["nsplit"] > 1), why
        assert (p["merge"] == "rows") == (p["nsplit"] > 1 and nq <= 4 and p["nsplit"] <= 512), why
        assert 0 <= p["lds"] <= 160 * 1024 and (p["lds"] > 0) == (p["family"] == "pipe"), why
        for g in (p["grid"], p["mgrid"], p["fgrid"]):
            assert 0 < g[0] < 2 ** 31 and 0 < g[1] <= 65535 and 0 < g[2] <= 65535, why
    if not env:                                                          # the grid reaches what the properties speak of
        assert {f for f, *_ in seen} == {"pipe", "wide", "split"} and {m for _, _, m, *_ in seen} == {"none", "tiles", "rows", "pipe"} and {st for _, st, *_ in seen} == {"none", "copy", "pad"}, seen
        assert any(big for *_, big in seen), seen
    if env.get("CDNA4_FA_PIPE") == "2":                                  # head size 128 has no 2-wave form: those calls take the older kernels, unsplit where that is a 128-row kernel
        assert ("wide", "none", "none", 0, False) in seen and not any(f == "pipe" and nw != 2 for f, _, _, nw, _ in seen), seen


# calls FLASH_ATTN_EXT must refuse: (D_q, D_k, D_v, D_dst, n_q, n_head, n_kv, n_head_kv, kv_type, mask, max_bias, k_offset) and the message — those of the launcher before it had a plan
FATTN_REJECTED = [
    ((128, 128, 128, -1, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: q, k, v and dst are required"),
    ((0, 0, 0, 0, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: head size must be 1..256"),
    ((300, 300, 300, 300, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: head size must be 1..256"),
    ((128, 128, 128, 128, 64, 8, 0, 8, 1, 1, 0, 0), "flash_attn_ext: no keys"),
    ((128, 128, 128, 128, 64, 8, 512, 8, 1, 3, 0, 0), "flash_attn_ext: mask must be F16 [n_kv, >= n_q]"),
    ((128, 128, 128, 128, 64, 8, 512, 8, 1, 0, 8, 0), "flash_attn_ext: ALiBi needs a mask"),
    ((128, 128, 128, 128, 1, 65536, 512, 65536, 1, 1, 0, 0), "flash_attn_ext: too many heads / batches for one grid"),
    ((128, 128, 128, 128, 64, 8, 512, 8, 1, 1, 0, 2), "flash_attn_ext: k / v rows and dst must be 16-byte aligned"),
    ((128, 128, 128, 128, 64, 8, 512, 3, 1, 1, 0, 0), "flash_attn_ext: heads / batch not broadcastable over k / v"),
    ((128, 128, 128, 128, 64, 8, 512, 8, 12, 1, 0, 0), "flash_attn_ext: k / v must be F16, BF16 or Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0"),
    # q's head size against that of k, v and dst, on every staging: nothing staged (F16, raw Q8_0), fp16 copy (Q4_1), padded
    ((64, 128, 128, 128, 1, 8, 64, 8, 1, 1, 0, 0), "flash_attn_ext: k / v shape mismatch"),
    ((64, 128, 128, 128, 1, 8, 64, 8, 8, 1, 0, 0), "flash_attn_ext: k / v shape mismatch"),
    ((64, 100, 100, 100, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: k / v shape mismatch"),
    ((128, 64, 128, 128, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: k / v shape mismatch"),
    ((128, 128, 64, 128, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: k / v shape mismatch"),
    ((128, 128, 128, 64, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: dst must be [head_size, n_head, n_q, batch]"),
    ((64, 128, 128, 128, 1, 8, 64, 8, 3, 1, 0, 0), "flash_attn_ext: bad k / v shape"),
    ((80, 128, 80, 80, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: bad k / v shape"),
    ((80, 80, 80, 128, 64, 8, 512, 8, 1, 1, 0, 0), "flash_attn_ext: dst must be [head_size, n_head, n_q, batch]"),
]


def test_flash_attn_refuses_invalid_calls_before_any_launch():
    """ggml_cdna4_op_flash_attn_ext itself (the checks in front of the plan's execution) on operands without memory behind them: every call of FATTN_REJECTED
    returns -1 with its message, and none reaches a kernel (which would end the harness with a fault)"""
    got = _emul_module("fattn_emul_check").reject([c for c, _ in FATTN_REJECTED])
    assert got == [(-1, m) for _, m in FATTN_REJECTED], [(c, g, m) for (c, m), g in zip(FATTN_REJECTED, got) if g != (-1, m)]


# Prefill GEMM routing plans (gemm_q_plan.hpp's gemm_q_make_plan through `lib_emul plan`).  Call: "type M K B splitk variant w_offset xf image" (type: the ggml type id; w_offset: of
# the weights from a 4096-byte boundary; xf: the fp32 rows are handed over; image: a resident image is registered), under a CU count and routing knobs.  The expected values are what the
# launcher did BEFORE it had a plan: recorded from the launches of the probe-era library (kernel instantiation, grid, gemm_params, where W points, the zero-fill / conversion / re-layout
# launches in front, k_epilogue behind) with the launch calls replaced by prints — not taken from gemm_q_make_plan.  (tail of a call with an explicit split or variant, which the
# fused entry point cannot name: the kernels' own rule — k_gemm_q and the atomic-sum split store the plain product.)
GEMM_PLAN_TABLE = [
    (256, {}, "12 4096 4096 1024 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=1 ntiles=256 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 256 512 64 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=288 kmul=1 term=t64 tm=128 splitk=2 ntiles=2 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 2048 128 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=1152 kmul=1 term=t64 tm=128 splitk=4 ntiles=32 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 128 4096 16 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=8 ntiles=1 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 16384 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=256 splitk=1 ntiles=256 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1", "CDNA4_T64_HANDOFF": "1"}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=11 reenc=0 tail=1 fq=1 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=0 waits=1 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1"}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=11 reenc=0 tail=1 fq=1 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=0 waits=1 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 2 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 0 24576 0 1 0", "ok=1 kernel=14 route=14 reenc=0 tail=0 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=kq tm=128 splitk=1 ntiles=128 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 512 4096 0 0 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=288 kmul=1 term=r8 tm=256 splitk=1 ntiles=256 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "13 4096 512 4096 0 0 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=352 kmul=1 term=r8 tm=256 splitk=1 ntiles=256 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "8 4096 1024 2816 0 0 0 1 1", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=resident wtype=108 wrow=1088 kmul=1 term=r8 tm=256 splitk=1 ntiles=176 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1"}, "14 4096 1024 2048 0 0 0 1 1", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=resident wtype=115 wrow=1152 kmul=1 term=r8 tm=256 splitk=2 ntiles=128 ticketed=0 waits=1 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1"}, "8 4096 8192 512 0 0 0 1 1", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=resident wtype=108 wrow=8704 kmul=1 term=r8 tm=256 splitk=8 ntiles=32 ticketed=0 waits=1 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "2 4096 4096 512 0 0 0 1 1", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=resident wtype=102 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "2 4096 512 4096 0 0 0 1 1", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=resident wtype=102 wrow=288 kmul=1 term=r8 tm=256 splitk=1 ntiles=256 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 0 335544320 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=r8 tm=256 splitk=1 ntiles=32 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "8 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=208 wrow=4352 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=65 sb_split=8 xchg_l2=1"),
    (256, {}, "8 256 768 64 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=208 wrow=816 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=65 sb_split=0 xchg_l2=0"),
    (256, {}, "14 4096 11008 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=214 wrow=9030 kmul=1 term=w8 tm=128 splitk=1 ntiles=128 ticketed=0 waits=0 zero=0 opt=65 sb_split=0 xchg_l2=0"),
    (256, {}, "8 256 256 64 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=relaid wtype=108 wrow=272 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=20 sb_split=0 xchg_l2=0"),
    (256, {}, "14 256 512 64 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=relaid wtype=114 wrow=448 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=20 sb_split=0 xchg_l2=0"),
    (256, {}, "2 256 512 64 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=relaid wtype=102 wrow=288 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=20 sb_split=0 xchg_l2=0"),
    (256, {}, "8 4096 1024 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=relaid wtype=108 wrow=1088 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=20 sb_split=2 xchg_l2=1"),
    (256, {}, "13 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=2816 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=64 sb_split=8 xchg_l2=1"),
    (256, {}, "13 256 1024 64 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=704 kmul=1 term=w8 tm=128 splitk=2 ntiles=2 ticketed=1 waits=0 zero=0 opt=20 sb_split=2 xchg_l2=0"),
    (256, {}, "13 4096 11008 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=7568 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=64 sb_split=22 xchg_l2=1"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1"}, "13 4096 4096 512 2 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=2816 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=0 waits=1 zero=0 opt=64 sb_split=8 xchg_l2=1"),
    (256, {}, "12 4096 4096 512 0 4119 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=65 sb_split=8 xchg_l2=1"),
    (256, {}, "12 4096 4096 512 4 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=0 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=w8 tm=128 splitk=4 ntiles=128 ticketed=0 waits=0 zero=1 opt=65 sb_split=0 xchg_l2=0"),
    (256, {}, "13 256 1024 64 4 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=0 fq=0 src=given wtype=13 wrow=704 kmul=1 term=w8 tm=128 splitk=4 ntiles=2 ticketed=0 waits=0 zero=1 opt=20 sb_split=0 xchg_l2=0"),
    (256, {}, "13 4096 4096 512 0 663 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=2816 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=20 sb_split=8 xchg_l2=1"),
    (256, {}, "8 4096 4032 512 0 0 0 1 0", "ok=1 kernel=14 route=14 reenc=0 tail=0 fq=0 src=given wtype=8 wrow=4284 kmul=1 term=kq tm=128 splitk=1 ntiles=128 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "8 256 320 64 0 0 0 1 0", "ok=1 kernel=14 route=14 reenc=0 tail=0 fq=0 src=given wtype=8 wrow=340 kmul=1 term=kq tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "8 4096 4032 512 3 0 0 1 0", "ok=1 kernel=14 route=14 reenc=0 tail=0 fq=0 src=given wtype=8 wrow=4284 kmul=1 term=kq tm=128 splitk=3 ntiles=128 ticketed=0 waits=0 zero=1 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "6 256 768 64 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=reencoded wtype=208 wrow=816 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=65 sb_split=0 xchg_l2=0"),
    (256, {}, "20 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=reencoded wtype=208 wrow=4352 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=65 sb_split=8 xchg_l2=1"),
    (256, {}, "11 256 768 64 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=reencoded wtype=214 wrow=630 kmul=1 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=65 sb_split=0 xchg_l2=0"),
    (256, {}, "3 256 256 64 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=relaid wtype=108 wrow=544 kmul=2 term=w8 tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=20 sb_split=0 xchg_l2=0"),
    (256, {}, "7 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=reencoded wtype=208 wrow=8704 kmul=2 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=65 sb_split=16 xchg_l2=1"),
    (256, {}, "10 256 768 64 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=reencoded wtype=214 wrow=1260 kmul=2 term=w8 tm=128 splitk=2 ntiles=2 ticketed=1 waits=0 zero=0 opt=65 sb_split=3 xchg_l2=0"),
    (256, {}, "23 256 512 64 0 0 0 1 0", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=relaid wtype=114 wrow=896 kmul=2 term=w8 tm=128 splitk=2 ntiles=2 ticketed=1 waits=0 zero=0 opt=20 sb_split=2 xchg_l2=0"),
    (256, {}, "6 4096 4096 512 0 0 0 1 1", "ok=1 kernel=13 route=113 reenc=1 tail=1 fq=0 src=resident wtype=208 wrow=4352 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=65 sb_split=8 xchg_l2=1"),
    (256, {}, "6 256 320 64 0 0 0 1 0", "ok=1 kernel=14 route=114 reenc=1 tail=0 fq=0 src=reencoded wtype=8 wrow=340 kmul=1 term=kq tm=128 splitk=1 ntiles=2 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (8, {}, "12 256 512 64 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=288 kmul=1 term=t64 tm=128 splitk=2 ntiles=2 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (8, {}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=r8 tm=256 splitk=1 ntiles=32 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (8, {}, "12 4096 1024 100 0 0 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=576 kmul=1 term=r8 tm=256 splitk=1 ntiles=16 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (8, {}, "8 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=208 wrow=4352 kmul=1 term=w8 tm=128 splitk=1 ntiles=128 ticketed=0 waits=0 zero=0 opt=65 sb_split=0 xchg_l2=0"),
    (8, {}, "13 4096 4096 512 0 0 0 1 0", "ok=1 kernel=12 route=12 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=2816 kmul=1 term=r8 tm=256 splitk=1 ntiles=32 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (8, {"GGML_CDNA4_OWNED_DEVICE": "1"}, "8 256 4096 256 0 0 0 1 1", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=208 wrow=4352 kmul=1 term=w8 tm=128 splitk=2 ntiles=4 ticketed=1 waits=0 zero=0 opt=65 sb_split=8 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 0 24577 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {}, "12 4096 4096 512 0 40961 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=256 splitk=1 ntiles=64 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"CDNA4_NO_R8": "1"}, "12 4096 512 4096 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=288 kmul=1 term=t64 tm=256 splitk=1 ntiles=512 ticketed=0 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1", "CDNA4_NO_FUSEQ": "1"}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=10 reenc=0 tail=1 fq=0 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=0 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"GGML_CDNA4_OWNED_DEVICE": "1", "CDNA4_FQ_TICKETED": "1"}, "12 4096 4096 512 0 0 0 1 0", "ok=1 kernel=10 route=11 reenc=0 tail=1 fq=1 src=given wtype=12 wrow=2304 kmul=1 term=t64 tm=128 splitk=2 ntiles=128 ticketed=1 waits=1 zero=0 opt=0 sb_split=0 xchg_l2=0"),
    (256, {"CDNA4_W8_HANDOFF": "1", "GGML_CDNA4_OWNED_DEVICE": "1"}, "13 4096 4096 512 0 0 0 1 0", "ok=1 kernel=13 route=13 reenc=0 tail=1 fq=0 src=given wtype=13 wrow=2816 kmul=1 term=w8 tm=128 splitk=2 ntiles=128 ticketed=0 waits=1 zero=0 opt=64 sb_split=8 xchg_l2=1"),
]


def _gemm_plans_by_setting(rows):
    """rows (cus, env, call, ..) -> their plans, one `lib_emul plan` process per (cus, env)"""
    mod, out, groups = _emul_module("lib_emul_check"), {}, {}
    for i, r in enumerate(rows):
        groups.setdefault((r[0], tuple(sorted(r[1].items()))), []).append(i)
    for (cus, env), idx in groups.items():
        for i, p in zip(idx, mod.plan([rows[i][2].split() for i in idx], cus=cus, env=dict(env))):
            out[i] = p
    return [out[i] for i in range(len(rows))]


def test_prefill_gemm_routing_plans_of_a_table_of_shapes():
    """every routing rule of the prefill GEMM at a shape that takes it, with the plan the call must get (see GEMM_PLAN_TABLE): kernel and route id, re-encoding, tail and quantizer
    in the launch, where the weights come from and in which format, the terminal's tiles, split, exchange and schedule.  And the call on the same arguments executes it (rc 0)."""
    for (cus, env, call, want), p in zip(GEMM_PLAN_TABLE, _gemm_plans_by_setting(GEMM_PLAN_TABLE)):
        assert p["line"] == want and p["pure"] == 1 and p["rc"] == 0, (cus, env, call, p["line"], p["msg"])


@pytest.mark.parametrize("cus,env", [(256, {}), (256, {"GGML_CDNA4_OWNED_DEVICE": "1"}), (8, {}), (8, {"GGML_CDNA4_OWNED_DEVICE": "1"})])
def test_prefill_gemm_routing_plan_properties(cus, env):
    """what holds for the plan of ANY call, over some ten thousand (type, M, K, B, splitk, variant, alignment, image) cells in the shared and the owned mode: the plan refuses exactly
    the calls cdna4_launch_gemm_q refuses, with its message; the tail is outside the store exactly on k_gemm_q and on the atomic-sum split of the 128 x 128-tile kernels; the quantizer
    rides only in k_gemm_kq_t64 on Q4_K's 128-row tiles of a device the caller owns; AUTO never waits for a co-resident work-group on a shared device; planning is repeatable
    and leaves the error text alone"""
    r8 = (1 << 28) | (1 << 26)
    knobs = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (8, 0), (0, 8193), (0, 24577), (0, 40961), (2, 8193), (0, 1 << 28), (0, r8), (2, r8), (0, 23 | 2048), (0, 23 | 4096), (0, 23 | (20 << 5)),
             (0, 23), (0, 4), (4, 23 | 2048), (0, 8192)]
    cells = [(t, m, k, b, sk, v, off, 1, img) for _, t in LIB_TYPES for m in (130, 256, 4096) for k in (256, 768, 1024, 4032, 4096, 11008) for b in (9, 65, 128, 512, 2048)
             for sk, v in knobs for off, img in ((0, 0), (2, 0), (0, 1)) if (off == 0 and img == 0) or (sk, v) == (0, 0)]
    cells += [(12, 0, 256, 64, 0, 0, 0, 1, 0), (12, 256, 256, 0, 0, 0, 0, 1, 0), (12, 32768, 8192, 512, 0, 0, 0, 1, 0), (8, 16384, 8192, 512, 0, 0, 0, 1, 1), (8, 8192, 8192, 512, 0, 0, 0, 1, 1)]
    assert len(cells) > 20000
    owned = bool(env)
    seen = set()
    for c, p in zip(cells, _emul_module("lib_emul_check").plan(cells, cus=cus, env=env)):
        why = (c, p["line"], p["rc"], p["msg"])
        assert p["pure"] == 1, why
        assert (p["ok"] == 1) == (p["rc"] == 0), why
        if not p["ok"]:
            assert p["rc"] == -1 and p["plan_err"] == 1 and (p["kernel"], p["route"], p["tail"], p["fq"]) == (0, 0, 0, 0), why
            continue
        if p["term"] == "none":
            assert c[1] <= 0 or c[3] <= 0, why
            continue
        seen.add((p["term"], p["src"], p["fq"], p["waits"], p["reenc"]))
        assert p["kernel"] == {"t64": 10, "r8": 12, "w8": 13, "kq": 14}[p["term"]] and p["route"] == (11 if p["fq"] else p["kernel"] + 100 * p["reenc"]), why
        assert (p["tail"] == 0) == (p["kernel"] == 14 or (p["kernel"] == 13 and p["zero"] == 1)), why
        if p["fq"]:
            assert owned and p["kernel"] == 10 and p["wtype"] == 12 and c[0] == 12 and p["tm"] == 128 and p["waits"] == 1, why
        if not owned:                                                    # AUTO, and explicit splits too: a shared device gives them a form that does not wait, or refuses them
            assert p["waits"] == 0, why
    terms, srcs = {s[0] for s in seen}, {s[1] for s in seen}
    assert terms == {"t64", "r8", "w8", "kq"} and srcs == {"given", "resident", "reencoded", "relaid"}, seen
    assert any(s[2] for s in seen) == owned and any(s[3] for s in seen) == owned, seen      # (the grid reaches the one-launch step and the waiting splits where they may exist)


# MUL_MAT_ID routing plans (mul_mat_id_plan.hpp's mmid_make_plan through `lib_emul plan_id`).  Call: "type M K n_expert n_used n_b n_tok as_offset b_offset ws_offset ws_bytes image
# prepared [dst_gap b_gap]" (type: the ggml type id; the offsets: of the expert stack, b and the workspace from aligned bases; ws_bytes 0: the public workspace size; image: a resident
# image of the stack is registered; prepared: the `prepared` twin is called; the gaps: elements between the tokens of dst / b), under a CU count and routing knobs.  The expected
# values are what the calls did BEFORE they had a plan: recorded from the launches of the library in which mul_mat_id_impl, the front key and the grouped launchers each decided for
# themselves, with the launch calls replaced by prints (kernel instantiation, grid, the parameter structs: where W points, row and expert strides, image rows, the work queue's spans,
# units, capacity and cost weights, tile rows, tile tables, split, weights through LDS), from that library's return codes, messages and public front key, and `need` as the smallest
# workspace at which that library's launches are those of the full-size call — not taken from mmid_make_plan.  (A refusal or an empty call names nothing but its return code.)
MMID_PLAN_TABLE = [
    (256, {}, "12 130 256 4 2 1 16 0 0 0 0 0 0", "kind=gemv rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=45824 rows=16 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=256 upt=2 cap=5 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {}, "12 4096 4096 8 2 1 512 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=4249344 rows=512 G=256 upt=512 cap=17 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (8, {}, "12 4096 4096 8 2 1 512 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=4249344 rows=512 G=8 upt=512 cap=17 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {}, "12 130 256 1024 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=82432 rows=17 G=256 upt=2 cap=35 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {}, "12 130 256 1025 2 1 17 0 0 0 0 0 0", "kind=gemv rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=46848 rows=17 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 130 256 4 2 1 17 2 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=12 w=as+2 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 130 256 8 2 1 131072 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=136904960 rows=263168 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {}, "14 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=14 w=as+0 wrow=210 wexp=27300 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "8 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=8 w=as+0 wrow=272 wexp=35360 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "14 130 256 1 1 1 33 0 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=14 w=as+0 wrow=210 wexp=27300 need=166144 rows=256 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "14 130 256 2 1 1 33 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=14 w=as+0 wrow=210 wexp=27300 need=232704 rows=384 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "13 130 256 1 1 1 33 0 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=13 w=as+0 wrow=176 wexp=22880 need=166144 rows=256 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=1 key=0", 0, ""),
    (256, {}, "13 130 256 1 1 1 33 2 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=13 w=as+2 wrow=176 wexp=22880 need=166144 rows=256 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "13 130 256 4 2 1 17 2 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=13 w=as+2 wrow=176 wexp=22880 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "2 130 256 4 2 1 17 0 0 0 0 1 0", "kind=queue rc=0 wtype=102 w=img+0 wrow=144 wexp=18720 need=51200 rows=17 G=256 upt=2 cap=5 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154050", 0, ""),
    (256, {}, "2 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=2 w=as+0 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "2 130 256 1 1 1 33 0 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=2 w=as+0 wrow=144 wexp=18720 need=166144 rows=256 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "2 130 320 4 2 1 17 0 0 0 0 1 0", "kind=gemv rc=0 wtype=2 w=as+0 wrow=180 wexp=23400 need=52992 rows=17 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "2 130 256 1 1 1 33 0 0 0 0 1 0", "kind=tiles_t64 rc=0 wtype=102 w=img+0 wrow=144 wexp=18720 need=166144 rows=256 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=1 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "2 130 256 4 2 1 17 0 0 0 0 1 0", "kind=tiles_mmq rc=0 wtype=2 w=as+0 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 130 256 4 2 1 17 0 0 0 51199 0 0", "kind=gemv rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=46848 rows=17 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "14 130 256 1 1 1 33 0 0 0 166143 0 0", "kind=gemv rc=0 wtype=14 w=as+0 wrow=210 wexp=27300 need=59648 rows=33 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "14 130 256 1 1 1 33 0 0 0 1000 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: workspace too small"),
    (256, {}, "14 130 32768 8 1 1 32767 0 0 0 0 0 0", "kind=gemv rc=0 wtype=14 w=as+0 wrow=26880 wexp=3494400 need=3372150272 rows=32767 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 4096 4096 8 2 1 1 0 0 0 0 0 0", "kind=gemv_1 rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 4096 4096 8 2 1 1 0 4 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "quantize_q8_K: x must be 16-byte aligned"),
    (256, {}, "3 130 256 4 2 2 1 0 0 0 0 0 0", "kind=gemv_1 rc=0 wtype=3 w=as+0 wrow=160 wexp=20800 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "8 130 544 4 2 1 1 0 0 0 0 0 0", "kind=gemv rc=0 wtype=8 w=as+0 wrow=578 wexp=75140 need=35328 rows=1 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "12 4096 4096 8 2 1 512 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=16826624 rows=2048 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MOE_SK": "0"}, "12 4096 4096 8 2 1 512 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=16826624 rows=2048 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "12 512 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=294912 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=1 split=1 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MOE_SK": "0"}, "12 512 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=294912 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "12 4096 256 8 2 1 320 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=144 wexp=589824 need=898304 rows=1664 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=1 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_TM": "128"}, "12 4096 4096 8 2 1 512 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=2304 wexp=9437184 need=16826624 rows=2048 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=1 split=1 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_TM": "256"}, "12 130 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=74880 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=256 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_PLAN": "0"}, "12 130 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=74880 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=0 split=1 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_PLAN": "0"}, "12 130 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=74880 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=0 split=1 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_SPLITK": "2"}, "12 130 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=74880 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=1 split=1 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MOE_SK": "0", "CDNA4_MOE_SPLITK": "2"}, "12 130 1024 4 2 1 17 0 0 0 0 0 0", "kind=tiles_t64 rc=0 wtype=12 w=as+0 wrow=576 wexp=74880 need=1348864 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=128 tables=0 split=2 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MMQ_IDS": "2"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_MMQ_IDS": "2"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_mmq rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_MMQ_IDS": "2"}, "12 130 256 1 1 1 33 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=56320 rows=33 G=256 upt=2 cap=2 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {"CDNA4_NO_MMQ_IDS": "1"}, "14 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=14 w=as+0 wrow=210 wexp=27300 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (8, {"CDNA4_NO_MMQ_IDS": "1"}, "8 130 256 4 2 1 17 0 0 0 0 0 0", "kind=tiles_kq rc=0 wtype=8 w=as+0 wrow=272 wexp=35360 need=365824 rows=640 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {"CDNA4_SK_CW": "4,6,8,10"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=256 upt=2 cap=5 cw=4,6,8,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (8, {"CDNA4_SK_CW": "4,6,8,10"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=8 upt=2 cap=5 cw=4,6,8,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {"CDNA4_SK_SPANS": "40"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=40 upt=2 cap=5 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (8, {"CDNA4_SK_SPANS": "40"}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=40 upt=2 cap=5 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (8, {}, "12 130 256 4 2 1 17 0 0 0 0 0 0", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=8 upt=2 cap=5 cw=10,10,10,10 front=1 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {}, "12 130 256 4 2 1 17 0 0 0 0 0 1", "kind=queue rc=0 wtype=12 w=as+0 wrow=144 wexp=18720 need=51200 rows=17 G=256 upt=2 cap=5 cw=10,10,10,10 front=2 tm=0 tables=0 split=0 wlds=0 key=1297154049", 0, ""),
    (256, {}, "2 130 256 4 2 1 17 0 0 0 0 1 1", "kind=queue rc=0 wtype=102 w=img+0 wrow=144 wexp=18720 need=51200 rows=17 G=256 upt=2 cap=5 cw=10,10,10,10 front=2 tm=0 tables=0 split=0 wlds=0 key=1297154050", 0, ""),
    (256, {}, "14 130 256 4 2 1 17 0 0 0 0 0 1", "kind=refused rc=-2 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -2, "mul_mat_id_prepared: a call of this shape leaves no front (ggml_cdna4_mul_mat_id_front_key == 0)"),
    (256, {}, "12 130 256 4 2 1 17 0 4 0 0 0 1", "kind=refused rc=-2 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -2, "mul_mat_id_prepared: misaligned operands"),
    (256, {}, "12 130 256 4 2 1 17 0 0 128 0 0 1", "kind=refused rc=-2 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -2, "mul_mat_id_prepared: misaligned operands"),
    (256, {"CDNA4_MOE_SK": "0"}, "12 130 256 4 2 1 17 0 0 0 0 0 1", "kind=refused rc=-2 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -2, "mul_mat_id_prepared: a call of this shape leaves no front (ggml_cdna4_mul_mat_id_front_key == 0)"),
    (256, {}, "0 130 256 4 2 1 17 0 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: unsupported weight type"),
    (256, {}, "12 0 256 4 2 1 17 0 0 0 0 0 0", "kind=empty rc=0 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", 0, ""),
    (256, {}, "12 130 100 4 2 1 17 0 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: K is not a whole number of blocks"),
    (256, {}, "12 130 256 4 3 2 17 0 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: n_used must be a multiple of b.ne[1]"),
    (256, {}, "12 130 256 4 2 1 17 0 0 0 0 0 0 1 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: dst must be contiguous over (slot, token)"),
    (256, {}, "12 130 256 4 2 1 17 0 0 0 0 0 0 0 4", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: b must be contiguous over (row, token)"),
    (256, {}, "12 130 256 4 2 1 16 0 0 128 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: workspace must be 256-byte aligned"),
    (256, {}, "12 130 256 4 2 1 16 0 0 0 1000 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "mul_mat_id: workspace too small"),
    (256, {}, "12 130 256 4 2 1 16 0 4 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "quantize_q8_K: x must be 16-byte aligned"),
    (256, {}, "8 130 256 4 2 1 16 0 4 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "quantize_q8_0: x must be 16-byte aligned"),
    (256, {}, "3 130 256 4 2 1 16 0 4 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "quantize_q8_1: x must be 16-byte aligned"),
    (256, {}, "8 130 256 4 2 1 16 1 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "gemv_q: misaligned operands"),
    (256, {}, "14 130 4096 8 2 1 131072 0 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "gemv_q: too many MUL_MAT_ID columns"),
    (256, {}, "12 130 256 4 2 1 16 2 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "gemv_q: Q4_K/Q5_K rows must be 16-byte aligned"),
    (256, {}, "13 130 256 4 2 1 1 2 0 0 0 0 0", "kind=refused rc=-1 wtype=0 w=as+0 wrow=0 wexp=0 need=0 rows=0 G=0 upt=0 cap=0 cw=0,0,0,0 front=0 tm=0 tables=0 split=0 wlds=0 key=0", -1, "gemv_q: Q4_K/Q5_K rows must be 16-byte aligned"),
]


def _mmid_plans_by_setting(rows):
    """rows (cus, env, call, ..) -> their plans, one `lib_emul plan_id` process per (cus, env)"""
    mod, out, groups = _emul_module("lib_emul_check"), {}, {}
    for i, r in enumerate(rows):
        groups.setdefault((r[0], tuple(sorted(r[1].items()))), []).append(i)
    for (cus, env), idx in groups.items():
        for i, p in zip(idx, mod.plan_id([rows[i][2].split() for i in idx], cus=cus, env=dict(env))):
            out[i] = p
    return [out[i] for i in range(len(rows))]


def test_mul_mat_id_routing_plans_of_a_table_of_calls():
    """every routing rule of MUL_MAT_ID at a call that takes it, with the plan the call must get (see MMID_PLAN_TABLE): the kind, what the kernel reads, the workspace view's
    bytes, the work queue's geometry, the grouped k_gemm_kq_t64's tiles / tables / split, k_gemm_q's weights through LDS, the front key; every refusal with its return code and
    message.  And the call on the same arguments answers what the plan says."""
    for (cus, env, call, want, want_rc, want_msg), p in zip(MMID_PLAN_TABLE, _mmid_plans_by_setting(MMID_PLAN_TABLE)):
        assert p["line"] == want and p["pure"] == 1 and (p["call_rc"], p["msg"]) == (want_rc, want_msg), (cus, env, call, p["line"], p["call_rc"], p["msg"])


def _mmid_cells():
    """(type, M, K, n_expert, n_used, n_b, n_tok, as_offset, b_offset, ws_offset, ws_bytes, image, prepared): every accepted type x shapes on both sides of every threshold x
    operand alignments x workspace sizes x a registered stack image x the `prepared` twin"""
    cells = []
    for _, t in LIB_TYPES:
        for m in (130, 4096):
            for k in (256, 320, 4096):                                   # (320: whole blocks of the 32-weight formats only, and no whole 128-k panel)
                for ne, nu, nb in ((1, 1, 1), (4, 2, 1), (8, 2, 2), (1025, 2, 1), (4, 3, 2)):
                    for nt in (1, 16, 17, 33, 129, 512):
                        for ao, bo, wo, ws, img in ((0, 0, 0, 0, 0), (2, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 4, 0, 0, 0), (0, 0, 128, 0, 0), (0, 0, 0, 65536, 0), (0, 0, 0, 1 << 20, 0),
                                                    (0, 0, 0, 0, 1), (2, 0, 0, 0, 1)):
                            if img and t not in (2, 8, 12):
                                continue
                            for prep in (0, 1):
                                if prep and (nt < 17 or ws == 65536 or ao == 1):
                                    continue
                                cells.append((t, m, k, ne, nu, nb, nt, ao, bo, wo, ws, img, prep))
    # an empty call; more tile records than the planner holds (the per-tile launches); an expert-sorted image that 32-bit byte offsets do not reach (GEMV, too many columns)
    cells += [(12, 0, 256, 4, 2, 1, 17, 0, 0, 0, 0, 0, 0), (12, 130, 256, 4, 2, 1, 0, 0, 0, 0, 0, 0, 0), (12, 130, 256, 8, 2, 1, 131072, 0, 0, 0, 0, 0, 0), (12, 130, 256, 8, 2, 1, 131072, 0, 0, 0, 0, 0, 1),
              (12, 130, 4096, 8, 2, 1, 131072, 0, 0, 0, 0, 0, 0), (14, 130, 4096, 8, 2, 1, 131072, 0, 0, 0, 0, 0, 0), (2, 130, 256, 8, 2, 1, 131072, 0, 0, 0, 0, 1, 0)]
    return cells


MMID_SETTINGS = [(256, {}), (8, {}), (256, {"CDNA4_MOE_SK": "0"}), (8, {"CDNA4_MOE_SK": "0"}), (256, {"CDNA4_MMQ_IDS": "2"}), (8, {"CDNA4_MMQ_IDS": "2"})]


@pytest.mark.parametrize("cus,env", MMID_SETTINGS)
def test_mul_mat_id_routing_plan_properties(cus, env):
    """what holds for the plan of ANY MUL_MAT_ID call, over more than twenty thousand cells (_mmid_cells) under the default routing, without the work-queue form and with the int8
    matrix cores forced: planning is repeatable and leaves the error text alone; the plan refuses exactly the calls the call refuses, with the same return code and message;
    the public front key is non-zero exactly on the work-queue kind and is the plan's; an aligned `prepared` call succeeds exactly where the key is non-zero; the kernels read a
    Q4_0R image exactly when one is registered for a Q4_0 stack of whole superblocks (on the fp16 grouped kinds: the integer-dot kinds read the caller's Q4_0 blocks), and the
    caller's stack otherwise; the bytes a plan made with the public workspace size needs never exceed that size; every kind occurs."""
    cells = _mmid_cells()
    assert len(cells) > 20000
    kinds = set()
    checked = 0
    for c, p in zip(cells, _emul_module("lib_emul_check").plan_id(cells, cus=cus, env=env)):
        t, m, k, ne, nu, nb, nt, ao, bo, wo, ws, img, prep = c
        why = (c, p["line"], p["call_rc"], p["msg"])
        assert p["pure"] == 1, why
        assert (p["kind"] == "refused") == (p["call_rc"] != 0) and p["rc"] == p["call_rc"], why
        if p["kind"] == "refused":
            assert p["rc"] in (-1, -2) and p["plan_err"] == 1 and p["key"] == 0, why
        aligned = not (bo or wo)                                         # (the key is asked with aligned stand-ins for b and the workspace)
        assert p["key"] == (p["pubkey"] if p["kind"] == "queue" else 0) and (aligned or p["kind"] != "queue"), why
        if aligned:
            assert (p["pubkey"] != 0) == (p["kind"] == "queue"), why
        if prep:
            assert p["kind"] in ("queue", "refused") and p["rc"] == (0 if p["kind"] == "queue" else -2) and p["front"] == (2 if p["kind"] == "queue" else 0), why
            assert p["msg"] == ("" if p["kind"] == "queue" else "mul_mat_id_prepared: misaligned operands" if p["pubkey"] else
                                "mul_mat_id_prepared: a call of this shape leaves no front (ggml_cdna4_mul_mat_id_front_key == 0)"), why
        else:
            assert p["front"] == (1 if p["kind"] == "queue" else 0) and p["rc"] in (0, -1), why
        image = bool(img) and t == 2 and k % 256 == 0
        if p["kind"] in ("queue", "tiles_t64", "tiles_kq"):
            assert (p["wtype"], p["w"], p["wrow"], p["wexp"]) == ((102, "img+0", k // 256 * 144, m * (k // 256 * 144)) if image else (t, "as+%d" % ao, p["wrow"], m * p["wrow"])), why
        elif p["kind"] not in ("refused", "empty"):
            assert (p["wtype"], p["w"]) == (t, "as+%d" % ao), why
        if not ws:
            assert p["msg"] != "mul_mat_id: workspace too small" and (p["kind"] == "refused" or p["need"] <= p["size"]), why
        if env.get("CDNA4_MOE_SK") == "0":
            assert p["kind"] != "queue", why
        kinds.add(p["kind"])
        checked += 1
    assert checked == len(cells)
    want = {"empty", "refused", "tiles_mmq", "tiles_t64", "tiles_kq", "gemv_1", "gemv"} | (set() if env.get("CDNA4_MOE_SK") == "0" else {"queue"})
    assert kinds == want, kinds


def test_each_mul_mat_id_knob_is_read_in_one_place():
    """CDNA4_MMQ_IDS used to be read twice under two names (in front of the work queue and in front of the int8 route): once now, in the plan's knobs"""
    text = open(os.path.join(ROOT, "ggml_amd", "csrc", "capi.hip")).read()
    assert text.count('getenv("CDNA4_MMQ_IDS")') == 1
    for knob in ("CDNA4_MOE_SK", "CDNA4_NO_MMQ_IDS", "CDNA4_SK_CW"):
        assert text.count('getenv("%s")' % knob) == 1, knob


def test_no_route_probe_is_left_in_the_kernel_library():
    """the armed probe (a thread-local switch that made the launcher return in front of its first side effect) is gone: the queries read the plan"""
    csrc = os.path.join(ROOT, "ggml_amd", "csrc")
    for d, _, files in os.walk(csrc):
        for f in files:
            text = open(os.path.join(d, f), errors="replace").read()
            assert "g_probe" not in text and "ROUTE_END" not in text, os.path.join(d, f)


def test_hardware_verified_kernels_are_unchanged():
    """tools/isa_manifest.py: the ISA of every kernel that was part of a build with a green hardware session (profiles/rNN/isa_manifest.json,
    `hw`: true) is what hipcc emits for it today — so what was added since (listed there as `hw`: false, or new) cannot have changed the
    kernels the MI355X numbers and parity results belong to.  Comparable only under the compiler that wrote the record."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    import glob
    import importlib.util
    mans = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "isa_manifest.json")))
    assert mans, "no profiles/rNN/isa_manifest.json"
    spec = importlib.util.spec_from_file_location("isa_manifest", os.path.join(ROOT, "tools", "isa_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ok, changed_hw, changed, new, gone = mod.check(mans[-1])
    if not ok:
        pytest.skip("the manifest was written under another compiler version")
    gone_hw = [g for g in gone if json_hw(mans[-1], g)]
    if changed_hw or gone_hw:
        # Round 3 works on the kernels themselves with the GPU in the loop: a changed kernel is not an error, it is a kernel whose evidence is
        # the NEXT hardware session (scripts/gpu_tests_only.sh), after which the manifest is rewritten.  The emulator is a lint, not a gate.
        pytest.skip("%d hardware-verified kernels changed / %d gone since %s was written (e.g. %s): their evidence is the next GPU session"
                    % (len(changed_hw), len(gone_hw), os.path.relpath(mans[-1], ROOT), (changed_hw + gone_hw)[:3]))


def json_hw(path, fk):
    import json
    return json.load(open(path))["kernels"][fk[0]][fk[1]]["hw"]


# ---- the WHOLE library on the CPU (tools/emul/lib_emul.h): ggml_cdna4_mul_mat / _mul_mat_id through the C-ABI of a host build of the product's own sources.
# (Wave-collectives complete among the lanes that execute them — tools/emul/hip_emul.h, Sync — so any shape runs, partial waves included.)
LIB_TYPES = [("q4_0", 2), ("q4_1", 3), ("q5_0", 6), ("q5_1", 7), ("q8_0", 8), ("q2_K", 10), ("q3_K", 11), ("q4_K", 12), ("q5_K", 13), ("q6_K", 14), ("iq4_nl", 20), ("iq4_xs", 23)]


@pytest.mark.parametrize("name,t", LIB_TYPES)
def test_whole_library_mul_mat_on_the_cpu(name, t):
    """every accepted weight type through ggml_cdna4_mul_mat on the CPU, the three regimes of the AUTO route: one row (quantizer inside the GEMV
    launch), four rows (quantize + GEMV; Q8_1 activations for Q4_1 / Q5_1), 32 rows (the MFMA GEMM: its own kernel for the five headline formats —
    k_gemm_kq_t64 / w8p / the staging w12 with a split-K hand-off —, an exact re-encoding for the others: Q5_0 / IQ4_NL -> Q8_0, Q3_K -> Q6_K, and
    the two-part forms of Q2_K / Q4_1 / Q5_1 / IQ4_XS against the doubled activation image) — the host code between the C-ABI and the kernels
    included.  GEMV <= 1e-5, GEMM <= 1e-3 from the oracle's MUL_MAT of that type."""
    mod = _emul_module("lib_emul_check")
    for m, k, b, bar in ((40, 1024, 1, 1e-5), (24, 1024, 4, 1e-5), (130, 768, 32, 1e-3)):
        r = mod.mul_mat(t, m, k, b, seed=t + b, timeout=300)
        if r is None:
            pytest.skip("the environment cannot host the emulation")
        assert r[0] < bar, (name, m, k, b, r[0])


@pytest.mark.parametrize("t", [12, 13])
@pytest.mark.parametrize("m,k,b,cus", [(512, 1024, 256, 2), (300, 512, 300, 2), (256, 2048, 200, 1)])
def test_whole_library_large_grid_route_on_the_cpu(m, k, b, cus, t):
    """Q4_K / Q5_K where the 256 x 256 tiles of k_gemm_r8 fill (a pretend chip of `cus` CUs): AUTO takes that kernel, unsplit — two tiles on 2 CUs, four
    ragged tiles on 2 CUs, one tile on 1 CU (its split-K exchange: tools/emul/emul_check.py, kernel="lds") — through the C-ABI on the CPU, within the GEMM bar of the oracle"""
    r = _emul_module("lib_emul_check").mul_mat(t, m, k, b, seed=m + b, cus=cus, timeout=900)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 1e-3, r[0]


@pytest.mark.parametrize("m,k,b,cus", [(512, 768, 80, 8), (512, 512, 100, 8), (512, 256, 100, 4)])
def test_whole_library_one_launch_step_on_the_cpu(m, k, b, cus):
    """round 5's one-launch step (k_gemm_kq_t64<.., FQ>: activation quantizer -> two-level grid barrier -> multiply) through the C-ABI on the CPU, on pretend chips whose
    grids are resident and whose quantizer share is one pass: split in two with an uneven superblock count (hand-off inside the launch), split in two evenly on 8 work-groups,
    unsplit — each bit-identical to the two launches it replaces (CDNA4_NO_FUSEQ=1), with the LDS-DMA landing immediately and as late as the counted waits allow"""
    mod = _emul_module("lib_emul_check")
    import numpy as np
    got = {}
    for tag, envs in (("one", {}), ("two", {"CDNA4_NO_FUSEQ": "1"}), ("one_deferred", {"EMU_DEFER_DMA": "1"})):
        old = {k_: os.environ.get(k_) for k_ in ("CDNA4_NO_FUSEQ", "EMU_DEFER_DMA")}
        os.environ.update(envs)
        try:
            r = mod.mul_mat(12, m, k, b, path=2, seed=m + b, cus=cus, timeout=900)
        finally:
            for k_, v_ in old.items():
                if v_ is None:
                    os.environ.pop(k_, None)
                else:
                    os.environ[k_] = v_
        if r is None:
            pytest.skip("the environment cannot host the emulation")
        assert r[0] < 1e-3, (tag, r[0])
        got[tag] = r[1]
    assert np.array_equal(got["one"].view(np.uint32), got["two"].view(np.uint32))
    assert np.array_equal(got["one"].view(np.uint32), got["one_deferred"].view(np.uint32))
    # and it IS the one-launch route on that chip (asked of the emulated library's own routing; in a process of its own: the CU count is cached per process)
    import subprocess, sys
    code = ("import ctypes, sys; so = ctypes.CDLL(sys.argv[1]); f = so.ggml_cdna4_mul_mat_route; f.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3; "
            "print(f(12, %d, %d, %d))" % (m, k, b))
    r = subprocess.run([sys.executable, "-c", code, mod.build_so()], capture_output=True, text=True, timeout=300, env=dict(os.environ, EMU_CUS=str(cus)))
    assert r.returncode == 0 and r.stdout.strip() == "11", (r.stdout, r.stderr[-500:])


@pytest.mark.parametrize("name,t", [("q4_1", 3), ("iq4_nl", 20), ("iq4_xs", 23), ("q2_K", 10)])
def test_whole_library_small_k_gemm_route_on_the_cpu(name, t):
    """K = 256: the re-encoded matrix is too shallow for the staging kernel (2 superblocks of the target format) and takes the re-layout + 8-wave
    kernel; the shape of the stock harness's MUL_MAT cases (m = 16, k = 256, n = 16 -> here 32 activation rows for whole waves)"""
    r = _emul_module("lib_emul_check").mul_mat(t, 16, 256, 32, seed=t, timeout=300)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 1e-3, r[0]


@pytest.mark.parametrize("name,t", [("q4_1", 3), ("q5_1", 7), ("iq4_nl", 20), ("iq4_xs", 23), ("q4_K", 12)])
def test_whole_library_mul_mat_id_on_the_cpu(name, t):
    """ggml_cdna4_mul_mat_id on the CPU: one token (one launch, quantizer inside, ids read on the device) and four tokens with a broadcast
    activation row (quantize + GEMV with per-column experts)"""
    mod = _emul_module("lib_emul_check")
    for n_b, n_tok in ((2, 1), (1, 4)):
        r = mod.mul_mat_id(t, 64, 1024, 4, 2, n_b, n_tok, seed=t + n_tok, timeout=300)
        if r is None:
            pytest.skip("the environment cannot host the emulation")
        assert r < 1e-5, (name, n_b, n_tok, r)


@pytest.mark.parametrize("t,m,k,ne,nu,nb,nt", [(12, 128, 512, 4, 2, 2, 32), (12, 40, 256, 8, 2, 1, 40), (13, 130, 512, 3, 2, 2, 40), (14, 64, 256, 4, 2, 1, 40), (2, 50, 512, 4, 2, 2, 33), (8, 64, 256, 4, 2, 2, 33),
                                                (12, 64, 512, 2, 1, 1, 60)])
def test_whole_library_few_rows_per_expert_mul_mat_id_on_the_cpu(t, m, k, ne, nu, nb, nt):
    """MUL_MAT_ID with more than 32 (token, slot) rows but at most 32 per expert on average: the int8 matrix-core kernels over 32-row chunks of the expert-sorted
    image (k_mmq_*<2, 8> with the grouped argument block: expert from tile_expert, output rows through row_dst, chunks past a run exit; the last case gives one
    expert ~30 rows: two chunks of its tile, the second ragged) — the CPU's integer block dots: <= 1e-5 from the oracle, where the grouped fp16 GEMM sits at 3e-4"""
    os.environ["CDNA4_MMQ_IDS"] = "2"                                 # (Q4_K keeps its grouped fp16 GEMM in AUTO — faster on MI355X, capi.hip; forced here so that its kernel is covered too)
    try:
        r = _emul_module("lib_emul_check").mul_mat_id(t, m, k, ne, nu, nb, nt, seed=7, timeout=900)
    finally:
        os.environ.pop("CDNA4_MMQ_IDS", None)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r < 1e-5, r


@pytest.mark.parametrize("m,k,ne,nu,nb,nt,cus", [(300, 512, 3, 2, 2, 70, 2), (256, 1024, 4, 2, 1, 90, 4)])
def test_whole_library_grouped_mul_mat_id_on_256_row_tiles_on_the_cpu(m, k, ne, nu, nb, nt, cus):
    """the grouped Q4_K launch on k_gemm_kq_t64<.., 256, IDS> (taken once the grouped grid offers 3/4 of a 256-row tile per CU of a pretend small chip): ragged m, padding rows,
    broadcast activation rows — within the GEMM bar of the oracle's MUL_MAT_ID"""
    r = _emul_module("lib_emul_check").mul_mat_id(12, m, k, ne, nu, nb, nt, seed=3, cus=cus, timeout=900)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r < 1e-3, r


@pytest.mark.parametrize("m,k,ne,nu,nb,nt", [(130, 1024, 3, 2, 2, 70), (256, 2048, 4, 2, 1, 40)])
def test_whole_library_grouped_mul_mat_id_with_the_ticketed_k_split_on_the_cpu(m, k, ne, nu, nb, nt):
    """the grouped Q4_K launch where its tiles outnumber (a pretend chip of 2) CUs: every tile is computed by TWO work-groups over half of K each; the
    last one to arrive adds both partial tiles in the order ks = 0, 1 and stores (nobody waits: the tiles need not be co-resident); ticket counters
    back at zero afterwards (the next call of the same process — the second size — starts from them)"""
    mod = _emul_module("lib_emul_check")
    os.environ["CDNA4_MOE_SPLITK"] = "2"                             # (opt-in: a measured loss on MI355X, gemm_q_t64.hip)
    try:
        r = mod.mul_mat_id(12, m, k, ne, nu, nb, nt, seed=5, cus=2, timeout=900)
    finally:
        os.environ.pop("CDNA4_MOE_SPLITK", None)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r < 1e-3, r


@pytest.mark.parametrize("name,t", LIB_TYPES)
def test_whole_library_stock_harness_shapes_on_the_cpu(name, t):
    """the shapes of the reference's test-backend-ops MUL_MAT sweep (m = 16, k = 256, n = 1 / 9 / 16: tests/test-backend-ops.cpp:4005-4081) through the
    C-ABI on the CPU — quantizers with partly filled waves, the shallow-K GEMM routes, the two-part forms at their smallest size"""
    mod = _emul_module("lib_emul_check")
    for b in (1, 9, 16):
        r = mod.mul_mat(t, 16, 256, b, seed=t + b, timeout=300)
        if r is None:
            pytest.skip("the environment cannot host the emulation")
        assert r[0] < (1e-5 if b <= 8 else 1e-3), (name, b, r[0])


@pytest.mark.parametrize("name,t", [("q4_0", 2), ("q8_0", 8), ("q5_0", 6), ("q4_1", 3), ("q5_1", 7), ("iq4_nl", 20)])
@pytest.mark.parametrize("k", [544, 992, 96])
def test_32_weight_formats_with_k_not_a_multiple_of_64_on_the_cpu(name, t, k):
    """a bug of round 2's decode kernel that only the whole-library emulation showed: lds_swz() permutes 16-byte chunks of the int8 activation row
    inside groups of four, so with K % 64 == 32 and K mod 1024 >= 512 the row's last two chunks landed on its scales (K = 544: rel-L2 1e27).  Such
    K now take the quantize + GEMV pair (cdna4_gemv_fused_supported); one row, and MUL_MAT_ID's single-token form, through the C-ABI"""
    mod = _emul_module("lib_emul_check")
    r = mod.mul_mat(t, 16, k, 1, seed=k, timeout=300)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r[0] < 1e-5, (name, k, r[0])
    assert mod.mul_mat_id(t, 32, k, 4, 2, 2, 1, seed=k + 1, timeout=300) < 1e-5


_GEMV_ENTRY_POINTS = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import refutil as R
so, t = C.CDLL(sys.argv[1]), int(sys.argv[3])
i64, vp = C.c_int64, C.c_void_p
so.cdna4_emul_alloc.restype = vp; so.cdna4_emul_alloc.argtypes = [C.c_size_t]
so.ggml_cdna4_mul_mat_workspace_size.restype = C.c_size_t; so.ggml_cdna4_mul_mat_workspace_size.argtypes = [C.c_int, i64, i64]
so.ggml_cdna4_last_error.restype = C.c_char_p
so.ggml_cdna4_mul_mat.restype = C.c_int
so.ggml_cdna4_mul_mat.argtypes = [C.c_int, vp, i64, vp, i64, vp, i64, i64, i64, i64, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
def dev(a):                                     # "device" memory of the emulation: a shared mapping the work-group processes write into
    a = np.ascontiguousarray(a); p = so.cdna4_emul_alloc(max(a.nbytes, 1))
    v = np.frombuffer((C.c_uint8 * max(a.nbytes, 1)).from_address(p), a.dtype, a.size).reshape(a.shape); v[...] = a
    return p, v
def call(m, k, b, path=0, w_pad=0, k_ref=None):
    # k_ref: the K the operands are made for (a bad call names another K on them); w_pad: extra bytes between weight rows
    kr = k_ref or k
    w = R.random_weights(t, m, kr, seed=t + b).view(np.uint8).reshape(m, -1)
    x = np.random.default_rng(t + b + 1).uniform(-1, 1, (b, kr)).astype(np.float32)
    wp, _ = dev(np.pad(w, ((0, 0), (0, w_pad)))); xp, _ = dev(x)
    yp, y = dev(np.full((b, m), -12345.0, np.float32))
    nws = so.ggml_cdna4_mul_mat_workspace_size(t, kr, b); ws, _ = dev(np.zeros(nws + 256, np.uint8))
    rc = so.ggml_cdna4_mul_mat(t, wp, w.shape[1] + w_pad, xp, kr, yp, m, m, k, b, ws, nws, path, 0, 0, None)
    return rc, y.copy(), (so.ggml_cdna4_last_error() or b"").decode(), R.o_mul_mat(t, w, x, m, kr)
kq, main5 = R.BLCK[t] == 256, t in (R.Q4_K, R.Q5_K, R.Q6_K, R.Q4_0, R.Q8_0)
good = [("fused", dict(m=24, k=256, b=1))]
if main5: good += [("fused_n", dict(m=24, k=256, b=3))]
good += [("plain", dict(m=24, k=256, b=9, path=1) if kq else dict(m=24, k=288, b=9))]
bad = [("k", dict(m=24, k=288 if kq else 272, k_ref=512, b=bb)) for bb in (1, 3, 9)]
if t == R.Q4_K: bad += [("pitch", dict(m=24, k=256, b=bb, w_pad=2, path=pp)) for bb, pp in ((1, 0), (3, 0), (9, 1))]
out = {"good": [], "bad": []}
for name, kw in good:
    rc, y, msg, ref = call(**kw)
    out["good"].append([name, rc, msg if rc else "", bool((y != -12345.0).all()) and R.rel_l2(y, ref)])
for name, kw in bad:
    rc, y, msg, _ = call(**kw)
    out["bad"].append([name, kw["b"], rc, msg, bool((y == -12345.0).all())])
print(json.dumps(out))
"""


@pytest.mark.parametrize("name,t", LIB_TYPES)
def test_whole_library_gemv_entry_points_accept_and_reject_on_the_cpu(name, t):
    """every weight type through ggml_cdna4_mul_mat of the emulated library at the smallest shapes that reach each GEMV launcher of gemv_q.hip — one row (the one-launch
    form), three rows of the five headline formats (the one-launch form for 2..8 rows), nine rows on the plain quantize + GEMV pair (K = 288 for the 32-weight
    formats; an explicit GEMV path for the superblock formats) — within the GEMV bar of the oracle.  (The staged form takes over from 32 K activation values per
    call, beyond these sizes: test_small_batch_decode_kernel_source_on_the_cpu launches it directly.)  And the calls
    the launchers and the call in front of them refuse: a K that is not a whole number of blocks, and for Q4_K a row pitch that is not a multiple of 16 bytes.
    Those return non-zero with their own message and leave the output untouched."""
    import json
    import sys
    mod = _emul_module("lib_emul_check")
    r = subprocess.run([sys.executable, "-c", _GEMV_ENTRY_POINTS, mod.build_so(), os.path.join(ROOT, "tests"), str(t)], capture_output=True, text=True, timeout=600)
    if r.returncode == 77:
        pytest.skip("the environment cannot host the emulation")
    assert r.returncode == 0, (r.stdout + r.stderr)[-800:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = ["fused"] + (["fused_n"] if t in (12, 13, 14, 2, 8) else []) + ["plain"]
    assert [g[0] for g in got["good"]] == want
    for form, rc, msg, err in got["good"]:
        assert rc == 0 and err is not False and err < 1e-5, (name, form, rc, msg, err)
    assert len(got["bad"]) == (6 if t == 12 else 3)
    for kind, b, rc, msg, untouched in got["bad"]:
        assert rc != 0 and untouched, (name, kind, b, rc, msg)
        assert msg == ("mul_mat: K is not a whole number of blocks" if kind == "k" else "gemv_q: Q4_K/Q5_K rows must be 16-byte aligned"), (name, kind, b, msg)


@pytest.mark.parametrize("t,m,k,ne,nu,nb,nt", [(12, 128, 512, 4, 2, 2, 32), (12, 64, 256, 8, 2, 1, 40), (12, 130, 768, 3, 2, 2, 70),
                                                (13, 130, 512, 3, 2, 2, 40), (14, 64, 256, 4, 2, 1, 40), (2, 130, 384, 3, 2, 2, 40), (8, 64, 256, 4, 2, 2, 33)])
def test_whole_library_grouped_mul_mat_id_on_the_cpu(t, m, k, ne, nu, nb, nt):
    """prefill-sized MUL_MAT_ID through the C-ABI on the CPU: the device-side counting sort of the expert ids (k_moe_plan), the gathering
    activation quantizer (Q8_K / Q8_0) and the grouped launch — k_gemm_kq_t64<.., IDS> for Q4_K, k_gemm_q<.., IDS> for Q5_K / Q6_K / Q4_0 / Q8_0 —
    ragged per-expert counts, padding rows, broadcast activation rows"""
    r = _emul_module("lib_emul_check").mul_mat_id(t, m, k, ne, nu, nb, nt, seed=5, timeout=300)
    if r is None:
        pytest.skip("the environment cannot host the emulation")
    assert r < 1e-3, r
