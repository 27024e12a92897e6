#!/bin/bash
# full GPU session: every -m gpu test, smoke, bench, rocprofv3 kernel stats + PMC passes (separate runs, kernel-trace only)
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
OUT=$(mkdir -p "${CDNA4_OUT:-out}" && cd "${CDNA4_OUT:-out}" && pwd); export CDNA4_OUT="$OUT"      # all output of the session, the tests' reports included
rm -rf "$OUT"/summary.txt "$OUT"/parity_report.jsonl "$OUT"/gpt2_parity.jsonl "$OUT"/prof_* "$OUT"/pmc_*
export PYTHONUNBUFFERED=1
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > "$OUT"/pytest_gpu.log 2>&1
  echo "pytest -m gpu rc=$?" >> "$OUT"/summary.txt; tail -5 "$OUT"/pytest_gpu.log >> "$OUT"/summary.txt
fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" > "$OUT"/smoke.log 2>&1; echo "smoke rc=$?" >> "$OUT"/summary.txt
timeout -k 10 600 python bench.py --full > "$OUT"/bench.log 2>&1; echo "bench rc=$?" >> "$OUT"/summary.txt
# gemm_bench (product kernels): auto route, the round-1 loader-wave kernel (4119), k_gemm_kq_t64 with 128-row (24583) and 256-row (40967) tiles
GB_SPLITKS="0" GB_VARIANTS="0,4119,24583" timeout 180 tools/microbench/gemm_bench 4096 4096 512 "" 2>&1 | grep -E "^M=|^variant" > "$OUT"/gemm_bench.txt
for shape in "4096 11008 512" "8192 4096 512" "8192 8192 512" "4096 14336 512"; do
  GB_SPLITKS="0" GB_VARIANTS="0,4119,24583" timeout 180 tools/microbench/gemm_bench $shape "" 2>&1 | grep -E "^M=|^variant" >> "$OUT"/gemm_bench.txt
done
GB_SPLITKS="0" GB_VARIANTS="0,4119,24583,40967" timeout 180 tools/microbench/gemm_bench 32768 8192 512 "" 2>&1 | grep -E "^M=|^variant" >> "$OUT"/gemm_bench.txt
# timing-only ablations + in-kernel stage trace of k_gemm_kq_t64 (tools/microbench: make abl), the MFMA / VALU probe
if [ -x tools/microbench/gemm_bench_abl ]; then
  B=40967; V="$B"; for a in 1 3 4 8 15 32; do V="$V,$((B + a*65536))"; done
  (cd tools/microbench; GB_VARIANTS="$V" GB_SPLITKS=1 GB_TRACE_REPS=30 timeout 300 ./gemm_bench_abl 32768 8192 512 "$((B + 256*65536))") > "$OUT"/t64_ablations.txt 2>&1
  B=24583; V="4119,$B"; for a in 1 3 4 8 15 32; do V="$V,$((B + a*65536))"; done
  (cd tools/microbench; GB_VARIANTS="$V" GB_SPLITKS=2 GB_TRACE_SPLITK=2 GB_TRACE_REPS=30 timeout 300 ./gemm_bench_abl 4096 4096 512 "$((B + 256*65536))") >> "$OUT"/t64_ablations.txt 2>&1
fi
timeout 120 tools/microbench/mfma_valu 2000 > "$OUT"/mfma_valu_probe.txt 2>&1
bash scripts/gpu_pmc1.sh > "$OUT"/pmc_gemm_bench_sq.txt 2>&1
R=$PWD; cd /tmp; export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -o r1 -- python "$R/bench.py" --steps 200 --warmup 20 --lean > "$OUT/rocprof_stats.log" 2>&1
echo "rocprof stats rc=$?" >> "$OUT/summary.txt"
for pmc in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU"; do
  name=$(echo "$pmc" | tr ' ' '+')
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $pmc --output-format csv -d "$OUT/pmc_$name" -o p -- python "$R/bench.py" --steps 100 --warmup 10 --lean > "$OUT/rocprof_pmc_$name.log" 2>&1
  echo "pmc [$pmc] rc=$?" >> "$OUT/summary.txt"
done
cd "$R"
# only summaries travel back (gpurun merges at most 64 MiB): condense, then drop the raw rocprofv3 output
rocminfo > "$OUT"/rocminfo.txt 2>&1; nproc > "$OUT"/nproc.txt
python tools/summarize_prof.py "$OUT" "$OUT"/profile_summary > "$OUT"/summarize.log 2>&1
rm -rf "$OUT"/prof_stats "$OUT"/pmc_* "$OUT"/pmcg_*
cat "$OUT"/summary.txt; grep -E "^M=|^variant" "$OUT"/gemm_bench.txt | head -60; tail -1 "$OUT"/bench.log
