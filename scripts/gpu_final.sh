#!/bin/bash
# a round's full session on HEAD: every -m gpu test, smoke, bench.py --full (all legs, then the driver's shape without extras), rocprofv3 kernel stats + four PMC passes over `bench.py --lean`
# (separate runs, kernel-trace only), the same for the decode loop at 4096 x 14336 and (stats only) the grouped MUL_MAT_ID loop, gemm_bench over the BASELINE shapes; condensed on
# the box (tools/summarize_prof.py) -> $CDNA4_OUT/profile_summary/, to be copied into profiles/rNN/
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
OUT=$(mkdir -p "${CDNA4_OUT:-out}" && cd "${CDNA4_OUT:-out}" && pwd); export CDNA4_OUT="$OUT"      # all output of the session, the tests' reports included
R=$PWD; export TMPDIR=/tmp PYTHONUNBUFFERED=1
rm -rf "$OUT"/summary.txt "$OUT"/parity_report.jsonl "$OUT"/gpt2_parity.jsonl "$OUT"/split_report.jsonl "$OUT"/prof_* "$OUT"/pmc_* "$OUT"/profile_summary
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 2400 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > "$OUT"/pytest_gpu.log 2>&1
  echo "pytest -m gpu rc=$?" >> "$OUT"/summary.txt; tail -5 "$OUT"/pytest_gpu.log >> "$OUT"/summary.txt
fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" > "$OUT"/smoke.log 2>&1; echo "smoke rc=$?" >> "$OUT"/summary.txt
timeout -k 10 700 python bench.py --full > "$OUT"/bench.log 2> "$OUT"/bench.err; echo "bench rc=$?" >> "$OUT"/summary.txt
timeout -k 10 200 python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-extras --no-cpu-baseline > "$OUT"/bench_driver_cmd.log 2>> "$OUT"/bench.err; echo "bench (driver's shape, no extras) rc=$?" >> "$OUT"/summary.txt
( cd tools/microbench
  for shape in "4096 4096 512" "4096 11008 512" "8192 4096 512"; do GB_SPLITKS=0 GB_VARIANTS="0,24583" GB_ROUNDS=5 timeout 120 ./gemm_bench $shape ""; done
  L=268435456; R8=$((L+67108864))
  for shape in "32768 8192 512" "16384 8192 512"; do GB_SPLITKS=0 GB_VARIANTS="0,40967,$R8" GB_ROUNDS=5 timeout 120 ./gemm_bench $shape ""; done
) 2>&1 | grep -E "^M=|^variant" > "$OUT"/gemm_bench.txt
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -o r1 -- python "$R/bench.py" --steps 200 --warmup 20 --lean > "$OUT/rocprof_stats.log" 2>&1
echo "rocprof stats rc=$?" >> "$OUT/summary.txt"
for pmc in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU"; do
  name=$(echo "$pmc" | tr ' ' '+')
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $pmc --output-format csv -d "$OUT/pmc_$name" -o p -- python "$R/bench.py" --steps 100 --warmup 10 --lean > "$OUT/rocprof_pmc_$name.log" 2>&1
  echo "pmc [$pmc] rc=$?" >> "$OUT/summary.txt"
done
cd "$R"
rocminfo > "$OUT"/rocminfo.txt 2>&1; nproc > "$OUT"/nproc.txt
python tools/summarize_prof.py "$OUT" "$OUT"/profile_summary > "$OUT"/summarize.log 2>&1
# the decode kernel at 4096 x 14336: kernel stats + instruction / wave-cycle counters + traffic (the one-launch k_gemv_q_fused<Q4_K, 16, 1>)
cd /tmp
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_decode" -o r1 -- python "$R/scripts/decode_loop.py" > "$OUT/rocprof_decode.log" 2>&1
for pmc in "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM" "FETCH_SIZE" "WRITE_SIZE"; do
  name=$(echo "$pmc" | tr ' ' '+' | cut -c1-40)
  timeout -k 10 200 rocprofv3 --kernel-trace --pmc $pmc --output-format csv -d "$OUT/pmcd_$name" -o p -- python "$R/scripts/decode_loop.py" > "$OUT/rocprof_pmcd_$name.log" 2>&1
done
cd "$R"
python3 - > "$OUT"/profile_summary/pmc_decode_counters.txt <<'PY'
import csv, glob, collections, os
print("# rocprofv3 --kernel-trace --pmc <pass> -- python scripts/decode_loop.py (Q4_K 4096 x 14336, one launch per token, rotating matrices); per-launch averages")
for d in sorted(glob.glob(os.environ['CDNA4_OUT'] + '/pmcd_*')):
    f=os.path.join(d,'p_counter_collection.csv')
    if not os.path.isdir(d) or not os.path.exists(f): continue
    agg=collections.defaultdict(lambda: collections.defaultdict(list)); dur=collections.defaultdict(list)
    for r in csv.DictReader(open(f)): agg[r['Kernel_Name']][r['Counter_Name']].append(float(r['Counter_Value']))
    for r in csv.DictReader(open(os.path.join(d,'p_kernel_trace.csv'))): dur[r['Kernel_Name']].append((int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e3)
    for k,cs in agg.items():
        if 'gemv' not in k: continue
        print(os.path.basename(d)[6:], k[:60], 'n=%d' % len(next(iter(cs.values()))), 'avg_dur_us(profiled)=%.2f' % (sum(dur[k])/max(1,len(dur[k]))), {c: round(sum(v)/len(v)) for c,v in cs.items()})
PY
( cd /tmp && timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_moe" -o r1 -- python "$R/scripts/moe_ab.py" > "$OUT/rocprof_moe.log" 2>&1 )
MS=$(find "$OUT"/prof_moe -name "*kernel_stats.csv" 2>/dev/null | head -1)
if [ -n "$MS" ]; then head -6 "$MS" > "$OUT"/profile_summary/rocprofv3_moe_kernel_stats.csv; grep tag "$OUT"/rocprof_moe.log > "$OUT"/profile_summary/moe_under_profiler.txt; fi
if [ -f "$OUT"/prof_decode/r1_kernel_stats.csv ]; then cp "$OUT"/prof_decode/r1_kernel_stats.csv "$OUT"/profile_summary/rocprofv3_decode_kernel_stats.csv; fi
cp "$OUT"/pytest_gpu.log "$OUT"/profile_summary/pytest_gpu_final.log 2>/dev/null
cp "$OUT"/bench_driver_cmd.log "$OUT"/profile_summary/ 2>/dev/null
cp "$OUT"/bench.log "$OUT"/profile_summary/bench_final.log 2>/dev/null; cp "$OUT"/summary.txt "$OUT"/profile_summary/summary_final.txt
rm -rf "$OUT"/prof_stats "$OUT"/prof_decode "$OUT"/prof_moe "$OUT"/pmc_* "$OUT"/pmcd_*
cat "$OUT"/summary.txt; cat "$OUT"/gemm_bench.txt | cut -c1-160; cat "$OUT"/profile_summary/pmc_decode_counters.txt | cut -c1-400; head -c 1200 "$OUT"/bench_driver_cmd.log; echo; grep -v '^$' "$OUT"/profile_summary/pmc_summary.txt | cut -c1-330 | head -40
