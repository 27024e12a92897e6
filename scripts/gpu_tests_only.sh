#!/bin/bash
# every -m gpu test WITHOUT -x (one failure must not hide the rest), per-test results kept: $CDNA4_OUT/pytest_gpu.log (-rA lines) + junit xml
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
OUT=$(mkdir -p "${CDNA4_OUT:-out}" && cd "${CDNA4_OUT:-out}" && pwd); export CDNA4_OUT="$OUT"      # all output of the session, the tests' reports included
rm -f "$OUT"/gpt2_parity.jsonl "$OUT"/parity_report.jsonl "$OUT"/split_report.jsonl
timeout -k 10 ${GPU_TESTS_TIMEOUT:-1800} python -m pytest tests -m gpu -q --tb=short -rA -p no:cacheprovider --junitxml="$OUT"/pytest_gpu.xml "$@" > "$OUT"/pytest_gpu.log 2>&1
echo "pytest -m gpu rc=$?"; grep -E "^(FAILED|ERROR)" "$OUT"/pytest_gpu.log | head -40; tail -3 "$OUT"/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke.log 2>&1; echo "smoke rc=$?"; tail -2 "$OUT"/smoke.log
