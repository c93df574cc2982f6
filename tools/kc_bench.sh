#!/bin/bash
# GPU-box: configs[2] bench with and without the validator-key cache, then the key-cache tests.
# Logs go to $EDC_OUT_DIR (default bench_out).
out=${EDC_OUT_DIR:-bench_out}
mkdir -p "$out"
for kc in "" "--keycache"; do
  for r in 1 2; do
    timeout -k 10 120 python -u bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --profile-steps 1 $kc > "$out/kcb.log" 2>&1 || exit $?
    echo "kc='$kc' $(tail -1 "$out/kcb.log" | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"], d["phases_ms"])')"
  done
done
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > "$out/gpu_tests.log" 2>&1; rc=$?; tail -1 "$out/gpu_tests.log"; exit $rc
