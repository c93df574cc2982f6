#!/bin/bash
# configs[1] (2^16 distinct keys): step time by (window bits, MSM parts), one batch at a time
# (INFLIGHT=1, with the per-phase times) or pipelined (INFLIGHT=8). Logs go to $EDC_OUT_DIR
# (default bench_out).
set -o pipefail
out=${EDC_OUT_DIR:-bench_out}
mkdir -p "$out"
inf=${INFLIGHT:-1}
for wb in ${BITS:-11 12 13}; do for p in ${PARTS:-1 2 4 8}; do
  timeout -k 10 120 python -u bench.py --full --config c2 --steps 30 --warmup 4 --inflight $inf --no-cpu-baseline --window-bits $wb --msm-parts $p > "$out/c2s.log" 2>&1 || { echo fail; tail -5 "$out/c2s.log"; exit 1; }
  echo "wb=$wb parts=$p inflight=$inf $(tail -1 "$out/c2s.log" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); ph=d["phases_ms"]; print(d["ms_per_step"], ph["msm_bin"], ph["msm_bucket"], ph["msm_window_final"])')"
done; done
