#!/bin/bash
# Timing and per-kernel split of alq_hess_vecp (tools/gpu_hvp.py): profiles/hvp_*.json, profiles/hvp_*_kernel_stats.csv and the
# table in DESIGN.md.  Every GPU step runs under its own time limit and the chain stops at the first step that fails.  The
# profiler runs are separate processes (program directly after `--`, kernel trace only: no counters in the same run).
# usage: tools/run_hvp_profile.sh [output dir, default profiles]
set -eo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$ROOT/profiles}"
TMP="$(mktemp -d)"
mkdir -p "$OUT"
cd "$ROOT"
timeout -k 10 240 python3 tools/gpu_hvp.py --net netc --out "$OUT/hvp_netc32_B32.json" &&
timeout -k 10 420 python3 tools/gpu_hvp.py --net netb --out "$OUT/hvp_netb_B200.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$TMP/netc" -o stats --output-format csv -- python3 tools/gpu_hvp.py --net netc --reps 2 > /dev/null &&
timeout -k 10 480 rocprofv3 --kernel-trace --stats -d "$TMP/netb" -o stats --output-format csv -- python3 tools/gpu_hvp.py --net netb --reps 2 > /dev/null || exit 1
for n in netc32_B32:netc netb_B200:netb; do
  f="$(find "$TMP/${n#*:}" -name '*kernel_stats.csv' | head -1)"
  cp "$f" "$OUT/hvp_${n%%:*}_kernel_stats.csv"
  python3 tools/gpu_hvp.py --stats "$OUT/hvp_${n%%:*}_kernel_stats.csv" --out "$OUT/hvp_${n%%:*}.json" > /dev/null
done
python3 tools/gpu_hvp.py --table "$OUT/hvp_netc32_B32.json" "$OUT/hvp_netb_B200.json" --design "$ROOT/DESIGN.md"
rm -rf "$TMP"
