#!/bin/bash
# Timing, peak memory and per-kernel split of the diagonal Fisher's two arms (tools/gpu_diagfisher.py): profiles/diagf_*.json,
# profiles/diagf_*_kernel_stats.csv and the table in DESIGN.md.  Every GPU step runs under its own time limit and the chain stops
# at the first step that fails.  The profiler run is a process of its own (program directly after `--`, kernel trace only: no
# counters in the same run) and traces the fused arm alone.
# usage: tools/run_diagfisher_profile.sh [output dir, default profiles]
set -eo pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${1:-$ROOT/profiles}"
TMP="$(mktemp -d)"
mkdir -p "$OUT"
cd "$ROOT"
timeout -k 10 240 python3 tools/gpu_diagfisher.py --net netc --out "$OUT/diagf_netc32_B64.json" &&
timeout -k 10 420 python3 tools/gpu_diagfisher.py --net netb --out "$OUT/diagf_netb_B64.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$TMP/netc" -o stats --output-format csv -- python3 tools/gpu_diagfisher.py --net netc --arm fused --reps 2 > /dev/null &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats -d "$TMP/netb" -o stats --output-format csv -- python3 tools/gpu_diagfisher.py --net netb --arm fused --reps 2 > /dev/null || exit 1
for n in netc32_B64:netc netb_B64:netb; do
  f="$(find "$TMP/${n#*:}" -name '*kernel_stats.csv' | head -1)"
  cp "$f" "$OUT/diagf_${n%%:*}_kernel_stats.csv"
  python3 tools/gpu_diagfisher.py --stats "$OUT/diagf_${n%%:*}_kernel_stats.csv" --out "$OUT/diagf_${n%%:*}.json" > /dev/null
done
python3 tools/gpu_diagfisher.py --table "$OUT/diagf_netc32_B64.json" "$OUT/diagf_netb_B64.json" --design "$ROOT/DESIGN.md"
rm -rf "$TMP"
