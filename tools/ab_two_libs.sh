#!/bin/bash
# Same-box A/B of two builds of the library on the default bench: arm A = the other build (e.g. the parent commit's, built from a
# second checkout with csrc/build.sh and copied next to libalq.so under another name), arm B = libalq.so.
#   bash tools/ab_two_libs.sh <tag> <file name of the other build inside the package> [rounds]
# 1. bench.py --steps 1 --warmup 1 --dump-outputs per arm: sha256 of every .npy, both lists and the verdict;
# 2. <rounds> alternating rounds of the default command at 20 steps; every branch round must beat every parent round and the median
#    gain must exceed three times the parent arm's own spread (max - min) for the script to call it a gain;
# 3. one rocprofv3 --kernel-trace --stats run of `bench.py --lanes 1 --no-accuracy` per arm: per-launch times of the first conv and
#    the up2 kernels, of the fused enc2 backward launch (e3d_bwd_kernel = row sweep, e3d_bwdz_kernel = z plane sweep), and the sum of the
#    13 main-chain launches of a pass (neighbouring launches trade clock: only the sum counts).
# Everything lands in $OUT (bench_out by default): <tag>_ab.txt, <tag>_checksums.txt, <tag>_{parent,branch}_lanes1_kernel_stats.csv.
# Every GPU step has its own time limit and the script stops at the first step that fails.
set -eo pipefail
TAG=$1; OTHER=$2; R=${3:-3}
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${OUT:-$ROOT/bench_out}"; mkdir -p "$OUT"; export TMPDIR=/tmp
cd "$ROOT"
test -f "nn-active-learning_amd/$OTHER"
arm() { if [ "$1" = parent ]; then echo "ALQ_LIB=$OTHER"; fi; }      # environment of an arm: the branch arm loads libalq.so
for A in parent branch; do
  rm -rf "$OUT/${TAG}_dump_$A"
  timeout -k 10 300 env $(arm $A) python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --dump-outputs "$OUT/${TAG}_dump_$A" > "$OUT/${TAG}_dump_$A.json" 2> "$OUT/${TAG}_dump_$A.err"
  echo "dump $A done"
done
python3 - "$OUT" "$TAG" <<'PY'
import hashlib, os, sys
out, tag = sys.argv[1:3]
sums = {}
for arm in ('parent', 'branch'):
    d = os.path.join(out, '%s_dump_%s' % (tag, arm))
    sums[arm] = {}
    for root, _, files in os.walk(d):
        for f in sorted(files):
            if f.endswith('.npy'):
                sums[arm][os.path.relpath(os.path.join(root, f), d)] = hashlib.sha256(open(os.path.join(root, f), 'rb').read()).hexdigest()
names = sorted(set(sums['parent']) | set(sums['branch']))
same = bool(names) and all(sums['parent'].get(n) == sums['branch'].get(n) for n in names)
with open(os.path.join(out, tag + '_checksums.txt'), 'w') as fh:
    fh.write('sha256 of bench.py --steps 1 --warmup 1 --dump-outputs, parent build / this build\n')
    for n in names:
        fh.write('%-12s %s %s %s\n' % (n, sums['parent'].get(n), sums['branch'].get(n), 'equal' if sums['parent'].get(n) == sums['branch'].get(n) else 'DIFFERENT'))
    fh.write('all byte-equal: %s\n' % same)
print(open(os.path.join(out, tag + '_checksums.txt')).read())
sys.exit(0 if same else 1)
PY
rm -rf "$OUT/${TAG}_dump_parent" "$OUT/${TAG}_dump_branch"
for i in $(seq 1 $R); do
  for A in parent branch; do
    timeout -k 10 300 env $(arm $A) python3 bench.py --gpus 1 --steps 20 --warmup 2 --no-cpu-baseline > "$OUT/${TAG}_${A}_$i.json" 2> "$OUT/${TAG}_${A}_$i.err"
    echo "round $i $A done"
  done
done
python3 - "$OUT" "$TAG" "$R" <<'PY'
import json, os, statistics, sys
out, tag, R = sys.argv[1], sys.argv[2], int(sys.argv[3])
v = {a: [json.loads(open(os.path.join(out, '%s_%s_%d.json' % (tag, a, i))).read().strip().splitlines()[-1])['value'] for i in range(1, R + 1)]
     for a in ('parent', 'branch')}
mp, mb = statistics.median(v['parent']), statistics.median(v['branch'])
spread = max(v['parent']) - min(v['parent'])
gain = mb - mp
clear = min(v['branch']) > max(v['parent']) and gain > 3 * spread
lines = ['default bench, 20 steps, arms alternating in one job on one machine (patches/s)',
         'parent rounds: ' + ' '.join('%.1f' % x for x in v['parent']),
         'branch rounds: ' + ' '.join('%.1f' % x for x in v['branch']),
         'medians: parent %.1f  branch %.1f  gain %.1f (%.2f %%)' % (mp, mb, gain, 100 * gain / mp),
         'parent spread (max - min): %.1f (%.2f %%)   3 x spread: %.1f' % (spread, 100 * spread / mp, 3 * spread),
         'every branch round beats every parent round: %s' % (min(v['branch']) > max(v['parent'])),
         'clearly faster (both conditions): %s' % clear]
open(os.path.join(out, tag + '_ab.txt'), 'w').write('\n'.join(lines) + '\n')
print('\n'.join(lines))
PY
for A in parent branch; do
  timeout -k 10 400 env $(arm $A) rocprofv3 --kernel-trace --stats -d "$OUT/${TAG}_${A}_stats" -o stats --output-format csv -- python3 bench.py --lanes 1 --no-cpu-baseline --no-accuracy > "$OUT/${TAG}_${A}_lanes1_under_rocprof.json" 2> "$OUT/${TAG}_${A}_rp.err"
  cp "$OUT/${TAG}_${A}_stats"/*/stats_kernel_stats.csv "$OUT/${TAG}_${A}_lanes1_kernel_stats.csv" 2>/dev/null || cp "$OUT/${TAG}_${A}_stats"/stats_kernel_stats.csv "$OUT/${TAG}_${A}_lanes1_kernel_stats.csv"
  rm -rf "$OUT/${TAG}_${A}_stats"
  echo "trace $A done"
done
python3 - "$OUT" "$TAG" <<'PY' | tee -a "$OUT/${TAG}_ab.txt"
import csv, os, sys
out, tag = sys.argv[1:3]
print('per-launch averages, --lanes 1 kernel trace (us): parent -> branch')
rows = {a: {r['Name']: r for r in csv.DictReader(open(os.path.join(out, '%s_%s_lanes1_kernel_stats.csv' % (tag, a))))} for a in ('parent', 'branch')}
def pick(a, key):
    return [(n, float(r['AverageNs']) / 1e3, int(r['Calls'])) for n, r in rows[a].items() if key in n]
for key in ('direct_conv_pool_kernel', 't3d_bwd_kernel', 't3d_fwd_kernel', 'd3d_bwd', 'c3d_fwd', 'c3d_bwd7', 'e3d_bwd'):
    p, b = pick('parent', key), pick('branch', key)
    print('  %-26s %s -> %s' % (key, ' '.join('%.1f (%d calls)' % (t, c) for _, t, c in p), ' '.join('%.1f (%d calls)' % (t, c) for _, t, c in b)))
# the main chain of a NET-C Fisher pass: the first conv + the twelve contraction launches, once per pass each
chain = ('direct_conv_pool_kernel', 'f3d_fwd', 'igemm4_kernel', 't3d8_fwd', 'd3d_fwd', 't3d_fwd_kernel', 'c3d_fwd', 'c3d_bwd7', 't3d_bwd_kernel', 'd3d_bwd',
         't3d8_bwd', 'e3d_bwd')
tot = {a: sum(t for key in chain for _, t, _ in pick(a, key)) for a in ('parent', 'branch')}
cnt = {a: sum(1 for key in chain for _ in pick(a, key)) for a in ('parent', 'branch')}
print('  main chain, sum of %d / %d launches: %.1f -> %.1f us per pass (%+.2f %%)' % (cnt['parent'], cnt['branch'], tot['parent'], tot['branch'],
                                                                                   100 * (tot['branch'] - tot['parent']) / tot['parent']))
PY
