#!/bin/bash
# Per-kernel serial times (rocprofv3 --stats, every kernel alone on the chip) of the
# parent commit's library (variants/liborbx_parent.so, built by tools/build_parent_lib.sh) and
# the working tree's, alternating, twice each.
#   tools/parent_ab_serial.sh [OUTDIR=bench_out/parent_serial]
set -o pipefail
cd "$(dirname "$0")/.."; export TMPDIR=/tmp
O=${1:-bench_out/parent_serial}; mkdir -p $O
for i in 1 2; do
  for v in parent new; do
    if [ $v = parent ]; then export ORBX_LIB_VARIANT=parent; else unset ORBX_LIB_VARIANT; fi
    OUT=$O/${v}_$i
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -o run -- python3 bench.py --allow-diag --serial --steps 20 --warmup 3 --cpu-sample 0 --no-latency --no-host-stream > $OUT.log 2>&1 || { echo "$v $i failed"; tail -5 $OUT.log; exit 1; }
    echo "== $v $i"
    python3 tools/stats_brief.py $OUT/run_kernel_stats.csv | grep -E "pyr_band|blur_kernel|fast_cells|orient_brief|quadtree|hamming_top2"
  done
done | tee $O/summary.txt
