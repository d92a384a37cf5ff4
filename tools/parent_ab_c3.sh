#!/bin/bash
# Plain bench.py with the parent commit's library and the working tree's, alternating.
#   tools/parent_ab_c3.sh [PAIRS=5] [OUTDIR=bench_out/parent_ab]
# The parent's library is orb_slam_cuda_amd/variants/liborbx_parent.so, built by
# tools/build_parent_lib.sh (a plain build of HEAD~1, no -DORBX_DIAG), loaded
# with ORBX_LIB_VARIANT=parent; both sides run with --allow-diag so the lines match.
# After the pairs, one line per side for --config euroc and --config kitti14.
set -o pipefail
cd "$(dirname "$0")/.."
N=${1:-5}; O=${2:-bench_out/parent_ab}; mkdir -p $O
run() {  # tag side [bench args]
  local tag=$1 v=$2; shift 2
  if [ $v = parent ]; then export ORBX_LIB_VARIANT=parent; else unset ORBX_LIB_VARIANT; fi
  timeout -k 10 240 python3 bench.py --allow-diag "$@" > $O/$tag.log 2>&1 || { echo "$tag failed"; tail -5 $O/$tag.log; return 1; }
  python3 -c "import json;d=json.loads(open('$O/$tag.log').read().strip().splitlines()[-1]);print('$tag',d['value'],d.get('ms_per_step'))" | tee -a $O/summary.txt
}
for i in $(seq 1 $N); do
  run kitti_parent_$i parent || exit 1
  run kitti_new_$i new || exit 1
done
for cfg in euroc kitti14; do
  for v in parent new; do run ${cfg}_$v $v --config $cfg || exit 1; done
done
