#!/bin/bash
# Build liborbx.so of another commit (default: HEAD~1, the parent) as
# orb_slam_cuda_amd/variants/liborbx_parent.so, for tools/parent_ab_c3.sh and
# tools/parent_ab_serial.sh (loaded with ORBX_LIB_VARIANT=parent). A plain build
# with the Makefile's flags, in a temporary git worktree that is removed again.
#   tools/build_parent_lib.sh [COMMIT]
set -e
cd "$(dirname "$0")/.."
rev=${1:-HEAD~1}
wt=$(mktemp -d)/orbx_parent
git worktree add --detach "$wt" "$rev" > /dev/null
trap 'git worktree remove --force "$wt"' EXIT
make -s -j8 -C "$wt/orb_slam_cuda_amd/csrc"
mkdir -p orb_slam_cuda_amd/variants
cp "$wt/orb_slam_cuda_amd/liborbx.so" orb_slam_cuda_amd/variants/liborbx_parent.so
echo "built orb_slam_cuda_amd/variants/liborbx_parent.so from $(git rev-parse --short "$rev")"
