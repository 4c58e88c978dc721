#!/bin/bash
# Per-kernel durations of the bench step (and of what a --full run adds: per-kernel events, tail, e2e): rocprofv3 kernel
# trace -> $PROF_OUT/<tag>_kernel_stats.csv (default prof_out/)
# usage (on the GPU box): bash tools/prof_kernels.sh <tag> [extra bench args]
tag=${1:-run}; shift
repo=$(pwd)
out=${PROF_OUT:-$repo/prof_out}
export TMPDIR=/tmp
mkdir -p $out
cd /tmp && rm -rf /tmp/prof_$tag && timeout 600 rocprofv3 --kernel-trace -d /tmp/prof_$tag -- python $repo/bench.py --steps 12 --warmup 3 --full --no-cpu-baseline --no-extras "$@" > $out/${tag}_bench.json 2> $out/${tag}_prof.err
db=$(find /tmp/prof_$tag -name "*.db" | head -1)
python $repo/tools/rocpd_kernel_stats.py $db $out/${tag}_kernel_stats.csv > /dev/null
head -14 $out/${tag}_kernel_stats.csv | sed 's/"_ZN2lt[0-9]*\(k_[a-z_0-9]*\)[^"]*"/\1/' | cut -c1-120
python $repo/tools/rocpd_timeline.py $db > $out/${tag}_timeline.txt 2>&1
