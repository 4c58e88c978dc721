#!/bin/bash
# Round-6 measurement set on the GPU box (repo root): kernel stats / timelines (rocprofv3 --kernel-trace) of the default
# bench step, of the exhaustive mode and of BASELINE config 3; counter file (tools/prof_pmc_json.sh); bench lines.
# Everything lands in $PROF_OUT/r06_* (default prof_out/); copy what is to be judged into profiles/.
repo=$(pwd)
export PROF_OUT=${PROF_OUT:-$repo/prof_out}
export TMPDIR=/tmp
mkdir -p $PROF_OUT
run_trace() {  # tag, bench args...
  tag=$1; shift
  cd /tmp && rm -rf /tmp/prof_$tag
  timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_$tag -- python $repo/bench.py --full --no-cpu-baseline --no-extras "$@" \
      > $PROF_OUT/${tag}_trace_bench.json 2> $PROF_OUT/${tag}_prof.err
  db=$(find /tmp/prof_$tag -name "*.db" | head -1)
  python $repo/tools/rocpd_kernel_stats.py $db $PROF_OUT/${tag}_kernel_stats.csv > /dev/null
  python $repo/tools/rocpd_timeline.py $db > $PROF_OUT/${tag}_timeline.txt 2>&1
  python $repo/tools/rocpd_step_timeline.py $db > $PROF_OUT/${tag}_step_timeline.txt 2>&1
  cd $repo
}
run_trace r06 --steps 30 --warmup 3
run_trace r06_exhaustive --steps 6 --warmup 1 --mode exhaustive
run_trace r06_config3 --steps 12 --warmup 2 --config3
TAG=r06 bash tools/prof_pmc_json.sh > $PROF_OUT/r06_pmc_summary.txt 2>&1
bash tools/prof_stream_pmc.sh > $PROF_OUT/r06_stream_pmc_summary.txt 2>&1
cp $PROF_OUT/r06_pmc.json $PROF_OUT/r06_stream_pmc.json profiles/ 2>/dev/null  # (bench.py quotes the counters of the matching hash)
python bench.py --full > $PROF_OUT/bench_r06.json 2> $PROF_OUT/bench_r06.err
python bench.py --stream > $PROF_OUT/bench_r06_stream.json 2> $PROF_OUT/bench_r06_stream.err
python bench.py --mode exhaustive --full --no-cpu-baseline --no-extras > $PROF_OUT/bench_r06_exhaustive.json 2> $PROF_OUT/bench_r06_exhaustive.err
python bench.py --config3 --full --no-cpu-baseline --no-extras > $PROF_OUT/bench_r06_config3_n1.json 2> $PROF_OUT/bench_r06_config3.err
LT_BENCH_FORCE_DIST=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29541 \
    bench.py --gpus 1 --full --no-cpu-baseline > $PROF_OUT/bench_r06_forcedist.json 2> $PROF_OUT/bench_r06_forcedist.err
head -12 $PROF_OUT/r06_kernel_stats.csv | cut -c1-150
cat $PROF_OUT/r06_step_timeline.txt
tail -8 $PROF_OUT/r06_pmc_summary.txt | cut -c1-300
tail -3 $PROF_OUT/r06_stream_pmc_summary.txt | cut -c1-400
