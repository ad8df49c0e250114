#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/tools_profile.sh <tag> [bench args...]
# runs the GPU tests, a rocprofv3 kernel-trace of bench.py --full and an un-profiled bench --full line
tag=$1; shift
: "${GRAFT_REPO_ROOT:?run this on the GPU box (gpurun sets it)}"
root=$GRAFT_REPO_ROOT
out=${BENCH_OUT:-$root/bench_out}
mkdir -p $out
timeout -k 10 600 python -m pytest $root/tests -q -m gpu --timeout 300 > $out/gpu_tests.log 2>&1; echo "pytest rc=$?"; tail -3 $out/gpu_tests.log
export TMPDIR=${TMPDIR:-/tmp} && cd $TMPDIR && rm -rf $out/prof_$tag
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --full --steps 300 --warmup 200 --no-cpu-baseline "$@" > $out/bench_prof_$tag.log 2>&1; echo "prof rc=$?"
cd $root && timeout -k 10 300 python bench.py --full --no-cpu-baseline "$@" > $out/bench_$tag.log 2>$out/bench_$tag.err; echo "bench rc=$?"; cat $out/bench_$tag.log
