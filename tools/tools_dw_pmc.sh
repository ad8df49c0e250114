#!/bin/bash
# usage (GPU box, repo root): bash tools/tools_dw_pmc.sh <tag>   -- which unit bounds the weight gradient's 64 x 64-block
# kernel (k_conv_dw_pairs) inside the bench's own step?  Two rocprofv3 --pmc passes of their own over the bench command (no
# trace domains in a --pmc run): SQ (vector-memory read instructions, MFMA busy) and vector L1 (accesses, clocked share);
# tools/tools_dw_pmc_summary.py writes $BENCH_OUT/dw_vec_pmc_<tag>.txt (default bench_out/).  BENCH=<path> profiles another tree's bench.py
# (the parent commit's, for the before / after pair).
set -u
root=$(cd "$(dirname "$0")/.." && pwd)
tag=${1:?tag}
bench=${BENCH:-$root/bench.py}
out=$(cd $root && mkdir -p ${BENCH_OUT:-bench_out} && cd ${BENCH_OUT:-bench_out} && pwd)
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
pass() { # name counters...
  n=$1; shift
  rm -rf $out/pmc_dw_${tag}_$n
  timeout -k 10 300 rocprofv3 --pmc "$@" --output-format csv -d $out/pmc_dw_${tag}_$n -- python3 $bench --gpus 1 --steps 3 --warmup 2 --no-prewarm --min-timed-s 0 > $out/pmc_dw_${tag}_$n.log 2>&1
  rc=$?
  echo "$n rc=$rc"
  return $rc
}
pass sq SQ_INSTS_VMEM_RD SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE || exit 1
pass tcp TCP_TOTAL_CACHE_ACCESSES TCP_TCC_READ_REQ TCP_GATE_EN1 TCP_GATE_EN2 GRBM_GUI_ACTIVE || exit 1
cd $root && python3 tools/tools_dw_pmc_summary.py $tag $out > $out/dw_vec_pmc_$tag.txt || exit 1
rm -rf $out/pmc_dw_${tag}_sq $out/pmc_dw_${tag}_tcp
cat $out/dw_vec_pmc_$tag.txt
