#!/bin/bash
# The four bench lines a round keeps under profiles/ (run on the GPU box from the repo root):
#   default command, the driver's command, bf16 storage, configs[4].   usage: tools_bench_lines.sh [tag] [first|second|all]
# Lines go to $BENCH_OUT (default bench_out/).  All but the driver's command run with --full.
R=${1:-r06}
W=${2:-all}
OUT=${BENCH_OUT:-bench_out}
mkdir -p $OUT
if [ "$W" != second ]; then
timeout -k 10 560 python bench.py --full > $OUT/${R}_bench_line.json 2> $OUT/${R}_bench_line.err
timeout -k 10 560 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/${R}_bench_line_driver_command.json 2> $OUT/${R}_bench_line_driver_command.err
fi
if [ "$W" != first ]; then
timeout -k 10 560 python bench.py --full --dtype bf16 > $OUT/${R}_bench_line_bf16.json 2> $OUT/${R}_bench_line_bf16.err
timeout -k 10 560 python bench.py --full --config 4 > $OUT/${R}_bench_line_config4.json 2> $OUT/${R}_bench_line_config4.err
fi
python - <<PY
import json
for f in ["", "_driver_command", "_bf16", "_config4"]:
    try:
        d = json.load(open("$OUT/${R}_bench_line%s.json" % f))
    except Exception as e:
        print(f or "default", "unreadable:", e); continue
    vs = d.get("voxel_scatter", {})
    rf = d.get("roofline", {})      # the driver's command is a plain run: no roofline
    print(f or "default", d["value"], d["ms_per_step"], d["dtype"], rf.get("frac"), rf.get("traffic"),
          vs.get("device_seconds"), vs.get("traffic_over_algorithmic"),
          {k: v.get("scenes_per_s") for k, v in d.get("extras", {}).items() if isinstance(v, dict)})
PY
