"""Summarise the two --pmc passes of tools/tools_dw_pmc.sh (argv[1] = tag, argv[2] = its output directory): the weight-gradient kernels of the bench's step,
per kernel instance and grid size, mean per launch, and per CU and elapsed cycle (GRBM_GUI_ACTIVE of the same pass is summed
over the 8 XCDs).  The last block adds the launches of one instance up: what a step's worth of it asks of each unit."""
import collections
import csv
import glob
import os
import re
import sys

TAG = sys.argv[1]
OUT = sys.argv[2] if len(sys.argv) > 2 else "bench_out"
PASSES = ("sq", "tcp")
CUS, SIMDS = 256, 1024


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*\)$", "", name)
    return name.replace("aabr::", "").replace(" ", "")


def rows(p):
    files = glob.glob("%s/pmc_dw_%s_%s/**/*counter_collection.csv" % (OUT, TAG, p), recursive=True)
    return list(csv.DictReader(open(max(files, key=os.path.getmtime)))) if files else []


acc = {}
for p in PASSES:
    d = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in rows(p):
        k = short(r["Kernel_Name"])
        if "k_conv_dw" in k:
            d[(k, int(r.get("Grid_Size", 0)))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    acc[p] = d

print("# tools/tools_dw_pmc.sh %s: rocprofv3 --pmc, two passes of their own over `bench.py --gpus 1 --steps 3 --warmup 2 "
      "--no-prewarm --min-timed-s 0` (fp32)." % TAG)
print("# per (kernel, grid size in work-items): launches, then per counter the mean per launch | per CU and elapsed cycle")
print("# derived: vmem_rd x 32 clk / cycles = share of the launch a CU's vector L1 needs at one load instruction per 32 clocks")
print("#          (each CU sees vmem_rd / 256 of the wave instructions); mfma = MFMA busy cycles / (1024 SIMDs x cycles)")
tot = collections.defaultdict(lambda: collections.defaultdict(float))
for key in sorted(acc["sq"], key=lambda k: (k[0], -k[1])):
    k, grid = key
    line = ["%s grid=%d" % (k, grid)]
    der = {}
    for p in PASSES:
        c = acc[p].get(key, {})
        gui = c.get("GRBM_GUI_ACTIVE", [])
        if not gui:
            continue
        cyc = sum(gui) / len(gui) / 8.0
        line.append("  [%s] launches %d, %.0f cycles" % (p, len(gui), cyc))
        tot[k]["cycles_" + p] += sum(gui) / 8.0
        tot[k]["launches_" + p] += len(gui)
        for n in sorted(c):
            if n == "GRBM_GUI_ACTIVE":
                continue
            v = sum(c[n]) / len(c[n])
            tot[k][n] += sum(c[n])
            line.append("    %-28s %14.1f | %8.4f" % (n, v, v / (CUS * cyc)))
            der[n] = v / cyc
    if "SQ_INSTS_VMEM_RD" in der:
        line.append("    derived: L1 instruction share %.3f, mfma busy %.3f" % (
            der["SQ_INSTS_VMEM_RD"] / CUS * 32.0, der.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / SIMDS))
    print("\n".join(line))
print("# totals over all launches of an instance in the profiled run (5 steps)")
for k in sorted(tot):
    t = tot[k]
    cs, ct = t.get("cycles_sq", 0.0), t.get("cycles_tcp", 0.0)
    if cs <= 0:
        continue
    print("%s: %d launches, %.0f cycles; vmem_rd %.0f (L1 instruction share %.3f), mfma busy %.3f%s" % (
        k, t["launches_sq"], cs, t["SQ_INSTS_VMEM_RD"], t["SQ_INSTS_VMEM_RD"] / CUS * 32.0 / cs,
        t["SQ_VALU_MFMA_BUSY_CYCLES"] / (SIMDS * cs),
        "; L1 accesses per CU and cycle %.3f, L1 clocked %.3f" % (t["TCP_TOTAL_CACHE_ACCESSES"] / (CUS * ct),
                                                                  t["TCP_GATE_EN1"] / (CUS * ct)) if ct > 0 else ""))
