"""Dev tool: time the six pooling passes (csrc/pool.hip: Max / Average / UnPooling, forward and backward) at the input
level of a BASELINE configs[2]-sized batch (4 synthetic wall scenes, synth_scenes.make_batch), 2/2 and 3/2 windows, 32 and
128 planes, fp32 and bf16 storage, against what a user would otherwise write in torch over the same rule pairs:
  max      zeros.index_reduce_(0, out_rows, x.index_select(0, in_rows), 'amax')          backward: a masked index_add_
  average  zeros.index_add_(0, out_rows, x.index_select(0, in_rows) / vol)               backward: index_add_ the other way
  unpool   zeros.index_add_(0, in_rows, coarse.index_select(0, out_rows))                backward: index_add_ the other way
(the pair lists are built once, outside the timed region; the torch forms use float atomics and are not reproducible).

Device events around `--iters` back-to-back calls after a warm-up of each form; the two forms alternate in `--repeats`
windows; median and min .. max over the windows.  Algorithmic bytes per pass: rules x planes x element size read (twice for
the max backward, which reads y and dy, plus its x rows), destination rows x planes x element size written, vol x
destination rows x 4 table bytes; GB/s = those bytes over the device time.  The parent starts the child under its own
`timeout`.  Writes `--out` (profiles/pool_timing.txt)."""
import argparse
import importlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def child_time(args):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    importlib.import_module("automatic-as-built-reconstruction_amd")
    import torch
    import synth_scenes as S
    import sparseconvnet as scn
    from sparseconvnet import SCN
    locs, _ = S.make_batch(args.batch, args.npts, 0, 20)
    L = lambda v: torch.LongTensor([int(i) for i in v])
    results = []

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    for size, stride in ((2, 2), (3, 2)):
        spatial = [s + (size - stride) for s in S.FULL_SCALE]          # an exact fit of the windows
        layer = scn.InputLayer(3, spatial, mode=4)
        layer.site_order = "brick"
        x0 = layer([torch.as_tensor(locs).to(DEV), torch.zeros((len(locs), 1), device=DEV)])
        md, fine = x0.metadata, x0.spatial_size
        coarse = (fine - size) // stride + 1
        geom = (fine, coarse, L([size] * 3), L([stride] * 3))
        tb = md.getRuleBook(*geom)
        vol, V, Vo = tb.vol, tb.V_in, tb.V_out
        t = tb.out.table
        k_, out_rows = (t >= 0).nonzero(as_tuple=True)
        in_rows = t[k_, out_rows].long()
        n_rules = int(in_rows.numel())
        for planes in (32, 128):
            for dtype in (torch.float32, torch.bfloat16):
                es = 2 if dtype == torch.bfloat16 else 4
                torch.manual_seed(0)
                x = torch.randn((V, planes), device=DEV).to(dtype)
                dy = torch.randn((Vo, planes), device=DEV).to(dtype)
                dfine = torch.randn((V, planes), device=DEV).to(dtype)
                y, dx, a, z, dc = (torch.empty(0, device=DEV, dtype=dtype) for _ in range(5))
                dc = torch.empty((Vo, planes), device=DEV, dtype=dtype)
                SCN.MaxPooling_updateOutput(*geom, md, x, y, 0)
                zeros = lambda rows: torch.zeros((rows, planes), device=DEV, dtype=dtype)
                rd, wr = n_rules * planes * es, lambda rows: rows * planes * es + vol * rows * 4
                passes = [
                    ("max fwd", lambda: SCN.MaxPooling_updateOutput(*geom, md, x, y, 0),
                     lambda: zeros(Vo).index_reduce_(0, out_rows, x.index_select(0, in_rows), "amax"), rd + wr(Vo)),
                    ("max bwd", lambda: SCN.MaxPooling_updateGradInput(*geom, md, x, dx, y, dy, 0),
                     lambda: zeros(V).index_add_(0, in_rows, dy.index_select(0, out_rows) *
                                                 (y.index_select(0, out_rows) == x.index_select(0, in_rows))),
                     2 * rd + V * planes * es + wr(V)),
                    ("avg fwd", lambda: SCN.AveragePooling_updateOutput(*geom, md, x, a, 0),
                     lambda: zeros(Vo).index_add_(0, out_rows, x.index_select(0, in_rows) / vol), rd + wr(Vo)),
                    ("avg bwd", lambda: SCN.AveragePooling_updateGradInput(*geom, md, x, dx, dy, 0),
                     lambda: zeros(V).index_add_(0, in_rows, dy.index_select(0, out_rows) / vol), rd + wr(V)),
                    ("unpool fwd", lambda: SCN.UnPooling_updateOutput(geom[1], geom[0], geom[2], geom[3], md, dy, z, 0),
                     lambda: zeros(V).index_add_(0, in_rows, dy.index_select(0, out_rows)), rd + wr(V)),
                    ("unpool bwd", lambda: SCN.UnPooling_updateGradInput(geom[1], geom[0], geom[2], geom[3], md, dc,
                                                                         dfine, 0),
                     lambda: zeros(Vo).index_add_(0, out_rows, dfine.index_select(0, in_rows)), rd + wr(Vo)),
                ]
                for name, dev_fn, torch_fn, nbytes in passes:
                    dev_fn()
                    try:
                        torch_fn()
                        have_torch = True
                    except Exception:                  # a form torch does not offer for this dtype
                        have_torch = False
                    td, tt = [], []
                    for _ in range(args.repeats):
                        td.append(timed(dev_fn))
                        if have_torch:
                            tt.append(timed(torch_fn))
                    med = lambda v: [sorted(v)[len(v) // 2], min(v), max(v)] if v else None
                    results.append(dict(window="%d/%d" % (size, stride), planes=planes, dtype=str(dtype).split(".")[1],
                                        name=name, rows_in=V, rows_out=Vo, rules=n_rules, bytes=nbytes, device=med(td),
                                        torch=med(tt)))
        del md, x0, tb, t
    print("RESULT " + json.dumps(results))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--npts", type=int, default=80000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--child", choices=("time",))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pool_timing.txt"))
    args = ap.parse_args()
    if args.child == "time":
        return child_time(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "time"]
    for k in ("batch", "npts", "iters", "repeats"):
        cmd += ["--" + k, str(getattr(args, k))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stdout.write(r.stdout)
        raise SystemExit("the timing child ended with status %d" % r.returncode)
    res = json.loads(line[-1][7:])
    lines = ["pooling passes (csrc/pool.hip) at the input level of %d synthetic scenes x %d points, brick site order; device "
             "events around %d calls, median of %d windows (min .. max), device and torch forms alternating after a warm-up "
             "of each" % (args.batch, args.npts, args.iters, args.repeats),
             "torch form: index_select + index_reduce_('amax') / index_add_ over the same rule pairs (pair lists built "
             "outside the timed region)",
             "bytes: rules x planes x element size read (max bwd: twice, + its x rows), destination rows x planes x element "
             "size written, vol x destination rows x 4 of table",
             "back-to-back calls on the same tensors: a case's working set (the MB column) mostly stays in the 256 MiB "
             "Infinity Cache, so GB/s is a rate of algorithmic bytes with warm caches, not an HBM rate",
             "%-6s %-6s %-9s %-11s %9s %9s %9s %10s %8s  %s" % ("window", "planes", "storage", "pass", "rows in", "rows out",
                                                               "rules", "MB", "GB/s", "device us (min .. max) | torch us")]
    for r_ in res:
        d, t = r_["device"], r_["torch"]
        lines.append("%-6s %-6d %-9s %-11s %9d %9d %9d %10.2f %8.0f  %8.1f (%.1f .. %.1f) | %s" % (
            r_["window"], r_["planes"], r_["dtype"], r_["name"], r_["rows_in"], r_["rows_out"], r_["rules"],
            r_["bytes"] / 1e6, r_["bytes"] / (d[0] * 1e-3) / 1e9, 1e3 * d[0], 1e3 * d[1], 1e3 * d[2],
            "%.1f (%.1f .. %.1f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2]) if t else "not available"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
