"""Dev tool: time the RPN head (rpn_glue.rpn_head, csrc/rpn_head.hip) over six maps at the benchmark's size, forward and
forward + backward, in three forms on the same tensors and parameters:
  fused        rpn_glue.rpn_head: one launch for all maps
  torch        what bench.py's own head does: torch.cat of the maps' rows, three torch Linears, ReLU
  dense_linear roi_glue.dense_linear map by map and layer by layer (csrc/roi_mlp.hip)
The site total is the bench's (profiles/r06_bench_line.json: anchors_per_scene summed over the 4 scenes / 4 yaws =
17356 sites); its split over the six maps is a stand-in (`--rows`), C = 128, A = 4.

The parent starts two children, each under its own `timeout` and only while the one before ended well: `--child time`
alternates the forms in `--repeats` windows of `--iters` calls after `--warmup` calls of every form (device events
around a window that ends in a synchronise; median and min .. max over the windows), `--child count` counts the device
operations per call of each form with torch.profiler, in a process of its own.  Writes `--out`
(profiles/rpn_head_timing.txt)."""
import argparse
import importlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FORMS = ("fused", "torch", "dense_linear")
MODES = (("forward", False), ("forward+backward", True))


def setup(rows, C, A):
    sys.path.insert(0, REPO)
    importlib.import_module("automatic-as-built-reconstruction_amd")
    import torch
    import roi_glue
    import rpn_glue
    torch.manual_seed(0)
    lin = [torch.nn.Linear(C, C), torch.nn.Linear(C, A), torch.nn.Linear(C, 7 * A)]
    for l in lin:
        torch.nn.init.normal_(l.weight, std=0.01)
        l.to(DEV)
    feats = [torch.randn((n, C), device=DEV, requires_grad=True) for n in rows]
    g_obj = [torch.randn(n * A, device=DEV) for n in rows]
    g_reg = [torch.randn((n * A, 7), device=DEV) for n in rows]
    params = [q for l in lin for q in (l.weight, l.bias)]

    def forward(form):
        if form == "fused":
            return rpn_glue.rpn_head(feats, *params)
        if form == "torch":
            t = torch.relu(lin[0](torch.cat(feats)))
            return [lin[1](t).reshape(-1)], [lin[2](t).reshape(-1, 7)]
        obj, reg = [], []
        for f in feats:
            t = roi_glue.dense_linear(f, lin[0].weight, lin[0].bias, relu=True)
            obj.append(roi_glue.dense_linear(t, lin[1].weight, lin[1].bias).reshape(-1))
            reg.append(roi_glue.dense_linear(t, lin[2].weight, lin[2].bias).reshape(-1, 7))
        return obj, reg

    def call(form, backward):
        if not backward:
            with torch.no_grad():
                return forward(form)
        for q in params + feats:
            q.grad = None
        obj, reg = forward(form)
        if form == "torch":
            torch.autograd.backward(obj + reg, [torch.cat(g_obj), torch.cat(g_reg)])
        else:
            torch.autograd.backward(obj + reg, g_obj + g_reg)
    return torch, call


def child_time(args):
    torch, call = setup(args.rows, args.C, args.A)
    out = {}
    for mode, backward in MODES:
        for form in FORMS:
            for _ in range(args.warmup):
                call(form, backward)
        ts = {f: [] for f in FORMS}
        for _ in range(args.repeats):
            for form in FORMS:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    call(form, backward)
                e1.record()
                torch.cuda.synchronize()
                ts[form].append(1000.0 * e0.elapsed_time(e1) / args.iters)
        for form in FORMS:
            t = sorted(ts[form])
            out["%s|%s" % (mode, form)] = [t[len(t) // 2], t[0], t[-1]]
    print("RESULT " + json.dumps(out))


def child_count(args):
    torch, call = setup(args.rows, args.C, args.A)
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for mode, backward in MODES:
        for form in FORMS:
            call(form, backward)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                call(form, backward)
                torch.cuda.synchronize()
            out["%s|%s" % (mode, form)] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    print("RESULT " + json.dumps(out))


def run_child(kind, args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind, "--iters",
           str(args.iters), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--C", str(args.C), "--A",
           str(args.A), "--rows"] + [str(n) for n in args.rows]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stdout.write(r.stdout)
        raise SystemExit("child `%s` ended with status %d: nothing further is started" % (kind, r.returncode))
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[3470, 1040, 350, 8680, 2950, 866])
    ap.add_argument("--C", type=int, default=128)
    ap.add_argument("--A", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--child", choices=("time", "count"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rpn_head_timing.txt"))
    args = ap.parse_args()
    if args.child == "time":
        return child_time(args)
    if args.child == "count":
        return child_count(args)
    times = run_child("time", args, 240)
    counts = run_child("count", args, 120)
    n, C, A = sum(args.rows), args.C, args.A
    macs = n * (C * C + 8 * A * C)
    lines = ["RPN head: %d maps, rows %s (%d sites), C = %d, A = %d; fp32" % (len(args.rows), args.rows, n, C, A),
             "median of %d windows of %d calls after %d warm-up calls of every form (min .. max); device events; the forms "
             "alternate window by window in one process" % (args.repeats, args.iters, args.warmup),
             "%.3f GFLOP forward (multiply-adds x 2), three times that forward + backward" % (2e-9 * macs)]
    for mode, _ in MODES:
        for form in FORMS:
            m, lo, hi = times["%s|%s" % (mode, form)]
            lines.append("%-17s %-13s %9.1f us (%.1f .. %.1f);  %d device operations per call"
                         % (mode, form, m, lo, hi, counts["%s|%s" % (mode, form)]))
        for form in FORMS[1:]:
            lines.append("%s: fused / %s = %.2f" % (mode, form, times["%s|fused" % mode][0] / times["%s|%s" % (mode, form)][0]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
