"""Time one optimizer step on the bench's parameter set (FPN_Net plus the RPN head, as bench.py builds them), three ways:

  (i)   torch.optim.SGD built by the reference's recipe (solver/build.py: one parameter group per parameter, momentum 0.9,
        the bias rule) -- the yardstick: the same arithmetic, issued group by group
  (ii)  dp.FlatParams.sgd_step, the plain `p -= lr * g` of the bench step -- a lower bound, not a comparison: no
        momentum, no weight decay, 12 bytes per parameter instead of 20
  (iii) solver_glue.FusedSGD (csrc/solver.hip): the same arithmetic as (i) in one library launch

and count the device operations (kernels and copies) one step issues, from torch.profiler.  The gradients are views of
one buffer with stable addresses, as the compiled backward hands them out.

    python tools/tools_solver_timing.py [--reps 30] [--out profiles/solver_timing.txt]

Every measurement runs in a child process of its own under its own time limit; the chain stops at the first child that
fails, and the file then says which numbers are missing.  Times are medians over `--reps` (>= 20) repetitions after 5
warm-up steps: device time between two events around the step, and host wall time of the step ending in a synchronise.
The streaming bound is 20 bytes per parameter (p, m, g read; p, m written) over the 6.29 TB/s a float4 copy reaches."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("torch_sgd", "sgd_step", "fused_sgd")
LABEL = {"torch_sgd": "(i)   torch.optim.SGD, one group per parameter", "sgd_step": "(ii)  dp.FlatParams.sgd_step (p -= lr g only)",
         "fused_sgd": "(iii) solver_glue.FusedSGD"}
COPY_RATE = 6.29e12      # bytes/s, float4 copy on the MI355X
CHILD_LIMIT_S = 300


def _setup(case):
    sys.path.insert(0, REPO)
    importlib.import_module("automatic-as-built-reconstruction_amd")
    import torch
    import sparseconvnet as scn
    import bench
    import dp
    import solver_glue
    from maskrcnn_benchmark.solver import make_optimizer
    from maskrcnn_benchmark.solver.build import param_groups
    dev = "cuda:0"
    net, head = bench.build_net(scn, torch, dev, torch.float32)
    model = torch.nn.ModuleList([net, head])
    cfg = solver_glue.solver_cfg()
    flat = dp.FlatParams([net, head])
    n = flat.flat.numel()
    torch.manual_seed(1)
    grad = torch.randn(n, device=dev) * 1e-3
    o = 0
    for p in flat.params:                 # stable addresses: views of one buffer
        p.grad = grad[o:o + p.numel()].view_as(p)
        o += p.numel()
    if case == "torch_sgd":
        groups = param_groups(cfg, model.named_parameters())
        opt = torch.optim.SGD(groups, groups[-1]["lr"], momentum=cfg.SOLVER.MOMENTUM)
        step = opt.step
    elif case == "sgd_step":
        step = lambda: flat.sgd_step(1e-5, 1)
    else:
        opt = make_optimizer(cfg, model, flat=flat)
        step = opt.step
    return torch, step, n, len(flat.params)


def child_time(case, reps):
    torch, step, n, n_tensors = _setup(case)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    dev_us, wall_us, enq_us = [], [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        step()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dev_us.append(e0.elapsed_time(e1) * 1e3)
        wall_us.append((t2 - t0) * 1e6)
        enq_us.append((t1 - t0) * 1e6)
    print(json.dumps(dict(case=case, n=n, tensors=n_tensors, reps=reps, device_us=statistics.median(dev_us),
                          wall_us=statistics.median(wall_us), enqueue_us=statistics.median(enq_us),
                          device_us_min=min(dev_us), device_us_max=max(dev_us))))


def child_count(case):
    torch, step, n, n_tensors = _setup(case)
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA"):
            names[ev.name] = names.get(ev.name, 0) + 1
    if not names:
        raise RuntimeError("torch.profiler recorded no device events")
    top = sorted(names.items(), key=lambda kv: -kv[1])[:4]
    print(json.dumps(dict(case=case, device_ops=sum(names.values()), top=top)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "solver_timing.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--case", default=None, choices=CASES)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child == "time":
        return child_time(a.case, a.reps)
    if a.child == "count":
        return child_count(a.case)
    commands, got, failed = [], {}, None
    for kind in ("time", "count"):
        for case in CASES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--case", case, "--reps", str(a.reps)]
            commands.append("timeout %d python tools/tools_solver_timing.py --child %s --case %s --reps %d"
                            % (CHILD_LIMIT_S, kind, case, a.reps))
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                                   timeout=CHILD_LIMIT_S)
            except subprocess.TimeoutExpired:
                failed = "%s %s: no result within %d s" % (kind, case, CHILD_LIMIT_S)
                break
            if r.returncode != 0:
                failed = "%s %s: exit status %d: %s" % (kind, case, r.returncode, (r.stderr.strip().splitlines() or [""])[-1])
                break
            got[(kind, case)] = json.loads(r.stdout.strip().splitlines()[-1])
        if failed:
            break               # nothing more is started on the GPU after a failure
    lines = ["One optimizer step on the bench's parameter set (tools/tools_solver_timing.py).", "", "commands (one child "
             "process each, in this order; the chain stops at the first failure):"]
    lines += ["  " + c for c in commands]
    t = {c: got.get(("time", c)) for c in CASES}
    c_ = {c: got.get(("count", c)) for c in CASES}
    any_t = next((v for v in t.values() if v), None)
    if any_t:
        n = any_t["n"]
        bound_us = 20.0 * n / COPY_RATE * 1e6
        lines += ["", "%d parameters in %d tensors (%.1f MB fp32); medians of %d repetitions after 5 warm-up steps"
                  % (n, any_t["tensors"], 4e-6 * n, any_t["reps"]),
                  "streaming bound of the momentum step: 20 B x parameters / 6.29 TB/s = %.1f us" % bound_us, "",
                  "%-50s %12s %12s %12s %16s" % ("case", "device us", "wall us", "enqueue us", "device ops/step")]
        for c in CASES:
            if t[c]:
                lines.append("%-50s %12.1f %12.1f %12.1f %16s" % (LABEL[c], t[c]["device_us"], t[c]["wall_us"],
                                                                 t[c]["enqueue_us"],
                                                                 c_[c]["device_ops"] if c_[c] else "not measured"))
            else:
                lines.append("%-50s %12s" % (LABEL[c], "not measured"))
        lines.append("  (device us: min .. max over the repetitions: " + ", ".join(
            "%s %.1f .. %.1f" % (c, t[c]["device_us_min"], t[c]["device_us_max"]) for c in CASES if t[c]) + ")")
        if t["fused_sgd"]:
            f = t["fused_sgd"]
            lines += ["", "FusedSGD: %.3f of the streaming bound by device time (%.1f / %.1f us)"
                      % (bound_us / f["device_us"], bound_us, f["device_us"])]
            if t["torch_sgd"]:
                lines.append("FusedSGD against torch.optim.SGD (reported, not gated): device %.2fx, wall %.2fx"
                             % (t["torch_sgd"]["device_us"] / f["device_us"], t["torch_sgd"]["wall_us"] / f["wall_us"]))
        for c in CASES:
            if c_[c]:
                lines.append("device operations of %s: %d  (most frequent: %s)"
                             % (c, c_[c]["device_ops"], "; ".join("%d x %s" % (k, nm[:60]) for nm, k in c_[c]["top"])))
    else:
        lines += ["", "times: still to be taken (no measurement completed)"]
    if failed:
        lines += ["", "STOPPED at the first failure -- %s; everything after it is not measured" % failed]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
