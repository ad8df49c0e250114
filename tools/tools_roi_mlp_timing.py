"""Dev tool: time the box head's dense layers (roi_glue.box_head_mlp + box_predictions, csrc/roi_mlp.hip) at the
reference's default shape -- 2000 ROIs, C = 128, pooled (5, 11, 4), MLP_HEAD_DIM 512, 3 classes -- forward and
forward + backward, (a) `fused = True`, the library's GEMMs, against (b) `fused = False`, the torch modules themselves
(rocBLAS / MIOpen) on the same tensors and parameters: the yardstick.  The input is a pooled tensor (the pooler has a
tool of its own, tools_roi_pool_bench.py).

Both paths alternate inside one process: `--repeats` windows of `--iters` calls each after `--warmup` calls, device
events around a window that ends in a synchronise; the median and the spread (min .. max) over the windows are reported,
with the achieved TFLOP/s (forward 2 * 58.7 GFLOP of multiply-adds at the default shape, forward + backward three
times that) against the 155 TF fp32 MFMA rate, and the device operations per call counted with torch.profiler in windows
of their own.  Writes the text report to `--out` (profiles/roi_mlp_timing.txt)."""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import torch  # noqa: E402

DEV = "cuda:0"
PEAK_TF = 155.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "roi_mlp_timing.txt"))
    args = ap.parse_args()
    import roi_glue
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    C, res, R, n = 128, (5, 11, 4), 512, args.rois
    hw = res[0] * res[1]
    torch.manual_seed(0)
    cfg = roi_glue.box_head_cfg(C=C, resolution=res, R=R, scales=(0.5, 0.25), track=False)
    ext, pred = make_roi_box_feature_extractor(cfg).to(DEV), make_roi_box_predictor(cfg).to(DEV)
    pooled = torch.randn((n, C) + res, device=DEV, requires_grad=True)
    g_l, g_d = torch.randn((n, 3), device=DEV), torch.randn((n, 21), device=DEV)
    macs = n * hw * C * res[2] * R + n * hw * R * R + n * R * R + n * R * 24
    flop = {"forward": 2.0 * macs, "forward+backward": 6.0 * macs}

    def call(fused, backward):
        ext.fused = pred.fused = fused
        if backward:
            pooled.grad = None
            ext.zero_grad(set_to_none=True)
            pred.zero_grad(set_to_none=True)
            logits, deltas = pred(ext.head(pooled))
            torch.autograd.backward([logits, deltas], [g_l, g_d])
        else:
            with torch.no_grad():
                logits, deltas = pred(ext.head(pooled))
        return logits

    def window(fused, backward):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            call(fused, backward)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def count(fused, backward):
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(fused, backward)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

    lines = ["box head dense layers: %d ROIs, C = %d, pooled %s, R = %d, 3 classes (class specific); fp32" % (n, C, res, R),
             "median of %d windows of %d calls after %d warm-up calls (min .. max); device events" %
             (args.repeats, args.iters, args.warmup)]
    med = {}
    for mode, backward in (("forward", False), ("forward+backward", True)):
        for fused in (True, False):
            for _ in range(args.warmup):
                call(fused, backward)
        ts = {True: [], False: []}
        for _ in range(args.repeats):
            for fused in (True, False):
                ts[fused].append(window(fused, backward))
        for fused in (True, False):
            t = sorted(ts[fused])
            m = t[len(t) // 2]
            med[(mode, fused)] = m
            lines.append("%-17s %-14s %8.3f ms (%.3f .. %.3f)  %6.1f TFLOP/s = %4.1f %% of %.0f TF;  %d device operations per call"
                         % (mode, "fused = True" if fused else "fused = False", m, t[0], t[-1], flop[mode] / m / 1e9,
                            100 * flop[mode] / m / 1e9 / PEAK_TF, PEAK_TF, count(fused, backward)))
    for mode in ("forward", "forward+backward"):
        lines.append("%s: fused / torch composition = %.2f" % (mode, med[(mode, True)] / med[(mode, False)]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
