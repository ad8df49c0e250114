"""Dev tool: time the multi-level ROI pooler, forward + backward, (a) Pooler(fused=True) -- roi_glue.pool_rois,
csrc/roi_pool.hip: one launch for ROI rows and levels, one gather for all levels, one memset + one launch backward --
against (b) Pooler(fused=False), the reference's loop (modeling/poolers_3d.py:126-168): torch expressions for the ROI rows
and levels, then per level nonzero (a host read) + index + ROIAlignRotated3D + indexed write into a zero-filled result,
backward through autograd.  (b) is built only from entry points that existed before the pooler: the yardstick.

Shape: the box head's training shape -- 4 scenes x 500 proposals, C = 128, output (5, 11, 4), sampling 2, `--levels` 2
or 3 feature maps (extents 128x128x16, 64x64x8, 32x32x4 at occupancy 1/6, scales 0.5 / 0.25 / 0.125 over a 256x256x32 box
frame, canonical size 10 / 14 so that every level receives ROIs).
Both paths alternate inside one process: `--repeats` windows of `--iters` calls each after warm-up, device events and the
host clock around a window that ends in a synchronise; the median and the spread (min .. max) over the windows are
reported.  `--count-ops` then counts the device operations (kernels, memsets, copies) of `--count-iters` calls per path
with torch.profiler, in windows of their own.  Writes one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
EXTENTS = ((128, 128, 16), (64, 64, 8), (32, 32, 4))
SCALES = (0.5, 0.25, 0.125)
FRAME = (256, 256, 32)
OUT, SAMPLING, C = (5, 11, 4), 2, 128


class _List(object):
    mode = "yx_zb"

    def __init__(self, bbox3d):
        self.bbox3d = bbox3d


def make_level(rng, ext, nb, occupancy=1.0 / 6):
    import sparseconvnet as scn
    h, w, z = ext
    rows = []
    for b in range(nb):
        m = rng.random((h, w, z)) < occupancy
        m[h - 1, w - 1, z - 1] = True
        yxz = np.argwhere(m)
        rows.append(np.concatenate([yxz, np.full((len(yxz), 1), b)], 1))
    sites = np.concatenate(rows).astype(np.int64)
    feats = rng.standard_normal((len(sites), C)).astype(np.float32)
    x = scn.InputLayer(3, [h, w, z], mode=4)([torch.as_tensor(sites).to(DEV), torch.as_tensor(feats).to(DEV)])
    f = x.features.detach().clone().requires_grad_(True)
    return scn.SparseConvNetTensor(f, x.metadata, x.spatial_size), f


def make_boxes(rng, n, canonical, n_levels):
    """wall-like yx_zb boxes over FRAME; sqrt(longer side) / canonical uniform over the span of the levels' scales"""
    lo, hi = SCALES[n_levels - 1] * 0.6, SCALES[0] * 1.2
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = rng.uniform(0, FRAME[0], n)
    b[:, 1] = rng.uniform(0, FRAME[1], n)
    b[:, 2] = rng.uniform(0, FRAME[2] / 2, n)
    b[:, 4] = (rng.uniform(lo, hi, n) * canonical) ** 2               # the longer side decides the level
    b[:, 3] = rng.uniform(1.0, 6.0, n)
    b[:, 5] = rng.uniform(4.0, FRAME[2] / 2, n)
    b[:, 6] = rng.uniform(-np.pi / 2, np.pi / 2, n)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=2, choices=(1, 2, 3))
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--path", choices=("both", "fused", "loop"), default="both")
    ap.add_argument("--count-ops", action="store_true")
    ap.add_argument("--count-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    nl = args.levels
    canonical = 14.0 if nl == 2 else 10.0
    rng = np.random.default_rng(0)
    xs, fs = zip(*[make_level(rng, EXTENTS[l], args.scenes) for l in range(nl)])
    boxes = [_List(torch.as_tensor(make_boxes(rng, args.rows, canonical, nl)).to(DEV)) for _ in range(args.scenes)]
    n = args.scenes * args.rows
    grad = torch.randn((n, C) + OUT, generator=torch.Generator().manual_seed(1)).to(DEV)
    poolers = {}
    for name, fused in (("fused", True), ("loop", False)):
        poolers[name] = Pooler(OUT, SCALES[:nl], SAMPLING, canonical)
        poolers[name].fused = fused

    def call(name):
        for f in fs:
            f.grad = None
        out = poolers[name](list(xs), boxes)
        out.backward(grad)
        return out

    def window(name):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h0 = time.perf_counter()
        for _ in range(args.iters):
            call(name)
        e1.record()
        torch.cuda.synchronize()
        h1 = time.perf_counter()
        return e0.elapsed_time(e1) * 1e3 / args.iters, (h1 - h0) * 1e6 / args.iters

    names = [p for p in ("fused", "loop") if args.path in ("both", p)]
    import roi_glue
    lv = roi_glue.roi_rows_and_levels([b.bbox3d for b in boxes], SCALES[:nl], canonical)[1]
    res = {"tool": "tools_roi_pool_bench", "levels": nl, "scenes": args.scenes, "rows_per_scene": args.rows, "channels": C,
           "output": list(OUT), "sampling": SAMPLING, "iters": args.iters, "repeats": args.repeats,
           "sites_per_level": [int(f.shape[0]) for f in fs], "rois_per_level": torch.bincount(lv, minlength=nl).tolist()}
    first = {}
    for name in names:
        for _ in range(args.warmup):
            first[name] = call(name).detach()
        first[name + "_grads"] = [f.grad.clone() for f in fs]
    if len(names) == 2:
        res["same_forward"] = bool(torch.equal(first["fused"], first["loop"]))
        res["max_grad_diff"] = max(float((a - b).abs().max()) for a, b in zip(first["fused_grads"], first["loop_grads"]))
    times = {name: [] for name in names}
    for _ in range(args.repeats):                                     # alternate the two paths window by window
        for name in names:
            times[name].append(window(name))
    for name in names:
        dev = sorted(t[0] for t in times[name])
        host = sorted(t[1] for t in times[name])
        res[name + "_device_us"] = {"median": round(dev[len(dev) // 2], 1), "min": round(dev[0], 1), "max": round(dev[-1], 1)}
        res[name + "_host_us"] = {"median": round(host[len(host) // 2], 1), "min": round(host[0], 1),
                                  "max": round(host[-1], 1)}
    if args.count_ops:
        from torch.profiler import ProfilerActivity, profile
        for name in names:
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(args.count_iters):
                    call(name)
                torch.cuda.synchronize()
            kernels, copies, kinds = 0, 0, {}
            for e in prof.events():
                if e.device_type != torch.autograd.DeviceType.CUDA:
                    continue
                low = e.name.lower()
                if "memcpy" in low or "copybuffer" in low:
                    copies += 1
                else:
                    kernels += 1
                short = e.name.split("(")[0].split("<")[0][-60:]
                kinds[short] = kinds.get(short, 0) + 1
            res[name + "_device_ops_per_call"] = {"kernels_and_memsets": round(kernels / args.count_iters, 2),
                                                  "copies": round(copies / args.count_iters, 2)}
            res[name + "_op_kinds_per_call"] = {k: round(v / args.count_iters, 2) for k, v in sorted(kinds.items())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fo_:
            fo_.write(line + "\n")


if __name__ == "__main__":
    main()
