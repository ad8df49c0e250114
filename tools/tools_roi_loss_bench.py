"""Dev tool: time the box head's loss on the device, (a) roi_glue.box_head_targets + roi_glue.box_head_loss forward and
backward (csrc/roi_loss.hip) against (b) the same result composed from the entry points that existed before it, looped the
way FastRCNNLossComputation loops (box_head_3d/loss.py:189-293, 295-382): per scene boxlist_iou_3d + torch.max + the
threshold masks + BoxCoder3D.encode + BalancedPositiveNegativeSampler + nonzero, then F.cross_entropy + the map_inds
gather + smooth_l1_loss, backward through autograd.  (b) is the yardstick.

Shape: 4 scenes x (1000 proposals + G appended ground-truth boxes), G = 50, `--classes C` (4 and 7), fp32,
class-specific regression, FG = BG = 0.5, LABEL_AUG_THICKNESS 0.3 / 0.3, 500 per scene at 0.25 positive.
Both paths alternate inside one process: `--repeats` windows of `--iters` calls each after warm-up, device events and
the host clock around a window that ends in a synchronise; the median and the spread (min .. max) over the windows are
reported.  Writes one JSON line.  Device operations per call come from a separate
`rocprofv3 --kernel-trace --stats` run with `--path fused` / `--path composed` and `--repeats 1`."""
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
import torch.nn.functional as F  # noqa: E402

import synth_scenes as S  # noqa: E402

DEV = "cuda:0"
AUG = {"target_Y": 0.3, "target_Z": 0.3, "anchor_Y": 0.3, "anchor_Z": 0.3}
FG = BG = 0.5
B, FRAC, BETA = 500, 0.25, 1.0 / 5
W = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0)


def make_inputs(nb, n, g, c, seed=0):
    rng = np.random.default_rng(seed)
    props, gts, tls = [], [], []
    for b in range(nb):
        p = S.make_nms_boxes(n, 50 + b, n_gt=30)[0]
        t = (p[rng.choice(n, g, replace=False)] + rng.normal(0, 0.03, (g, 7))).astype(np.float32)
        props.append(np.concatenate([p, t]).astype(np.float32))      # ADD_GT_PROPOSALS
        gts.append(t)
        tls.append(rng.integers(1, c, g).astype(np.int64))
    return props, gts, tls


class _List(object):
    mode = "yx_zb"

    def __init__(self, bbox3d):
        self.bbox3d = bbox3d


def composed_targets(props, gts, tls, coder, sampler):
    from maskrcnn_benchmark.structures.boxlist_ops_3d import boxlist_iou_3d
    labels, regt = [], []
    for p, t, tl in zip(props, gts, tls):
        iou = boxlist_iou_3d(_List(t), _List(p), AUG, -1, flag="roi_label_generation")
        vals, idx = iou.max(dim=0)
        idx = idx.clone()
        idx[vals < BG] = -1
        idx[(vals >= BG) & (vals < FG)] = -2
        lab = tl[idx.clamp(min=0)].clone()
        lab[idx == -1] = 0
        lab[idx == -2] = -1
        labels.append(lab)
        regt.append(coder.encode(t[idx.clamp(min=0)], p))
    pos, neg = sampler(labels)
    out = []
    for p, lab, rt, pm, nm in zip(props, labels, regt, pos, neg):
        rows = torch.nonzero(pm | nm).squeeze(1)                      # a host read per scene
        out.append((rows, p[rows], lab[rows], rt[rows]))
    return out


def composed_loss(logits, reg, labels, regt):
    cls = F.cross_entropy(logits, labels)
    pos = torch.nonzero(labels > 0).squeeze(1)
    lp = labels[pos]
    map_inds = 7 * lp[:, None] + torch.arange(7, device=logits.device)
    d = torch.abs(reg[pos[:, None], map_inds] - regt[pos])
    box = torch.where(d < BETA, 0.5 * d * d / BETA, d - 0.5 * BETA).sum() / labels.numel()
    return cls, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--gt", type=int, default=50)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--path", choices=("both", "fused", "composed"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import roi_glue
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    c = args.classes
    props, gts, tls = make_inputs(args.scenes, args.rows, args.gt, c)
    tp = [torch.as_tensor(p).to(DEV) for p in props]
    tg = [torch.as_tensor(g).to(DEV) for g in gts]
    tl = [torch.as_tensor(l).to(DEV) for l in tls]
    coder = BoxCoder3D(False, W)
    sampler = BalancedPositiveNegativeSampler(B, FRAC)
    sampler.seed = 3
    ns = args.scenes * B
    gen = torch.Generator().manual_seed(1)
    logits = torch.randn(ns, c, generator=gen).to(DEV).requires_grad_()
    reg = (torch.randn(ns, 7 * c, generator=gen) * 0.3).to(DEV).requires_grad_()

    def fused():
        out = roi_glue.box_head_targets(tp, tg, tl, FG, BG, AUG, B, FRAC, W, 3)
        labels = torch.cat([o["labels"] for o in out])
        regt = torch.cat([o["regression_targets"] for o in out])
        logits.grad = reg.grad = None
        cls, box = roi_glue.box_head_loss(logits[:labels.numel()], reg[:labels.numel()], labels, regt, True)
        (cls + box).backward()
        return out, cls, box

    def composed():
        out = composed_targets(tp, tg, tl, coder, sampler)
        labels = torch.cat([o[2] for o in out])
        regt = torch.cat([o[3] for o in out])
        logits.grad = reg.grad = None
        cls, box = composed_loss(logits[:labels.numel()], reg[:labels.numel()], labels, regt)
        (cls + box).backward()
        return out, cls, box

    def window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        h1 = time.perf_counter()
        return e0.elapsed_time(e1) * 1e3 / args.iters, (h1 - h0) * 1e6 / args.iters

    paths = [("fused", fused), ("composed", composed)]
    paths = [p for p in paths if args.path in ("both", p[0])]
    res = {"tool": "tools_roi_loss_bench", "scenes": args.scenes, "rows_per_scene": args.rows + args.gt, "gt": args.gt,
           "classes": c, "iters": args.iters, "repeats": args.repeats}
    first = {}
    for name, fn in paths:
        for _ in range(args.warmup):
            first[name] = fn()
    if len(first) == 2:
        (fo, fc, fb), (co, cc, cb) = first["fused"], first["composed"]
        res["same_sample"] = bool(all(torch.equal(a["rows"], b[0]) and torch.equal(a["labels"], b[2]) and
                                      torch.equal(a["regression_targets"], b[3]) for a, b in zip(fo, co)))
        res["loss_fused"], res["loss_composed"] = [fc.item(), fb.item()], [cc.item(), cb.item()]
    times = {name: [] for name, _ in paths}
    for _ in range(args.repeats):                                     # alternate the two paths window by window
        for name, fn in paths:
            times[name].append(window(fn))
    for name, _ in paths:
        dev = sorted(t[0] for t in times[name])
        host = sorted(t[1] for t in times[name])
        res[name + "_device_us"] = {"median": round(dev[len(dev) // 2], 1), "min": round(dev[0], 1), "max": round(dev[-1], 1)}
        res[name + "_host_us"] = {"median": round(host[len(host) // 2], 1), "min": round(host[0], 1),
                                  "max": round(host[-1], 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fo_:
            fo_.write(line + "\n")


if __name__ == "__main__":
    main()
