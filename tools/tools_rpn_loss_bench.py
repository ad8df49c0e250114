"""Dev tool: time rpn_glue.rpn_loss (forward + backward) at BASELINE configs[2] shape -- 4 scenes x S80k @ 2 cm through the
default FPN_Net's six maps (brick-major rows), 40 ground-truth walls per scene, bf16 head outputs -- against the reference's
torch composition of RPNLossComputation.__call__ (modeling/rpn/loss_3d.py:201-251: per example nonzero + randperm, cat of
the scales, nonzero of the masks, gathers, smooth L1 + BCE) on the same labels.  Device events around `--iters` calls after
warm-up; the host's enqueue time is the loop's wall time without a synchronise inside.  Writes one JSON line (stdout, and
`--out` if given).  The kernel split and launch count come from a separate `rocprofv3 --kernel-trace --stats` run of this
script with a small --iters."""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import synth_scenes as S  # noqa: E402

DEV = "cuda:0"
PEAK_HBM_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E spec
LABEL_AUG = {"target_Y": 0.4, "anchor_Y": 0.0, "target_Z": 0.8, "anchor_Z": 0.0}
YAWS = (0, -1.57, -0.785, 0.785)
SIZES = [[0.4, 1.5, 1.5], [1.5, 1.5, 1.0], [4, 4, 1.5], [0.2, 0.5, 3], [0.4, 1.5, 3], [0.6, 2.5, 3]]
STRIDES = [[2.0 ** s] * 3 for s in (5, 6, 7)] + [[2.0 ** s] * 3 for s in (4, 5, 6)]


def reference_step(obj, reg, labels, counts, A, B=256, f=0.5, beta=1.0 / 9):
    """loss_3d.py:201-249 as the reference runs it, on plain tensors (cat_scales_obj_reg's regrouping by torch.cat)"""
    nb, n_maps = len(labels), len(obj)
    lab_f = []
    for l in labels:
        m = l[0]
        t = (m >= 0).to(torch.float32)
        t[m == -2] = -1
        lab_f.append(t)
    pos_m, neg_m = [], []
    for t in lab_f:                                             # BalancedPositiveNegativeSampler
        positive = torch.nonzero(t >= 1).squeeze(1)
        negative = torch.nonzero(t == 0).squeeze(1)
        num_pos = min(positive.numel(), int(B * f))
        num_neg = min(negative.numel(), B - num_pos)
        p = positive[torch.randperm(positive.numel(), device=t.device)[:num_pos]]
        n = negative[torch.randperm(negative.numel(), device=t.device)[:num_neg]]
        pm = torch.zeros_like(t, dtype=torch.uint8)
        nm = torch.zeros_like(t, dtype=torch.uint8)
        pm[p] = 1
        nm[n] = 1
        pos_m.append(pm)
        neg_m.append(nm)
    sp = torch.nonzero(torch.cat(pos_m)).squeeze(1)
    sn = torch.nonzero(torch.cat(neg_m)).squeeze(1)
    lab = torch.cat(lab_f)
    tgt = torch.cat([l[3] for l in labels])
    o_parts, r_parts, s0 = [], [], [0] * n_maps
    for b in range(nb):
        for m in range(n_maps):
            c = counts[m][b]
            o_parts.append(obj[m][s0[m] * A:(s0[m] + c) * A])
            r_parts.append(reg[m][s0[m] * A:(s0[m] + c) * A])
            s0[m] += c
    o, r = torch.cat(o_parts).float(), torch.cat(r_parts).float()
    sampled = torch.cat([sp, sn])
    d = torch.abs(r[sp] - tgt[sp])
    box = torch.where(d < beta, 0.5 * d ** 2 / beta, d - 0.5 * beta).sum() / sampled.numel()
    objl = F.binary_cross_entropy_with_logits(o[sampled], lab[sampled])
    return objl, box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-reference", action="store_true")
    args = ap.parse_args()
    import rpn_glue
    from test_cabi_and_host import default_fpn
    torch.manual_seed(0)
    net = default_fpn().to(DEV)
    net.set_site_order("brick")
    locs, feats = S.make_batch(4, 80000, 9000, 50)
    with torch.no_grad():
        maps, _ = net([torch.as_tensor(locs).to(DEV), torch.as_tensor(feats).to(DEV)])
    base = [torch.tensor([[0.0, 0.0, 0.0] + list(s) + [y] for y in YAWS], dtype=torch.float32) for s in SIZES]
    A = len(YAWS)
    gts = [torch.as_tensor(S.make_gt_boxes(40, 7000 + i)).to(DEV) for i in range(4)]
    labels = rpn_glue.rpn_label_matches(maps, base, STRIDES, 50.0, gts, LABEL_AUG, 6, regression_targets=True)
    counts = [[int((m.get_spatial_locations()[:, 3] == b).sum()) for b in range(4)] for m in maps]
    g = torch.Generator().manual_seed(1)
    obj = [(torch.randn(sum(c) * A, generator=g) * 2).to(DEV, torch.bfloat16).requires_grad_() for c in counts]
    reg = [(torch.randn(sum(c) * A, 7, generator=g) * 0.3).to(DEV, torch.bfloat16).requires_grad_() for c in counts]
    n_anchor = sum(l[0].numel() for l in labels)
    n_sites = sum(sum(c) for c in counts)
    P = [int((l[0] >= 0).sum()) for l in labels]
    N = [int((l[0] == -1).sum()) for l in labels]

    def ours():
        lo, lb = rpn_glue.rpn_loss(maps, obj, reg, labels, base, seed=3)
        (lo + lb).backward()

    def theirs():
        lo, lb = reference_step(obj, reg, labels, counts, A)
        (lo + lb).backward()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters, (h1 - h0) * 1e6 / args.iters

    dev_us, host_us = timed(ours)
    res = {"tool": "tools_rpn_loss_bench", "shape": "4 x S80k @ 2 cm, 6 maps, A=4, 40 GT per scene, bf16 head outputs",
           "anchors": n_anchor, "sites": n_sites, "positives": P, "negatives": N, "iters": args.iters,
           "rpn_loss_fwd_bwd_device_us": round(dev_us, 2), "rpn_loss_fwd_bwd_host_enqueue_us": round(host_us, 2)}
    # bytes the three selection passes must read: the int64 label of every anchor (the coordinates, 16 B per site, are
    # shared by the A anchors of a site and read once per pass from cache at best)
    by = 3 * (8 * n_anchor + 16 * n_sites)
    res["selection_pass_bytes"] = by
    res["selection_bytes_over_call_time_fraction_of_hbm_peak"] = round(by / (dev_us * 1e-6) / 1e9 / PEAK_HBM_GBS, 4)
    if not args.skip_reference:
        ref_us, ref_host = timed(theirs)
        res.update(reference_torch_fwd_bwd_device_us=round(ref_us, 2), reference_torch_host_us=round(ref_host, 2))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
