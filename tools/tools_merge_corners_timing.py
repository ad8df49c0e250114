"""Dev tool: time merging wall detections by their corners (csrc/merge_corners.hip, roi_glue.merge_by_corners: one launch
for all scenes) against a plain torch composition of the same definition on the device -- the reference's form
(maskrcnn_benchmark/structures/bounding_box_3d.py:843-923) in this project's own words: per scene a Python loop over the
2W corners, each iteration a distance row, two masks, two host reads and, where corners meet, a gathered mean.

Shape: `--scenes` scenes of `--dets` detections, half of them walls (a grid of rooms: L, T and cross joints), the others
boxes of another label; default 4 x 100.  Both sides alternate inside one process: `--repeats` windows of `--iters` calls
after `--warmup` calls, device events around a window that ends in a synchronise; median (min .. max) over the windows.
The two sides are checked against each other before anything is timed (same merged corners, boxes within 1e-4).  Writes the
text report to `--out` (profiles/merge_corners_timing.txt)."""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def make_scene(rng, dets):
    """dets // 2 walls: the south and west walls of a grid of 4 m rooms, thickness 0.08, jittered by 3 mm; the rest far
    boxes of label 2; rows shuffled"""
    n_w = dets // 2
    walls, g = [], int(np.ceil(np.sqrt(n_w / 2.0)))
    for i in range(g):
        for j in range(g):
            walls.append([4.0 * i + 2.0, 4.0 * j, 0.0, 0.08, 4.0, 2.5, -np.pi / 2])
            walls.append([4.0 * i, 4.0 * j + 2.0, 0.0, 0.08, 4.0, 2.5, 0.0])
    walls = np.array(walls[:n_w])
    walls[:, 0:2] += rng.uniform(-0.003, 0.003, (n_w, 2))
    others = rng.uniform(-5, 5, (dets - n_w, 7))
    others[:, 0:2] += 100.0
    others[:, 3:6] = np.abs(others[:, 3:6]) + 0.1
    boxes = np.concatenate([walls, others]).astype(np.float32)
    labels = np.array([1] * n_w + [2] * (dets - n_w), np.int64)
    order = rng.permutation(dets)
    return boxes[order], labels[order]


def torch_merge(boxes, labels, threshold):
    """one scene -> (boxes out, merged flags per wall corner)"""
    from utils3d.bbox3d_ops_torch import Box3D_Torch
    wall_ids = torch.nonzero(labels == 1).squeeze(1)
    c = Box3D_Torch.from_yxzb_to_2corners(boxes[wall_ids])
    p = torch.stack([c[:, [0, 1, 5]], c[:, [2, 3, 5]]], 1)
    off = p.mean(1, keepdim=True) - p
    top = (p + off / off.norm(dim=2, keepdim=True) * c[:, 6].view(-1, 1, 1) * 0.5).reshape(-1, 3)
    n = top.shape[0]
    flags = torch.zeros(n, dtype=torch.int32, device=boxes.device)
    for i in range(n):
        near = (top[i:i + 1] - top).norm(dim=1) < threshold
        near[i ^ 1] = False
        ids = torch.nonzero(near).squeeze(1)
        if bool((near[0::2] & near[1::2]).any()):
            continue
        if ids.numel() > 1:
            top[ids] = top[ids].mean(0, keepdim=True)
            flags[ids] = 1
    t = top.view(-1, 2, 3)
    off = t - t.mean(1, keepdim=True)
    t = t + off / off.norm(dim=2, keepdim=True) * c[:, 6].view(-1, 1, 1) * 0.5
    c2 = c.clone()
    c2[:, 0:2], c2[:, 2:4] = t[:, 0, 0:2], t[:, 1, 0:2]
    c2[:, 5] = t[:, :, 2].mean(1)
    c2[:, 4] = c[:, 4].mean()
    out = boxes.clone()
    out[wall_ids] = Box3D_Torch.from_2corners_to_yxzb(c2)
    return out, flags.view(-1, 2), wall_ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "merge_corners_timing.txt"))
    args = ap.parse_args()
    import roi_glue
    rng = np.random.default_rng(args.scenes * 1000 + args.dets)
    scenes = [make_scene(rng, args.dets) for _ in range(args.scenes)]
    boxes = [torch.as_tensor(b).to(DEV) for b, _ in scenes]
    labels = [torch.as_tensor(l).to(DEV) for _, l in scenes]

    def hip():
        return roi_glue.merge_by_corners(boxes, labels, threshold=0.1, return_merged=True)

    def composed():
        return [torch_merge(b, l, 0.1) for b, l in zip(boxes, labels)]

    outs, merged = hip()
    n_merged = 0
    for o, m, (ro, rm, ids) in zip(outs, merged, composed()):                    # the two sides agree
        assert torch.equal(m[ids], rm) and int(m.sum()) == int(rm.sum())
        assert float((o - ro).abs().max()) < 1e-4
        n_merged += int(rm.sum())

    def window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    fns = {"hip": hip, "torch": composed}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn))
    ts = {k: sorted(v) for k, v in ts.items()}
    med = {k: v[len(v) // 2] for k, v in ts.items()}
    fmt = lambda k: "%9.3f ms (%.3f .. %.3f)" % (med[k], ts[k][0], ts[k][-1])
    lines = ["merging walls by their corners: csrc/merge_corners.hip against a plain torch composition of the same definition "
             "on the device; fp32",
             "median of %d windows of %d calls after %d warm-up calls (min .. max); device events around windows that end in "
             "a synchronise" % (args.repeats, args.iters, args.warmup),
             "",
             "%d scenes x %d detections, %d walls each (%d corners per scene, %d merged corners in all)"
             % (args.scenes, args.dets, args.dets // 2, 2 * (args.dets // 2), n_merged),
             "  roi_glue.merge_by_corners, one call for all scenes (cat, offsets upload, 1 launch)  " + fmt("hip"),
             "  torch composition, a Python loop per scene (two host reads per corner)              " + fmt("torch"),
             "  torch / device = %.0f" % (med["torch"] / med["hip"])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
