"""Dev tool: time the detection evaluation (eval_glue.detection_eval, csrc/det_eval.hip) against the host composition a
user had before it, on the same tensors:
  device  eval_glue.detection_eval: 4 library launches + one sort, one host read
  host    per scene and class utils3d.rotate_nms_3d_torch.boxes_iou_3d(flag='eval') on the device and a read of the matrix,
          then the numpy loops of the restatement (tests/det_eval_ref.py) -- the reference's own structure
Default size: 200 scenes x 100 detections x 50 ground-truth boxes, 7 classes (background included).

Both forms end with their results on the host, so a host clock around a call measures the whole of it.  `--child time`
alternates the forms in `--repeats` windows (`--iters` device calls, one host call) after a warm-up call of each; median
and min .. max over the windows.  The two results are compared first: flags and gt_index exactly, AP and the tables bit for
bit.  The parent starts the child under its own `timeout`.  Writes `--out` (profiles/det_eval_timing.txt)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
AUG = {"target_Y": 0.3, "target_Z": 0.0, "anchor_Y": 0.3, "anchor_Z": 0.0}


def setup(args):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    importlib.import_module("automatic-as-built-reconstruction_amd")
    import numpy as np
    import torch
    import det_eval_ref as R
    import eval_glue
    import roi_post_ref as RP
    from utils3d.rotate_nms_3d_torch import boxes_iou_3d
    rng = np.random.default_rng(0)
    S, n, g, C = args.scenes, args.dets, args.gts, args.classes
    sc = {k: [] for k in ("det_boxes", "det_labels", "det_scores", "gt_boxes", "gt_labels")}
    for s in range(S):
        gt = RP.wall_proposals(g, 1000 + s, n_gt=g).copy()
        det = RP.wall_proposals(n, 5000 + s).copy()
        k = min(n, 2 * g)
        j = np.arange(k) % g
        det[:k] = gt[j] + (rng.normal(0, 1, (k, 7)) * np.array([0.05, 0.05, 0.05, 0.02, 0.5, 0.1, 0.02]) *
                           rng.uniform(0, 1, (k, 1))).astype(np.float32)
        det[:k, 3:6] = np.maximum(det[:k, 3:6], np.float32(0.05))
        gl = rng.integers(1, C, g).astype(np.int64)
        dl = rng.integers(1, C, n).astype(np.int64)
        dl[:k] = gl[j]
        sc["gt_boxes"].append(gt), sc["gt_labels"].append(gl), sc["det_boxes"].append(det.astype(np.float32))
        sc["det_labels"].append(dl), sc["det_scores"].append(rng.random(n).astype(np.float32))
    dev = {k: [torch.as_tensor(v).to(DEV) for v in vs] for k, vs in sc.items()}

    def device():
        return eval_glue.detection_eval(dev["det_boxes"], dev["det_labels"], dev["det_scores"], dev["gt_boxes"],
                                        dev["gt_labels"], C, args.iou_thresh, AUG)

    def host():
        labels = [l.cpu().numpy() for l in dev["det_labels"]]
        scores = [v.cpu().numpy() for v in dev["det_scores"]]
        gt_labels = [l.cpu().numpy() for l in dev["gt_labels"]]

        def iou_fn(s, gt_rows, det_rows):
            t = dev["gt_boxes"][s][torch.as_tensor(gt_rows, device=DEV)]
            a = dev["det_boxes"][s][torch.as_tensor(det_rows, device=DEV)]
            return boxes_iou_3d(t, a, AUG, -1, True, "eval").cpu().numpy()      # only_xy, as the device form
        return R.evaluate(labels, scores, gt_labels, C, args.iou_thresh, iou_fn)
    return torch, R, device, host


def child_time(args):
    torch, R, device, host = setup(args)
    a, b = device(), host()                                    # (warm-up of both forms, and the comparison)
    same = (a["match"].cpu().numpy().tolist() == b["match"].tolist() and
            a["gt_index"].cpu().numpy().tolist() == b["gt_index"].tolist() and
            all(R.same_bits(a[k], b[k]) for k in ("ap", "map", "recall_precision_score_iou_10steps", "pr_score_th5",
                                                  "pr_score_th7")))
    for _ in range(3):
        device()
    ts = {"device": [], "host": []}
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            device()
        ts["device"].append(1e3 * (time.perf_counter() - t0) / args.iters)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        ts["host"].append(1e3 * (time.perf_counter() - t0))
    out = {"same": bool(same), "map": float(a["map"]), "n_tp": int(a["n_tp"].sum()), "n_det": int(a["n_det"].sum())}
    for k, v in ts.items():
        v = sorted(v)
        out[k] = [v[len(v) // 2], v[0], v[-1]]
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=200)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=50)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--iou-thresh", dest="iou_thresh", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--child", choices=("time",))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "det_eval_timing.txt"))
    args = ap.parse_args()
    if args.child == "time":
        return child_time(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "time"]
    for k in ("scenes", "dets", "gts", "classes", "iters", "repeats"):
        cmd += ["--" + k, str(getattr(args, k))]
    cmd += ["--iou-thresh", str(args.iou_thresh)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stdout.write(r.stdout)
        raise SystemExit("the timing child ended with status %d" % r.returncode)
    res = json.loads(line[-1][7:])
    lines = ["detection evaluation: %d scenes x %d detections x %d ground-truth boxes, %d classes, iou_thresh %g; "
             "%d detections, %d flagged, mAP %.4f" % (args.scenes, args.dets, args.gts, args.classes, args.iou_thresh,
                                                      res["n_det"], res["n_tp"], res["map"]),
             "host clock around a whole call, results on the host at its end; median of %d windows (min .. max); device: "
             "%d calls per window, host: 1; the forms alternate in one process after a warm-up call of each"
             % (args.repeats, args.iters),
             "device  eval_glue.detection_eval (4 launches + 1 sort, 1 read)                %10.2f ms (%.2f .. %.2f)"
             % tuple(res["device"]),
             "host    boxes_iou_3d + read per scene and class, numpy loops of the restatement %10.2f ms (%.2f .. %.2f)"
             % tuple(res["host"]),
             "host / device = %.1f" % (res["host"][0] / res["device"][0]),
             "the two results agree (flags and gt_index exactly, AP and tables bit for bit): %s" % res["same"]]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
