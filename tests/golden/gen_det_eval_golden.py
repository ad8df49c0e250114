"""Generate tests/golden/det_eval_golden.npz by RUNNING the reference's own evaluation
(data3d/evaluation/suncg/suncg_eval.py: calc_detection_suncg_prec_rec, calc_detection_suncg_ap, pr_of_score_threshold,
through eval_detection_suncg with use_07_metric=True) on a small seeded data set.  Build container only (needs
/root/reference); the committed fixture is data only: the inputs and what the reference returned.

The module file is loaded on its own.  What it imports and cannot be imported here is a placeholder: numba / spconv
(gen_iou_golden's decorator-only modules), open3d, skimage, utils3d.bbox3d_ops, utils3d.color_list and the BoxList3D
module, whose BoxList3D is a minimal duck type (bbox3d, size3d, mode, constants, get_field).  boxlist_iou_3d is the
reference's own utils3d.rotate_nms_3d_torch.boxes_iou_3d (thickness clamps per flag, DEBUG = 1 => only_xy) with its CUDA
launch wrapper rotate_iou_gpu_eval replaced by the host pair loop over the reference's devRotateIoUEval +
check_same_boxes, exactly as gen_box_golden.py drives it.  `np.float = float` restores the alias the module uses.

Scores are handed over as float64 arrays holding float32 values: the reference's `np.max(scores) + 0.01` was a float64
sum under the NumPy it ran on (an np.float32 scalar and a Python float), and this keeps it one whatever NumPy runs the
generator; nothing else in the reference's arithmetic depends on the scores' type (every comparison of a float32 value
with 0.5 or 0.7 gives the same answer in float64).

Data set: 6 scenes, C = 4 (labels 1 .. 3; 0 is the background).  Scene 1 has no detections, scene 2 no ground truth;
class 2 has ground truth and no detection anywhere; class 3 has detections and no ground truth; class 1 carries clusters
of several detections on one ground-truth box.  Asserted, so that the reference's open choices (argsort ties, argmax ties,
the float32 threshold comparison) cannot matter: the scores of a class are pairwise distinct; no IoU lies within 1e-4 of
iou_thresh; for no detection with two or more ground-truth boxes of its class are its two largest IoUs within 1e-4 of
each other."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_iou_golden as G  # noqa: E402

REF = "/root/reference"
IOU_THRESH = 0.5
AUG = {"target_Y": 0.3, "target_Z": 0.0, "anchor_Y": 0.3, "anchor_Z": 0.0}
C = 4


class BoxList3D(object):
    """the duck type the evaluation needs of maskrcnn_benchmark.structures.bounding_box_3d.BoxList3D"""

    def __init__(self, bbox3d, size3d=None, mode="yx_zb", examples_idxscope=None, constants=None):
        self.bbox3d = torch.as_tensor(bbox3d)
        self.size3d, self.mode, self.constants = size3d, mode, constants or {}
        self.fields = {}

    def get_field(self, name):
        return self.fields[name]

    def __len__(self):
        return int(self.bbox3d.shape[0])


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference():
    os.environ.setdefault("MPLBACKEND", "Agg")
    np.float = float
    G._install_placeholders()
    for name in ("open3d", "skimage", "skimage.io", "utils3d.color_list", "utils3d.bbox3d_ops"):
        if name not in sys.modules:
            _module(name, COLOR_LIST=[], Bbox3D=None)
    sys.path.insert(0, REF)
    nms_gpu = importlib.import_module("second.core.non_max_suppression.nms_gpu")
    rn3 = importlib.import_module("utils3d.rotate_nms_3d_torch")

    def host_rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        _, iou = G.ref_iou_matrix(nms_gpu, boxes.astype(np.float32), query_boxes.astype(np.float32), criterion)
        return iou

    rn3.rotate_iou_gpu_eval = host_rotate_iou_gpu_eval

    def boxlist_iou_3d(targets, anchors, aug_thickness, criterion, only_xy=False, flag=""):
        return rn3.boxes_iou_3d(targets.bbox3d, anchors.bbox3d, aug_thickness, criterion, only_xy, flag)

    saved = {k: sys.modules.get(k) for k in ("maskrcnn_benchmark.structures.bounding_box_3d",
                                             "maskrcnn_benchmark.structures.boxlist_ops_3d")}
    _module("maskrcnn_benchmark.structures.bounding_box_3d", BoxList3D=BoxList3D, merge_by_corners=None)
    _module("maskrcnn_benchmark.structures.boxlist_ops_3d", boxlist_iou_3d=boxlist_iou_3d)
    spec = importlib.util.spec_from_file_location("ref_suncg_eval",
                                                  os.path.join(REF, "data3d/evaluation/suncg/suncg_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.BoxList3D = BoxList3D
    mod.boxlist_iou_3d = boxlist_iou_3d
    return mod, boxlist_iou_3d


def make_scenes():
    """walls on a coarse grid (no two ground-truth boxes of a scene overlap); detections are ground-truth boxes moved
    at graded sizes, so IoUs spread from ~0.9 down to ~0.2, plus detections of class 3 and, only where their class
    has at most one ground-truth box in the scene, detections far from everything"""
    rng = np.random.default_rng(20)
    F = np.float32

    def wall(i, j):
        yaw = [0.0, np.pi / 2, 0.3, -0.7][(i + j) % 4]
        return np.array([6.0 * i + rng.uniform(-0.5, 0.5), 6.0 * j + rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1),
                         rng.uniform(0.08, 0.25), rng.uniform(2.5, 4.5), rng.uniform(2.4, 2.8), yaw], F)

    def moved(box, keep):
        # the same wall cut to about `keep` of its length and nudged sideways: IoU near `keep`, never 0
        b = box.astype(np.float64).copy()
        b[0:2] += rng.normal(0, 0.01, 2)
        b[4] *= keep * (1.0 + rng.uniform(-0.08, 0.08))
        b[6] += rng.normal(0, 0.004)
        return b.astype(F)

    # per scene: class-1 boxes, class-2 boxes, detections per class-1 box (cluster sizes), far class-1 detections,
    # class-3 detections
    plan = [(4, 2, [3, 3, 1, 0], 0, 2), (2, 1, None, 0, 0), (0, 0, [], 3, 1), (1, 0, [4], 2, 1), (3, 1, [2, 0, 2], 0, 0),
            (5, 2, [1, 2, 0, 3, 1], 0, 3)]
    scenes = []
    for n1, n2, clusters, far, n3 in plan:
        cells = [(i, j) for i in range(4) for j in range(4)]
        rng.shuffle(cells)
        gtb = [wall(*cells.pop()) for _ in range(n1 + n2)]
        gtl = [1] * n1 + [2] * n2
        mix = rng.permutation(len(gtb))
        gtb, gtl = [gtb[k] for k in mix], [gtl[k] for k in mix]
        db, dl = [], []
        if clusters is not None:
            ones = [k for k in range(len(gtb)) if gtl[k] == 1]
            for k, c in zip(ones, clusters):
                for r in range(c):
                    db.append(moved(gtb[k], [0.92, 0.72, 0.4, 0.25][r]))
                    dl.append(1)
            for _ in range(far):
                db.append(wall(*cells.pop()))
                dl.append(1)
            for _ in range(n3):
                db.append(wall(*cells.pop()))
                dl.append(3)
        mix = rng.permutation(len(db))
        db, dl = [db[k] for k in mix], [dl[k] for k in mix]
        scenes.append({"gt_boxes": np.array(gtb, F).reshape(-1, 7), "gt_labels": np.array(gtl, np.int64),
                       "det_boxes": np.array(db, F).reshape(-1, 7), "det_labels": np.array(dl, np.int64)})
    total = sum(len(s["det_labels"]) for s in scenes)
    scores = (rng.permutation(total) + 1).astype(np.float64) / (total + 1)       # pairwise distinct, inside (0, 1)
    o = 0
    for s in scenes:
        n = len(s["det_labels"])
        s["det_scores"] = scores[o:o + n].astype(F)
        o += n
    return scenes


def main():
    mod, boxlist_iou_3d = load_reference()
    scenes = make_scenes()
    S = len(scenes)
    assert S == 6
    alls = np.concatenate([s["det_scores"] for s in scenes])
    alll = np.concatenate([s["det_labels"] for s in scenes])
    for l in range(C):
        v = alls[alll == l]
        assert len(np.unique(v)) == len(v), "scores of class %d are not distinct" % l
    assert any(len(s["det_labels"]) == 0 for s in scenes) and any(len(s["gt_labels"]) == 0 for s in scenes)
    allg = np.concatenate([s["gt_labels"] for s in scenes])
    assert (allg == 2).any() and not (alll == 2).any() and (alll == 3).any() and not (allg == 3).any()
    preds, gts = [], []
    for s in scenes:
        p = BoxList3D(s["det_boxes"])
        p.fields["labels"] = torch.from_numpy(s["det_labels"])
        p.fields["scores"] = torch.from_numpy(s["det_scores"].astype(np.float64))
        g = BoxList3D(s["gt_boxes"])
        g.fields["labels"] = torch.from_numpy(s["gt_labels"])
        preds.append(p), gts.append(g)
        for l in range(1, C):                          # the conditions under which the open choices cannot matter
            dsel, gsel = s["det_labels"] == l, s["gt_labels"] == l
            if dsel.any() and gsel.any():
                iou = boxlist_iou_3d(BoxList3D(s["gt_boxes"][gsel]), BoxList3D(s["det_boxes"][dsel]), AUG, -1,
                                     flag="eval").numpy()
                assert (np.abs(iou - IOU_THRESH) > 1e-4).all(), "an IoU within 1e-4 of the threshold"
                if iou.shape[0] >= 2:
                    top = np.sort(iou, axis=0)[-2:]
                    assert (top[1] - top[0] > 1e-4).all(), "two largest IoUs of a detection within 1e-4"
    metas = types.SimpleNamespace(label_2_class={0: "background", 1: "wall", 2: "door", 3: "window"})
    with np.errstate(invalid="ignore", divide="ignore"):
        res = mod.eval_detection_suncg(preds, gts, IOU_THRESH, metas, use_07_metric=True, eval_aug_thickness=AUG)
    out = {"iou_thresh": np.float64(IOU_THRESH), "aug": np.array([AUG[k] for k in ("target_Y", "target_Z", "anchor_Y",
                                                                                  "anchor_Z")], np.float64),
           "num_classes": np.int64(C), "n_scenes": np.int64(S)}
    for i, s in enumerate(scenes):
        for k, v in s.items():
            out["s%d_%s" % (i, k)] = v
    out["ap"], out["map"] = np.asarray(res["ap"], np.float64), np.float64(res["map"])
    out["steps"] = np.asarray(res["recall_precision_score_iou_10steps"], np.float64)
    out["pr_score_th5"], out["pr_score_th7"] = res["pr_score_th5"], res["pr_score_th7"]
    n = len(res["ap"])
    has = np.zeros(n, np.int64)
    for l, rp in enumerate(res["rec_prec_score_iou_org"]):
        if rp.dtype != object:                         # (a class without detections is a [1, 4] array of None)
            has[l] = 1
            out["org_%d" % l] = np.asarray(rp, np.float64)
    out["has_curve"] = has
    # gt_index and match per detection from the returned pred_for_each_gt: key >= 0 is the ground-truth index inside
    # the scene's boxes of the class, its list is in score order and the first entry is the one flagged 1.  An entry's
    # 'pred_idx' is pred_ids_l[pi] with pi the position in SCORE order but pred_ids_l left in row order
    # (suncg_eval.py:801,841), so it names the pi-th row of the class, not the detection: pi is recovered as its rank
    # and the detection is row order[pi] of the class (scores are distinct, so `order` is not open).
    name_2_label = {v: k for k, v in metas.label_2_class.items()}
    gt_index = [np.full(len(s["det_labels"]), -1, np.int64) for s in scenes]
    match = [np.zeros(len(s["det_labels"]), np.int8) for s in scenes]
    for name, per_scene in res["pred_for_each_gt"].items():
        for bi, d in enumerate(per_scene):
            rows_l = np.nonzero(scenes[bi]["det_labels"] == name_2_label[name])[0]
            order = np.argsort(-scenes[bi]["det_scores"][rows_l].astype(np.float64), kind="stable")
            for key, lst in d.items():
                pis = [int(np.searchsorted(rows_l, e["pred_idx"])) for e in lst]
                assert pis == sorted(pis) and all(rows_l[pi] == e["pred_idx"] for pi, e in zip(pis, lst))
                for r, pi in enumerate(pis):
                    if key >= 0:
                        gt_index[bi][rows_l[order[pi]]] = key
                        match[bi][rows_l[order[pi]]] = r == 0
    for l in range(1, n):                              # the flags must reproduce the reference's own tp counts
        if has[l]:
            sel = alll == l
            sc, m = alls[sel], np.concatenate(match)[sel]
            order = np.argsort(-sc.astype(np.float64), kind="stable")
            tp = np.cumsum(m[order] == 1)
            assert (tp == np.rint(out["org_%d" % l][:, 1] * np.arange(1, len(tp) + 1))).all(), "flags vs prec, class %d" % l
    out["gt_index"], out["match"] = np.concatenate(gt_index), np.concatenate(match)
    np.savez_compressed(os.path.join(HERE, "det_eval_golden.npz"), **out)
    print("wrote det_eval_golden.npz; ap", out["ap"], "map", out["map"], "detections", len(alls), "matches",
          int(out["match"].sum()))
    print(out["steps"][1])


if __name__ == "__main__":
    main()
