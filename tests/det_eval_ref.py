"""numpy restatement of the detection evaluation (eval_glue.detection_eval, csrc/det_eval.hip), written from its stated
semantics -- the VOC-style evaluation of the reference (data3d/evaluation/suncg/suncg_eval.py:733-986, 11-point metric):

  per scene and class: IoU matrix [ground truth of the class, detections of the class] from `iou_fn`; per detection
  the first maximum (np.argmax: a NaN wins) and its value; gt_index -1 where the value < float32(iou_thresh);
  detections visited in score order, the first on each ground-truth box is flagged 1, all others 0;
  per class over all scenes: score order, tp / fp running counts, prec = tp / (tp + fp), rec = tp / n_pos in float64,
  the 11 rows [t, p, s, iou] over t = 0.0 + 0.1 i with AP = sum of p / 11, and [prec[k], rec[k]] at
  k = count(score > th) - 1 for th = 0.5 and 0.7 (k = -1 indexes the last element);
  epilogue: arrays cut at the largest label seen + 1, row 0 := mean of the other rows, map = nanmean(ap).

Score order: descending score, NaN scores last, equal scores by ascending row (of the scene for the flags, of the
scene-major concatenation for the curves).  Scores enter the float64 tables as float64 values, so `max + 0.01` is a
float64 sum -- what the reference's NumPy formed from an np.float32 scalar and a Python float.

`iou_fn(scene, gt_rows, det_rows)` returns the float32 matrix [len(gt_rows), len(det_rows)] of that scene's rows; the two
factories below build it from the C oracle or from matrices recorded elsewhere (the device's own), so the decisions can be
checked exactly while the values are checked at a tolerance."""
import os
import warnings

import numpy as np


def score_order(scores):
    """positions in descending score, NaN last, equal scores by ascending position (-0.0 == +0.0)"""
    s = np.asarray(scores, np.float64)
    return np.array(sorted(range(len(s)), key=lambda i: (1, 0.0, i) if np.isnan(s[i]) else (0, -s[i], i)), np.int64)


def oracle_iou(gt_boxes, det_boxes, aug=(0, 0, 0, 0), only_xy=True):
    import oracle_lib as O

    def fn(s, gt_rows, det_rows):
        return O.boxes_iou_3d(gt_boxes[s][gt_rows], det_boxes[s][det_rows], aug, -1, only_xy)
    return fn


def matrix_iou(mats):
    """mats[s]: [g_s, n_s] float32 with at least the entries of equal label filled in"""
    def fn(s, gt_rows, det_rows):
        return np.asarray(mats[s], np.float32)[np.ix_(gt_rows, det_rows)]
    return fn


def match_scenes(det_labels, det_scores, gt_labels, C, iou_thresh, iou_fn):
    """per-detection gt_index int64, pred_iou float32 and match int8 (scene-major concatenations) and n_pos [C]"""
    gi_all, iou_all, m_all = [], [], []
    n_pos = np.zeros(C, np.int64)
    th = np.float32(iou_thresh)
    for s, (dl, sc, gl) in enumerate(zip(det_labels, det_scores, gt_labels)):
        dl, gl = np.asarray(dl, np.int64), np.asarray(gl, np.int64)
        n = len(dl)
        gi, pi, m = np.full(n, -1, np.int64), np.zeros(n, np.float32), np.zeros(n, np.int8)
        for l in range(C):
            det_rows, gt_rows = np.nonzero(dl == l)[0], np.nonzero(gl == l)[0]
            n_pos[l] += len(gt_rows)
            if len(det_rows) == 0 or len(gt_rows) == 0:
                continue
            M = np.asarray(iou_fn(s, gt_rows, det_rows), np.float32)
            first = M.argmax(axis=0)
            val = M[first, np.arange(len(det_rows))]
            with np.errstate(invalid="ignore"):
                first[val < th] = -1
            gi[det_rows], pi[det_rows] = first, val
            taken = set()
            for j in score_order(np.asarray(sc)[det_rows]):
                if first[j] >= 0 and first[j] not in taken:
                    taken.add(int(first[j]))
                    m[det_rows[j]] = 1
        gi_all.append(gi), iou_all.append(pi), m_all.append(m)
    return np.concatenate(gi_all), np.concatenate(iou_all), np.concatenate(m_all), n_pos


def class_curve(scores, match, pred_iou, n_pos):
    """one class: scores float32, match, pred_iou in the scene-major concatenation -> dict (None without detections)"""
    if len(scores) == 0:
        return None
    order = score_order(scores)
    sc = np.asarray(scores, np.float32)[order].astype(np.float64)
    mt = np.asarray(match)[order]
    iou = np.asarray(pred_iou, np.float32)[order].astype(np.float64)
    tp, fp = np.cumsum(mt == 1), np.cumsum(mt == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = tp / (fp + tp)
        rec = tp / int(n_pos)
        ap, rows = 0.0, []
        for i in range(11):
            t = 0.0 + i * 0.1
            ge, le = rec >= t, rec <= t
            p = np.max(np.nan_to_num(prec)[ge]) if ge.any() else 0.0
            u = np.max(np.nan_to_num(iou)[ge]) if ge.any() else 0.0
            s = np.min(sc[le]) if le.any() else np.max(sc) + 0.01
            ap += p / 11
            rows.append([t, p, s, u])
        picks = []
        for th in (0.5, 0.7):
            k = int(np.sum(sc > th)) - 1
            picks.append([prec[k], rec[k]])
    return {"prec": prec, "rec": rec, "scores": sc, "iou": iou, "ap": ap, "steps": np.array(rows, np.float64),
            "th5": picks[0], "th7": picks[1], "tp": int(tp[-1])}


def evaluate(det_labels, det_scores, gt_labels, C, iou_thresh, iou_fn):
    gt_index, pred_iou, match, n_pos = match_scenes(det_labels, det_scores, gt_labels, C, iou_thresh, iou_fn)
    labels = np.concatenate([np.asarray(l, np.int64) for l in det_labels])
    scores = np.concatenate([np.asarray(s, np.float32) for s in det_scores])
    curves = []
    for l in range(C):
        sel = labels == l
        curves.append(class_curve(scores[sel], match[sel], pred_iou[sel], n_pos[l]))
    seen = [l for l in range(C) if n_pos[l] > 0 or curves[l] is not None]
    if not seen:
        raise ValueError("no label inside [0, C)")
    n = max(seen) + 1
    ap = np.array([np.nan if curves[l] is None else curves[l]["ap"] for l in range(n)], np.float64)
    steps = np.full((n, 11, 4), np.nan, np.float64)
    for l in range(n):
        if curves[l] is not None:
            steps[l] = curves[l]["steps"]
    out = {}
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name in ("th5", "th7"):
            t = np.array([[np.nan, np.nan]] + [curves[l][name] for l in range(1, n) if curves[l] is not None], np.float64)
            t[0, :] = t[1:, :].mean(0)
            out["pr_score_" + name] = t
        steps[0] = steps[1:].mean(0)
        ap[0] = ap[1:].mean()
        out["map"] = np.nanmean(ap)
    out.update(ap=ap, recall_precision_score_iou_10steps=steps, gt_index=gt_index, pred_iou=pred_iou, match=match,
               n_pos=n_pos[:n], n_det=np.array([0 if c is None else len(c["prec"]) for c in curves[:n]], np.int64),
               n_tp=np.array([0 if c is None else c["tp"] for c in curves[:n]], np.int64),
               rec_prec_score_iou_org=[None if c is None else np.stack([c["rec"], c["prec"], c["scores"], c["iou"]], 1)
                                       for c in curves[:n]])
    return out


def same_bits(a, b):
    """float64 arrays equal bit for bit, every NaN counting as one value"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the recorded run of the reference's own evaluation (tests/golden/gen_det_eval_golden.py) ------------------------------
def load_golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_eval_golden.npz"))
    S = int(g["n_scenes"])
    scenes = {k: [g["s%d_%s" % (i, k)] for i in range(S)]
              for k in ("det_boxes", "det_labels", "det_scores", "gt_boxes", "gt_labels")}
    return g, scenes


def check_against_golden(res, g):
    """`res`: a result dict in the reference's layout (restatement or device)"""
    assert same_bits(res["ap"], g["ap"]) and same_bits(res["map"], g["map"])
    assert same_bits(res["recall_precision_score_iou_10steps"], g["steps"])
    assert same_bits(res["pr_score_th5"], g["pr_score_th5"]) and same_bits(res["pr_score_th7"], g["pr_score_th7"])
    assert len(res["rec_prec_score_iou_org"]) == len(g["has_curve"])
    for l, has in enumerate(g["has_curve"]):
        got = res["rec_prec_score_iou_org"][l]
        if not has:
            assert got is None
            continue
        want = g["org_%d" % l]
        assert same_bits(got[:, :3], want[:, :3]), "class %d: rec / prec / score" % l
