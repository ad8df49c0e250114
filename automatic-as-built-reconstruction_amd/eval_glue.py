"""Detection evaluation on the device (csrc/det_eval.hip, aabr_det_eval_match / aabr_det_eval_curves): final detections
and ground truth of a whole data set -> matches, precision / recall curves and per-class AP.  The counterpart of the
reference's eval_detection_suncg (data3d/evaluation/suncg/suncg_eval.py:733-986, use_07_metric=True) without its Python
loops over scenes and classes; the reference-named module data3d/evaluation/suncg/suncg_eval.py calls this one."""
import warnings

import numpy as np
import torch

import _hip
from _hip import check, ptr

# aabr_det_eval_curves' `cls`: 64-bit words of a class's row and the offsets inside it (csrc/det_eval.h kEvalClassWords /
# kEvalWord*, include/aabr_hip.h; tests/test_det_eval_host.py holds the two lists against each other)
CLASS_WORDS = 64
WORD_AP, WORD_TABLE, WORD_TH5, WORD_TH7 = 0, 1, 45, 47          # float64: AP, [11][4] table, [prec, rec] at 0.5 / 0.7
WORD_NPOS, WORD_NDET, WORD_TP, WORD_BEGIN = 56, 57, 58, 59      # int64: ground truth, detections, flagged, first row
WORD_BAD_GT, WORD_BAD_DET = 60, 61                              # int64, class 0's row only: labels outside [0, C)
_AUG_KEYS = ("target_Y", "target_Z", "anchor_Y", "anchor_Z")


def _cat(ts, shape, dtype, dev):
    ts = [t.reshape(shape) for t in ts]
    out = torch.cat(ts) if ts else torch.zeros((0,) + tuple(shape[1:]), dtype=dtype)
    return out.to(device=dev, dtype=dtype).contiguous()


def _offsets(counts, dev):
    """[0, c0, c0 + c1, ...] from list lengths known on the host, uploaded (no device read)"""
    return torch.tensor(np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)).to(dev)


def detection_eval(det_boxes, det_labels, det_scores, gt_boxes, gt_labels, num_classes, iou_thresh=0.5,
                   aug_thickness=None, only_xy=True, debug=None):
    """Lists over S >= 1 scenes of device tensors: det_boxes [n_s, 7] yx_zb, det_labels int64 [n_s], det_scores [n_s],
    gt_boxes [g_s, 7], gt_labels int64 [g_s].  `num_classes` counts the background (2 .. 32).

    Per detection: IoU with the scene's ground truth of its class as `boxlist_iou_3d(gt, pred, aug_thickness,
    criterion=-1, flag='eval')` computes it (`aug_thickness`: dict with target_Y / target_Z / anchor_Y / anchor_Z, the
    ground truth being the target; None: no clamps; `only_xy` defaults to what the reference's DEBUG = 1 forces),
    `pred_iou` = the maximum, `gt_index` = the first maximum's index among the scene's boxes of that class (a NaN wins),
    -1 below `iou_thresh` (strictly) or without such a box; `match` = 1 for the first detection in score order on each
    ground-truth box.  Score order everywhere: descending score, NaN scores last, equal scores by ascending row (of the
    scene, and of the scene-major concatenation for the per-class curves).  Labels outside [0, num_classes) are skipped
    and counted in `bad_labels`.

    Returns the reference's result dict -- `ap` [n], `map`, `rec_prec_score_iou_org` (per class [n_l, 4] float64 rows
    rec, prec, score, iou in score order; None for a class without detections), `recall_precision_score_iou_10steps`
    [n, 11, 4], `pr_score_th5` / `pr_score_th7` (row 0 = mean, then one [prec, rec] row per class >= 1 that has
    detections), n = largest label seen + 1, row 0 of `ap` and of the tables replaced by the mean of the others as the
    reference does -- plus `gt_index` int64, `pred_iou` fp32 and `match` int8 per detection (scene-major, on the device),
    `n_pos` / `n_det` / `n_tp` per class and `bad_labels` = (ground truth, detections).  `pred_for_each_gt` is not built.
    4 library launches and one stable torch sort whatever S; the one host read is at the end.  `debug` (a dict) receives
    `iou`: list of [g_s, n_s] matrices holding the entries of equal label (zeros elsewhere)."""
    lib = _hip.load()
    S = len(det_boxes)
    if not (S == len(det_labels) == len(det_scores) == len(gt_boxes) == len(gt_labels)):
        raise ValueError("the five lists differ in length")
    if S == 0:
        raise ValueError("no scene to evaluate")
    C = int(num_classes)
    if not 2 <= C <= 32:
        raise ValueError("num_classes must be 2 .. 32 (background included), got %d" % C)
    _hip.require_gpu(det_boxes[0])
    dev = det_boxes[0].device
    n_s = [int(b.shape[0]) for b in det_boxes]
    g_s = [int(b.shape[0]) for b in gt_boxes]
    if any(int(l.numel()) != n or int(s.numel()) != n for l, s, n in zip(det_labels, det_scores, n_s)):
        raise ValueError("det_labels / det_scores do not match det_boxes")
    if any(int(l.numel()) != g for l, g in zip(gt_labels, g_s)):
        raise ValueError("gt_labels do not match gt_boxes")
    aug = aug_thickness or {}
    aug = [float(aug.get(k, 0.0)) for k in _AUG_KEYS]
    db = _cat(det_boxes, (-1, 7), torch.float32, dev)
    dl = _cat(det_labels, (-1,), torch.int64, dev)
    ds = _cat(det_scores, (-1,), torch.float32, dev)
    gb = _cat(gt_boxes, (-1, 7), torch.float32, dev)
    gl = _cat(gt_labels, (-1,), torch.int64, dev)
    N, G = sum(n_s), sum(g_s)
    d_begin, g_begin = _offsets(n_s, dev), _offsets(g_s, dev)
    words = int(lib.aabr_det_eval_scratch_words(N, G))
    if words < 0:
        raise _hip.AabrError("detection_eval: more than 2^31 - 1 rows")
    scratch = _hip.workspace("det_eval", words + 2, torch.int32, dev)
    off = (-scratch.data_ptr() // 4) % 2                                  # 8-byte alignment of the first word
    gt_index = torch.empty(N, dtype=torch.int64, device=dev)
    pred_iou = torch.empty(N, dtype=torch.float32, device=dev)
    match = torch.empty(N, dtype=torch.int8, device=dev)
    key = torch.empty(N, dtype=torch.int64, device=dev)
    iou = iou_begin = None
    if debug is not None:
        iou = torch.zeros(sum(n * g for n, g in zip(n_s, g_s)), dtype=torch.float32, device=dev)
        iou_begin = _offsets([n * g for n, g in zip(n_s, g_s)], dev)
    check(lib.aabr_det_eval_match(ptr(db), ptr(dl), ptr(ds), ptr(gb), ptr(gl), S, ptr(d_begin), ptr(g_begin), N, G,
                                  max(n_s), C, float(iou_thresh), _hip.f32x4(aug), int(bool(only_xy)), ptr(gt_index),
                                  ptr(pred_iou), ptr(match), ptr(key), ptr(iou), ptr(iou_begin),
                                  scratch.data_ptr() + 4 * off, _hip.stream()))
    sorted_key, order = torch.sort(key, stable=True)                       # class-major, descending score, ascending row
    out = torch.empty(C * CLASS_WORDS + 4 * N, dtype=torch.int64, device=dev)   # per-class words, then the curve rows
    rows_ptr = out.data_ptr() + 8 * C * CLASS_WORDS
    check(lib.aabr_det_eval_curves(ptr(sorted_key), ptr(order), ptr(match), ptr(pred_iou), ptr(ds), ptr(gl), N, G, C,
                                   rows_ptr if N else None, ptr(out), _hip.stream()))
    if debug is not None:
        mats, o = [], 0
        for n, g in zip(n_s, g_s):
            mats.append(iou[o:o + n * g].view(g, n))
            o += n * g
        debug["iou"] = mats
    host = out.cpu().numpy()                                              # the one read of the stage
    res = summarize(host[:C * CLASS_WORDS].reshape(C, CLASS_WORDS), host[C * CLASS_WORDS:].view(np.float64).reshape(N, 4))
    res.update(gt_index=gt_index, pred_iou=pred_iou, match=match)
    return res


def summarize(cls_words, rows):
    """the host epilogue over aabr_det_eval_curves' output (numpy int64 [C, 64] and float64 [N, 4]): truncation to the
    largest label seen + 1, row 0 := mean of the other rows, map = nanmean(ap) -- the reference's own quirks
    (suncg_eval.py:758-768, 872, 984-985)"""
    cd = cls_words.view(np.float64)
    n_pos, n_det, n_tp, begin = (cls_words[:, w].copy() for w in (WORD_NPOS, WORD_NDET, WORD_TP, WORD_BEGIN))
    seen = np.nonzero((n_pos > 0) | (n_det > 0))[0]
    if seen.size == 0:
        raise ValueError("neither a detection nor a ground-truth box carries a label inside [0, num_classes)")
    n = int(seen.max()) + 1
    ap = cd[:n, WORD_AP].copy()
    steps = cd[:n, WORD_TABLE:WORD_TABLE + 44].reshape(n, 11, 4).copy()
    org = [rows[begin[l]:begin[l] + n_det[l]].copy() if n_det[l] else None for l in range(n)]
    th = {}
    for name, w in (("pr_score_th5", WORD_TH5), ("pr_score_th7", WORD_TH7)):
        t = np.array([[np.nan, np.nan]] + [[cd[l, w], cd[l, w + 1]] for l in range(1, n) if n_det[l]])
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)             # (a data set whose only label is 0: the mean
            t[0, :] = t[1:, :].mean(0)                                    # of nothing, NaN in the reference too)
        th[name] = t
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        steps[0] = steps[1:].mean(0)
        ap[0] = ap[1:].mean()
        m = np.nanmean(ap)
    res = {"ap": ap, "map": m, "rec_prec_score_iou_org": org, "recall_precision_score_iou_10steps": steps,
           "n_pos": n_pos[:n], "n_det": n_det[:n], "n_tp": n_tp[:n],
           "bad_labels": (int(cls_words[0, WORD_BAD_GT]), int(cls_words[0, WORD_BAD_DET]))}
    res.update(th)
    return res


def check_eval_thickness(aug_thickness):
    """boxes_iou_3d(flag='eval') asserts anchor_Y <= 0.3 and target_Y <= 0.3 (utils3d/rotate_nms_3d_torch.py:40-42)"""
    a = aug_thickness or {}
    if float(a.get("anchor_Y", 0.0)) > 0.3 or float(a.get("target_Y", 0.0)) > 0.3:
        raise ValueError("evaluation needs aug_thickness anchor_Y <= 0.3 and target_Y <= 0.3")
    return aug_thickness
