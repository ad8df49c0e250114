"""eval_detection_suncg of the reference (data3d/evaluation/suncg/suncg_eval.py:733-986) on the device: the box lists
of a whole data set go to eval_glue.detection_eval in one call (csrc/det_eval.hip: 4 launches + one sort, one host read)
instead of one IoU launch and one read per scene and class.

Built: the VOC-style match, per-class precision / recall, the 11-point AP, the 11-row table and the precision / recall at
score 0.5 and 0.7, with the reference's quirks (row 0 = mean of the other rows, map = nanmean(ap), arrays cut at the
largest label seen).  Refused with a ValueError: `use_07_metric=False` (the reference never passes it), and
`pred_for_each_gt` / `parse_pred_for_each_gt` with the regression statistics built on them and all drawing are not
here -- the result carries `gt_index`, `pred_iou` and `match` per detection so a caller can build those on the host.
Datasets, result files and their formats stay outside the package."""
import numpy as np

import eval_glue


def _lists(boxlists):
    return [b.bbox3d for b in boxlists], [b.get_field("labels") for b in boxlists]


def eval_detection_suncg(pred_boxlists, gt_boxlists, iou_thresh, dset_metas, use_07_metric=True, eval_aug_thickness=None,
                         score_threshold=0.5, pred_for_each_gt=False, draw=False):
    """pred_boxlists / gt_boxlists: lists over scenes of objects with `.bbox3d` [n, 7] yx_zb device tensors and
    `.get_field("labels")` (and `"scores"` for the predictions) -- DetectionList3D qualifies, so PostProcessor's output
    goes straight in.  `dset_metas` needs `label_2_class` only (its length is the class count, background included).
    `score_threshold` is accepted and unused, as in the reference.  Returns eval_glue.detection_eval's dict."""
    if not use_07_metric:
        raise ValueError("only the 11-point metric (use_07_metric=True) is implemented: the reference passes no other")
    if pred_for_each_gt:
        raise ValueError("pred_for_each_gt and the regression statistics built on it are not implemented; "
                         "the result's gt_index / pred_iou / match arrays carry what they are built from")
    if draw:
        raise ValueError("drawing is not part of this package")
    if len(gt_boxlists) != len(pred_boxlists):
        raise ValueError("%d prediction lists for %d ground-truth lists: one of each per scene is needed"
                         % (len(pred_boxlists), len(gt_boxlists)))
    eval_glue.check_eval_thickness(eval_aug_thickness)
    det_boxes, det_labels = _lists(pred_boxlists)
    gt_boxes, gt_labels = _lists(gt_boxlists)
    det_scores = [b.get_field("scores") for b in pred_boxlists]
    return eval_glue.detection_eval(det_boxes, det_labels, det_scores, gt_boxes, gt_labels, len(dset_metas.label_2_class),
                                    iou_thresh=iou_thresh, aug_thickness=eval_aug_thickness)


def result_str(result, label_2_class):
    """mAP and one AP line per class (class 0's line is the mean the reference stores there)"""
    ap = result["ap"]
    lines = ["mAP: %.4f" % result["map"]]
    for l in range(len(ap)):
        name = "ave" if l == 0 else str(label_2_class[l])
        lines.append("%-16s AP: %s" % (name, "nan" if np.isnan(ap[l]) else "%.4f" % ap[l]))
    return "\n".join(lines) + "\n"


def evaluate_dataset(dataset, predictions, iou_thresh, eval_aug_thickness=None, logger=None):
    """Scores `predictions` (one box list per scene) against the ground truth `dataset` holds for them.  Of the data set
    only `get_groundtruth(data_id)` and `dset_metas.label_2_class` are used; a prediction names its scene through
    `constants["data_id"]` and, where it carries none, counts as the scene at its own position in the list.
    Without a single predicted box, or without a single ground-truth box, there is nothing to score and the answer is
    None.  Otherwise: eval_detection_suncg's dict plus `label_2_class`; the per-class lines go to `logger` if given."""
    if not any(len(p) for p in predictions):
        return None
    ground_truth = []
    for position, p in enumerate(predictions):
        data_id = (getattr(p, "constants", None) or {}).get("data_id", position)
        ground_truth.append(dataset.get_groundtruth(data_id))
    if not any(len(g) for g in ground_truth):
        return None
    names = dataset.dset_metas.label_2_class
    result = eval_detection_suncg(predictions, ground_truth, iou_thresh, dataset.dset_metas,
                                  eval_aug_thickness=eval_aug_thickness)
    result["label_2_class"] = names
    if logger is not None:
        logger.info(result_str(result, names))
    return result
