"""CPU restatement of the separated-classifier groups of the box head (MODEL.SEPARATE_CLASSES; the reference's
maskrcnn_benchmark/modeling/seperate_classifier.py; csrc/sep_groups.h, the grouped entry points of csrc/roi_loss.hip and
csrc/roi_post.hip) in numpy -- TEST INFRASTRUCTURE ONLY.

Written from the rule, not from the implementation: the group tables, the per-group filter of a scene's ground truth,
and the grouped stages as compositions over the single-group restatements that are already pinned (roi_loss_ref,
roi_post_ref): a group is run on its gathered rows and columns exactly as the reference loops over groups."""
import numpy as np

import roi_post_ref as RP

F = np.float32


def group_tables(seperate_classes, num_input_classes):
    """-> dict: grouped_classes, class_nums, C_tot, org_to_sep {original label: (group, group-local id)}.  Group 0: every
    class not named, ascending (background 0 included); group g >= 1: its own background column num_input_classes + g - 1,
    then the named classes ascending."""
    sep = [sorted(int(c) for c in g) for g in seperate_classes]
    named = set(c for g in sep for c in g)
    assert 0 not in named
    grouped = [[c for c in range(num_input_classes) if c not in named]]
    for g, s in enumerate(sep):
        grouped.append([num_input_classes + g] + s)
    org_to_sep = {}
    for g, gc in enumerate(grouped):
        for i, c in enumerate(gc):
            org_to_sep[c] = (g, i)
    return {"grouped_classes": grouped, "class_nums": [len(g) for g in grouped],
            "C_tot": num_input_classes + len(grouped) - 1, "org_to_sep": org_to_sep}


def filter_gt(labels, grouped_classes, g):
    """a scene's ground-truth labels (original) -> (rows of the boxes of group g, their group-local labels), ordered by
    (group-local label ascending, row ascending): per class of the group in turn, the rows that carry it"""
    labels = np.asarray(labels, np.int64)
    rows, local = [], []
    for i, c in enumerate(grouped_classes[g]):
        r = np.nonzero(labels == c)[0]
        rows.append(r)
        local.append(np.full(len(r), i, np.int64))
    return np.concatenate(rows).astype(np.int64), np.concatenate(local)


def stage_b_grouped(prob32, boxes32, sep_id, n_per_scene, grouped_classes, score_thresh=0.05, nms=0.5,
                    nms_aug_thickness=None, detections_per_img=100, stats=None):
    """prob32 fp32 [N, C_tot], boxes32 fp32 [N, 7] (class agnostic), sep_id [N], rows scene-major -> per scene
    (rows, labels): for every group in ascending order roi_post_ref.stage_b on the group's rows of the scene and the
    group's columns (so: threshold, NMS per column, the detections_per_img cut per (scene, group)), the rows mapped back
    to the scene, the labels to the original ids.  `stats` receives per scene the list of the groups' stage_b stats."""
    prob, boxes, sep_id = np.asarray(prob32, F), np.asarray(boxes32, F), np.asarray(sep_id, np.int64)
    out, r0 = [], 0
    for n in n_per_scene:
        rows_s, labels_s, st_s = [], [], []
        for g, cols in enumerate(grouped_classes):
            idx = np.nonzero(sep_id[r0:r0 + n] == g)[0]
            pg = np.ascontiguousarray(prob[r0 + idx][:, cols])
            bg = np.repeat(boxes[r0 + idx].reshape(-1, 1, 7), len(cols), 1)
            st = []
            (rows, labels), = RP.stage_b(pg, bg, [len(idx)], score_thresh, nms, nms_aug_thickness, detections_per_img, stats=st)
            rows_s.append(idx[rows])
            labels_s.append(np.asarray(cols, np.int64)[labels])
            st_s.append(st[0])
        out.append((np.concatenate(rows_s).astype(np.int64), np.concatenate(labels_s).astype(np.int64)))
        if stats is not None:
            stats.append(st_s)
        r0 += n
    return out
