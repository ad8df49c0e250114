"""CPU restatement of the ROI box post-processor (PostProcessor.forward / filter_results of the reference,
maskrcnn_benchmark/modeling/roi_heads/box_head_3d/inference.py:44-162) -- TEST INFRASTRUCTURE ONLY.

Built only from what is already pinned: an fp64 softmax, oracle/box_oracle.decode_centroid_box (pinned by
tests/golden/box_golden.npz), oracle_lib.rotate_nms_3d(decision="clip") (the C oracle's matrix as the `> 0` pre-filter
and the exact polygon IoU for the decision), and numpy for the threshold, the ordering rule and the
kthvalue cut.  The reference's own PostProcessor cannot be run for a fixture: it needs BoxList3D and the spconv NMS
loop, which DESIGN section 4 lists as unpinnable -- so the rule for that loop is this project's stated one, and the
rule for equal scores (ascending proposal row; torch.topk leaves it open) is this project's as well.

Two stages, so that a test can compare values with a tolerance (stage A) and decisions exactly (stage B, fed the
implementation's own fp32 prob and boxes)."""
import sys

import numpy as np

import oracle_lib as O

sys.path.insert(0, O.ORACLE_DIR)
import box_oracle as BO  # noqa: E402

F = np.float32
PRE_NMS, POST_NMS = 2000, 500      # boxlist_nms_3d(flag='roi_post') -> rotate_nms_3d(pre_max_size=2000, post_max_size=500)


def stage_a(logits, regression, proposals, weights=(1.0,) * 7, bbox_xform_clip=10000.0, class_specific=True):
    """-> prob64 [N, C] (softmax in fp64 of the fp32 logits), boxes fp32 [N, C, 7] (the decode oracle; one box per row
    repeated over the classes when the regression is not class specific, inference.py:102-104)"""
    x = np.asarray(logits, F).astype(np.float64)
    n, c = x.shape
    if n == 0:
        return x, np.zeros((0, c, 7), F)
    e = np.exp(x - x.max(1, keepdims=True))
    prob = e / e.sum(1, keepdims=True)
    dec = BO.decode_centroid_box(np.asarray(regression, F).reshape(n, -1), np.asarray(proposals, F).reshape(n, 7), weights,
                                 bbox_xform_clip)
    boxes = dec.reshape(n, c, 7) if class_specific else np.repeat(dec.reshape(n, 1, 7), c, 1)
    return prob, boxes.astype(F)


def cut(scores, detections_per_img):
    """inference.py:153-161 -> boolean keep mask: with M > D > 0, score >= the (M - D + 1)-th smallest"""
    s = np.asarray(scores, F)
    m, d = len(s), int(detections_per_img)
    if not (m > d > 0):
        return np.ones(m, bool)
    return s >= np.sort(s, kind="stable")[m - d]


def class_survivors(prob_j, boxes_j, score_thresh, nms, aug):
    """one turn of the loop inference.py:125-141 -> proposal rows of the survivors, in survivor order"""
    cand = np.nonzero(prob_j > F(score_thresh))[0]
    if len(cand) == 0:
        return cand.astype(np.int64), 0
    b = boxes_j[cand].copy()
    b[:, 3:5] = np.maximum(b[:, 3:5], F(aug[0]))          # boxlist_ops_3d.py:42-44
    b[:, 5] = np.maximum(b[:, 5], F(aug[1]))
    # argsort(-scores, stable) inside: descending score, equal scores by ascending position = ascending row
    keep = O.rotate_nms_3d(b, prob_j[cand], PRE_NMS, POST_NMS, nms, only_xy=True, decision="clip")
    return cand[keep].astype(np.int64), len(cand)


def stage_b(prob32, boxes32, n_per_scene, score_thresh=0.05, nms=0.5, nms_aug_thickness=None, detections_per_img=100,
            stats=None):
    """prob32 fp32 [N, C], boxes32 fp32 [N, C, 7], rows scene-major -> per scene (rows, labels), rows scene-local.
    `stats` (a list) receives per scene a dict: candidates / survivors per class, M before the cut."""
    prob = np.asarray(prob32, F)
    boxes = np.asarray(boxes32, F)
    aug = (0.0, 0.0) if nms_aug_thickness is None else nms_aug_thickness
    c = prob.shape[1]
    out, r0 = [], 0
    for n in n_per_scene:
        p, bx = prob[r0:r0 + n], boxes[r0:r0 + n]
        r0 += n
        rows, labels, ncand, nkeep = [], [], [], []
        for j in range(1, c):
            k, nc_ = class_survivors(p[:, j], bx[:, j], score_thresh, nms, aug)
            rows.append(k)
            labels.append(np.full(len(k), j, np.int64))
            ncand.append(nc_)
            nkeep.append(len(k))
        rows, labels = np.concatenate(rows), np.concatenate(labels)
        keep = cut(p[rows, labels], detections_per_img)
        if stats is not None:
            stats.append({"candidates": ncand, "survivors": nkeep, "M": len(rows), "kept": int(keep.sum())})
        out.append((rows[keep], labels[keep]))
    return out


# ---- seeded inputs shared by the host and the GPU tests ------------------------------------------------------------------
def wall_proposals(n, seed, n_gt=30):
    """[n, 7] wall-like boxes (thin, long, yaw in the anchor set +- noise) clustered around n_gt walls"""
    import synth_scenes as S
    return S.make_nms_boxes(n, seed, n_gt=n_gt)[0] if n else np.zeros((0, 7), F)


def separated_proposals(n, pitch=10.0):
    """[n, 7] boxes on a square lattice, far enough apart that nothing overlaps"""
    i = np.arange(n)
    b = np.zeros((n, 7), F)
    b[:, 0] = (i % 32) * pitch
    b[:, 1] = (i // 32) * pitch
    b[:, 3], b[:, 4], b[:, 5] = 0.2, 3.0, 2.5
    return b
