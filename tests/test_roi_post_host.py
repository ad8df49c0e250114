"""The ROI box post-processor without a GPU: the restatement (tests/roi_post_ref.py) against torch.kthvalue and against a
brute-force loop written from the reference's filter_results, and the C ABI / Python surface of the feature."""
import os
import re

import numpy as np
import pytest
import torch

import oracle_lib as O
import roi_post_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.mark.parametrize("m,d", [(50, 10), (50, 49), (50, 50), (7, 100), (50, 0), (50, -1), (1, 1), (0, 5)])
def test_cut_equals_kthvalue(m, d):
    """inference.py:153-161: keep = s >= kthvalue(s, M - D + 1) when M > D > 0, everything otherwise"""
    rng = np.random.default_rng(m * 131 + d + 7)
    s = rng.random(m).astype(F)
    keep = R.cut(s, d)
    if m > d > 0:
        t, _ = torch.kthvalue(torch.from_numpy(s), m - d + 1)
        want = (torch.from_numpy(s) >= t.item()).numpy()
        assert (keep == want).all() and keep.sum() == d      # distinct scores: exactly D
    else:
        assert keep.all() and len(keep) == m


def test_cut_keeps_every_tie_at_the_cut():
    """duplicates of the D-th largest score all stay: more than D detections"""
    s = np.array([0.9, 0.5, 0.7, 0.5, 0.2, 0.5, 0.8, 0.1], F)
    keep = R.cut(s, 4)                                        # 4th largest = 0.5, three of them
    t, _ = torch.kthvalue(torch.from_numpy(s), len(s) - 4 + 1)
    assert t.item() == F(0.5)
    assert (keep == (torch.from_numpy(s) >= t.item()).numpy()).all()
    assert keep.sum() == 6 and keep.tolist() == [True, True, True, True, False, True, True, False]


def _brute_force(prob, boxes, score_thresh, nms, aug):
    """filter_results, inference.py:125-141, one scene: threshold, per class gather, the boxlist_nms_3d clamps, the 2000
    best in descending score (equal scores by ascending row), a plain greedy loop over pairwise verdicts (pre-filter matrix
    > 0 and exact polygon IoU >= thresh), the first 500"""
    rows, labels = [], []
    inds_all = prob > F(score_thresh)
    for j in range(1, prob.shape[1]):
        inds = np.nonzero(inds_all[:, j])[0]
        scores_j = prob[inds, j]
        b = boxes[inds, j].copy()
        b[:, 3:5] = np.maximum(b[:, 3:5], F(aug[0]))
        b[:, 5] = np.maximum(b[:, 5], F(aug[1]))
        order = sorted(range(len(inds)), key=lambda i: (-float(scores_j[i]), i))[:2000]
        b = b[order]
        pre = O.boxes_iou_3d(b, b, (0, 0, 0, 0), -1, True)
        dec = O.clip_iou_matrix(b)
        dead = np.zeros(len(order), bool)
        kept = []
        for i in range(len(order)):
            if dead[i]:
                continue
            kept.append(i)
            for k in range(i + 1, len(order)):
                if pre[i, k] > 0 and dec[i, k] >= F(nms):
                    dead[k] = True
        kept = kept[:500]
        rows += [int(inds[order[i]]) for i in kept]
        labels += [j] * len(kept)
    return np.array(rows, np.int64), np.array(labels, np.int64)


def test_stage_b_equals_brute_force_loop():
    rng = np.random.default_rng(3)
    n, c = 300, 4
    props = R.wall_proposals(n, 11, n_gt=12)
    logits = rng.normal(0, 2.0, (n, c)).astype(F)
    logits[40] = logits[17]                                   # equal scores inside the classes
    reg = rng.normal(0, 0.05, (n, 7 * c)).astype(F)
    prob64, boxes = R.stage_a(logits, reg, props)
    prob = prob64.astype(F)
    assert prob[40, 1] == prob[17, 1]
    stats = []
    (rows, labels), = R.stage_b(prob, boxes, [n], 0.05, 0.5, (0.2, 0.2), 0, stats=stats)
    want_rows, want_labels = _brute_force(prob, boxes, 0.05, 0.5, (0.2, 0.2))
    assert rows.tolist() == want_rows.tolist() and labels.tolist() == want_labels.tolist()
    assert sum(stats[0]["candidates"]) > len(rows) > 0        # something was suppressed, something stayed
    # and with the cut
    (rows_d, labels_d), = R.stage_b(prob, boxes, [n], 0.05, 0.5, (0.2, 0.2), 20)
    keep = R.cut(prob[want_rows, want_labels], 20)
    assert rows_d.tolist() == want_rows[keep].tolist() and labels_d.tolist() == want_labels[keep].tolist()
    assert len(rows) > 20 and len(rows_d) == 20


def test_stage_a_class_agnostic_repeats_the_row_box():
    rng = np.random.default_rng(5)
    props = R.wall_proposals(20, 2)
    reg = rng.normal(0, 0.1, (20, 7)).astype(F)
    prob, boxes = R.stage_a(rng.normal(0, 1, (20, 3)).astype(F), reg, props, class_specific=False)
    assert boxes.shape == (20, 3, 7) and (boxes[:, 0] == boxes[:, 2]).all()
    np.testing.assert_allclose(prob.sum(1), 1.0, rtol=1e-12)


def test_header_and_binding_declare_the_roi_post_entries():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    for name in ("aabr_roi_post_scratch_words", "aabr_roi_post_detections"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _hip._SIGS, name
    ver = int(re.search(r"#define AABR_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _hip.ABI_VERSION and ver >= 620
    assert _hip.load().aabr_version() == ver


def test_python_surface_and_corner_coder_refused():
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import PostProcessor, make_roi_box_post_processor
    assert callable(roi_glue.box_detections)
    pp = PostProcessor(0.05, 0.45, nms_aug_thickness=[0.2, 0.2], detections_per_img=200,
                       box_coder=BoxCoder3D(False, (1.0,) * 7), class_specific=False)
    assert (pp.score_thresh, pp.nms, pp.detections_per_img, pp.class_specific) == (0.05, 0.45, 200, False)
    d = PostProcessor()
    assert (d.score_thresh, d.nms, d.nms_aug_thickness, d.detections_per_img, d.class_specific) == (0.05, 0.5, None, 100,
                                                                                                    True)

    class NS(object):
        def __init__(self, **kw):
            self.__dict__.update(kw)

    def cfg(corner):
        heads = NS(USE_FPN=True, BBOX_REG_WEIGHTS=(1.0,) * 7, SCORE_THRESH=0.05, NMS=0.45,
                   NMS_AUG_THICKNESS_Y_Z=[0.2, 0.2], DETECTIONS_PER_IMG=200)
        return NS(MODEL=NS(ROI_HEADS=heads, CORNER_ROI=corner, CLASS_SPECIFIC=False))

    pp = make_roi_box_post_processor(cfg(False))
    assert (pp.nms, pp.detections_per_img, pp.class_specific, pp.nms_aug_thickness) == (0.45, 200, False, [0.2, 0.2])
    with pytest.raises(ValueError):
        make_roi_box_post_processor(cfg(True))

    class Corner(object):
        is_corner_roi = True
    with pytest.raises(ValueError):
        PostProcessor(box_coder=Corner())


def test_argument_validation_without_gpu():
    """shape limits are refused with a message before any device work"""
    import _hip
    lib = _hip.load()

    def call(nb, C, pre_max, post_max=500):
        return lib.aabr_roi_post_detections(None, None, None, nb, None, C, 1, None, 1e4, 0.05, 0.5, 0.0, 0.0, 1, pre_max,
                                            post_max, 100, None, None, None, None, None, None, None, None, None)
    assert call(1, 1, 2000) == -1 and b"C must be" in lib.aabr_last_error()
    assert call(1, 33, 2000) == -1 and b"C must be" in lib.aabr_last_error()
    assert call(17, 7, 2000) == -1 and b"nb must be" in lib.aabr_last_error()
    assert call(0, 7, 2000) == -1 and b"nb must be" in lib.aabr_last_error()
    assert call(4, 7, 2049) == -1 and b"pre_max" in lib.aabr_last_error()
    assert call(4, 7, 2000, 2001) == -1 and b"post_max" in lib.aabr_last_error()
    assert call(4, 7, 2000) == -1 and b"null" in lib.aabr_last_error()
    assert lib.aabr_roi_post_scratch_words(17, 1000, 7, 2000) == -1
    assert lib.aabr_roi_post_scratch_words(4, 1000, 1, 2000) == -1
    assert lib.aabr_roi_post_scratch_words(4, 1000, 7, 2049) == -1
    w = lib.aabr_roi_post_scratch_words(4, 1000, 7, 2000)
    # at least: prob + boxes of 4000 rows, and the suppression words of 24 lists of 1000
    assert w >= 4000 * 7 * 8 + 24 * 1000 * 16 * 2
