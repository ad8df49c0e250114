"""The ROI box post-processor on the device (csrc/roi_post.hip, roi_glue.box_detections, PostProcessor) against the CPU
restatement tests/roi_post_ref.py.  The comparison is split so that no tolerance touches a discrete decision:

Stage A, values.  `prob` against an fp64 softmax within a per-element bound derived from the kernel's operation
sequence (u = 2^-24, fp32 round to nearest; x the fp32 logits, m their maximum, d_k = x_k - m <= 0):
  * the subtraction is one rounding: the argument of expf is d_k (1 + e), |e| <= u, which moves exp by a relative
    |d_k| u (exp(d e) - 1 ~ d e);
  * expf returns within 1 ulp (the bound HIP's math API documents for expf), and 1 ulp <= 2^-23 = 2 u relative:
    each term carries theta_k with |theta_k| <= (|d_k| + 2) u;
  * the sum runs in class order with C - 1 additions of positive terms: relative (C - 1) u on top of the terms' own
    errors, of which the largest is at most (max_k |d_k| + 2) u;
  * one correctly rounded division: u.
  Together |prob - prob64| <= prob64 (|d_c| + max_k |d_k| + C + 4) u, taken times 1.01 for the second-order terms, plus
  2^-126 for results in the subnormal range (flushed or short of bits).  Nothing in it comes from a device run.
`boxes` against oracle/box_oracle.decode_centroid_box at the tolerance test_box_coder_encode_decode_vs_reference_torch_golden
uses and justifies (1e-6 absolute / relative), and bit-equal to BoxCoder3D.decode on the same inputs.

Stage B, decisions.  The restatement's stage_b is fed the DEVICE's prob and boxes; from there every step is exact on fp32
data (comparison, total-order sort, clamps, the oracle's NMS on identical boxes, rank cut), so rows and labels must be
equal exactly and in order, scores == prob[rows, labels] and bbox3d == boxes[rows, labels] bit for bit."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import roi_post_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
U = 2.0 ** -24


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _prob_slack(logits, prob64):
    x = np.asarray(logits, F).astype(np.float64)
    d = np.abs(x - x.max(1, keepdims=True))
    c = x.shape[1]
    return prob64 * (d + d.max(1, keepdims=True) + c + 4) * U * 1.01 + 2.0 ** -126


def _run(logits, reg, props, class_specific, weights=None, **kw):
    """one call on the device, checked against both stages; returns (detections as numpy, restatement's stats, prob)"""
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    n_b = [len(p) for p in props]
    allp = np.concatenate(props) if props else np.zeros((0, 7), F)
    dbg = {}
    dets = roi_glue.box_detections(_t(logits), _t(reg), [_t(p) for p in props], weights=weights,
                                   class_specific=class_specific, debug=dbg, **kw)
    prob, boxes = dbg["prob"].cpu().numpy(), dbg["boxes"].cpu().numpy()
    w = (1.0,) * 7 if weights is None else weights
    # ---- stage A
    prob64, boxes_ref = R.stage_a(logits, reg, allp, w, 10000.0, class_specific)
    err, slack = np.abs(prob.astype(np.float64) - prob64), _prob_slack(logits, prob64)
    if err.size:
        print("prob: max err %.3e, max err / bound %.3f" % (err.max(), (err / slack).max()))
    assert (err <= slack).all()
    np.testing.assert_allclose(boxes, boxes_ref, rtol=1e-6, atol=1e-6)
    if len(allp):
        dec = BoxCoder3D(False, weights).decode(_t(reg), _t(allp)).cpu().numpy()
        dec = dec.reshape(len(allp), -1, 7)
        assert (boxes == (dec if class_specific else np.repeat(dec, logits.shape[1], 1))).all()
    # ---- stage B
    stats = []
    ref = R.stage_b(prob, boxes, n_b, kw.get("score_thresh", 0.05), kw.get("nms", 0.5), kw.get("nms_aug_thickness"),
                    kw.get("detections_per_img", 100), stats=stats)
    out, r0 = [], 0
    assert len(dets) == len(n_b)
    for b, (d, (rows, labels)) in enumerate(zip(dets, ref)):
        g = {k: v.cpu().numpy() for k, v in d.items()}
        assert g["rows"].dtype == np.int64 and g["labels"].dtype == np.int64 and g["scores"].dtype == F
        assert g["rows"].tolist() == rows.tolist(), "scene %d: rows differ" % b
        assert g["labels"].tolist() == labels.tolist(), "scene %d: labels differ" % b
        p, bx = prob[r0:r0 + n_b[b]], boxes[r0:r0 + n_b[b]]
        assert (g["scores"] == p[rows, labels]).all()
        assert (g["bbox3d"].view(np.uint32) == np.ascontiguousarray(bx[rows, labels]).view(np.uint32)).all()
        assert dbg["info"][b][0] == len(rows) and dbg["info"][b][1] == stats[b]["M"]
        assert dbg["info"][b][2] == sum(stats[b]["candidates"])
        r0 += n_b[b]
        out.append(g)
    return out, stats, prob


def _main_case(class_specific, c=7, seed=0):
    """4 scenes of unequal length, one empty, one short; wall-like proposals clustered around a few dozen walls"""
    rng = np.random.default_rng(seed)
    n_b = [700, 0, 20, 1000]
    props = [R.wall_proposals(n, 100 + i) for i, n in enumerate(n_b)]
    n = sum(n_b)
    logits = rng.normal(0, 2.0, (n, c)).astype(F)
    if c > 3:
        logits[700:720, 3] = -30.0                            # scene 2, class 3: no candidate
    reg = (rng.normal(0, 0.05, (n, 7 * c if class_specific else 7)) * np.array([1, 1, 1, 1, 1, 1, 0.3] * (c if class_specific else 1))).astype(F)
    return logits, reg, props


@pytest.mark.parametrize("class_specific", [True, False])
def test_main_case_c7_four_scenes(class_specific):
    logits, reg, props = _main_case(class_specific)
    w = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0)
    out, stats, _ = _run(logits, reg * np.tile(np.array(w, F), reg.shape[1] // 7), props, class_specific, weights=w,
                         nms_aug_thickness=(0.2, 0.2), detections_per_img=100)
    # the cases are really hit (on the restatement's result alone)
    assert stats[1]["M"] == 0 and stats[1]["candidates"] == [0] * 6                       # the empty scene
    assert stats[2]["candidates"][2] == 0 and sum(stats[2]["candidates"]) > 0             # a segment with no candidate
    assert 0 < stats[2]["M"] <= 100 and stats[2]["kept"] == stats[2]["M"]                 # M <= D
    assert stats[3]["M"] > 100 and stats[3]["kept"] == 100                                # M > D, distinct scores
    assert sum(stats[3]["candidates"]) > sum(stats[3]["survivors"]) > 0                   # suppression acts
    assert stats[0]["M"] > 100
    assert len(out[1]["rows"]) == 0 and out[1]["bbox3d"].shape == (0, 7)


@pytest.mark.parametrize("class_specific", [True, False])
def test_two_classes_one_scene_no_cut(class_specific):
    """C = 2, nb = 1, detections_per_img = 0 keeps everything"""
    rng = np.random.default_rng(1)
    n = 600
    logits = rng.normal(0, 2.0, (n, 2)).astype(F)
    reg = rng.normal(0, 0.05, (n, 14 if class_specific else 7)).astype(F)
    out, stats, _ = _run(logits, reg, [R.wall_proposals(n, 7)], class_specific, nms_aug_thickness=(0.2, 0.2),
                         detections_per_img=0)
    assert stats[0]["M"] > 100 and stats[0]["kept"] == stats[0]["M"] == len(out[0]["rows"])
    assert stats[0]["candidates"][0] > stats[0]["survivors"][0] > 0


def test_pre_nms_cut_acts():
    """a segment with more than 2000 candidates: the list form is not limited to the RPN's 1000 rows per scene"""
    rng = np.random.default_rng(2)
    n = 2600
    logits = rng.normal(0, 1.0, (n, 2)).astype(F)
    logits[:, 1] += 2.0
    logits[5] = logits[1900]                                 # and a pair of equal scores somewhere
    reg = rng.normal(0, 0.05, (n, 7)).astype(F)
    out, stats, prob = _run(logits, reg, [R.wall_proposals(n, 9, n_gt=60)], False, nms_aug_thickness=(0.2, 0.2))
    assert stats[0]["candidates"][0] > 2000
    # the cut changes the result: a candidate below the 2000 best would have survived
    order = np.argsort(-prob[:, 1], kind="stable")
    cand = order[prob[order, 1] > F(0.05)]
    assert len(cand) > 2000


def test_post_nms_cut_and_ties_at_the_detection_cut():
    """800 well-separated boxes of one class: more than 500 survive, the post-NMS cut leaves 500; five duplicate logit rows
    straddle the 100th place, so the detections_per_img cut returns more than 100"""
    n = 800
    logits = np.zeros((n, 2), F)
    logits[:, 1] = np.linspace(6.0, -1.0, n).astype(F)
    logits[98:103] = logits[98]
    reg = np.zeros((n, 7), F)
    out, stats, prob = _run(logits, reg, [R.separated_proposals(n)], False, detections_per_img=100)
    assert stats[0]["candidates"][0] > 500 and stats[0]["survivors"][0] == 500           # the post-NMS cut acts
    assert stats[0]["M"] == 500 and stats[0]["kept"] == 103 > 100                         # ties at the cut all stay
    assert len(np.unique(prob[98:103, 1])) == 1
    assert out[0]["rows"].tolist() == list(range(103))


def test_equal_scores_row_order_decides_the_survivors():
    """B (row 0) and A (row 1) have exactly equal scores; B overlaps A and C, A and C do not overlap.  Ascending row puts B
    first: B suppresses both.  The other order would keep A and C."""
    props = R.separated_proposals(40)
    props[:, 0] += 100.0
    props[0, :2], props[1, :2], props[2, :2] = (0.0, 0.0), (0.0, -1.2), (0.0, 1.2)
    props[:3, 3], props[:3, 4] = 0.3, 4.0
    logits = np.zeros((40, 2), F)
    logits[:, 1] = np.linspace(1.0, 0.0, 40).astype(F)
    logits[0, 1] = logits[1, 1] = 3.0
    logits[2, 1] = 2.0
    out, stats, prob = _run(logits, np.zeros((40, 7), F), [props], False, detections_per_img=0)
    assert prob[0, 1] == prob[1, 1] > prob[2, 1]
    assert stats[0]["survivors"][0] == 38
    # restatement alone: the order of the tied pair changes the survivors
    b = props[:3]
    assert O.rotate_nms_3d(b, np.array([3.0, 3.0, 2.0], F), 2000, 500, 0.5).tolist() == [0]
    assert O.rotate_nms_3d(b, np.array([3.0, 3.5, 2.0], F), 2000, 500, 0.5).tolist() == [1, 2]
    assert out[0]["rows"][:1].tolist() == [0] and 1 not in out[0]["rows"] and 2 not in out[0]["rows"]


def test_no_rows_at_all():
    out, stats, _ = _run(np.zeros((0, 3), F), np.zeros((0, 21), F), [np.zeros((0, 7), F), np.zeros((0, 7), F)], True)
    assert [len(o["rows"]) for o in out] == [0, 0] and out[0]["bbox3d"].shape == (0, 7)


def test_bit_identical_run_to_run_and_no_sync_before_finish():
    import roi_glue
    logits, reg, props = _main_case(True, seed=4)
    tl, tr, tp = _t(logits), _t(reg), [_t(p) for p in props]
    runs = []
    for _ in range(3):
        dbg = {}
        d = roi_glue.box_detections(tl, tr, tp, nms_aug_thickness=(0.2, 0.2), debug=dbg)
        runs.append([[v.cpu().numpy().copy() for v in (s["rows"], s["labels"], s["scores"], s["bbox3d"])] for s in d] +
                    [[dbg["prob"].cpu().numpy(), dbg["boxes"].cpu().numpy()]])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for x, y in zip(a, b):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
    roi_glue.box_detections(tl, tr, tp, nms_aug_thickness=(0.2, 0.2))      # (buffers and the mailbox exist)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        finish = roi_glue.box_detections(tl, tr, tp, nms_aug_thickness=(0.2, 0.2), defer=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    d = finish()
    for s, ref in zip(d, runs[0]):
        assert s["rows"].cpu().numpy().tobytes() == ref[0].tobytes()
        assert s["scores"].cpu().numpy().tobytes() == ref[2].tobytes()


class _Boxes(object):
    def __init__(self, bbox3d, size3d):
        self.bbox3d, self.size3d, self.mode = bbox3d, size3d, "yx_zb"

    def __len__(self):
        return int(self.bbox3d.shape[0])


def test_post_processor_returns_the_same_lists():
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import PostProcessor
    logits, reg, props = _main_case(False, seed=6)
    w = (1.0,) * 7
    pp = PostProcessor(0.05, 0.45, nms_aug_thickness=[0.2, 0.2], detections_per_img=200, box_coder=BoxCoder3D(False, w),
                       class_specific=False)
    boxes = [_Boxes(_t(p), torch.tensor([[0.0, 0.0, 0.0, 16.0, 12.0, 3.0]])) for p in props]
    res = pp((_t(logits), _t(reg), None), boxes)
    want = roi_glue.box_detections(_t(logits), _t(reg), [_t(p) for p in props], 0.05, 0.45, [0.2, 0.2], 200, w, False)
    assert len(res) == 4 and sum(len(r) for r in res) > 0
    for r, d, b in zip(res, want, boxes):
        assert r.mode == "yx_zb" and r.size3d is b.size3d and len(r) == len(d["rows"])
        assert set(r.fields()) >= {"scores", "labels"}
        assert r.get_field("labels").dtype == torch.int64
        assert torch.equal(r.bbox3d, d["bbox3d"]) and torch.equal(r.get_field("scores"), d["scores"])
        assert torch.equal(r.get_field("labels"), d["labels"])
        if len(r) > 2:
            sub = r[torch.tensor([0, 2], device=DEV)]
            assert len(sub) == 2 and torch.equal(sub.get_field("scores"), d["scores"][[0, 2]])


def test_same_survivors_as_boxlist_nms_3d_looped_the_reference_way():
    """one scene, per class nonzero + boxlist_nms_3d(flag='roi_post') (the existing, separately tested path) + the kthvalue
    cut, against the fused call; distinct scores (the existing path's topk leaves ties open)"""
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
    from maskrcnn_benchmark.structures.boxlist_ops_3d import boxlist_nms_3d
    rng = np.random.default_rng(8)
    n, c = 500, 3
    logits = rng.normal(0, 1.5, (n, c)).astype(F)
    reg = rng.normal(0, 0.05, (n, 7 * c)).astype(F)
    props = R.wall_proposals(n, 21, n_gt=15)
    dbg = {}
    d, = roi_glue.box_detections(_t(logits), _t(reg), [_t(props)], 0.05, 0.5, [0.2, 0.2], 100, debug=dbg)
    # the loop starts from the fused call's own prob and boxes (torch.softmax may differ from the kernel's softmax in the
    # last bit, which could flip a comparison): what is compared is the selection, the suppression and the cut
    prob, dec = dbg["prob"], dbg["boxes"]
    assert torch.allclose(prob, torch.softmax(_t(logits), -1), rtol=1e-5, atol=1e-8)
    assert torch.equal(dec.reshape(n, 7 * c), BoxCoder3D(False, None).decode(_t(reg), _t(props)))
    for j in range(1, c):
        assert len(torch.unique(prob[:, j])) == n, "the seeded scores of a class must be distinct"
    boxes, scores, labels = [], [], []
    for j in range(1, c):
        inds = (prob[:, j] > 0.05).nonzero().squeeze(1)
        bl = DetectionList3D(dec[inds, j], None, {"scores": prob[inds, j]})
        bl = boxlist_nms_3d(bl, 0.5, nms_aug_thickness=[0.2, 0.2], score_field="scores", flag="roi_post")
        boxes.append(bl.bbox3d)
        scores.append(bl.get_field("scores"))
        labels.append(torch.full((len(bl),), j, dtype=torch.int64, device=DEV))
    boxes, scores, labels = torch.cat(boxes), torch.cat(scores), torch.cat(labels)
    assert len(scores) > 100
    t, _ = torch.kthvalue(scores.cpu(), len(scores) - 100 + 1)
    keep = (scores >= t.item()).nonzero().squeeze(1)
    assert torch.equal(d["labels"], labels[keep])
    assert torch.equal(d["bbox3d"], boxes[keep])
    assert torch.equal(d["scores"], scores[keep])
    assert len(keep) < len(scores)                                         # the cut acted
