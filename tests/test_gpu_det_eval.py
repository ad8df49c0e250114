"""Detection evaluation on the device (csrc/det_eval.hip, eval_glue.detection_eval, data3d.evaluation) against the numpy
restatement tests/det_eval_ref.py.  Split the way test_gpu_roi_post.py and test_gpu_roi_loss.py are, so that no tolerance
touches a discrete decision:

Values.  The device's IoU entries (debug listing: every pair of equal label) and the returned pred_iou against the C
oracle's boxes_iou_3d at atol 2e-5 -- the figure test_gpu_roi_loss.py uses for the same arithmetic (k_roi_match's pair loop,
which k_eval_match repeats) and test_gpu_labels.py justifies.

Decisions.  The restatement is fed the DEVICE's IoU entries.  From there every step is exact on fp32 / integer data (a
maximum, a first index, one comparison, an order, integer running sums) and float64 quotients of exact integers, so
gt_index and match must be equal exactly, pred_iou bit for bit, and every float64 output bit for bit (all NaNs counting
as one value: which NaN a 0 / 0 yields is the platform's)."""
import types

import numpy as np
import pytest
import torch

import det_eval_ref as R
import oracle_lib as O
import roi_post_ref as RP

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
AUG = {"target_Y": 0.3, "target_Z": 0.0, "anchor_Y": 0.3, "anchor_Z": 0.0}
KEYS = ("det_boxes", "det_labels", "det_scores", "gt_boxes", "gt_labels")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _aug4(aug):
    a = aug or {}
    return tuple(float(a.get(k, 0.0)) for k in ("target_Y", "target_Z", "anchor_Y", "anchor_Z"))


def _device(sc, C, thresh, aug, only_xy, dbg=None):
    import eval_glue
    return eval_glue.detection_eval(*[[_t(v) for v in sc[k]] for k in KEYS], C, thresh, aug, only_xy, debug=dbg)


def _same_result(res, ref):
    assert res["gt_index"].cpu().numpy().tolist() == ref["gt_index"].tolist(), "gt_index"
    assert res["match"].cpu().numpy().tolist() == ref["match"].tolist(), "match"
    assert res["match"].dtype == torch.int8 and res["gt_index"].dtype == torch.int64
    got = res["pred_iou"].cpu().numpy()
    assert ((got.view(np.uint32) == ref["pred_iou"].view(np.uint32)) | (np.isnan(got) & np.isnan(ref["pred_iou"]))).all()
    for k in ("n_pos", "n_det", "n_tp"):
        assert res[k].tolist() == ref[k].tolist(), k
    for k in ("ap", "map", "recall_precision_score_iou_10steps", "pr_score_th5", "pr_score_th7"):
        assert R.same_bits(res[k], ref[k]), (k, res[k], ref[k])
    assert len(res["rec_prec_score_iou_org"]) == len(ref["rec_prec_score_iou_org"])
    for l, (a, b) in enumerate(zip(res["rec_prec_score_iou_org"], ref["rec_prec_score_iou_org"])):
        assert (a is None) == (b is None), l
        if a is not None:
            assert R.same_bits(a, b), "class %d: rec / prec / score / iou rows" % l


def _run(sc, C, thresh=0.5, aug=AUG, only_xy=True):
    """one evaluation on the device, checked against values and decisions; returns (device result, restatement)"""
    dbg = {}
    res = _device(sc, C, thresh, aug, only_xy, dbg)
    mats = [m.cpu().numpy() for m in dbg["iou"]]
    # ---- values
    worst = 0.0
    for s in range(len(mats)):
        assert mats[s].shape == (len(sc["gt_labels"][s]), len(sc["det_labels"][s]))
        for l in range(C):
            g, d = np.nonzero(sc["gt_labels"][s] == l)[0], np.nonzero(sc["det_labels"][s] == l)[0]
            if len(g) and len(d):
                want = O.boxes_iou_3d(sc["gt_boxes"][s][g], sc["det_boxes"][s][d], _aug4(aug), -1, only_xy)
                got = mats[s][np.ix_(g, d)]
                ok = ~(np.isnan(want) | np.isnan(got))
                if ok.any():
                    worst = max(worst, float(np.abs(got - want)[ok].max()))
                np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    print("iou: max abs difference to the oracle %.3e" % worst)
    by_oracle = R.match_scenes(sc["det_labels"], sc["det_scores"], sc["gt_labels"], C, thresh,
                               R.oracle_iou(sc["gt_boxes"], sc["det_boxes"], _aug4(aug), only_xy))[1]
    np.testing.assert_allclose(res["pred_iou"].cpu().numpy(), by_oracle, rtol=0, atol=2e-5)
    # ---- decisions
    ref = R.evaluate(sc["det_labels"], sc["det_scores"], sc["gt_labels"], C, thresh, R.matrix_iou(mats))
    _same_result(res, ref)
    return res, ref


def _scenes(n_s, g_s, C, seed, n_scores=None):
    """wall-like ground truth; the first detections of a scene are ground-truth boxes under jitters of graded size (IoU
    from ~1 down to 0, several per box), mostly with the box's label, the rest other walls; n_scores: draw the scores
    from that many distinct values"""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in KEYS}
    for i, (n, g) in enumerate(zip(n_s, g_s)):
        gt = RP.wall_proposals(g, seed * 100 + 50 + i, n_gt=max(g, 1)).copy()
        gl = rng.integers(1, C, g).astype(np.int64)
        det = RP.wall_proposals(n, seed * 100 + i).copy()
        dl = rng.integers(1, C, n).astype(np.int64)
        k = min(n, 3 * g)
        if k:
            j = np.arange(k) % g
            scale = (np.arange(k) // g / 3.0)[:, None] + rng.uniform(0, 0.3, (k, 1))
            jit = rng.normal(0, 1, (k, 7)) * np.array([0.05, 0.05, 0.05, 0.02, 0.5, 0.1, 0.02]) * scale
            det[:k] = (gt[j] + jit).astype(F)
            det[:k, 3:6] = np.maximum(det[:k, 3:6], F(0.05))
            keep = rng.random(k) < 0.8
            dl[:k][keep] = gl[j][keep]
        sc = rng.random(n).astype(F) if n_scores is None else (rng.integers(1, n_scores + 1, n) / F(n_scores + 1)).astype(F)
        p = rng.permutation(n)
        out["det_boxes"].append(np.ascontiguousarray(det[p], F)), out["det_labels"].append(dl[p])
        out["det_scores"].append(sc), out["gt_boxes"].append(np.ascontiguousarray(gt, F)), out["gt_labels"].append(gl)
    return out


def test_golden_inputs():
    """case 1: the data set the reference's own evaluation was recorded on -- no IoU lies within 1e-4 of the threshold and
    no two largest IoUs within 1e-4 of each other there, so the device must reproduce the recorded decisions and, from
    them, the recorded float64 results bit for bit"""
    g, sc = R.load_golden()
    aug = dict(zip(("target_Y", "target_Z", "anchor_Y", "anchor_Z"), g["aug"].tolist()))
    res, _ = _run(sc, int(g["num_classes"]), float(g["iou_thresh"]), aug)
    assert res["match"].cpu().numpy().tolist() == g["match"].tolist()
    assert res["gt_index"].cpu().numpy().tolist() == g["gt_index"].tolist()
    R.check_against_golden(res, g)
    assert res["bad_labels"] == (0, 0)


def test_ground_truth_past_one_lds_chunk():
    """case 2: one scene, 133 ground-truth boxes (130 of class 1, 3 of class 2 at rows 5, 60 and 131), 40 detections.
    Rows 127 and 128 -- the last of the first staged chunk and the first of the second -- are the same box: the detection
    on it must take the first.  Detections sit on boxes of the second chunk, on a class-2 box with label 1 (the label
    filter: no match) and on the class-2 box of the second chunk with label 2."""
    gt = RP.separated_proposals(133)
    gt[128] = gt[127]
    gl = np.ones(133, np.int64)
    gl[[5, 60, 131]] = 2
    on = list(range(110, 133)) + [0, 1, 2, 60, 5, 64, 127, 127, 129, 130, 132, 100, 101, 102, 3, 4, 6]
    assert len(on) == 40
    det = gt[on].copy()
    rng = np.random.default_rng(3)
    det[:, 4] *= rng.uniform(0.55, 1.0, 40).astype(F)            # IoU = the length ratio: all above the threshold
    dl = np.ones(40, np.int64)
    dl[on.index(131)] = 2
    sc = {"det_boxes": [det], "det_labels": [dl], "det_scores": [rng.permutation(40).astype(F) / F(41)],
          "gt_boxes": [gt], "gt_labels": [gl]}
    res, ref = _run(sc, 3, aug=None)
    rank = np.cumsum(gl == 1) - 1                                 # class-local index of a class-1 row
    gi = ref["gt_index"]
    assert gi[on.index(129)] == rank[129] == 127 and gi[on.index(132)] == rank[132] == 129     # first maximum in chunk 2
    dup = [i for i, r in enumerate(on) if r in (127, 128)]
    assert len(dup) == 4 and all(gi[i] == rank[127] for i in dup)                               # equal maxima: the first
    assert ref["match"][dup].sum() == 1
    assert gi[on.index(60)] == -1 and gi[on.index(5)] == -1 and gi[on.index(131)] == 2          # label filter
    assert ref["n_pos"].tolist() == [0, 130, 3]


def test_partial_lane_groups_and_bad_labels():
    """case 3: detection counts 1, 15, 16, 17 and 0 in one call (16 lanes per detection, 16 detections per workgroup:
    partial groups, a full workgroup, one detection in a second workgroup, a scene whose workgroup has nothing to do), a
    scene without ground truth, and labels outside [0, C) on both sides, which are skipped and counted"""
    sc = _scenes([1, 15, 16, 17, 0], [3, 4, 0, 6, 2], 3, 11)
    sc["det_labels"][3][4] = 7
    sc["det_labels"][1][0] = -1
    sc["gt_labels"][3][1] = 3
    res, ref = _run(sc, 3)
    assert res["bad_labels"] == (1, 2)
    gi = res["gt_index"].cpu().numpy()
    assert gi[1] == -1 and gi[1 + 15 + 16 + 4] == -1 and (gi[16:32] == -1).all() and (gi >= 0).any()


def test_one_class_past_one_scan_chunk():
    """case 4: chunk * 4 + 1 detections of one class over 12 scenes (one more pass of the scan than fills whole chunks),
    scores from 8 distinct values so that runs of equal scores cross the chunk edges; a few detections of a second class"""
    import _hip
    chunk = _hip.load().aabr_det_eval_scan_chunk()
    total = 4 * chunk + 1
    n_s = [total // 12] * 11 + [total - 11 * (total // 12)]
    sc = _scenes(n_s, [9] * 12, 2, 21, n_scores=8)
    sc["det_boxes"][0] = np.concatenate([sc["det_boxes"][0], sc["gt_boxes"][0][:3]])
    sc["det_labels"][0] = np.concatenate([sc["det_labels"][0], np.full(3, 2, np.int64)])
    sc["det_scores"][0] = np.concatenate([sc["det_scores"][0], np.array([0.9, 0.2, 0.2], F)])
    sc["gt_labels"][0][:2] = 2
    far = RP.separated_proposals(3)
    far[:, 0] += 500.0                                            # three boxes nothing detects: recall stays below 1
    sc["gt_boxes"][1] = np.concatenate([sc["gt_boxes"][1], far])
    sc["gt_labels"][1] = np.concatenate([sc["gt_labels"][1], np.ones(3, np.int64)])
    res, ref = _run(sc, 3)
    assert ref["n_det"].tolist() == [0, total, 3] and 0 < ref["n_tp"][1] < ref["n_pos"][1]
    s = ref["rec_prec_score_iou_org"][1][:, 2]
    assert len(np.unique(s)) == 8 and all(s[k * chunk - 1] == s[k * chunk] for k in range(1, 5))     # ties at every edge


def test_threshold_edges():
    """case 5, S = 1: identical boxes at iou_thresh = 1.0 match (the comparison is strict); with only_xy off, two zero
    heights at the same z give 0 / 0 in the z factor: that NaN is the detection's maximum, the first NaN by index, and
    matches; class 2 has detections and no ground truth: AP 0, rec NaN"""
    gt = RP.separated_proposals(4)
    gt[2] = gt[1]                                                 # the NaN pair: rows 1 and 2 of the ground truth
    gt[1:3, 5] = 0.0
    det = np.concatenate([gt[[0, 1, 3]], RP.separated_proposals(6)[4:]])
    det[2, 4] *= F(0.9)                                           # 0.9 < 1.0: no match
    sc = {"det_boxes": [det], "det_labels": [np.array([1, 1, 1, 2, 2], np.int64)],
          "det_scores": [np.array([0.9, 0.8, 0.7, 0.6, 0.55], F)], "gt_boxes": [gt],
          "gt_labels": [np.ones(4, np.int64)]}
    res, ref = _run(sc, 3, thresh=1.0, aug=None, only_xy=False)
    assert ref["gt_index"].tolist() == [0, 1, -1, -1, -1] and ref["match"].tolist() == [1, 1, 0, 0, 0]
    assert ref["pred_iou"][0] == 1.0 and np.isnan(ref["pred_iou"][1])
    assert ref["ap"][2] == 0.0 and np.isnan(ref["rec_prec_score_iou_org"][2][:, 0]).all()
    assert res["pr_score_th7"].shape == (3, 2)


def _cut(boxes, rows, keep):
    """the boxes `rows` cut to `keep` of their length: the IoU with the uncut box is the ratio (within rounding)"""
    d = boxes[list(rows)].copy()
    d[:, 4] *= np.asarray(keep, F)
    return d


def test_hand_computed_case_on_the_device():
    """the case worked out in test_det_eval_host.test_hand_computed_case, put through the kernels: 3 separate ground-truth
    boxes, detections that are cuts of them (IoU = length ratio: 0.8 and 0.7 on g0, 0.6 on g1, 0.2 and 0.9 on g2), scores
    0.9 0.8 0.7 0.6 0.3.  Expected there: flags 1 0 1 0 1, prec 1, 1/2, 2/3, 1/2, 3/5, rec 1/3, 1/3, 2/3, 2/3, 1,
    AP = 8.4 / 11, [prec, rec] = [1/2, 2/3] at score 0.5 and [1/2, 1/3] at 0.7."""
    gt = RP.separated_proposals(3)
    ratios = [0.8, 0.7, 0.6, 0.2, 0.9]
    sc = {"det_boxes": [_cut(gt, [0, 0, 1, 2, 2], ratios)], "det_labels": [np.ones(5, np.int64)],
          "det_scores": [np.array([0.9, 0.8, 0.7, 0.6, 0.3], F)], "gt_boxes": [gt], "gt_labels": [np.ones(3, np.int64)]}
    res, _ = _run(sc, 2, aug=None)
    assert res["gt_index"].cpu().numpy().tolist() == [0, 0, 1, -1, 2] and res["match"].cpu().numpy().tolist() == [1, 0, 1, 0, 1]
    np.testing.assert_allclose(res["pred_iou"].cpu().numpy(), ratios, rtol=0, atol=2e-5)
    org = res["rec_prec_score_iou_org"][1]
    assert org[:, 1].tolist() == [1.0, 1 / 2, 2 / 3, 2 / 4, 3 / 5] and org[:, 0].tolist() == [1 / 3, 1 / 3, 2 / 3, 2 / 3, 1.0]
    assert abs(res["ap"][1] - 8.4 / 11) < 1e-15 and abs(res["map"] - 8.4 / 11) < 1e-15 and res["ap"][0] == res["ap"][1]
    steps = res["recall_precision_score_iou_10steps"][1]
    assert steps[:, 1].tolist() == [1.0] * 4 + [2 / 3] * 3 + [3 / 5] * 4
    assert steps[:4, 2].tolist() == [float(F(0.9)) + 0.01] * 4 and steps[4, 2] == float(F(0.8)) and steps[10, 2] == float(F(0.3))
    assert res["pr_score_th5"].tolist() == [[1 / 2, 2 / 3]] * 2 and res["pr_score_th7"].tolist() == [[1 / 2, 1 / 3]] * 2
    assert res["n_pos"].tolist() == [0, 3] and res["n_tp"].tolist() == [0, 3]


def test_equal_scores_and_the_last_element_pick_on_the_device():
    """three detections of equal score on one box: the lowest row is the true positive although its IoU is the lowest,
    the curve keeps row order (prec 1, 1/2, 1/3), and with no score above 0.5 both picks read the LAST position
    (k = -1).  Across scenes equal scores go by the scene-major position: scene 0's unmatched detection comes first."""
    gt = RP.separated_proposals(1)
    sc = {"det_boxes": [_cut(gt, [0, 0, 0], [0.6, 0.9, 0.7])], "det_labels": [np.ones(3, np.int64)],
          "det_scores": [np.full(3, 0.4, F)], "gt_boxes": [gt], "gt_labels": [np.ones(1, np.int64)]}
    res, _ = _run(sc, 2, aug=None)
    assert res["match"].cpu().numpy().tolist() == [1, 0, 0]
    assert res["rec_prec_score_iou_org"][1][:, 1].tolist() == [1.0, 1 / 2, 1 / 3]
    assert res["pr_score_th5"][1].tolist() == [1 / 3, 1.0] and res["pr_score_th7"][1].tolist() == [1 / 3, 1.0]
    sc = {"det_boxes": [gt.copy(), gt.copy()], "det_labels": [np.ones(1, np.int64)] * 2,
          "det_scores": [np.array([0.8], F)] * 2, "gt_boxes": [np.zeros((0, 7), F), gt],
          "gt_labels": [np.zeros(0, np.int64), np.ones(1, np.int64)]}
    res, _ = _run(sc, 2, aug=None)
    assert res["match"].cpu().numpy().tolist() == [0, 1] and res["rec_prec_score_iou_org"][1][:, 1].tolist() == [0.0, 1 / 2]


def test_nan_zero_and_infinite_scores_on_the_device():
    """the device's score key on the values the header is checked with on the host: pairs of detections on one box each
    -- NaN against 0.5 (NaN is last: 0.5 is flagged), +0.0 in the higher row against -0.0 in the lower (one key: the lower
    row), -inf against +inf, a denormal against 0.0 -- and the same order in the class's curve"""
    gt = RP.separated_proposals(4)
    scores = np.array([np.nan, 0.5, -0.0, 0.0, -np.inf, np.inf, 0.0, 1e-45], F)
    sc = {"det_boxes": [_cut(gt, [0, 0, 1, 1, 2, 2, 3, 3], [0.9, 0.8] * 4)], "det_labels": [np.ones(8, np.int64)],
          "det_scores": [scores], "gt_boxes": [gt], "gt_labels": [np.ones(4, np.int64)]}
    res, ref = _run(sc, 2, aug=None)
    assert res["match"].cpu().numpy().tolist() == [0, 1, 1, 0, 0, 1, 0, 1]
    got = res["rec_prec_score_iou_org"][1][:, 2]
    assert got[0] == np.inf and got[1] == 0.5 and got[2] == float(F(1e-45)) and got[6] == -np.inf and np.isnan(got[7])
    assert np.signbit(got[3:6]).tolist() == [True, False, False]            # -0.0 (row 2), +0.0 (row 3), 0.0 (row 6)
    assert np.isnan(res["recall_precision_score_iou_10steps"][1][10, 2])     # lowest score where rec <= 1: the NaN


def test_evaluate_through_a_dataset_object():
    """data3d.evaluation.evaluate: ground truth fetched by each prediction's constants["data_id"] (here the scenes in
    reverse), by position where a prediction has none; equal to eval_detection_suncg on the aligned lists"""
    import data3d.evaluation as E
    from data3d.evaluation.suncg.suncg_eval import eval_detection_suncg
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
    sc = _scenes([20, 9, 14], [5, 3, 4], 3, 61)
    metas = types.SimpleNamespace(label_2_class={0: "background", 1: "wall", 2: "door"})
    gts = [DetectionList3D(_t(b), None, {"labels": _t(l)}) for b, l in zip(sc["gt_boxes"], sc["gt_labels"])]
    preds = [DetectionList3D(_t(b), None, {"labels": _t(l), "scores": _t(s)})
             for b, l, s in zip(sc["det_boxes"], sc["det_labels"], sc["det_scores"])]
    asked = []

    class _Dataset(object):
        dset_metas = metas

        def get_groundtruth(self, data_id):
            asked.append(data_id)
            return gts[data_id]
    shuffled = [preds[2], preds[1], preds[0]]
    shuffled[0].constants = {"data_id": 2}
    shuffled[2].constants = {"data_id": 0}                        # (the middle one has no constants: its position, 1)
    got = E.evaluate(dataset=_Dataset(), predictions=shuffled, iou_thresh_eval=0.4, output_folder=None, box_only=False,
                     epoch=1, is_train=False, eval_aug_thickness=AUG)
    assert asked == [2, 1, 0] and got["label_2_class"] is metas.label_2_class
    want = eval_detection_suncg(shuffled, [gts[2], gts[1], gts[0]], 0.4, metas, eval_aug_thickness=AUG)
    for k in ("ap", "map", "recall_precision_score_iou_10steps", "pr_score_th5", "pr_score_th7"):
        assert R.same_bits(got[k], want[k])
    assert got["match"].cpu().numpy().tobytes() == want["match"].cpu().numpy().tobytes() and got["n_tp"].sum() > 0


def test_no_detections_at_all():
    """two scenes with ground truth and not one detection: no match or curve launch has anything to do; every class
    with ground truth has AP NaN, as in the reference (prec[l] is None)"""
    sc = _scenes([0, 0], [3, 2], 3, 51)
    res, ref = _run(sc, 3)
    assert res["gt_index"].numel() == 0 and np.isnan(res["ap"]).all() and np.isnan(res["map"])
    assert res["n_pos"].sum() == 5 and all(a is None for a in res["rec_prec_score_iou_org"])


def test_forty_scenes():
    """case 5, S = 40: the per-scene offsets are device arrays, so nothing is limited to the 16 scenes of a training batch"""
    rng = np.random.default_rng(5)
    sc = _scenes(rng.integers(0, 12, 40).tolist(), rng.integers(0, 6, 40).tolist(), 5, 31)
    res, ref = _run(sc, 5)
    assert len(ref["ap"]) == 5 and ref["n_tp"].sum() > 0


class _Boxes(object):
    def __init__(self, bbox3d):
        self.bbox3d, self.size3d, self.mode = bbox3d, None, "yx_zb"

    def __len__(self):
        return int(self.bbox3d.shape[0])


def test_post_processor_output_goes_straight_in():
    """case 6: PostProcessor's DetectionList3D lists through eval_detection_suncg = detection_eval on the same tensors"""
    import eval_glue
    from data3d.evaluation.suncg.suncg_eval import eval_detection_suncg, result_str
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D, PostProcessor
    rng = np.random.default_rng(8)
    n_b, c = [300, 0, 40], 4
    props = [RP.wall_proposals(n, 200 + i) for i, n in enumerate(n_b)]
    logits = rng.normal(0, 2.0, (sum(n_b), c)).astype(F)
    reg = rng.normal(0, 0.05, (sum(n_b), 7)).astype(F)
    pp = PostProcessor(0.05, 0.45, nms_aug_thickness=[0.2, 0.2], detections_per_img=60, box_coder=BoxCoder3D(False, (1.0,) * 7),
                       class_specific=False)
    preds = pp((_t(logits), _t(reg), None), [_Boxes(_t(p)) for p in props])
    assert sum(len(p) for p in preds) > 20
    gts = []
    for i, p in enumerate(props):
        k = min(len(p), 6)
        gts.append(DetectionList3D(_t(p[:k]), None, {"labels": _t(rng.integers(1, c, k).astype(np.int64))}))
    metas = types.SimpleNamespace(label_2_class={0: "background", 1: "wall", 2: "door", 3: "window"})
    got = eval_detection_suncg(preds, gts, 0.3, metas, use_07_metric=True, eval_aug_thickness=AUG)
    want = eval_glue.detection_eval([p.bbox3d for p in preds], [p.get_field("labels") for p in preds],
                                    [p.get_field("scores") for p in preds], [g.bbox3d for g in gts],
                                    [g.get_field("labels") for g in gts], 4, 0.3, AUG)
    for k in ("gt_index", "pred_iou", "match"):
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes()
    for k in ("ap", "map", "recall_precision_score_iou_10steps", "pr_score_th5", "pr_score_th7"):
        assert R.same_bits(got[k], want[k])
    assert got["n_tp"].sum() > 0 and result_str(got, metas.label_2_class).startswith("mAP: ")


def test_bit_identical_run_to_run():
    """case 7: the claim is an integer minimum and every sum an integer: two runs agree in every byte"""
    sc = _scenes([60, 0, 33, 90], [8, 2, 0, 12], 4, 41, n_scores=5)
    runs = []
    for _ in range(2):
        r = _device(sc, 4, 0.4, AUG, True)
        runs.append([r[k].cpu().numpy().tobytes() for k in ("gt_index", "pred_iou", "match")] +
                    [np.asarray(r[k]).tobytes() for k in ("ap", "map", "recall_precision_score_iou_10steps", "pr_score_th5",
                                                          "pr_score_th7", "n_tp")] +
                    [b"" if a is None else a.tobytes() for a in r["rec_prec_score_iou_org"]])
    assert runs[0] == runs[1]
