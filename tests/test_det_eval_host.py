"""Detection evaluation without a GPU: the numpy restatement (tests/det_eval_ref.py) against what the reference's own
evaluation returned (tests/golden/det_eval_golden.npz, written by tests/golden/gen_det_eval_golden.py), a case worked out
by hand, the tie rule and the k = -1 quirk, and the library's new entry points refusing bad arguments before any launch."""
import os
import types

import numpy as np
import pytest

import det_eval_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


def test_restatement_reproduces_the_reference():
    import oracle_lib as O  # noqa: F401  (the C oracle must be built)
    g, sc = R.load_golden()
    res = R.evaluate(sc["det_labels"], sc["det_scores"], sc["gt_labels"], int(g["num_classes"]), float(g["iou_thresh"]),
                     R.oracle_iou(sc["gt_boxes"], sc["det_boxes"], tuple(g["aug"]), True))
    assert res["match"].tolist() == g["match"].tolist()
    assert res["gt_index"].tolist() == g["gt_index"].tolist()
    R.check_against_golden(res, g)
    # the IoU column is a value (the oracle restates the reference's float32 arithmetic): the tolerance of the other IoU
    # comparisons against it (test_gpu_roi_loss.py: atol 2e-5)
    for l, has in enumerate(g["has_curve"]):
        if has:
            np.testing.assert_allclose(res["rec_prec_score_iou_org"][l][:, 3], g["org_%d" % l][:, 3], rtol=0, atol=2e-5)
    # the features the fixture was built for
    assert np.isnan(res["ap"][2]) and res["n_pos"][2] > 0 and res["n_det"][2] == 0        # ground truth, no detection
    assert res["ap"][3] == 0.0 and res["n_pos"][3] == 0 and res["n_det"][3] > 0           # detections, no ground truth
    assert np.isnan(res["rec_prec_score_iou_org"][3][:, 0]).all()
    assert 0 < res["match"].sum() < (res["gt_index"] >= 0).sum()                          # clusters: matched, not flagged


def _one_scene(scores, M, n_gt, labels=None, gt_labels=None):
    n = len(scores)
    dl = [np.ones(n, np.int64) if labels is None else np.asarray(labels, np.int64)]
    gl = [np.ones(n_gt, np.int64) if gt_labels is None else np.asarray(gt_labels, np.int64)]
    return R.evaluate(dl, [np.asarray(scores, F)], gl, 2, 0.5, R.matrix_iou([np.asarray(M, F)]))


def test_hand_computed_case():
    """1 scene, 1 class, 3 ground-truth boxes, 5 detections, iou_thresh 0.5:

        detection   score   best box (IoU)    flag
        d0          0.9     g0 (0.8)          1
        d1          0.8     g0 (0.7)          0   second on g0
        d2          0.7     g1 (0.6)          1
        d3          0.6     g2 (0.2)          0   below the threshold: gt_index -1
        d4          0.3     g2 (0.9)          1

    tp = 1 1 2 2 3, fp = 0 1 1 2 2; prec = 1, 1/2, 2/3, 1/2, 3/5; rec = 1/3, 1/3, 2/3, 2/3, 1.
    t = 0.0 .. 0.3: every position has rec >= t, max prec = 1           (4 thresholds)
    t = 0.4 .. 0.6: positions 2 .. 4,            max prec = 2/3         (3 thresholds; 6 * 0.1 = 0.6000000000000001 <= 2/3)
    t = 0.7 .. 1.0: position 4 (rec = 1 >= 10 * 0.1 = 1.0), prec = 3/5  (4 thresholds)
    AP = (4 * 1 + 3 * 2/3 + 4 * 3/5) / 11 = 8.4 / 11 = 0.763636...
    score > 0.5 holds for 4 detections: k = 3, [prec, rec] = [1/2, 2/3]; score > 0.7 for 2 (float32 0.7 is below 0.7):
    k = 1, [1/2, 1/3].  Only class 1 exists, so row 0 (the mean of the others) repeats it and map = AP."""
    M = np.zeros((3, 5), F)
    M[0, 0], M[0, 1], M[1, 2], M[2, 3], M[2, 4] = 0.8, 0.7, 0.6, 0.2, 0.9
    M[1, 0] = 0.1
    res = _one_scene([0.9, 0.8, 0.7, 0.6, 0.3], M, 3)
    assert res["gt_index"].tolist() == [0, 0, 1, -1, 2] and res["match"].tolist() == [1, 0, 1, 0, 1]
    assert res["pred_iou"].tolist() == [F(0.8), F(0.7), F(0.6), F(0.2), F(0.9)]
    org = res["rec_prec_score_iou_org"][1]
    assert org[:, 1].tolist() == [1.0, 1 / 2, 2 / 3, 2 / 4, 3 / 5] and org[:, 0].tolist() == [1 / 3, 1 / 3, 2 / 3, 2 / 3, 1.0]
    assert abs(res["ap"][1] - 8.4 / 11) < 1e-15 and abs(res["map"] - 8.4 / 11) < 1e-15 and res["ap"][0] == res["ap"][1]
    steps = res["recall_precision_score_iou_10steps"][1]
    assert steps[:, 1].tolist() == [1.0] * 4 + [2 / 3] * 3 + [3 / 5] * 4
    # s: the lowest score with rec <= t, else max + 0.01: rec <= t first holds at t = 0.4 (rec 1/3: positions 0, 1)
    assert steps[:4, 2].tolist() == [float(F(0.9)) + 0.01] * 4 and steps[4, 2] == float(F(0.8)) and steps[10, 2] == float(F(0.3))
    assert steps[:4, 3].tolist() == [float(F(0.9))] * 4 and steps[10, 3] == float(F(0.9))
    assert res["pr_score_th5"].tolist() == [[1 / 2, 2 / 3]] * 2 and res["pr_score_th7"].tolist() == [[1 / 2, 1 / 3]] * 2


def test_tie_rule_and_last_element_quirk():
    # two detections of equal score on one box: the lower row is the true positive, whatever the IoUs
    M = np.array([[0.6, 0.9, 0.7]], F)
    res = _one_scene([0.4, 0.4, 0.4], M, 1)
    assert res["match"].tolist() == [1, 0, 0]
    # the curve keeps equal scores in row order too: prec = 1, 1/2, 1/3
    assert res["rec_prec_score_iou_org"][1][:, 1].tolist() == [1.0, 1 / 2, 1 / 3]
    # no score above 0.5: k = -1 reads the LAST element of prec / rec, as numpy indexing does
    assert res["pr_score_th5"][1].tolist() == [1 / 3, 1.0] and res["pr_score_th7"][1].tolist() == [1 / 3, 1.0]
    # across scenes: equal scores are ordered by the scene-major position
    dl = [np.array([1], np.int64), np.array([1], np.int64)]
    gl = [np.zeros(0, np.int64), np.array([1], np.int64)]
    res = R.evaluate(dl, [np.array([0.8], F), np.array([0.8], F)], gl, 2, 0.5,
                     R.matrix_iou([np.zeros((0, 1), F), np.array([[1.0]], F)]))
    assert res["match"].tolist() == [0, 1] and res["rec_prec_score_iou_org"][1][:, 1].tolist() == [0.0, 1 / 2]
    # IoU == iou_thresh matches (the comparison is strict), a NaN IoU wins and matches
    res = _one_scene([0.9, 0.8], np.array([[0.5, 0.2], [0.1, np.nan], [0.3, np.nan]], F), 3)
    assert res["gt_index"].tolist() == [0, 1] and res["match"].tolist() == [1, 1] and np.isnan(res["pred_iou"][1])


def test_new_symbols_refuse_bad_arguments_without_a_gpu():
    import _hip
    lib = _hip.load()
    assert lib.aabr_version() == 640
    one = 4096                                         # a non-null pointer nobody follows
    aug = _hip.f32x4([0, 0, 0, 0])
    E = -1

    def match(S=2, N=8, G=4, nmax=5, C=4, det=one, begin=one, scratch=one, aug_=aug):
        return lib.aabr_det_eval_match(det, one, one, one, one, S, begin, one, N, G, nmax, C, 0.5, aug_, 1, one, one, one,
                                       one, None, None, scratch, None)

    for kw, what in (({"C": 1}, b"C"), ({"C": 33}, b"C"), ({"S": 0}, b"n_scenes"), ({"S": 65536}, b"n_scenes"),
                     ({"N": -1}, b"negative"), ({"G": -1}, b"negative"), ({"nmax": 9}, b"n_det_max"),
                     ({"N": 1 << 31, "nmax": 1}, b"2^31"), ({"det": None}, b"null"), ({"begin": None}, b"null"),
                     ({"scratch": None}, b"null"), ({"aug_": None}, b"null"), ({"scratch": 4100}, b"aligned")):
        assert match(**kw) == E, kw
        err = lib.aabr_last_error()
        assert b"aabr_det_eval_match" in err and what in err, (kw, err)

    def curves(N=8, G=4, C=4, key=one, cls=one, gl=one):
        return lib.aabr_det_eval_curves(key, one, one, one, one, gl, N, G, C, one, cls, None)

    for kw, what in (({"C": 1}, b"C"), ({"C": 33}, b"C"), ({"N": -1}, b"negative"), ({"G": -2}, b"negative"),
                     ({"key": None}, b"null"), ({"cls": None}, b"null"), ({"gl": None}, b"null")):
        assert curves(**kw) == E, kw
        err = lib.aabr_last_error()
        assert b"aabr_det_eval_curves" in err and what in err, (kw, err)
    assert lib.aabr_det_eval_scratch_words(-1, 0) == -1 and lib.aabr_det_eval_scratch_words(0, 1 << 31) == -1
    assert lib.aabr_det_eval_scratch_words(10, 3) >= 2 * 3 + 3 + 10
    assert lib.aabr_det_eval_scan_chunk() >= 64
    for name in ("aabr_det_eval_scratch_words", "aabr_det_eval_match", "aabr_det_eval_curves", "aabr_det_eval_scan_chunk"):
        assert name in _hip.EXPORTED_SYMBOLS


def test_reference_named_module_and_its_refusals():
    import data3d.evaluation as E
    from data3d.evaluation.suncg.suncg_eval import eval_detection_suncg, evaluate_dataset, result_str
    metas = types.SimpleNamespace(label_2_class={0: "background", 1: "wall"})
    with pytest.raises(ValueError, match="use_07_metric"):
        eval_detection_suncg([], [], 0.5, metas, use_07_metric=False)
    with pytest.raises(ValueError, match="pred_for_each_gt"):
        eval_detection_suncg([], [], 0.5, metas, pred_for_each_gt=True)
    with pytest.raises(ValueError, match="drawing"):
        eval_detection_suncg([], [], 0.5, metas, draw=True)
    with pytest.raises(ValueError, match="0.3"):
        eval_detection_suncg([], [], 0.5, metas, eval_aug_thickness={"target_Y": 0.4, "anchor_Y": 0.0})
    with pytest.raises(ValueError):
        eval_detection_suncg([], [], 0.5, metas)                      # no scene
    # nothing predicted, or nothing to find: no evaluation (and no GPU is asked for)
    class _Empty(object):
        def __len__(self):
            return 0

    class _One(_Empty):
        def __len__(self):
            return 1

    class _Dataset(object):
        dset_metas = metas

        def get_groundtruth(self, data_id):
            return _Empty()
    assert E.evaluate(dataset=_Dataset(), predictions=[_Empty(), _Empty()], iou_thresh_eval=0.5, output_folder=None,
                      box_only=False, epoch=3, is_train=True, eval_aug_thickness=None) is None
    assert evaluate_dataset(_Dataset(), [_One()], 0.5) is None
    text = result_str({"ap": np.array([0.25, 0.5, np.nan]), "map": 0.375}, {0: "background", 1: "wall", 2: "door"})
    assert text.splitlines()[0] == "mAP: 0.3750" and "wall" in text and text.splitlines()[-1].endswith("nan")


def test_host_epilogue_on_recorded_class_words():
    """eval_glue.summarize (truncation, row 0 = mean, compressed score-threshold rows) on class words written from the
    restatement's per-class results of the golden: the same dict as the reference's"""
    import eval_glue
    g, sc = R.load_golden()
    C = int(g["num_classes"]) + 2                      # two classes past the largest label seen: cut off
    res = R.evaluate(sc["det_labels"], sc["det_scores"], sc["gt_labels"], C, float(g["iou_thresh"]),
                     R.oracle_iou(sc["gt_boxes"], sc["det_boxes"], tuple(g["aug"]), True))
    G = eval_glue
    words = np.zeros((C, G.CLASS_WORDS), np.int64)
    wd = words.view(np.float64)
    wd[:, :G.WORD_TH7 + 2] = np.nan
    rows, begin = [], 0
    labels = np.concatenate(sc["det_labels"])
    scores = np.concatenate(sc["det_scores"])
    for l in range(len(res["ap"])):
        sel = labels == l
        c = R.class_curve(scores[sel], res["match"][sel], res["pred_iou"][sel], res["n_pos"][l])
        words[l, [G.WORD_NPOS, G.WORD_NDET, G.WORD_TP, G.WORD_BEGIN]] = [res["n_pos"][l], res["n_det"][l], res["n_tp"][l], begin]
        if c is not None:
            wd[l, G.WORD_AP], wd[l, G.WORD_TABLE:G.WORD_TABLE + 44] = c["ap"], c["steps"].reshape(-1)
            wd[l, G.WORD_TH5:G.WORD_TH5 + 2], wd[l, G.WORD_TH7:G.WORD_TH7 + 2] = c["th5"], c["th7"]
            rows.append(np.stack([c["rec"], c["prec"], c["scores"], c["iou"]], 1))
            begin += len(c["prec"])
    got = eval_glue.summarize(words, np.concatenate(rows))
    R.check_against_golden(got, g)
    assert got["bad_labels"] == (0, 0) and got["n_pos"].tolist() == res["n_pos"].tolist()


def test_word_offsets_match_the_header():
    """eval_glue's names for the words of a class's row against csrc/det_eval.h, which the kernel writes by"""
    import re
    import eval_glue as G
    hdr = open(os.path.join(os.path.dirname(HERE), "automatic-as-built-reconstruction_amd", "csrc", "det_eval.h")).read()
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int kEval(\w+) = (\d+);", hdr)}
    want = {"ClassWords": G.CLASS_WORDS, "WordAp": G.WORD_AP, "WordTable": G.WORD_TABLE, "WordTh5": G.WORD_TH5,
            "WordTh7": G.WORD_TH7, "WordNPos": G.WORD_NPOS, "WordNDet": G.WORD_NDET, "WordTp": G.WORD_TP,
            "WordBegin": G.WORD_BEGIN, "WordBadGt": G.WORD_BAD_GT, "WordBadDet": G.WORD_BAD_DET, "Steps": 11}
    assert {n: k.get(n) for n in want} == want
    assert {n for n in k if n.startswith("Word")} == {n for n in want if n.startswith("Word")}
