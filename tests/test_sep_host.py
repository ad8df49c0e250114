"""The separated-classifier groups of the box head without a GPU: the group tables of SeperateClassifier against the
worked case and the restatement (tests/sep_ref.py), the refusals, and the C ABI / Python surface of the grouped entry
points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sep_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aabr_roi_gt_group_keys", "aabr_roi_targets_grouped", "aabr_roi_box_loss_grouped_scratch_floats",
               "aabr_roi_box_loss_grouped_forward", "aabr_roi_box_loss_grouped_backward",
               "aabr_roi_post_detections_grouped")


def _sc(sep, n, class_specific=False):
    from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
    return SeperateClassifier(sep, n, class_specific, "ROI_LOSS")


def test_worked_tables_seven_classes_two_groups():
    s = _sc([[1], [5, 4]], 7)
    assert s.need_seperate and s.group_num == 3
    assert s.grouped_classes == [[0, 2, 3, 6], [7, 1], [8, 4, 5]]
    assert s.class_nums == [4, 2, 3]
    assert s.seperated_num_classes_total == 9
    want = {0: (0, 0), 2: (0, 1), 3: (0, 2), 6: (0, 3), 7: (1, 0), 1: (1, 1), 8: (2, 0), 4: (2, 1), 5: (2, 2)}
    got = s.org_labels_to_sep_labels.tolist()
    assert len(got) == 9 and {c: tuple(v) for c, v in enumerate(got)} == want
    assert [t.tolist() for t in s.sep_labels_to_org_labels] == s.grouped_classes
    # the restatement builds the same tables
    ref = SR.group_tables([[1], [5, 4]], 7)
    assert ref["grouped_classes"] == s.grouped_classes and ref["class_nums"] == s.class_nums
    assert ref["C_tot"] == 9 and ref["org_to_sep"] == want
    # the two consequences the kernels rely on
    for g, gc in enumerate(s.grouped_classes):
        assert gc[0] == (0 if g == 0 else 7 + g - 1)
        assert all(0 < c < 7 for c in gc[1:])
    new = s.update_labels_to_seperated_id([torch.tensor([1, 5, 4, 2, 6, 0]), torch.zeros(0, dtype=torch.int64)])
    assert new[0].tolist() == [1, 2, 1, 1, 3, 0] and new[0].dtype == torch.int64 and new[1].numel() == 0


def test_tables_one_group_of_five_classes():
    s = _sc([[1]], 5)
    assert s.grouped_classes == [[0, 2, 3, 4], [5, 1]] and s.class_nums == [4, 2] and s.group_num == 2
    assert s.seperated_num_classes_total == 6
    assert s.org_labels_to_sep_labels.tolist() == [[0, 0], [1, 1], [0, 1], [0, 2], [0, 3], [1, 0]]
    assert SR.group_tables([[1]], 5)["grouped_classes"] == s.grouped_classes
    empty = _sc([], 5, class_specific=True)
    assert empty.need_seperate is False


def test_refusals():
    with pytest.raises(ValueError, match="CLASS_SPECIFIC"):
        _sc([[1]], 5, class_specific=True)
    with pytest.raises(ValueError, match="background"):
        _sc([[1], [0, 2]], 5)
    with pytest.raises(ValueError, match="groups"):
        _sc([[c] for c in range(1, 9)], 10)                       # G = 9
    _sc([[c] for c in range(1, 8)], 10)                           # G = 8 is the limit
    with pytest.raises(ValueError):
        _sc([[1], [1]], 5)                                        # a class in two groups
    with pytest.raises(ValueError):
        _sc([2], 5)                                               # not a list of lists
    with pytest.raises(ValueError):
        _sc([[3]], 34)                                            # C_tot = 35 > 32
    s = _sc([[1]], 5)
    for name in ("seperate_rpn_assin", "seperate_rpn_selector", "seperate_rpn_loss_evaluator"):
        with pytest.raises(NotImplementedError, match="later change"):
            getattr(s, name)(None)
    assert not hasattr(s, "group_id_include_wall")
    with pytest.raises(TypeError):
        s.seperate_subsample([], [], lambda p, t: p)
    with pytest.raises(TypeError):
        s.post_processor(None, None, None, [], lambda x, b: b)
    with pytest.raises(TypeError):
        s.roi_box_loss_seperated(len, None, None, None, None, None)


def test_filter_gt_order():
    gc = [[0, 2, 3, 6], [7, 1], [8, 4, 5]]
    labels = [5, 4, 1, 5, 2, 4, 6, 2]
    assert [v.tolist() for v in SR.filter_gt(labels, gc, 2)] == [[1, 5, 0, 3], [1, 1, 2, 2]]
    assert [v.tolist() for v in SR.filter_gt(labels, gc, 0)] == [[4, 7, 6], [1, 1, 3]]
    assert [v.tolist() for v in SR.filter_gt(labels, gc, 1)] == [[2], [1]]
    assert SR.filter_gt([], gc, 1)[0].size == 0


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    ver = int(re.search(r"#define AABR_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _hip.ABI_VERSION == 640
    lib = _hip.load()
    assert lib.aabr_version() == 640
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS, name
        assert hasattr(lib, name), name
        decl = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        nargs = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert nargs == len(_hip._SIGS[name][1]), name
    mk = open(os.path.join(REPO, "automatic-as-built-reconstruction_amd", "csrc", "Makefile")).read()
    assert "sep_groups.h" in mk


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


GOOD = (3, 9, [4, 2, 3], [0, 2, 3, 6, 7, 1, 8, 4, 5])
BAD_TABLES = [((1, 9, [9], list(range(9))), b"group count"),
              ((9, 9, [1] * 9, list(range(9))), b"group count"),
              ((2, 33, [31, 2], list(range(33))), b"C_tot"),
              ((3, 9, [4, 2, 3], [0, 2, 3, 6, 7, 1, 9, 4, 5]), b"outside"),
              ((3, 9, [4, 2, 3], [0, 2, 3, 6, 7, 1, 8, 4, 4]), b"two groups"),
              ((3, 9, [4, 0, 3], [0, 2, 3, 6, 8, 4, 5]), b"columns")]


def test_argument_validation_without_gpu():
    import _hip
    lib = _hip.load()
    assert lib.aabr_roi_box_loss_grouped_scratch_floats() > 0

    def keys(tab, nb=2):
        G, c_tot, cn, cols = tab
        return lib.aabr_roi_gt_group_keys(None, nb, _i64([3] * nb), G, c_tot, _i32(cn), _i32(cols), None, None)

    def fwd(tab, n=10, beta=0.2):
        G, c_tot, cn, cols = tab
        return lib.aabr_roi_box_loss_grouped_forward(None, None, 0, n, G, c_tot, _i32(cn), _i32(cols), None, None, None,
                                                     beta, None, None, None, None, None, None)

    def bwd(tab, n=10):
        G, c_tot, cn, cols = tab
        return lib.aabr_roi_box_loss_grouped_backward(None, None, 0, n, G, c_tot, _i32(cn), _i32(cols), None, None, None,
                                                      0.2, None, None, None, None, None, None)

    def post(tab, nb=2, pre=2000, post_=500):
        G, c_tot, cn, cols = tab
        return lib.aabr_roi_post_detections_grouped(None, None, None, None, nb, _i64([5] * nb), G, c_tot, _i32(cn),
                                                    _i32(cols), None, 0, 10000.0, 0.05, 0.5, 0.0, 0.0, 1, pre, post_, 100,
                                                    None, None, None, None, None, None, None, None, None)

    def tgt(nb, G, B=500, num_pos=125):
        return lib.aabr_roi_targets_grouped(None, None, None, None, nb, G, None, None, None, -1, 1, 0.5, 0.5, None, 0, 1, B,
                                            num_pos, None, None, None, None, None, None, None, None, None, None, None)

    for tab, msg in BAD_TABLES:
        for fn in (keys, fwd, bwd, post):
            assert fn(tab) == -1 and msg in lib.aabr_last_error(), (fn.__name__, tab, lib.aabr_last_error())
    assert keys(GOOD, nb=6) == -1 and b"scenes x groups" in lib.aabr_last_error()        # 18 segments
    assert keys(GOOD, nb=2) == -1 and b"null" in lib.aabr_last_error()
    assert fwd(GOOD, beta=0.0) == -1 and fwd(GOOD, n=-1) == -1
    assert fwd(GOOD) == -1 and b"null" in lib.aabr_last_error()
    assert bwd(GOOD) == -1 and b"null" in lib.aabr_last_error()
    assert post(GOOD, nb=17) == -1 and b"nb must be" in lib.aabr_last_error()
    assert post(GOOD, pre=4000) == -1 and b"pre_max" in lib.aabr_last_error()
    assert post(GOOD) == -1 and b"null" in lib.aabr_last_error()
    assert tgt(2, 1) == -1 and b"group count" in lib.aabr_last_error()
    assert tgt(2, 9) == -1 and b"group count" in lib.aabr_last_error()
    assert tgt(6, 3) == -1 and b"scenes x groups" in lib.aabr_last_error()
    assert tgt(2, 3, B=513) == -1 and b"batch_size_per_image" in lib.aabr_last_error()
    assert tgt(2, 3) == -1 and b"null" in lib.aabr_last_error()


def test_glue_refuses_bad_groups_before_the_gpu():
    import roi_glue
    gc, c_tot, cn, cols = roi_glue.sep_group_tables([[0, 2, 3, 6], [7, 1], [8, 4, 5]])
    assert c_tot == 9 and list(cn) == [4, 2, 3] and list(cols) == [0, 2, 3, 6, 7, 1, 8, 4, 5]
    assert roi_glue.sep_group_tables(_sc([[1]], 5))[1] == 6
    for bad in ([[0, 1]], [[0, 1], [1, 2]], [[0]] * 9, [[0, 1], []], [[0, 40], [1]]):
        with pytest.raises(ValueError):
            roi_glue.sep_group_tables(bad)
    z = torch.zeros
    with pytest.raises(ValueError):                  # class-specific width
        roi_glue.box_head_loss_grouped(z(3, 9), z(3, 63), z(3), z(3, dtype=torch.int64), z(3, 7), gc)
    with pytest.raises(ValueError):                  # C_tot columns
        roi_glue.box_head_loss_grouped(z(3, 8), z(3, 7), z(3), z(3, dtype=torch.int64), z(3, 7), gc)
    with pytest.raises(ValueError):
        roi_glue.box_head_targets_grouped([z(4, 7)], [[2, 1, 0]], [z(0, 7)], [z(0, dtype=torch.int64)], gc)
    with pytest.raises(_hip_error()):
        roi_glue.box_head_targets_grouped([z(0, 7)] * 6, [[0, 0, 0]] * 6, [z(0, 7)] * 6, [z(0, dtype=torch.int64)] * 6, gc)


def _hip_error():
    import _hip
    return _hip.AabrError


def test_box_head_cfg_and_loss_evaluator_surface():
    import roi_glue
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss import FastRCNNLossComputation, make_roi_box_loss_evaluator
    from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
    plain = roi_glue.box_head_cfg()
    assert plain.MODEL.SEPARATE_CLASSES_ID == [] and plain.MODEL.SEPARATE_CLASSES == []
    ev, sep = make_roi_box_loss_evaluator(plain)
    assert sep is None and ev.need_seperate is False
    cfg = roi_glue.box_head_cfg(class_specific=False, separate=("wall",), separate_ids=[[1]])
    assert cfg.MODEL.SEPARATE_CLASSES_ID == [[1]] and cfg.MODEL.SEPARATE_CLASSES == ["wall"]
    ev, sep = make_roi_box_loss_evaluator(cfg)
    assert isinstance(sep, SeperateClassifier) and ev.seperate_classifier is sep and ev.need_seperate is True
    assert sep.grouped_classes == [[0, 2], [3, 1]]
    with pytest.raises(ValueError):
        make_roi_box_loss_evaluator(roi_glue.box_head_cfg(class_specific=True, separate=("wall",), separate_ids=[[1]]))
    with pytest.raises(ValueError):                  # groups need this package's classifier and class-agnostic boxes
        FastRCNNLossComputation(ev.proposal_matcher, ev.fg_bg_sampler, ev.box_coder, "Diff", True, ev.aug_thickness, sep, True)
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import ROIBoxHead3D
    head = ROIBoxHead3D(cfg)
    assert head.need_seperate is True and head.predictor.num_classes == 4
    assert ROIBoxHead3D(plain).need_seperate is False
    assert set(head._roi_losses([1, 2], [3, 4])) == {"loss_classifier_roi_0", "loss_classifier_roi_1",
                                                     "loss_box_reg_roi_0", "loss_box_reg_roi_1"}
