"""The box head's loss without a GPU: the restatement (tests/roi_loss_ref.py) against the reference's own composition
written with torch on the CPU in float64, a brute-force loop for the matcher's tie rule, and the C ABI / Python surface
of the feature."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import roi_loss_ref as R
import roi_post_ref as RP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("aabr_roi_targets_scratch_words", "aabr_roi_targets", "aabr_roi_box_loss_scratch_floats",
               "aabr_roi_box_loss_forward", "aabr_roi_box_loss_backward")


def _iou_like(g, n, seed):
    """an fp32 [g, n] matrix in [0, 1] with exact ties and exact threshold hits"""
    rng = np.random.default_rng(seed)
    m = rng.random((g, n)).astype(F) ** 3
    if g > 2 and n > 8:
        m[2, 3] = m[0, 3] = m[:, 3].max() + F(0.01)           # a tie for the maximum: the first one wins
        m[:, 5] = 0.0                                          # all equal: index 0
        m[:, 6] = np.minimum(m[:, 6], F(0.5))
        m[1, 6] = 0.5                                          # the maximum exactly at fg_iou = 0.5: a match
        m[:, 7] = np.minimum(m[:, 7], F(0.3))
        m[g - 1, 7] = 0.3                                      # exactly at bg_iou = 0.3: between, not below
    return m


@pytest.mark.parametrize("fg,bg", [(0.5, 0.5), (0.6, 0.3)])
@pytest.mark.parametrize("g,n", [(1, 1), (1, 40), (37, 200), (5, 9)])
def test_match_equals_torch_max_and_thresholds(fg, bg, g, n):
    """matcher.py:85-95: torch.max(dim=0), then the two threshold masks"""
    iou = _iou_like(g, n, g * 1000 + n)
    mi, mv = R.match(iou, fg, bg)
    v32, matches = torch.from_numpy(iou).max(dim=0)
    matches = matches.clone()
    lo, hi = torch.tensor(bg, dtype=torch.float32), torch.tensor(fg, dtype=torch.float32)
    below, between = v32 < lo, (v32 >= lo) & (v32 < hi)
    matches[below] = -1
    matches[between] = -2
    assert (mv == v32.numpy()).all()
    # torch.max's index at ties is not pinned by its documentation: compared where the maximum is unique; the tie rule has
    # its own test below
    unique = (iou == iou.max(0, keepdims=True)).sum(0) == 1
    assert (mi[unique] == matches.numpy()[unique]).all()
    assert ((mi < 0) == (matches.numpy() < 0)).all() and (mi[mi < 0] == matches.numpy()[mi < 0]).all()
    if fg != bg and g > 2 and n > 8:
        assert mi[7] == -2 and mi[6] == (1 if fg == 0.5 else -2)
        assert (mi == -2).any() and (mi == -1).any()


def test_match_tie_rule_brute_force():
    """the first maximum wins: a plain loop with a strict `>`"""
    iou = _iou_like(9, 60, 5)
    iou[:, 10:12] = np.minimum(iou[:, 10:12], F(0.7))
    iou[4, 10] = iou[7, 10] = 0.9
    iou[0, 11] = iou[8, 11] = 0.75
    mi, mv = R.match(iou, 0.5, 0.5)
    for j in range(iou.shape[1]):
        best, bi = -np.inf, 0
        for i in range(iou.shape[0]):
            if iou[i, j] > best:
                best, bi = iou[i, j], i
        assert mv[j] == best
        assert mi[j] == (bi if best >= F(0.5) else -1)
    assert mi[10] == 4 and mi[11] == 0 and mi[3] == 0 and mi[5] == -1
    e, v = R.match(np.zeros((0, 4), F), 0.5, 0.5)
    assert e.tolist() == [-1] * 4 and v.tolist() == [0.0] * 4


def test_match_nan_entry_follows_torch_max():
    """a NaN entry is its column's maximum, the first one by index, and the proposal stays matched (both threshold
    comparisons are false): what torch.max followed by the reference's two masks does, and what k_roi_match states"""
    iou = _iou_like(9, 20, 11)
    iou[[6, 2], 4] = np.nan
    iou[8, 9] = np.nan
    mi, mv = R.match(iou, 0.6, 0.3)
    v32, matches = torch.from_numpy(iou).max(dim=0)
    assert mi[4] == 2 and mi[9] == 8 and np.isnan(mv[[4, 9]]).all() and np.isnan(mv).sum() == 2
    assert matches[4].item() == 2 and matches[9].item() == 8 and torch.isnan(v32[[4, 9]]).all()
    assert not ((v32 < 0.3) | ((v32 >= 0.3) & (v32 < 0.6)))[[4, 9]].any()
    assert R.labels_of(mi, np.arange(1, 10))[[4, 9]].tolist() == [3, 9]


def test_labels_and_sample_follow_the_reference_steps():
    """loss.py:213-222 with torch indexing; the sample is the sampler's two index sets merged ascending, and the counts
    are BalancedPositiveNegativeSampler's"""
    iou = _iou_like(12, 900, 8)
    tl = np.arange(12) % 3 + 1
    mi, _ = R.match(iou, 0.6, 0.3)
    lab = R.labels_of(mi, tl)
    t_mi = torch.from_numpy(mi)
    want = torch.from_numpy(tl)[t_mi.clamp(min=0)].clone()
    want[t_mi == -1] = 0
    want[t_mi == -2] = -1
    assert (lab == want.numpy()).all()
    assert R.labels_of(np.full(5, -1), np.zeros(0, np.int64)).tolist() == [0] * 5
    (rows, kp, kn), = R.sample([lab], 17, 64, 0.25)
    P, N = int((lab >= 1).sum()), int((lab == 0).sum())
    assert kp == min(P, 16) and kn == min(N, 64 - kp) and len(rows) == kp + kn
    assert (np.diff(rows) > 0).all() and (lab[rows] >= 0).all() and (lab[rows] >= 1).sum() == kp
    (rows2, _, _), = R.sample([lab], 18, 64, 0.25)
    assert rows.tolist() != rows2.tolist()


@pytest.mark.parametrize("class_specific", [True, False])
@pytest.mark.parametrize("c", [2, 4, 7])
def test_losses_equal_the_reference_composition_in_torch(class_specific, c):
    """F.cross_entropy and the map_inds indexing of loss.py:352-360 with smooth_l1 (beta 1/5, sum) / labels.numel(), float64
    autograd on the CPU"""
    rng = np.random.default_rng(c * 2 + class_specific)
    n = 300
    x = rng.normal(0, 2, (n, c))
    r = rng.normal(0, 0.3, (n, 7 * c if class_specific else 7))
    t = rng.normal(0, 0.3, (n, 7))
    lab = rng.integers(0, c, n)
    lab[:5] = 0
    cls, box, gx, gr, _, _ = R.loss_and_grads(x, r, lab, t, class_specific)
    tx, tr = torch.tensor(x, requires_grad=True), torch.tensor(r, requires_grad=True)
    tt, tlab = torch.tensor(t), torch.tensor(lab)
    pos = torch.nonzero(tlab > 0).squeeze(1)
    lp = tlab[pos]
    if class_specific:
        map_inds = 7 * lp[:, None] + torch.tensor([0, 1, 2, 3, 4, 5, 6])
        rp = tr[pos[:, None], map_inds]
    else:
        rp = tr[pos, :]
    d = torch.abs(rp - tt[pos])
    tbox = torch.where(d < R.BETA, 0.5 * d ** 2 / R.BETA, d - 0.5 * R.BETA).sum() / tlab.numel()
    tcls = TF.cross_entropy(tx, tlab)
    (tcls + tbox).backward()
    np.testing.assert_allclose([cls, box], [tcls.item(), tbox.item()], rtol=1e-12)
    np.testing.assert_allclose(gx, tx.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(gr, tr.grad.numpy(), rtol=1e-10, atol=1e-15)
    # a label out of range: nothing added, zero gradients in its row; the other rows unchanged up to the same divisor
    lab2 = lab.copy()
    lab2[7], lab2[9] = c, -3
    cls2, box2, gx2, gr2, ce2, bx2 = R.loss_and_grads(x, r, lab2, t, class_specific)
    assert ce2[7] == ce2[9] == bx2[7] == bx2[9] == 0 and not gx2[[7, 9]].any() and not gr2[[7, 9]].any()
    keep = np.ones(n, bool)
    keep[[7, 9]] = False
    assert (gx2[keep] == gx[keep]).all()
    e = R.loss_and_grads(np.zeros((0, c)), np.zeros((0, r.shape[1])), np.zeros(0, np.int64), np.zeros((0, 7)), class_specific)
    assert np.isnan(e[0]) and np.isnan(e[1])


def test_regression_targets_use_the_clamped_match():
    props = RP.wall_proposals(50, 3)
    tg = RP.wall_proposals(4, 4)
    mi = np.array([-1, -2, 3, 0] * 12 + [1, 2], np.int64)
    rt = R.regression_targets(mi, tg, props, (10, 10, 10, 5, 5, 5, 10))
    assert rt.dtype == F and rt.shape == (50, 7)
    import box_oracle as BO
    assert (rt[:2] == BO.encode_centroid_box(tg[[0, 0]], props[:2], (10, 10, 10, 5, 5, 5, 10))).all()
    assert (R.regression_targets(np.full(50, -1), np.zeros((0, 7), F), props) == 0).all()


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _hip._SIGS, name
    ver = int(re.search(r"#define AABR_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _hip.ABI_VERSION == 640
    lib = _hip.load()
    assert lib.aabr_version() == 640
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    # the number of arguments the header declares is the number the binding passes
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        nargs = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert nargs == len(_hip._SIGS[name][1]), name
    src = open(os.path.join(REPO, "automatic-as-built-reconstruction_amd", "csrc", "Makefile")).read()
    assert "roi_loss.hip" in src


def test_argument_validation_without_gpu():
    import _hip
    lib = _hip.load()
    assert lib.aabr_roi_targets_scratch_words(0) == -1 and lib.aabr_roi_targets_scratch_words(17) == -1
    assert lib.aabr_roi_targets_scratch_words(16) >= lib.aabr_rpn_loss_scratch_words(16) + 16 * 512 * 2

    def call(nb, B, num_pos):
        return lib.aabr_roi_targets(None, None, None, nb, None, None, None, -1, 1, 0.5, 0.5, None, 1, B, num_pos, None, None,
                                    None, None, None, None, None, None, None, None, None, None)
    assert call(0, 500, 125) == -1 and b"nb must be" in lib.aabr_last_error()
    assert call(17, 500, 125) == -1 and b"nb must be" in lib.aabr_last_error()
    assert call(4, 513, 125) == -1 and b"batch_size_per_image" in lib.aabr_last_error()
    assert call(4, 500, 501) == -1 and b"num_pos_max" in lib.aabr_last_error()
    assert call(4, 500, 125) == -1 and b"null" in lib.aabr_last_error()
    assert lib.aabr_roi_box_loss_forward(None, None, 0, 10, 0, 1, None, None, 0.2, None, None, None, None, None) == -1
    assert lib.aabr_roi_box_loss_forward(None, None, 0, 10, 4, 1, None, None, 0.0, None, None, None, None, None) == -1
    assert lib.aabr_roi_box_loss_forward(None, None, 0, 10, 4, 1, None, None, 0.2, None, None, None, None, None) == -1
    assert b"null" in lib.aabr_last_error()
    assert lib.aabr_roi_box_loss_scratch_floats() > 0


class _NS(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _cfg(corner=False, separate=(), yaw="Diff"):
    heads = _NS(FG_IOU_THRESHOLD=0.6, BG_IOU_THRESHOLD=0.3, BBOX_REG_WEIGHTS=(10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0),
                BATCH_SIZE_PER_IMAGE=500, POSITIVE_FRACTION=0.25, LABEL_AUG_THICKNESS_Y_TAR_ANC=[0.3, 0.1],
                LABEL_AUG_THICKNESS_Z_TAR_ANC=[0.4, 0.2])
    return _NS(MODEL=_NS(ROI_HEADS=heads, CORNER_ROI=corner, CLASS_SPECIFIC=True, SEPARATE_CLASSES_ID=list(separate),
                         LOSS=_NS(YAW_MODE=yaw), RPN=_NS(ADD_GT_PROPOSALS=True)),
               INPUT=_NS(CLASSES=["background", "wall", "door"]))


def test_python_surface_and_refusals():
    import roi_glue
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss import FastRCNNLossComputation, make_roi_box_loss_evaluator
    assert callable(roi_glue.box_head_targets) and callable(roi_glue.box_head_loss)
    assert (Matcher.BELOW_LOW_THRESHOLD, Matcher.BETWEEN_THRESHOLDS) == (-1, -2)
    m = Matcher(0.6, 0.3)
    assert (m.high_threshold, m.low_threshold, m.allow_low_quality_matches) == (0.6, 0.3, False)
    ev, sep = make_roi_box_loss_evaluator(_cfg())
    assert sep is None and isinstance(ev, FastRCNNLossComputation)
    assert (ev.high_threshold, ev.low_threshold, ev.class_specific, ev.need_seperate) == (0.6, 0.3, True, False)
    assert ev.aug_thickness == {"target_Y": 0.3, "anchor_Y": 0.1, "target_Z": 0.4, "anchor_Z": 0.2}
    assert ev.fg_bg_sampler.batch_size_per_image == 500 and ev.box_coder.weights.view(7).tolist()[3] == 5.0
    with pytest.raises(ValueError):
        make_roi_box_loss_evaluator(_cfg(corner=True))
    with pytest.raises(ValueError):
        make_roi_box_loss_evaluator(_cfg(separate=[2]))
    with pytest.raises(ValueError):
        make_roi_box_loss_evaluator(_cfg(yaw="SinDiff"))
    args = (Matcher(0.5, 0.5), BalancedPositiveNegativeSampler(500, 0.25), BoxCoder3D(False, None), "Diff", True,
            {"target_Y": 0, "target_Z": 0, "anchor_Y": 0, "anchor_Z": 0})
    with pytest.raises(ValueError):
        FastRCNNLossComputation(*args, _NS(need_seperate=True), True)
    FastRCNNLossComputation(*args, _NS(need_seperate=False), True)

    class Corner(object):
        is_corner_roi = True
        weights = None
    with pytest.raises(ValueError):
        FastRCNNLossComputation(args[0], args[1], Corner(), "Diff", True, args[5], None, True)
    ev = FastRCNNLossComputation(*args, None, True)
    with pytest.raises(ValueError):
        ev(torch.zeros(3, 4), torch.zeros(3, 28), torch.zeros(3, 16))          # corners_semantic is not None
    with pytest.raises(RuntimeError):
        ev(torch.zeros(3, 4), torch.zeros(3, 28), None)                         # before subsample
    with pytest.raises(ValueError):
        roi_glue.box_head_loss(torch.zeros(3, 4), torch.zeros(3, 28), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 7),
                               yaw_loss_mode="SinDiff")
