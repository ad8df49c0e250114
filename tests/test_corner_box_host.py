"""The corner form of the box coder and of the box head without a GPU.

csrc/corner_box.h compiled for the host (tests/corner_box_host_harness.cpp) -- the statement sequence the HIP kernels run
-- against
  * tests/golden/corner_golden.npz: the REFERENCE's own BoxCoder3D(True, w), Box3D_Torch and second_corner_box_* run on
    the CPU by tests/golden/gen_corner_golden.py (every vector of the fixture is the reference's; none is a restatement);
  * tests/corner_box_ref.py: the float64 restatement written from the cited lines, which also derives every bound used
    here from the fp32 operation sequence (its module docstring).
A comparison with the restatement is held to the bound B of one fp32 evaluation; a comparison with the reference's vector,
itself an fp32 evaluation (with fp32 sin / cos), to B + B_ref.  The decoded yaw's bound carries asin's condition number
1 / sqrt(1 - s^2) per element, evaluated from the restatement, and yaw is compared modulo pi.  No case is left out of any
comparison: the fixture keeps every box at least 1e-3 x length off the adjust_corner_order tie (asserted here too).

Then the modules: FPN2MLPFeatureExtractor, FPNPredictor and ROIBoxHead3D in corner form construct from
roi_glue.box_head_cfg(corner=True, resolution=(2, 11, 2)) with the reference's parameter names and shapes, and the
refusals that remain (corner-connection loss weights, a resolution whose second axis is not 11)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import corner_box_ref as R
from corner_box_host import CLIP, Host, build_harness

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW_SYMBOLS = ("aabr_box_to_2corners", "aabr_box_from_2corners", "aabr_box_encode_corner", "aabr_box_decode_corner",
               "aabr_roi_targets_coder", "aabr_roi_post_detections_coder", "aabr_roi_mlp_forward_window",
               "aabr_roi_mlp_backward_input_window", "aabr_roi_mlp_backward_weight_window")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "corner_golden.npz")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(build_harness(tmp_path_factory.mktemp("corner_host")))


def _within(name, diff, bound):
    print("%-28s worst |diff| %.3e, worst diff / bound %.3f over %d elements" % (name, diff.max(), (diff / np.maximum(bound, 1e-300)).max(), diff.size))
    bad = np.argwhere(diff > bound)
    assert bad.size == 0, "%s: %d elements beyond their bound, first at %s: diff %g > %g" % (
        name, len(bad), bad[0], diff[tuple(bad[0])], bound[tuple(bad[0])])


def test_fixture_inputs_keep_off_the_corner_order_tie_and_cover_the_branches(golden):
    for k in ("boxes", "anchors", "targets"):
        assert (R.tie_margin(golden[k]) >= 1e-3).all(), k
    yaw = golden["boxes"][:, 6]
    hp = np.float32(np.pi / 2)
    assert (yaw == 0).any() and (yaw == hp).any() and (yaw == -hp).any()          # -pi/2: the unrotated branch
    assert (np.abs(np.abs(yaw) - np.pi / 4) < 0.051).sum() >= 4                   # pi/4 +- 0.05 on both sides
    assert (golden["dec_enc"][:, 3:6] > CLIP).any()                              # one encoding beyond the clip
    assert golden["dec3_enc"].shape[1] == 21                                     # the 3-class layout
    assert golden["weights_w1"].tolist() == [1.0] * 7 and golden["weights_w2"].tolist() == [10, 10, 10, 5, 5, 5, 2]


def test_yxzb_to_2corners(golden, host):
    for k in ("boxes", "anchors", "targets"):
        b = golden[k]
        got = host.to_2corners(b)
        _within("to_2corners/restatement", np.abs(got - R.to_2corners(b)), R.corners_bound_rows(b))
        assert (got[:, 6] == b[:, 3]).all()                                      # the thickness is a copy
    _within("to_2corners/reference", np.abs(host.to_2corners(golden["boxes"]).astype(np.float64) - golden["corners"]),
            R.corners_bound_rows(golden["boxes"]) + R.corners_bound_rows(golden["boxes"], ref=True))
    # the unrotated branch is plain fp32 additions in the reference too: bit-equal there
    flat = golden["boxes"][:, 6] == -np.float32(np.pi / 2)
    assert flat.any() and (host.to_2corners(golden["boxes"])[flat] == golden["corners"][flat]).all()
    # a tie swaps (strict > 0): a wall along (1, -1) has component sum 0 at both ends
    # (at yaw - pi/2 = -pi/4; whether fp32 lands exactly on the tie depends on the length, so several are tried)
    tie = np.zeros((64, 7), np.float32)
    tie[:, 3], tie[:, 4], tie[:, 5], tie[:, 6] = 0.25, 0.5 + 0.25 * np.arange(64), 2, -np.pi / 4
    c = host.to_2corners(tie)
    on_tie = ((c[:, 0] - (c[:, 0] + c[:, 2]) / 2) + (c[:, 1] - (c[:, 1] + c[:, 3]) / 2)) == 0
    assert on_tie.any() and (c[on_tie, 0] > c[on_tie, 2]).all()                  # swapped: corner 0 is the +x end


def test_corners_to_yxzb_and_round_trip(golden, host):
    c = golden["corners"]
    got = host.from_2corners(c)
    _within("from_2corners/restatement", R.diff_rows(got, R.from_2corners(c)), R.from_corner_bounds(c))
    _within("from_2corners/reference", R.diff_rows(got, golden["boxes_back"]),
            R.from_corner_bounds(c) + R.from_corner_bounds(c, ref=True))
    # everything but the yaw is the same fp32 operations as CPU torch's: bit-equal to the reference
    assert (got[:, :6] == golden["boxes_back"][:, :6]).all()
    # yx_zb -> corners -> yx_zb returns the box: the corners carry E_xy / E_z into the way back
    b = golden["boxes"]
    exy, ez = R.corner_bounds(b)
    back = host.from_2corners(host.to_2corners(b))
    _within("round trip", R.diff_rows(back, b), R.from_corner_bounds(R.to_2corners(b), exy, ez))
    assert (np.abs(back[:, 6]) <= np.float32(np.pi / 2)).all()


def test_encode(golden, host):
    t, a = golden["targets"], golden["anchors"]
    for name in ("w1", "w2"):
        w = golden["weights_" + name]
        got = host.encode(t, a, w)
        _within("encode %s/restatement" % name, np.abs(got - R.encode(t, a, w)), R.encode_bounds(t, a, w))
        _within("encode %s/reference" % name, np.abs(got.astype(np.float64) - golden["enc_" + name]),
                R.encode_bounds(t, a, w) + R.encode_bounds(t, a, w, ref=True))
    # second_corner_box_encode itself (no weights) is the unit-weight coder
    _within("encode raw/reference", np.abs(host.encode(t, a, np.ones(7)).astype(np.float64) - golden["enc_raw"]),
            R.encode_bounds(t, a, np.ones(7)) + R.encode_bounds(t, a, np.ones(7), ref=True))
    # z0, z1 and thickness go through no rotation: bit-equal to the reference
    assert (host.encode(t, a, golden["weights_w2"])[:, 4:] == golden["enc_w2"][:, 4:]).all()


def test_decode(golden, host):
    a = golden["anchors"]
    for name in ("w1", "w2"):
        w, e = golden["weights_" + name], golden["dec_enc"]
        got = host.decode(e, a, w)
        _within("decode %s/restatement" % name, R.diff_rows(got, R.decode(e, a, w, CLIP)), R.decode_bounds(e, a, w, CLIP))
        _within("decode %s/reference" % name, R.diff_rows(got, golden["dec_" + name]),
                R.decode_bounds(e, a, w, CLIP) + R.decode_bounds(e, a, w, CLIP, ref=True))
    # the clamp acts at unit weights (20000 > 10000) and not at weight 5 (4000): z0 and z1 of that row differ by it
    assert np.isfinite(host.decode(golden["dec_enc"], a, golden["weights_w1"])[5]).all()
    e3, w = golden["dec3_enc"], golden["weights_w2"]
    got = host.decode(e3, a[:64], w)
    assert got.shape == (64, 21)
    _within("decode 3 classes/restatement", R.diff_rows(got, R.decode(e3, a[:64], w, CLIP)), R.decode_bounds(e3, a[:64], w, CLIP))
    _within("decode 3 classes/reference", R.diff_rows(got, golden["dec3_w2"]),
            R.decode_bounds(e3, a[:64], w, CLIP) + R.decode_bounds(e3, a[:64], w, CLIP, ref=True))
    # class c of row i is the single-class decode of its 7 columns against the same proposal
    for c in range(3):
        assert (host.decode(np.ascontiguousarray(e3[:, 7 * c:7 * c + 7]), a[:64], w) == got[:, 7 * c:7 * c + 7]).all()
    # decode(encode(t)) returns the target
    t = golden["targets"]
    enc = host.encode(t, a, w)
    eb = R.encode_bounds(t, a, w)
    back = host.decode(enc, a, w)
    # the encodings' own error, moved through the decode: |d corner| = d e / w x denominator
    an = R.to_2corners(a)
    xyd = np.hypot(an[:, 0] - an[:, 2], an[:, 1] - an[:, 3])
    azs = np.abs(an[:, 4] - an[:, 5])
    exy = (eb[:, 0:4] / w[0:4]).max(1) * xyd
    ez = (eb[:, 4:6] / w[4:6]).max(1) * azs
    eth = eb[:, 6] / w[6] * np.abs(a[:, 3])
    bound = R.decode_bounds(enc, a, w, CLIP) + R.from_corner_bounds(R.to_2corners(t), exy + R.corner_bounds(t)[0],
                                                                    ez + R.corner_bounds(t)[1], eth)
    _within("decode(encode)", R.diff_rows(back, t), bound)


def test_zero_size_anchor_gives_the_ieee_result(host):
    t = np.array([[1, 2, 0, 0.2, 3, 2.5, 0.3]], np.float32)
    flat = np.array([[1, 2, 0, 0.2, 3, 0.0, 0.3]], np.float32)                   # zero height
    point = np.array([[1, 2, 0, 0.2, 0.0, 2.5, 0.3]], np.float32)                # zero length
    with np.errstate(all="ignore"):
        e = host.encode(t, flat, np.ones(7))
        assert np.isfinite(e[0, :4]).all() and np.isinf(e[0, 5]) and not np.isfinite(e[0, 4])
        e = host.encode(t, point, np.ones(7))
        assert not np.isfinite(e[0, :4]).any() and np.isfinite(e[0, 4:]).all()


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_corner_modules_have_the_reference_parameters():
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import ROIBoxHead3D, build_roi_box_head
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    cfg = roi_glue.box_head_cfg(corner=True, resolution=(2, 11, 2))              # C = 8, R = 12, 3 classes
    # roi_box_feature_extractors.py:75-80,93-106: conv3d as in the centroid form; roi_all_cor_body = [11, 3, 7]
    ext = make_roi_box_feature_extractor(cfg)
    assert _shapes(ext) == {"conv3d.0.weight": (12, 8, 1, 1, 2), "conv3d.0.bias": (12,), "conv3d.1.weight": (12,),
                            "conv3d.1.bias": (12,), "fc6_cor.weight": (12, 12 * 2 * 3), "fc6_cor.bias": (12,),
                            "fc6_body.weight": (12, 12 * 2 * 7), "fc6_body.bias": (12,), "fc7_cor.weight": (12, 12),
                            "fc7_cor.bias": (12,), "fc7_body.weight": (12, 12), "fc7_body.bias": (12,)}
    assert list(ext.state_dict()) == ["conv3d.0.weight", "conv3d.0.bias", "conv3d.1.weight", "conv3d.1.bias",
                                      "fc6_cor.weight", "fc6_cor.bias", "fc6_body.weight", "fc6_body.bias",
                                      "fc7_cor.weight", "fc7_cor.bias", "fc7_body.weight", "fc7_body.bias"]
    for l in (ext.fc6_cor, ext.fc6_body, ext.fc7_cor, ext.fc7_body):             # kaiming_uniform_(a=1), zero bias
        bound = float(np.sqrt(3.0 / l.weight.shape[1]))
        assert (l.bias == 0).all() and float(l.weight.detach().abs().max()) <= bound
        assert float(l.weight.detach().abs().max()) > 0.8 * bound
    assert ext.fused and ext.corner_roi
    # roi_box_predictors.py:61-70, class specific and not
    pred = make_roi_box_predictor(cfg)
    assert _shapes(pred) == {"cls_score_body.weight": (3, 12), "cls_score_body.bias": (3,),
                             "bbox_pred_body.weight": (9, 12), "bbox_pred_body.bias": (9,),
                             "bbox_pred_cor.weight": (6, 12), "bbox_pred_cor.bias": (6,),
                             "bbox_corner_semantic.weight": (8, 12), "bbox_corner_semantic.bias": (8,),
                             "score_pred_cor.weight": (1, 12), "score_pred_cor.bias": (1,)}
    assert float(pred.cls_score_body.bias.detach().abs().max()) > 0               # nn.Linear's default initialisation
    pred = make_roi_box_predictor(roi_glue.box_head_cfg(corner=True, resolution=(2, 11, 2), class_specific=False))
    assert _shapes(pred)["bbox_pred_body.weight"] == (3, 12) and _shapes(pred)["bbox_pred_cor.weight"] == (2, 12)
    # at the reference's sizes
    big = roi_glue.box_head_cfg(C=128, corner=True, resolution=(5, 11, 4), R=512)
    s = _shapes(make_roi_box_feature_extractor(big))
    assert s["fc6_cor.weight"] == (512, 512 * 5 * 3) and s["fc6_body.weight"] == (512, 512 * 5 * 7)
    head = build_roi_box_head(cfg)
    assert isinstance(head, ROIBoxHead3D) and head.corner_roi
    assert set(k.split(".")[0] for k in head.state_dict()) == {"feature_extractor", "predictor"}
    assert head.loss_evaluator.box_coder.is_corner_roi and head.post_processor_.box_coder.is_corner_roi
    assert BoxCoder3D(True, None).is_corner_roi and not BoxCoder3D(False, None).is_corner_roi
    # what stays refused: the corner-connection losses, named by their weights; a second axis that is not 11
    for lw in ((1, 1, 1, 1, 1, 0, 0), (1, 1, 1, 1, 0, 0.5, 0), (1, 1, 1, 1, 0, 0, 2)):
        with pytest.raises(ValueError, match=r"LOSS\.WEIGHTS"):
            build_roi_box_head(roi_glue.box_head_cfg(corner=True, resolution=(2, 11, 2), loss_weights=lw))
    with pytest.raises(ValueError, match="11"):
        make_roi_box_feature_extractor(roi_glue.box_head_cfg(corner=True, resolution=(2, 10, 2)))
    with pytest.raises(ValueError, match=r"LOSS\.WEIGHTS"):
        head.loss_evaluator(torch.zeros(3, 3), torch.zeros(3, 21), torch.zeros(3, 16))
    # the centroid form does not look at the loss weights
    build_roi_box_head(roi_glue.box_head_cfg(loss_weights=(1, 1, 1, 1, 1, 1, 1)))


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640 == _hip.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name
    # the record of the window entry points: the header's fields in the binding's order
    body = re.search(r"typedef struct AabrMlpWindow \{(.*?)\} AabrMlpWindow;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for stmt in body.split(";") if stmt.strip()
             for n in stmt.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _hip.AabrMlpWindow._fields_]
    assert C.sizeof(_hip.AabrMlpWindow) == 40


def test_argument_checks_return_before_any_device_work():
    import _hip
    lib = _hip.load()
    one, E = 4096, -1                                                            # a non-null pointer nobody follows
    w = (C.c_float * 7)(*([1.0] * 7))
    assert lib.aabr_box_to_2corners(one, -1, one, None) == E
    assert lib.aabr_box_to_2corners(None, 3, one, None) == E and b"null" in lib.aabr_last_error()
    assert lib.aabr_box_to_2corners(None, 0, None, None) == 0
    assert lib.aabr_box_from_2corners(one, 3, None, None) == E
    assert lib.aabr_box_encode_corner(one, one, 3, None, one, None) == E
    assert lib.aabr_box_encode_corner(None, None, 0, w, None, None) == 0
    assert lib.aabr_box_decode_corner(one, one, 3, 0, w, 1e4, one, None) == E
    assert lib.aabr_box_decode_corner(one, None, 3, 1, w, 1e4, one, None) == E

    def win(n=4, ph=2, pw=11, R=12, wlen=3, blocks=2, w0=(0, 8)):
        v = _hip.AabrMlpWindow()
        v.n_rois, v.ph, v.pw, v.R, v.wlen, v.blocks = n, ph, pw, R, wlen, blocks
        v.w0[0], v.w0[1] = w0
        return v

    fwd, bi, bw = (lib.aabr_roi_mlp_forward_window, lib.aabr_roi_mlp_backward_input_window,
                   lib.aabr_roi_mlp_backward_weight_window)
    assert fwd(None, win(), one, None, 1, 12, one, None) == E and b"null" in lib.aabr_last_error()
    assert fwd(None, win(n=0), None, None, 1, 12, None, None) == 0               # no ROI: nothing to do
    for bad in (win(w0=(0, 9)), win(w0=(-1, 8)), win(blocks=3), win(blocks=0), win(wlen=0), win(wlen=12, blocks=1),
                win(ph=0), win(R=0), win(n=-1)):
        assert fwd(one, bad, one, None, 1, 12, one, None) == E and b"window" in lib.aabr_last_error()
        assert bi(one, None, one, bad, 12, -1, -1, one, None) == E
        assert bw(one, None, one, bad, 12, 0, one, None, None, None) == E
    assert fwd(one, None, one, None, 1, 12, one, None) == E
    assert fwd(one, win(R=3, ph=1, wlen=1, blocks=1), one, None, 1, 12, one, None) == E   # K = 3: not a multiple of 4
    assert bi(one, None, one, win(w0=(0, 2)), 12, -1, -1, one, None) == E and b"overlap" in lib.aabr_last_error()
    assert bi(one, None, one, win(), 12, 11, -1, one, None) == E                 # acc_w outside the pw axis
    assert bi(one, None, one, win(), 12, 2, 8, None, None) == E
    assert bw(one, None, one, win(), 12, 5, one, None, None, None) == E          # perm_hw does not divide K
    assert bw(one, None, one, win(n=300), 12, 6, one, None, None, None) == E and b"scratch" in lib.aabr_last_error()
