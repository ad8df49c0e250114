"""The box head's dense layers without a GPU: the fp64 definition (tests/roi_mlp_ref.py) against torch's CPU modules in
float64, the new modules' state_dict against a list typed out from the reference's files, their refusals, and the new
C-ABI symbols (header, binding, library, argument checks that return before any HIP call)."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import roi_mlp_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aabr_roi_mlp_tile", "aabr_roi_mlp_dw_splits", "aabr_roi_mlp_dw_scratch_floats", "aabr_roi_mlp_forward",
               "aabr_roi_mlp_backward_input", "aabr_roi_mlp_backward_weight", "aabr_roi_mlp_pack_fc6")


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("n,C,res,R,nc,spec", [(5, 8, (2, 3, 2), 12, 3, True), (3, 5, (3, 2, 4), 8, 4, False)])
def test_definition_agrees_with_torch_float64_modules(n, C, res, R, nc, spec):
    torch.manual_seed(7)
    ph, pw, pz = res
    conv = nn.Sequential(nn.Conv3d(C, R, kernel_size=[1, 1, pz], stride=[1, 1, 1]),
                         nn.BatchNorm3d(R, track_running_stats=False), nn.ReLU(inplace=True))
    fc6, fc7 = nn.Linear(R * ph * pw, R), nn.Linear(R, R)
    cls, reg = nn.Linear(R, nc), nn.Linear(R, 7 * nc if spec else 7)
    with torch.no_grad():
        conv[1].weight.uniform_(0.5, 1.5)
        conv[1].bias.uniform_(-0.5, 0.5)
    # the definition takes every parameter at its float32 value (fp64_yardstick.f32): float32 values, float64 arithmetic
    conv[1].eps = float(np.float32(conv[1].eps))
    for m in (conv, fc6, fc7, cls, reg):
        m.double()
    pooled = torch.randn(n, C, ph, pw, pz, dtype=torch.float64, requires_grad=True)
    x1 = conv(pooled)
    x4 = torch.relu(fc7(torch.relu(fc6(x1.view(x1.size(0), -1)))))
    logits, deltas = cls(x4), reg(x4)
    g_l, g_d = torch.randn_like(logits), torch.randn_like(deltas)
    ((logits * g_l).sum() + (deltas * g_d).sum()).backward()
    mods = {"conv": conv[0], "bn": conv[1], "fc6": fc6, "fc7": fc7, "cls": cls, "reg": reg}
    p = {"%s_%s" % (k, "w" if a == "weight" else "b"): getattr(m, a).detach().numpy() for k, m in mods.items()
         for a in ("weight", "bias")}
    out = M.head(pooled.detach().numpy(), p, eps=conv[1].eps, g_logits=g_l.numpy(), g_deltas=g_d.numpy())
    assert _rel(out["x4"].v, x4.detach().numpy()) < 1e-12
    assert _rel(out["logits"].v, logits.detach().numpy()) < 1e-12 and _rel(out["deltas"].v, deltas.detach().numpy()) < 1e-12
    for k, m in mods.items():
        assert _rel(out["d_%s_w" % k].v, m.weight.grad.numpy()) < 1e-12, k
        if k == "conv":      # BatchNorm removes the mean: this gradient is a sum that cancels to zero, so measure it
            scale = np.abs(out["d_conv_w"].v).max()                             # against the layer's gradient scale
            assert np.abs(out["d_conv_b"].v - m.bias.grad.numpy()).max() < 1e-12 * scale
            continue
        assert _rel(out["d_%s_b" % k].v, m.bias.grad.numpy()) < 1e-12, k
    assert _rel(out["d_pooled"].v, pooled.grad.numpy()) < 1e-12
    for v in out.values():
        assert (v.s >= 0).all() and np.isfinite(v.s).all()


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_keys_and_shapes_are_the_reference_modules():
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    # roi_box_feature_extractors.py:75-85 at nPlaneMap 128, (5, 11, 4), MLP_HEAD_DIM 512; TRACK_RUNNING_STATS False
    ext = make_roi_box_feature_extractor(M.make_cfg(C=128, resolution=(5, 11, 4), R=512, track=False))
    assert _shapes(ext) == {"conv3d.0.weight": (512, 128, 1, 1, 4), "conv3d.0.bias": (512,), "conv3d.1.weight": (512,),
                            "conv3d.1.bias": (512,), "fc6.weight": (512, 28160), "fc6.bias": (512,),
                            "fc7.weight": (512, 512), "fc7.bias": (512,)}
    assert ext.fused and ext.pooler.box_scale == 1.0 and (ext.fc6.bias == 0).all() and (ext.fc7.bias == 0).all()
    ext = make_roi_box_feature_extractor(M.make_cfg(C=8, resolution=(2, 3, 2), R=12, track=True))
    assert _shapes(ext) == {"conv3d.0.weight": (12, 8, 1, 1, 2), "conv3d.0.bias": (12,), "conv3d.1.weight": (12,),
                            "conv3d.1.bias": (12,), "conv3d.1.running_mean": (12,), "conv3d.1.running_var": (12,),
                            "conv3d.1.num_batches_tracked": (), "fc6.weight": (12, 72), "fc6.bias": (12,),
                            "fc7.weight": (12, 12), "fc7.bias": (12,)}
    # roi_box_predictors.py:37-58
    pred = make_roi_box_predictor(M.make_cfg(R=12, classes=("background", "wall", "door"), class_specific=True))
    assert _shapes(pred) == {"cls_score.weight": (3, 12), "cls_score.bias": (3,), "bbox_pred.weight": (21, 12),
                             "bbox_pred.bias": (21,)} and pred.num_classes == 3 and pred.fused
    pred = make_roi_box_predictor(M.make_cfg(R=12, class_specific=False))
    assert _shapes(pred)["bbox_pred.weight"] == (7, 12) and _shapes(pred)["cls_score.weight"] == (3, 12)
    pred = make_roi_box_predictor(M.make_cfg(R=12, class_specific=True, separate=("door",)))
    assert _shapes(pred)["cls_score.weight"] == (4, 12) and _shapes(pred)["bbox_pred.weight"] == (28, 12)
    assert float(pred.cls_score.weight.detach().std()) < 0.05 and (pred.bbox_pred.bias == 0).all()


def test_box_head_builds_and_refuses_what_is_not_part_of_it():
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import ROIBoxHead3D, build_roi_box_head
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    head = build_roi_box_head(M.make_cfg())
    assert isinstance(head, ROIBoxHead3D)
    assert set(k.split(".")[0] for k in head.state_dict()) == {"feature_extractor", "predictor"}
    for make in (make_roi_box_feature_extractor, make_roi_box_predictor, build_roi_box_head):
        with pytest.raises(ValueError, match="CORNER_ROI"):
            make(M.make_cfg(corner=True))
    with pytest.raises(ValueError, match="FEATURE_EXTRACTOR"):
        make_roi_box_feature_extractor(M.make_cfg(extractor="ResNet50Conv5ROIFeatureExtractor"))
    with pytest.raises(ValueError, match="PREDICTOR"):
        make_roi_box_predictor(M.make_cfg(predictor="FastRCNNPredictor"))
    with pytest.raises(ValueError, match="eval_in_train"):
        build_roi_box_head(M.make_cfg(eval_in_train=1))


def test_glue_refuses_bf16_before_it_needs_a_gpu():
    import roi_glue
    x, w = torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(3, 8)
    with pytest.raises(TypeError):
        roi_glue.dense_linear(x, w, None, False)
    with pytest.raises(TypeError):
        roi_glue.box_predictions(x, w, None, w, None)
    with pytest.raises(TypeError):
        roi_glue.box_head_mlp(torch.zeros(1, 4, 1, 1, 2, dtype=torch.bfloat16), torch.zeros(4, 4, 1, 1, 2), None, None,
                              None, {}, torch.zeros(4, 4), None, torch.zeros(4, 4), None)


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name


def test_dispatch_functions_and_argument_checks():
    import _hip
    lib = _hip.load()
    t = lib.aabr_roi_mlp_tile
    assert t(0, 5) == 0 and t(1, 1) == 64 and t(128 * 191, 128) == 64 and t(128 * 191 + 1, 128) == 128
    assert t(110000, 512) == 128 and t(2000, 512) == 64
    s = lib.aabr_roi_mlp_dw_splits
    assert s(0, 4, 4) == 0 and s(256, 1, 4) == 1 and s(257, 1, 4) == 2 and s(10 ** 6, 1, 4) == 64
    assert s(2000, 512, 28160) == 1 and s(110000, 512, 512) == 8
    for (m, n, k) in ((257, 1, 4), (2000, 512, 512), (110000, 512, 512), (24449, 3, 8)):
        sp = s(m, n, k)
        per = -(-(-(-m // sp)) // 32) * 32
        assert per * (sp - 1) < m <= per * sp                                   # whole chunks, no empty run
        assert lib.aabr_roi_mlp_dw_scratch_floats(m, n, k) == (sp * (n * k + n) if sp > 1 else 0)
    one = 4096                                                                   # a non-null pointer nobody follows
    fwd, bi, bw = lib.aabr_roi_mlp_forward, lib.aabr_roi_mlp_backward_input, lib.aabr_roi_mlp_backward_weight
    E = -1
    assert fwd(one, 0, 0, 0, one, None, 0, 4, 3, 6, one, None) == E and b"multiple of 4" in lib.aabr_last_error()
    assert fwd(one, 0, 0, 0, one, None, 0, 4, 3, 0, one, None) == E
    assert fwd(one, 0, 0, 0, one, None, 0, -1, 3, 8, one, None) == E
    assert fwd(one, 0, 0, 0, one, None, 0, 4, 0, 8, one, None) == E
    assert fwd(None, 0, 0, 0, one, None, 0, 4, 3, 8, one, None) == E and b"null" in lib.aabr_last_error()
    assert fwd(one, 2, 0, 0, one, None, 0, 4, 3, 8, one, None) == E
    assert fwd(one, 1, 3, 2, one, None, 0, 4, 3, 8, one, None) == E              # M is no multiple of hw
    assert fwd(one, 1, 2, 3, one, None, 0, 4, 3, 8, one, None) == E              # K is no multiple of pz
    assert fwd(None, 0, 0, 0, None, None, 0, 0, 3, 8, None, None) == 0           # M == 0: nothing to do
    assert bi(one, None, None, 4, 3, 8, 0, 0, 0, one, None) == E
    assert bi(one, None, one, 4, 3, 10, 0, 0, 0, one, None) == E
    assert bi(None, None, None, 0, 3, 8, 0, 0, 0, None, None) == 0
    assert bw(one, None, one, 0, 0, 0, 4, 3, 8, 0, None, None, None, None) == E
    assert bw(one, None, one, 0, 0, 0, 4, 3, 8, 3, one, None, None, None) == E   # perm_hw does not divide K
    assert bw(one, None, one, 0, 0, 0, 300, 3, 8, 0, one, None, None, None) == E and b"scratch" in lib.aabr_last_error()
    assert lib.aabr_roi_mlp_pack_fc6(None, 4, 4, 4, one, None) == E
    assert lib.aabr_roi_mlp_pack_fc6(one, 0, 4, 4, one, None) == E
