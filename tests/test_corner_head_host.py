"""The fp64 definition of the corner box head (tests/corner_head_ref.py), which the GPU tests hold the device to, against
float64 autograd of the reference's own statements: the modules' `fused = False` path (the reference's lines, torch on the
CPU) converted to float64.  Values and every gradient agree to float64 rounding, at N = 1 (the unsqueezed case: the
reference's squeeze() would drop the ROI axis there) and N = 5, class specific and not."""
import numpy as np
import pytest
import torch

import corner_head_ref as CH
import roi_mlp_ref as M


def _rel(a, b):
    b = np.asarray(b, np.float64)
    # (a floor of 1 on the scale: conv_b's gradient is zero in exact arithmetic, the BatchNorm removes the bias)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1.0))


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("class_specific", [True, False])
def test_definition_is_float64_autograd_of_the_reference_statements(n, class_specific):
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    torch.manual_seed(11)
    cfg = M.make_cfg(C=8, resolution=(2, 11, 2), R=12, corner=True, class_specific=class_specific)
    ext, pred = make_roi_box_feature_extractor(cfg), make_roi_box_predictor(cfg)
    with torch.no_grad():
        for prm in list(ext.parameters()) + list(pred.parameters()):
            if prm.dim() == 1:
                prm.uniform_(-0.5, 0.5)
        ext.conv3d[1].weight.uniform_(0.5, 1.5)
    # the definition takes every parameter at its float32 value: float32 values, float64 arithmetic
    p = {k: v.detach().numpy().copy() for k, v in CH.params_of(ext, pred).items()}
    ext.conv3d[1].eps = float(np.float32(ext.conv3d[1].eps))
    ext.double()
    pred.double()
    ext.fused = pred.fused = False
    ext.train()
    pooled = torch.randn(n, 8, 2, 11, 2).float().double().requires_grad_(True)
    x = ext.head(pooled)
    assert isinstance(x, list) and len(x) == 3 and all(tuple(v.shape) == (n, 12) for v in x)
    scores, reg, sem = pred(x)
    k = 3 if class_specific else 1
    assert tuple(scores.shape) == (n, 3) and tuple(reg.shape) == (n, 7 * k) and tuple(sem.shape) == (n, 16)
    rng = np.random.default_rng(5)
    g_s, g_r, g_m = (rng.standard_normal(tuple(t.shape)) for t in (scores, reg, sem))
    ((scores * torch.as_tensor(g_s)).sum() + (reg * torch.as_tensor(g_r)).sum() + (sem * torch.as_tensor(g_m)).sum()).backward()
    ref = CH.head(pooled.detach().numpy(), p, eps=ext.conv3d[1].eps, class_specific=class_specific, g_scores=g_s,
                  g_reg=g_r, g_sem=g_m)
    tol = 1e-11
    assert _rel(torch.cat([x[0], x[1]]).detach().numpy(), ref["x_cor"].v) < tol
    assert _rel(x[2].detach().numpy(), ref["x_body"].v) < tol
    assert _rel(scores.detach().numpy(), ref["scores"].v) < tol
    assert _rel(reg.detach().numpy(), ref["regression"].v) < tol
    assert _rel(sem.detach().numpy(), ref["semantics"].v) < tol
    assert _rel(pooled.grad.numpy(), ref["d_pooled"].v) < 1e-9
    for key, prm in CH.params_of(ext, pred).items():
        assert _rel(prm.grad.numpy(), ref["d_" + key].v) < 1e-9, key
    assert pred.score_pred_cor.weight.grad is None                               # never computed, as in the reference
    for v in ref.values():
        assert (v.s >= 0).all() and np.isfinite(v.s).all()


def test_windows_and_their_adjoint():
    rng = np.random.default_rng(0)
    n, ph, R = 3, 2, 4
    x = rng.standard_normal((n * ph * 11, R))
    X = torch.as_tensor(x).view(n, ph, 11, R).permute(0, 3, 1, 2)                # the reference's [n, R, ph, 11]
    for win, sl in ((CH.COR0, slice(0, 3)), (CH.BODY, slice(2, 9)), (CH.COR1, slice(8, 11))):
        want = X[:, :, :, sl].contiguous().view(n, -1).numpy()
        got = CH.window_cols(x, n, ph, R, win)
        assert np.array_equal(got, want)
        g = rng.standard_normal(got.shape)
        assert np.isclose((CH.window_scatter(g, n, ph, R, win).reshape(x.shape) * x).sum(), (g * got).sum())
