"""fp64 definition of the corner form of the box head's dense layers, with a per-element bound for every result: the values
of roi_mlp_ref.py's machinery (V = value + bound, linear_fwd / linear_bwd with the (K + 1) u sum |a w| GEMM bound, bn_fwd /
bn_bwd) arranged as the reference's corner statements.  tests/test_corner_head_host.py checks the values against float64
autograd of those statements themselves.

Definition (roi_box_feature_extractors.py:122-147, roi_box_predictors.py:79-103), X = relu(bn(conv(pooled))) [n, R, ph, 11]:
  cor0 = X[..., 0:3], body = X[..., 2:9], cor1 = X[..., 8:11], each `.contiguous().view(n, -1)`: column r (ph wlen) + h wlen + w
  x4_cor_i = relu(fc7_cor(relu(fc6_cor(cor_i)))), x4_body = relu(fc7_body(relu(fc6_body(body))))
  scores = cls_score_body(x4_body); body3 = bbox_pred_body(x4_body); cor_i2 = bbox_pred_cor(x4_cor_i);
  regression = [cor0 xy, cor1 xy, body3] per class ([n, 7 C] class specific, else [n, 7]);
  semantics = [bbox_corner_semantic(x4_cor0), bbox_corner_semantic(x4_cor1)]  [n, 16]
The two corners share their layers, so each corner layer is ONE layer over 2 n rows (corner 0's rows, then corner 1's):
that is how the device runs it and how the weight gradient's bound counts its reduction (M = 2 n).

The gradient into X adds the windows' contributions; at w = 2 and w = 8 two of them meet, added once in fp32 on the
device: bound = the two bounds + u (|corner term| + |body term|)."""
import numpy as np

import roi_mlp_ref as M

V, U = M.V, M.U
PW = 11
COR0, COR1, BODY = (0, 3), (8, 3), (2, 7)
OVERLAP = (2, 8)


def window_cols(x, n, ph, R, win):
    """rows [n ph 11, R] -> the window as the reference's view(n, -1): [n, R ph wlen]"""
    w0, wlen = win
    return x.reshape(n, ph, PW, R)[:, :, w0:w0 + wlen, :].transpose(0, 3, 1, 2).reshape(n, R * ph * wlen)


def window_scatter(g, n, ph, R, win):
    """the adjoint: [n, R ph wlen] -> [n, ph, 11, R], zero outside the window"""
    w0, wlen = win
    out = np.zeros((n, ph, PW, R))
    out[:, :, w0:w0 + wlen, :] = g.reshape(n, R, ph, wlen).transpose(0, 2, 3, 1)
    return out


def assemble(c0, c1, b3, n, nc, class_specific):
    if class_specific:
        return np.concatenate([c0.reshape(n, nc, 2), c1.reshape(n, nc, 2), b3.reshape(n, nc, 3)], 2).reshape(n, -1)
    return np.concatenate([c0, c1, b3], 1)


def split_regression(g, n, nc, class_specific):
    """the adjoint of assemble: -> (corner rows [2 n, 2 k], body [n, 3 k])"""
    k = nc if class_specific else 1
    g = g.reshape(n, k, 7)
    return (np.concatenate([g[:, :, 0:2].reshape(n, 2 * k), g[:, :, 2:4].reshape(n, 2 * k)], 0),
            g[:, :, 4:7].reshape(n, 3 * k))


def _two(da1, da2):
    """one GEMM over two weights concatenated along N: the sum of the two bounds covers it with one more rounding"""
    return V(da1.v + da2.v, da1.s + da2.s + U * (np.abs(da1.v) + np.abs(da2.v)))


def fc6_windows(x, p, n, ph, R, g_cor=None, g_body=None, sp=None):
    """the two fc6 over windows of x = V rows [n ph 11, R].  Returns a dict of V: y_cor [2 n, .], y_body [n, .] (after the
    ReLU) and, given the gradients of those, d_x [n ph 11, R] and the four parameter gradients."""
    sp = sp or {}
    win = lambda q, w: window_cols(q, n, ph, R, w)
    x2c = V(np.concatenate([win(x.v, COR0), win(x.v, COR1)]), np.concatenate([win(x.s, COR0), win(x.s, COR1)]))
    x2b = V(win(x.v, BODY), win(x.s, BODY))
    y_cor, pre_c = M.linear_fwd(x2c, p["fc6_cor_w"], p["fc6_cor_b"], relu=True)
    y_body, pre_b = M.linear_fwd(x2b, p["fc6_body_w"], p["fc6_body_b"], relu=True)
    out = {"y_cor": y_cor, "y_body": y_body, "pre_cor": pre_c, "pre_body": pre_b, "x2_cor": x2c, "x2_body": x2b}
    if g_cor is None:
        return out
    g2c, out["d_fc6_cor_w"], out["d_fc6_cor_b"] = M.linear_bwd(g_cor, pre_c, x2c, p["fc6_cor_w"], sp.get("fc6_cor", 1))
    g2b, out["d_fc6_body_w"], out["d_fc6_body_b"] = M.linear_bwd(g_body, pre_b, x2b, p["fc6_body_w"], sp.get("fc6_body", 1))
    sc = lambda q, w: window_scatter(q, n, ph, R, w)
    cor_v = sc(g2c.v[:n], COR0) + sc(g2c.v[n:], COR1)            # the corner windows do not overlap each other
    cor_s = sc(g2c.s[:n], COR0) + sc(g2c.s[n:], COR1)
    body_v, body_s = sc(g2b.v, BODY), sc(g2b.s, BODY)
    both = np.zeros((1, 1, PW, 1))
    both[0, 0, list(OVERLAP), 0] = 1.0
    s = cor_s + body_s + both * U * (np.abs(cor_v) + np.abs(body_v))
    out["d_x"] = V((cor_v + body_v).reshape(n * ph * PW, R), s.reshape(n * ph * PW, R))
    return out


def head(pooled, p, eps=1e-5, class_specific=True, g_scores=None, g_reg=None, g_sem=None, dw_splits=None, stats_u=0.0):
    """pooled [n, C, ph, 11, pz] (the device's own: exact input); p: fp32 parameters in the reference's layouts -- conv_w,
    conv_b, bn_w, bn_b, fc6_cor_w/b, fc6_body_w/b, fc7_cor_w/b, fc7_body_w/b, cls_w/b (cls_score_body), body_w/b
    (bbox_pred_body), cor_w/b (bbox_pred_cor), sem_w/b (bbox_corner_semantic).  dw_splits: layer -> the device's split
    count of that weight gradient.  Returns a dict of V."""
    sp = dw_splits or {}
    n, c, ph, pw, pz = pooled.shape
    assert pw == PW
    R, nc = p["conv_w"].shape[0], p["cls_w"].shape[0]
    A = V(M.pooled_rows(pooled))
    wc = np.asarray(p["conv_w"], np.float64).reshape(R, c * pz)
    x1, _ = M.linear_fwd(A, wc, p["conv_b"])
    x1n, r = M.bn_fwd(x1, p["bn_w"], p["bn_b"], eps, stats_u=stats_u)
    f6 = fc6_windows(x1n, p, n, ph, R)
    x4c, pre4c = M.linear_fwd(f6["y_cor"], p["fc7_cor_w"], p["fc7_cor_b"], relu=True)
    x4b, pre4b = M.linear_fwd(f6["y_body"], p["fc7_body_w"], p["fc7_body_b"], relu=True)
    scores, _ = M.linear_fwd(x4b, p["cls_w"], p["cls_b"])
    b3, _ = M.linear_fwd(x4b, p["body_w"], p["body_b"])
    c2, _ = M.linear_fwd(x4c, p["cor_w"], p["cor_b"])
    sem, _ = M.linear_fwd(x4c, p["sem_w"], p["sem_b"])
    asm = lambda q: assemble(q(c2)[:n], q(c2)[n:], q(b3), n, nc, class_specific)
    out = {"x_cor": x4c, "x_body": x4b, "scores": scores, "regression": V(asm(lambda t: t.v), asm(lambda t: t.s)),
           "semantics": V(np.concatenate([sem.v[:n], sem.v[n:]], 1), np.concatenate([sem.s[:n], sem.s[n:]], 1))}
    if g_scores is None:
        return out
    g_c2, g_b3 = split_regression(np.asarray(g_reg, np.float64), n, nc, class_specific)
    g_semr = np.concatenate([g_sem[:, :8], g_sem[:, 8:]], 0)
    da1, out["d_cls_w"], out["d_cls_b"] = M.linear_bwd(V(g_scores), None, x4b, p["cls_w"], sp.get("pred_body", 1))
    da2, out["d_body_w"], out["d_body_b"] = M.linear_bwd(V(g_b3), None, x4b, p["body_w"], sp.get("pred_body", 1))
    da3, out["d_cor_w"], out["d_cor_b"] = M.linear_bwd(V(g_c2), None, x4c, p["cor_w"], sp.get("pred_cor", 1))
    da4, out["d_sem_w"], out["d_sem_b"] = M.linear_bwd(V(g_semr), None, x4c, p["sem_w"], sp.get("pred_cor", 1))
    g3b, out["d_fc7_body_w"], out["d_fc7_body_b"] = M.linear_bwd(_two(da1, da2), pre4b, f6["y_body"], p["fc7_body_w"],
                                                                 sp.get("fc7_body", 1))
    g3c, out["d_fc7_cor_w"], out["d_fc7_cor_b"] = M.linear_bwd(_two(da3, da4), pre4c, f6["y_cor"], p["fc7_cor_w"],
                                                               sp.get("fc7_cor", 1))
    out.update({k: v for k, v in fc6_windows(x1n, p, n, ph, R, g3c, g3b, sp).items() if k.startswith("d_")})
    g1, out["d_bn_w"], out["d_bn_b"] = M.bn_bwd(out["d_x"], x1, r, p["bn_w"])
    dA, dwc, out["d_conv_b"] = M.linear_bwd(g1, None, A, wc, sp.get("conv", 1))
    out["d_conv_w"] = V(dwc.v.reshape(p["conv_w"].shape), dwc.s.reshape(p["conv_w"].shape))
    out["d_pooled"] = V(M.rows_pooled(dA.v, pooled.shape), M.rows_pooled(dA.s, pooled.shape))
    return out


PARAMS = {"conv_w": "feature_extractor.conv3d.0.weight", "conv_b": "feature_extractor.conv3d.0.bias",
          "bn_w": "feature_extractor.conv3d.1.weight", "bn_b": "feature_extractor.conv3d.1.bias",
          "fc6_cor_w": "feature_extractor.fc6_cor.weight", "fc6_cor_b": "feature_extractor.fc6_cor.bias",
          "fc6_body_w": "feature_extractor.fc6_body.weight", "fc6_body_b": "feature_extractor.fc6_body.bias",
          "fc7_cor_w": "feature_extractor.fc7_cor.weight", "fc7_cor_b": "feature_extractor.fc7_cor.bias",
          "fc7_body_w": "feature_extractor.fc7_body.weight", "fc7_body_b": "feature_extractor.fc7_body.bias",
          "cls_w": "predictor.cls_score_body.weight", "cls_b": "predictor.cls_score_body.bias",
          "body_w": "predictor.bbox_pred_body.weight", "body_b": "predictor.bbox_pred_body.bias",
          "cor_w": "predictor.bbox_pred_cor.weight", "cor_b": "predictor.bbox_pred_cor.bias",
          "sem_w": "predictor.bbox_corner_semantic.weight", "sem_b": "predictor.bbox_corner_semantic.bias"}


def params_of(ext, pred):
    """the definition's parameter dict (torch tensors) of a corner extractor and predictor"""
    named = {"feature_extractor." + k: v for k, v in ext.named_parameters()}
    named.update({"predictor." + k: v for k, v in pred.named_parameters()})
    return {k: named[v] for k, v in PARAMS.items()}
