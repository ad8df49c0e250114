"""fp64 definition of the box head's dense layers (FPN2MLPFeatureExtractor after its pooler and FPNPredictor), written
from the reference's modules line by line, with a per-element SLACK for every result.

Definition (roi_box_feature_extractors.py:75-80, 152-157; roi_box_predictors.py:105-109):
  x1[n, r, h, w] = sum over (c, z) of pooled[n, c, h, w, z] * conv_w[r, c, 0, 0, z] + conv_b[r]      Conv3d([1, 1, pz])
  BatchNorm3d over (n, h, w) per r, biased variance, then ReLU                                         (fp64_yardstick)
  x2 = x1.view(N, -1): column r * hw + s with s = h * pw + w, the reference's (r, h, w) order
  x3 = relu(x2 fc6_w^T + fc6_b), x4 = relu(x3 fc7_w^T + fc7_b); logits = x4 cls_w^T + cls_b, deltas = x4 reg_w^T + reg_b

Slack, u = 2^-24.  The fp32-input MFMA is a bitwise fmaf chain (one rounding per step), so a length-K dot product plus
bias computed in ANY order of fused or unfused steps is within (K + 1) u (sum |a_k w_k| + |bias|) of exact (the
standard gamma_n bound with n = K + 1 roundings on the longest path; terms of order u^2 are dropped throughout).  A
reduction split into S partial chains whose results are then added in order puts at most ceil(K / S) + S roundings on a
path, which (K + S) covers.  ReLU adds nothing.  An input that itself carries a bound s_a adds sum |w_k| s_a_k (first
order).  Backward, for a layer with g = dY:
  masked g: where the forward value y is within its own bound of zero the device may take either branch, so the masked
            gradient is off by up to |g| there: s_gm = s_g where y > s_y, 0 where y < -s_y, |g| + s_g otherwise
  dA = gm W       (N + 1) u (|gm| |W|)        + s_gm |W|
  dW = gm^T A     (M + S) u (|gm|^T |A|)      + s_gm^T |A| + |gm|^T s_A + s_gm^T s_A
  db = 1^T gm     (M + S) u sum |gm|          + sum s_gm
BatchNorm: fp64_yardstick.bn_forward_exact / bn_backward_exact give the kernel's own arithmetic bound for exact inputs;
an input bound s_x reaches the output to first order through y = a (x - mean) invstd:
  |dy_i| <= |a| (s_i + mean(s) + |xh_i| mean(|xh| s)),  xh = (x - mean) invstd
and the backward pass d_in = sw (d - mean(d) - xh mean(xh d)) moves by
  |sw| (s_d_i + mean(s_d) + |xh_i| mean(|xh| s_d))                        from the bound s_d on d
  |sw| (s_xh_i |mean(xh d)| + |xh_i| mean(s_xh |d|)) + e |d_in_i|           from the bound on xh and on invstd,
  s_xh_i = invstd (s_i + mean(s)) + |xh_i| e,  e = invstd^2 mean(|x - mean| s)  (the relative change of invstd)
with the same terms (summed) for dw = sum xh d and db = sum d.

The torch composition (`fused = False`), the other side of the fused-against-torch comparison, obeys the GEMM bounds
(any summation order) but NOT the BatchNorm ones: its BatchNorm takes the batch statistics in fp32, the library in fp64.
`stats_u = u` adds what fp32 statistics by any of the usual algorithms can cost (n rows per plane):
  mean:      n - 1 additions and a division            |dmean| <= (n + 2) u mean|x|
  variance:  the one-pass form E[x^2] - mean^2 is the worst: (n + 1) u mean(x^2) for E[x^2], 2 |mean| |dmean| + u mean^2
             <= (2 n + 5) u mean(x^2) for the square (mean^2 and |mean| mean|x| are both <= mean(x^2)), u for the
             subtraction: <= 4 (n + 2) u mean(x^2); two-pass and Welford forms stay below it
             -> relative change of invstd  e32 = dvar / (2 (var + eps))
  forward:   xh moves by invstd |dmean| + |xh| e32, the output by |weight| times that; both join s_xh and e above
  backward:  sum d and sum xh d in fp32: (n + 1) u sum|d| and (n + 2) u sum|xh d|, which enter d_in through
             sw (. / n + |xh| . / n), and dw, db directly.
A plane whose variance is far below mean(x^2) makes e32 large (1e-2 at the 1-ROI case), so for it the first-order form
is not enough: invstd' / invstd = (1 + t)^(-1/2) with |t| <= 2 e32 moves by at most e32 (1 - 2 e32)^(-3/2), which
replaces e32, and the backward pass keeps the products of two such changes (s_xh s_xh |d| and e times the first-order
terms).  Products of e32 with u are dropped.
"""
import numpy as np

import fp64_yardstick as Y

U = Y.U
F = np.float32


class V(object):
    """a value in fp64 and the bound on the device's distance from it"""

    def __init__(self, v, s=None):
        self.v = np.asarray(v, np.float64)
        self.s = np.zeros_like(self.v) if s is None else np.asarray(s, np.float64)


def pooled_rows(pooled):
    """[n, C, ph, pw, pz] -> the GEMM operand [n hw, C pz]: row n hw + s, column c pz + z"""
    n, c, ph, pw, pz = pooled.shape
    return np.asarray(pooled, np.float64).transpose(0, 2, 3, 1, 4).reshape(n * ph * pw, c * pz)


def rows_pooled(a, shape):
    n, c, ph, pw, pz = shape
    return a.reshape(n, ph, pw, c, pz).transpose(0, 3, 1, 2, 4)


def linear_fwd(a, w, b=None, relu=False):
    """a: V [M, K]; w [N, K], b [N] or None (exact fp32 parameters).  Returns V [M, N] (after the ReLU when relu) and the
    pre-activation V the backward mask needs."""
    w = np.asarray(w, np.float64)
    K = w.shape[1]
    bb = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    y = a.v @ w.T + bb
    s = (K + 1) * U * (np.abs(a.v) @ np.abs(w).T + np.abs(bb)) + a.s @ np.abs(w).T
    pre = V(y, s)
    return (V(np.maximum(y, 0.0), s) if relu else pre), pre


UNDECIDED = []      # (elements whose ReLU branch the bound leaves open, elements) of every masked() since the last clear


def undecided_share():
    """the share of ReLU inputs since the last UNDECIDED.clear() that lay within their own bound of zero: there the
    masked gradient's bound is the whole gradient, which passes whatever the device returns -- callers cap it at 1 %"""
    return sum(u for u, _ in UNDECIDED) / max(1, sum(t for _, t in UNDECIDED))


def masked(g, pre):
    """g: V (dY); pre: V of the forward pre-activation, or None (no ReLU)"""
    if pre is None:
        return g
    on, off = pre.v > pre.s, pre.v < -pre.s
    UNDECIDED.append((int((~on & ~off).sum()), int(on.size)))
    gm = np.where(pre.v > 0, g.v, 0.0)
    return V(gm, np.where(on, g.s, np.where(off, 0.0, np.abs(g.v) + g.s)))


def linear_bwd(g, pre, a, w, splits=1):
    """gradients of act(a w^T + b): returns (dA, dW, db) as V"""
    w = np.asarray(w, np.float64)
    gm = masked(g, pre)
    M, N = gm.v.shape
    d_a = V(gm.v @ w, (N + 1) * U * (np.abs(gm.v) @ np.abs(w)) + gm.s @ np.abs(w))
    k = (M + splits) * U
    d_w = V(gm.v.T @ a.v, k * (np.abs(gm.v).T @ np.abs(a.v)) + gm.s.T @ np.abs(a.v) + np.abs(gm.v).T @ a.s + gm.s.T @ a.s)
    d_b = V(gm.v.sum(0), k * np.abs(gm.v).sum(0) + gm.s.sum(0))
    return d_a, d_w, d_b


def bn_fwd(x, weight, bias, eps, train=True, running_mean=None, running_var=None, momentum=0.9, stats_u=0.0):
    """x: V [rows, R].  BatchNorm + ReLU; returns (V out, the yardstick's dict with xh / e added)"""
    r = Y.bn_forward_exact(x.v, weight, bias, eps=eps, momentum=momentum, leak=0.0, train=train,
                           running_mean=running_mean, running_var=running_var)
    xm = x.v - r["mean"]
    xh = xm * r["invstd"]
    s = x.s
    if train:
        prop = np.abs(r["a"]) * (s + s.mean(0) + np.abs(xh) * (np.abs(xh) * s).mean(0))
        r["e"] = r["invstd"] ** 2 * (np.abs(xm) * s).mean(0)
        r["s_xh"] = r["invstd"] * (s + s.mean(0)) + np.abs(xh) * r["e"]
    else:
        prop = np.abs(r["a"]) * s
        r["e"], r["s_xh"] = np.zeros(x.v.shape[1]), r["invstd"] * s
    r["stats_u"] = stats_u
    if train and stats_u:
        n = x.v.shape[0]
        mean_err = (n + 2) * stats_u * np.abs(x.v).mean(0)
        e32 = 4 * (n + 2) * stats_u * (x.v * x.v).mean(0) / (2 * (r["var"] + float(Y.f32(eps))))
        with np.errstate(divide="ignore", invalid="ignore"):
            e32 = np.where(2 * e32 < 1, e32 * (1 - 2 * e32) ** -1.5, np.inf)
        d_xh = r["invstd"] * mean_err + np.abs(xh) * e32
        prop = prop + np.abs(1.0 if weight is None else Y.f32(weight)) * d_xh
        r["e"], r["s_xh"] = r["e"] + e32, r["s_xh"] + d_xh
    r["xh"], r["s_y"] = xh, r["slack"] + prop
    return V(r["out"], r["s_y"]), r


def bn_bwd(g, x, r, weight):
    """g: V d_out; x: V input; r: bn_fwd's dict (training).  Returns (d_in, dw, db) as V"""
    pre = V(r["y"], r["s_y"])
    d = masked(g, pre)
    b = Y.bn_backward_exact(x.v, r["y"], g.v, r["mean"], r["invstd"], weight, leak=0.0)
    sw = np.abs(r["invstd"] * (1.0 if weight is None else Y.f32(weight)))
    xh, s_xh, e = r["xh"], r["s_xh"], r["e"]
    # the yardstick's backward takes the saved mean / invstd at their float32 values (the device's); the definition's
    # VALUES are formed here from the exact ones, its kernel-arithmetic bounds are the yardstick's
    wv = 1.0 if weight is None else Y.f32(weight)
    dot = (xh * d.v).sum(0)
    b["d_in"] = (d.v - d.v.mean(0) - xh * dot / x.v.shape[0]) * r["invstd"] * wv
    b["dw"], b["db"] = dot, d.v.sum(0)
    from_d = sw * (d.s + d.s.mean(0) + np.abs(xh) * (np.abs(xh) * d.s).mean(0))
    from_x = sw * (s_xh * np.abs((xh * d.v).mean(0)) + np.abs(xh) * (s_xh * np.abs(d.v)).mean(0)) + e * np.abs(b["d_in"])
    # the device keeps mean / invstd in fp32 (u and 5 u relative, fp64_yardstick): the same first-order terms with
    # s_xh = |xh| 6 u + u |mean| invstd and e = 5 u
    s_f = np.abs(xh) * 6 * U + U * np.abs(r["mean"]) * r["invstd"]
    from_f = sw * (s_f * np.abs((xh * d.v).mean(0)) + np.abs(xh) * (s_f * np.abs(d.v)).mean(0)) + 5 * U * np.abs(b["d_in"])
    n, su = x.v.shape[0], r.get("stats_u", 0.0)
    if su:                                                   # second order in the (large) fp32-statistics changes
        from_x = from_x * (1 + e) + sw * s_xh * (s_xh * np.abs(d.v)).mean(0)
    ds = (n + 1) * su * np.abs(d.v).sum(0)                  # fp32 sums of the torch composition's backward (stats_u)
    ddot = (n + 2) * su * np.abs(xh * d.v).sum(0)
    from_s = sw * (ds / n + np.abs(xh) * ddot / n)
    d_in = V(b["d_in"], b["slack"] + from_d + from_x + from_f + from_s)
    dw = V(b["dw"], b["tol_dw"] + (np.abs(xh) * d.s).sum(0) + ((s_xh + s_f) * (np.abs(d.v) + d.s)).sum(0) + ddot)
    db = V(b["db"], b["tol_db"] + d.s.sum(0) + ds)
    return d_in, dw, db


def head(pooled, p, eps=1e-5, class_specific=None, g_x4=None, g_logits=None, g_deltas=None, dw_splits=None, bn_eval=None, stats_u=0.0):
    """the whole definition.  pooled [n, C, ph, pw, pz] (the device's own, exact input); p: dict of fp32 parameters in the
    reference's layouts (conv_w [R, C, 1, 1, pz], conv_b, bn_w, bn_b, fc6_w, fc6_b, fc7_w, fc7_b and optionally cls_w,
    cls_b, reg_w, reg_b).  Gradients flow from g_x4 (no predictor) or from g_logits / g_deltas.  dw_splits: dict layer ->
    the device's split count (default 1).  bn_eval = (running_mean, running_var): evaluation mode with tracked
    statistics (forward only).  stats_u = U: the bounds of the torch composition, whose BatchNorm keeps fp32
    statistics (see the header).  Returns a dict of V: x4, logits, deltas, d_<parameter>, d_pooled."""
    sp = dw_splits or {}
    n, c, ph, pw, pz = pooled.shape
    hw = ph * pw
    R = p["conv_w"].shape[0]
    A = V(pooled_rows(pooled))
    wc = np.asarray(p["conv_w"], np.float64).reshape(R, c * pz)
    x1, _ = linear_fwd(A, wc, p["conv_b"])
    if bn_eval is None:
        x1n, r = bn_fwd(x1, p["bn_w"], p["bn_b"], eps, stats_u=stats_u)
    else:
        x1n, r = bn_fwd(x1, p["bn_w"], p["bn_b"], eps, train=False, running_mean=bn_eval[0], running_var=bn_eval[1])
    out_x1 = x1
    to_ref = lambda q: q.reshape(n, hw, R).transpose(0, 2, 1).reshape(n, R * hw)      # rows [n hw, R] -> view(N, -1)
    from_ref = lambda q: q.reshape(n, R, hw).transpose(0, 2, 1).reshape(n * hw, R)
    x2 = V(to_ref(x1n.v), to_ref(x1n.s))
    x3, pre3 = linear_fwd(x2, p["fc6_w"], p["fc6_b"], relu=True)
    x4, pre4 = linear_fwd(x3, p["fc7_w"], p["fc7_b"], relu=True)
    out = {"x4": x4, "x1": out_x1}
    g4 = None
    if "cls_w" in p:
        out["logits"], _ = linear_fwd(x4, p["cls_w"], p["cls_b"])
        out["deltas"], _ = linear_fwd(x4, p["reg_w"], p["reg_b"])
        if g_logits is not None:
            da1, out["d_cls_w"], out["d_cls_b"] = linear_bwd(V(g_logits), None, x4, p["cls_w"], sp.get("pred", 1))
            da2, out["d_reg_w"], out["d_reg_b"] = linear_bwd(V(g_deltas), None, x4, p["reg_w"], sp.get("pred", 1))
            # one GEMM over both weights: a reduction of length N_cls + N_reg; the sum of the two bounds covers it with
            # one more rounding
            g4 = V(da1.v + da2.v, da1.s + da2.s + U * (np.abs(da1.v) + np.abs(da2.v)))
    elif g_x4 is not None:
        g4 = V(g_x4)
    if g4 is None:
        return out
    g3, out["d_fc7_w"], out["d_fc7_b"] = linear_bwd(g4, pre4, x3, p["fc7_w"], sp.get("fc7", 1))
    g2, out["d_fc6_w"], out["d_fc6_b"] = linear_bwd(g3, pre3, x2, p["fc6_w"], sp.get("fc6", 1))
    g1n = V(from_ref(g2.v), from_ref(g2.s))
    g1, out["d_bn_w"], out["d_bn_b"] = bn_bwd(g1n, x1, r, p["bn_w"])
    dA, dwc, out["d_conv_b"] = linear_bwd(g1, None, A, wc, sp.get("conv", 1))
    out["d_conv_w"] = V(dwc.v.reshape(p["conv_w"].shape), dwc.s.reshape(p["conv_w"].shape))
    out["d_pooled"] = V(rows_pooled(dA.v, pooled.shape), rows_pooled(dA.s, pooled.shape))
    return out


def worst(got, ref):
    """max |got - ref.v| / ref.s (0 / 0 = 0), and the count of elements outside the bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.v.shape, (got.shape, ref.v.shape)
    err = np.abs(got - ref.v)
    bad = err > ref.s
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / ref.s)
    return (float(ratio.max()) if ratio.size else 0.0), int(bad.sum())


# ------------------------------------------------------------------------------------------------ shared test inputs
def make_cfg(**kw):
    """roi_glue.box_head_cfg: a cfg with the keys the box head reads"""
    import roi_glue
    return roi_glue.box_head_cfg(**kw)
