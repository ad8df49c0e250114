"""The corner form of the box head on the device (MODEL.CORNER_ROI): the coder's list kernels, targets and detections in
corner form, fc6 over windows of the convolution rows, and ROIBoxHead3D.

  * list kernels: bit-equal to csrc/corner_box.h compiled for the host (tests/corner_box_host_harness.cpp) on the
    fixture's inputs -- the same code on both sides; the host side is held to the reference in test_corner_box_host.py;
  * targets / detections: bit-equal to BoxCoder3D(True).encode / decode on the matched pairs / all rows; labels, samples
    and keep decisions are those of the centroid run / of tests/roi_post_ref.py fed the device's boxes;
  * dense layers: every value and gradient inside the bound of tests/corner_head_ref.py (each GEMM element
    (K + 1) 2^-24 sum |a w| plus what its inputs carry), the gradient at the window columns w = 2 and w = 8, where two
    windows meet, looked at on their own; two runs bit-identical.  C = 8, resolution (2, 11, 2), R = 12 at N = 1, 5 and
    70: at N = 70 the stacked corner GEMM has 140 rows and crosses the 64- and the 128-row tile;
  * the module against `fused = False` within the sum of the two sides' bounds."""
import os

import numpy as np
import pytest
import torch

import corner_head_ref as CH
import roi_mlp_ref as M
import roi_pool_ref as P
import roi_post_ref as RP
from corner_box_host import Host, build_harness

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
W = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 2.0)
PH, R_, C_ = 2, 12, 8


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F).view(np.uint32)


def _ok(what, got, ref):
    w, bad = M.worst(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("%s: max |device - fp64| / bound = %.4g" % (what, w))
    assert bad == 0, (what, w)


# ------------------------------------------------------------------------------------------------ the coder
def test_list_kernels_are_the_host_code_bit_for_bit(tmp_path):
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from utils3d.bbox3d_ops_torch import Box3D_Torch
    host = Host(build_harness(tmp_path))
    g = dict(np.load(os.path.join(HERE, "golden", "corner_golden.npz")))
    for k in ("boxes", "anchors", "targets"):
        assert (_bits(Box3D_Torch.from_yxzb_to_2corners(_t(g[k]))) == _bits(host.to_2corners(g[k]))).all(), k
    assert (_bits(Box3D_Torch.from_2corners_to_yxzb(_t(g["corners"]))) == _bits(host.from_2corners(g["corners"]))).all()
    c3 = np.ascontiguousarray(g["corners"][:60].reshape(20, 21))                 # the [n, 7 k] form
    assert (_bits(Box3D_Torch.from_2corners_to_yxzb(_t(c3))) == _bits(host.from_2corners(c3.reshape(-1, 7)).reshape(20, 21))).all()
    for name, w in (("w1", None), ("w2", W)):
        coder = BoxCoder3D(True, w)
        wv = g["weights_" + name]
        assert coder.weights.view(7).tolist() == wv.tolist()
        enc = coder.encode(_t(g["targets"]), _t(g["anchors"]))
        assert (_bits(enc) == _bits(host.encode(g["targets"], g["anchors"], wv))).all(), name
        dec = coder.decode(_t(g["dec_enc"]), _t(g["anchors"]))
        assert (_bits(dec) == _bits(host.decode(g["dec_enc"], g["anchors"], wv))).all(), name
    dec3 = BoxCoder3D(True, W).decode(_t(g["dec3_enc"]), _t(g["anchors"][:64]))
    assert tuple(dec3.shape) == (64, 21)
    assert (_bits(dec3) == _bits(host.decode(g["dec3_enc"], g["anchors"][:64], g["weights_w2"]))).all()
    # empty lists, and no tensor of the results lives on the host
    assert BoxCoder3D(True, None).encode(_t(np.zeros((0, 7), F)), _t(np.zeros((0, 7), F))).shape == (0, 7)
    assert Box3D_Torch.from_yxzb_to_2corners(_t(np.zeros((0, 7), F))).shape == (0, 7)
    assert enc.is_cuda and dec.is_cuda


def _scenes(n_b, g, seed):
    """per scene: wall proposals; ground truth = g of the proposals moved a little, so that matches occur"""
    rng = np.random.default_rng(seed)
    props, gts, tls = [], [], []
    for i, n in enumerate(n_b):
        p = RP.wall_proposals(n, seed * 100 + i)
        rows = rng.choice(n, g, replace=False)
        t = (p[rows] + rng.normal(0, 1, (g, 7)) * np.array([0.05, 0.05, 0.03, 0.01, 0.1, 0.05, 0.02])).astype(F)
        t[:, 3:6] = np.maximum(t[:, 3:6], F(0.05))
        props.append(np.ascontiguousarray(p, F))
        gts.append(np.ascontiguousarray(t, F))
        tls.append(rng.integers(1, 3, g).astype(np.int64))
    return props, gts, tls


def test_targets_in_corner_form():
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    props, gts, tls = _scenes([5, 70], 3, 4)
    runs = {}
    for corner in (True, False):
        dbg = {}
        out = roi_glue.box_head_targets([_t(p) for p in props], [_t(t) for t in gts], [_t(l) for l in tls], 0.5, 0.5, None,
                                        16, 0.25, seed=77, debug=dbg, box_coder=BoxCoder3D(corner, W))
        runs[corner] = (out, dbg)
    (out_c, dc), (out_0, d0) = runs[True], runs[False]
    # matching, labels and the sampled sets do not depend on the coder
    for k in ("matched_idx", "labels", "samp_rows", "samp_labels", "samp_boxes"):
        assert torch.equal(dc[k], d0[k]), k
    assert (_bits(dc["matched_val"]) == _bits(d0["matched_val"])).all() and dc["info"] == d0["info"]
    assert (dc["labels"] > 0).any() and (dc["labels"] == 0).any()
    midx, regt = dc["matched_idx"].cpu().numpy(), dc["regression_targets"]
    o = 0
    for b, (p, t) in enumerate(zip(props, gts)):
        sl = slice(o, o + len(p))
        enc = BoxCoder3D(True, W).encode(_t(t[np.maximum(midx[sl], 0)]), _t(p))
        assert (_bits(regt[sl]) == _bits(enc)).all(), "scene %d" % b
        cen = BoxCoder3D(False, W).encode(_t(t[np.maximum(midx[sl], 0)]), _t(p))
        assert (_bits(d0["regression_targets"][sl]) == _bits(cen)).all() and not torch.equal(enc, cen)
        rows = out_c[b]["rows"]
        assert torch.equal(rows, out_0[b]["rows"]) and torch.equal(out_c[b]["labels"], out_0[b]["labels"])
        assert (_bits(out_c[b]["regression_targets"]) == _bits(regt[sl][rows])).all()
        o += len(p)


@pytest.mark.parametrize("class_specific", [True, False])
def test_detections_in_corner_form(class_specific):
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    rng = np.random.default_rng(3)
    n_b, c = [40, 40], 3
    props = [RP.wall_proposals(n, 300 + i) for i, n in enumerate(n_b)]
    allp = np.concatenate(props)
    logits = rng.normal(0, 2.0, (80, c)).astype(F)
    k = c if class_specific else 1
    reg = (rng.normal(0, 0.05, (80, 7 * k)) * np.tile(np.array(W), k)).astype(F)
    coder, dbg = BoxCoder3D(True, W), {}
    dets = roi_glue.box_detections(_t(logits), _t(reg), [_t(p) for p in props], class_specific=class_specific, debug=dbg,
                                   box_coder=coder, detections_per_img=20)
    prob, boxes = dbg["prob"].cpu().numpy(), dbg["boxes"].cpu().numpy()
    dec = coder.decode(_t(reg), _t(allp)).cpu().numpy().reshape(80, -1, 7)
    assert (_bits(boxes) == _bits(dec if class_specific else np.repeat(dec, c, 1))).all()
    cen = BoxCoder3D(False, W).decode(_t(reg), _t(allp)).cpu().numpy().reshape(80, -1, 7)
    assert not np.array_equal(dec, cen)
    # the keep decisions are the post-processor's own on these boxes
    stats = []
    ref = RP.stage_b(prob, boxes, n_b, 0.05, 0.5, None, 20, stats=stats)
    assert sum(len(r[0]) for r in ref) > 0
    r0 = 0
    for b, (d, (rows, labels)) in enumerate(zip(dets, ref)):
        assert d["rows"].cpu().numpy().tolist() == rows.tolist() and d["labels"].cpu().numpy().tolist() == labels.tolist()
        bx = boxes[r0:r0 + n_b[b]]
        assert (_bits(d["bbox3d"]) == _bits(bx[rows, labels])).all()
        assert dbg["info"][b][0] == len(rows)
        r0 += n_b[b]


# ------------------------------------------------------------------------------------------------ the dense layers
def _splits(n):
    """the device's split count of each weight gradient at n ROIs (the bound counts one more rounding per split)"""
    import _hip
    s = _hip.load().aabr_roi_mlp_dw_splits
    return {"conv": s(n * PH * 11, R_, C_ * 2), "fc6_cor": s(2 * n, R_, R_ * PH * 3), "fc6_body": s(n, R_, R_ * PH * 7),
            "fc7_cor": s(2 * n, R_, R_), "fc7_body": s(n, R_, R_), "pred_cor": s(2 * n, 14, R_), "pred_body": s(n, 12, R_)}


def _poison(like):
    """leave NaN in the block the next allocation of this size is likely to reuse: an element that a kernel does not
    write then shows"""
    t = torch.full_like(like, float("nan"))
    del t


@pytest.mark.parametrize("n", [1, 5, 70])
def test_fc6_over_windows(n):
    import roi_glue
    rng = np.random.default_rng(20 + n)
    x = rng.standard_normal((n * PH * 11, R_)).astype(F)
    p = {"fc6_cor_w": rng.normal(0, 0.2, (R_, R_ * PH * 3)).astype(F), "fc6_cor_b": rng.uniform(-0.5, 0.5, R_).astype(F),
         "fc6_body_w": rng.normal(0, 0.2, (R_, R_ * PH * 7)).astype(F), "fc6_body_b": rng.uniform(-0.5, 0.5, R_).astype(F)}
    g_c, g_b = rng.standard_normal((2 * n, R_)).astype(F), rng.standard_normal((n, R_)).astype(F)
    runs = []
    for _ in range(2):
        xt = _t(x).requires_grad_(True)
        pt = {k: _t(v).requires_grad_(True) for k, v in p.items()}
        y_cor, y_body = roi_glue._CornerFc6.apply(xt, pt["fc6_cor_w"], pt["fc6_cor_b"], pt["fc6_body_w"], pt["fc6_body_b"],
                                                  (n, PH, 11, R_))
        _poison(xt)
        ((y_cor * _t(g_c)).sum() + (y_body * _t(g_b)).sum()).backward()
        runs.append(dict(y_cor=y_cor.detach(), y_body=y_body.detach(), d_x=xt.grad, **{"d_" + k: v.grad for k, v in pt.items()}))
    got = runs[0]
    assert all(torch.equal(got[k], runs[1][k]) for k in got), "two runs differ"
    M.UNDECIDED.clear()
    ref = CH.fc6_windows(M.V(x), p, n, PH, R_, M.V(g_c), M.V(g_b), _splits(n))
    assert M.undecided_share() <= 0.01
    for k in ("y_cor", "y_body", "d_fc6_cor_w", "d_fc6_cor_b", "d_fc6_body_w", "d_fc6_body_b"):
        _ok(k, got[k], ref[k])
    # the input gradient: where one window writes, and where two meet
    d_x, want = got["d_x"].cpu().numpy().reshape(n, PH, 11, R_), ref["d_x"]
    assert np.isfinite(d_x).all()
    wv, ws = want.v.reshape(n, PH, 11, R_), want.s.reshape(n, PH, 11, R_)
    for name, cols in (("w = 2", [2]), ("w = 8", [8]), ("one window", [0, 1, 3, 4, 5, 6, 7, 9, 10])):
        _ok("d_x at " + name, d_x[:, :, cols], M.V(wv[:, :, cols], ws[:, :, cols]))
        assert float(np.abs(wv[:, :, cols]).max()) > 0
    # ... a lost contribution would show: at the overlap each term alone is outside the bound somewhere
    sc = lambda q, w: CH.window_scatter(q, n, PH, R_, w)
    body_only = sc(M.linear_bwd(M.V(g_b), ref["pre_body"], ref["x2_body"], p["fc6_body_w"])[0].v, CH.BODY)
    assert (np.abs(body_only[:, :, [2, 8]] - wv[:, :, [2, 8]]) > ws[:, :, [2, 8]]).any()


def _build(class_specific=True, seed=3):
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    torch.manual_seed(seed)
    cfg = M.make_cfg(C=C_, resolution=(PH, 11, 2), R=R_, corner=True, class_specific=class_specific, scales=P.SCALES,
                     canonical=P.CANONICAL)
    ext, pred = make_roi_box_feature_extractor(cfg).to(DEV), make_roi_box_predictor(cfg).to(DEV)
    with torch.no_grad():                                   # biases and weights away from their constant initial values
        for prm in list(ext.parameters()) + list(pred.parameters()):
            if prm.dim() == 1:
                prm.uniform_(-0.5, 0.5)
        ext.conv3d[1].weight.uniform_(0.5, 1.5)
    return ext, pred


def _head_run(ext, pred, pooled_np, g):
    ext.zero_grad()
    pred.zero_grad()
    pooled = _t(pooled_np).requires_grad_(True)
    x = ext.head(pooled)
    scores, reg, sem = pred(x)
    ((scores * _t(g[0])).sum() + (reg * _t(g[1])).sum() + (sem * _t(g[2])).sum()).backward()
    out = dict(x_cor=torch.cat([x[0], x[1]]).detach(), x_body=x[2].detach(), scores=scores.detach(),
               regression=reg.detach(), semantics=sem.detach(), d_pooled=pooled.grad.clone())
    out.update({"d_" + k: v.grad.clone() for k, v in CH.params_of(ext, pred).items()})
    return out, x


@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("class_specific", [True, False])
def test_dense_layers_against_the_definition(n, class_specific):
    ext, pred = _build(class_specific)
    rng = np.random.default_rng(40 + n)
    pooled = rng.standard_normal((n, C_, PH, 11, 2)).astype(F)
    k = 3 if class_specific else 1
    g = [rng.standard_normal(s).astype(F) for s in ((n, 3), (n, 7 * k), (n, 16))]
    got, x = _head_run(ext, pred, pooled, g)
    assert isinstance(x, list) and len(x) == 3 and all(tuple(v.shape) == (n, R_) for v in x)
    assert x[0].data_ptr() == x.x_cor.data_ptr() and x[1].data_ptr() == x.x_cor[n:].data_ptr()   # views of the stacked rows
    assert tuple(got["regression"].shape) == (n, 7 * k) and tuple(got["semantics"].shape) == (n, 16)
    again, _ = _head_run(ext, pred, pooled, g)
    assert all(torch.equal(got[key], again[key]) for key in got), "two runs differ"
    assert pred.score_pred_cor.weight.grad is None
    p = {key: v.detach().cpu().numpy() for key, v in CH.params_of(ext, pred).items()}
    M.UNDECIDED.clear()
    ref = CH.head(pooled, p, eps=ext.conv3d[1].eps, class_specific=class_specific, g_scores=g[0], g_reg=g[1], g_sem=g[2],
                  dw_splits=_splits(n))
    share = M.undecided_share()
    print("ReLU inputs within their bound of zero: %.5f of %d" % (share, sum(t for _, t in M.UNDECIDED)))
    assert share <= 0.01
    for key in got:
        _ok(key, got[key], ref[key])
    # `fused = False`, the reference's statements in torch, against the same definition with fp32 batch statistics;
    # the two sides then differ by at most the sum of their bounds
    ext.fused = pred.fused = False
    other, xl = _head_run(ext, pred, pooled, g)
    assert type(xl) is list
    ref_t = CH.head(pooled, p, eps=ext.conv3d[1].eps, class_specific=class_specific, g_scores=g[0], g_reg=g[1], g_sem=g[2],
                    dw_splits=_splits(n), stats_u=M.U)
    for key in ("x_cor", "x_body", "scores", "regression", "semantics", "d_pooled"):
        diff = np.abs((got[key] - other[key]).cpu().numpy())
        bound = ref[key].s + ref_t[key].s
        print("%s: max |fused - torch| / (sum of bounds) = %.4g" % (key, float((diff / bound).max())))
        assert (diff <= bound).all(), key


# ------------------------------------------------------------------------------------------------ the module
class _Boxes(object):
    mode = "yx_zb"

    def __init__(self, bbox3d, labels=None):
        self.bbox3d, self.size3d, self._labels = bbox3d, torch.tensor([[0.0, 0.0, 0.0, 48.0, 40.0, 12.0]]), labels

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def get_field(self, name):
        assert name == "labels"
        return self._labels


def _pyramid(counts):
    """a tests/roi_pool_ref.py case: a tiny feature pyramid (its first two levels hold the boxes) and the scenes' boxes"""
    import sparseconvnet as scn
    case = P.PoolCase("corner_%d_%d" % counts, 700 + sum(counts), C_, (PH, 11, 2), 2, counts)
    lv = [scn.InputLayer(3, [h + 3, w + 2, z + 1], mode=4)([_t(s.astype(np.int64)), _t(f)])
          for (h, w, z), s, f in zip(P.EXTENTS, case.sites, case.feats)]
    return case, lv


def test_box_head_in_corner_form_against_fused_false():
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import build_roi_box_head
    case, xs = _pyramid((23, 14))
    boxes = [_Boxes(_t(b)) for b in case.boxes]
    targets = [_Boxes(_t(np.ascontiguousarray(b[:4])), _t(np.array([1, 2, 1, 2], np.int64))) for b in case.boxes]
    torch.manual_seed(5)
    cfg = M.make_cfg(C=C_, resolution=(PH, 11, 2), R=R_, corner=True, scales=P.SCALES, canonical=P.CANONICAL, detections=20)
    head = build_roi_box_head(cfg).to(DEV)
    with torch.no_grad():
        for prm in head.parameters():
            if prm.dim() == 1:
                prm.uniform_(-0.5, 0.5)
        head.feature_extractor.conv3d[1].weight.uniform_(0.5, 1.5)
    head.loss_evaluator.fg_bg_sampler.seed = 9
    ext, pred = head.feature_extractor, head.predictor
    seen = {}
    ext.pooler.register_forward_hook(lambda m, i, o: seen.__setitem__("pooled", o.detach()))
    pred.register_forward_hook(lambda m, i, o: seen.__setitem__("pred", [t.detach() for t in o]))
    p = {k: v.detach().cpu().numpy() for k, v in CH.params_of(ext, pred).items()}
    for training in (True, False):
        head.train(training)
        res = {}
        for fused in (True, False):
            ext.fused = pred.fused = fused
            with torch.set_grad_enabled(training):
                x, props, losses = head(xs, boxes, targets if training else None)
            res[fused] = dict(x=[t.detach() for t in x], props=props, losses=losses, pooled=seen["pooled"], pred=seen["pred"])
        a, b = res[True], res[False]
        assert torch.equal(a["pooled"], b["pooled"])                          # the same (sampled) proposals on both sides
        n = int(a["pooled"].shape[0])
        assert len(a["x"]) == 3 and all(tuple(t.shape) == (n, R_) for t in a["x"])
        sp = _splits(n)
        ref = CH.head(a["pooled"].cpu().numpy(), p, eps=ext.conv3d[1].eps, dw_splits=sp)
        ref_t = CH.head(a["pooled"].cpu().numpy(), p, eps=ext.conv3d[1].eps, dw_splits=sp, stats_u=M.U)
        named = {"x_cor": lambda r: torch.cat(r["x"][:2]), "x_body": lambda r: r["x"][2], "scores": lambda r: r["pred"][0],
                 "regression": lambda r: r["pred"][1], "semantics": lambda r: r["pred"][2]}
        for key, get in named.items():
            _ok("%s (training=%s)" % (key, training), get(a), ref[key])
            diff = np.abs((get(a) - get(b)).cpu().numpy())
            assert (diff <= ref[key].s + ref_t[key].s).all(), key
        if training:
            assert set(a["losses"]) == {"loss_classifier_roi", "loss_box_reg_roi"} == set(b["losses"])
            assert n == sum(len(q) for q in a["props"]) and 0 < n <= 32
            labels = torch.cat([q.get_field("labels") for q in a["props"]]).cpu().numpy()
            assert (labels > 0).any()
            s_log = ref["scores"].s + ref_t["scores"].s
            s_reg = (ref["regression"].s + ref_t["regression"].s).reshape(n, 3, 7)
            # cross-entropy moves by at most 2 max_c |d logit| per row (mean over rows); smooth-L1 is 1-Lipschitz in
            # each of the positive rows' 7 selected columns (sum / n); the loss kernels' own fp32 sums add a relative
            # (n C + 8) u
            lim_cls = float((2 * s_log.max(1)).mean())
            lim_box = float(sum(s_reg[i, labels[i]].sum() for i in range(n) if labels[i] > 0) / n)
            for key, lim in (("loss_classifier_roi", lim_cls), ("loss_box_reg_roi", lim_box)):
                va, vb = float(a["losses"][key]), float(b["losses"][key])
                lim += (n * 21 + 8) * M.U * (abs(va) + abs(vb))
                print("%s: fused %.7g torch %.7g, |difference| / bound = %.3g" % (key, va, vb, abs(va - vb) / lim))
                assert np.isfinite(va) and abs(va - vb) <= lim
            ext.fused = pred.fused = True
            head.zero_grad()
            _, _, losses = head(xs, boxes, targets)
            (losses["loss_classifier_roi"] + losses["loss_box_reg_roi"]).backward()
            for key in ("feature_extractor.conv3d.0.weight", "feature_extractor.fc6_cor.weight",
                        "feature_extractor.fc6_body.weight", "predictor.bbox_pred_cor.weight"):
                grad = dict(head.named_parameters())[key].grad
                assert grad is not None and float(grad.abs().max()) > 0, key
            sem = dict(head.named_parameters())["predictor.bbox_corner_semantic.weight"].grad             # dropped: no corner loss
            assert sem is None or float(sem.abs().max()) == 0
        else:
            assert a["losses"] == {} and len(a["props"]) == 2 and n == 37
            for d in a["props"]:
                assert len(d) <= 20 and d.bbox3d.shape[1] == 7
    with pytest.raises(ValueError, match=r"LOSS\.WEIGHTS"):
        build_roi_box_head(M.make_cfg(corner=True, resolution=(PH, 11, 2), loss_weights=(1, 1, 1, 1, 0, 1, 0)))
