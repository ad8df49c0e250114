"""The box head's dense layers on the device (csrc/roi_mlp.hip, roi_glue.dense_linear / box_head_mlp / box_predictions,
the FPN2MLPFeatureExtractor / FPNPredictor / ROIBoxHead3D modules) against the fp64 definition of tests/roi_mlp_ref.py:
every element inside its derived bound; the one undecided mechanism (a ReLU input within its bound of zero, whose
gradient bound is then the whole gradient) is counted and capped at 1 % in the extractor test.  Shapes are the smallest that reach each path: one partial
tile, several tiles with remainders in M, N and K, both tile sizes and both sides of the split of the weight gradient
(placed with the library's own dispatch functions), both A layouts."""
import numpy as np
import pytest
import torch

import fp64_yardstick as Y
import roi_mlp_ref as M
import roi_pool_ref as P

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
KSTEP = 32            # include/aabr_hip.h: "The reduction runs in chunks of 32"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lib():
    import _hip
    return _hip.load()


def _ok(what, got, ref):
    w, bad = M.worst(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("%s: max |device - fp64| / bound = %.4g" % (what, w))
    assert bad == 0, (what, w)


def _tile_crossing():
    """M, N, K that each cross one tile edge (of every product's output) and one reduction chunk by a non-multiple"""
    lib = _lib()
    t = lib.aabr_roi_mlp_tile(70, 70)
    assert lib.aabr_roi_mlp_tile(t + 5, t + 4) == t
    return (t + 5, t + 3, t + 4)


def _entry_shapes():
    lib = _lib()
    shapes = [(1, 1, 4), (37, 10, 12), _tile_crossing()]
    lo = 1
    while lib.aabr_roi_mlp_tile(lo * 128 + 1, 1) != 128:                 # the tile threshold: rows on both sides of it
        lo += 1
    shapes += [(lo * 128, 1, 4), (lo * 128 + 1, 1, 4), (1, lo * 128 + 1, 4)]
    m = 1
    while lib.aabr_roi_mlp_dw_splits(m + 1, 1, 4) == 1:                   # the split threshold of the weight gradient
        m += 1
    shapes += [(m, 1, 4), (m + 1, 1, 4), (3 * m + 9, 10, 12)]
    shapes.append((13 * 128 + 7, 13 * 128 + 40, KSTEP + 4))               # 14 x 14 tiles of 128: the large tile in M and N
    assert lib.aabr_roi_mlp_tile(*shapes[-1][:2]) == 128
    return shapes


def _run_entry(M_, N, K, relu, bias, pooled=None, seed=0):
    """forward and the three gradients through the C ABI; `pooled` = (C, ph, pw, pz): A in the pooler's layout"""
    import _hip
    from _hip import check, ptr, stream
    lib = _lib()
    rng = np.random.default_rng(seed + 7 * M_ + 3 * N + K)
    W = rng.standard_normal((N, K)).astype(F)
    b = rng.standard_normal(N).astype(F) if bias else None
    if pooled is None:
        A = rng.standard_normal((M_, K)).astype(F)
        A_dev, rows, layout, hw, pz = _t(A), A.astype(np.float64), _hip.MLP_ROWS, 0, 0
    else:
        C, ph, pw, pz = pooled
        hw = ph * pw
        assert M_ % hw == 0 and K == C * pz
        A = rng.standard_normal((M_ // hw, C, ph, pw, pz)).astype(F)
        A_dev, rows, layout = _t(A), M.pooled_rows(A), _hip.MLP_POOLED
    W_d, b_d = _t(W), (_t(b) if bias else None)
    y = torch.empty((M_, N), dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_mlp_forward(ptr(A_dev), layout, hw, pz, ptr(W_d), ptr(b_d), int(relu), M_, N, K, ptr(y), stream()))
    tag = "(%d, %d, %d)%s%s%s" % (M_, N, K, " relu" if relu else "", " bias" if bias else "", " pooled" if pooled else "")
    ref, _ = M.linear_fwd(M.V(rows), W, b, relu)
    y_np = y.cpu().numpy()
    _ok("forward " + tag, y_np, ref)
    if relu:
        assert (y_np >= 0).all()
    g = rng.standard_normal((M_, N)).astype(F)
    gm = np.where(y_np > 0, g, 0) if relu else g                          # the mask is an input: the device's own Y
    g_d = _t(g)
    d_a = torch.full(A_dev.shape, float("nan"), dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_mlp_backward_input(ptr(g_d), ptr(y) if relu else None, ptr(W_d), M_, N, K, layout, hw, pz,
                                          ptr(d_a), stream()))
    splits = lib.aabr_roi_mlp_dw_splits(M_, N, K)
    r_a, r_w, r_b = M.linear_bwd(M.V(gm), None, M.V(rows), W, splits)
    if pooled is not None:
        r_a = M.V(M.rows_pooled(r_a.v, A.shape), M.rows_pooled(r_a.s, A.shape))
    _ok("input gradient " + tag, d_a, r_a)
    floats = lib.aabr_roi_mlp_dw_scratch_floats(M_, N, K)
    assert (floats > 0) == (splits > 1)
    scr = torch.empty(max(floats, 1), dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2 if splits > 1 else 1):
        d_w = torch.full((N, K), float("nan"), dtype=torch.float32, device=DEV)
        d_b = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV) if bias else None
        check(lib.aabr_roi_mlp_backward_weight(ptr(g_d), ptr(y) if relu else None, ptr(A_dev), layout, hw, pz, M_, N, K,
                                               0, ptr(d_w), ptr(d_b), ptr(scr) if floats else None, stream()))
        outs.append((d_w.cpu().numpy(), d_b.cpu().numpy() if bias else None))
    _ok("weight gradient (splits %d) " % splits + tag, outs[0][0], r_w)
    if bias:
        _ok("bias gradient " + tag, outs[0][1], r_b)
    if splits > 1:                                                         # determinism: equal bits run to run
        assert outs[0][0].tobytes() == outs[1][0].tobytes()
        assert not bias or outs[0][1].tobytes() == outs[1][1].tobytes()
    return splits


@pytest.mark.parametrize("relu,bias", [(False, False), (True, True)])
def test_entry_points_rows_layout(relu, bias):
    seen = set()
    for (m, n, k) in _entry_shapes():
        seen.add(_run_entry(m, n, k, relu, bias) > 1)
    assert seen == {False, True}                                           # both sides of the split were run


def test_entry_points_relu_without_bias_and_bias_without_relu():
    for (m, n, k) in [(37, 10, 12), _tile_crossing()]:
        _run_entry(m, n, k, True, False)
        _run_entry(m, n, k, False, True)


@pytest.mark.parametrize("C,res", [(8, (2, 3, 2)), (5, (2, 3, 4))])
@pytest.mark.parametrize("relu,bias", [(False, True), (True, False)])
def test_entry_points_pooled_layout(C, res, relu, bias):
    hw = res[0] * res[1]
    for n in (1, 5, 37):
        _run_entry(n * hw, 10, C * res[2], relu, bias, pooled=(C,) + res)
    _run_entry(60 * hw, _tile_crossing()[1], C * res[2], relu, bias, pooled=(C,) + res)   # the split, several column tiles


@pytest.mark.parametrize("relu,bias", [(False, True), (True, False)])
def test_entry_points_pooled_layout_on_both_sides_of_the_tile_threshold(relu, bias):
    """the 128 x 128 tile with the pooled layout: forward and input gradient (rows = ROIs x hw past the threshold),
    weight gradient (columns = C x pz past it), and the last shape before each"""
    lib = _lib()
    C, res = 8, (2, 3, 2)
    hw, pz = res[0] * res[1], res[2]
    n = 1
    while lib.aabr_roi_mlp_tile(n * hw, 1) != 128:                        # the first ROI count whose rows take the large tile
        n += 1
    assert lib.aabr_roi_mlp_tile(n * hw, C * pz) == 128 and lib.aabr_roi_mlp_tile((n - 1) * hw, C * pz) == 64
    for rois in (n - 1, n):
        _run_entry(rois * hw, 1, C * pz, relu, bias, pooled=(C,) + res)
    _run_entry((n // 2 + 1) * hw, 130, C * pz, relu, bias, pooled=(C,) + res)  # large tile, two column tiles, the second partial
    assert lib.aabr_roi_mlp_tile((n // 2 + 1) * hw, 130) == 128
    k = 4
    while lib.aabr_roi_mlp_tile(1, k) != 128:                             # the first K whose [N, K] gradient takes the large tile
        k += 4
    for kk in (k - 4, k):
        assert kk % pz == 0
        _run_entry(2 * hw, 1, kk, relu, bias, pooled=(kk // pz,) + res)
    _run_entry(50 * hw, 130, k // 2 + 6, relu, bias, pooled=((k // 2 + 6) // pz,) + res)   # large tile in N and K, split rows
    assert lib.aabr_roi_mlp_tile(130, k // 2 + 6) == 128 and lib.aabr_roi_mlp_dw_splits(50 * hw, 130, k // 2 + 6) > 1


@pytest.mark.parametrize("n", [9, 300], ids=["one_run", "split_rows"])
def test_fc6_pack_and_permuted_weight_gradient(n):
    import _hip
    from _hip import check, ptr, stream
    lib = _lib()
    hw, R, N = 6, 12, 10
    splits = lib.aabr_roi_mlp_dw_splits(n, N, hw * R)
    assert (splits > 1) == (n == 300)                                      # the permutation in the second stage too
    scr = torch.empty(max(1, lib.aabr_roi_mlp_dw_scratch_floats(n, N, hw * R)), dtype=torch.float32, device=DEV)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((N, R * hw)).astype(F)
    Wp = torch.empty((N, hw * R), dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_mlp_pack_fc6(ptr(_t(W)), N, R, hw, ptr(Wp), stream()))
    assert (Wp.cpu().numpy() == W.reshape(N, R, hw).transpose(0, 2, 1).reshape(N, hw * R)).all()
    A = rng.standard_normal((n, hw * R)).astype(F)                         # columns s R + r
    g = rng.standard_normal((n, N)).astype(F)
    d_w = torch.full((N, R * hw), float("nan"), dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_mlp_backward_weight(ptr(_t(g)), None, ptr(_t(A)), _hip.MLP_ROWS, 0, 0, n, N, hw * R, hw, ptr(d_w),
                                           None, ptr(scr) if splits > 1 else None, stream()))
    A_ref = A.reshape(n, hw, R).transpose(0, 2, 1).reshape(n, R * hw)      # the reference's column order r hw + s
    _ok("fc6 weight gradient in the reference's layout", d_w, M.linear_bwd(M.V(g), None, M.V(A_ref), W, splits)[1])


def test_empty_batch_returns_empty_tensors():
    import roi_glue
    x = torch.zeros((0, 12), device=DEV, requires_grad=True)
    w = torch.randn((5, 12), device=DEV, requires_grad=True)
    b = torch.randn(5, device=DEV, requires_grad=True)
    y = roi_glue.dense_linear(x, w, b, True)
    assert tuple(y.shape) == (0, 5)
    y.sum().backward()
    assert tuple(x.grad.shape) == (0, 12) and (w.grad == 0).all() and (b.grad == 0).all()
    a, d = roi_glue.box_predictions(x.detach(), w.detach(), b.detach(), w.detach(), b.detach())
    assert tuple(a.shape) == (0, 5) and tuple(d.shape) == (0, 5)


def test_dense_linear_autograd_matches_the_definition():
    import roi_glue
    rng = np.random.default_rng(11)
    m, n, k = 300, 7, 20
    assert _lib().aabr_roi_mlp_dw_splits(m, n, k) > 1
    A, W, b, g = (rng.standard_normal(s).astype(F) for s in ((m, k), (n, k), (n,), (m, n)))
    x, w, bb = (_t(v).requires_grad_(True) for v in (A, W, b))
    y = roi_glue.dense_linear(x.t().contiguous().t(), w, bb, True)         # a non-contiguous input is made contiguous
    y.backward(_t(g))
    fwd, pre = M.linear_fwd(M.V(A), W, b, True)
    _ok("dense_linear", y, fwd)
    gm = np.where(y.detach().cpu().numpy() > 0, g, 0)
    r_a, r_w, r_b = M.linear_bwd(M.V(gm), None, M.V(A), W, _lib().aabr_roi_mlp_dw_splits(m, n, k))
    _ok("dense_linear d_x", x.grad, r_a)
    _ok("dense_linear d_w", w.grad, r_w)
    _ok("dense_linear d_b", bb.grad, r_b)
    with pytest.raises(TypeError):
        roi_glue.dense_linear(x.detach().to(torch.bfloat16), w, bb, True)


# ------------------------------------------------------------------------------------------------ the modules
class _Boxes(object):
    mode = "yx_zb"

    def __init__(self, bbox3d, labels=None):
        self.bbox3d, self.size3d, self._labels = bbox3d, torch.tensor([[0.0, 0.0, 0.0, 48.0, 40.0, 12.0]]), labels

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def get_field(self, name):
        assert name == "labels"
        return self._labels


_CASES = {}


def _case(counts):
    """a tests/roi_pool_ref.py case at C = 8, output (2, 3, 2): the levels as test_gpu_roi_pool.py builds its own"""
    import sparseconvnet as scn
    if counts not in _CASES:
        case = P.PoolCase("mlp_%d_%d" % counts, 400 + sum(counts), 8, (2, 3, 2), 2, counts)
        lv = []
        for (h, w, z), sites, feats in zip(P.EXTENTS, case.sites, case.feats):
            lv.append(scn.InputLayer(3, [h + 3, w + 2, z + 1], mode=4)([_t(sites.astype(np.int64)), _t(feats)]))
        _CASES[counts] = (case, lv)
    return _CASES[counts]


def _inputs(counts):
    import sparseconvnet as scn
    case, lv = _case(counts)
    fs = [x.features.detach().clone().requires_grad_(True) for x in lv]
    xs = [scn.SparseConvNetTensor(f, x.metadata, x.spatial_size) for f, x in zip(fs, lv)]
    return case, fs, xs, [_Boxes(_t(b)) for b in case.boxes]


def _params(ext, pred=None):
    p = {"conv_w": ext.conv3d[0].weight, "conv_b": ext.conv3d[0].bias, "bn_w": ext.conv3d[1].weight,
         "bn_b": ext.conv3d[1].bias, "fc6_w": ext.fc6.weight, "fc6_b": ext.fc6.bias, "fc7_w": ext.fc7.weight,
         "fc7_b": ext.fc7.bias}
    if pred is not None:
        p.update(cls_w=pred.cls_score.weight, cls_b=pred.cls_score.bias, reg_w=pred.bbox_pred.weight,
                 reg_b=pred.bbox_pred.bias)
    return p


def _build(class_specific=True, track=False, seed=3):
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_predictors import make_roi_box_predictor
    torch.manual_seed(seed)
    cfg = M.make_cfg(C=8, resolution=(2, 3, 2), R=12, class_specific=class_specific, track=track, scales=P.SCALES,
                     canonical=P.CANONICAL)
    ext, pred = make_roi_box_feature_extractor(cfg).to(DEV), make_roi_box_predictor(cfg).to(DEV)
    with torch.no_grad():                                   # biases and weights away from their constant initial values
        for prm in list(ext.parameters()) + list(pred.parameters()):
            if prm.dim() == 1:
                prm.uniform_(-0.5, 0.5)
        ext.conv3d[1].weight.uniform_(0.5, 1.5)
        pred.cls_score.weight.normal_(std=0.3)
        pred.bbox_pred.weight.normal_(std=0.3)
    return ext, pred


@pytest.mark.parametrize("counts", [(1, 0), (23, 14)], ids=["1roi", "37rois"])
@pytest.mark.parametrize("class_specific", [True, False])
def test_extractor_and_predictor_against_the_definition(counts, class_specific):
    ext, pred = _build(class_specific)
    case, fs, xs, boxes = _inputs(counts)
    n = sum(counts)
    rng = np.random.default_rng(17)
    res = {}
    for fused in (True, False):
        ext.fused = pred.fused = fused
        ext.zero_grad()
        pred.zero_grad()
        for f in fs:
            f.grad = None
        pooled = ext.pooler(xs, boxes)
        pooled.retain_grad()
        x4 = ext.head(pooled)
        logits, deltas = pred(x4)
        if fused:
            assert tuple(x4.shape) == (n, 12) and tuple(logits.shape) == (n, 3)
            assert tuple(deltas.shape) == (n, 21 if class_specific else 7)
            g_l = rng.standard_normal(tuple(logits.shape)).astype(F)
            g_d = rng.standard_normal(tuple(deltas.shape)).astype(F)
        ((logits * _t(g_l)).sum() + (deltas * _t(g_d)).sum()).backward()
        res[fused] = dict(pooled=pooled.detach(), x4=x4.detach(), logits=logits.detach(), deltas=deltas.detach(),
                          d_pooled=pooled.grad.clone(), d_feats=[f.grad.clone() for f in fs],
                          grads={k: v.grad.clone() for k, v in _params(ext, pred).items()})
    got = res[True]
    assert torch.equal(got["pooled"], res[False]["pooled"])
    p = {k: v.detach().cpu().numpy() for k, v in _params(ext, pred).items()}
    M.UNDECIDED.clear()
    ref = M.head(got["pooled"].cpu().numpy(), p, eps=ext.conv3d[1].eps, g_logits=g_l, g_deltas=g_d)
    share = M.undecided_share()
    print("ReLU inputs within their bound of zero: %.5f of %d" % (share, sum(t for _, t in M.UNDECIDED)))
    assert share <= 0.01                                                   # there the gradient's bound decides nothing
    for k in ("x4", "logits", "deltas"):
        _ok(k, got[k], ref[k])
    for k in p:
        _ok("d_" + k, got["grads"][k], ref["d_" + k])
    _ok("d_pooled", got["d_pooled"], ref["d_pooled"])
    # the torch composition obeys the GEMM bounds (any summation order) and, with fp32 batch statistics, the wider
    # BatchNorm bounds of roi_mlp_ref's `stats_u`: the two sides differ by at most the sum of their own bounds ...
    M.UNDECIDED.clear()
    ref_t = M.head(got["pooled"].cpu().numpy(), p, eps=ext.conv3d[1].eps, g_logits=g_l, g_deltas=g_d, stats_u=M.U)
    print("torch composition: ReLU inputs within their (wider) bound of zero: %.5f" % M.undecided_share())
    for k in ("x4", "logits", "deltas", "d_pooled"):                       # figures: the torch side against its own bound
        print("torch composition %s: max |torch - fp64| / bound = %.4g" % (k, M.worst(res[False][k].cpu().numpy(), ref_t[k])[0]))
    bound = ref["d_pooled"].s + ref_t["d_pooled"].s
    print("d_pooled: max |fused - torch| / (sum of bounds) = %.4g"
          % float((np.abs((got["d_pooled"] - res[False]["d_pooled"]).cpu().numpy()) / bound).max()))
    assert (np.abs((got["d_pooled"] - res[False]["d_pooled"]).cpu().numpy()) <= bound).all()
    # ... and so do the level gradients, through the pooler's adjoint: its weights are non-negative, so the bound on
    # d_pooled is carried by the same backward pass; the fp32 atomic adds of both runs add T u sum |terms| with T the
    # terms a cell can receive (ROIs x bins x 2^3 samples x 8 corners)
    T = n * 12 * 8 * 8
    pooled = ext.pooler(xs, boxes)
    carried = torch.autograd.grad(pooled, fs, grad_outputs=_t(bound.astype(F)), retain_graph=True)
    mag = torch.autograd.grad(pooled, fs, grad_outputs=got["d_pooled"].abs() + res[False]["d_pooled"].abs())
    for l in range(len(fs)):
        diff = (got["d_feats"][l] - res[False]["d_feats"][l]).abs()
        lim = carried[l] * (1 + T * Y.U) + T * Y.U * mag[l]
        print("level %d: max |fused - torch| = %.3g" % (l, float(diff.max()) if diff.numel() else 0.0))
        assert bool((diff <= lim).all())
    if n > 1:
        assert any(float(d.abs().max()) > 0 for d in got["d_feats"])


def test_batchnorm_modes():
    case, fs, xs, boxes = _inputs((23, 14))
    ext, _ = _build(track=False)
    with torch.no_grad():
        pooled = ext.pooler(xs, boxes)
        ext.train()
        a = ext.head(pooled)
        ext.eval()
        b = ext.head(pooled)
    assert torch.equal(a, b) and "conv3d.1.running_mean" not in ext.state_dict()       # batch statistics in both modes
    ext, _ = _build(track=True)
    bn = ext.conv3d[1]
    ext.train()
    with torch.no_grad():
        a = ext.head(pooled)
    p = {k: v.detach().cpu().numpy() for k, v in _params(ext).items()}
    ref = M.head(pooled.cpu().numpy(), p, eps=bn.eps)
    _ok("x4, training", a, ref["x4"])
    x1 = ref["x1"]
    r = Y.bn_forward_exact(x1.v, p["bn_w"], p["bn_b"], eps=bn.eps, momentum=1.0 - bn.momentum, leak=0.0, train=True)
    rows = x1.v.shape[0]
    xm = np.abs(x1.v - r["mean"])
    mom = float(Y.f32(1.0 - bn.momentum))
    # the convolution's own bound s on x1 moves the mean by mean(s) and the unbiased variance by 2 mean(|x - mean| s) n / (n - 1)
    tol_rm = r["tol_rm"] + (1 - mom) * x1.s.mean(0)
    tol_rv = r["tol_rv"] + (1 - mom) * 2 * (xm * x1.s).mean(0) * rows / (rows - 1)
    rm, rv = bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy()
    assert (np.abs(rm - r["running_mean"]) <= tol_rm).all() and (np.abs(rv - r["running_var"]) <= tol_rv).all()
    assert int(bn.num_batches_tracked) == 1
    ext.eval()
    with torch.no_grad():
        b = ext.head(pooled)
    assert not torch.equal(a, b)
    _ok("x4, evaluation with the running statistics", b, M.head(pooled.cpu().numpy(), p, eps=bn.eps, bn_eval=(rm, rv))["x4"])
    assert torch.equal(bn.running_mean, _t(rm)) and int(bn.num_batches_tracked) == 1    # evaluation leaves them alone


def test_box_head_training_and_evaluation_calls():
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import build_roi_box_head
    case, fs, xs, boxes = _inputs((23, 14))
    torch.manual_seed(5)
    cfg = M.make_cfg(C=8, resolution=(2, 3, 2), R=12, scales=P.SCALES, canonical=P.CANONICAL, detections=20)
    head = build_roi_box_head(cfg).to(DEV)
    targets = []
    for b in case.boxes:                                   # ground truth: a few of the proposals themselves
        g = np.ascontiguousarray(b[:4])
        targets.append(_Boxes(_t(g), _t(np.array([1, 2, 1, 2], np.int64))))
    head.train()
    x, sampled, losses = head(xs, boxes, targets)
    assert set(losses) == {"loss_classifier_roi", "loss_box_reg_roi"} and len(sampled) == 2
    assert x.shape[0] == sum(len(s) for s in sampled) and x.shape[1] == 12
    total = losses["loss_classifier_roi"] + losses["loss_box_reg_roi"]
    assert bool(torch.isfinite(total))
    total.backward()
    sd = dict(head.named_parameters())
    for k in ("feature_extractor.conv3d.0.weight", "feature_extractor.fc6.weight", "predictor.cls_score.weight"):
        assert sd[k].grad is not None and float(sd[k].grad.abs().max()) > 0, k
    head.eval()
    with torch.no_grad():
        x, dets, losses = head(xs, boxes)
    assert losses == {} and len(dets) == 2 and x.shape[0] == 37
    for d in dets:
        assert len(d) <= cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG
