"""The box head's loss on the device (csrc/roi_loss.hip, roi_glue.box_head_targets / box_head_loss,
FastRCNNLossComputation) against the CPU restatement tests/roi_loss_ref.py.  Split the way test_gpu_roi_post.py is, so that
no tolerance touches a discrete decision:

Values.  The device's IoU matrices against the C oracle's boxes_iou_3d at atol 2e-5 (the figure test_gpu_labels.py uses and
justifies), and the regression targets bit-equal to BoxCoder3D.encode on the gathered rows.

Decisions.  The restatement is fed the DEVICE's IoU matrices; from there every step is exact on fp32 / integer data
(maximum, first index, two comparisons, a gather, the hash keys, a sort), so matched_idx, matched_val, labels, the sampled
rows and their order, the counts and the gathered sample must be equal exactly.

Losses and gradients, against float64 torch autograd on the same sample, within bounds derived from the kernels'
operation sequence (u = 2^-24, fp32 round to nearest; expf and logf within 1 ulp <= 2 u relative, the bound HIP's math
API documents; nothing comes from a device run).  Row i, logits x, m = max x, d_k = x_k - m <= 0, D = max |d_k|,
s = sum_k exp(d_k) in [1, C], label l, n rows:
  * d_k is one rounding, which moves exp(d_k) by |d_k| u; expf 2 u; C - 1 additions of positive terms (C - 1) u:
    s carries (D + C + 1) u relative, so log s moves by as much absolutely; logf adds 2 u log s <= 2 u log C;
    m + log s is one rounding, u |m + log s|; the subtraction of x_l one more, u |t_i| (t_i the row's term):
        E_i = u (D + C + 1 + 2 log C + |m + log s| + |t_i|);
  * the terms are added per thread in row order (r = ceil(n / (256 nblk)) rows each, nblk = min(512, ceil(n / 256))
    workgroups), in an 8-level tree per workgroup, then workgroup by workgroup: at most r + 8 + nblk additions lie on
    any term's path, each within u of a partial sum of magnitude <= sum |t_i|; the division by n is one more u:
        |cls - cls64| <= 1.01 (sum_i E_i + (r + 9 + nblk) u sum_i |t_i|) / n;
  * a box element smoothL1(|pred - target|): the difference is one rounding (u on d, 2 u on d^2), d * d u, / beta u,
    beta = fl(1/5) u: 5 u relative on the quadratic branch; d - 0.5 beta: u (d + 0.5 beta + term) <= 4 u term on the
    linear one (term >= 0.5 beta there); the branches agree to second order at d = beta, so a comparison decided the
    other way costs nothing at this order.  Six additions inside the row, then the same path: all terms are >= 0, so
        |box - box64| <= 1.01 (5 + 6 + r + 9 + nblk) u box64;
  * logit gradient (p_k - y_k) g / n: p_k = expf(d_k) / s carries (|d_k| + 2) u + (D + C + 1) u + u; the subtraction,
    fl(g / n) and the product u each on the result:
        |grad - grad64| <= 1.01 u ((|d_k| + D + C + 4) p_k |g| / n + 3 |grad64|) + 2^-126;
  * regression gradient h g / n, h = diff / beta or sign(diff): diff u, beta u, the division u, fl(g / n) u, the product
    u: 5 u |grad64| (a branch decided the other way at |diff| within rounding of beta moves h by <= 3 u, inside it).
    Where the exact gradient is zero the bound is zero: those stores must be exactly 0.
bf16 inputs are rounded first; the arithmetic is the same fp32, so the same bounds hold on the rounded values, and a bf16
gradient store must be the round-to-nearest-even of a value inside the bound (fp64_yardstick.assert_bf16_rounded)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import fp64_yardstick as Y
import oracle_lib as O
import roi_loss_ref as R
import roi_post_ref as RP

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
U = 2.0 ** -24
AUG = {"target_Y": 0.3, "target_Z": 0.4, "anchor_Y": 0.0, "anchor_Z": 0.0}
W = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _scenes(n_b, g_b, seed, append_gt=False, n_classes=4):
    """per scene: proposals from roi_post_ref.wall_proposals; ground truth = other walls from the same generator, the first
    min(G, n // 4) of them replaced by distinct proposals moved by a jitter of graded size (IoU spread from ~1 down to 0),
    so that matches, between-threshold cases and background all occur.  append_gt: the ground truth is appended to the
    proposals (what the RPN does with ADD_GT_PROPOSALS)."""
    rng = np.random.default_rng(seed)
    props, gts, tls = [], [], []
    for i, (n, g) in enumerate(zip(n_b, g_b)):
        p = RP.wall_proposals(n, seed * 100 + i)
        t = RP.wall_proposals(g, seed * 100 + 50 + i, n_gt=max(g, 1)).copy()
        k = min(g, n // 4)
        if k:
            rows = rng.choice(n, k, replace=False)
            scale = np.linspace(0.0, 1.0, k)[:, None] ** 2
            jit = rng.normal(0, 1, (k, 7)) * np.array([0.15, 0.15, 0.1, 0.05, 0.3, 0.2, 0.05]) * scale
            t[:k] = (p[rows] + jit).astype(F)
            t[:k, 3:6] = np.maximum(t[:k, 3:6], F(0.05))
        if append_gt:
            p = np.concatenate([p, t]).astype(F)
        props.append(np.ascontiguousarray(p, F))
        gts.append(np.ascontiguousarray(t, F))
        tls.append(rng.integers(1, n_classes, g).astype(np.int64))
    return props, gts, tls


def _aug4(aug):
    a = aug or {}
    return tuple(float(a.get(k, 0.0)) for k in ("target_Y", "target_Z", "anchor_Y", "anchor_Z"))


def _run_targets(props, gts, tls, fg, bg, seed, aug=AUG, B=500, frac=0.25, weights=W):
    """one call on the device, checked against values and decisions; returns (sample dicts as numpy, restatement, debug)"""
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    dbg = {}
    out = roi_glue.box_head_targets([_t(p) for p in props], [_t(g) for g in gts], [_t(l) for l in tls], fg, bg, aug, B,
                                    frac, weights, seed, debug=dbg)
    nb = len(props)
    assert len(out) == nb
    midx, mval = dbg["matched_idx"].cpu().numpy(), dbg["matched_val"].cpu().numpy()
    labels, regt = dbg["labels"].cpu().numpy(), dbg["regression_targets"].cpu().numpy()
    ious = [m.cpu().numpy() for m in dbg["iou"]]
    # ---- values
    worst = 0.0
    for b in range(nb):
        want = O.boxes_iou_3d(gts[b], props[b], _aug4(aug), -1, True)
        assert ious[b].shape == want.shape
        if want.size:
            worst = max(worst, float(np.abs(ious[b] - want).max()))
        np.testing.assert_allclose(ious[b], want, rtol=0, atol=2e-5)
    print("iou: max abs difference to the oracle %.3e" % worst)
    ref = R.targets_stage(ious, props, gts, tls, fg, bg, seed, B, frac, weights)
    o = 0
    for b in range(nb):
        n, g = len(props[b]), len(gts[b])
        sl = slice(o, o + n)
        r = ref[b]
        np.testing.assert_allclose(regt[sl], r["regression_targets"], rtol=1e-6, atol=1e-6)   # (still a value)
        if n and g:
            enc = BoxCoder3D(False, weights).encode(_t(gts[b][np.maximum(midx[sl], 0)]), _t(props[b])).cpu().numpy()
            assert (regt[sl].view(np.uint32) == enc.view(np.uint32)).all(), "scene %d: regression targets" % b
        elif n:
            assert (regt[sl] == 0).all() and (labels[sl] == 0).all() and (midx[sl] == -1).all()
        # ---- decisions
        assert midx[sl].tolist() == r["matched_idx"].tolist(), "scene %d: matched_idx" % b
        assert (mval[sl].view(np.uint32) == r["matched_val"].view(np.uint32)).all(), "scene %d: matched_val" % b
        assert labels[sl].tolist() == r["labels"].tolist(), "scene %d: labels" % b
        got = {k: v.cpu().numpy() for k, v in out[b].items()}
        assert got["rows"].dtype == np.int64 and got["labels"].dtype == np.int64
        assert got["rows"].tolist() == r["rows"].tolist(), "scene %d: sampled rows" % b
        info = dbg["info"][b]
        assert info == [len(r["rows"]), r["num_pos"], r["num_neg"], r["P"], r["N"], r["ignored"], 0, 0], (b, info)
        rows = r["rows"]
        assert got["labels"].tolist() == labels[sl][rows].tolist()
        assert (got["regression_targets"].view(np.uint32) == regt[sl][rows].view(np.uint32)).all()
        assert (got["bbox3d"].view(np.uint32) == props[b][rows].view(np.uint32)).all()
        m = len(rows)
        assert (dbg["samp_rows"][b, m:] == -1).all().item() and (dbg["samp_labels"][b, m:] == -1).all().item()
        assert (dbg["samp_targets"][b, m:] == 0).all().item() and (dbg["samp_boxes"][b, m:] == 0).all().item()
        out[b] = got
        o += n
    return out, ref, dbg


N16 = [0, 1, 1000, 2000] * 4
G16 = [0, 1, 37, 300, 1, 37, 300, 0, 37, 300, 0, 1, 300, 0, 1, 37]


@pytest.mark.parametrize("name,n_b,g_b,fg,bg,append", [
    ("one_scene", [1000], [37], 0.5, 0.5, False),
    ("four_mixed", [1000, 0, 1, 2000], [37, 1, 300, 0], 0.6, 0.3, False),
    ("four_appended", [1000, 2000, 1, 0], [37, 300, 1, 0], 0.5, 0.5, True),
    ("sixteen", N16, G16, 0.6, 0.3, False),
    ("sixteen_equal_thresholds", N16, G16[::-1], 0.5, 0.5, True),
    ("few_candidates", [300, 40, 1000], [5, 5, 2], 0.6, 0.3, False),
])
def test_targets_values_and_decisions(name, n_b, g_b, fg, bg, append):
    props, gts, tls = _scenes(n_b, g_b, len(name) + len(n_b), append)
    aug = None if append else AUG
    out, ref, dbg = _run_targets(props, gts, tls, fg, bg, 77, aug=aug)
    labs = [r["labels"] for r in ref]
    # the cases are really hit (on the restatement's result alone)
    for b, (n, g) in enumerate(zip(n_b, g_b)):
        if (n + g if append else n) == 0:
            assert len(out[b]["rows"]) == 0 and out[b]["bbox3d"].shape == (0, 7)
        if g == 0 and n:
            assert (labs[b] == 0).all() and ref[b]["num_pos"] == 0                    # an all-background scene
            assert ref[b]["num_neg"] == min(n, 500)
        if n >= 1000 and g >= 37:
            assert ref[b]["P"] > 0 and ref[b]["N"] > 0
        if append and g:
            mi, mv = ref[b]["matched_idx"][-g:], ref[b]["matched_val"][-g:]
            assert (np.abs(mv - 1.0) <= 2e-5).all()                                    # a box's IoU with itself
            assert (mi == np.arange(g)).mean() > 0.9 and (mi >= 0).all()
    if fg != bg:
        assert any((l == -1).any() for l in labs), "no proposal between the thresholds"
        for r in ref:
            assert (r["labels"][r["rows"]] >= 0).all()                                 # ignored rows are never sampled
    if name == "few_candidates":
        assert ref[0]["P"] + ref[0]["N"] < 500 and len(ref[0]["rows"]) == ref[0]["P"] + ref[0]["N"]
        assert 0 < ref[0]["P"] < 125 and ref[0]["num_pos"] == ref[0]["P"]              # fewer positives than num_pos_max
        assert len(ref[1]["rows"]) <= 40
    if name == "four_mixed":
        assert len(ref[2]["rows"]) == (1 if ref[2]["labels"][0] >= 0 else 0)           # the one-proposal scene
    if name == "sixteen":
        assert any(r["P"] > 125 and r["num_pos"] == 125 for r in ref), "the positive cut never acted"
        assert any(0 < r["P"] < 125 for r in ref)


def test_nan_entry_is_the_maximum(monkeypatch):
    """with the z factor on (only_xy off), two zero heights at the same z and no thickness clamp make it 0 / 0: the NaN
    entry wins its column, the first one by index, as in torch.max / np.argmax, and the proposal is matched to that box
    (roi_loss.hip states the rule).  Ground truth 20 and 3 of 37 are such boxes for proposal 5; 20 lies in a later
    lane's share than 3."""
    import _nms
    import roi_glue
    monkeypatch.setattr(_nms, "REFERENCE_DEBUG_ONLY_XY", False)
    props, gts, tls = _scenes([40], [37], 4)
    p, t = props[0].copy(), gts[0].copy()
    p[5, 5] = 0.0
    for g in (20, 3):
        t[g] = p[5]
    dbg = {}
    roi_glue.box_head_targets([_t(p)], [_t(t)], [_t(tls[0])], 0.6, 0.3, None, 500, 0.25, W, 1, debug=dbg)
    iou = dbg["iou"][0].cpu().numpy()
    assert np.isnan(iou[[3, 20], 5]).all() and np.isnan(iou).sum() == 2
    midx, mval = dbg["matched_idx"].cpu().numpy(), dbg["matched_val"].cpu().numpy()
    want_idx, want_val = R.match(iou, 0.6, 0.3)
    assert want_idx[5] == 3 and np.isnan(want_val[5])
    assert midx.tolist() == want_idx.tolist()
    assert (mval.view(np.uint32) == want_val.view(np.uint32)).all()
    assert dbg["labels"].cpu().numpy().tolist() == R.labels_of(want_idx, tls[0]).tolist()


def test_positive_cut_and_small_batch():
    """B = 64, fraction 0.5: num_pos = 32 of many positives; and B = 512 (the limit)"""
    props, gts, tls = _scenes([2000, 1000], [300, 37], 9)
    for B, frac in ((64, 0.5), (512, 0.25), (1, 1.0)):
        out, ref, _ = _run_targets(props, gts, tls, 0.5, 0.5, 5, B=B, frac=frac)
        assert ref[0]["P"] > int(B * frac) and ref[0]["num_pos"] == int(B * frac)
        assert len(ref[0]["rows"]) == B


def _reference(logits, reg, labels, tgt, class_specific):
    """float64 torch autograd of loss.py:328, 343-377 on the CPU (labels all inside [0, C)); g_cls = 1, g_box = 2"""
    x = logits.detach().double().cpu().requires_grad_()
    r = reg.detach().double().cpu().requires_grad_()
    lab, t = torch.as_tensor(labels), torch.as_tensor(tgt).double()
    pos = torch.nonzero(lab > 0).squeeze(1)
    lp = lab[pos]
    if class_specific:
        map_inds = 7 * lp[:, None] + torch.tensor([0, 1, 2, 3, 4, 5, 6])
        rp = r[pos[:, None], map_inds]
    else:
        rp = r[pos, :]
    d = torch.abs(rp - t[pos])
    box = torch.where(d < R.BETA, 0.5 * d ** 2 / R.BETA, d - 0.5 * R.BETA).sum() / lab.numel()
    cls = TF.cross_entropy(x, lab)
    (cls + 2 * box).backward()
    return cls.item(), box.item(), x.grad.numpy(), r.grad.numpy()


def _bounds(x64, labels, ce, cls64, box64, gx64, gr64, g_cls=1.0):
    """the docstring's bounds: (cls, box, per-element logit gradient, per-element regression gradient)"""
    n, c = x64.shape
    nblk = min(512, max(1, -(-n // 256)))
    r = -(-n // (256 * nblk))
    m = x64.max(1, keepdims=True)
    d = np.abs(x64 - m)
    D = d.max(1)
    s = np.exp(x64 - m).sum(1)
    ok = (labels >= 0) & (labels < c)
    E = U * (D + c + 1 + 2 * np.log(c) + np.abs(m[:, 0] + np.log(s)) + np.abs(ce)) * ok
    b_cls = 1.01 * (E.sum() + (r + 9 + nblk) * U * np.abs(ce).sum()) / n
    b_box = 1.01 * (5 + 6 + r + 9 + nblk) * U * box64
    p = np.exp(x64 - m) / s[:, None]
    b_gx = (1.01 * U * ((d + D[:, None] + c + 4) * p * abs(g_cls) / n + 3 * np.abs(gx64)) + 2.0 ** -126) * ok[:, None]
    return b_cls, b_box, b_gx, 5 * U * np.abs(gr64)


def _sample_for_loss(c, seed=3):
    import roi_glue
    props, gts, tls = _scenes([1000, 300, 2000, 0], [37, 5, 300, 4], seed, n_classes=c)
    out = roi_glue.box_head_targets([_t(p) for p in props], [_t(g) for g in gts], [_t(l) for l in tls], 0.6, 0.3, AUG, 500,
                                    0.25, W, 11)
    labels = torch.cat([o["labels"] for o in out])
    tgt = torch.cat([o["regression_targets"] for o in out])
    assert (labels > 0).sum().item() > 100 and (labels == 0).sum().item() > 100 and labels.max().item() == c - 1
    return labels, tgt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("class_specific", [True, False])
@pytest.mark.parametrize("c", [2, 4, 7])
def test_losses_and_gradients_within_derived_bounds(c, class_specific, dtype):
    _check_losses_and_gradients(*_sample_for_loss(c), c, class_specific, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("class_specific", [True, False])
def test_losses_and_gradients_c33_two_workgroups(class_specific, dtype):
    """C = 33: one column more than the separated-classifier group tables can hold (csrc/sep_groups.h) -- the plain loss
    has no such limit.  257 rows are two workgroups, the second with a single row (the workgroup-order sum and the tail
    guard); the labels i % 33 meet every class and the background."""
    n, c = 257, 33
    labels = (torch.arange(n) % c).to(DEV)
    tgt = (torch.randn(n, 7, generator=torch.Generator().manual_seed(33)) * 0.3).to(DEV)
    _check_losses_and_gradients(labels, tgt, c, class_specific, dtype)


def _check_losses_and_gradients(labels, tgt, c, class_specific, dtype):
    import roi_glue
    n = labels.numel()
    g = torch.Generator().manual_seed(c * 4 + class_specific)
    logits = (torch.randn(n, c, generator=g) * 2).to(DEV, dtype).requires_grad_()
    reg = (torch.randn(n, 7 * c if class_specific else 7, generator=g) * 0.3).to(DEV, dtype)
    reg = (reg.float() + tgt.repeat(1, c if class_specific else 1) * 0.9).to(dtype).requires_grad_()   # both branches
    cls, box, flag = roi_glue.box_head_loss(logits, reg, labels, tgt, return_flag=True)        # told from the width
    assert cls.dtype == box.dtype == torch.float32 and cls.dim() == box.dim() == 0
    (cls + 2 * box).backward()
    assert flag.item() == 0
    assert logits.grad.dtype == dtype and reg.grad.dtype == dtype and reg.grad.shape == reg.shape
    lab_np, tgt_np = labels.cpu().numpy(), tgt.cpu().numpy()
    x64 = logits.detach().float().cpu().numpy().astype(np.float64)          # bf16 inputs: the rounded values
    r64 = reg.detach().float().cpu().numpy().astype(np.float64)
    cls64, box64, gx64, gr64 = _reference(logits.detach().float(), reg.detach().float(), lab_np, tgt_np, class_specific)
    c2, b2, gx2, gr2, ce, bx = R.loss_and_grads(x64, r64, lab_np, tgt_np, class_specific)
    np.testing.assert_allclose([c2, b2], [cls64, box64], rtol=1e-12)        # the restatement is the autograd composition
    np.testing.assert_allclose(gx2, gx64, rtol=1e-10, atol=1e-16)
    np.testing.assert_allclose(gr2 * 2, gr64, rtol=1e-10, atol=1e-16)
    b_cls, b_box, b_gx, b_gr = _bounds(x64, lab_np, ce, cls64, box64, gx64, gr64)
    e_cls, e_box = abs(cls.item() - cls64), abs(box.item() - box64)
    print("cls %.8g err %.3e bound %.3e | box %.8g err %.3e bound %.3e" % (cls64, e_cls, b_cls, box64, e_box, b_box))
    assert e_cls <= b_cls and e_box <= b_box
    gx, gr = logits.grad.float().cpu().numpy().astype(np.float64), reg.grad.float().cpu().numpy().astype(np.float64)
    assert (gr[gr64 == 0] == 0).all(), "a regression gradient that is exactly zero was stored as non-zero"
    assert (gr64 != 0).sum() == 7 * (lab_np > 0).sum()
    if dtype == torch.float32:
        print("grad logits max err / bound %.3f, grad reg %.3f" % ((np.abs(gx - gx64) / b_gx).max(),
                                                                    (np.abs(gr - gr64)[gr64 != 0] / b_gr[gr64 != 0]).max()))
        assert (np.abs(gx - gx64) <= b_gx).all() and (np.abs(gr - gr64) <= b_gr).all()
    else:
        Y.assert_bf16_rounded(logits.grad, gx64, b_gx, "logit gradient")
        Y.assert_bf16_rounded(reg.grad, gr64, b_gr, "regression gradient")


def test_empty_sample_and_out_of_range_label():
    """N_s == 0: NaN losses, empty gradients, no flag; a label outside [0, C): flag set, nothing read out of bounds, the
    row adds nothing and its gradients are exactly zero, every other row within the bounds, all gradients finite"""
    import roi_glue
    out = roi_glue.box_head_targets([_t(np.zeros((0, 7), F))] * 2, [_t(RP.wall_proposals(3, 1)), _t(np.zeros((0, 7), F))],
                                    [_t(np.ones(3, np.int64)), _t(np.zeros(0, np.int64))], seed=1)
    assert [len(o["rows"]) for o in out] == [0, 0]
    lg = torch.zeros((0, 4), device=DEV, requires_grad=True)
    rg = torch.zeros((0, 28), device=DEV, requires_grad=True)
    cls, box, flag = roi_glue.box_head_loss(lg, rg, torch.cat([o["labels"] for o in out]),
                                            torch.cat([o["regression_targets"] for o in out]), return_flag=True)
    (cls + box).backward()
    assert np.isnan(cls.item()) and np.isnan(box.item()) and flag.item() == 0
    assert lg.grad.shape == (0, 4) and rg.grad.shape == (0, 28)
    c = 4
    labels, tgt = _sample_for_loss(c)
    n = labels.numel()
    lab = labels.clone()
    bad = [3, n // 2, n - 1]
    lab[bad[0]], lab[bad[1]], lab[bad[2]] = c, -1, 1 << 40
    g = torch.Generator().manual_seed(2)
    for class_specific in (True, False):
        logits = (torch.randn(n, c, generator=g) * 2).to(DEV).requires_grad_()
        reg = (torch.randn(n, 7 * c if class_specific else 7, generator=g) * 0.3).to(DEV).requires_grad_()
        cls, box, flag = roi_glue.box_head_loss(logits, reg, lab, tgt, class_specific=class_specific, return_flag=True)
        (cls + 2 * box).backward()
        assert flag.item() == 1
        gx, gr = logits.grad.cpu().numpy().astype(np.float64), reg.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(gx).all() and np.isfinite(gr).all() and np.isfinite([cls.item(), box.item()]).all()
        assert (gx[bad] == 0).all() and (gr[bad] == 0).all()
        lab_np, tgt_np = lab.cpu().numpy(), tgt.cpu().numpy()
        x64, r64 = logits.detach().cpu().numpy().astype(np.float64), reg.detach().cpu().numpy().astype(np.float64)
        c2, b2, gx64, gr64, ce, bx = R.loss_and_grads(x64, r64, lab_np, tgt_np, class_specific)
        b_cls, b_box, b_gx, b_gr = _bounds(x64, lab_np, ce, c2, b2, gx64, 2 * gr64)
        assert abs(cls.item() - c2) <= b_cls and abs(box.item() - b2) <= b_box
        assert (np.abs(gx - gx64) <= b_gx).all() and (np.abs(gr - 2 * gr64) <= b_gr).all()
        assert (gr[gr64 == 0] == 0).all()


def test_determinism_seeds_and_no_host_sync():
    import roi_glue
    props, gts, tls = _scenes([1000, 2000, 300, 0], [37, 300, 5, 1], 21)
    tp, tg, tl = [_t(p) for p in props], [_t(g) for g in gts], [_t(l) for l in tls]

    def run(seed):
        dbg = {}
        out = roi_glue.box_head_targets(tp, tg, tl, 0.6, 0.3, AUG, 500, 0.25, W, seed, debug=dbg)
        keys = ("matched_idx", "matched_val", "labels", "regression_targets", "samp_rows", "samp_labels", "samp_targets",
                "samp_boxes")
        return out, [dbg[k].cpu().numpy().tobytes() for k in keys] + [m.cpu().numpy().tobytes() for m in dbg["iou"]], dbg["info"]

    a, ba, ia = run(7)
    b, bb, ib = run(7)
    c, bc, ic = run(8)
    assert ba == bb and ia == ib
    assert ia == ic, "another seed must draw the same counts"
    assert any(not torch.equal(x["rows"], y["rows"]) for x, y in zip(a, c)), "another seed must draw another sample"
    assert bc[:4] == ba[:4]                                                       # the per-proposal results do not depend on it
    torch.manual_seed(11)
    s1 = roi_glue.box_head_targets(tp, tg, tl, 0.6, 0.3, AUG)
    torch.manual_seed(11)
    s2 = roi_glue.box_head_targets(tp, tg, tl, 0.6, 0.3, AUG)
    assert all(torch.equal(x["rows"], y["rows"]) for x, y in zip(s1, s2))
    labels = torch.cat([o["labels"] for o in a])
    tgt = torch.cat([o["regression_targets"] for o in a])
    n = labels.numel()
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(n, 4, generator=g).to(DEV).requires_grad_()
    reg = (torch.randn(n, 28, generator=g) * 0.3).to(DEV).requires_grad_()
    res = []
    for _ in range(2):
        logits.grad = reg.grad = None
        cls, box = roi_glue.box_head_loss(logits, reg, labels, tgt)
        (cls + box).backward()
        res.append((cls.clone(), box.clone(), logits.grad.clone(), reg.grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        finish = roi_glue.box_head_targets(tp, tg, tl, 0.6, 0.3, AUG, 500, 0.25, W, 7, defer=True)
        cls, box = roi_glue.box_head_loss(logits, reg, labels, tgt)
        (cls + 2 * box).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    d = finish()
    assert all(torch.equal(x["rows"], y["rows"]) and torch.equal(x["bbox3d"], y["bbox3d"]) for x, y in zip(d, a))
    torch.cuda.synchronize()


class _Boxes(object):
    def __init__(self, bbox3d, size3d, labels=None):
        self.bbox3d, self.size3d, self.mode, self._labels = bbox3d, size3d, "yx_zb", labels

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def get_field(self, name):
        assert name == "labels"
        return self._labels


def test_through_the_object():
    """FastRCNNLossComputation.subsample then __call__ equals the two glue calls"""
    import roi_glue
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss import FastRCNNLossComputation
    props, gts, tls = _scenes([1000, 300, 0], [37, 5, 2], 31)
    size3d = torch.tensor([[0.0, 0.0, 0.0, 16.0, 12.0, 3.0]])
    sampler = BalancedPositiveNegativeSampler(500, 0.25)
    sampler.seed = 5
    for class_specific in (True, False):
        ev = FastRCNNLossComputation(Matcher(0.6, 0.3), sampler, BoxCoder3D(False, W), "Diff", True, AUG, None, class_specific)
        with pytest.raises(RuntimeError):
            ev(torch.zeros(1, 4, device=DEV), torch.zeros(1, 28, device=DEV), None)
        sub = ev.subsample([_Boxes(_t(p), size3d) for p in props], [_Boxes(_t(g), size3d, _t(l)) for g, l in zip(gts, tls)])
        want = roi_glue.box_head_targets([_t(p) for p in props], [_t(g) for g in gts], [_t(l) for l in tls], 0.6, 0.3, AUG,
                                         500, 0.25, W, 5)
        assert len(sub) == 3 and len(sub[2]) == 0
        for s, w in zip(sub, want):
            assert s.mode == "yx_zb" and s.size3d is size3d and set(s.fields()) >= {"labels", "regression_targets", "rows"}
            assert torch.equal(s.bbox3d, w["bbox3d"]) and torch.equal(s.get_field("labels"), w["labels"])
            assert torch.equal(s.get_field("regression_targets"), w["regression_targets"])
            assert torch.equal(s.get_field("rows"), w["rows"])
        n = sum(len(s) for s in sub)
        g = torch.Generator().manual_seed(6)
        logits = torch.randn(n, 4, generator=g).to(DEV).requires_grad_()
        reg = (torch.randn(n, 28 if class_specific else 7, generator=g) * 0.3).to(DEV).requires_grad_()
        cls, box, corner = ev(logits, reg, None)
        assert corner == {}
        assert ev.last_flag.dtype == torch.int32 and ev.last_flag.item() == 0
        (cls + box).backward()
        g1 = (logits.grad.clone(), reg.grad.clone())
        logits.grad = reg.grad = None
        c2, b2 = roi_glue.box_head_loss(logits, reg, torch.cat([w["labels"] for w in want]),
                                        torch.cat([w["regression_targets"] for w in want]), class_specific=class_specific)
        (c2 + b2).backward()
        assert torch.equal(cls, c2) and torch.equal(box, b2)
        assert torch.equal(g1[0], logits.grad) and torch.equal(g1[1], reg.grad)
        with pytest.raises(ValueError):
            ev(logits, reg, torch.zeros(n, 16, device=DEV))
        # a label the logits have no column for: skipped, and the object hands the flag on
        assert any((w["labels"] == 3).any().item() for w in want)
        cls3, box3, _ = ev(logits.detach()[:, :3].contiguous(), reg.detach()[:, :21 if class_specific else 7].contiguous(), None)
        assert ev.last_flag.item() == 1 and torch.isfinite(cls3).item() and torch.isfinite(box3).item()
