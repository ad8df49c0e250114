"""The box head with separated-classifier groups on the device (MODEL.SEPARATE_CLASSES: csrc/sep_groups.h, the grouped
entry points of csrc/roi_loss.hip and csrc/roi_post.hip, roi_glue.box_head_targets_grouped / box_head_loss_grouped /
box_detections_grouped, SeperateClassifier) against what the parent code can already do: the single-group calls run
once per group on gathered rows and columns, and the restatements tests/sep_ref.py, roi_loss_ref.py, roi_post_ref.py.

Targets.  A segment (scene, group) must be to the grouped call what a scene is to box_head_targets: the same kernels run
on the same values in the same order, so everything is compared bit for bit with box_head_targets run on the segments
as scenes, the ground truth filtered and ordered on the host (sep_ref.filter_gt) and the labels remapped.

Losses and gradients, against float64 torch autograd of the per-group definition, within the bounds test_gpu_roi_loss.py
derives from the kernel's operation sequence, restated for a group (u = 2^-24; expf / logf within 2 u relative).  The
grouped kernels run the same statements per row with the group's c_g columns in place of C, keep one accumulator set per
group, and divide by the group's row count n_g.  Row i of group g, x its c_g logits, m = max x, d_k = x_k - m,
D = max |d_k|, s = sum exp(d_k) in [1, c_g], t_i its cross-entropy term:
  * E_i = u (D + c_g + 1 + 2 log c_g + |m + log s| + |t_i|), as there with c_g for C;
  * the terms of a group are added per thread in row order -- a thread meets at most r = ceil(n / (256 nblk)) rows of ALL
    groups (n the total row count, nblk = min(512, ceil(n / 256)) workgroups), so at most r of one group --, in the 8-level
    tree, then workgroup by workgroup: at most r + 8 + nblk additions on a term's path; the division by n_g (an integer
    below 2^24, exact in fp32) is one more rounding:
        |cls_g - cls64_g| <= 1.01 (sum_{i in g} E_i + (r + 9 + nblk) u sum_{i in g} |t_i|) / n_g;
  * the box term: 5 u on an element, six additions in the row, the same path: |box_g - box64_g| <= 1.01 (20 + r + nblk) u box64_g;
  * logit gradient (p_k - y_k) g_g / n_g on the group's columns:
        |grad - grad64| <= 1.01 u ((|d_k| + D + c_g + 4) p_k |g_g| / n_g + 3 |grad64|) + 2^-126,
    and exactly 0 on every column outside the row's group;
  * regression gradient: 5 u |grad64|, exactly 0 where the exact gradient is 0.
bf16 inputs are rounded first; a bf16 gradient store must be the round-to-nearest-even of a value inside the bound.

Detections.  `prob` per element against the fp64 softmax over the row's group columns within test_gpu_roi_post's bound
with c_g for C (so a group's columns sum to 1 within the sum of their bounds), exact zeros elsewhere, the decode bit-equal
to BoxCoder3D.decode; the decisions exactly equal to sep_ref.stage_b_grouped fed the device's own prob and boxes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import fp64_yardstick as Y
import roi_loss_ref as R
import roi_pool_ref as P
import roi_post_ref as RP
import sep_ref as SR

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
U = 2.0 ** -24
AUG = {"target_Y": 0.3, "target_Z": 0.4, "anchor_Y": 0.0, "anchor_Z": 0.0}
W = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0)
GROUPS = [[0, 2, 3, 6], [7, 1], [8, 4, 5]]
G2 = [[0, 2, 3, 4], [5, 1]]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ targets
def _segment(n, classes, g, seed):
    """n proposals of a segment and g ground-truth boxes for it with labels drawn from `classes`: the first
    min(g, n // 4) boxes are proposals moved by a jitter of graded size (matches, between-threshold cases and background
    all occur), the rest other walls"""
    rng = np.random.default_rng(seed)
    p = RP.wall_proposals(n, seed)
    t = RP.wall_proposals(g, seed + 50, n_gt=max(g, 1)).copy()
    k = min(g, n // 4)
    if k:
        rows = rng.choice(n, k, replace=False)
        scale = np.linspace(0.0, 1.0, k)[:, None] ** 2
        t[:k] = (p[rows] + rng.normal(0, 1, (k, 7)) * np.array([0.15, 0.15, 0.1, 0.05, 0.3, 0.2, 0.05]) * scale).astype(F)
        t[:k, 3:6] = np.maximum(t[:k, 3:6], F(0.05))
    return np.ascontiguousarray(p, F), np.ascontiguousarray(t, F), rng.choice(classes, g).astype(np.int64)


def _grouped_case(sizes, gt_counts, groups, seed):
    """per scene: group-major proposals, the whole ground truth (the groups' boxes shuffled together, ORIGINAL labels)"""
    rng = np.random.default_rng(seed)
    props, gts, tls = [], [], []
    for b, (sz, gc) in enumerate(zip(sizes, gt_counts)):
        ps, ts, ls = [], [], []
        for g, (n, k) in enumerate(zip(sz, gc)):
            p, t, l = _segment(n, groups[g][1:], k, seed * 100 + b * 10 + g)
            ps.append(p), ts.append(t), ls.append(l)
        order = rng.permutation(sum(gc))
        props.append(np.concatenate(ps))
        gts.append(np.concatenate(ts)[order])
        tls.append(np.concatenate(ls)[order])
    return props, gts, tls


def _segments_as_scenes(props, sizes, gts, tls, groups):
    """the per-group loop's inputs: every segment a scene, its ground truth filtered, ordered and relabelled on the host"""
    sp, sg, sl, srows = [], [], [], []
    for p, sz, t, l in zip(props, sizes, gts, tls):
        o = 0
        for g, n in enumerate(sz):
            rows, local = SR.filter_gt(l, groups, g)
            sp.append(p[o:o + n]), sg.append(t[rows]), sl.append(local), srows.append(rows)
            o += n
    return sp, sg, sl, srows


SAMP = ("samp_rows", "samp_labels", "samp_targets", "samp_boxes", "labels", "regression_targets", "matched_val")


def _check_identity(props, sizes, gts, tls, groups, seed, B=500, frac=0.25, fg=0.6, bg=0.3, aug=AUG):
    import roi_glue
    G = len(groups)
    dbg, ref_dbg = {}, {}
    out = roi_glue.box_head_targets_grouped([_t(p) for p in props], sizes, [_t(t) for t in gts], [_t(l) for l in tls], groups,
                                            fg, bg, aug, B, frac, W, seed, debug=dbg)
    sp, sg, sl, srows = _segments_as_scenes(props, sizes, gts, tls, groups)
    ref = roi_glue.box_head_targets([_t(p) for p in sp], [_t(t) for t in sg], [_t(l) for l in sl], fg, bg, aug, B, frac, W,
                                    seed, debug=ref_dbg)
    for k in SAMP:
        a, b = dbg[k].cpu().numpy(), ref_dbg[k].cpu().numpy()
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert dbg["info"] == ref_dbg["info"]
    # matched_idx: the row in the scene's ORIGINAL ground-truth list
    mi, want, o = dbg["matched_idx"].cpu().numpy(), ref_dbg["matched_idx"].cpu().numpy().copy(), 0
    for p, rows in zip(sp, srows):
        w = want[o:o + len(p)]
        w[w >= 0] = rows[w[w >= 0]]
        o += len(p)
    assert mi.tolist() == want.tolist()
    # the per-scene lists: the groups' samples one after the other
    for b, d in enumerate(out):
        seg = ref[b * G:(b + 1) * G]
        first = np.concatenate([[0], np.cumsum(sizes[b])[:-1]])
        assert torch.equal(d["rows"], torch.cat([s["rows"] + int(o) for s, o in zip(seg, first)]))
        for k in ("bbox3d", "labels", "regression_targets"):                # (bits: a target may be NaN)
            want_k = torch.cat([s[k] for s in seg])
            assert d[k].shape == want_k.shape and d[k].cpu().numpy().tobytes() == want_k.cpu().numpy().tobytes(), k
        assert d["sep_counts"] == [len(s["rows"]) for s in seg]
        assert d["sep_id"].dtype == torch.int32
        assert d["sep_id"].tolist() == [g for g, s in enumerate(seg) for _ in range(len(s["rows"]))]
        cn = torch.tensor([len(c) for c in groups], device=DEV)[d["sep_id"].long()]
        assert bool(((d["labels"] >= 0) & (d["labels"] < cn)).all())
    return out, dbg, ref_dbg


def test_targets_equal_the_per_group_loop_bit_for_bit():
    """2 scenes x 3 groups; segment sizes 0, 1, 17 and 300; scene 0 has 130 boxes of group 0 (a second LDS chunk) and none
    of group 1; the labels of a group's boxes are mixed and their rows shuffled among the other groups'"""
    sizes = [[300, 17, 0], [1, 300, 17]]
    gt_counts = [[130, 0, 9], [5, 37, 3]]
    props, gts, tls = _grouped_case(sizes, gt_counts, GROUPS, 3)
    assert not (tls[0] == 1).any() and (np.isin(tls[0], [2, 3, 6])).sum() == 130
    out, dbg, ref_dbg = _check_identity(props, sizes, gts, tls, GROUPS, seed=11)
    info = dbg["info"]
    assert info[1][0] == 17 and info[1][1] == 0, "a segment without ground truth of its group: all background"
    assert not dbg["regression_targets"][300:317].any()
    assert info[2][0] == 0 and info[3][0] <= 1, "the empty segment and the one-row segment"
    assert info[0][1] > 0 and info[4][1] > 0, "positives occur"
    lab = dbg["labels"].cpu().numpy()
    assert (lab[:300] == -1).any() and set(np.unique(lab[:300])) >= {0, 1, 2, 3}
    # a smaller batch per segment, and the positive cut
    _check_identity(props, sizes, gts, tls, GROUPS, seed=12, B=64, frac=0.25)
    # two groups
    sizes2 = [[40, 9], [0, 33]]
    p2, g2, l2 = _grouped_case(sizes2, [[7, 3], [4, 6]], G2, 5)
    _check_identity(p2, sizes2, g2, l2, G2, seed=13)


def test_targets_tie_goes_to_the_lower_group_local_label():
    """two identical ground-truth boxes of classes 5 and 4 (group 2: local 2 and 1), the class-5 box first in the scene's
    list: a proposal equal to them is matched to the class-4 box, the lower group-local label"""
    import roi_glue
    sizes = [[4, 0, 30]]
    props, gts, tls = _grouped_case(sizes, [[2, 0, 6]], GROUPS, 8)
    rows2 = np.nonzero(np.isin(tls[0], [4, 5]))[0]
    a, b = rows2[0], rows2[-1]
    tls[0][a], tls[0][b] = 5, 4
    props[0][4 + 7, 0] += 500.0                                   # (away from every other box)
    gts[0][a] = gts[0][b] = props[0][4 + 7]
    out, dbg, _ = _check_identity(props, sizes, gts, tls, GROUPS, seed=2, aug=None)
    assert dbg["matched_idx"][4 + 7].item() == b > a and dbg["labels"][4 + 7].item() == 1
    assert dbg["matched_val"][4 + 7].item() > 0.99


def test_targets_nan_entry_wins(monkeypatch):
    """test_gpu_roi_loss.test_nan_entry_is_the_maximum's construction inside a group: with the z factor on, two zero
    heights at the same z give 0 / 0; the NaN entry wins, the first one in the group's order (group-local label, row)"""
    import _nms
    monkeypatch.setattr(_nms, "REFERENCE_DEBUG_ONLY_XY", False)
    sizes = [[3, 40, 0]]
    props, gts, tls = _grouped_case(sizes, [[4, 0, 37]], GROUPS, 4)
    gts[0] = np.concatenate([gts[0], np.zeros((2, 7), F)])
    tls[0] = np.concatenate([tls[0], [1, 1]])                    # group 1's only ground truth: the two NaN boxes
    props[0][3 + 5, 5] = 0.0
    gts[0][-2:] = props[0][3 + 5]
    out, dbg, ref_dbg = _check_identity(props, sizes, gts, tls, GROUPS, seed=1, aug=None)
    assert np.isnan(dbg["matched_val"][3 + 5].item()) and np.isnan(dbg["matched_val"].cpu().numpy()).sum() == 1
    assert dbg["matched_idx"][3 + 5].item() == len(tls[0]) - 2 and dbg["labels"][3 + 5].item() == 1


# --------------------------------------------------------------------------------------------------------------- loss
def _loss_inputs(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    sep = torch.randint(0, 3, (n,), generator=g)
    cn = torch.tensor([len(c) for c in GROUPS])
    lab = (torch.rand(n, generator=g) * cn[sep]).long().clamp(max=3)
    lab = torch.minimum(lab, cn[sep] - 1)
    tgt = torch.randn(n, 7, generator=g) * 0.3
    logits = (torch.randn(n, 9, generator=g) * 2).to(dtype)
    reg = ((torch.randn(n, 7, generator=g) * 0.3) + tgt * 0.9).to(dtype)                # both smooth-L1 branches
    return logits, reg, sep.to(torch.int32), lab, tgt


def _reference_grouped(logits, reg, sep, lab, tgt, g_cls, g_box):
    """float64 torch autograd of the per-group definition on the CPU.  A row whose sep_id is outside [0, G) is in no group;
    a row whose label is outside its group's range counts in n_g and adds nothing (this project's rule).  Returns per
    group cls, box, n_g, and the gradients of sum_g (g_cls[g] cls_g + g_box[g] box_g) over the groups with rows; plus the
    per-row terms and statistics the bounds need."""
    x = logits.detach().float().double().cpu().requires_grad_()
    r = reg.detach().float().double().cpu().requires_grad_()
    sep, lab, t = sep.cpu().long(), lab.cpu().long(), tgt.cpu().double()
    n = x.shape[0]
    cls, box, ng, total = [], [], [], 0.0
    ce = np.zeros(n)
    for g, cols in enumerate(GROUPS):
        rows = torch.nonzero(sep == g).squeeze(1)
        ok = rows[(lab[rows] >= 0) & (lab[rows] < len(cols))]
        ng.append(len(rows))
        if len(rows) == 0:
            cls.append(float("nan")), box.append(float("nan"))
            continue
        terms = TF.cross_entropy(x[ok][:, cols], lab[ok], reduction="none")
        ce[ok.numpy()] = terms.detach().numpy()
        c = terms.sum() / len(rows)
        pos = ok[lab[ok] > 0]
        d = torch.abs(r[pos] - t[pos])
        bx = torch.where(d < R.BETA, 0.5 * d ** 2 / R.BETA, d - 0.5 * R.BETA).sum() / len(rows)
        total = total + g_cls[g] * c + g_box[g] * bx
        cls.append(c.item()), box.append(bx.item())
    if torch.is_tensor(total):
        total.backward()
    gx = x.grad.numpy() if x.grad is not None else np.zeros((n, 9))
    gr = r.grad.numpy() if r.grad is not None else np.zeros((n, 7))
    return cls, box, ng, gx, gr, ce


def _bounds_grouped(x64, sep, lab, ce, cls64, box64, ng, gx64, gr64, g_cls):
    """the docstring's bounds: per group (cls, box), per element the logit and the regression gradient"""
    n = x64.shape[0]
    nblk = min(512, max(1, -(-n // 256)))
    r = -(-n // (256 * nblk))
    b_cls, b_box = [], []
    b_gx = np.zeros_like(gx64)
    for g, cols in enumerate(GROUPS):
        rows = np.nonzero(sep == g)[0]
        ok = rows[(lab[rows] >= 0) & (lab[rows] < len(cols))]
        if len(rows) == 0:
            b_cls.append(0.0), b_box.append(0.0)
            continue
        c = len(cols)
        xg = x64[ok][:, cols]
        m = xg.max(1, keepdims=True)
        d = np.abs(xg - m)
        D = d.max(1)
        s = np.exp(xg - m).sum(1)
        E = U * (D + c + 1 + 2 * np.log(c) + np.abs(m[:, 0] + np.log(s)) + np.abs(ce[ok]))
        b_cls.append(1.01 * (E.sum() + (r + 9 + nblk) * U * np.abs(ce[ok]).sum()) / len(rows))
        b_box.append(1.01 * (5 + 6 + r + 9 + nblk) * U * box64[g])
        p = np.exp(xg - m) / s[:, None]
        b_gx[np.ix_(ok, cols)] = (1.01 * U * ((d + D[:, None] + c + 4) * p * abs(g_cls[g]) / len(rows)
                                              + 3 * np.abs(gx64[np.ix_(ok, cols)])) + 2.0 ** -126)
    return b_cls, b_box, b_gx, 5 * U * np.abs(gr64)


G_CLS, G_BOX = [1.0, 1.5, 2.0], [2.0, 1.75, 1.5]


def _run_loss(logits, reg, sep, lab, tgt):
    import roi_glue
    lg = logits.to(DEV).requires_grad_()
    rg = reg.to(DEV).requires_grad_()
    cls, box, flag = roi_glue.box_head_loss_grouped(lg, rg, sep.to(DEV), lab.to(DEV), tgt.to(DEV), GROUPS, return_flag=True)
    assert cls.shape == box.shape == (3,) and cls.dtype == box.dtype == torch.float32
    live = torch.nonzero(~torch.isnan(cls)).squeeze(1)
    gc, gb = torch.tensor(G_CLS, device=DEV), torch.tensor(G_BOX, device=DEV)
    if lg.shape[0]:
        ((cls * gc)[live].sum() + (box * gb)[live].sum()).backward()
    else:
        (cls.sum() + box.sum()).backward()
    return cls, box, flag, lg.grad, rg.grad


def _check_loss(logits, reg, sep, lab, tgt, dtype, want_flag=0):
    cls, box, flag, gx_t, gr_t = _run_loss(logits, reg, sep, lab, tgt)
    assert flag.item() == want_flag
    assert gx_t.dtype == dtype and gr_t.dtype == dtype and gx_t.shape == logits.shape and gr_t.shape == reg.shape
    cls64, box64, ng, gx64, gr64, ce = _reference_grouped(logits, reg, sep, lab, tgt, G_CLS, G_BOX)
    x64 = logits.float().numpy().astype(np.float64)
    sep_np, lab_np = sep.numpy().astype(np.int64), lab.numpy()
    b_cls, b_box, b_gx, b_gr = _bounds_grouped(x64, sep_np, lab_np, ce, cls64, box64, ng, gx64, gr64, G_CLS)
    for g in range(3):
        if ng[g] == 0:
            assert np.isnan(cls[g].item()) and np.isnan(box[g].item()), "a group without rows gives NaN"
            continue
        e_c, e_b = abs(cls[g].item() - cls64[g]), abs(box[g].item() - box64[g])
        print("group %d n_g %d: cls %.8g err %.3e bound %.3e | box %.8g err %.3e bound %.3e"
              % (g, ng[g], cls64[g], e_c, b_cls[g], box64[g], e_b, b_box[g]))
        assert e_c <= b_cls[g] and e_b <= b_box[g]
    gx, gr = gx_t.float().cpu().numpy().astype(np.float64), gr_t.float().cpu().numpy().astype(np.float64)
    foreign = np.ones_like(gx, bool)
    for g, cols in enumerate(GROUPS):
        foreign[np.ix_(np.nonzero(sep_np == g)[0], cols)] = False
    assert (gx[foreign] == 0).all(), "the gradient of a column outside the row's group must be exactly 0"
    assert (gr[gr64 == 0] == 0).all(), "a regression gradient that is exactly zero was stored as non-zero"
    if dtype == torch.float32:
        assert (np.abs(gx - gx64) <= b_gx).all() and (np.abs(gr - gr64) <= b_gr).all()
    elif gx.size:
        Y.assert_bf16_rounded(gx_t, gx64, b_gx, "logit gradient")
        Y.assert_bf16_rounded(gr_t, gr64, b_gr, "regression gradient")
    return cls, box, gx_t, gr_t, ng


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [0, 1, 300, 5000])
def test_grouped_losses_and_gradients_within_derived_bounds(n, dtype):
    logits, reg, sep, lab, tgt = _loss_inputs(n, dtype, 40 + n)
    cls, box, gx, gr, ng = _check_loss(logits, reg, sep, lab, tgt, dtype)
    if n >= 300:
        assert min(ng) > 50 and (lab == 0).sum() > 50 and (lab > 0).sum() > 50
    if n <= 1:
        assert sum(v == 0 for v in ng) == 3 - n, "a group without rows gives NaN, the other groups are unaffected"
    # two runs are bit-identical
    cls2, box2, _flag, gx2, gr2 = _run_loss(logits, reg, sep, lab, tgt)
    assert _bits(cls).tobytes() == _bits(cls2).tobytes() and _bits(box).tobytes() == _bits(box2).tobytes()
    assert torch.equal(gx, gx2) and torch.equal(gr, gr2)


def test_grouped_loss_empty_group_and_out_of_range_rows():
    """group 1 has no rows: NaN there, the others inside their bounds; a sep_id outside [0, G) or a label outside the
    group's range is never an index: the flag is raised, the row's gradients are exactly zero, a row with a bad label
    still counts in n_g"""
    logits, reg, sep, lab, tgt = _loss_inputs(700, torch.float32, 9)
    lab[sep == 1] = 0
    sep[sep == 1] = 2                                             # (label 0 is valid in every group)
    _, _, _, _, ng = _check_loss(logits, reg, sep, lab, tgt, torch.float32)
    assert ng[1] == 0 and ng[0] > 100 and ng[2] > 100
    logits, reg, sep, lab, tgt = _loss_inputs(700, torch.float32, 10)
    bad_sep, bad_lab = [3, 350], [10, 699]
    sep[bad_sep[0]], sep[bad_sep[1]] = 3, -1
    sep[bad_lab[0]], lab[bad_lab[0]] = 1, 2                       # group 1 has 2 columns
    lab[bad_lab[1]] = -1
    cls, box, gx, gr, ng = _check_loss(logits, reg, sep, lab, tgt, torch.float32, want_flag=1)
    assert not gx[bad_sep + bad_lab].any() and not gr[bad_sep + bad_lab].any()
    assert bool(torch.isfinite(cls).all()) and bool(torch.isfinite(gx).all())
    assert sum(ng) == 698


# --------------------------------------------------------------------------------------------------------- detections
def _prob_slack(xg, prob64):
    d = np.abs(xg - xg.max(1, keepdims=True))
    return prob64 * (d + d.max(1, keepdims=True) + xg.shape[1] + 4) * U * 1.01 + 2.0 ** -126


def _run_detections(logits, reg, props, sep_id, groups=GROUPS, **kw):
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    n_b = [len(p) for p in props]
    allp = np.concatenate(props)
    dbg = {}
    dets = roi_glue.box_detections_grouped(_t(logits), _t(reg), [_t(p) for p in props], _t(sep_id.astype(np.int32)), groups,
                                           weights=W, debug=dbg, **kw)
    prob, boxes = dbg["prob"].cpu().numpy(), dbg["boxes"].cpu().numpy()
    assert prob.shape == logits.shape and boxes.shape == (len(allp), 7)
    foreign = np.ones_like(prob, bool)
    for g, cols in enumerate(groups):
        rows = np.nonzero(sep_id == g)[0]
        foreign[np.ix_(rows, cols)] = False
        xg = logits[rows][:, cols].astype(np.float64)
        e = np.exp(xg - xg.max(1, keepdims=True))
        p64 = e / e.sum(1, keepdims=True)
        pg = prob[rows][:, cols].astype(np.float64)
        slack = _prob_slack(xg, p64)
        assert (np.abs(pg - p64) <= slack).all()
        assert (np.abs(pg.sum(1) - 1.0) <= slack.sum(1)).all(), "a row's group columns sum to 1"
    assert (prob[foreign] == 0).all() and not np.signbit(prob[foreign]).any(), "every other column is exactly 0"
    dec = BoxCoder3D(False, W).decode(_t(reg), _t(allp)).cpu().numpy()
    assert (_bits(boxes) == _bits(dec)).all()
    stats = []
    ref = SR.stage_b_grouped(prob, boxes, sep_id, n_b, groups, kw.get("score_thresh", 0.05), kw.get("nms", 0.5),
                             kw.get("nms_aug_thickness"), kw.get("detections_per_img", 100), stats=stats)
    out, r0 = [], 0
    for b, (d, (rows, labels)) in enumerate(zip(dets, ref)):
        g = {k: v.cpu().numpy() for k, v in d.items()}
        assert g["rows"].dtype == np.int64 and g["labels"].dtype == np.int64 and g["scores"].dtype == F
        assert g["rows"].tolist() == rows.tolist(), "scene %d: rows differ" % b
        assert g["labels"].tolist() == labels.tolist(), "scene %d: labels differ" % b
        p, bx = prob[r0:r0 + n_b[b]], boxes[r0:r0 + n_b[b]]
        assert (g["scores"] == p[rows, labels]).all()
        assert (_bits(g["bbox3d"]) == _bits(bx[rows])).all()
        assert not np.isin(g["labels"], [c[0] for c in groups]).any(), "a background column is never a label"
        assert dbg["info"][b][0] == len(rows) and dbg["info"][b][1] == sum(s["M"] for s in stats[b])
        assert dbg["info"][b][2] == sum(sum(s["candidates"]) for s in stats[b]) and dbg["info"][b][5] == 0
        r0 += n_b[b]
        out.append(g)
    return out, stats, dbg


def _det_case(seed):
    """2 scenes x 400 wall-like proposals, mixed sep_id; scene 1 has no row of group 1"""
    rng = np.random.default_rng(seed)
    props = [RP.wall_proposals(400, 200 + seed), RP.wall_proposals(400, 300 + seed)]
    sep_id = rng.integers(0, 3, 800)
    sep_id[400:][sep_id[400:] == 1] = 2 * rng.integers(0, 2, (sep_id[400:] == 1).sum())
    logits = rng.normal(0, 2.0, (800, 9)).astype(F)
    reg = (rng.normal(0, 0.05, (800, 7)) * np.array([1, 1, 1, 1, 1, 1, 0.3]) * np.array(W)).astype(F)
    return logits, reg, props, sep_id


def test_grouped_detections_main_case():
    logits, reg, props, sep_id = _det_case(0)
    out, stats, _ = _run_detections(logits, reg, props, sep_id, nms_aug_thickness=(0.2, 0.2), detections_per_img=100)
    assert not (sep_id[400:] == 1).any() and stats[1][1]["M"] == 0, "a group without rows in a scene"
    assert all(s["M"] > 0 for s in stats[0]) and len(out[0]["rows"]) > 0
    assert any(sum(s["candidates"]) > sum(s["survivors"]) > 0 for s in stats[0]), "suppression acts"
    # the groups come in ascending order, each group's columns in group-local order
    for b in range(2):
        grp = np.array([[g for g, c in enumerate(GROUPS) if l in c][0] for l in out[b]["labels"]])
        assert (np.diff(grp) >= 0).all()
        assert (sep_id[400 * b:400 * (b + 1)][out[b]["rows"]] == grp).all(), "a row is detected only in its own group"


def test_grouped_detections_per_group_cut_with_a_tie():
    """detections_per_img = 5 acts per (scene, group): group 0 has four equal scores straddling its 5th place and keeps
    7, group 1 keeps exactly 5, group 2 has 3 candidates and keeps them all"""
    n = 120
    props = [RP.separated_proposals(n), RP.separated_proposals(n)]
    sep_id = np.zeros(2 * n, np.int64)
    sep_id[40:80] = 1
    sep_id[n + 40:n + 80] = 1
    sep_id[80:83] = 2
    sep_id[83:n] = 1
    sep_id[n + 80:] = 2
    logits = np.zeros((2 * n, 9), F)
    logits[:, [3, 6, 5]] = -20.0
    for b in range(2):
        for g, col in ((0, 2), (1, 1), (2, 4)):
            rows = np.nonzero(sep_id[b * n:(b + 1) * n] == g)[0] + b * n
            logits[rows, col] = np.linspace(6.0, 1.0, len(rows)).astype(F)
    logits[4:7] = logits[3]                                        # rows 3 .. 6 of scene 0, group 0: one score
    out, stats, dbg = _run_detections(logits, np.zeros((2 * n, 7), F), props, sep_id, detections_per_img=5)
    assert len(np.unique(dbg["prob"].cpu().numpy()[3:7, 2])) == 1
    s0 = stats[0]
    assert s0[0]["M"] == 40 and s0[0]["kept"] == 7, "ties at the cut all stay"
    assert s0[1]["M"] > 5 and s0[1]["kept"] == 5
    assert s0[2]["M"] == 3 == s0[2]["kept"], "fewer than the cut: all stay"
    assert out[0]["rows"].tolist()[:7] == list(range(7)) and len(out[0]["rows"]) == 15
    assert [s["kept"] for s in stats[1]] == [5, 5, 5]


def test_grouped_detections_negative_threshold_keeps_foreign_columns_out():
    """score_thresh < 0: every probability passes, an exact 0 of a foreign column too -- only the membership test keeps a
    row out of another group's columns"""
    logits, reg, props, sep_id = _det_case(1)
    out, stats, dbg = _run_detections(logits, reg, props, sep_id, score_thresh=-1.0, nms_aug_thickness=(0.2, 0.2),
                                      detections_per_img=50)
    for b in range(2):
        s = sep_id[400 * b:400 * (b + 1)]
        assert dbg["info"][b][2] == sum((s == g).sum() * (len(c) - 1) for g, c in enumerate(GROUPS))
        assert dbg["info"][b][2] < 400 * 6
    bad = sep_id.copy()
    bad[7], bad[405] = 3, -1                                        # out of range: no group's candidate, info[b][5] raised
    import roi_glue
    d2 = {}
    roi_glue.box_detections_grouped(_t(logits), _t(reg), [_t(p) for p in props], _t(bad.astype(np.int32)), GROUPS,
                                    score_thresh=-1.0, weights=W, debug=d2)
    assert d2["info"][0][5] == 1 and d2["info"][1][5] == 1
    assert not d2["prob"][[7, 405]].any()
    assert d2["info"][0][2] == dbg["info"][0][2] - (len(GROUPS[sep_id[7]]) - 1)


# ---------------------------------------------------------------------------------------------- no host synchronisation
class _CountingLib(object):
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("aabr_roi_") or "scratch" in name:
            return fn

        def counted(*a):
            self._calls.append(name)
            return fn(*a)
        return counted


def test_no_host_read_before_finish_and_calls_do_not_depend_on_g(monkeypatch):
    """test_gpu_roi_loss's method: with torch's sync debug mode on "error", the three grouped stages go out without a
    host read (`defer=True`); and the library is entered the same number of times at G = 2 and G = 3 -- every entry point
    issues a fixed number of launches (include/aabr_hip.h), so the launch count does not depend on G"""
    import _hip
    import roi_glue
    calls = []
    real = _hip.load()
    monkeypatch.setattr(roi_glue._hip, "load", lambda: _CountingLib(real, calls))
    per_g = {}
    for groups, sizes, gtc in ((G2, [[40, 9], [5, 33]], [[7, 3], [4, 6]]),
                               (GROUPS, [[40, 9, 12], [5, 33, 0]], [[7, 3, 5], [4, 6, 0]])):
        G, c_tot = len(groups), sum(len(c) for c in groups)
        props, gts, tls = _grouped_case(sizes, gtc, groups, 6)
        tp, tg, tl = [_t(p) for p in props], [_t(g) for g in gts], [_t(l) for l in tls]
        n = sum(len(p) for p in props)
        sep = _t(np.concatenate([np.repeat(np.arange(G), s) for s in sizes]).astype(np.int32))
        gen = torch.Generator().manual_seed(1)
        logits = torch.randn(n, c_tot, generator=gen).to(DEV)
        reg = (torch.randn(n, 7, generator=gen) * 0.1).to(DEV)

        def run():
            fin_t = roi_glue.box_head_targets_grouped(tp, sizes, tg, tl, groups, 0.6, 0.3, AUG, 16, 0.25, W, 7, defer=True)
            lab = torch.zeros(n, dtype=torch.int64, device=DEV)
            lg, rg = logits.clone().requires_grad_(), reg.clone().requires_grad_()
            cls, box = roi_glue.box_head_loss_grouped(lg, rg, sep, lab, torch.zeros(n, 7, device=DEV), groups)
            (cls.sum() + box.sum()).backward()
            fin_d = roi_glue.box_detections_grouped(logits, reg, tp, sep, groups, defer=True)
            return fin_t, fin_d
        want = [f() for f in run()]                                 # (buffers and the mailbox exist)
        torch.cuda.synchronize()
        calls.clear()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fins = run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        per_g[G] = list(calls)
        got = [f() for f in fins]
        for a, b in zip(want[0] + want[1], got[0] + got[1]):
            assert torch.equal(a["rows"], b["rows"]) and torch.equal(a["bbox3d"], b["bbox3d"])
    assert per_g[2] == per_g[3] == ["aabr_roi_gt_group_keys", "aabr_roi_targets_grouped", "aabr_roi_box_loss_grouped_forward",
                                    "aabr_roi_box_loss_grouped_backward", "aabr_roi_post_detections_grouped"]


# ------------------------------------------------------------------------------------------------ through the objects
class _Boxes(object):
    mode = "yx_zb"

    def __init__(self, bbox3d, labels=None):
        self.bbox3d, self.size3d, self._labels = bbox3d, torch.tensor([[0.0, 0.0, 0.0, 48.0, 40.0, 12.0]]), labels

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def get_field(self, name):
        assert name == "labels"
        return self._labels


@pytest.mark.parametrize("corner", [False, True])
def test_box_head_with_groups_through_the_objects(corner):
    """ROIBoxHead3D with classes (background, wall, door, window) and separated groups [[wall], [window]]: training gives
    finite per-group losses whose backward reaches the predictor; evaluation gives original labels, never a background
    column, and every detection in its own row's group"""
    import roi_glue
    import sparseconvnet as scn
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import build_roi_box_head
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
    res = (2, 11, 2) if corner else (2, 3, 2)
    case = P.PoolCase("sep_%d" % corner, 900 + corner, 8, res, 2, (23, 14))
    xs = [scn.InputLayer(3, [h + 3, w + 2, z + 1], mode=4)([_t(s.astype(np.int64)), _t(f)])
          for (h, w, z), s, f in zip(P.EXTENTS, case.sites, case.feats)]
    cfg = roi_glue.box_head_cfg(C=8, resolution=res, R=12, classes=("background", "wall", "door", "window"),
                                class_specific=False, separate=("wall", "window"), separate_ids=[[1], [3]], corner=corner,
                                scales=P.SCALES, canonical=P.CANONICAL, detections=20)
    torch.manual_seed(5)
    head = build_roi_box_head(cfg).to(DEV)
    sc = head.seperate_classifier
    assert head.need_seperate and sc.grouped_classes == [[0, 2], [4, 1], [5, 3]] and head.predictor.num_classes == 6
    head.loss_evaluator.fg_bg_sampler.seed = 9
    rng = np.random.default_rng(3)
    boxes, targets = [], []
    for b in case.boxes:
        sid = _t(rng.integers(0, 3, len(b)).astype(np.int32))
        boxes.append(DetectionList3D(_t(b), torch.tensor([[0.0, 0.0, 0.0, 48.0, 40.0, 12.0]]), {"sep_id": sid}))
        targets.append(_Boxes(_t(np.ascontiguousarray(b[:6])), _t(np.array([1, 2, 3, 1, 2, 3], np.int64))))
    head.train()
    x, props, losses = head(xs, boxes, targets)
    assert set(losses) == {"loss_%s_roi_%d" % (k, g) for k in ("classifier", "box_reg") for g in range(3)}
    assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in losses.values())
    for q, src in zip(props, boxes):
        sid, rows = q.get_field("sep_id").long(), q.get_field("rows")
        assert torch.equal(src.get_field("sep_id").long()[rows], sid), "a sampled row keeps its group"
        assert torch.equal(src.bbox3d[rows], q.bbox3d)
        assert bool((q.get_field("labels") < torch.tensor(sc.class_nums, device=DEV)[sid]).all())
        assert q.sep_counts == [int((sid == g).sum()) for g in range(3)]
    assert any(bool((q.get_field("labels") > 0).any()) for q in props)
    sum(losses.values()).backward()
    names = (("predictor.cls_score_body.weight", "predictor.bbox_pred_body.weight") if corner
             else ("predictor.cls_score.weight", "predictor.bbox_pred.weight"))
    for key in names:
        grad = dict(head.named_parameters())[key].grad
        assert grad is not None and float(grad.abs().max()) > 0 and bool(torch.isfinite(grad).all()), key
    head.eval()
    with torch.no_grad():
        x, dets, losses = head(xs, boxes, None)
    assert losses == {} and len(dets) == 2 and sum(len(d) for d in dets) > 0
    for d, src in zip(dets, boxes):
        lab, rows = d.get_field("labels"), d.get_field("rows")
        assert lab.dtype == torch.int64 and bool(((lab >= 1) & (lab <= 3)).all()), "original ids, never a background column"
        grp = torch.tensor([-1, 1, 0, 2], device=DEV)[lab]
        assert torch.equal(src.get_field("sep_id").long()[rows], grp)
        assert bool((torch.diff(grp) >= 0).all())
    # the reference-named methods give the values __call__ computed
    ev = head.loss_evaluator
    head.train()
    with torch.no_grad():
        x, props, losses = head(xs, boxes, targets)
        logits, reg = head.predictor(x)[:2]
        labels = torch.cat([q.get_field("labels") for q in props])
        tgt = torch.cat([q.get_field("regression_targets") for q in props])
        cls_l = sc.roi_cross_entropy_seperated(logits, labels, props)
        box_l, corner_l = sc.roi_box_loss_seperated(ev.box_loss, labels, reg, tgt, None, None)
    assert corner_l == [] and len(cls_l) == len(box_l) == 3 and all(v.dim() == 0 for v in cls_l + box_l)
    for g in range(3):
        assert torch.equal(cls_l[g], losses["loss_classifier_roi_%d" % g])
        assert torch.equal(box_l[g], losses["loss_box_reg_roi_%d" % g])
    # seperate_proposals: one sort, the rows of a group in ascending order
    pg, ids = sc.seperate_proposals(boxes)
    o = 0
    for b, src in enumerate(boxes):
        for g in range(3):
            want = torch.nonzero(src.get_field("sep_id") == g).squeeze(1)
            assert torch.equal(pg[g][b].bbox3d, src.bbox3d[want])
        o += len(src)
    assert torch.equal(ids[1], torch.cat([torch.nonzero(s.get_field("sep_id") == 1).squeeze(1) + off
                                          for s, off in zip(boxes, (0, len(boxes[0])))]))
    cat = sc.cat_boxlist_3d_seperated([pg[g] for g in range(3)])
    assert [c.sep_counts for c in cat] == [[len(pg[g][b]) for g in range(3)] for b in range(2)]
    assert all(bool((torch.diff(c.get_field("sep_id").long()) >= 0).all()) for c in cat)
