"""The RPN stages with separated-classifier groups on the device (rpn_glue.rpn_group_targets, rpn_label_matches_grouped,
rpn_loss_grouped, rpn_proposals_grouped, RPNModule with MODEL.SEPARATE_CLASSES) against the per-group loop built from the
single-group entry points: the grouped call of a stage gives, for every group, exactly what the plain call gives on that
group's slices of the head outputs and on that group's ground truth -- labels, selections, info words, losses and
gradients bit for bit, proposals torch.equal.  Inputs are small: 2 scenes (6 for the two-chunk case), 2 maps of a few
hundred sites, A = 2, G = 2 and 3, batch_size_per_image = 16 so that the sampler's cut bites."""
import numpy as np
import pytest
import torch

import sep_ref as SR
import synth_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = ("background", "wall", "door", "window")
GROUPS = {2: (("wall",), [[1]]), 3: (("wall", "window"), [[1], [3]])}
STRIDES = [[4.0] * 3, [8.0] * 3]
AUG = {"target_Y": 0.4, "anchor_Y": 0, "target_Z": 0.8, "anchor_Z": 0}
B = 16


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(ts):
    return b"".join(t.detach().float().cpu().numpy().tobytes() for t in ts)


class _Target(object):
    def __init__(self, b, labels):
        self.bbox3d, self.size3d, self._labels = b, None, labels

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def get_field(self, name):
        assert name == "labels"
        return self._labels


def _maps(nb, npts):
    """`nb` scenes, 2 maps of a few hundred sites, 32 channels: a strided convolution chain, no FPN"""
    import sparseconvnet as scn
    torch.manual_seed(2)
    locs, feats = S.make_batch(nb, npts, 31, 20)
    layer = scn.InputLayer(3, list(S.FULL_SCALE), mode=4)
    c1 = scn.Convolution(3, 9, 32, 2, 2, False).to(DEV)
    c2 = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
    c3 = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
    with torch.no_grad():
        x = layer([torch.as_tensor(locs).to(DEV), torch.as_tensor(feats).to(DEV)])
        m0 = c2(c1(x))
        m1 = c3(m0)
    return [m0, m1]


_cache = {}


def _inputs(nb):
    """maps, anchor generator and the scenes' labelled ground truth, made once per batch size and never changed.  Scene 1
    has no wall and no window: its segments of the named groups are empty."""
    if nb not in _cache:
        import rpn_glue
        from maskrcnn_benchmark.modeling.rpn.anchor_generator_sparse3d import make_anchor_generator
        maps = _maps(nb, 1500 if nb == 2 else 400)
        assert all(50 <= m.features.shape[0] <= 1500 * nb for m in maps), [m.features.shape for m in maps]
        gen = make_anchor_generator(rpn_glue.rpn_cfg(C=32, strides=STRIDES, voxel_scale=20.0))
        gts, labels = [], []
        for b in range(nb):
            n = 6 if b != 1 else 4
            gts.append(_t(S.make_gt_boxes(n, 3 + b)))
            labels.append(_t(np.array([1, 2, 3, 1, 2, 3][:n] if b != 1 else [2, 2, 2, 2], np.int64)))
        _cache[nb] = (maps, gen, gts, labels)
    return _cache[nb]


def _sc(G):
    from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
    return SeperateClassifier(GROUPS[G][1], len(CLASSES), False, "RPN")


def _head_outputs(maps, G, A, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    obj = [torch.randn(G, m.features.shape[0] * A, generator=g).to(DEV).to(dtype) for m in maps]
    reg = [(0.3 * torch.randn(G, m.features.shape[0] * A, 7, generator=g)).to(DEV).to(dtype) for m in maps]
    return obj, reg


def _labels(nb, G):
    """(grouped labels flat [nb G], group targets) -- also checked against the per-group call"""
    import rpn_glue
    maps, gen, gts, labels = _inputs(nb)
    boxes, local, rows, counts = rpn_glue.rpn_group_targets(gts, labels, _sc(G))
    flat = [boxes[b][g] for b in range(nb) for g in range(G)]
    lab = rpn_glue.rpn_label_matches_grouped(maps, gen.cell_anchors, STRIDES, 20.0, flat, G, AUG, 6, 0.55, 0.2,
                                             batch_size=nb, yaw_threshold=0.7)
    return lab, (boxes, local, rows, counts)


# ------------------------------------------------------------------------------------------------ targets and labels
@pytest.mark.parametrize("G", [2, 3])
def test_group_targets_and_labels_equal_the_per_group_calls(G):
    import _hip
    import rpn_glue
    nb = 2
    maps, gen, gts, labels = _inputs(nb)
    sc = _sc(G)
    reads = []
    orig = _hip.read_back
    _hip.read_back = lambda t: (reads.append(1), orig(t))[1]
    try:
        lab, (boxes, local, rows, counts) = _labels(nb, G)
    finally:
        _hip.read_back = orig
    assert len(reads) == 1                                                       # the counts, once
    for b in range(nb):
        for g in range(G):
            r, l = SR.filter_gt(labels[b].cpu().numpy(), sc.grouped_classes, g)
            assert rows[b][g].tolist() == r.tolist() and local[b][g].tolist() == l.tolist() and counts[b][g] == len(r)
            assert torch.equal(boxes[b][g], gts[b][_t(r)])
    assert counts[1][G - 1] == 0                                                 # a segment without ground truth
    for g in range(G):
        want = rpn_glue.rpn_label_matches(maps, gen.cell_anchors, STRIDES, 20.0, [boxes[b][g] for b in range(nb)], AUG, 6,
                                          0.55, 0.2, batch_size=nb, yaw_threshold=0.7, regression_targets=True)
        for b in range(nb):
            got = lab[b * G + g]
            assert torch.equal(got[0], want[b][0]) and _bits([got[1]]) == _bits([want[b][1]])
            assert got[2] is None and _bits([got[3]]) == _bits([want[b][3]])
    assert any(bool((l[0] >= 0).any()) for l in lab)
    assert bool((lab[1 * G + G - 1][0] < 0).all())                               # no ground truth: nothing positive


# ------------------------------------------------------------------------------------------------ the loss
def _loss_case(nb, G, dtype, kill_group=None, seed=77):
    import rpn_glue
    maps, gen, gts, labels = _inputs(nb)
    A = gen.num_anchors_per_location()
    lab, _ = _labels(nb, G)
    if kill_group is not None:                                                   # every anchor of one group ignored
        lab = [(torch.full_like(l[0], -2),) + tuple(l[1:]) if e % G == kill_group else l for e, l in enumerate(lab)]
    obj, reg = _head_outputs(maps, G, A, dtype, 5)
    leaves = [t.clone().requires_grad_(True) for t in obj + reg]
    lo, lb, sel, info = rpn_glue.rpn_loss_grouped(maps, leaves[:2], leaves[2:], lab, gen.cell_anchors, G, B, 0.5, "Diff",
                                                  seed=seed, return_samples=True)
    assert tuple(lo.shape) == tuple(lb.shape) == (G,) and tuple(sel.shape) == (nb * G, B) and tuple(info.shape) == (nb * G, 8)
    up_o, up_b = torch.linspace(0.5, 1.5, G, device=DEV), torch.linspace(2.0, 1.0, G, device=DEV)
    ((lo * up_o)[~torch.isnan(lo)].sum() + (lb * up_b)[~torch.isnan(lb)].sum() + 0 * lo.nansum()).backward()
    for g in range(G):
        pl = [t[g].clone().requires_grad_(True) for t in obj + reg]
        wo, wb, wsel, winfo = rpn_glue.rpn_loss(maps, pl[:2], pl[2:], [lab[b * G + g] for b in range(nb)], gen.cell_anchors,
                                                B, 0.5, "Diff", seed=seed, return_samples=True, return_info=True)
        print("G %d group %d: losses %.6g %.6g, N_s %d" % (G, g, float(wo.detach()), float(wb.detach()), int(winfo[0, 7])))
        assert _bits([lo[g]]) == _bits([wo]) and _bits([lb[g]]) == _bits([wb])
        assert torch.equal(sel[g::G], wsel) and torch.equal(info[g::G], winfo)
        if bool(torch.isnan(wo)):
            assert all(not bool(t.grad[g].any()) for t in leaves)
            continue
        (wo * up_o[g] + wb * up_b[g]).backward()
        for t, q in zip(leaves, pl):
            assert _bits([t.grad[g]]) == _bits([q.grad])
        assert float(leaves[0].grad[g].float().abs().max()) > 0
    return lo, lb, info


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G", [2, 3])
def test_grouped_loss_equals_the_plain_loss_per_group(G, dtype):
    lo, lb, info = _loss_case(2, G, dtype)
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(lb).all())
    assert int(info[:, 0].sum()) > 0 and int((info[:, 0] + info[:, 1]).max()) == B     # positives; the cut bites


def test_grouped_loss_over_two_chunks_of_segments():
    _loss_case(6, 3, torch.float32)                                              # 18 segments


def test_a_group_without_a_sample_gives_nan_losses_and_zero_gradients():
    lo, lb, info = _loss_case(2, 3, torch.float32, kill_group=1)
    assert bool(torch.isnan(lo[1])) and bool(torch.isnan(lb[1])) and int(info[1::3, 7].max()) == 0
    assert bool(torch.isfinite(lo[0])) and bool(torch.isfinite(lo[2]))


def test_seed_none_draws_one_seed_per_call():
    import rpn_glue
    maps, gen, gts, labels = _inputs(2)
    lab, _ = _labels(2, 2)
    obj, reg = _head_outputs(maps, 2, gen.num_anchors_per_location(), torch.float32, 5)
    torch.manual_seed(11)
    a = rpn_glue.rpn_loss_grouped(maps, obj, reg, lab, gen.cell_anchors, 2, B, 0.5, return_samples=True)
    torch.manual_seed(11)
    seed = rpn_glue.draw_seed()
    b = rpn_glue.rpn_loss_grouped(maps, obj, reg, lab, gen.cell_anchors, 2, B, 0.5, seed=seed, return_samples=True)
    assert torch.equal(a[2], b[2]) and _bits(a[:2]) == _bits(b[:2])


# ------------------------------------------------------------------------------------------------ proposals
@pytest.mark.parametrize("G", [2, 3])
def test_grouped_proposals_equal_the_plain_proposals_per_group_with_one_read(G):
    import _hip
    import rpn_glue
    nb = 2
    maps, gen, gts, labels = _inputs(nb)
    A = gen.num_anchors_per_location()
    obj, reg = _head_outputs(maps, G, A, torch.float32, 9)
    reads = []
    orig = _hip.read_back
    _hip.read_back = lambda t: (reads.append(1), orig(t))[1]
    try:
        fin = rpn_glue.rpn_proposals_grouped(maps, obj, reg, G, gen.cell_anchors, STRIDES, 20.0, 300, 60, 0.5, (0.3, 0.3),
                                             batch_size=nb, defer=True)
        assert reads == []                                                       # deferred: nothing read yet
        got = fin()
    finally:
        _hip.read_back = orig
    assert len(reads) == 1 and len(got) == G and all(len(s) == nb for s in got)
    for g in range(G):
        want = rpn_glue.rpn_proposals(maps, [o[g] for o in obj], [r[g] for r in reg], gen.cell_anchors, STRIDES, 20.0, 300,
                                      60, 0.5, (0.3, 0.3), batch_size=nb)
        for (gb, gs), (wb, ws) in zip(got[g], want):
            assert torch.equal(gb, wb) and torch.equal(gs, ws) and 0 < len(gb) <= 60
    now = rpn_glue.rpn_proposals_grouped(maps, obj, reg, G, gen.cell_anchors, STRIDES, 20.0, 300, 60, 0.5, (0.3, 0.3),
                                         batch_size=nb)
    assert all(torch.equal(a[0], b[0]) for g in range(G) for a, b in zip(now[g], got[g]))


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("G", [2, 3])
def test_rpn_module_with_groups_equals_the_explicit_sequence_and_feeds_the_box_head(G):
    import roi_glue
    import rpn_glue
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.box_head import build_roi_box_head
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import build_rpn
    nb = 2
    maps, _gen, gts, labels = _inputs(nb)
    targets = [_Target(g, l) for g, l in zip(gts, labels)]
    names, ids = GROUPS[G]
    cfg = rpn_glue.rpn_cfg(C=32, strides=STRIDES, voxel_scale=20.0, pre_nms_top_n=(300, 200), post_nms_top_n=(60, 40),
                           separate=names, separate_ids=ids, classes=CLASSES, batch_size_per_image=B)
    torch.manual_seed(5)
    mod = build_rpn(cfg).to(DEV)
    with torch.no_grad():
        for q in mod.parameters():
            q.normal_(std=0.3)
    mod.seed = 77
    h, gen, sc = mod.head, mod.anchor_generator, mod.seperate_classifier
    assert sc.group_num == G and sc.flag == "RPN" and h.seperate_rpn == G
    A = gen.num_anchors_per_location()

    def explicit(train):
        obj, reg = rpn_glue.rpn_head_grouped(maps, h.conv.weight, h.conv.bias, h.cls_logits.weight, h.cls_logits.bias,
                                             h.bbox_pred.weight, h.bbox_pred.bias, G)
        assert all(o.shape == (G, m.features.shape[0] * A) and r.shape == (G, m.features.shape[0] * A, 7)
                   for o, r, m in zip(obj, reg, maps))
        pre, post = (300, 60) if train else (200, 40)
        with torch.no_grad():
            props = rpn_glue.rpn_proposals_grouped(maps, [o.detach() for o in obj], [r.detach() for r in reg], G,
                                                   gen.cell_anchors, STRIDES, 20.0, pre, post, 0.5, (0.3, 0.3), batch_size=nb)
        if not train:
            return props, None, None
        boxes, _local, _rows, _counts = rpn_glue.rpn_group_targets(gts, labels, sc)
        flat = [boxes[b][g] for b in range(nb) for g in range(G)]
        lab = rpn_glue.rpn_label_matches_grouped(maps, gen.cell_anchors, STRIDES, 20.0, flat, G, AUG, 6, 0.55, 0.2,
                                                 batch_size=nb, yaw_threshold=0.7)
        return props, rpn_glue.rpn_loss_grouped(maps, obj, reg, lab, gen.cell_anchors, G, B, 0.5, "Diff", seed=77), boxes

    mod.train()
    boxes, losses = mod(None, maps, targets)
    props, (lo, lb), gt_g = explicit(True)
    assert set(losses) == {"loss_%s_%d" % (k, g) for k in ("objectness", "rpn_box_reg") for g in range(G)}
    for g in range(G):
        assert torch.equal(losses["loss_objectness_%d" % g], lo[g]) and torch.equal(losses["loss_rpn_box_reg_%d" % g], lb[g])
        assert losses["loss_objectness_%d" % g].dim() == 0
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(lb).all())
    assert len(boxes) == G and all(len(s) == nb for s in boxes)
    for g in range(G):
        for b, (pb, ps) in zip(boxes[g], props[g]):
            assert torch.equal(b.bbox3d, pb) and torch.equal(b.get_field("objectness"), ps) and 0 < len(b) <= 60
    sum(losses.values()).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in mod.parameters())
    assert float(h.conv.weight.grad.abs().max()) > 0
    assert bool((h.cls_logits.weight.grad.view(A, G, -1).abs().amax((0, 2)) > 0).all())      # every group's branch

    mod.add_gt_proposals = True                                                  # a group's own ground truth behind
    with_gt, _ = mod(None, maps, targets)
    for g in range(G):
        for bi, (b, (pb, ps)) in enumerate(zip(with_gt[g], props[g])):
            gt = gt_g[bi][g]
            assert torch.equal(b.bbox3d, torch.cat([pb, gt])) and len(b) == len(pb) + len(gt)
            assert torch.equal(b.get_field("objectness"), torch.cat([ps, torch.ones(len(gt), device=DEV)]))
    mod.add_gt_proposals = False

    mod.rpn_only = True                                                          # RPN__ONLY in training: no decode
    none, only = mod(None, maps, targets)
    assert none is None and all(torch.equal(only["loss_objectness_%d" % g], lo[g]) for g in range(G))
    mod.rpn_only = False

    mod.eval()
    ev, no_loss = mod(None, maps)
    props_e, _, _ = explicit(False)
    assert no_loss == {}
    for g in range(G):
        for b, (pb, ps) in zip(ev[g], props_e[g]):
            assert torch.equal(b.bbox3d, pb) and torch.equal(b.get_field("objectness"), ps) and 0 < len(b) <= 40
    mod.rpn_only = True                                                          # RPN-only evaluation: sorted by confidence
    srt, _ = mod(None, maps)
    for scenes in srt:
        for b in scenes:
            s = b.get_field("objectness")
            assert bool((s[:-1] >= s[1:]).all())
    mod.rpn_only = False
    with pytest.raises(ValueError, match="labels"):                              # plain tensors cannot be split by group
        mod.train()
        mod(None, maps, gts)

    # into the box head's grouped path
    cat = sc.cat_boxlist_3d_seperated(with_gt)
    assert [c.sep_counts for c in cat] == [[len(with_gt[g][b]) for g in range(G)] for b in range(nb)]
    hcfg = roi_glue.box_head_cfg(C=32, resolution=(2, 3, 2), R=12, classes=CLASSES, class_specific=False, separate=names,
                                 separate_ids=ids, scales=(0.25, 0.125), voxel_scale=20.0, detections=20)
    torch.manual_seed(6)
    head = build_roi_box_head(hcfg).to(DEV)
    head.loss_evaluator.fg_bg_sampler.seed = 9
    head.train()
    _x, sampled, hl = head(maps, cat, targets)
    assert set(hl) == {"loss_%s_roi_%d" % (k, g) for k in ("classifier", "box_reg") for g in range(G)}
    assert all(bool(torch.isfinite(v)) for v in hl.values())
    assert all(q.sep_counts is not None for q in sampled)
