"""The shared anchor list (csrc/anchor_list.h) where one locate for every RPN stage can go wrong, on the smallest layout
that reaches those places: three maps, three examples, A = 3; map 1 has no sites for example 1, example 2 has no sites
in any map.  Every stage is compared with the same work done on MATERIALISED anchors (rpn_glue.grid_anchors, the
examples' lists concatenated in map order) and on concatenated head outputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, NB, VS = 3, 3, 20.0
# per map: spatial size, points per example (before the input layer merges duplicates), stride
MAPS = (((24, 24, 6), (30, 26), (4.0, 4.0, 4.0)), ((12, 12, 4), (28, 0), (8.0, 8.0, 8.0)), ((8, 8, 2), (12, 20), (16.0, 16.0, 16.0)))
WEIGHTS = (1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5)
LABEL_AUG = {"target_Y": 0.4, "anchor_Y": 0.0, "target_Z": 0.8, "anchor_Z": 0.0}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Layout(object):
    pass


@pytest.fixture(scope="module")
def lay():
    import sparseconvnet as scn
    import rpn_glue
    rng = np.random.default_rng(11)
    L = _Layout()
    L.maps, L.bases, L.strides, L.counts, anchors = [], [], [], [], []
    for mi, (sp, pts, st) in enumerate(MAPS):
        b = np.concatenate([np.full(n, e, np.int64) for e, n in enumerate(pts)])
        n = b.size
        coords = np.stack([rng.integers(0, sp[0], n), rng.integers(0, sp[1], n), rng.integers(0, sp[2], n), b], 1)
        x = scn.InputLayer(3, list(sp), mode=3)([_t(coords), _t(np.zeros((n, 1), np.float32))])
        sc = x.get_spatial_locations()
        assert (np.diff(sc[:, 3].numpy()) >= 0).all()                      # batch-contiguous rows
        base = torch.zeros((A, 7), dtype=torch.float32)
        base[:, 3:6] = torch.tensor([0.3 * (mi + 1), 1.4 * (mi + 1), 2.5])
        base[:, 6] = torch.tensor([0.0, -1.57, 0.785])
        L.maps.append(x)
        L.bases.append(base)
        L.strides.append(st)
        L.counts.append([int((sc[:, 3] == e).sum()) for e in range(NB)])
        anchors.append(rpn_glue.grid_anchors(sc, base, VS, st))             # on the host: [V_m * A, 7], rows [site, yaw]
    assert L.counts[1][1] == 0 and all(c[2] == 0 for c in L.counts) and min(L.counts[m][0] for m in range(3)) > 0
    L.seg, L.site, L.n_anchor = rpn_glue._anchor_tables(L.counts, A)
    total = sum(L.n_anchor)
    # every anchor a distinct logit: torch.topk has one answer.  The first and the last anchor of every non-empty
    # segment hold their example's largest logits, so a top-k of exactly that many must pick the segments' ends
    L.ends = [sorted({j for m in range(3) if L.seg[4 * e + m + 1] > L.seg[4 * e + m]
                      for j in (L.seg[4 * e + m], L.seg[4 * e + m + 1] - 1)}) for e in range(NB)]
    by_example = []
    for e in range(NB):
        rank = rng.permutation(L.n_anchor[e])
        rest = np.setdiff1d(np.arange(L.n_anchor[e]), L.ends[e])
        order = np.concatenate([rng.permutation(rest), rng.permutation(L.ends[e])]).astype(np.int64)   # ascending logit
        rank[order] = np.arange(L.n_anchor[e])
        by_example.append((torch.as_tensor(rank).float() - L.n_anchor[e] / 2) * 0.03125)
    # example-major lists -> the maps' [site, yaw] rows
    per_map = [[by_example[e][L.seg[4 * e + m]:L.seg[4 * e + m + 1]] for e in range(NB)] for m in range(3)]
    logit = torch.cat([v for m in range(3) for v in per_map[m]])
    L.obj, L.reg, o = [], [], 0
    for m in range(3):
        n = sum(L.counts[m]) * A
        L.obj.append(logit[o:o + n].to(DEV))
        L.reg.append(_t((rng.standard_normal((n, 7)) * 0.3).astype(np.float32)))
        o += n

    def cat(per_map, e):
        """example e's slice of a per-map [V_m * A, ...] list, concatenated in map order"""
        rows = [(sum(L.counts[m][:e]) * A, sum(L.counts[m][:e + 1]) * A) for m in range(3)]
        return torch.cat([per_map[m][lo:hi] for m, (lo, hi) in enumerate(rows)])
    L.anchors = [cat(anchors, e).to(DEV) for e in range(NB)]
    L.logits = [cat(L.obj, e) for e in range(NB)]
    L.regs = [cat(L.reg, e) for e in range(NB)]
    assert [a.shape[0] for a in L.anchors] == L.n_anchor and L.n_anchor[2] == 0
    return L


def _topk(L, ks):
    import _hip
    lib = _hip.load()
    kmax = max(max(ks), 1)
    sel = torch.full((NB, kmax), -7, dtype=torch.int64, device=DEV)
    info = torch.empty((NB, 2), dtype=torch.int32, device=DEV)
    scr = torch.empty(int(lib.aabr_rpn_topk_scratch_words(NB)) + 2, dtype=torch.int32, device=DEV)
    off = (-scr.data_ptr() // 4) % 2
    _hip.check(lib.aabr_rpn_topk_maps(3, _hip.ptrs(L.obj), NB, _hip.i32xn(L.seg), _hip.i32xn(L.site), A, _hip.i32xn(ks),
                                      _hip.ptr(sel), kmax, _hip.ptr(info), scr.data_ptr() + 4 * off, _hip.stream()))
    assert info[:, 1].tolist() == [0] * NB                                  # no overflow, no fallback
    return sel


def test_topk_and_decode_against_materialised_anchors(lay):
    import _hip
    from sparseconvnet import SCN
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    L, lib = lay, _hip.load()
    whole = _topk(L, L.n_anchor)
    first = _topk(L, [min(1, n) for n in L.n_anchor])
    ends = _topk(L, [len(v) for v in L.ends])
    coder = BoxCoder3D(False, WEIGHTS)
    coder.bbox_xform_clip = 0.25                                            # a clip that some encodings reach
    coords_p = _hip.ptrs([x.metadata.grids[SCN._key(x.spatial_size)].coords for x in L.maps])
    obj_p, reg_p = _hip.ptrs(L.obj), _hip.ptrs(L.reg)
    ba = torch.cat(L.bases).to(DEV)
    for e in range(NB):
        n = L.n_anchor[e]
        if n == 0:
            continue
        want = torch.topk(L.logits[e], n, sorted=True).indices
        sel = whole[e, :n]
        assert torch.equal(sel, want)
        assert torch.equal(first[e, :1], want[:1])
        seg = L.seg[e * 4:(e + 1) * 4]
        assert len(L.ends[e]) >= 4 and sorted(ends[e, :len(L.ends[e])].tolist()) == L.ends[e]   # a cut right behind the ends
        boxes = torch.empty((n, 7), dtype=torch.float32, device=DEV)
        nms_boxes = torch.empty((n, 7), dtype=torch.float32, device=DEV)
        scores = torch.empty(n, dtype=torch.float32, device=DEV)
        _hip.check(lib.aabr_rpn_decode_maps(3, coords_p, obj_p, reg_p, _hip.i32xn(seg), _hip.i32xn(L.site[e * 3:(e + 1) * 3]),
                                            _hip.f32xn([v for st in L.strides for v in st]), _hip.ptr(ba), A, VS,
                                            _hip.f32xn(WEIGHTS), coder.bbox_xform_clip, 0.3, 0.3, _hip.ptr(sel), n,
                                            _hip.ptr(boxes), _hip.ptr(nms_boxes), _hip.ptr(scores), _hip.stream()))
        assert (L.regs[e][sel][:, 3:6] / torch.tensor(WEIGHTS[3:6], device=DEV) > coder.bbox_xform_clip).any()
        assert torch.equal(boxes, coder.decode(L.regs[e][sel], L.anchors[e][sel]))     # one function on both sides
        clamped = boxes.clone()
        clamped[:, 3:6] = clamped[:, 3:6].clamp(min=0.3)
        assert torch.equal(nms_boxes, clamped)
        x = L.logits[e][sel]
        own = 1.0 / (1.0 + torch.exp(-x))                                   # the kernel's expression, fp32 on the device
        ulps = (scores.view(torch.int32) - torch.sigmoid(x).view(torch.int32)).abs().max().item()
        print("example %d: scores == 1 / (1 + exp(-x)): %s, ulps from torch.sigmoid: %d" % (e, torch.equal(scores, own), ulps))
        assert torch.equal(scores, own)
        assert ulps <= 1


def test_padded_logits(lay):
    import _hip
    L, lib = lay, _hip.load()
    lmax = max(L.n_anchor) + 5
    out = torch.zeros((NB, lmax), dtype=torch.float32, device=DEV)
    _hip.check(lib.aabr_rpn_gather_logits(3, _hip.ptrs(L.obj), NB, _hip.i32xn(L.seg), _hip.i32xn(L.site), A, lmax,
                                          _hip.ptr(out), _hip.stream()))
    for e in range(NB):
        assert torch.equal(out[e, :L.n_anchor[e]], L.logits[e])
        assert (out[e, L.n_anchor[e]:] == float("-inf")).all()


@pytest.fixture(scope="module")
def labels(lay):
    """ground truth near some of example 0's anchors; example 1 without ground truth; example 2 without sites"""
    import rpn_glue
    a0 = lay.anchors[0]
    pick = torch.arange(0, a0.shape[0], 17, device=DEV)
    gt = a0[pick].clone()
    gt[:, 0:3] += 0.05
    gt[:, 3:6] *= 1.1
    targets = [gt, torch.zeros((0, 7), device=DEV), gt[:2].clone()]
    return targets, rpn_glue.rpn_label_matches(lay.maps, lay.bases, lay.strides, VS, targets, LABEL_AUG, 6,
                                               regression_targets=True, weights=WEIGHTS)


def test_regression_targets_against_materialised_anchors(lay, labels):
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    targets, lab = labels
    coder = BoxCoder3D(False, WEIGHTS)
    assert len(lab) == NB
    for e in range(NB):
        midx, mval, mat, regt = lab[e]
        n = lay.n_anchor[e]
        assert midx.shape == (n,) and mval.shape == (n,) and regt.shape == (n, 7) and mat is None
    assert (lab[0][0] >= 0).any() and (lab[0][0] < 0).any()                 # matched and unmatched anchors
    assert torch.equal(lab[0][3], coder.encode(targets[0][lab[0][0].clamp(min=0)], lay.anchors[0]))
    assert (lab[1][0] == -1).all()                                          # no ground truth: all negatives, and the
    assert torch.equal(lab[1][3], coder.encode(lay.anchors[1], lay.anchors[1]))   # anchors encoded against themselves


def test_loss_over_the_anchor_list(lay, labels, monkeypatch):
    import rpn_glue
    import test_gpu_rpn_loss as T
    monkeypatch.setattr(T, "A", A)                                          # its reference slices the maps by its own A
    _, lab = labels
    obj = [o.clone().requires_grad_() for o in lay.obj]
    reg = [r.clone().requires_grad_() for r in lay.reg]
    B = 16
    lo, lb, sel = rpn_glue.rpn_loss(lay.maps, obj, reg, lab, lay.bases, batch_size_per_image=B, seed=3, return_samples=True)
    (lo + lb).backward()
    assert sel.shape == (NB, B)
    begin, samples, sampled = 0, [], []
    for e in range(NB):
        row = sel[e][sel[e] >= 0].cpu().numpy()
        assert ((row >= begin) & (row < begin + lay.n_anchor[e])).all()     # inside this example's list
        local = row - begin
        cls = lab[e][0].cpu().numpy()[local]
        pos, neg = local[cls >= 0], local[cls == -1]
        assert len(pos) + len(neg) == len(local) == len(set(local.tolist()))
        assert np.array_equal(local, np.concatenate([pos, neg]))            # positives, then negatives
        samples.append((pos, neg))
        sampled.append(row)
        begin += lay.n_anchor[e]
    assert len(samples[0][0]) > 0 and len(samples[1][1]) == B and len(sampled[2]) == 0
    ro, rbx, go, gr = T._reference(obj, reg, lab, lay.counts, samples)
    np.testing.assert_allclose(lo.item(), ro, rtol=1e-5)
    np.testing.assert_allclose(lb.item(), rbx, rtol=1e-5)
    # gradients: the reference's inside the sample, exactly zero outside it
    hit = torch.zeros(sum(lay.n_anchor), dtype=torch.bool)
    hit[torch.as_tensor(np.concatenate(sampled))] = True
    o = 0
    inside = [torch.zeros(sum(c) * A, dtype=torch.bool) for c in lay.counts]
    for e in range(NB):
        for m in range(3):
            lo_, n = sum(lay.counts[m][:e]) * A, lay.counts[m][e] * A
            inside[m][lo_:lo_ + n] = hit[o:o + n]
            o += n
    for m in range(3):
        g_o, g_r = obj[m].grad.cpu(), reg[m].grad.cpu()
        assert (g_o[~inside[m]] == 0).all() and (g_r[~inside[m]] == 0).all()
        assert (g_o[inside[m]] != 0).all()
        np.testing.assert_allclose(g_o.numpy(), go[m], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(g_r.numpy(), gr[m], rtol=1e-5, atol=1e-9)
