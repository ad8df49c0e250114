"""The multi-level ROI pooler on the device (csrc/roi_pool.hip, roi_glue.pool_rois, modeling/poolers_3d.py).

Inputs: the cases of tests/roi_pool_ref.py -- three feature levels built independently with scn.InputLayer (extents
24x20x6, 12x10x3, 6x5x2, occupancy about 1/6, two scenes) under scales (0.5, 0.25, 0.125) over a 48x40x12 box frame,
canonical size 10.  Yardsticks: tests/roi_pool_ref.py for the ROI rows and levels (pinned by the reference's golden in
test_roi_pool_host.py), aabr_roi_align_rotated_3d_sparse_forward run per level for bit identity, tests/roi_align_ref.py
(fp64 with a derived slack) for the values; test_roi_pool_host.py shows that nothing in these cases is undecided beyond
the 1 % cap.  Nothing outside the repository is read."""
import math
import os

import numpy as np
import pytest
import torch

import roi_align_ref as R
import roi_pool_ref as P

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = P.gpu_cases()
NL = len(P.SCALES)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Boxes(object):
    mode = "yx_zb"

    def __init__(self, bbox3d):
        self.bbox3d = bbox3d

    def __len__(self):
        return int(self.bbox3d.shape[0])


_BUILT = {}


def _levels(case):
    """per level (SparseConvNetTensor, sites [V, 4] int32 in the device's row order, features [V, C] in that order)"""
    import sparseconvnet as scn
    if case.name not in _BUILT:
        out = []
        for (h, w, z), sites, feats in zip(P.EXTENTS, case.sites, case.feats):
            x = scn.InputLayer(3, [h + 3, w + 2, z + 1], mode=4)([_t(sites.astype(np.int64)), _t(feats)])
            key = tuple(int(v) for v in x.spatial_size.tolist())
            dev_sites = x.metadata.grids[key].coords.cpu().numpy().astype(np.int32)
            dev_feats = x.features.detach().cpu().numpy()
            o0, o1 = np.lexsort(sites.T[::-1]), np.lexsort(dev_sites.T[::-1])     # the layer only renumbers rows
            assert (sites[o0] == dev_sites[o1]).all() and (feats[o0] == dev_feats[o1]).all()
            out.append((x, dev_sites, dev_feats))
        _BUILT[case.name] = out
    return _BUILT[case.name]


def _at_sites(a, sites):
    if a.ndim == 5:
        return a[sites[:, 3], :, sites[:, 0], sites[:, 1], sites[:, 2]]
    return a[sites[:, 3], sites[:, 0], sites[:, 1], sites[:, 2]]


class _SiteResult(object):
    """a backward Result restricted to the active sites (what the sparse forms return)"""

    def __init__(self, ref, sites):
        self.values, self.slack = _at_sites(ref.values, sites), _at_sites(ref.slack, sites)
        self.undecided = np.broadcast_to(_at_sites(ref.undecided, sites)[:, None], self.values.shape)


def _check(name, what, got, ref):
    worst, und, bad = R.compare(got, ref)
    print("%s %s: max |device - fp64| / slack = %.4g (undecided share %.5f)" % (name, what, worst, und))
    assert bad == 0, (name, what, worst)
    return worst


def _same_bits(a, b):
    """equal bit patterns wherever neither is NaN, NaN in the same places"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a.view(np.int32)[~nan] == b.view(np.int32)[~nan]).all()


def _prepare(scenes, box_scale, scales, cs):
    import roi_glue
    rois, levels = roi_glue.roi_rows_and_levels([_t(np.asarray(s, F).reshape(-1, 7)) for s in scenes], scales, cs, box_scale)
    assert rois.dtype == torch.float32 and levels.dtype == torch.int32
    return rois.cpu().numpy(), levels.cpu().numpy()


def _cabi(case, level_v=None, levels_override=None):
    """the three entry points' inputs on the device: (table, keep-alive list, rois_d, levels_d, per-level pieces)"""
    import _hip
    from _hip import ptr, stream, check
    lib = _hip.load()
    lv = _levels(case)
    tab = (_hip.AabrRoiLevel * NL)()
    keep, off, pieces = [], 0, []
    for l, ((h, w, z), (x, sites, feats)) in enumerate(zip(P.EXTENTS, lv)):
        V = len(sites) if level_v is None or level_v[l] is None else level_v[l]
        sites_d, feats_d = _t(sites), _t(feats)
        cm = torch.empty((P.BATCH, h, w, z), dtype=torch.int32, device=DEV)
        check(lib.aabr_roi_cellmap(ptr(sites_d), len(sites), _hip.i32x3((h, w, z)), P.BATCH, ptr(cm), stream()))
        t = tab[l]
        t.feats, t.cellmap = (ptr(feats_d), ptr(cm)) if V else (None, None)
        t.height, t.width, t.zsize, t.nb = h, w, z, P.BATCH
        t.V, t.row_offset, t.spatial_scale = V, off, P.SCALES[l]
        keep += [sites_d, feats_d, cm]
        pieces.append((feats_d, cm, off, V, sites))
        off += V
    levels = case.levels if levels_override is None else levels_override
    return tab, keep, _t(case.rois), _t(np.asarray(levels, np.int32)), pieces, off


# ------------------------------------------------------------------------------------------------ 1. prepare
def test_prepare_matches_the_restatement_on_the_golden_and_random_inputs():
    from maskrcnn_benchmark.modeling.poolers_3d import LevelMapper_3d
    g = np.load(os.path.join(REPO, "tests", "golden", "pooler_golden.npz"))
    sets = []
    for k in "abc":
        counts = g[k + "_counts"]
        scenes = np.split(g[k + "_boxes"], np.cumsum(counts)[:-1])
        sets.append((k, scenes, float(g[k + "_box_scale"]), tuple(g[k + "_scales"].tolist()), float(g[k + "_canonical_size"]),
                     g[k + "_rois"], g[k + "_levels"]))
    for c in CASES:
        sets.append((c.name, c.boxes, 1.0, P.SCALES, P.CANONICAL, c.rois, c.levels))
    # hand-placed rows: the exact tie, a NaN size, a negative size, yaws at +-pi/2 (+pi/2 does not survive the reference's
    # yx_zb constructor, so the golden has none) and 0, an empty scene first and last
    h = F(math.pi / 2)
    edge = np.array([[1, 2, 3, 9.0, 4.0, 2, h], [1, 2, 3, 2.0, 9.0, 2, -h], [1, 2, 3, np.nan, 3.0, 2, 0.0],
                     [1, 2, 3, 3.0, np.nan, 2, 0.3], [1, 2, 3, -4.0, -1.0, 2, -0.3], [5, 6, 1, 30.0, 2.0, 4, 2 * h],
                     [5, 6, 1, 1.0, 1.5, 4, -2 * h], [5, 6, 1, 36.0, 36.0, 4, np.nextafter(h, F(0))]], F)
    empty = np.zeros((0, 7), F)
    er, el = P.rois_and_levels([empty, edge, empty], 1.0, (0.5, 0.25), 8)
    assert el[:5].tolist() == [0, 0, 0, 0, 0] and set(el.tolist()) == {0, 1} and (er[:, 0] == 1).all()
    assert er[0, 7] == 0.0 and er[1, 7] == 0.0 and er[2, 7] == 90.0
    sets.append(("edge", [empty, edge, empty], 1.0, (0.5, 0.25), 8, er, el))
    for name, scenes, box_scale, scales, cs, rois, levels in sets:
        got_rois, got_levels = _prepare(scenes, box_scale, scales, cs)
        assert (got_levels == levels).all(), (name, np.nonzero(got_levels != levels)[0][:10])
        assert _same_bits(got_rois, rois), (name, np.argwhere(got_rois != rois)[:10])
        if box_scale == 1.0:
            lm = LevelMapper_3d(scales, cs)([_Boxes(_t(np.asarray(s, F).reshape(-1, 7))) for s in scenes])
            assert lm.dtype == torch.int64 and (lm.cpu().numpy() == levels).all(), name


# ------------------------------------------------------------------------------------------------ 2, 3. C entry points
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_c_entry_points_forward_and_backward(case):
    import _hip
    from _hip import ptr, stream, check
    lib = _hip.load()
    tab, keep, rois_d, levels_d, pieces, total = _cabi(case)
    n, C = case.n, case.C
    PH, PW, PZ = case.out_size
    grad = case.grad()
    grad_d = _t(grad)
    out = torch.full((n, C, PH, PW, PZ), 7.0, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_pool_forward(tab, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), n, PH, PW, PZ, case.sampling,
                                    ptr(out), stream()))
    d_all = torch.full((total, C), 7.0, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_pool_backward(tab, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), n, PH, PW, PZ, case.sampling,
                                     ptr(grad_d), ptr(d_all), total, stream()))
    single = []
    for l, (idx, _, _) in enumerate(case.reference()):
        feats_d, cm, off, V, sites = pieces[l]
        h, w, z = P.EXTENTS[l]
        sub = _t(case.rois[idx])
        o = torch.full((len(idx), C, PH, PW, PZ), 7.0, dtype=torch.float32, device=DEV)
        check(lib.aabr_roi_align_rotated_3d_sparse_forward(ptr(feats_d), C, ptr(cm), P.BATCH, h, w, z, ptr(sub), len(idx),
                                                           float(P.SCALES[l]), PH, PW, PZ, case.sampling, ptr(o), stream()))
        single.append(o)
    torch.cuda.synchronize()
    out, d_all = out.cpu().numpy(), d_all.cpu().numpy()
    assert (out != 7.0).all() or n == 0                                # every output element is written
    for l, (idx, rf, rb) in enumerate(case.reference()):
        _, _, off, V, sites = pieces[l]
        # forward: the single-level kernel's bits on the level's subset, and within the fp64 slack
        assert out[idx].tobytes() == single[l].cpu().numpy().tobytes(), (case.name, l)
        _check(case.name, "level %d forward" % l, out[idx], rf)
        sl = d_all[off:off + V]
        if len(idx) == 0:
            assert not sl.any(), (case.name, l)                        # a level without ROIs: exactly zero
        _check(case.name, "level %d backward" % l, sl, _SiteResult(rb, sites))


def test_level_without_sites_and_level_outside_the_table_give_zeros():
    import _hip
    from _hip import ptr, stream, check
    lib = _hip.load()
    case = CASES[0]
    lv = case.levels.copy()
    outside = np.array([0, 5, 11])
    lv[outside[0]], lv[outside[1]], lv[outside[2]] = NL, -1, 100
    tab, keep, rois_d, levels_d, pieces, total = _cabi(case, level_v=[None, 0, None], levels_override=lv)
    n, C = case.n, case.C
    PH, PW, PZ = case.out_size
    out = torch.full((n, C, PH, PW, PZ), 7.0, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_pool_forward(tab, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), n, PH, PW, PZ, case.sampling,
                                    ptr(out), stream()))
    d_all = torch.full((total, C), 7.0, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_pool_backward(tab, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), n, PH, PW, PZ, case.sampling,
                                     ptr(_t(case.grad())), ptr(d_all), total, stream()))
    torch.cuda.synchronize()
    out, d_all = out.cpu().numpy(), d_all.cpu().numpy()
    zero = (lv == 1) | (lv < 0) | (lv >= NL)
    assert zero.sum() > 3 and not out[zero].any() and (out[~zero] != 7.0).all()
    # the other ROIs are what they were; the gradient rows receive those ROIs only
    ref_rows = np.nonzero(~zero)[0]
    for l, (idx, rf, rb) in enumerate(case.reference()):
        if l == 1:
            continue
        same = np.intersect1d(idx, ref_rows)
        _check(case.name, "level %d forward, others zeroed" % l, out[same], _Rows(rf, np.searchsorted(idx, same)))
    assert np.isfinite(d_all).all() and (d_all != 7.0).all()


class _Rows(object):
    """a forward Result restricted to some of its ROIs"""

    def __init__(self, ref, rows):
        self.values, self.slack, self.undecided = ref.values[rows], ref.slack[rows], ref.undecided[rows]


# ------------------------------------------------------------------------------------------------ 4. adjoint identity
def test_adjoint_identity_on_device_outputs():
    """<pool(f), g> = sum_l <f_l, pool^T(g)_l> with both sides from the device, accumulated on the host in fp64, within
    the sum of the two slacks (the bound of test_gpu_roi_align.py::test_adjoint_identity_on_device_outputs).  No sample
    lies above a map and nothing is undecided (test_roi_pool_host.py checks both for this case)."""
    import roi_glue
    import sparseconvnet as scn
    case = P.adjoint_case()
    lv = _levels(case)
    fs = [_t(feats).requires_grad_(True) for _, _, feats in lv]
    xs = [scn.SparseConvNetTensor(f, x.metadata, x.spatial_size) for f, (x, _, _) in zip(fs, lv)]
    out = roi_glue.pool_rois(xs, [_t(b) for b in case.boxes], case.out_size, P.SCALES, case.sampling, P.CANONICAL)
    grad = case.grad()
    out.backward(_t(grad))
    torch.cuda.synchronize()
    out = out.detach().cpu().numpy().astype(np.float64)
    g64 = grad.astype(np.float64)
    lhs, rhs, bound = (g64 * out).sum(), 0.0, 0.0
    for l, (idx, rf, rb) in enumerate(case.reference()):
        assert not rf.undecided.any() and not (rb.undecided & rb.touched).any()
        sites, feats = lv[l][1], lv[l][2].astype(np.float64)
        rhs += (fs[l].grad.cpu().numpy().astype(np.float64) * feats).sum()
        bound += (np.abs(g64[idx]) * rf.slack).sum() + (_at_sites(rb.slack, sites) * np.abs(feats)).sum()
    print("adjoint: |diff| / bound %.4g" % (abs(lhs - rhs) / bound))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ------------------------------------------------------------------------------------------------ 5. module
def _module_inputs(case):
    import sparseconvnet as scn
    lv = _levels(case)
    fs = [_t(feats).requires_grad_(True) for _, _, feats in lv]
    xs = [scn.SparseConvNetTensor(f, x.metadata, x.spatial_size) for f, (x, _, _) in zip(fs, lv)]
    return lv, fs, xs, [_Boxes(_t(b)) for b in case.boxes]


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]], ids=[CASES[i].name for i in (1, 3, 4)])
def test_module_fused_equals_the_loop_and_autograd_reaches_every_level(case):
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    lv, fs, xs, boxes = _module_inputs(case)
    pooler = Pooler(case.out_size, P.SCALES, case.sampling, P.CANONICAL, canonical_level=None)
    assert pooler.fused
    fused = pooler(xs, boxes)
    assert tuple(fused.shape) == (case.n, case.C) + case.out_size
    pooler.fused = False
    loop = pooler(xs, boxes)
    assert torch.equal(fused, loop)
    fused.backward(_t(case.grad()))
    torch.cuda.synchronize()
    for l, (idx, rf, rb) in enumerate(case.reference()):
        assert fs[l].grad is not None and fs[l].grad.shape == fs[l].shape, l
        got = fs[l].grad.cpu().numpy()
        if len(idx) == 0:
            assert not got.any()
        _check(case.name, "module level %d backward" % l, got, _SiteResult(rb, lv[l][1]))
        _check(case.name, "module level %d forward" % l, fused.detach().cpu().numpy()[idx], rf)


def test_module_one_level_and_box_scale():
    from maskrcnn_benchmark.layers.roi_align_rotated_3d import ROIAlignRotated3D
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    import roi_glue
    case = CASES[0]
    lv, fs, xs, boxes = _module_inputs(case)
    one = Pooler(case.out_size, P.SCALES[:1], case.sampling, P.CANONICAL)
    got = one(xs[:1], boxes)
    want = ROIAlignRotated3D(case.out_size, P.SCALES[0], case.sampling)(xs[0], _t(case.rois))
    assert torch.equal(got, want)
    one.fused = False
    assert torch.equal(one(xs[:1], boxes), want)
    # box_scale: metric boxes (divided by 50 in fp32) times 50 in the launch -- the ROI rows of the restatement
    metric = [(b / F(50)).astype(F) for b in case.boxes]
    rois50, levels50 = P.rois_and_levels(metric, 50.0, P.SCALES, P.CANONICAL)
    scaled = Pooler(case.out_size, P.SCALES, case.sampling, P.CANONICAL, box_scale=50.0)
    rows = scaled.convert_to_roi_format([_Boxes(_t(m)) for m in metric])
    assert _same_bits(rows.cpu().numpy(), rois50)
    dbg = {}
    out = roi_glue.pool_rois(xs, [_t(m) for m in metric], case.out_size, P.SCALES, case.sampling, P.CANONICAL, 50.0, dbg)
    assert _same_bits(dbg["rois"].cpu().numpy(), rois50) and (dbg["levels"].cpu().numpy() == levels50).all()
    assert torch.equal(out, scaled(xs, [_Boxes(_t(m)) for m in metric]))


# ------------------------------------------------------------------------------------------------ 6, 7 and N = 0
def test_forward_determinism_no_rois_and_no_host_sync():
    import roi_glue
    case = CASES[1]
    lv, fs, xs, boxes = _module_inputs(case)
    props = [b.bbox3d for b in boxes]
    grad_d = _t(case.grad())

    def run():
        for f in fs:
            f.grad = None
        out = roi_glue.pool_rois(xs, props, case.out_size, P.SCALES, case.sampling, P.CANONICAL)
        out.backward(grad_d)
        return out.detach().clone()
    a = run()                                                          # also fills the extent and cell-map caches
    b = run()
    assert torch.equal(a, b)
    # N = 0: an empty result, zero gradients of each level's own shape
    for f in fs:
        f.grad = None
    none = [torch.zeros((0, 7), device=DEV), torch.zeros((0, 7), device=DEV)]
    e = roi_glue.pool_rois(xs, none, case.out_size, P.SCALES, case.sampling, P.CANONICAL)
    assert tuple(e.shape) == (0, case.C) + case.out_size
    e.sum().backward()
    assert all(f.grad.shape == f.shape and not f.grad.any() for f in fs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        c = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, c)
