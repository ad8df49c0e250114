"""bf16 feature storage into the heads on the device: the RPN head (csrc/rpn_head.hip), the multi-level ROI pooler
(csrc/roi_pool.hip), the single-level sparse ROI-align (csrc/roi.hip), their glue and modules, and FPN_Net.cast_outputs.

Widening bf16 to fp32 is exact and all three kernels compute in fp32, so every input here is bf16-representable
(`x.to(torch.bfloat16)` on the existing helpers' arrays) and the yardstick is the fp32 entry point on `x16.float()`:
byte equality for everything that stays fp32, `fp32_result.to(torch.bfloat16)` byte for byte for the one rounded
output.  The ROI backward sums with fp32 atomics, so its fp32 accumulation buffer is held to the fp64 slack of
tests/roi_align_ref.py exactly as tests/test_gpu_roi_pool.py holds the fp32 path, and the bf16 rows to the rounding of
that buffer.  No tolerance of this file's own."""
import numpy as np
import pytest
import torch

import roi_pool_ref as P
import rpn_head_grouped_ref as RG
import rpn_head_ref as R
import synth_scenes as S
import test_gpu_roi_pool as TP
import test_gpu_rpn_head as TR

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
NAN = float("nan")
B16 = torch.bfloat16
NL = len(P.SCALES)
NAMES = ("conv_w", "conv_b", "cls_w", "cls_b", "reg_w", "reg_b")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lib():
    import _hip
    return _hip.load()


def _bits(ts):
    return b"".join(t.detach().cpu().reshape(-1).clone().view(torch.uint8).numpy().tobytes() for t in ts if t.numel())


# ------------------------------------------------------------------------------------------------ 1. RPN head, C ABI
class _Head(object):
    """one case through both storages of the C ABI (G None: plain, else grouped); every output is pre-filled with NaN"""

    def __init__(self, C, A, rows, seed, G=None):
        self.C, self.A, self.G, self.rows = C, A, G, list(rows)
        self.AG = A * (G or 1)
        p, f, g_obj, g_reg = R.make_case(C, self.AG, rows, seed)
        self.pd = {k: _t(v) for k, v in p.items()}
        self.f16 = [_t(x).to(B16) for x in f]
        self.f32 = [x.float() for x in self.f16]                                    # the widened rows: exact
        self.god, self.grd = [_t(g) for g in g_obj], [_t(g) for g in g_reg]         # grouped: read as group-major
        T = _lib().aabr_rpn_head_tile_rows(C)
        self.tiles = sum(-(-n // T) for n in rows)

    def _fn(self, what, bf16):
        return getattr(_lib(), "aabr_rpn_head%s_%s%s" % ("" if self.G is None else "_grouped", what, "_bf16" if bf16 else ""))

    def _table(self, feats, o, r, d=None):
        import _hip
        tab = (_hip.AabrRpnMap * len(self.rows))()
        for m, n in enumerate(self.rows):
            tab[m].features, tab[m].rows = _hip.ptr(feats[m]), n
            tab[m].objectness = _hip.ptr(o[m]) if o is not None else None
            tab[m].box_regression = _hip.ptr(r[m]) if r is not None else None
            tab[m].d_features = _hip.ptr(d[m]) if d is not None else None
        return tab

    def forward(self, bf16):
        from _hip import check, ptr, stream
        C, A, pd = self.C, self.A, self.pd
        lead = () if self.G is None else (self.G,)
        obj = [torch.full((n, self.AG), NAN, device=DEV) for n in self.rows]
        reg = [torch.full((n, 7 * self.AG), NAN, device=DEV) for n in self.rows]
        hidden = torch.full((sum(self.rows), C), NAN, device=DEV)
        check(self._fn("forward", bf16)(self._table(self.f16 if bf16 else self.f32, obj, reg), len(self.rows), C, A, *lead,
                                        *[ptr(pd[k]) for k in NAMES], ptr(hidden), stream()))
        return obj, reg, hidden

    def backward(self, bf16, hidden, null=False, zero=False):
        from _hip import check, ptr, stream
        lib = _lib()
        C, A, pd = self.C, self.A, self.pd
        lead = () if self.G is None else (self.G,)
        d_f = [torch.full((n, C), NAN, device=DEV, dtype=B16 if bf16 else torch.float32) for n in self.rows]
        grads = {k: torch.full(tuple(v.shape), NAN, device=DEV) for k, v in pd.items()}
        floats = (lib.aabr_rpn_head_scratch_floats if self.G is None else lib.aabr_rpn_head_grouped_scratch_floats)(
            self.tiles, C, A, *lead)
        scr = torch.full((max(floats, 1),), NAN, device=DEV)
        go = None if null else [torch.zeros_like(g) for g in self.god] if zero else self.god
        gr = None if null else [torch.zeros_like(g) for g in self.grd] if zero else self.grd
        check(self._fn("backward", bf16)(self._table(self.f16 if bf16 else self.f32, go, gr, d_f), len(self.rows), C, A,
                                         *lead, ptr(pd["conv_w"]), ptr(pd["cls_w"]), ptr(pd["reg_w"]), ptr(hidden),
                                         *[ptr(grads[k]) for k in NAMES], ptr(scr), stream()))
        return d_f, grads

    def check(self):
        """both storages forward and backward; returns the bf16 run's (hidden, d_f, grads)"""
        o32, r32, h32 = self.forward(False)
        o16, r16, h16 = self.forward(True)
        assert _bits(o16) == _bits(o32) and _bits(r16) == _bits(r32) and _bits([h16]) == _bits([h32])
        assert not torch.isnan(torch.cat(o16)).any() and not torch.isnan(h16).any()
        d32, g32 = self.backward(False, h32)
        d16, g16 = self.backward(True, h16)
        for k in NAMES:
            assert _bits([g16[k]]) == _bits([g32[k]]), k
            assert not torch.isnan(g16[k]).any(), k
        assert all(d.dtype == B16 for d in d16)
        assert not torch.isnan(torch.cat(d16).float()).any()                        # every d_f element is written
        assert _bits(d16) == _bits([d.to(B16) for d in d32])                        # ... and rounded once, to nearest even
        return h16, d16, g16


def _entry_shapes(T):
    want = {(32, 2), (32, 4), (128, 2), (128, 4), (96, 2)}
    return [c for c in R.entry_cases(T) if (c[0], c[1]) in want]


def test_rpn_entry_points_equal_the_fp32_ones_on_the_widened_rows():
    T = _lib().aabr_rpn_head_tile_rows(128)
    cases = _entry_shapes(T)
    assert len(cases) == 5 and all(rows == (T + 1, 0, 1) for _, _, rows, _ in cases)
    for C, A, rows, seed in cases:
        _Head(C, A, rows, seed).check()
        _Head(C, A, (7,), seed + 1).check()


def test_rpn_grouped_entry_points_equal_the_fp32_ones_on_the_widened_rows():
    T = _lib().aabr_rpn_head_tile_rows(32)
    (case,) = [c for c in RG.entry_cases(T) if c[:3] == (32, 2, 3)]
    C, A, G, rows, seed = case
    _Head(C, A, rows, seed, G=G).check()
    _Head(C, A, (7,), seed + 1, G=G).check()


def test_rpn_backward_is_deterministic_with_more_tiles_than_workgroups():
    lib = _lib()
    T, gmax = lib.aabr_rpn_head_tile_rows(32), lib.aabr_rpn_head_groups(2 ** 40)
    many = _Head(32, 2, ((gmax + 1) * T + 5,), 5)
    assert many.tiles == gmax + 2 and lib.aabr_rpn_head_groups(many.tiles) == gmax
    one = _Head(32, 2, (7,), 6)
    for run in (many, one):
        hidden, d_f, grads = run.check()
        d_f2, grads2 = run.backward(True, hidden)
        assert _bits(d_f) == _bits(d_f2)
        assert all(_bits([grads[k]]) == _bits([grads2[k]]) for k in NAMES)


def test_rpn_null_gradients_and_empty_maps():
    T = _lib().aabr_rpn_head_tile_rows(32)
    run = _Head(32, 2, (T + 3, 0, 2), 7)
    _, _, hidden = run.forward(True)
    d_n, g_n = run.backward(True, hidden, null=True)
    d_z, g_z = run.backward(True, hidden, zero=True)
    assert _bits(d_n) == _bits(d_z) and not torch.isnan(torch.cat(d_n).float()).any()
    assert all(_bits([g_n[k]]) == _bits([g_z[k]]) for k in NAMES)
    assert not torch.cat(d_n).any() and not any(v.any() for v in g_n.values())     # the bytes of zero gradients
    empty = _Head(64, 4, (0, 0), 8)
    obj, reg, hidden = empty.forward(True)
    assert all(o.numel() == 0 for o in obj + reg)
    _, grads = empty.backward(True, hidden)
    assert all(not v.any() and not torch.isnan(v).any() for v in grads.values())


# ------------------------------------------------------------------------------------------------ 2, 3. ROI kernels, C ABI
def _pool_tables(case, level_v=None, levels_override=None):
    """the level table twice -- bf16 rows and their widened fp32 copy -- over the same cell maps"""
    import _hip
    from _hip import ptr, stream, check
    lib = _hip.load()
    tab16, tab32 = (_hip.AabrRoiLevel * NL)(), (_hip.AabrRoiLevel * NL)()
    keep, off, pieces = [], 0, []
    for l, ((h, w, z), (x, sites, feats)) in enumerate(zip(P.EXTENTS, TP._levels(case))):
        V = len(sites) if level_v is None or level_v[l] is None else level_v[l]
        sites_d, f16 = _t(sites), _t(feats).to(B16)
        f32 = f16.float()
        cm = torch.empty((P.BATCH, h, w, z), dtype=torch.int32, device=DEV)
        check(lib.aabr_roi_cellmap(ptr(sites_d), len(sites), _hip.i32x3((h, w, z)), P.BATCH, ptr(cm), stream()))
        for t, f in ((tab16[l], f16), (tab32[l], f32)):
            t.feats, t.cellmap = (ptr(f), ptr(cm)) if V else (None, None)
            t.height, t.width, t.zsize, t.nb = h, w, z, P.BATCH
            t.V, t.row_offset, t.spatial_scale = V, off, P.SCALES[l]
        keep += [sites_d, f16, f32, cm]
        pieces.append((f16, f32, cm, off, V, sites))
        off += V
    levels = case.levels if levels_override is None else levels_override
    return tab16, tab32, keep, _t(case.rois), _t(np.asarray(levels, np.int32)), pieces, off


POOL_CASES = [TP.CASES[0], TP.CASES[1], TP.CASES[4]]         # [4]: no ROI maps to the middle level


@pytest.mark.parametrize("case", POOL_CASES, ids=[c.name for c in POOL_CASES])
def test_pool_entry_points_forward_and_backward(case):
    from _hip import ptr, stream, check
    lib = _lib()
    tab16, tab32, keep, rois_d, levels_d, pieces, total = _pool_tables(case)
    n, C = case.n, case.C
    PH, PW, PZ = case.out_size
    grad_d = _t(case.grad())
    geom = (n, PH, PW, PZ, case.sampling)
    out16 = torch.full((n, C, PH, PW, PZ), NAN, dtype=torch.float32, device=DEV)
    out32 = torch.full_like(out16, NAN)
    check(lib.aabr_roi_pool_forward_bf16(tab16, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(out16), stream()))
    check(lib.aabr_roi_pool_forward(tab32, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(out32), stream()))
    assert not torch.isnan(out16).any()                                  # every output element is written
    assert _bits([out16]) == _bits([out32])
    acc = torch.full((total, C), NAN, dtype=torch.float32, device=DEV)
    d16 = torch.full((total, C), NAN, dtype=B16, device=DEV)
    check(lib.aabr_roi_pool_backward_bf16(tab16, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(grad_d), ptr(acc),
                                          ptr(d16), total, stream()))
    assert _bits([d16]) == _bits([acc.to(B16)])                          # one rounding of the fp32 sums
    acc = acc.cpu().numpy()
    for l, (idx, rf, rb) in enumerate(case.reference()):
        _, _, _, off, V, sites = pieces[l]
        sl = acc[off:off + V]
        if len(idx) == 0:
            assert not sl.any() and not d16[off:off + V].any(), (case.name, l)       # a level without ROIs: exactly zero
        TP._check(case.name, "level %d backward, fp32 sums" % l, sl, TP._SiteResult(rb, sites))
        # 3. the single-level kernel on this level's subset
        f16, f32, cm, _, _, _ = pieces[l]
        h, w, z = P.EXTENTS[l]
        sub = _t(case.rois[idx])
        one = (P.BATCH, h, w, z, ptr(sub), len(idx), float(P.SCALES[l]), PH, PW, PZ, case.sampling)
        o16 = torch.full((len(idx), C, PH, PW, PZ), NAN, dtype=torch.float32, device=DEV)
        o32 = torch.full_like(o16, NAN)
        check(lib.aabr_roi_align_rotated_3d_sparse_forward_bf16(ptr(f16), C, ptr(cm), *one, ptr(o16), stream()))
        check(lib.aabr_roi_align_rotated_3d_sparse_forward(ptr(f32), C, ptr(cm), *one, ptr(o32), stream()))
        assert not torch.isnan(o16).any() and _bits([o16]) == _bits([o32]), (case.name, l)
        assert _bits([o16]) == _bits([out16[_t(idx)]]), (case.name, l)
        a1 = torch.full((V, C), NAN, dtype=torch.float32, device=DEV)
        d1 = torch.full((V, C), NAN, dtype=B16, device=DEV)
        check(lib.aabr_roi_align_rotated_3d_sparse_backward_bf16(ptr(_t(case.grad()[idx])), C, ptr(cm), *one, V, ptr(a1),
                                                                 ptr(d1), stream()))
        assert _bits([d1]) == _bits([a1.to(B16)]), (case.name, l)
        TP._check(case.name, "single level %d backward, fp32 sums" % l, a1.cpu().numpy(), TP._SiteResult(rb, sites))


def test_pool_level_without_sites_and_level_outside_the_table_give_zeros():
    from _hip import ptr, stream, check
    lib = _lib()
    case = TP.CASES[0]
    lv = case.levels.copy()
    lv[0], lv[5], lv[11] = NL, -1, 100
    tab16, tab32, keep, rois_d, levels_d, pieces, total = _pool_tables(case, level_v=[None, 0, None], levels_override=lv)
    n, C = case.n, case.C
    PH, PW, PZ = case.out_size
    geom = (n, PH, PW, PZ, case.sampling)
    out16 = torch.full((n, C, PH, PW, PZ), NAN, dtype=torch.float32, device=DEV)
    out32 = torch.full_like(out16, NAN)
    check(lib.aabr_roi_pool_forward_bf16(tab16, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(out16), stream()))
    check(lib.aabr_roi_pool_forward(tab32, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(out32), stream()))
    zero = _t((lv == 1) | (lv < 0) | (lv >= NL))
    assert int(zero.sum()) > 3 and not out16[zero].any() and not torch.isnan(out16).any()
    assert _bits([out16]) == _bits([out32])
    acc = torch.full((total, C), NAN, dtype=torch.float32, device=DEV)
    d16 = torch.full((total, C), NAN, dtype=B16, device=DEV)
    check(lib.aabr_roi_pool_backward_bf16(tab16, NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), *geom, ptr(_t(case.grad())),
                                          ptr(acc), ptr(d16), total, stream()))
    assert bool(torch.isfinite(acc).all()) and _bits([d16]) == _bits([acc.to(B16)])


# ------------------------------------------------------------------------------------------------ 4. glue and modules
def _maps16():
    import sparseconvnet as scn
    maps, strides = TR._small_maps()
    m16 = [scn.SparseConvNetTensor(m.features.to(B16), m.metadata, m.spatial_size) for m in maps]
    m32 = [scn.SparseConvNetTensor(m.features.float(), m.metadata, m.spatial_size) for m in m16]
    return m16, m32, strides


def _leaves(maps):
    import sparseconvnet as scn
    leaves = [m.features.detach().clone().requires_grad_(True) for m in maps]
    return leaves, [scn.SparseConvNetTensor(f, m.metadata, m.spatial_size) for f, m in zip(leaves, maps)]


def test_rpn_head_and_module_on_bf16_maps_equal_the_widened_run():
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead, build_rpn
    m16, m32, strides = _maps16()
    torch.manual_seed(11)
    head = RPNHead(rpn_glue.rpn_cfg(C=32), 32, 2).to(DEV)
    with torch.no_grad():
        for q in head.parameters():
            q.normal_(std=0.3)
    gts = [_t(S.make_gt_boxes(6, 3)), _t(S.make_gt_boxes(4, 4))]
    cfg = rpn_glue.rpn_cfg(C=32, strides=strides, voxel_scale=20.0, pre_nms_top_n=(300, 200), post_nms_top_n=(60, 40))
    torch.manual_seed(5)
    mod = build_rpn(cfg).to(DEV)
    with torch.no_grad():
        for q in mod.parameters():
            q.normal_(std=0.3)
    mod.seed = 77
    mod.train()

    def run_head(maps):
        head.zero_grad()
        leaves, xs = _leaves(maps)
        logits, bbox = head(xs)
        (sum(l.square().sum() for l in logits) + sum(b.sum() for b in bbox)).backward()
        return [l.detach() for l in logits + bbox], [f.grad for f in leaves], [q.grad.clone() for q in head.parameters()]

    def run_module(maps):
        mod.zero_grad()
        leaves, xs = _leaves(maps)
        boxes, losses = mod(None, xs, [TR._Target(g) for g in gts])
        (losses["loss_objectness"] + losses["loss_rpn_box_reg"]).backward()
        outs = [losses["loss_objectness"].detach(), losses["loss_rpn_box_reg"].detach()] + [b.bbox3d for b in boxes]
        return outs, [f.grad for f in leaves], [q.grad.clone() for q in mod.parameters()]

    for run in (run_head, run_module):
        o16, d16, p16 = run(m16)
        o32, d32, p32 = run(m32)
        assert len(o16) == len(o32) and all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(o16, o32))
        assert all(torch.isfinite(a).all() for a in o16)
        for a, b, m in zip(d16, d32, m16):
            assert a.dtype == B16 and b.dtype == torch.float32 and a.shape == m.features.shape
            assert torch.equal(a, b.to(B16))
        assert len(p16) == len(p32) and all(torch.equal(a, b) for a, b in zip(p16, p32))
        assert float(p16[0].abs().max()) > 0


POOLER_CASE = TP.CASES[1]


def _pooler_inputs(case, bf16):
    import sparseconvnet as scn
    lv = TP._levels(case)
    fs = [_t(feats).to(B16) for _, _, feats in lv]
    fs = [(f if bf16 else f.float()).requires_grad_(True) for f in fs]
    xs = [scn.SparseConvNetTensor(f, x.metadata, x.spatial_size) for f, (x, _, _) in zip(fs, lv)]
    return lv, fs, xs, [TP._Boxes(_t(b)) for b in case.boxes]


def test_pooler_module_on_bf16_levels():
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    case = POOLER_CASE
    lv, fs, xs, boxes = _pooler_inputs(case, True)
    _, _, xs32, _ = _pooler_inputs(case, False)
    pooler = Pooler(case.out_size, P.SCALES, case.sampling, P.CANONICAL, canonical_level=None)
    fused = pooler(xs, boxes)
    assert fused.dtype == torch.float32 and tuple(fused.shape) == (case.n, case.C) + case.out_size
    assert torch.equal(fused, pooler(xs32, boxes))                       # the fp32 run on the widened levels
    pooler.fused = False
    assert torch.equal(fused, pooler(xs, boxes))
    fused.backward(_t(case.grad()))
    for l, (idx, rf, rb) in enumerate(case.reference()):
        g = fs[l].grad
        assert g is not None and g.dtype == B16 and g.shape == fs[l].shape, l
        # one rounding of sums x that lie inside the fp64 slack.  bf16 keeps 8 significant bits, so to nearest
        # |bf16(x) - x| <= 2^-8 |x| (half of the ulp 2^-7 2^e, |x| >= 2^e), and |x| <= |ref| + slack.  (With 2^-9, the
        # bound of a 9-bit format, the first run measured 1.98 times the slack on 9654 elements of level 0.)
        ref = TP._SiteResult(rb, lv[l][1])
        ref.slack = ref.slack + 2.0 ** -8 * (np.abs(ref.values) + ref.slack)
        TP._check(case.name, "module level %d backward, bf16 rows" % l, g.float().cpu().numpy(), ref)
    # one level: the ROIAlignRotated3D module's own fused path
    one = Pooler(case.out_size, P.SCALES[:1], case.sampling, P.CANONICAL)
    fs[0].grad = None
    got = one(xs[:1], boxes)
    assert torch.equal(got, one(xs32[:1], boxes))
    got.sum().backward()
    assert fs[0].grad.dtype == B16 and fs[0].grad.shape == fs[0].shape


# ------------------------------------------------------------------------------------------------ 5. FPN_Net
def test_fpn_net_returns_bf16_maps_without_the_output_cast():
    from test_cabi_and_host import default_fpn
    torch.manual_seed(2)
    net = default_fpn(feature_dtype=B16).to(DEV)
    locs, feats = S.make_batch(2, 15000, 31, 20)
    l = _t(locs)
    gs = {}

    def run(cast):
        net.cast_outputs = cast
        net.zero_grad()
        rpn, roi = net([l, _t(feats)])
        maps = list(rpn) + list(roi)
        assert all(m.features.dtype == (torch.float32 if cast else B16) for m in maps)
        vals = [m.features.float() for m in maps]
        for i, v in enumerate(vals):                                     # bf16-representable weights of the loss
            if i not in gs:
                gs[i] = torch.randn(v.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(i)).to(B16).float()
        sum((v * gs[i]).sum() for i, v in enumerate(vals)).backward()
        return [v.detach() for v in vals], [(n, p.grad.clone()) for n, p in net.named_parameters() if p.grad is not None]

    v1, g1 = run(True)
    v0, g0 = run(False)
    assert len(v0) == len(v1) and all(torch.equal(a, b) for a, b in zip(v0, v1))
    assert [n for n, _ in g0] == [n for n, _ in g1] and len(g0) > 0
    for (n, a), (_, b) in zip(g0, g1):
        assert torch.equal(a, b), n


# ------------------------------------------------------------------------------------------------ 6. no host read
def test_bf16_head_and_pooler_enqueue_without_a_host_read():
    import roi_glue
    import rpn_glue
    C, A, rows = 32, 2, (130, 0, 5)
    p, f, g_obj, g_reg = R.make_case(C, A, rows, 12)
    pd = {k: _t(v).requires_grad_(True) for k, v in p.items()}
    fd = [_t(x).to(B16).requires_grad_(True) for x in f]
    go, gr = [_t(g).reshape(-1) for g in g_obj], [_t(g).reshape(-1, 7) for g in g_reg]
    case = POOLER_CASE
    lv, fs, xs, boxes = _pooler_inputs(case, True)
    props = [b.bbox3d for b in boxes]
    grad_d = _t(case.grad())

    def run():
        for q in list(pd.values()) + fd + fs:
            q.grad = None
        obj, reg = rpn_glue.rpn_head(fd, *[pd[k] for k in NAMES], feature_dtype=B16)
        torch.autograd.backward(obj + reg, go + gr)
        out = roi_glue.pool_rois(xs, props, case.out_size, P.SCALES, case.sampling, P.CANONICAL)
        out.backward(grad_d)
        return [o.detach().clone() for o in obj + reg] + [q.grad.clone() for q in list(pd.values()) + fd] + [out.detach().clone()]
    a = run()                                                            # sizes the workspace, fills the cell-map caches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _bits(a) == _bits(b)
    assert all(q.grad.dtype == B16 for q in fd + fs)
