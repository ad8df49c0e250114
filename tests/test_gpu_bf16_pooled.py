"""bf16 storage of the pooled ROI tensor on the device: the pooler's write-out and the head's Conv3d([1, 1, pz]) GEMMs
(csrc/roi_pool.hip, csrc/roi_mlp.hip: the *_pooled_bf16 entry points), roi_glue.pool_rois(pooled_dtype=...), _Mlp on a
bf16 pooled operand, Pooler.pooled_dtype and FPN2MLPFeatureExtractor.pooled_dtype.

The rule is that of tests/test_gpu_bf16_heads.py.  Storage only: a bf16 element is widened on load (exact), every
operation is the fp32 kernel's, a bf16 result is ONE rounding (nearest even) of the fp32 value.  So every bf16 input here
is bf16-representable by construction, the yardstick is the existing fp32 entry point on the widened values, and the
comparison is byte equality -- this file has no tolerance of its own.  Outputs are pre-filled with NaN and none may be
left.  The one place where bits cannot be compared is the pooler's backward, whose fp32 atomics fix no order: its fp32
sums are held to the fp64 slack of tests/roi_align_ref.py exactly as tests/test_gpu_roi_pool.py holds the fp32 path (the
fp64 reference is evaluated on the same bf16-representable gradient), and the bf16 rows to the rounding of those sums."""
import numpy as np
import pytest
import torch

import roi_align_ref as R
import roi_pool_ref as P
import test_gpu_bf16_heads as TH
import test_gpu_corner_head as TC
import test_gpu_roi_mlp as TM
import test_gpu_roi_pool as TP

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
B16 = torch.bfloat16
NAN = float("nan")
NL = len(P.SCALES)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lib():
    import _hip
    return _hip.load()


def _bits(t):
    """the tensor's bytes; no NaN may be left in it"""
    assert not torch.isnan(t).any()
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()


# ------------------------------------------------------------------------------------------------ 1. GEMM entry points
def _run_gemm(C, res, n, N, relu, bias, seed=0):
    """the three products on a pooled A [n, C, ph, pw, pz]: the bf16 entry points on A16 against the fp32 ones on
    A16.float() -> (weight gradient was split, the tile edges the three products ran with)"""
    import _hip
    from _hip import check, ptr, stream
    lib = _lib()
    ph, pw, pz = res
    hw, K, M_ = ph * pw, C * pz, n * ph * pw
    rng = np.random.default_rng(seed + 7 * M_ + 3 * N + K)
    A16 = _t(rng.standard_normal((n, C, ph, pw, pz)).astype(F)).to(B16)
    A32 = A16.float()
    W = _t(rng.standard_normal((N, K)).astype(F))
    b = _t(rng.standard_normal(N).astype(F)) if bias else None
    g = _t(rng.standard_normal((M_, N)).astype(F))
    tag = "C %d res %s n %d N %d%s%s" % (C, res, n, N, " relu" if relu else "", " bias" if bias else "")
    y16 = torch.full((M_, N), NAN, dtype=torch.float32, device=DEV)
    y32 = torch.full_like(y16, NAN)
    check(lib.aabr_roi_mlp_forward_pooled_bf16(ptr(A16), hw, pz, ptr(W), ptr(b), int(relu), M_, N, K, ptr(y16), stream()))
    check(lib.aabr_roi_mlp_forward(ptr(A32), _hip.MLP_POOLED, hw, pz, ptr(W), ptr(b), int(relu), M_, N, K, ptr(y32),
                                   stream()))
    assert _bits(y16) == _bits(y32), "forward " + tag
    mask = ptr(y32) if relu else None
    d16 = torch.full(A16.shape, NAN, dtype=B16, device=DEV)
    d32 = torch.full(A16.shape, NAN, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_mlp_backward_input_pooled_bf16(ptr(g), mask, ptr(W), M_, N, K, hw, pz, ptr(d16), stream()))
    check(lib.aabr_roi_mlp_backward_input(ptr(g), mask, ptr(W), M_, N, K, _hip.MLP_POOLED, hw, pz, ptr(d32), stream()))
    assert d16.dtype == B16 and _bits(d16) == _bits(d32.to(B16)), "input gradient " + tag
    splits = lib.aabr_roi_mlp_dw_splits(M_, N, K)
    floats = lib.aabr_roi_mlp_dw_scratch_floats(M_, N, K)
    scr = torch.empty(max(floats, 1), dtype=torch.float32, device=DEV)
    outs = []
    for which in ("bf16", "bf16 again", "fp32"):
        if which == "bf16 again" and splits == 1:
            continue
        dw = torch.full((N, K), NAN, dtype=torch.float32, device=DEV)
        db = torch.full((N,), NAN, dtype=torch.float32, device=DEV) if bias else None
        if which == "fp32":
            check(lib.aabr_roi_mlp_backward_weight(ptr(g), mask, ptr(A32), _hip.MLP_POOLED, hw, pz, M_, N, K, 0, ptr(dw),
                                                   ptr(db), ptr(scr) if floats else None, stream()))
        else:
            check(lib.aabr_roi_mlp_backward_weight_pooled_bf16(ptr(g), mask, ptr(A16), hw, pz, M_, N, K, 0, ptr(dw), ptr(db),
                                                               ptr(scr) if floats else None, stream()))
        outs.append(_bits(dw) + (_bits(db) if bias else b""))
    assert all(o == outs[-1] for o in outs), "weight / bias gradient (splits %d) " % splits + tag   # and equal run to run
    return splits > 1, {lib.aabr_roi_mlp_tile(M_, N), lib.aabr_roi_mlp_tile(M_, K), lib.aabr_roi_mlp_tile(N, K)}


def _threshold_shapes():
    """(C, res, n, N) on both sides of the 64 / 128 tile threshold in M and in K, found with aabr_roi_mlp_tile as
    tests/test_gpu_roi_mlp.py finds them"""
    lib = _lib()
    C, res = 8, (2, 3, 2)
    hw, pz = res[0] * res[1], res[2]
    n = 1
    while lib.aabr_roi_mlp_tile(n * hw, 1) != 128:
        n += 1
    assert lib.aabr_roi_mlp_tile(n * hw, C * pz) == 128 and lib.aabr_roi_mlp_tile((n - 1) * hw, C * pz) == 64
    k = 4
    while lib.aabr_roi_mlp_tile(1, k) != 128:
        k += 4
    assert (k - 4) % pz == 0 and k % pz == 0
    return [(C, res, n - 1, 1), (C, res, n, 1), (C, res, n // 2 + 1, 130),
            ((k - 4) // pz, res, 2, 1), (k // pz, res, 2, 1), ((k // 2 + 6) // pz, res, 50, 130)]


@pytest.mark.parametrize("relu,bias", [(False, True), (True, False)])
def test_gemm_entry_points_equal_the_fp32_ones_on_the_widened_tensor(relu, bias):
    split, tiles = set(), set()
    shapes = [(C, res, n, 10) for C, res in ((8, (2, 3, 2)), (5, (2, 3, 4))) for n in (1, 5, 37)]
    shapes += [(C, res, 60, TM._tile_crossing()[1]) for C, res in ((8, (2, 3, 2)), (5, (2, 3, 4)))]   # the split
    shapes += _threshold_shapes()
    shapes += [(4, (2, 3, 3), n, 10) for n in (1, 5, 37)] + [(4, (2, 3, 3), 60, TM._tile_crossing()[1])]   # odd pz, K = 12
    for C, res, n, N in shapes:
        s, t = _run_gemm(C, res, n, N, relu, bias)
        split.add(s)
        tiles |= t
    assert split == {False, True} and tiles == {64, 128}                  # both split sides and both tile sizes were run


# ------------------------------------------------------------------------------------------------ 2. pooler, C ABI
POOL_CASES = [TP.CASES[0], TP.CASES[1], TP.CASES[3], TP.CASES[4]]        # [3]: an empty scene; [4]: no ROI maps to level 1
_REF16 = {}


def _grad16(case):
    """the case's output gradient rounded to bf16: (device bf16 tensor, the same values as a float32 numpy array)"""
    g16 = _t(case.grad()).to(B16)
    return g16, g16.float().cpu().numpy()


def _ref16(case, keep=None):
    """per level the fp64 backward Result of tests/roi_align_ref.py for the bf16-representable gradient, over the level's
    ROIs (`keep`: a mask over all ROIs, the others add nothing); computed once per case"""
    key = (case.name, None if keep is None else keep.tobytes())
    if key not in _REF16:
        g = _grad16(case)[1]
        out = []
        for l, idx in enumerate(P.level_sets(case.levels, NL)):
            if keep is not None:
                idx = idx[keep[idx]]
            h, w, z = P.EXTENTS[l]
            out.append((idx, R.backward(g[idx], case.rois[idx], P.SCALES[l], case.out_size, (P.BATCH, case.C, h, w, z),
                                        case.sampling)))
        _REF16[key] = out
    return _REF16[key]


def _pool_both(case, tabs, rois_d, levels_d, total, f16):
    """forward and backward through the new entry points with fp32 (f16 = 0) or bf16 (1) levels, the forward against
    the existing entry point of that storage -> (out16, acc, d16 or None)"""
    from _hip import ptr, stream, check
    lib = _lib()
    n, C = case.n, case.C
    head = (tabs[f16], NL, C, P.BATCH, ptr(rois_d), ptr(levels_d), n) + case.out_size + (case.sampling,)
    out16 = torch.full((n, C) + case.out_size, NAN, dtype=B16, device=DEV)
    out32 = torch.full((n, C) + case.out_size, NAN, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_pool_forward_pooled_bf16(*head, f16, ptr(out16), stream()))
    check((lib.aabr_roi_pool_forward_bf16 if f16 else lib.aabr_roi_pool_forward)(*head, ptr(out32), stream()))
    assert _bits(out16) == _bits(out32.to(B16)), (case.name, f16)        # one rounding of the fp32 output, all written
    g16 = _grad16(case)[0]
    acc = torch.full((total, C), NAN, dtype=torch.float32, device=DEV)
    d16 = torch.full((total, C), NAN, dtype=B16, device=DEV) if f16 else None
    check(lib.aabr_roi_pool_backward_pooled_bf16(*head, f16, ptr(g16), ptr(acc), ptr(d16), total, stream()))
    assert not torch.isnan(acc).any()
    if f16:
        assert _bits(d16) == _bits(acc.to(B16)), (case.name, "one rounding of the fp32 sums")
    return out16, acc, d16


@pytest.mark.parametrize("f16", [0, 1], ids=["fp32_levels", "bf16_levels"])
@pytest.mark.parametrize("case", POOL_CASES, ids=[c.name for c in POOL_CASES])
def test_pool_entry_points_forward_and_backward(case, f16):
    tab16, tab32, keep, rois_d, levels_d, pieces, total = TH._pool_tables(case)
    out16, acc, d16 = _pool_both(case, (tab32, tab16), rois_d, levels_d, total, f16)
    acc = acc.cpu().numpy()
    for l, (idx, rb) in enumerate(_ref16(case)):
        _, _, _, off, V, sites = pieces[l]
        sl = acc[off:off + V]
        if len(idx) == 0:
            assert not sl.any() and (d16 is None or not d16[off:off + V].any()), (case.name, l)   # exactly zero
        TP._check(case.name, "level %d backward, fp32 sums" % l, sl, TP._SiteResult(rb, sites))


@pytest.mark.parametrize("f16", [0, 1], ids=["fp32_levels", "bf16_levels"])
def test_pool_level_without_sites_and_level_outside_the_table_give_zeros(f16):
    case = TP.CASES[0]
    lv = case.levels.copy()
    lv[0], lv[5], lv[11] = NL, -1, 100
    tab16, tab32, keep, rois_d, levels_d, pieces, total = TH._pool_tables(case, level_v=[None, 0, None], levels_override=lv)
    out16, acc, d16 = _pool_both(case, (tab32, tab16), rois_d, levels_d, total, f16)
    zero = _t((lv == 1) | (lv < 0) | (lv >= NL))
    assert int(zero.sum()) > 3 and not out16[zero].any() and out16[~zero].any()
    assert bool(torch.isfinite(acc).all())


@pytest.mark.parametrize("f16", [0, 1], ids=["fp32_levels", "bf16_levels"])
def test_pool_roi_with_a_scene_index_outside_the_batch(f16):
    """the cell maps cover one scene: the ROIs of scene 1 name an empty sample -- zeros forward, nothing backward"""
    case = TP.CASES[0]
    tab16, tab32, keep, rois_d, levels_d, pieces, total = TH._pool_tables(case)
    for tab in (tab16, tab32):
        for l in range(NL):
            tab[l].nb = 1
    out16, acc, d16 = _pool_both(case, (tab32, tab16), rois_d, levels_d, total, f16)
    inside = case.rois[:, 0] < 1
    assert 0 < inside.sum() < case.n and not out16[_t(~inside)].any() and out16[_t(inside)].any()
    acc = acc.cpu().numpy()
    for l, (idx, rb) in enumerate(_ref16(case, inside)):
        _, _, _, off, V, sites = pieces[l]
        TP._check(case.name, "level %d backward, scene 0 only" % l, acc[off:off + V], TP._SiteResult(rb, sites))


# ------------------------------------------------------------------------------------------------ 3. glue and modules
def _module_case(corner, counts):
    if corner:
        return P.PoolCase("bf16_pooled_corner_%d_%d" % counts, 900 + sum(counts), TC.C_, (TC.PH, 11, 2), 2, counts)
    return P.PoolCase("bf16_pooled_%d_%d" % counts, 800 + sum(counts), 8, (2, 3, 2), 2, counts)


def _extractor_run(ext, xs, fs, boxes, g, bf16):
    """the extractor forward and backward: pooled in bf16, or (the yardstick) the same module in fp32 with the pooler's
    result replaced by pooled.to(bf16).float() through a forward hook"""
    seen = {}

    def hook(_m, _i, out):
        out = out if bf16 else out.to(B16).float()
        out.retain_grad()
        seen["pooled"] = out
        return out
    ext.zero_grad()
    for f in fs:
        f.grad = None
    ext.pooled_dtype = B16 if bf16 else torch.float32
    handle = ext.pooler.register_forward_hook(hook)
    try:
        x = ext(xs, boxes)
    finally:
        handle.remove()
    outs = [x.x_cor, x[2]] if isinstance(x, list) else [x]
    sum((o * w).sum() for o, w in zip(outs, g)).backward()
    return dict(outs=[o.detach() for o in outs], pooled=seen["pooled"].detach(), d_pooled=seen["pooled"].grad.clone(),
                params={k: v.grad.clone() for k, v in ext.named_parameters()}, d_feats=[f.grad.clone() for f in fs])


@pytest.mark.parametrize("counts", [(1, 0), (23, 14)], ids=["1roi", "37rois"])
@pytest.mark.parametrize("corner", [False, True], ids=["plain", "corner"])
def test_extractor_with_a_bf16_pooled_tensor(corner, counts):
    ext = (TC._build() if corner else TM._build())[0]
    assert ext.pooled_dtype == torch.float32 and ext.fused
    case = _module_case(corner, counts)
    lv, fs, xs, boxes = TP._module_inputs(case)
    n, R_ = sum(counts), 12
    rng = np.random.default_rng(23)
    g = [_t(rng.standard_normal(s).astype(F)) for s in (((2 * n, R_), (n, R_)) if corner else ((n, R_),))]
    got = _extractor_run(ext, xs, fs, boxes, g, True)
    want = _extractor_run(ext, xs, fs, boxes, g, False)
    assert got["pooled"].dtype == B16 and got["d_pooled"].dtype == B16 and want["pooled"].dtype == torch.float32
    assert tuple(got["pooled"].shape) == (n, case.C) + case.out_size
    assert _bits(got["pooled"].float()) == _bits(want["pooled"])          # the pooler's bf16 write-out
    for a, b in zip(got["outs"], want["outs"]):
        assert a.dtype == torch.float32 and _bits(a) == _bits(b)
    assert sorted(got["params"]) == sorted(want["params"]) and len(got["params"]) == (12 if corner else 8)
    for k in got["params"]:
        assert _bits(got["params"][k]) == _bits(want["params"][k]), k     # convolution, BatchNorm, fc6, fc7
    assert any(float(v.abs().max()) > 0 for v in got["params"].values())
    # the gradient of the pooled tensor: one rounding of the fp32 value; the yardstick's autograd rounds it the same way
    # on its way through .to(bf16).float(), so both poolers' backward passes receive the same values ...
    assert _bits(got["d_pooled"]) == _bits(want["d_pooled"].to(B16))
    # ... and differ only in the order of their fp32 atomics: each side within the fp64 slack of that gradient's exact
    # level gradients, as tests/test_gpu_roi_pool.py holds the fp32 path
    g_np = got["d_pooled"].float().cpu().numpy()
    for l, idx in enumerate(P.level_sets(case.levels, NL)):
        h, w, z = P.EXTENTS[l]
        rb = TP._SiteResult(R.backward(g_np[idx], case.rois[idx], P.SCALES[l], case.out_size, (P.BATCH, case.C, h, w, z),
                                       case.sampling), lv[l][1])
        for side, res in (("bf16 pooled", got), ("yardstick", want)):
            d = res["d_feats"][l]
            assert d.dtype == torch.float32 and d.shape == fs[l].shape
            TP._check(case.name, "level %d gradient, %s" % (l, side), d.cpu().numpy(), rb)
        # ... and the two sides within that slack of EACH OTHER on the decided entries, the bound the feature was asked
        # to meet.  It asks more than the two checks above imply (they allow twice the slack): both sides add the same
        # fp32 contributions, so the slack's per-contribution part cancels in the difference and only the two orders'
        # summation errors remain, each at most gamma(m - 1) sum |contribution|.  An entry with zero slack (no
        # contribution) must be equal.
        diff = np.abs(got["d_feats"][l].cpu().numpy().astype(np.float64) - want["d_feats"][l].cpu().numpy().astype(np.float64))
        dec = ~np.broadcast_to(rb.undecided, diff.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(diff[dec] == 0, 0.0, diff[dec] / rb.slack[dec])
        print("level %d: max |bf16 pooled - yardstick| / slack = %.4g" % (l, float(ratio.max()) if ratio.size else 0.0))
        assert (diff[dec] <= rb.slack[dec]).all(), (case.name, l, float(ratio.max()))


def test_pooler_module_and_glue_with_a_bf16_pooled_tensor():
    import roi_glue
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    case = TP.CASES[1]
    for levels16 in (False, True):
        lv, fs, xs, boxes = TH._pooler_inputs(case, levels16)
        pooler = Pooler(case.out_size, P.SCALES, case.sampling, P.CANONICAL, canonical_level=None)
        want = pooler(xs, boxes)
        assert want.dtype == torch.float32
        pooler.pooled_dtype = B16
        fused = pooler(xs, boxes)
        assert fused.dtype == B16 and _bits(fused) == _bits(want.to(B16))
        pooler.fused = False                                               # the reference's loop, cast once: the yardstick
        assert _bits(pooler(xs, boxes)) == _bits(fused)
        g16 = _grad16(case)[0]
        fused.backward(g16)
        for l, (idx, rb) in enumerate(_ref16(case)):
            d = fs[l].grad
            assert d is not None and d.dtype == fs[l].dtype and d.shape == fs[l].shape
            if not levels16:
                TP._check(case.name, "module level %d backward" % l, d.cpu().numpy(), TP._SiteResult(rb, lv[l][1]))
    # one level with a bf16 pooled tensor: the same gather, rounded once
    one = Pooler(case.out_size, P.SCALES[:1], case.sampling, P.CANONICAL)
    want = one(xs[:1], boxes)
    one.pooled_dtype = B16
    assert _bits(one(xs[:1], boxes)) == _bits(want.to(B16))
    props = [b.bbox3d for b in boxes]
    with pytest.raises(TypeError):
        roi_glue.pool_rois(xs, props, case.out_size, P.SCALES, case.sampling, P.CANONICAL, pooled_dtype=torch.float16)
    x = torch.zeros((4, 8), device=DEV)
    with pytest.raises(TypeError):
        roi_glue.dense_linear(x.to(B16), torch.zeros((3, 8), device=DEV), None, False)
    ext = TM._build()[0]
    ext.fused = False
    ext.pooled_dtype = B16
    _, _, xs8, boxes8 = TP._module_inputs(_module_case(False, (23, 14)))
    with pytest.raises(TypeError):                                         # the torch modules are fp32
        ext(xs8, boxes8)


# ------------------------------------------------------------------------------------------------ 4. nothing moved
def test_calls_without_the_new_keyword_return_fp32():
    import roi_glue
    ext = TM._build()[0]
    case = _module_case(False, (23, 14))
    lv, fs, xs, boxes = TP._module_inputs(case)
    pooled = roi_glue.pool_rois(xs, [b.bbox3d for b in boxes], case.out_size, P.SCALES, case.sampling, P.CANONICAL)
    assert pooled.dtype == torch.float32 and torch.equal(pooled, ext.pooler(xs, boxes))
    conv, bn = ext.conv3d[0], ext.conv3d[1]
    state = {"eps": bn.eps, "momentum": bn.momentum, "training": True, "track_running_stats": False, "running_mean": None,
             "running_var": None}
    x4 = roi_glue.box_head_mlp(pooled, conv.weight, conv.bias, bn.weight, bn.bias, state, ext.fc6.weight, ext.fc6.bias,
                               ext.fc7.weight, ext.fc7.bias)
    assert x4.dtype == torch.float32 and torch.equal(x4, ext.head(pooled))
    x4.sum().backward()
    assert all(f.grad.dtype == torch.float32 for f in fs) and conv.weight.grad.dtype == torch.float32
