"""BLInputLayer / BLOutputLayer and input_pipeline.quantize_scenes_bl on a real MI355X.

The reference is tests/bl_ref.py, the numpy restatement of the batched input layer (pinned to the reference's own CPU
kernels by tests/test_bl_input_host.py); floating point is compared BIT FOR BIT -- the kernels do the same fp32
operations in the same order.  Both site orders run: "first_seen" must give the restatement's rows, "brick" a
permutation of them inside every sample, found through the site coordinates as in tests/test_gpu_brick.py."""
import functools

import numpy as np
import pytest
import torch

import bl_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = ["first_seen", "brick"]
FLAT_MODE = {1: 2, 2: 1, 3: 3, 4: 4}       # BL mode -> the flat InputLayer's mode with the same meaning


def _scn():
    import sparseconvnet as scn
    return scn


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _ckey(c):
    c = np.asarray(c, np.int64)
    return ((c[:, 3] * 70000 + c[:, 0]) * 70000 + c[:, 1]) * 70000 + c[:, 2]


def _match(dev_coords, ref_coords):
    """reference row of every device row (the two lists must hold the same sites, each once)"""
    kd, kr = _ckey(dev_coords), _ckey(ref_coords)
    assert len(kd) == len(kr) and len(np.unique(kd)) == len(kd)
    if len(kd) == 0:
        return np.zeros(0, np.int64)
    order = np.argsort(kr)
    pos = np.searchsorted(kr[order], kd)
    assert (pos < len(kr)).all() and (kr[order][pos] == kd).all(), "site sets differ"
    return order[pos]


def _layer(scn, spatial, mode, order):
    layer = scn.BLInputLayer(3, list(spatial), mode=mode)
    layer.site_order = order
    return layer


def _run(scn, coords, feats, spatial, mode, order):
    f = _t(feats).requires_grad_(True)
    return _layer(scn, spatial, mode, order)([_t(coords), f]), f


def _rows(x, rb, order):
    """r: device row i holds the restatement's row r[i]; checks the site list, the sample count and the sample offsets"""
    from sparseconvnet import SCN
    loc = x.get_spatial_locations().numpy()
    assert loc.shape == (rb["V"], 4) and x.features.shape[0] == rb["V"]
    if order == "first_seen":
        np.testing.assert_array_equal(loc, rb["site_coords"])
    r = _match(loc, rb["site_coords"])
    # samples are contiguous and in order; first row of every sample = the restatement's offsets, for exactly B samples
    assert (np.diff(loc[:, 3]) >= 0).all()
    np.testing.assert_array_equal(np.searchsorted(loc[:, 3], np.arange(rb["B"] + 1)), rb["sample_off"])
    assert SCN._batch_size(x.metadata) == rb["B"]
    return r


def _check_against_ref(scn, coords, feats, spatial, mode, order, rb, ref_out, rng):
    """everything test 1 and test 3 ask of one (batch, mode, order): sites, rule book, features, d features, BLOutputLayer
    and its gradient -- floating point bit for bit"""
    B, L, C_ = feats.shape
    x, f = _run(scn, coords, feats, spatial, mode, order)
    r = _rows(x, rb, order)
    md = x.metadata
    np.testing.assert_array_equal(md.input["point_site"].cpu().numpy()[rb["point_site"] >= 0],
                                  np.argsort(r)[rb["point_site"][rb["point_site"] >= 0]])
    assert (md.input["point_site"].cpu().numpy()[rb["point_site"] < 0] == -1).all()
    hdr, rules = md.blLayerRuleBook()
    assert hdr == [mode, rb["max_active"], B, L, rb["V"]]
    rules, want = rules.cpu().numpy(), rb["rules"][r]
    assert rules.shape == want.shape and rules.dtype == np.int32
    np.testing.assert_array_equal(rules[:, 0], want[:, 0])
    listed = np.arange(want.shape[1] - 1)[None, :] < want[:, :1]             # entries past the count are unspecified
    np.testing.assert_array_equal(rules[:, 1:][listed], want[:, 1:][listed])
    assert R.same_bits(x.features.detach().cpu().numpy(), ref_out[r])
    # d features
    g = rng.standard_normal(ref_out.shape).astype(np.float32)                # restatement's row order
    x.features.backward(_t(g[r]))
    d_in = f.grad.cpu().numpy()
    assert d_in.shape == (B, L, C_) and R.same_bits(d_in, R.backward(rb, g))
    unlisted = np.ones(B * L, bool)
    unlisted[[p for pts in rb["listed"] for p in pts]] = False
    assert unlisted.any() and not d_in.reshape(B * L, C_)[unlisted].any()    # empty / unselected rows: exactly zero
    # BLOutputLayer on fresh site rows, and its gradient
    h_ref = rng.standard_normal(ref_out.shape).astype(np.float32)
    h = _t(h_ref[r]).requires_grad_(True)
    out = scn.BLOutputLayer(3)(scn.SparseConvNetTensor(h, md, x.spatial_size))
    assert tuple(out.shape) == (B, L, C_) and out.dtype == torch.float32
    got = out.detach().cpu().numpy()
    assert R.same_bits(got, R.output_layer(rb, h_ref))
    assert not got.reshape(B * L, C_)[unlisted].any()
    go = rng.standard_normal((B, L, C_)).astype(np.float32)
    out.backward(_t(go))
    assert R.same_bits(h.grad.cpu().numpy(), R.output_layer_grad(rb, go)[r])


# ------------------------------------------------------------------ 1. the traps, at the smallest size
E = [-1, -1, -1]
TRAPS = np.array([[[2, 3, 4], [5, 5, 5], E, [2, 3, 4], [-1, 5, 6], [2, 3, 4], [7, 1, 0]],     # empty row in the middle,
                  [E] * 7,                                                                    # a row empty although
                  [[9, 9, 9], [2, 3, 4], E, [9, 9, 9], E, E, E]], np.int64)                  # y, z >= 0; (2,3,4) x 3 + 1


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_traps_smallest_size(mode, order):
    scn = _scn()
    rng = np.random.default_rng(mode)
    feats = rng.standard_normal((3, 7, 3)).astype(np.float32)
    rb = R.bl_rules(TRAPS, mode)
    assert rb["V"] == 5 and rb["sample_off"].tolist() == [0, 3, 3, 5] and len(rb["points"][0]) == 3
    _check_against_ref(scn, TRAPS, feats, (16, 16, 16), mode, order, rb, R.forward(rb, feats), rng)


# ------------------------------------------------------------------ 2. equivalence with the tested flat path
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_equals_input_layer_on_the_compacted_list(mode):
    scn = _scn()
    rng = np.random.default_rng(20 + mode)
    B, L, C_ = 3, 300, 5
    coords = np.stack([rng.integers(0, s, (B, L)) for s in (6, 5, 4)], 2).astype(np.int64)
    coords[rng.random((B, L)) < 0.2] = -1
    feats = rng.standard_normal((B, L, C_)).astype(np.float32)
    keep = coords[:, :, 0] >= 0
    flat = np.concatenate([coords[keep], np.nonzero(keep)[0][:, None]], 1)      # [n, 4], batch column appended
    torch.manual_seed(mode)
    conv = scn.SubmanifoldConvolution(3, C_, 8, 3, False).to(DEV)
    x, _ = _run(scn, coords, feats, (8, 8, 8), mode, "first_seen")
    y = scn.InputLayer(3, [8, 8, 8], mode=FLAT_MODE[mode])([_t(flat), _t(feats[keep])])
    assert torch.equal(x.get_spatial_locations(), y.get_spatial_locations())     # same sites, same order
    assert x.features.shape[0] < keep.sum() and torch.equal(x.features.detach(), y.features)
    with torch.no_grad():
        assert torch.equal(conv(x).features, conv(y).features)


# ------------------------------------------------------------------ 3. chunk and sample boundaries
@functools.lru_cache(maxsize=None)
def _boundary_case(planes, mode):
    """B = 3, L = 1500 over a 12 x 12 x 6 box (chains of several points at most sites), plus one voxel of sample 1 that
    holds 40 points on both sides of a chunk boundary: the numbering kernel's 1024-point chunks end inside samples and
    samples end inside chunks; empty rows at random, the last sample's tail empty"""
    rng = np.random.default_rng(planes)
    B, L = 3, 1500
    coords = np.stack([rng.integers(0, s, (B, L)) for s in (12, 12, 6)], 2).astype(np.int64)
    coords[rng.random((B, L)) < 0.1, 0] = -1 - rng.integers(0, 3)
    coords[2, 1100:] = -1
    coords[1, 400:1400:25] = (3, 3, 3)                          # flat rows 1900 .. 2875: chunk 1 and chunk 2
    feats = rng.standard_normal((B, L, planes)).astype(np.float32)
    rb = R.bl_rules(coords, mode)
    return coords, feats, rb, R.forward(rb, feats)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("planes", [3, 260])
def test_chunk_and_sample_boundaries(planes, mode, order):
    coords, feats, rb, ref_out = _boundary_case(planes, mode)
    assert rb["max_active"] >= 40                                # far beyond the in-register chain sort
    _check_against_ref(_scn(), coords, feats, (16, 16, 8), mode, order, rb, ref_out, np.random.default_rng(7))


# ------------------------------------------------------------------ 4. a trailing empty sample is still a sample
@pytest.mark.parametrize("order", ORDERS)
def test_trailing_empty_sample(order):
    scn = _scn()
    from sparseconvnet import SCN
    coords = np.array([[[0, 1, 2], [3, 3, 3], E, [0, 1, 2]], [E] * 4], np.int64)
    feats = np.arange(2 * 4 * 2, dtype=np.float32).reshape(2, 4, 2) + 1
    x, _ = _run(scn, coords, feats, (4, 4, 4), 3, order)
    assert x.features.shape[0] == 2 and SCN._batch_size(x.metadata) == 2
    dense = scn.SparseToDense(3, 2)(x).detach().cpu().numpy()
    assert dense.shape == (2, 2, 4, 4, 4)
    want = np.zeros_like(dense)
    want[0, :, 0, 1, 2] = feats[0, 0] + feats[0, 3]
    want[0, :, 3, 3, 3] = feats[0, 1]
    np.testing.assert_array_equal(dense, want)
    assert not dense[1].any()


# ------------------------------------------------------------------ 5. mode 0
@pytest.mark.parametrize("order", ORDERS)
def test_mode0_unique_and_all_present(order):
    scn = _scn()
    import _hip
    B, L, C_ = 2, 30, 4
    rng = np.random.default_rng(5)
    cells = np.stack([rng.permutation(64)[:L] for _ in range(B)])
    coords = np.stack([cells // 16, cells // 4 % 4, cells % 4], 2).astype(np.int64)
    feats = rng.standard_normal((B, L, C_)).astype(np.float32)
    x, f = _run(scn, coords, feats, (4, 4, 4), 0, order)
    rb = R.bl_rules(coords, 0)
    r = _rows(x, rb, order)                                         # first_seen: r = 0 .. B L - 1, rows in flat order
    assert R.same_bits(x.features.detach().cpu().numpy(), feats.reshape(B * L, C_)[r])
    assert x.metadata.blLayerRuleBook()[0] == [0, 1, B, L, B * L]
    dup, hole = coords.copy(), coords.copy()
    dup[1, 7] = dup[1, 3]
    hole[0, 11] = -1
    for bad in (dup, hole):
        with pytest.raises(_hip.AabrError, match="mode 0"):
            _run(scn, bad, feats, (4, 4, 4), 0, order)


# ------------------------------------------------------------------ 6. errors
@pytest.mark.parametrize("order", ORDERS)
def test_bad_coordinates_raise(order):
    scn = _scn()
    import _hip
    feats = np.ones((2, 3, 2), np.float32)
    for bad_row in ([3, -1, 2], [3, 2, -7], [1, 70000, 1], [65535, 0, 0]):
        coords = np.array([[[1, 1, 1], E, [2, 2, 2]], [[1, 1, 1], bad_row, E]], np.int64)
        with pytest.raises(_hip.AabrError, match="65534"):
            _run(scn, coords, feats, (16, 16, 16), 3, order)


def test_mixing_the_two_forms_raises():
    scn = _scn()
    import _hip
    coords = np.array([[[1, 1, 1], E, [2, 2, 2]]], np.int64)
    feats = np.ones((1, 3, 2), np.float32)
    x, _ = _run(scn, coords, feats, (16, 16, 16), 3, "first_seen")
    with pytest.raises(_hip.AabrError, match="BLOutputLayer"):
        scn.OutputLayer(3)(x)
    y = scn.InputLayer(3, [16, 16, 16], mode=3)([_t(coords[0][[0, 2]]), _t(feats[0][[0, 2]])])
    with pytest.raises(_hip.AabrError, match="OutputLayer"):
        scn.BLOutputLayer(3)(y)
    with pytest.raises(_hip.AabrError, match="BLInputLayer"):
        y.metadata.blLayerRuleBook()


# ------------------------------------------------------------------ 7. degenerate shapes
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(0, 5), (3, 0), (2, 6)])
def test_degenerate_shapes(shape, order):
    scn = _scn()
    from sparseconvnet import SCN
    B, L = shape
    coords = np.full((B, L, 3), -1, np.int64)
    if B and L:
        coords[:, :, 1:] = 4                                       # all rows empty, whatever y and z hold
    x, f = _run(scn, coords, np.ones((B, L, 3), np.float32), (8, 8, 8), 4, order)
    assert tuple(x.features.shape) == (0, 3) and SCN._batch_size(x.metadata) == B
    assert tuple(x.get_spatial_locations().shape) == (0, 4)
    out = scn.BLOutputLayer(3)(x)
    assert tuple(out.shape) == (B, L, 3) and not out.detach().cpu().numpy().any()
    out.sum().backward()
    assert tuple(f.grad.shape) == (B, L, 3) and not f.grad.cpu().numpy().any()
    dense = scn.SparseToDense(3, 3)(x)
    assert tuple(dense.shape) == (B, 3, 8, 8, 8) and not dense.detach().cpu().numpy().any()


# ------------------------------------------------------------------ 8. prepare
@pytest.mark.parametrize("order", ORDERS)
def test_prepare_is_picked_up_by_identity_and_version(order):
    scn = _scn()
    rng = np.random.default_rng(8)
    coords = np.stack([rng.integers(0, s, (2, 400)) for s in (10, 10, 5)], 2).astype(np.int64)
    coords[rng.random((2, 400)) < 0.1] = -1
    feats = rng.standard_normal((2, 400, 4)).astype(np.float32)
    want = _run(scn, coords, feats, (16, 16, 8), 4, order)[0]
    side = torch.cuda.Stream()
    for dt in (torch.int64, torch.int32):
        c = _t(coords).to(dt)
        layer = _layer(scn, (16, 16, 8), 4, order)
        layer.prepare(c, torch.device(DEV), side)
        assert len(layer._prepared) == 1
        prepared_md = layer._prepared[0][3]
        y = layer([c, _t(feats)])
        assert len(layer._prepared) == 0 and y.metadata is prepared_md
        assert torch.equal(y.features, want.features.detach())
        assert torch.equal(y.get_spatial_locations(), want.get_spatial_locations())
        # after an in-place edit of the tensor the prepared geometry is stale and must not be picked up
        layer.prepare(c, torch.device(DEV), side)
        stale_md = layer._prepared[0][3]
        c[0, 0] = torch.tensor([9, 9, 4], dtype=dt, device=DEV)
        z = layer([c, _t(feats)])
        assert len(layer._prepared) == 1 and z.metadata is not stale_md
        edited = coords.copy()
        edited[0, 0] = (9, 9, 4)
        zw = _run(scn, edited, feats, (16, 16, 8), 4, order)[0]
        assert torch.equal(z.features, zw.features.detach())
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 9. the quantiser
FULL, SCALE = (64, 64, 32), 20


def _scenes(rng, sizes, dtype, extra):
    xs = [torch.as_tensor((rng.random((n, 3)) * (3.4, 3.3, 1.7) + (-1.5, 3.0, 0.25)).astype(dtype)).to(DEV) for n in sizes]
    es = [torch.as_tensor(rng.standard_normal((n, extra)).astype(np.float32)).to(DEV) for n in sizes] if extra else None
    return xs, es


def _check_quantised(coords, feats, xs, es, L):
    import input_pipeline as P
    B, C_ = len(xs), 3 + (es[0].shape[1] if es else 0)
    assert tuple(coords.shape) == (B, L, 3) and coords.dtype == torch.int64
    assert tuple(feats.shape) == (B, L, C_) and feats.dtype == torch.float32
    locs, fl = P.quantize_scenes(xs, es, SCALE, FULL)
    o = 0
    for b, x in enumerate(xs):
        n = x.shape[0]
        assert torch.equal(coords[b, :n], locs[o:o + n, :3]), b
        assert bool((feats[b, :n] == fl[o:o + n]).all()), b
        assert bool((coords[b, n:] == -1).all()) and not bool(feats[b, n:].any()), b         # padding rows, exactly
        dropped = coords[b, :n, 0] < 0
        assert bool((coords[b, :n][dropped] == -1).all())
        o += n
    return locs


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quantize_scenes_bl_equals_quantize_scenes(dtype, extra):
    import input_pipeline as P
    rng = np.random.default_rng(90 + extra)
    sizes = [0, 1, 257, 1000]
    xs, es = _scenes(rng, sizes, dtype, extra)
    coords, feats = P.quantize_scenes_bl(xs, es, SCALE, FULL)
    locs = _check_quantised(coords, feats, xs, es, 1000)
    n_drop = int((locs[:, 0] < 0).sum())
    assert 0 < n_drop < sum(sizes) // 2                             # some points lie outside full_scale, most inside
    c2, f2 = P.quantize_scenes_bl(xs, es, SCALE, FULL, length=1024)
    _check_quantised(c2, f2, xs, es, 1024)
    assert torch.equal(c2[:, :1000], coords) and bool((f2[:, :1000] == feats).all())
    with pytest.raises(ValueError, match="999"):
        P.quantize_scenes_bl(xs, es, SCALE, FULL, length=999)


def test_quantize_scenes_bl_chunks_of_32():
    import input_pipeline as P
    rng = np.random.default_rng(33)
    xs, es = _scenes(rng, [5] * 33, np.float32, 2)
    coords, feats = P.quantize_scenes_bl(xs, es, SCALE, FULL)
    _check_quantised(coords, feats, xs, es, 5)


# ------------------------------------------------------------------ 10. end to end
@pytest.mark.parametrize("order", ORDERS)
def test_end_to_end_equals_the_flat_pipeline(order):
    scn = _scn()
    import input_pipeline as P
    rng = np.random.default_rng(10)
    xs, es = _scenes(rng, [300, 0, 777, 64], np.float32, 3)
    coords, feats = P.quantize_scenes_bl(xs, es, SCALE, FULL)
    layer = _layer(scn, FULL, 4, order)
    x = layer([coords, feats])
    locs, fl = P.quantize_scenes(xs, es, SCALE, FULL)
    flat = scn.InputLayer(3, list(FULL), mode=4)
    flat.site_order = order
    y = flat([locs, fl])
    assert x.features.shape[0] > 100
    assert torch.equal(x.get_spatial_locations(), y.get_spatial_locations())
    assert torch.equal(x.features, y.features)
