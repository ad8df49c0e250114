"""MaxPooling / AveragePooling / UnPooling (csrc/pool.hip) on a real MI355X against `pool_ref` -- the numpy restatement of
the reference's CPU kernels over the ORACLE's rule pairs (oracle_lib.convolution_rules), so independent of the device's
gather tables -- bit for bit, and against dense torch pooling as a second, independent definition.

Rows are compared in the oracle's order: device rows are matched to oracle rows through the site coordinates (the brick
site order is a permutation of the rows)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_lib as O
import pool_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
#        spatial size   pool size   stride
GEOMS = {"2/2": ((16, 16, 8), (2, 2, 2), (2, 2, 2)),
         "3/2": ((17, 15, 9), (3, 3, 3), (2, 2, 2)),
         "118/1": ((12, 12, 8), (1, 1, 8), (1, 1, 1))}


def _scn():
    import sparseconvnet as scn
    return scn


def _L(v):
    return torch.LongTensor([int(i) for i in v])


def _ckey(c):
    c = np.asarray(c, np.int64)
    return ((c[:, 3] * 70000 + c[:, 0]) * 70000 + c[:, 1]) * 70000 + c[:, 2]


def _match(dev_coords, ref_coords):
    """oracle row of every device row (the two lists must hold the same sites)"""
    kd, kr = _ckey(dev_coords), _ckey(ref_coords)
    assert len(kd) == len(kr) and len(np.unique(kd)) == len(kd)
    if len(kd) == 0:
        return np.zeros(0, np.int64)
    order = np.argsort(kr)
    pos = np.searchsorted(kr[order], kd)
    assert (pos < len(kr)).all() and (kr[order][pos] == kd).all(), "site sets differ"
    return order[pos]


def _unique_sites(rng, spatial, n, batch):
    c = np.stack([rng.integers(0, s, n) for s in spatial], 1)
    _, first = np.unique(c, axis=0, return_index=True)
    c = c[np.sort(first)]
    return np.concatenate([c, np.full((len(c), 1), batch)], 1).astype(np.int64)


def _geometry(coords, spatial, size, stride):
    """oracle side of one scene: rule pairs per offset, output sites, and four windows (output rows with at least two
    inputs) whose input sets are pairwise disjoint -- the places of the deliberate overwrites"""
    out_sp = [(s - f) // t + 1 for s, f, t in zip(spatial, size, stride)]
    rb, oc = O.convolution_rules(coords, list(size), list(stride), out_sp)
    rules = tuple(rb.pairs(k).astype(np.int64).copy() for k in range(rb.vol))
    ins = {}
    for r in rules:
        for i, o in r:
            ins.setdefault(int(o), []).append(int(i))
    used, windows = set(), []
    for o in sorted(ins):
        if len(ins[o]) >= 2 and not used & set(ins[o]):
            windows.append(np.array(ins[o]))
            used |= set(ins[o])
            if len(windows) == 4:
                break
    return dict(coords=coords, spatial=spatial, size=size, stride=stride, out_sp=out_sp, rules=rules, oc=oc,
                windows=windows, vol=rb.vol)


@functools.lru_cache(maxsize=None)
def _scene(gname):
    """two scenes of 3 000 drawn points each (the distinct ones are the sites)"""
    spatial, size, stride = GEOMS[gname]
    rng = np.random.default_rng(sum(map(ord, gname)))
    coords = np.concatenate([_unique_sites(rng, spatial, 3000, b) for b in range(2)])
    sc = _geometry(coords, spatial, size, stride)
    assert len(sc["windows"]) == 4
    return sc


def _values(sc, planes, seed, col=0, bf16=False, specials=("neg", "tie", "negzero", "nan")):
    """[V, planes] fp32 inputs: distinct nonzero values (asserted; bf16 storage has fewer values than the larger cases
    have elements, so there they are nonzero only), then the deliberate overwrites in column `col`"""
    V = len(sc["coords"])
    N = V * planes
    rng = np.random.default_rng(seed)
    if bf16:
        v = R.round_bf16(rng.standard_normal(N).astype(np.float32))
        v[v == 0] = np.float32(1.0)
    else:          # integers + 1/4, scaled by a power of two: exact in fp32 for N < 2^21
        v = (rng.permutation(N).astype(np.float32) - np.float32(N // 2) + np.float32(0.25)) * np.float32(2.0 ** -6)
        assert len(np.unique(v)) == N
    assert (v != 0).all() and not np.isnan(v).any()
    x = v.reshape(V, planes).copy()
    w = sc["windows"]
    if "neg" in specials:        # a window with only negatives, in every column
        x[w[0]] = -np.abs(x[w[0]])
    if "tie" in specials:        # an exact tie at the window's maximum
        x[w[1][:2], col] = np.float32(2.0 ** 20)
    if "negzero" in specials:    # -0.0 beside negatives: the window gives +0, which == -0.0
        x[w[2], col] = -np.abs(x[w[2], col])
        x[w[2][0], col] = np.float32(-0.0)
    if "nan" in specials:
        x[w[3][0], col] = np.float32(np.nan)
    return x


def _grad(shape, seed, bf16=False):
    g = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return R.round_bf16(g) if bf16 else g


def _device_input(sc, x_ref, order, dtype=torch.float32):
    """the scene's input level on the device with `x_ref` (oracle row order) as its features -> (tensor, ri) with ri = the
    oracle row of every device row"""
    scn = _scn()
    layer = scn.InputLayer(3, list(sc["spatial"]), mode=4)
    layer.site_order = order
    coords = sc["coords"]
    seed = layer([torch.as_tensor(coords).to(DEV), torch.zeros((len(coords), 1), device=DEV)])
    md = seed.metadata
    ri = _match(md.getSpatialLocations(seed.spatial_size).numpy(), coords)
    feats = torch.as_tensor(np.ascontiguousarray(x_ref[ri])).to(DEV).to(dtype).requires_grad_(True)
    return scn.SparseConvNetTensor(feats, md, seed.spatial_size), ri


def _np(t):
    return t.detach().float().cpu().numpy()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        "%s: %d of %d elements differ, first at %s: got %r want %r" % (
            what, (~same).sum(), same.size, tuple(np.argwhere(~same)[0]), got[~same][0], want[~same][0])


def _check_six_passes(gname, planes, drop, order, bf16=False):
    scn = _scn()
    sc = _scene(gname)
    store = "bf16" if bf16 else "fp32"
    dtype = torch.bfloat16 if bf16 else torch.float32
    size, stride, rules = list(sc["size"]), list(sc["stride"]), sc["rules"]
    V, Vo, P = len(sc["coords"]), len(sc["oc"]), planes - drop
    x_ref = _values(sc, planes, 1000 + planes, col=drop, bf16=bf16)
    x, ri = _device_input(sc, x_ref, order, dtype)
    md = x.metadata
    dy_ref = _grad((Vo, P), 7, bf16)

    # MaxPooling
    y = scn.MaxPooling(3, size, stride, drop)(x)
    assert y.metadata is md and y.spatial_size.tolist() == sc["out_sp"] and y.features.dtype == dtype
    ro = _match(md.getSpatialLocations(y.spatial_size).numpy(), sc["oc"])
    y_ref = R.max_forward(x_ref, rules, Vo, drop, store)
    assert (y_ref >= 0).all() and (y_ref[:, :] == 0).any()
    _bits_equal(_np(y.features), y_ref[ro], "MaxPooling forward")
    y.features.backward(_dev(dy_ref[ro], dtype))
    dx = _np(x.features.grad)
    assert not np.isnan(dx).any()                  # the NaN input's window behaves as if the NaN were absent
    _bits_equal(dx, R.max_backward(x_ref, y_ref, dy_ref, rules, drop, store)[ri], "MaxPooling backward")
    assert dx.shape == (V, planes) and (dx[:, :drop] == 0).all()

    # AveragePooling
    x.features.grad = None
    a = scn.AveragePooling(3, size, stride, drop)(x)
    _bits_equal(_np(a.features), R.average_forward(x_ref, rules, Vo, drop, store)[ro], "AveragePooling forward")
    a.features.backward(_dev(dy_ref[ro], dtype))
    _bits_equal(_np(x.features.grad), R.average_backward(dy_ref, rules, V, drop, store)[ri], "AveragePooling backward")

    # UnPooling: from the coarse level back to the fine one, which is reused, not rebuilt
    fine_key = tuple(sc["spatial"])
    fine_grid, n_grids, n_books = md.grids[fine_key], len(md.grids), len(md.rulebooks)
    c_ref = _grad((Vo, planes), 8, bf16)
    c = scn.SparseConvNetTensor(_dev(c_ref[ro], dtype).requires_grad_(True), md, y.spatial_size)
    z = scn.UnPooling(3, size, stride, drop)(c)
    assert z.spatial_size.tolist() == list(sc["spatial"]) and z.metadata is md
    assert md.grids[fine_key] is fine_grid and len(md.grids) == n_grids and len(md.rulebooks) == n_books
    _bits_equal(_np(z.features), R.unpool_forward(c_ref, rules, V, drop, store)[ri], "UnPooling forward")
    dz_ref = _grad((V, P), 9, bf16)
    z.features.backward(_dev(dz_ref[ri], dtype))
    dc = _np(c.features.grad)
    _bits_equal(dc, R.unpool_backward(dz_ref, rules, Vo, drop, store)[ro], "UnPooling backward")
    assert dc.shape == (Vo, planes) and (dc[:, :drop] == 0).all()


# ---- 1. bit-equality with pool_ref, fp32 -----------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["first_seen", "brick"])
@pytest.mark.parametrize("planes,drop", [(1, 0), (3, 0), (4, 0), (32, 0), (100, 0), (128, 0), (32, 1), (32, 4)])
@pytest.mark.parametrize("gname", ["2/2", "3/2", "118/1"])
def test_six_passes_equal_pool_ref_bit_for_bit(gname, planes, drop, order):
    _check_six_passes(gname, planes, drop, order)


# ---- 2. bf16 storage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [8, 36, 128])
@pytest.mark.parametrize("gname", ["2/2", "3/2"])
def test_bf16_storage_equals_pool_ref_bit_for_bit(gname, planes):
    """max forward / backward select and add stored values; average and unpooling run the fp32 arithmetic on the widened
    values and round once at the store -- all compared with the bf16 variant of pool_ref"""
    _check_six_passes(gname, planes, 0, "first_seen", bf16=True)


# ---- 3. an independent definition: dense torch pooling -----------------------------------------------------------------
def _sites_of_dense(dense, loc):
    """[V, planes] rows of a dense [B, planes, X, Y, Z] tensor at the sites `loc` (x, y, z, b)"""
    loc = torch.as_tensor(loc).to(dense.device)
    return dense[loc[:, 3], :, loc[:, 0], loc[:, 1], loc[:, 2]]


@pytest.mark.parametrize("gname", ["3/2", "2/2"])
def test_max_pooling_equals_dense_torch_max_pool(gname):
    """SparseToDense(MaxPooling(x)) == clamp(max_pool3d(SparseToDense(x)), min=0) exactly (inactive cells are zeros in the
    dense tensor, and the sparse maximum starts at +0), and so are the input gradients: with distinct nonzero inputs each
    window has one maximum, and with small integer weights every gradient sum is exact in any order.  A window whose
    dense maximum is an inactive cell's 0 gives zero gradient in both."""
    scn = _scn()
    sc = _scene(gname)
    P = 4
    x_ref = _values(sc, P, 31, specials=("neg",))
    x, ri = _device_input(sc, x_ref, "first_seen")
    size, stride = tuple(sc["size"]), tuple(sc["stride"])
    dense = scn.SparseToDense(3, P)(x)
    want = F.max_pool3d(dense, size, stride).clamp(min=0)
    got = scn.SparseToDense(3, P)(scn.MaxPooling(3, list(size), list(stride))(x))
    assert got.shape == want.shape and torch.equal(got, want)
    assert (want == 0).any() and (want > 0).any()
    torch.manual_seed(5)
    w = torch.randint(-8, 9, want.shape, device=DEV).float()
    (got * w).sum().backward()
    g_dev = x.features.grad.clone()
    x.features.grad = None
    (want * w).sum().backward()
    assert torch.equal(g_dev, x.features.grad) and (g_dev != 0).any()


@pytest.mark.parametrize("gname", ["3/2", "2/2"])
def test_average_pooling_agrees_with_dense_torch_avg_pool(gname):
    """Bound, from the operation counts (u = 2^-24, S = sum |x_i| / vol over the window = avg_pool3d(|dense|)):
    the device adds fl(x_i / vol) in turn: vol divisions and at most vol - 1 additions, each with relative error <= u on a
    quantity of magnitude <= S (1 + u)^vol -> |device - exact| <= (2 vol - 1) u S (1 + u)^vol;
    torch adds the vol cells (vol - 1 additions; zeros add nothing) and divides or multiplies by a rounded reciprocal
    (<= 2 roundings) -> |torch - exact| <= (vol + 1) u S (1 + u)^vol.  Together < (3 vol + 1) u S, taken with S in float64.
    The input gradient of a weighted sum of the outputs is the same arithmetic over the n_w <= prod(ceil(size / stride))
    windows that hold the input, with G = sum |w| / vol in place of S: < (3 n_w + 1) u G."""
    scn = _scn()
    sc = _scene(gname)
    P = 4
    x_ref = _values(sc, P, 32, specials=("neg",))
    x, ri = _device_input(sc, x_ref, "first_seen")
    size, stride = tuple(sc["size"]), tuple(sc["stride"])
    vol, u = sc["vol"], 2.0 ** -24
    dense = scn.SparseToDense(3, P)(x)
    want = F.avg_pool3d(dense, size, stride)
    got = scn.SparseToDense(3, P)(scn.AveragePooling(3, list(size), list(stride))(x))
    S = F.avg_pool3d(dense.detach().abs().double(), size, stride)
    err = (got.double() - want.double()).abs().detach()
    print("avg forward: max err %.3e, max bound %.3e, max err/bound %.3f" % (
        float(err.max()), float(((3 * vol + 1) * u * S).max()), float((err / ((3 * vol + 1) * u * S + 1e-300)).max())))
    assert got.shape == want.shape and bool((err <= (3 * vol + 1) * u * S).all())
    torch.manual_seed(6)
    w = torch.randint(-8, 9, want.shape, device=DEV).float()
    (got * w).sum().backward()
    g_dev = x.features.grad.clone()
    x.features.grad = None
    (want * w).sum().backward()
    g_torch = x.features.grad
    d = torch.zeros(dense.shape, dtype=torch.float64, device=DEV, requires_grad=True)
    (F.avg_pool3d(d, size, stride) * w.abs().double()).sum().backward()
    G = _sites_of_dense(d.grad, x.get_spatial_locations().numpy())
    n_w = int(np.prod([-(-f // t) for f, t in zip(size, stride)]))
    gerr = (g_dev.double() - g_torch.double()).abs().detach()
    print("avg backward: max err %.3e, max bound %.3e" % (float(gerr.max()), float(((3 * n_w + 1) * u * G).max())))
    assert bool((gerr <= (3 * n_w + 1) * u * G).all()) and (g_dev != 0).any()


# ---- 4. edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["first_seen", "brick"])
def test_empty_second_scene(order):
    """scenes 0 and 2 hold sites, scene 1 none"""
    scn = _scn()
    rng = np.random.default_rng(77)
    spatial, size, stride = GEOMS["3/2"]
    coords = np.concatenate([_unique_sites(rng, spatial, 800, b) for b in (0, 2)])
    sc = _geometry(coords, spatial, size, stride)
    x_ref = _values(sc, 8, 41, specials=("neg",))
    x, ri = _device_input(sc, x_ref, order)
    y = scn.MaxPooling(3, 3, 2)(x)
    ro = _match(x.metadata.getSpatialLocations(y.spatial_size).numpy(), sc["oc"])
    y_ref = R.max_forward(x_ref, sc["rules"], len(sc["oc"]))
    _bits_equal(_np(y.features), y_ref[ro], "MaxPooling forward")
    dy_ref = _grad(y_ref.shape, 3)
    y.features.backward(_dev(dy_ref[ro]))
    _bits_equal(_np(x.features.grad), R.max_backward(x_ref, y_ref, dy_ref, sc["rules"])[ri], "MaxPooling backward")


@pytest.mark.parametrize("order", ["first_seen", "brick"])
def test_entirely_empty_input(order):
    scn = _scn()
    layer = scn.InputLayer(3, [17, 15, 9], mode=4)
    layer.site_order = order
    seed = layer([torch.zeros((0, 4), dtype=torch.int64, device=DEV), torch.zeros((0, 1), device=DEV)])
    for cls in (scn.MaxPooling, scn.AveragePooling):
        f = torch.zeros((0, 6), device=DEV, requires_grad=True)
        y = cls(3, 3, 2, 2)(scn.SparseConvNetTensor(f, seed.metadata, seed.spatial_size))
        assert tuple(y.features.shape) == (0, 4) and y.spatial_size.tolist() == [8, 7, 4]
        y.features.sum().backward()
        assert tuple(f.grad.shape) == (0, 6)
    c = torch.zeros((0, 6), device=DEV, requires_grad=True)
    z = scn.UnPooling(3, 3, 2, 2)(scn.SparseConvNetTensor(c, seed.metadata, y.spatial_size))
    assert tuple(z.features.shape) == (0, 4) and z.spatial_size.tolist() == [17, 15, 9]
    z.features.sum().backward()
    assert tuple(c.grad.shape) == (0, 6)
    torch.cuda.synchronize()


def test_rule_book_is_shared_with_a_strided_convolution():
    scn = _scn()
    sc = _scene("2/2")
    x, _ = _device_input(sc, _values(sc, 8, 51, specials=()), "first_seen")
    md = x.metadata
    conv = scn.Convolution(3, 8, 8, 2, 2, False).to(DEV)
    yc = conv(x)
    loc = md.getSpatialLocations(yc.spatial_size).numpy().copy()
    grid, books = md.grids[tuple(sc["out_sp"])], dict(md.rulebooks)
    yp = scn.MaxPooling(3, 2, 2)(x)
    assert md.grids[tuple(sc["out_sp"])] is grid and md.rulebooks == books and len(books) == 1
    assert yp.features.shape == yc.features.shape
    np.testing.assert_array_equal(md.getSpatialLocations(yp.spatial_size).numpy(), loc)


def test_unpooling_without_the_fine_level_raises():
    scn = _scn()
    sc = _scene("2/2")
    x, _ = _device_input(sc, _values(sc, 4, 52, specials=()), "first_seen")
    with pytest.raises(RuntimeError, match=r"32, 32, 16"):        # the level UnPooling 2/2 would return to
        scn.UnPooling(3, 2, 2)(x)
    assert list(x.metadata.grids) == [tuple(sc["spatial"])]      # nothing was built on the way


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_pass_is_bit_identical_run_to_run(dtype):
    scn = _scn()
    sc = _scene("3/2")
    bf16 = dtype == torch.bfloat16
    x_ref = _values(sc, 40, 61, bf16=bf16)
    runs = []
    for _ in range(2):
        x, ri = _device_input(sc, x_ref, "first_seen", dtype)
        out = []
        for cls in (scn.MaxPooling, scn.AveragePooling):
            x.features.grad = None
            y = cls(3, 3, 2)(x)
            y.features.backward(_dev(_grad(tuple(y.features.shape), 5, bf16), dtype))
            out += [y.features.detach(), x.features.grad]
        c = y.features.detach().clone().requires_grad_(True)
        z = scn.UnPooling(3, 3, 2)(scn.SparseConvNetTensor(c, x.metadata, y.spatial_size))
        z.features.backward(_dev(_grad(tuple(z.features.shape), 6, bf16), dtype))
        runs.append([t.view(torch.int16 if bf16 else torch.int32).cpu() for t in out + [z.features.detach(), c.grad]])
    assert len(runs[0]) == 6 and all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 5. nets ---------------------------------------------------------------------------------------------------------
def _net_input(net, out_size, planes, seed):
    """two scenes through an InputLayer whose spatial size the net's own `input_spatial_size` gives"""
    scn = _scn()
    spatial = net.input_spatial_size(_L(out_size)).tolist()
    rng = np.random.default_rng(seed)
    coords = np.concatenate([_unique_sites(rng, spatial, 3000, b) for b in range(2)])
    feats = rng.standard_normal((len(coords), planes)).astype(np.float32)
    layer = scn.InputLayer(3, spatial, mode=4)
    return layer, coords, feats, spatial


def _run_net(net, layer, coords, feats):
    net.zero_grad(set_to_none=True)
    y = net(layer([torch.as_tensor(coords).to(DEV), torch.as_tensor(feats).to(DEV)]))
    torch.manual_seed(9)
    (y.features * torch.randn_like(y.features)).sum().backward()
    return y, [y.features.detach().clone()] + [p.grad.clone() for p in net.parameters()]


def _check_net(net, layer, coords, feats, rows_want):
    y, first = _run_net(net, layer, coords, feats)
    assert y.features.shape[0] == rows_want
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    _, second = _run_net(net, layer, coords, feats)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    return y


def test_vgg_net_forward_backward():
    scn = _scn()
    torch.manual_seed(0)
    net = scn.SparseVggNet(3, 3, [['C', 8], 'MP', ['C', 16], ['MP', 2, 2], ['C', 16]]).to(DEV)
    layer, coords, feats, spatial = _net_input(net, [4, 4, 2], 3, 70)
    assert spatial == [17, 17, 9]
    _, mid = O.convolution_rules(coords, [3, 3, 3], [2, 2, 2], [8, 8, 4])
    _, top = O.convolution_rules(mid, [2, 2, 2], [2, 2, 2], [4, 4, 2])
    y = _check_net(net, layer, coords, feats, len(top))
    assert y.spatial_size.tolist() == [4, 4, 2] and y.features.shape[1] == 16
    # the features after the first MaxPooling == pool_ref applied to the device's own preceding activations
    x = layer([torch.as_tensor(coords).to(DEV), torch.as_tensor(feats).to(DEV)])
    with torch.no_grad():
        h = net[1](net[0](x))
        p = net[2](h)
    rb, oc = O.convolution_rules(coords, [3, 3, 3], [2, 2, 2], [8, 8, 4])
    ri = _match(x.get_spatial_locations().numpy(), coords)
    ro = _match(p.get_spatial_locations().numpy(), oc)
    h_ref = np.empty((len(coords), 8), np.float32)
    h_ref[ri] = _np(h.features)
    want = R.max_forward(h_ref, [rb.pairs(k) for k in range(rb.vol)], len(oc))
    _bits_equal(_np(p.features), want[ro], "MaxPooling inside the VGG net")


def test_unet_forward_backward():
    scn = _scn()
    torch.manual_seed(1)
    net = scn.UNet(3, 1, [8, 16, 24], residual_blocks=True).to(DEV)
    layer, coords, feats, spatial = _net_input(net, [16, 16, 8], 8, 71)
    assert spatial == [16, 16, 8]
    y = _check_net(net, layer, coords, feats, len(coords))
    assert y.features.shape[1] == 8


def test_fully_convolutional_net_forward_backward():
    scn = _scn()
    torch.manual_seed(2)
    net = scn.FullyConvolutionalNet(3, 1, [8, 16]).to(DEV)
    layer, coords, feats, spatial = _net_input(net, [16, 16, 8], 8, 72)
    y = _check_net(net, layer, coords, feats, len(coords))
    assert y.features.shape[1] == 8 + 16 and y.spatial_size.tolist() == [16, 16, 8]
