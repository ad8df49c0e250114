"""FullConvolution / TransposeConvolution on a real MI355X: the grown level and its rule tables against the numpy restatement
(tests/full_conv_ref.py, written from FullConvolutionRules.h) in first-seen and in brick-major order, the arithmetic held
to tests/conv_exact.py (integer-granule operands: bit equality with float64), random operands inside the derived fp32
bound of the dense conv_transpose3d, and the layer composed with the layers that run on its new Metadata."""
import numpy as np
import pytest
import torch

import conv_exact as E
import full_conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24                     # unit roundoff of fp32


def _scn():
    import sparseconvnet as scn
    return scn


def _t(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.to(DEV)


def _lt(v):
    return torch.LongTensor([int(x) for x in v])


def _input(coords, spatial, order, planes=1):
    """an input-level tensor over `coords` (distinct sites, sample-major): first-seen rows = the list's order"""
    scn = _scn()
    layer = scn.InputLayer(3, list(spatial), mode=4)
    layer.site_order = order
    c = torch.as_tensor(np.array(coords, np.int64).reshape(-1, 4))
    return layer([c.to(DEV), torch.zeros((len(c), planes), device=DEV)])


# name: (spatial, live samples (one EMPTY in the middle), density, size, stride)
GEOMETRY = {
    "3/2 overlapping": ((6, 5, 4), [True, False, True], 0.30, (3, 3, 3), (2, 2, 2)),
    "2/2 disjoint": ((6, 5, 4), [True, False, True], 0.30, (2, 2, 2), (2, 2, 2)),
    "(3,1,2)/(1,2,2)": ((6, 5, 4), [True, False, True], 0.30, (3, 1, 2), (1, 2, 2)),
    "1/1 identity": ((6, 5, 4), [True, False, True], 0.30, (1, 1, 1), (1, 1, 1)),
    "no input site": ((6, 5, 4), [False, False, False], 0.30, (3, 3, 3), (2, 2, 2)),
    "E ~ 2700": ((6, 5, 4), [True, False, True], 0.4167, (3, 3, 3), (2, 2, 2)),          # 2 x 50 sites x 27
    "E ~ 80000": ((20, 18, 16), [True, False, True], 0.2570, (3, 3, 3), (2, 2, 2)),      # 2 x 1480 sites x 27: 313 blocks
}
_REF = {}


def _case(name):
    """(coords, spatial, size, stride, out_coords, rule book, t_out, t_in) of a geometry case; computed once, never changed"""
    if name not in _REF:
        spatial, live, density, size, stride = GEOMETRY[name]
        coords = R.input_sites(len(name), spatial, live, density)
        out, rb = R.full_convolution_rules(coords, size, stride)
        t_out, t_in = R.tables(rb, len(coords), len(out))
        for a in (coords, out, t_out, t_in):
            a.setflags(write=False)
        _REF[name] = (coords, spatial, size, stride, out, rb, t_out, t_in)
    return _REF[name]


def test_the_cases_have_the_sizes_they_are_named_for():
    for name, lo, hi in (("E ~ 2700", 2600, 2800), ("E ~ 80000", 78000, 82000)):
        coords, _, size, _, out, rb, _, _ = _case(name)
        assert lo <= len(coords) * int(np.prod(size)) <= hi and rb.total() == len(coords) * 27
    assert len(_case("E ~ 80000")[0]) * 27 > 256 * 256                   # past 256 scan blocks of 256 candidates
    assert len(_case("3/2 overlapping")[4]) < len(_case("3/2 overlapping")[0]) * 27     # deduplication matters
    assert len(_case("2/2 disjoint")[4]) == len(_case("2/2 disjoint")[0]) * 8
    assert len(_case("no input site")[0]) == 0


def _snapshot(md):
    return (sorted(md.grids), [id(md.grids[k]) for k in sorted(md.grids)], [md.grids[k].V for k in sorted(md.grids)],
            sorted(md.submanifold), sorted(md.rulebooks), md.site_order, md.fullConvolutionRuleBook)


def _book(x, size, stride):
    scn = _scn()
    md = x.metadata
    osz = R.out_spatial(x.spatial_size.tolist(), size, stride)
    new = scn.Metadata(3)
    before = _snapshot(md)
    tb = md.getFullConvolutionRuleBook(x.spatial_size, _lt(osz), _lt(size), _lt(stride), new)
    assert _snapshot(md) == before, "the caller's metadata changed"
    assert new.fullConvolutionRuleBook is tb and new.site_order == md.site_order
    isz = tuple(x.spatial_size.tolist())
    assert set(new.grids) == {isz, osz}
    if isz != osz:
        assert new.grids[isz] is md.grids[isz]                       # shared, never written
    assert md.getFullConvolutionRuleBook(x.spatial_size, _lt(osz), _lt(size), _lt(stride), new) is tb   # built once
    return new, tb, osz


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_first_seen_level_and_tables_equal_the_restatement(name):
    coords, spatial, size, stride, out, rb, t_out, t_in = _case(name)
    x = _input(coords, spatial, "first_seen")
    assert np.array_equal(x.get_spatial_locations().numpy().reshape(-1, 4), coords)
    new, tb, osz = _book(x, size, stride)
    got = new.getSpatialLocations(_lt(osz)).numpy().reshape(-1, 4)
    assert got.shape == out.shape and np.array_equal(got, out), "site list differs from the first-seen restatement"
    assert new.getNActive(_lt(osz)) == len(out)
    assert (tb.V_out, tb.V_in, tb.vol) == (len(coords), len(out), int(np.prod(size)))
    assert np.array_equal(tb.out.table.cpu().numpy(), t_out)
    assert np.array_equal(tb.inn.table.cpu().numpy(), t_in)
    if len(coords):
        assert (np.diff(got[:, 3]) >= 0).all() and set(got[:, 3]) == {0, 2}        # contiguous, the empty sample absent
        assert float(tb.total_rules()) == rb.total()
    # two runs give identical rows
    new2, tb2, _ = _book(_input(coords, spatial, "first_seen"), size, stride)
    assert torch.equal(new2.getSpatialLocations(_lt(osz)), new.getSpatialLocations(_lt(osz)))
    assert torch.equal(tb2.out.table, tb.out.table) and torch.equal(tb2.inn.table, tb.inn.table)


def _pairs_of(table_in, table_out, r_in, r_out, k):
    """the rules of offset k as sorted reference-row pairs, read from either table"""
    o = np.nonzero(table_in[k] >= 0)[0]
    a = sorted(zip(r_in[table_in[k][o]].tolist(), r_out[o].tolist()))
    u = np.nonzero(table_out[k] >= 0)[0]
    b = sorted(zip(r_in[u].tolist(), r_out[table_out[k][u]].tolist()))
    return a, b


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_brick_level_is_a_row_permutation_of_the_restatement(name):
    coords, spatial, size, stride, out, rb, t_out, t_in = _case(name)
    x = _input(coords, spatial, "brick")
    new, tb, osz = _book(x, size, stride)
    if len(coords):
        assert x.metadata.site_order == "brick" and new.grids[osz].brick is not None and new.grids[osz].keys is None
    r_in = R.match_rows(x.get_spatial_locations().numpy().reshape(-1, 4), coords)
    got = new.getSpatialLocations(_lt(osz)).numpy().reshape(-1, 4)
    r_out = R.match_rows(got, out)                                           # the same SET of sites
    assert (np.diff(got[:, 3]) >= 0).all(), "samples are not contiguous"
    assert (np.diff(R.brick_major_key(got)) > 0).all(), "rows are not in brick-major order"
    ti, to = tb.inn.table.cpu().numpy(), tb.out.table.cpu().numpy()
    assert ti.shape == t_in.shape and to.shape == t_out.shape
    assert (to >= 0).all()                                                   # complete by construction
    for k in range(rb.vol):
        want = sorted(map(tuple, rb.pairs(k).tolist()))
        a, b = _pairs_of(ti, to, r_in, r_out, k)
        assert a == want and b == want, "rules of offset %d differ under the row permutation" % k
    new2, tb2, _ = _book(_input(coords, spatial, "brick"), size, stride)
    assert torch.equal(new2.getSpatialLocations(_lt(osz)), new.getSpatialLocations(_lt(osz)))
    assert torch.equal(tb2.out.table, tb.out.table) and torch.equal(tb2.inn.table, tb.inn.table)


def test_a_site_outside_the_output_size_is_refused():
    """the InputLayer accepts a coordinate beyond its spatial size; the level a FullConvolution grows to does not"""
    import _hip
    for order in ("first_seen", "brick"):
        x = _input(np.array([[0, 0, 0, 0], [7, 1, 1, 0]]), (6, 5, 4), order)
        with pytest.raises(_hip.AabrError):
            _book(x, (3, 3, 3), (2, 2, 2))


# ---------------------------------------------------------------------------------------------------- exact arithmetic
def _layer(n_in, n_out, size, stride, bias, groups, seed):
    """a FullConvolution with integer weights in [-4, 4]; returns (layer, W [vol, g, nIn/g, nOut/g] float64, bias or None)"""
    scn = _scn()
    layer = scn.FullConvolution(3, n_in, n_out, list(size), list(stride), bias, groups).to(DEV)
    rng = np.random.default_rng(seed)
    W = rng.integers(-4, 5, tuple(layer.weight.shape)).astype(np.float64)
    b = rng.integers(-4, 5, n_out).astype(np.float64) if bias else None
    with torch.no_grad():
        layer.weight.copy_(_t(E.f32(W)))
        if bias:
            layer.bias.copy_(_t(E.f32(b)))
    return layer, W, b


def _run(layer, x_like, feats_dev, grad_of, dt):
    """one autograd pass; grad_of(new tensor) -> the gradient rows in device order"""
    scn = _scn()
    xs = scn.SparseConvNetTensor(_t(E.f32(feats_dev), dt).requires_grad_(True), x_like.metadata, x_like.spatial_size)
    layer.zero_grad()
    y = layer(xs)
    g = grad_of(y)
    y.features.backward(_t(E.f32(g), dt))
    return y, xs.features.grad, layer.weight.grad.clone(), (layer.bias.grad.clone() if hasattr(layer, "bias") else None)


def _exact_reference(feats, grad, W, b, rb, V_in, V_out):
    """float64 forward, input gradient, dW, d_bias over the restatement's rule book, group by group, with the exactness
    precondition of tests/conv_exact.py asserted on every sum"""
    vol, G, ci, co = W.shape
    acc, gin = np.zeros((V_out, G * co)), np.zeros((V_in, G * ci))
    dW = np.zeros(W.shape)
    for g in range(G):
        xg, gg, Wg = feats[:, g * ci:(g + 1) * ci], grad[:, g * co:(g + 1) * co], np.ascontiguousarray(W[:, g])
        bg = b[g * co:(g + 1) * co] if b is not None else np.zeros(co)
        op = E.Operands(xg, Wg, bg, np.zeros((V_out, co)), np.ones(co), False)
        E.require_exact_forward(op, rb, V_out, bias=b is not None, residual=False)
        ot = E.Operands(gg, Wg, None, None, np.ones(ci), True)
        E.require_exact_forward(ot, rb, V_in, bias=False, residual=False)
        E.require_exact_weight_grad(xg, gg, rb)
        acc[:, g * co:(g + 1) * co] = E.ref_forward(xg, Wg, rb, V_out, bg if b is not None else None)
        gin[:, g * ci:(g + 1) * ci] = E.ref_input_grad(gg, Wg, rb, V_in)
        dW[:, g] = E.ref_weight_grad(xg, gg, rb)[0]
    return acc, gin, dW, grad.sum(0)


EXACT = [  # n_in, n_out, dtype, bias, groups, geometry case, site order
    (8, 16, torch.float32, False, 1, "E ~ 2700", "first_seen"),
    (32, 32, torch.float32, True, 1, "E ~ 2700", "first_seen"),
    (64, 128, torch.float32, False, 1, "3/2 overlapping", "first_seen"),
    (32, 64, torch.bfloat16, True, 1, "E ~ 2700", "first_seen"),
    (16, 32, torch.float32, True, 2, "(3,1,2)/(1,2,2)", "first_seen"),
    (32, 32, torch.float32, True, 1, "2/2 disjoint", "first_seen"),               # filter == stride: the `single` question
    (64, 64, torch.float32, False, 1, "E ~ 80000", "first_seen"),                 # enough rows for every route to be asked
    (32, 32, torch.float32, True, 1, "E ~ 2700", "brick"),
    (32, 64, torch.bfloat16, False, 1, "2/2 disjoint", "brick"),
]


@pytest.mark.parametrize("n_in,n_out,dt,bias,groups,name,order", EXACT)
def test_layer_is_bit_exact(n_in, n_out, dt, bias, groups, name, order):
    coords, spatial, size, stride, out, rb, _, _ = _case(name)
    bf = dt == torch.bfloat16
    x = _input(coords, spatial, order)
    r_in = R.match_rows(x.get_spatial_locations().numpy().reshape(-1, 4), coords)
    layer, W, b = _layer(n_in, n_out, size, stride, bias, groups, n_in + 3 * n_out)
    rng = np.random.default_rng(n_in * 7 + n_out)
    feats, grad = E.rows(rng, len(coords), n_in), E.rows(rng, len(out), n_out)
    acc, gin, dW, db = _exact_reference(feats, grad, W, b, rb, len(coords), len(out))
    seen = {}

    def grad_of(y):
        assert tuple(y.spatial_size.tolist()) == R.out_spatial(spatial, size, stride)
        assert y.metadata is not x.metadata
        seen["r_out"] = R.match_rows(y.get_spatial_locations().numpy().reshape(-1, 4), out)
        return grad[seen["r_out"]]
    runs = [_run(layer, x, feats[r_in], grad_of, dt) for _ in range(2)]
    y, d_in, gW, gb = runs[0]
    r_out = seen["r_out"]
    if order == "first_seen":
        assert np.array_equal(r_in, np.arange(len(r_in))) and np.array_equal(r_out, np.arange(len(r_out)))
    assert y.features.dtype == dt and d_in.dtype == dt and gW.dtype == torch.float32
    if bf:
        E.assert_bits(y.features.detach(), E.expect_bf16(acc[r_out]), exact=E.to_f32_exact(acc[r_out]), what="forward")
        E.assert_bits(d_in, E.expect_bf16(gin[r_in]), exact=E.to_f32_exact(gin[r_in]), what="input gradient")
    else:
        E.assert_bits(y.features.detach().cpu().numpy(), E.to_f32_exact(acc[r_out]), what="forward")
        E.assert_bits(d_in.cpu().numpy(), E.to_f32_exact(gin[r_in]), what="input gradient")
    E.assert_bits(gW.cpu().numpy(), E.to_f32_exact(dW), what="dW")
    if bias:
        E.assert_bits(gb.cpu().numpy(), E.to_f32_exact(db), what="d_bias")
    # two runs are bit-identical
    y2, d_in2, gW2, gb2 = runs[1]
    E.assert_bits(y2.features.detach(), E.bits(y.features.detach()), what="second run, forward")
    E.assert_bits(d_in2, E.bits(d_in), what="second run, input gradient")
    E.assert_bits(gW2.cpu().numpy(), E.bits(gW), what="second run, dW")


def test_multiply_add_count_and_hidden_states():
    scn = _scn()
    coords, spatial, size, stride, out, rb, _, _ = _case("3/2 overlapping")
    x = _input(coords, spatial, "first_seen", planes=8)
    layer = scn.FullConvolution(3, 8, 16, 3, 2, False, groups=2).to(DEV)
    scn.forward_pass_multiplyAdd_count = 0
    scn.forward_pass_hidden_states = 0
    y = layer(x)
    assert float(scn.forward_pass_multiplyAdd_count) == rb.total() * 4 * 8 * 2      # nRules * ip * op * groups
    assert scn.forward_pass_hidden_states == len(out) * 16 == y.features.nelement()


# ---------------------------------------------------------------------------------------------------- random operands
def _dense_w(W, size):
    """[vol, nIn, nOut] (z fastest in vol) -> conv_transpose3d's [nIn, nOut, kx, ky, kz]"""
    return torch.from_numpy(np.asarray(W, np.float64).reshape(tuple(size) + W.shape[1:])).permute(3, 4, 0, 1, 2).contiguous()


def _at(dense, c):
    return dense[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]]


@pytest.mark.parametrize("n_in,n_out,name,bias", [(16, 24, "3/2 overlapping", True), (64, 64, "E ~ 2700", False),
                                                  (32, 32, "(3,1,2)/(1,2,2)", False)])
def test_random_operands_within_the_fp32_chain_bound(n_in, n_out, name, bias):
    """every forward element e = sum of K products (+ bias): each product and each of the additions rounds once, by at most
    2^-24 of a partial sum that never exceeds S = sum |terms| (1 + O(2^-24)) -- in ANY order of summation, through the MFMA
    and the tile read-add-write alike -- so |e - exact| <= (K + 1) 2^-24 S, the bound of the dense-layer tests.  Derived,
    not tuned."""
    scn = _scn()
    coords, spatial, size, stride, out, rb, _, _ = _case(name)
    osz = R.out_spatial(spatial, size, stride)
    rng = np.random.default_rng(n_in + n_out)
    feats = rng.standard_normal((len(coords), n_in)).astype(np.float32)
    layer = scn.FullConvolution(3, n_in, n_out, list(size), list(stride), bias).to(DEV)
    if bias:
        with torch.no_grad():
            layer.bias.copy_(_t(rng.standard_normal(n_out).astype(np.float32)))
    W = layer.weight.detach().cpu().numpy().astype(np.float64).reshape(-1, n_in, n_out)
    b = layer.bias.detach().cpu().numpy().astype(np.float64) if bias else None
    x = _input(coords, spatial, "first_seen")
    y = layer(scn.SparseConvNetTensor(_t(feats), x.metadata, x.spatial_size))
    got_coords = y.get_spatial_locations().numpy().reshape(-1, 4)
    assert np.array_equal(got_coords, out)
    dense = lambda f, w: torch.nn.functional.conv_transpose3d(
        torch.from_numpy(R.densify(coords, f, spatial, 3)), _dense_w(w, size), stride=stride).numpy()
    want = _at(dense(feats.astype(np.float64), W), out) + (b if bias else 0.0)
    S = _at(dense(np.abs(feats).astype(np.float64), np.abs(W)), out) + (np.abs(b) if bias else 0.0)
    K = E.rules_per_row(rb, len(out))[:, None] * n_in + (1 if bias else 0)
    err = np.abs(y.features.detach().cpu().numpy().astype(np.float64) - want)
    bound = (K + 1) * U * S
    worst = (err / np.maximum(bound, 1e-300)).max()
    print("%s %d->%d: largest error / bound = %.3f (K up to %d)" % (name, n_in, n_out, worst, K.max()))
    assert (err <= bound).all(), worst


# ---------------------------------------------------------------------------------------------------------- composition
def test_full_convolution_then_submanifold_then_dense():
    """FullConvolution -> SubmanifoldConvolution -> SparseToDense on the NEW metadata against conv_transpose3d -> conv3d in
    float64, masked to the grown site list (the first layer is exactly zero off it).  Bound per element, with
    S1 = sum |terms| of layer 1 (>= |y1|), K1 / K2 the term counts: layer 1 errs by at most B1 = (K1 + 1) u S1, which layer
    2 passes on as conv(B1, |W2|), and layer 2's own chain errs by (K2 + 1) u conv(|y1| + B1, |W2|) <= (K2 + 1) u (1 + u (K1 + 1))
    conv(S1, |W2|); K2 <= 27 * n_mid."""
    scn = _scn()
    coords, spatial, size, stride, out, rb, _, _ = _case("3/2 overlapping")
    osz = R.out_spatial(spatial, size, stride)
    n_in, n_mid, n_out = 8, 16, 8
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((len(coords), n_in)).astype(np.float32)
    net = scn.Sequential(scn.FullConvolution(3, n_in, n_mid, 3, 2, False),
                         scn.SubmanifoldConvolution(3, n_mid, n_out, 3, False), scn.SparseToDense(3, n_out)).to(DEV)
    x = _input(coords, spatial, "first_seen")
    got = net(scn.SparseConvNetTensor(_t(feats), x.metadata, x.spatial_size)).detach().cpu().numpy().astype(np.float64)
    assert got.shape == (3, n_out) + osz
    W1 = net[0].weight.detach().cpu().numpy().astype(np.float64).reshape(27, n_in, n_mid)
    W2 = net[1].weight.detach().cpu().numpy().astype(np.float64).reshape(27, n_mid, n_out)
    w2 = torch.from_numpy(W2.reshape(3, 3, 3, n_mid, n_out)).permute(4, 3, 0, 1, 2).contiguous()     # [out, in, kx, ky, kz]
    ct = lambda f, w: torch.nn.functional.conv_transpose3d(torch.from_numpy(R.densify(coords, f, spatial, 3)),
                                                           _dense_w(w, (3, 3, 3)), stride=stride)
    c3 = lambda d, w: torch.nn.functional.conv3d(d, w, padding=1).numpy()
    mask = np.zeros((3, 1) + osz)
    mask[out[:, 3], 0, out[:, 0], out[:, 1], out[:, 2]] = 1.0
    want = c3(ct(feats.astype(np.float64), W1), w2) * mask
    S1 = ct(np.abs(feats).astype(np.float64), np.abs(W1))
    K1 = np.zeros((3, 1) + osz)
    K1[out[:, 3], 0, out[:, 0], out[:, 1], out[:, 2]] = E.rules_per_row(rb, len(out)) * n_in
    B1 = (K1 + 1) * U * S1.numpy()
    K2 = 27 * n_mid
    bound = (c3(torch.from_numpy(B1), w2.abs()) + (K2 + 1) * U * (1 + U * (K1.max() + 1)) * c3(S1, w2.abs())) * mask
    err = np.abs(got - want)
    assert (got * (1 - mask) == 0).all()
    print("composition: largest error / bound = %.3f" % (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("order", ["first_seen", "brick"])
def test_strided_convolution_on_the_new_metadata(order):
    """FullConvolution 3/2 -> Convolution 3/2 back to the input's spatial size: the new Metadata builds further levels of
    its own (in brick order a brick pyramid under an object that has no input layer), and the level it builds under the
    input's spatial size is NOT the input level it shares with the caller -- every window that touches a grown site is a
    site.  Integer operands small enough that every sum is an exact fp32 integer in any order (layer 1: <= 8 rules x 8 planes
    x 4 x 2 = 512 per element; layer 2: <= 27 rules x 8 planes x 512 x 2 < 2^24), so the rows equal the float64 dense
    composition conv_transpose3d(stride 2) -> conv3d(stride 2) bit for bit."""
    scn = _scn()
    coords, spatial, size, stride, out, rb, _, _ = _case("3/2 overlapping")
    rng = np.random.default_rng(21)
    full = scn.FullConvolution(3, 8, 8, 3, 2, False).to(DEV)
    conv = scn.Convolution(3, 8, 8, 3, 2, False).to(DEV)
    W1 = rng.integers(-2, 3, (27, 8, 8)).astype(np.float64)
    W2 = rng.integers(-2, 3, (27, 8, 8)).astype(np.float64)
    with torch.no_grad():
        full.weight.copy_(_t(E.f32(W1)).view_as(full.weight))
        conv.weight.copy_(_t(E.f32(W2)).view_as(conv.weight))
    x = _input(coords, spatial, order)
    r_in = R.match_rows(x.get_spatial_locations().numpy().reshape(-1, 4), coords)
    before = _snapshot(x.metadata)
    feats = rng.integers(-4, 5, (len(coords), 8)).astype(np.float64)
    with torch.no_grad():
        y1 = full(scn.SparseConvNetTensor(_t(E.f32(feats[r_in])), x.metadata, x.spatial_size))
        y2 = conv(y1)
    assert y2.metadata is y1.metadata and y2.metadata is not x.metadata and _snapshot(x.metadata) == before
    assert y1.spatial_size.tolist() == [13, 11, 9] and y2.spatial_size.tolist() == list(spatial)
    got_c = y2.get_spatial_locations().numpy().reshape(-1, 4)
    d1 = torch.nn.functional.conv_transpose3d(torch.from_numpy(R.densify(coords, feats, spatial, 3)),
                                              _dense_w(W1, (3, 3, 3)), stride=2)
    touched = torch.nn.functional.conv3d(torch.from_numpy(R.densify(out, np.ones((len(out), 1)), (13, 11, 9), 3)),
                                         torch.ones((1, 1, 3, 3, 3), dtype=torch.float64), stride=2).numpy()[:, 0] > 0
    b, xs, ys, zs = np.nonzero(touched)
    R.match_rows(got_c, np.stack([xs, ys, zs, b], 1))                # the sites: every window that holds a grown site
    assert len(got_c) > len(coords)                                  # ... which are more than the shared input level's
    if order == "brick":
        assert (np.diff(R.brick_major_key(got_c)) > 0).all()
    w2 = torch.from_numpy(W2.reshape(3, 3, 3, 8, 8)).permute(4, 3, 0, 1, 2).contiguous()
    want = _at(torch.nn.functional.conv3d(d1, w2, stride=2).numpy(), got_c)
    assert np.abs(want).max() > 0
    E.assert_bits(y2.features.cpu().numpy(), E.to_f32_exact(want), what="Convolution on the new metadata")


def test_deconvolution_forward_equals_a_deconvolution_bit_for_bit():
    scn = _scn()
    spatial = (9, 7, 5)
    coords = R.input_sites(3, spatial, [True, False, True], 0.3)
    rng = np.random.default_rng(9)
    x = _input(coords, spatial, "first_seen")
    x = scn.SparseConvNetTensor(_t(rng.standard_normal((len(coords), 8)).astype(np.float32)), x.metadata, x.spatial_size)
    conv = scn.Convolution(3, 8, 16, 3, 2, False).to(DEV)
    full = scn.FullConvolution(3, 16, 8, 3, 2, True).to(DEV)
    dec = scn.Deconvolution(3, 16, 8, 3, 2, True).to(DEV)
    with torch.no_grad():
        full.bias.copy_(_t(rng.standard_normal(8).astype(np.float32)))
        dec.weight.copy_(full.weight)
        dec.bias.copy_(full.bias)
        mid = conv(x)
        a, b = full.deconvolutionForward(mid), dec(mid)
    assert a.metadata is mid.metadata and a.spatial_size.tolist() == list(spatial) == b.spatial_size.tolist()
    assert a.features.shape == (len(coords), 8)
    E.assert_bits(a.features.cpu().numpy(), E.bits(b.features), what="deconvolutionForward")
