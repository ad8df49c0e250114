"""Host side of FullConvolution / TransposeConvolution: the numpy restatement `full_conv_ref` against the definition of a
transposed convolution (torch's dense conv_transpose3d in float64), the layer's size arithmetic, `__repr__`, parameters,
and the argument refusals of the two new geometry entry points -- nothing here needs a GPU."""
import numpy as np
import pytest
import torch

import full_conv_ref as R

GEOMS = [((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 1, 2), (1, 2, 2)), ((1, 1, 1), (1, 1, 1)),
         ((2, 3, 1), (3, 1, 1))]


def _scn():
    import sparseconvnet as scn
    return scn


# ---------------------------------------------------------------------------------- the restatement against the definition
@pytest.mark.parametrize("size,stride", GEOMS)
def test_restatement_equals_dense_transposed_convolution(size, stride):
    spatial, n_in, n_out = (6, 5, 4), 3, 5
    coords = R.input_sites(7, spatial, [True, False, True], 0.3)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((len(coords), n_in))
    vol = int(np.prod(size))
    W = rng.standard_normal((vol, n_in, n_out))
    out_coords, rb = R.full_convolution_rules(coords, size, stride)
    osz = R.out_spatial(spatial, size, stride)
    got = R.densify(out_coords, R.scatter(x, W, rb, len(out_coords)), osz, 3)
    # vol is enumerated with z fastest: [kx, ky, kz, nIn, nOut] -> conv_transpose3d's [nIn, nOut, kx, ky, kz]
    Wd = torch.from_numpy(W.reshape(size + (n_in, n_out))).permute(3, 4, 0, 1, 2).contiguous()
    want = torch.nn.functional.conv_transpose3d(torch.from_numpy(R.densify(coords, x, spatial, 3)), Wd,
                                                stride=stride).numpy()
    assert want.shape == got.shape
    # float64 sums of <= vol * n_in terms of magnitude ~1 in two orders: 1e-12 is hundreds of ulps of headroom, and a
    # misplaced rule is an O(1) error
    assert np.abs(got - want).max() < 1e-12
    # exactly zero off the site list: the site list is everything a filter reaches
    off = np.ones(want.shape[:1] + want.shape[2:], bool)
    off[out_coords[:, 3], out_coords[:, 0], out_coords[:, 1], out_coords[:, 2]] = False
    assert off.any() and (want.transpose(0, 2, 3, 4, 1)[off] == 0).all()
    assert (got.transpose(0, 2, 3, 4, 1)[off] == 0).all()


def test_restatement_order_counts_and_tables():
    coords = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 2]], np.int64)
    out, rb = R.full_convolution_rules(coords, (3, 1, 1), (2, 1, 1))
    # first-seen: input rows ascending, then offsets; (2,0,0) of sample 0 is reached first by row 0 at offset 0
    assert out.tolist() == [[2, 0, 0, 0], [3, 0, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0],
                            [0, 0, 0, 2], [1, 0, 0, 2], [2, 0, 0, 2]]
    assert rb.total() == 9 and [len(rb.pairs(k)) for k in range(3)] == [3, 3, 3]
    assert rb.pairs(2).tolist() == [[0, 2], [1, 0], [2, 7]]
    t_out, t_in = R.tables(rb, 3, 8)
    assert (t_out >= 0).all()                                      # complete by construction
    assert t_in[:, 0].tolist() == [0, -1, 1] and (t_in >= 0).sum() == 9
    # samples contiguous and in batch order, brick-major key monotone over a sorted list
    assert (np.diff(out[:, 3]) >= 0).all()
    k = R.brick_major_key(np.array([[0, 0, 0, 0], [0, 0, 3, 0], [0, 1, 0, 0], [3, 3, 3, 0], [0, 0, 4, 0], [16, 0, 0, 0],
                                    [0, 0, 0, 1]]))
    assert (np.diff(k) > 0).all()


def test_identity_geometry_is_the_input_list():
    coords = R.input_sites(3, (6, 5, 4), [True, False, True], 0.4)
    out, rb = R.full_convolution_rules(coords, (1, 1, 1), (1, 1, 1))
    assert np.array_equal(out, coords) and np.array_equal(rb.pairs(0)[:, 0], rb.pairs(0)[:, 1])


# ------------------------------------------------------------------------------------------------------- the module
def test_names_and_alias():
    scn = _scn()
    assert scn.TransposeConvolution is scn.FullConvolution
    assert callable(scn.SCN.FullConvolution_updateOutput) and callable(scn.SCN.FullConvolution_backward)
    assert callable(scn.SCN.Metadata_3.getFullConvolutionRuleBook)
    assert scn.Metadata(3).fullConvolutionRuleBook is None


def test_repr_strings():
    scn = _scn()
    assert repr(scn.FullConvolution(3, 4, 8, 3, 2, False)) == "FullConvolution 4->8 C3/2"
    assert repr(scn.FullConvolution(3, 4, 8, [3, 1, 2], [1, 2, 2], False)) == "FullConvolution 4->8 C(3,1,2)/(1,2,2)"
    assert repr(scn.TransposeConvolution(3, 4, 8, 2, 2, True)) == "FullConvolution 4->8 C2/2"


def test_parameters_and_initialisation():
    scn = _scn()
    torch.manual_seed(0)
    m = scn.FullConvolution(3, 8, 16, [3, 1, 2], 2, True, groups=2)
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
    assert tuple(m.weight.shape) == (6, 2, 4, 8) and tuple(m.bias.shape) == (16,)
    assert m.filter_volume == 6 and m.dimension == 3 and m.groups == 2 and (m.nIn, m.nOut) == (8, 16)
    assert m.filter_size.tolist() == [3, 1, 2] and m.filter_stride.tolist() == [2, 2, 2]
    assert float(m.bias.detach().abs().max()) == 0.0
    assert [n for n, _ in scn.FullConvolution(3, 8, 16, 3, 2, False).named_parameters()] == ["weight"]
    # N(0, 2 g / (nIn vol)): the sample deviation of 64 * 64 * 27 values is within a few per cent of it
    big = scn.FullConvolution(3, 64, 64, 3, 2, False)
    std = (2.0 / 64 / 27) ** 0.5
    w = big.weight.detach()
    assert abs(float(w.std()) / std - 1.0) < 0.05 and abs(float(w.mean())) < 0.05 * std


@pytest.mark.parametrize("size,stride", GEOMS)
def test_size_arithmetic_round_trip(size, stride):
    scn = _scn()
    m = scn.FullConvolution(3, 4, 4, list(size), list(stride), False)
    in_sz = torch.LongTensor([6, 5, 4])
    out_sz = (in_sz - 1) * m.filter_stride + m.filter_size
    assert tuple(out_sz.tolist()) == R.out_spatial((6, 5, 4), size, stride)
    assert m.input_spatial_size(out_sz).tolist() == [6, 5, 4]


def test_input_spatial_size_asserts_on_a_size_no_input_gives():
    scn = _scn()
    m = scn.FullConvolution(3, 4, 4, 3, 2, False)
    assert m.input_spatial_size(torch.LongTensor([13, 11, 9])).tolist() == [6, 5, 4]
    with pytest.raises(AssertionError):
        m.input_spatial_size(torch.LongTensor([12, 11, 9]))


def test_plan_executor_refuses_the_module_by_name():
    scn = _scn()
    from sparseconvnet import planExecutor as P
    hits = [ln for ln in open(P.__file__).read().splitlines() if "FullConvolution" in ln and "Unsupported" in ln]
    assert hits, "planExecutor has no refusal that names FullConvolution"
    assert issubclass(P.Unsupported, Exception) and P.FullConvolution is scn.FullConvolution


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_forward_fails_loudly_without_gpu():
    scn = _scn()
    import _hip
    x = scn.InputLayer(3, [6, 5, 4], mode=4)
    with pytest.raises(_hip.AabrError):
        scn.FullConvolution(3, 2, 4, 3, 2, False)(x([torch.zeros(4, 3, dtype=torch.long), torch.zeros(4, 2)]))


# -------------------------------------------------------------------------------- argument refusals, before any launch
def _i3(v):
    import _hip
    return _hip.i32x3(v)


def test_full_convolution_sites_refuses_bad_arguments():
    import _hip
    lib = _hip.load()
    P = 4096                                    # a non-null, 16-byte aligned address: never dereferenced by a refusal
    ok = dict(coords=P, V=10, size=(3, 3, 3), stride=(2, 2, 2), osz=(13, 11, 9), keys=P, cap=512, scratch=P, out=P,
              meta=P)

    def call(**kw):
        a = dict(ok, **kw)
        g = lambda n: None if a[n] is None else _i3(a[n])
        return lib.aabr_full_convolution_sites(a["coords"], a["V"], g("size"), g("stride"), g("osz"), a["keys"], a["cap"],
                                               a["scratch"], a["out"], a["meta"], None)
    bad = [dict(V=-1), dict(size=None), dict(stride=None), dict(osz=None), dict(size=(65, 3, 3)), dict(size=(0, 3, 3)),
           dict(stride=(2, 0, 2)), dict(stride=(2, 65, 2)), dict(osz=(0, 11, 9)), dict(osz=(65536, 11, 9)),
           dict(cap=500), dict(cap=256),                    # not a power of two; below 1.5 E = 405
           dict(keys=None), dict(keys=P + 8), dict(out=None), dict(meta=None), dict(coords=None), dict(scratch=None),
           dict(V=1 << 27, cap=1 << 40),                    # E = 27 * 2^27 >= 2^31
           dict(V=1 << 31, cap=1 << 40)]
    for b in bad:
        assert call(**b) == -1, b
        assert b"aabr_full_convolution_sites" in lib.aabr_last_error(), b
    assert call(V=1 << 27, cap=1 << 40) == -1 and b"2^31" in lib.aabr_last_error()
    # composed non-overlapping levels keep the wide per-axis limit of aabr_convolution_sites, still below 2^31 candidates
    assert call(size=(4096, 4096, 4096), stride=(4096, 4096, 4096), V=1, cap=64) == -1


def test_brick_full_build_refuses_bad_arguments():
    import _hip
    lib = _hip.load()
    P = 4096
    ok = dict(coords=P, V=10, cnt=None, size=(3, 3, 3), stride=(2, 2, 2), osz=(13, 11, 9), dims=(1, 1, 1, 3), dir=P,
              bricks=P, nb_cap=64, bcoord=P, out=P, v_cap=270, meta=P, scratch=P, flags=1)

    def call(**kw):
        a = dict(ok, **kw)
        g = lambda n: None if a[n] is None else _hip.i32xn(a[n])
        return lib.aabr_brick_full_build(a["coords"], a["V"], a["cnt"], g("size"), g("stride"), g("osz"), g("dims"),
                                         a["dir"], a["bricks"], a["nb_cap"], a["bcoord"], a["out"], a["v_cap"], a["meta"],
                                         a["scratch"], a["flags"], None)
    bad = [dict(flags=2), dict(V=-1), dict(size=None), dict(stride=None), dict(osz=None), dict(size=(65, 3, 3)),
           dict(stride=(0, 2, 2)), dict(osz=(65536, 11, 9)), dict(dims=None), dict(dims=(0, 1, 1, 3)),
           dict(dims=(1, 1, 1, 0)), dict(dir=None), dict(bricks=None), dict(bcoord=None), dict(out=None), dict(meta=None),
           dict(scratch=None), dict(coords=None), dict(dir=P + 8), dict(scratch=P + 4), dict(nb_cap=0), dict(v_cap=0),
           dict(V=1 << 27)]                               # 27 * 2^27 candidates
    for b in bad:
        assert call(**b) == -1, b
        assert b"aabr_brick_full_build" in lib.aabr_last_error(), b
    assert call(V=1 << 27) == -1 and b"2^31" in lib.aabr_last_error()
    # the shrinking build keeps its own name in its messages
    assert lib.aabr_brick_build(P, -1, None, _i3((3, 3, 3)), _i3((2, 2, 2)), _i3((3, 3, 2)), _hip.i32xn((1, 1, 1, 3)), P, P,
                                64, P, P, 270, P, P, 1, None) == -1
    assert b"aabr_brick_build" in lib.aabr_last_error()
