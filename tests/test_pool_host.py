"""Host side of the pooling modules, activations and network builders: names, spatial-size arithmetic, `__repr__`, the
builders' layer order and parameter counts, the numpy restatement `pool_ref` on a hand-written case, and the no-GPU error."""
import numpy as np
import pytest
import torch

import pool_ref as R


def _scn():
    import sparseconvnet as scn
    return scn


def _leaves(net):
    return [type(m).__name__ for m in net.modules() if not list(m.children())]


def _nparams(net):
    return sum(p.numel() for p in net.parameters())


def test_names_exist():
    scn = _scn()
    for name in ("MaxPooling", "AveragePooling", "UnPooling", "Sigmoid", "LeakyReLU", "Tanh", "ReLU", "ELU", "SELU",
                 "SparseVggNet", "SparseResNet", "UNet", "FullyConvolutionalNet"):
        assert hasattr(scn, name), name
    for op in ("MaxPooling", "AveragePooling", "UnPooling"):
        for half in ("updateOutput", "updateGradInput"):
            assert callable(getattr(scn.SCN, "%s_%s" % (op, half)))
    from sparseconvnet.maxPooling import MaxPoolingFunction
    from sparseconvnet.averagePooling import AveragePoolingFunction
    from sparseconvnet.unPooling import UnPoolingFunction
    for f in (MaxPoolingFunction, AveragePoolingFunction, UnPoolingFunction):
        assert issubclass(f, torch.autograd.Function)


def test_abi_entries_validate_before_launching():
    import _hip
    lib = _hip.load()
    assert lib.aabr_version() == _hip.ABI_VERSION == 640
    ok = dict(src=8, bf16=0, ss=4, c0=0, planes=4, table=8, vol=8, rows=1, mode=0, div=0.0, dst=8, ds=4, dc0=0, dw=4)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.aabr_pool_gather(a["src"], a["bf16"], a["ss"], a["c0"], a["planes"], a["table"], a["vol"], a["rows"],
                                    a["mode"], a["div"], a["dst"], a["ds"], a["dc0"], a["dw"], None)
    for bad in (dict(planes=0), dict(vol=0), dict(mode=2), dict(src=None), dict(table=None), dict(dst=None),
                dict(rows=-1), dict(c0=1), dict(dw=3), dict(div=-1.0)):
        assert call(**bad) == -1, bad
    assert b"aabr_pool_gather" in lib.aabr_last_error()
    assert call(rows=0, src=None, table=None, dst=None) == 0          # an empty destination: no launch, no error
    mb = lambda x=8, planes=4, vol=8, rows=1, xs=4: lib.aabr_pool_max_backward(x, 8, 8, 0, xs, 0, planes, 8, vol, rows, 8,
                                                                                 None)
    assert mb(x=None) == -1 and mb(planes=0) == -1 and mb(vol=0) == -1 and mb(xs=5) == -1
    assert mb(rows=0) == 0


@pytest.mark.parametrize("cls", ["MaxPooling", "AveragePooling"])
def test_pooling_spatial_size_and_exact_fit(cls):
    scn = _scn()
    m = getattr(scn, cls)(3, 3, 2)
    assert m.input_spatial_size(torch.LongTensor([8, 7, 4])).tolist() == [17, 15, 9]
    assert m._coarse(torch.LongTensor([17, 15, 9])).tolist() == [8, 7, 4]
    x = scn.SparseConvNetTensor(torch.zeros(0, 4), scn.Metadata(3), torch.LongTensor([17, 15, 8]))
    with pytest.raises(AssertionError):
        m(x)                                 # 17 x 15 x 8 is no exact fit of 3/2 windows (checked before any device work)
    a = getattr(scn, cls)(3, [1, 1, 8], [1, 1, 1])
    assert a._coarse(torch.LongTensor([12, 12, 8])).tolist() == [12, 12, 1]


def test_unpooling_inverts_the_pooling_arithmetic():
    scn = _scn()
    u = scn.UnPooling(3, 3, 2)
    assert u._fine(torch.LongTensor([8, 7, 4])).tolist() == [17, 15, 9]
    assert u.input_spatial_size(torch.LongTensor([17, 15, 9])).tolist() == [8, 7, 4]
    with pytest.raises(AssertionError):
        u.input_spatial_size(torch.LongTensor([17, 15, 8]))
    assert u.unpool and not scn.MaxPooling(3, 3, 2).unpool


def test_repr_matches_the_reference_format():
    scn = _scn()
    assert repr(scn.MaxPooling(3, 3, 2)) == "MaxPooling3/2"
    assert repr(scn.MaxPooling(3, [1, 1, 8], [1, 1, 1])) == "MaxPooling(1,1,8)/(1,1,1)"
    assert repr(scn.AveragePooling(3, 2, 2)) == "AveragePooling2/2"
    assert repr(scn.UnPooling(3, 2, 2)) == "UnPooling2/2"
    assert repr(scn.UnPooling(3, [1, 1, 8], 1)) == "UnPooling(1,1,8)/(1,1,1)"
    assert repr(scn.MaxPooling(3, 3, 2, nFeaturesToDrop=4)) == "MaxPooling3/2 nFeaturesToDrop = 4"


def test_vgg_builder():
    scn = _scn()
    net = scn.SparseVggNet(3, 2, [['C', 8], ['C', 8], 'MP', ['C', 16]])
    assert list(net._modules) == [str(i) for i in range(7)]
    assert [type(m).__name__ for m in net] == ["SubmanifoldConvolution", "BatchNormReLU", "SubmanifoldConvolution",
                                               "BatchNormReLU", "MaxPooling", "SubmanifoldConvolution", "BatchNormReLU"]
    assert _nparams(net) == 432 + 16 + 1728 + 16 + 3456 + 32 == 5680
    assert net.input_spatial_size(torch.LongTensor([8, 7, 4])).tolist() == [17, 15, 9]
    assert set(net.state_dict()) >= {"0.weight", "1.weight", "1.bias", "1.running_mean", "5.weight", "6.running_var"}
    # ['MP', size, stride], 'C3/2' and a 'Plus' layer: Conv + BN, then [SubmConv | down-SubmConv-up] joined + BN
    net = scn.SparseVggNet(3, 4, ['C3/2', ['MP', 2, 2], ['C', 8, 4]])
    assert _leaves(net) == ["Convolution", "BatchNormReLU", "MaxPooling", "SubmanifoldConvolution", "Convolution",
                            "BatchNormReLU", "SubmanifoldConvolution", "BatchNormReLU", "Deconvolution", "JoinTable",
                            "BatchNormReLU"]
    assert repr(net[2]) == "MaxPooling2/2"
    assert _nparams(net) == (27 * 4 * 4 + 8) + 27 * 4 * 8 + (27 * 4 * 4 + 8 + 27 * 4 * 4 + 8 + 27 * 4 * 4) + 24


def test_unet_builder():
    """UNet(3, 1, [8, 16], residual_blocks=True) in the reference's layer order: block(8, 8); [Identity | BN, Convolution 2/2,
    U([16]) = block(16, 16), BN, Deconvolution 2/2]; JoinTable; block(16, 8) -- a residual block(a, b) being
    ConcatTable[Identity or NetworkInNetwork | BN(a), SubmConv a->b, BN(b), SubmConv b->b] + AddTable"""
    scn = _scn()
    net = scn.UNet(3, 1, [8, 16], residual_blocks=True)
    B, S = "BatchNormLeakyReLU", "SubmanifoldConvolution"
    block = lambda shortcut: [shortcut, B, S, B, S, "AddTable"]
    assert _leaves(net) == block("Identity") + ["Identity", B, "Convolution"] + block("Identity") + [B, "Deconvolution"] + \
        ["JoinTable"] + block("NetworkInNetwork")
    subm, bn = lambda a, b: 27 * a * b, lambda a: 2 * a
    res = lambda a, b: (a * b if a != b else 0) + bn(a) + subm(a, b) + bn(b) + subm(b, b)
    want = res(8, 8) + bn(8) + 8 * 8 * 16 + res(16, 16) + bn(16) + 8 * 16 * 8 + res(16, 8)
    assert _nparams(net) == want == 24832
    assert list(net._modules) == ["0", "1", "2", "3", "4", "5"]
    assert "2.1.2.0.1.1.weight" in net.state_dict()        # the inner U's first SubmConv
    assert net.input_spatial_size(torch.LongTensor([16, 16, 8])).tolist() == [16, 16, 8]
    # VGG-style blocks, leakiness and the first block's input planes
    net = scn.UNet(3, 2, [8, 16], leakiness=0.2, n_input_planes=3)
    assert _leaves(net)[:4] == [B, S, B, S] and net[0][1].nIn == 3 and net[1][1].nIn == 8
    assert net[0][0].leakiness == 0.2


def test_fully_convolutional_builder():
    """FullyConvolutionalNet(3, 1, [8, 16]): block(8, 8) = [BN, SubmConv]; [Identity | BN, Convolution 2/2, U([16]) =
    [BN, SubmConv 16->16], UnPooling 2/2]; JoinTable -- 8 + 16 output planes"""
    scn = _scn()
    net = scn.FullyConvolutionalNet(3, 1, [8, 16])
    assert _leaves(net) == ["BatchNormReLU", "SubmanifoldConvolution", "Identity", "BatchNormReLU", "Convolution",
                            "BatchNormReLU", "SubmanifoldConvolution", "UnPooling", "JoinTable"]
    assert _nparams(net) == (16 + 27 * 8 * 8) + 16 + 8 * 8 * 16 + (32 + 27 * 16 * 16) == 9728
    assert repr(net[1][1][3]) == "UnPooling2/2"
    res = scn.FullyConvolutionalNet(3, 2, [8, 16, 24], residual_blocks=True)
    assert _leaves(res).count("UnPooling") == 2 and _leaves(res).count("AddTable") == 6


def test_resnet_builder():
    scn = _scn()
    net = scn.SparseResNet(3, 4, [['basic', 8, 2, 1], ['basic', 16, 1, 2]])
    B, S = "BatchNormReLU", "SubmanifoldConvolution"
    assert _leaves(net) == [B, S, B, S, "NetworkInNetwork", "AddTable",          # rep 0: 4 -> 8 planes, stride 1
                            B, S, B, S, "Identity", "AddTable",                  # rep 1
                            B, "Convolution", B, S, "Convolution", "AddTable",   # 8 -> 16 planes, stride 2
                            B]
    assert _nparams(net) == (8 + 27 * 4 * 8 + 16 + 27 * 8 * 8 + 4 * 8) + (16 + 27 * 8 * 8 + 16 + 27 * 8 * 8) + \
        (16 + 27 * 8 * 16 + 32 + 27 * 16 * 16 + 27 * 8 * 16) + 32


def test_pool_ref_on_a_hand_written_case():
    """four input rows on a line, 2/1-like windows written by hand: window 0 = rows (0, 1), window 1 = rows (1, 2),
    window 2 = rows (2, 3); offset 0 = a window's left row, offset 1 = its right row"""
    rules = [np.array([[0, 0], [1, 1], [2, 2]]), np.array([[1, 0], [2, 1], [3, 2]])]
    nan = np.float32(np.nan)
    #            all negative | tie in window 1   | NaN beside 0.5
    x = np.array([[-1.0, 2.0, 5.0], [-3.0, 7.0, nan], [-2.0, 7.0, 0.5], [-4.0, 1.0, 0.25]], np.float32)
    y = R.max_forward(x, rules, 3)
    np.testing.assert_array_equal(y, np.array([[0, 7, 5], [0, 7, 0.5], [0, 7, 0.5]], np.float32))
    assert not np.signbit(y[:, 0]).any()
    dy = np.array([[1, 10, 100], [2, 20, 200], [4, 40, 400]], np.float32)
    dx = R.max_backward(x, y, dy, rules)
    np.testing.assert_array_equal(dx, np.array([[0, 0, 100], [0, 30, 0], [0, 60, 600], [0, 0, 0]], np.float32))
    # a -0.0 input equals the +0 a window of negatives gives, as in the reference's `==`
    xz = np.array([[-0.0], [-1.0], [-1.0], [-1.0]], np.float32)
    yz = R.max_forward(xz, rules, 3)
    assert not np.signbit(yz).any() and (yz == 0).all()
    np.testing.assert_array_equal(R.max_backward(xz, yz, dy[:, :1], rules)[:, 0], [1, 0, 0, 0])
    # average: x / vol per term, fp32, ascending offset; unpool: plain sums over the transposed pairs
    a = R.average_forward(x[:, :2], rules, 3)
    want = np.float32(-1.0) / np.float32(2) + np.float32(-3.0) / np.float32(2)
    assert a[0, 0] == want and a.dtype == np.float32
    np.testing.assert_array_equal(R.average_backward(dy, rules, 4)[:, 0], [0.5, 1.5, 3.0, 2.0])
    np.testing.assert_array_equal(R.unpool_forward(dy, rules, 4)[:, 0], [1, 3, 6, 4])
    np.testing.assert_array_equal(R.unpool_backward(x[:, :1], rules, 3)[:, 0], [-4, -5, -6])
    # nFeaturesToDrop: the forward reads columns [drop, C), the gradient is full width with zeros in front
    yd = R.max_forward(x, rules, 3, drop=1)
    np.testing.assert_array_equal(yd, y[:, 1:])
    dxd = R.max_backward(x, yd, dy[:, 1:], rules, drop=1)
    np.testing.assert_array_equal(dxd, np.concatenate([np.zeros((4, 1), np.float32), dx[:, 1:]], 1))
    # bf16 store: one rounding to nearest even
    r = R.round_bf16(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, np.nan], np.float32))
    assert r[0] == 1.0 and r[1] == np.float32(1.0 + 2.0 ** -6) and r[2] == np.float32(1.0 + 2.0 ** -7) and np.isnan(r[3])
    assert R.average_forward(R.round_bf16(x[:, :2]), rules, 3, store="bf16")[0, 0] == np.float32(-2.0)


@pytest.mark.parametrize("name,fn", [("Sigmoid", torch.sigmoid), ("Tanh", torch.tanh),
                                     ("ReLU", torch.nn.functional.relu), ("ELU", torch.nn.functional.elu),
                                     ("SELU", torch.nn.functional.selu),
                                     ("LeakyReLU", lambda t: torch.nn.functional.leaky_relu(t, 1 / 3))])
def test_activations_are_torch_on_the_features(name, fn):
    scn = _scn()
    torch.manual_seed(4)
    f = torch.randn(50, 7, requires_grad=True)
    md, size = object(), torch.LongTensor([9, 8, 7])
    act = getattr(scn, name)()
    out = act(scn.SparseConvNetTensor(f, md, size))
    assert out.metadata is md and out.spatial_size is size
    assert torch.equal(out.features, fn(f))
    out.features.sum().backward()
    g = torch.autograd.grad(fn(f).sum(), f)[0]
    assert torch.equal(f.grad, g)
    assert act.input_spatial_size(size) is size
    assert scn.LeakyReLU().leak == 1 / 3 and scn.LeakyReLU(0.1).leak == 0.1


def test_operators_refuse_host_tensors():
    """the hot path has no CPU fallback: host tensors raise the package's error, with or without a GPU in the machine"""
    scn = _scn()
    import _hip
    sz = lambda *v: torch.LongTensor(list(v))
    md = scn.Metadata(3)
    x, e = torch.zeros(4, 8), torch.zeros(0)
    geom = (sz(17, 15, 9), sz(8, 7, 4), sz(3, 3, 3), sz(2, 2, 2))
    S = scn.SCN
    calls = [lambda: S.MaxPooling_updateOutput(*geom, md, x, e.clone(), 0),
             lambda: S.MaxPooling_updateGradInput(*geom, md, x, e.clone(), x, x, 0),
             lambda: S.AveragePooling_updateOutput(*geom, md, x, e.clone(), 0),
             lambda: S.AveragePooling_updateGradInput(*geom, md, x, e.clone(), x, 0),
             lambda: S.UnPooling_updateOutput(geom[1], geom[0], geom[2], geom[3], md, x, e.clone(), 0),
             lambda: S.UnPooling_updateGradInput(geom[1], geom[0], geom[2], geom[3], md, x.clone(), x, 0)]
    for call in calls:
        with pytest.raises(_hip.AabrError):
            call()
    with pytest.raises(_hip.AabrError):
        scn.MaxPooling(3, 3, 2)(scn.SparseConvNetTensor(x, md, geom[0]))
