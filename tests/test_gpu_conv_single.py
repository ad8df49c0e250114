"""The single-rule convolution kernel (csrc/conv_single.hip, k_conv_single) against the wide kernel it replaces for rule
books with exactly one rule per output row: the C ABI called directly, `aabr_conv_forward_single` against
`aabr_conv_forward_wide_res` on the same inputs, weight packs and residual -- BIT-EQUAL outputs (one MFMA chain per output
element in the same K order, then + bias, + residual; k_conv_cs' tile adds it to an exact zero).  Identity books (filter
volume 1, forward and transposed form), a permuted one, a deconvolution book the library builds (filter 2, stride 2) with
an empty offset, one of exactly 16 pairs and one whose count is no multiple of 16; then the compiled FPN graph with the
route on and off."""
import numpy as np
import pytest
import torch

import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 15, 16, 17, 40, 70, 200, 1000)      # 1 .. 32 steps of 32 pairs: every tail length and the four-step loop


@pytest.fixture
def route_on():
    """the route on for every supported book, whatever its size"""
    _hip.set_knob("CONV_SINGLE", 1)
    _hip.set_knob("SINGLE_ROWS", 0)
    yield
    for k in ("CONV_SINGLE", "SINGLE_ROWS", "SINGLE_CHUNK"):
        _hip.set_knob(k)


def _p(t):
    return _hip.ptr(t)


def _streams(table, T=64):
    """(offset pairs, wide tile blocks) of a gather table [vol][V] (int32, device), built by the library"""
    lib = _hip.load()
    vol, V = table.shape
    nb = (V + 255) // 256
    c = torch.zeros((vol, nb * 256), dtype=torch.int32, device=DEV)
    c[:, :V] = (table >= 0).to(torch.int32)
    counts = c.view(vol, nb, 256).sum(2, dtype=torch.int32).contiguous()
    pairs = torch.empty(max(lib.aabr_offset_pairs_words(V, vol), 1), dtype=torch.int32, device=DEV)
    _hip.check(lib.aabr_build_offset_pairs(_p(table), _p(counts), V, vol, _p(pairs), _hip.stream()))
    blocks = torch.empty(max(lib.aabr_wide_blocks_words(V, vol, T), 1), dtype=torch.int32, device=DEV)
    _hip.check(lib.aabr_build_wide_blocks(_p(table), V, vol, T, _p(blocks), _hip.stream()))
    return pairs, blocks


def _both(table, rows_in, n_in, n_out, transposed, bias, residual, seed, T=64):
    """the two launches over `table`; returns (single's output, wide's output) or the single launch's refusal"""
    lib = _hip.load()
    vol, V = table.shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((rows_in, n_in), generator=g).to(DEV)
    # the weight as the layer holds it: [vol][nIn][nOut]; the transposed (input-gradient) launch reads W[k]^T
    W = torch.randn((vol, n_out, n_in) if transposed else (vol, n_in, n_out), generator=g).to(DEV)
    b = torch.randn(n_out, generator=g).to(DEV) if bias else None
    r = torch.randn((V, n_out), generator=g).to(DEV) if residual else None
    flags = 3 if transposed else 0
    wpack = torch.empty(lib.aabr_conv_wpack_floats(vol, n_in, n_out), dtype=torch.float32, device=DEV)
    pairs, blocks = _streams(table, T)
    got = torch.full((V, n_out), 7.0, device=DEV)
    _hip.check(lib.aabr_conv_pack_weights(_p(W), vol, n_in, n_out, 1 if transposed else 0, _p(wpack), _hip.stream()))
    rc = lib.aabr_conv_forward_single(_p(x), n_in, rows_in, _p(got), n_out, V, _p(pairs), vol, _p(b), flags, _p(wpack),
                                      _p(r), _hip.stream())
    if rc != 0:
        return lib.aabr_last_error().decode()
    assert lib.aabr_conv_last_variant().decode() == "k_conv_single<%d>" % (n_in // 32)
    want = torch.full((V, n_out), -7.0, device=DEV)
    _hip.check(lib.aabr_conv_forward_wide_res(_p(x), n_in, rows_in, _p(want), n_out, V, _p(blocks), T, vol, _p(b), flags & 3,
                                              _p(wpack), _p(r), _hip.stream()))
    assert lib.aabr_conv_last_variant().decode().startswith("k_conv_cs<")
    return got, want, x, W


@pytest.mark.parametrize("n_in,n_out", [(32, 128), (64, 128), (128, 128), (128, 32), (128, 64)])
def test_identity_books_equal_the_wide_kernel_bit_for_bit(route_on, n_in, n_out):
    seed = 0
    for V in ROWS:
        table = torch.arange(V, dtype=torch.int32, device=DEV).view(1, V)
        for transposed, bias, residual in ((0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 1, 1), (0, 1, 0),
                                           (1, 0, 0)):
            seed += 1
            out = _both(table, V, n_in, n_out, transposed, bias, residual, seed)
            if n_out % 64:
                assert isinstance(out, str) and "n_out must be a multiple of 64" in out, out
                continue
            got, want, x, W = out
            assert torch.equal(got, want), (V, transposed, bias, residual, float((got - want).abs().max()))
            if not bias and not residual:      # and it is the product it claims to be
                w = W[0].double().t() if transposed else W[0].double()
                ref = x.double() @ w           # an fp32 chain of n_in terms: n_in roundings of at most 2^-24 of sum |x||w|
                assert float((got.double() - ref).abs().max()) <= n_in * 2.0 ** -23 * float((x.double().abs() @ w.abs()).max())


def test_both_chunk_lengths_and_a_permuted_book(route_on):
    """1000 pairs in chunks of 256 (a partly filled last chunk, surplus workgroups) and in one chunk of 1024; the rows
    gathered in a random order (still one rule per output row)"""
    V = 1000
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV).view(1, V)
    for chunk in (256, 1024):
        _hip.set_knob("SINGLE_CHUNK", chunk)
        for table in (torch.arange(V, dtype=torch.int32, device=DEV).view(1, V), perm):
            got, want, _, _ = _both(table, V, 128, 128, 0, 1, 1, 11 + chunk)
            assert torch.equal(got, want), chunk


def _deconv_book():
    """a filter 2 / stride 2 rule book built by the library from 300 random coarse sites whose children are chosen so
    that one filter offset has no pair, one exactly 16 and one a count that is no multiple of 16"""
    import sparseconvnet as scn
    from sparseconvnet import SCN
    rng = np.random.default_rng(5)
    cells = rng.choice(16 * 16 * 16, 300, replace=False)
    coarse = np.stack([cells // 256, (cells // 16) % 16, cells % 16], 1)
    child = rng.random((300, 8)) < 0.5
    child[:, 0] = False                       # this child position: never
    child[:, 1] = False
    child[rng.choice(300, 16, replace=False), 1] = True       # exactly 16 times
    child[:, 2] = False
    child[rng.choice(300, 37, replace=False), 2] = True       # 37 times
    child[:, 7] |= ~child.any(1)              # every coarse site exists
    ci, k = np.nonzero(child)
    fine = coarse[ci] * 2 + np.stack([k // 4, (k // 2) % 2, k % 2], 1)
    coords = np.concatenate([fine, np.zeros((len(fine), 1), np.int64)], 1).astype(np.int64)
    feats = torch.zeros((len(fine), 32), device=DEV)
    x = scn.InputLayer(3, [32, 32, 32], mode=4)([torch.as_tensor(coords).to(DEV), feats])
    conv = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
    y = conv(x)
    tb = x.metadata.getRuleBook(x.spatial_size, y.spatial_size, conv.filter_size, conv.filter_stride)
    SCN.flush_geom()
    torch.cuda.synchronize()
    assert (tb.V_in, tb.V_out, tb.vol) == (len(fine), 300, 8)
    return tb.inn.table.view(8, tb.V_in), tb.V_out   # the deconvolution's gather: per fine row its coarse row, per offset


def test_deconvolution_book_equals_the_wide_kernel_bit_for_bit(route_on):
    table, rows_in = _deconv_book()
    counts = (table >= 0).sum(1).tolist()
    assert int((table >= 0).sum(0).min()) == int((table >= 0).sum(0).max()) == 1      # one rule per output row
    assert 0 in counts and 16 in counts and any(c % 16 for c in counts), counts
    for n_in, n_out, bias, residual in ((128, 128, 0, 1), (128, 128, 1, 0), (64, 128, 0, 0), (32, 64, 1, 1)):
        for T in (64, 128):
            got, want, x, W = _both(table, rows_in, n_in, n_out, 0, bias, residual, 23 + n_in + T, T)
            assert torch.equal(got, want), (n_in, n_out, bias, residual, T)
    # and through the module: a Deconvolution with filter == stride takes the route by itself
    import sparseconvnet as scn
    coords = torch.as_tensor(np.stack(np.unravel_index(np.arange(0, 4096, 7), (16, 16, 16)) + (np.zeros(586, np.int64),), 1))
    x = scn.InputLayer(3, [16, 16, 16], mode=4)([coords.to(DEV), torch.randn((586, 64), device=DEV)])
    down, up = scn.Convolution(3, 64, 128, 2, 2, False).to(DEV), scn.Deconvolution(3, 128, 64, 2, 2, False).to(DEV)
    with torch.no_grad():
        mid = down(x)
        a = up(mid).features.clone()
        assert _hip.load().aabr_conv_last_variant().decode() == "k_conv_single<4>"
        _hip.set_knob("CONV_SINGLE", 0)
        _hip.set_knob("CONV_WIDE", 1)          # (a book this small would otherwise go to the 64-row-tile kernels)
        try:
            b = up(mid).features.clone()
        finally:
            _hip.set_knob("CONV_WIDE")
        assert _hip.load().aabr_conv_last_variant().decode().startswith("k_conv_cs<")
    assert torch.equal(a, b)


def test_compiled_fpn_graph_is_bit_equal_with_the_route_on_and_off(route_on):
    """a small FPN through the compiled graph: maps, input gradient and parameter gradients equal between CONV_SINGLE = 1
    (every supported one-rule launch on k_conv_single, SINGLE_ROWS = 0) and = 0; the "on" lists hold the new record kind
    in both directions and not one add record more.  Both runs with CONV_WIDE = 1: the route replaces k_conv_cs launches
    (the default SINGLE_ROWS keeps it to books k_conv_cs serves), and at this scene's few rows the default dispatch would
    hand the "off" run's launches to the 64-row-tile kernels, whose waves split a row's channels -- another summation
    order, equal to k_conv_cs only to rounding."""
    import synth_scenes as S
    from sparseconvnet import planExecutor
    from test_cabi_and_host import default_fpn
    torch.manual_seed(6)
    net = default_fpn().to(DEV)
    net.compiled_graph = True
    state = {k: v.clone() for k, v in net.state_dict().items()}
    locs, feats = S.make_batch(2, 20000, 41, 20)
    l = torch.as_tensor(locs).to(DEV)

    def run(on):
        _hip.set_knob("CONV_SINGLE", on)
        _hip.set_knob("CONV_WIDE", 1)
        net.load_state_dict(state)
        net.train(True)
        net.zero_grad()
        f = torch.as_tensor(feats).to(DEV).requires_grad_(True)
        planExecutor.debug_kinds = kinds = []
        try:
            rpn, roi = net([l, f])
            w = [torch.linspace(0.5, 1.5, m.features.numel(), device=DEV).view_as(m.features) for m in rpn + roi]
            sum((m.features * wi).square().mean() for m, wi in zip(rpn + roi, w)).backward()
            torch.cuda.synchronize()
        finally:
            planExecutor.debug_kinds = None
            _hip.set_knob("CONV_WIDE")
        return ([m.features.detach().clone() for m in rpn + roi], f.grad.clone(),
                {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, kinds)

    on, off = run(1), run(0)
    print("maps: largest difference per map", [float((a - b).abs().max()) for a, b in zip(on[0], off[0])])
    for a, b in zip(on[0], off[0]):
        assert torch.equal(a, b)
    assert torch.equal(on[1], off[1])
    assert on[2].keys() == off[2].keys() and len(on[2]) > 100
    for n in on[2]:
        assert torch.equal(on[2][n], off[2][n]), n
    K_ADD, K_SINGLE = planExecutor.K_ADD, planExecutor.K_SINGLE
    assert [d for d, _ in on[3]] == [d for d, _ in off[3]] == ["fwd", "bwd"]
    for (d, k_on), (_, k_off) in zip(on[3], off[3]):
        assert K_SINGLE in k_on and K_SINGLE not in k_off, d
        assert k_on.count(K_ADD) <= k_off.count(K_ADD) and len(k_on) <= len(k_off), d
