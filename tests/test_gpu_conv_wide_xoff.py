"""The wide kernel's steps over a tile's block list (csrc/conv_wide.hip, k_conv_cs<.., XO>, knob WIDE_XOFF): a step takes
blocks (b, b + 1) of the compiled stream whatever their filter offsets, instead of never straddling an offset.  Same
stream, same tile, same LDS, and the SAME BITS: per output element the sum still runs offset ascending, each term one MFMA
chain from zero.  Every case runs the entry points as they are (knob CONV_WIDE = 1 so that a small book takes the wide
kernel; tile rows as that query answers, 64, and the 112 rows the 64-plane layers of a step run with) and holds
  * `out` with WIDE_XOFF on torch.equal to `out` with it off, on normal-distributed operands (any change of the sum order
    would show), the statistics buffers byte-equal, two runs the same bytes, the reported instance name the same;
  * on the integer operands of tests/conv_exact.py the result exactly the float64 sum, equal to the 64-row-tile route of
    csrc/conv.hip, the statistics the exact fp64 sums.
The submanifold book is chosen so that its stream, READ BACK from the device, holds every kind of step the new loop
distinguishes (asserted): two blocks of different offsets, two of different offsets that name the same local row (the
read-add-write hazard), two of one offset, an unpaired last block; and offsets of 0, 1, 2 and 3 blocks in some tile.
Books and operands come from tests/test_gpu_conv_exact.py and tests/conv_exact.py, unchanged."""
import numpy as np
import pytest
import torch

import _hip
import conv_exact as E
import oracle_lib as O
import test_gpu_conv_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SITES = 791                         # ~23 % of a 12^3 cube per sample, two samples; 7 tiles of 112 rows + 7 rows, 12 of 64 + 23
T_STEP = 112                        # rows per tile of the <= 64-channel fp32 layers (conv_wide_tiles.h wide_default_rows)
PLANES = [(32, 64), (64, 64), (64, 128)]
_cache = {}


@pytest.fixture
def knobs(request):
    X._knobs(request, CONV_WIDE=1)
    request.addfinalizer(lambda: (_hip.set_knob("WIDE_XOFF", None), _hip.set_knob("WIDE_ROWS", None)))


def _tile_rows(bk, n_in, n_out):
    """(what the dispatch query answers for this small book, the tile of a step's 64-plane layers)"""
    lib = _hip.load()
    small = lib.aabr_conv_wide_tile_rows(n_in, n_out, bk.rows_in, bk.V_out, bk.vol)
    _hip.set_knob("WIDE_ROWS", T_STEP)
    try:
        ship = lib.aabr_conv_wide_tile_rows(n_in, n_out, bk.rows_in, bk.V_out, bk.vol)
    finally:
        _hip.set_knob("WIDE_ROWS", None)
    assert small == 64 and ship == T_STEP
    assert bk.V_out % small and bk.V_out % ship, "the last tile must be partial"
    return small, ship


def _strided_books():
    """filter 2 / stride 2 over the sites of the submanifold book: the Convolution's gather and the Deconvolution's"""
    if "s2" not in _cache:
        import sparseconvnet as scn
        x, il = X._input(E.site_coords(SITES, 7 + SITES), [16, 16, 16])
        conv = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
        xs = scn.SparseConvNetTensor()
        xs.metadata, xs.spatial_size = x.metadata, x.spatial_size
        xs.features = torch.zeros((il["V"], 32), device=DEV)
        y = conv(xs)
        tb = x.metadata.getRuleBook(x.spatial_size, y.spatial_size, conv.filter_size, conv.filter_stride)
        X._flush()
        rb, oc = O.convolution_rules(il["coords"], [2] * 3, [2] * 3, [8] * 3)
        n, nc = il["V"], oc.shape[0]
        assert (tb.V_in, tb.V_out, tb.vol) == (n, nc, 8) and np.array_equal(y.get_spatial_locations().numpy(), oc)
        _cache["s2"] = (X.Book(tb.out.table.view(8, nc), rb, nc, n), X.Book(tb.inn.table.view(8, n), rb, n, nc, in_col=1))
    return _cache["s2"]


def _book(name):
    if name == "subm":
        return X.sub_book(SITES)
    return _strided_books()[0 if name == "down" else 1]


# ------------------------------------------------------------------------------------- the stream, read back
def _stream(bk, T):
    w = bk.wide_blocks(T).cpu().numpy()
    nt, vol = (bk.V_out + T - 1) // T, bk.vol
    pre = w[:nt * (vol + 1)].reshape(nt, vol + 1)
    ent = w[nt * (vol + 1):nt * (vol + 1) + nt * (T // 16) * vol * 16].reshape(nt, (T // 16) * vol, 16)
    return pre, ent


def _step_kinds(pre, ent):
    """counts of the steps (b, b + 1), b even, by kind, and the set of blocks-per-offset figures over all tiles"""
    kinds = {"different offsets": 0, "different offsets, shared row": 0, "one offset": 0, "unpaired": 0}
    per_offset = set()
    for t in range(pre.shape[0]):
        p = pre[t].astype(np.int64)
        nblk = int(p[-1])
        per_offset |= set(np.diff(p).tolist())
        off = np.searchsorted(p, np.arange(nblk), side="right") - 1      # the k with p[k] <= b < p[k + 1]
        assert all(p[off[b]] <= b < p[off[b] + 1] for b in range(nblk))
        rows = [set((e[e >= 0] & 255).tolist()) for e in ent[t, :nblk]]
        assert all(rows), "a block without a pair"
        for b in range(0, nblk, 2):
            if b + 1 == nblk:
                kinds["unpaired"] += 1
            elif off[b] == off[b + 1]:
                assert not rows[b] & rows[b + 1], "two blocks of one offset never share an output row"
                kinds["one offset"] += 1
            else:
                kinds["different offsets"] += 1
                kinds["different offsets, shared row"] += bool(rows[b] & rows[b + 1])
    return kinds, per_offset


# ------------------------------------------------------------------------------------------------ the launches
def _normal(op, seed):
    """operands of the shapes of `op`, normal-distributed: sums that depend on their order"""
    rng = np.random.default_rng(seed)
    return {k: X._t(rng.standard_normal(np.shape(getattr(op, k))).astype(np.float32)) for k in ("x", "W", "bias", "residual")}


def _bn(bk, n_out, leak):
    x, mean, invstd, gam, bet, o = X._bn_operands(bk.V_out, n_out, 3 + bk.V_out, False)
    return (x, mean, o), (X._t(E.f32(x)), X._t(E.f32(mean)), X._t(E.f32(invstd)), X._t(E.f32(gam)), X._t(E.f32(bet)), leak)


def _run(bk, t, flags, bias, res, T, mode, bn, xoff):
    _hip.set_knob("WIDE_XOFF", xoff)
    out, stats = X.run_wide(bk, t["x"], t["W"], t["bias"] if bias else None, t["residual"] if res else None, flags, False,
                            T=T, mode=mode, bn=bn)
    name = X._ran(prefix="k_conv_cs<")
    torch.cuda.synchronize()
    return out, stats, name


def _same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _forms(bk):
    """(name, flags, residual, mode): forward, flipped (the input gradient; a book that is its own mirror), with a
    residual, with the following BatchNorm's forward parts, with the backward parts of the BatchNorm ahead"""
    f = [("forward", 0, 0, "res"), ("residual", 0, 1, "res"), ("bn forward", 0, 0, "stats"),
         ("bn backward", 3 if bk.mirrored else 0, 0, "bwd")]
    return f + ([("flipped", 3, 0, "res")] if bk.mirrored else [])


@pytest.mark.parametrize("n_in,n_out", PLANES)
@pytest.mark.parametrize("book", ["subm", "down", "up"])
def test_steps_across_offsets_write_the_same_bits(knobs, book, n_in, n_out):
    bk = _book(book)
    tiles = _tile_rows(bk, n_in, n_out)
    if book == "subm":
        kinds, per_offset = _step_kinds(*_stream(bk, T_STEP))
        assert all(v > 0 for v in kinds.values()), kinds
        assert {0, 1, 2, 3} <= per_offset, per_offset
        assert all(v > 0 for v in _step_kinds(*_stream(bk, tiles[0]))[0].values())
    leak = 0.25
    for form, flags, res, mode in _forms(bk):
        (bx, bmean, bo), bn = _bn(bk, n_out, leak) if mode == "bwd" else ((None, None, None), None)
        for bias in (0, 1):
            op, acc, _ = X._operands(bk, n_in, n_out, flags, 1)
            t = _normal(op, 100 + flags + 2 * bias)
            for T in tiles:
                what = "%s %s bias %d T %d" % (book, form, bias, T)
                on, s_on, name_on = _run(bk, t, flags, bias, res, T, mode, bn, 1)
                off, s_off, name_off = _run(bk, t, flags, bias, res, T, mode, bn, 0)
                again, s_again, _ = _run(bk, t, flags, bias, res, T, mode, bn, 1)
                assert name_on == name_off, (name_on, name_off)
                assert bool(torch.isfinite(on).all()), what
                assert torch.equal(on, off), "%s: %d elements differ with WIDE_XOFF on and off" % (what, int((on != off).sum()))
                assert _same_bytes(s_on, s_off), what + ": statistics differ with WIDE_XOFF on and off"
                assert _same_bytes(on, again) and _same_bytes(s_on, s_again), what + ": two runs differ"
                # exact operands: the float64 sum's bits, knob on (check_exact asserts them); the 64-row-tile route the same
                _hip.set_knob("WIDE_XOFF", 1)
                kw = {"bn": bn} if mode == "bwd" else {}
                opx, stored, stats = X.check_exact("wide xoff", X.run_wide, bk, n_in, n_out, flags, bias, res, False,
                                                   prefix="k_conv_cs<", T=T, mode=mode, **kw)
                if mode == "stats":
                    E.require_exact_stats(stored, opx.col, T)
                    E.assert_bits(stats.cpu().numpy(), E.tile_stats(stored, T), what=what + " statistics")
                elif mode == "bwd":
                    want, mag = X._bwd_stats_want(stored, bx, bmean, bo, leak, T)
                    assert (mag / (opx.col / 4)).max() < E.FP64_LIMIT
                    E.assert_bits(stats.cpu().numpy(), want, what=what + " backward statistics")
                elif not res:
                    X.check_exact("tiles", X.run_tiles, bk, n_in, n_out, flags, bias, 0, False)
