"""Every sparse-convolution kernel family held to the exact-arithmetic yardstick of tests/conv_exact.py, with ZERO
tolerance: on integer-valued operands (features m * 2^a, weights / bias / residual integers times a per-output-column
power of two; the precondition "all |terms| of a sum < 2^24 granules" asserted before every launch) each kernel's output
must be the float64 reference's bits -- in fp32 storage the exact sum, in bf16 storage ITS round-to-nearest-even bf16
(with a residual: the documented two roundings), statistics exactly the fp64 sums of the stored values -- and a non-finite
input row must reach exactly the outputs a rule connects it to (the rules-only property: padding entries of the tile,
wide, pair-list and table formats never leak a row).  The C ABI is called directly (reference: SCN/CPU/Convolution.cpp:
46-185, Deconvolution.cpp:7-77 through the oracle's rule books); every case asserts the kernel instance that ran, and the
last test checks that the names seen cover the launch tables of csrc/conv.hip, csrc/conv_dw.hip and csrc/conv_wide.hip."""
import numpy as np
import pytest
import torch

import _hip
import conv_dw_rule as RD
import conv_exact as E
import conv_tiles_rule as R
import conv_wide_rule as RW
import oracle_lib as O
import test_gpu_conv_tiles as TT
import test_gpu_conv_wide as TW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 17, 129, 700)            # sites of the forward-form rule books: below one 16-row group, ragged, three tiles, ~11
SEEN = set()                        # kernel instances the cases of this file ran
LARGEST = {}                        # per family: the largest sum |x||w| / granule the precondition saw
_cache = {}
TILE_INSTANCES = [k for k in R.compiled_instances() if R.KINDS[k[0]] != "generic"]
DW_INSTANCES = RD.compiled_instances()


def _p(t):
    return _hip.ptr(t)


def _t(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _lib():
    return _hip.load()


def _ran(expect=None, prefix=None):
    v = _lib().aabr_conv_last_variant().decode()
    if expect is not None:
        assert v == expect, (v, expect)
    if prefix is not None:
        assert v.startswith(prefix), (v, prefix)
    SEEN.add(v)
    return v


def _knobs(request, **kn):
    for k, v in kn.items():
        _hip.set_knob(k, v)
        request.addfinalizer(lambda k=k: _hip.set_knob(k, None))


def _note(family, largest):
    LARGEST[family] = max(LARGEST.get(family, 0.0), largest)


# ------------------------------------------------------------------------------------------------------ rule books
class Book(object):
    """a gather table of the library [vol, V_out] (device), the oracle's rule book it must equal, and its streams"""
    serial = 0

    def __init__(self, table, rb, V_out, rows_in, in_col=0, mirrored=False):
        self.table, self.rb, self.V_out, self.rows_in, self.in_col, self.mirrored = table, rb, V_out, rows_in, in_col, mirrored
        self.vol = rb.vol
        self._s = {}
        Book.serial += 1
        self.key = Book.serial
        want = E.gather_table(rb, V_out, in_col)
        assert np.array_equal(table.cpu().numpy().reshape(self.vol, V_out), want), "device and oracle rule books differ"
        self.nrules = E.rules_per_row(rb, V_out, in_col)

    def tile_blocks(self):
        if "tile" not in self._s:
            lib = _lib()
            w = torch.empty(max(lib.aabr_tile_blocks_words(self.V_out, self.vol), 1), dtype=torch.int32, device=DEV)
            _hip.check(lib.aabr_build_tile_blocks(_p(self.table), self.V_out, self.vol, _p(w), _hip.stream()))
            self._s["tile"] = w
        return self._s["tile"]

    def wide_blocks(self, T):
        if ("wide", T) not in self._s:
            lib = _lib()
            w = torch.empty(max(lib.aabr_wide_blocks_words(self.V_out, self.vol, T), 1), dtype=torch.int32, device=DEV)
            _hip.check(lib.aabr_build_wide_blocks(_p(self.table), self.V_out, self.vol, T, _p(w), _hip.stream()))
            self._s[("wide", T)] = w
        return self._s[("wide", T)]

    def pairs(self):
        """offset-major pair lists (tests/test_gpu_conv_single.py::_streams)"""
        if "pairs" not in self._s:
            lib = _lib()
            V, vol = self.V_out, self.vol
            nb = (V + 255) // 256
            c = torch.zeros((vol, nb * 256), dtype=torch.int32, device=DEV)
            c[:, :V] = (self.table.view(vol, V) >= 0).to(torch.int32)
            counts = c.view(vol, nb, 256).sum(2, dtype=torch.int32).contiguous()
            w = torch.empty(max(lib.aabr_offset_pairs_words(V, vol), 1), dtype=torch.int32, device=DEV)
            _hip.check(lib.aabr_build_offset_pairs(_p(self.table), _p(counts), V, vol, _p(w), _hip.stream()))
            self._s["pairs"] = w
        return self._s["pairs"]


def _flush():
    from sparseconvnet import SCN
    SCN.flush_geom()
    torch.cuda.synchronize()


def _input(coords, spatial):
    """the input layer's sites on the device and in the oracle, in the same row order"""
    import sparseconvnet as scn
    n = coords.shape[0]
    zeros = np.zeros((n, 1), np.float32)
    x = scn.InputLayer(3, spatial, mode=4)([_t(coords), _t(zeros)])
    il = O.input_layer(coords, zeros, 4)
    assert x.features.shape[0] == il["V"] == n
    assert np.array_equal(x.get_spatial_locations().numpy(), il["coords"])
    return x, il


def sub_book(n, fs=3):
    """3^3 (or 1^3) submanifold book of n sites drawn from a 12^3 cube, batch of 2"""
    if ("sub", n, fs) not in _cache:
        x, il = _input(E.site_coords(n, 7 + n), [16, 16, 16])
        tb = x.metadata.getSubmanifoldRuleBook(x.spatial_size, torch.LongTensor([fs] * 3))
        _flush()
        rb = O.submanifold_rules(il["coords"], [fs] * 3)
        assert (tb.V_out, tb.vol) == (n, fs ** 3)
        bk = Book(tb.out.table.view(tb.vol, n), rb, n, n, mirrored=True)
        bk.x = x
        _cache[("sub", n, fs)] = bk
    return _cache[("sub", n, fs)]


def _stride2_coords():
    """fine sites of 300 random coarse sites (tests/test_gpu_conv_single.py::_deconv_book: one child position never
    taken, one 16 times, one 37 times)"""
    rng = np.random.default_rng(5)
    cells = rng.choice(16 * 16 * 16, 300, replace=False)
    coarse = np.stack([cells // 256, (cells // 16) % 16, cells % 16], 1)
    child = rng.random((300, 8)) < 0.5
    child[:, 0] = False
    child[:, 1] = False
    child[rng.choice(300, 16, replace=False), 1] = True
    child[:, 2] = False
    child[rng.choice(300, 37, replace=False), 2] = True
    child[:, 7] |= ~child.any(1)
    ci, k = np.nonzero(child)
    fine = coarse[ci] * 2 + np.stack([k // 4, (k // 2) % 2, k % 2], 1)
    return np.concatenate([fine, np.zeros((len(fine), 1), np.int64)], 1).astype(np.int64)


def stride2_books():
    """filter 2 / stride 2 over 300 coarse sites: (the Convolution's gather: per coarse row its fine rows; the
    Deconvolution's: per fine row its one coarse row), the tensor they were built for"""
    if "s2" not in _cache:
        import sparseconvnet as scn
        x, il = _input(_stride2_coords(), [32, 32, 32])
        conv = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
        xs = scn.SparseConvNetTensor()
        xs.metadata, xs.spatial_size = x.metadata, x.spatial_size
        xs.features = torch.zeros((il["V"], 32), device=DEV)
        y = conv(xs)
        tb = x.metadata.getRuleBook(x.spatial_size, y.spatial_size, conv.filter_size, conv.filter_stride)
        _flush()
        rb, oc = O.convolution_rules(il["coords"], [2] * 3, [2] * 3, [16] * 3)
        n = il["V"]
        assert (tb.V_in, tb.V_out, tb.vol, oc.shape[0]) == (n, 300, 8, 300)
        assert np.array_equal(y.get_spatial_locations().numpy(), oc)
        down = Book(tb.out.table.view(8, 300), rb, 300, n)
        up = Book(tb.inn.table.view(8, n), rb, n, 300, in_col=1)
        assert int(up.nrules.min()) == int(up.nrules.max()) == 1 and 0 in rb.counts and 16 in rb.counts
        _cache["s2"] = (down, up, x)
    return _cache["s2"]


def perm_book(V):
    """one offset, every output row one rule into a random other row (rules written by hand: no geometry has them)"""
    if ("perm", V) not in _cache:
        perm = np.random.default_rng(3).permutation(V).astype(np.int32)
        rules = np.zeros((1, V, 2), np.int32)
        rules[0, :, 0], rules[0, :, 1] = perm, np.arange(V)
        _cache[("perm", V)] = Book(_t(perm).view(1, V), O.Rules(rules, np.array([V], np.int64), V), V, V)
    return _cache[("perm", V)]


def tiles_book(name):
    """the rule books of tests/test_gpu_conv_tiles.py (its `large` one reaches the instances of >= 512 workgroups)"""
    if ("tiles", name) not in _cache:
        ga, rb = TT._book(name)
        _flush()
        _cache[("tiles", name)] = Book(ga.table.view(ga.vol, ga.rows), rb, ga.rows, ga.rows, mirrored=True)
    return _cache[("tiles", name)]


# ------------------------------------------------------------------------------------------------------- launches
def _dims(W, flags):
    return (W.shape[2], W.shape[1]) if flags & 1 else (W.shape[1], W.shape[2])


def _out(bk, n_out, bf):
    return torch.full((bk.V_out, n_out), float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device=DEV)


def _pack(bk, W, flags, bf):
    lib = _lib()
    n_in, n_out = _dims(W, flags)
    if bf:
        n = int(lib.aabr_conv_wpack_bf16_elems(bk.vol, W.shape[1], W.shape[2]))
        pf, pt = (torch.empty(n, dtype=torch.bfloat16, device=DEV) for _ in range(2))
        _hip.check(lib.aabr_conv_pack_weights2_bf16(_p(W), bk.vol, W.shape[1], W.shape[2], _p(pf), _p(pt), _hip.stream()))
        return pt if flags & 1 else pf
    wp = torch.empty(int(lib.aabr_conv_wpack_floats(bk.vol, n_in, n_out)), device=DEV)
    _hip.check(lib.aabr_conv_pack_weights(_p(W), bk.vol, n_in, n_out, flags & 1, _p(wp), _hip.stream()))
    return wp


def run_tiles(bk, x, W, b, r, flags, bf):
    assert r is None
    lib = _lib()
    n_in, n_out = _dims(W, flags)
    out = _out(bk, n_out, bf)
    if bf:
        wp = torch.empty(int(lib.aabr_conv_wpack_bf16_elems(bk.vol, n_in, n_out)), dtype=torch.bfloat16, device=DEV)
        fn = lib.aabr_conv_forward_bf16
    else:
        wp = torch.empty(int(lib.aabr_conv_wpack_floats(bk.vol, n_in, n_out)), device=DEV)
        fn = lib.aabr_conv_forward
    _hip.check(fn(_p(x), n_in, bk.rows_in, _p(out), n_out, bk.V_out, _p(bk.tile_blocks()), bk.vol, _p(W), _p(b), flags,
                  _p(wp), _hip.stream()))
    return out, None


def run_wide(bk, x, W, b, r, flags, bf, T=64, mode="res", bn=None):
    """mode "res": aabr_conv_forward_wide_res / _bf16_res; "stats": _wide_stats / _bf16_stats; "bwd": _wide_bwd_stats /
    _bf16_bwd_stats with bn = (x, mean, invstd, weight, bias, leak) resp. (x, out, mean, leak)"""
    lib = _lib()
    n_in, n_out = _dims(W, flags)
    out, wp, blocks = _out(bk, n_out, bf), _pack(bk, W, flags, bf), bk.wide_blocks(T)
    a = (_p(x), n_in, bk.rows_in, _p(out), n_out, bk.V_out, _p(blocks), T, bk.vol, _p(b), flags, _p(wp))
    ntile = (bk.V_out + T - 1) // T
    stats = None
    if mode != "res":
        assert lib.aabr_conv_wide_stats_doubles(bk.V_out, T, n_out) == ntile * 2 * n_out
        stats = torch.full((ntile, 2, n_out), float("nan"), dtype=torch.float64, device=DEV)
    st = _hip.stream()
    if mode == "res":
        if bf:
            _hip.check(lib.aabr_conv_forward_wide_bf16_res(*a, _p(r), None, None, None, None, 0.0, st))
        else:
            _hip.check(lib.aabr_conv_forward_wide_res(*a, _p(r), st))
    elif mode == "stats":
        if bf:
            assert r is None
            _hip.check(lib.aabr_conv_forward_wide_bf16_stats(*a, _p(stats), st))
        else:
            _hip.check(lib.aabr_conv_forward_wide_stats(*a, _p(r), _p(stats), st))
    elif bf:
        assert r is None
        bx, bo, mean, leak = bn
        _hip.check(lib.aabr_conv_forward_wide_bf16_bwd_stats(*a, _p(stats), _p(bx), _p(bo), _p(mean), leak, st))
    else:
        bx, mean, invstd, gam, bet, leak = bn
        _hip.check(lib.aabr_conv_forward_wide_bwd_stats(*a, _p(r), _p(stats), _p(bx), _p(mean), _p(invstd), _p(gam), _p(bet),
                                                        leak, st))
    return out, stats


def run_split(bk, x, W, b, r, flags, bf, parts=2, T=64, plain=False):
    """aabr_conv_forward_wide_split / _split_bf16_res (plain: _split_bf16); the scratch starts as NaN: every part
    writes its whole partial tile"""
    lib = _lib()
    n_in, n_out = _dims(W, flags)
    out, wp, blocks = _out(bk, n_out, bf), _pack(bk, W, flags, bf), bk.wide_blocks(T)
    scratch = torch.full((int(lib.aabr_conv_wide_split_scratch_floats(bk.V_out, n_out, parts)),), float("nan"), device=DEV)
    a = (_p(x), n_in, bk.rows_in, _p(out), n_out, bk.V_out, _p(blocks), T, bk.vol, _p(b), flags, _p(wp))
    if not bf:
        _hip.check(lib.aabr_conv_forward_wide_split(*a, _p(r), parts, _p(scratch), _hip.stream()))
    elif plain:
        assert r is None
        _hip.check(lib.aabr_conv_forward_wide_split_bf16(*a, parts, _p(scratch), _hip.stream()))
    else:
        _hip.check(lib.aabr_conv_forward_wide_split_bf16_res(*a, parts, _p(scratch), _p(r), _hip.stream()))
    return out, None


def run_narrow(bk, x, W, b, r, flags, bf, mode="plain", bn=None):
    assert r is None and W.shape[1:] == (32, 32)
    lib = _lib()
    out = _out(bk, 32, bf)
    a = (_p(x), bk.rows_in, _p(out), bk.V_out, _p(bk.table), bk.vol, _p(W), _p(b), flags)
    stats = None
    if mode != "plain":
        nparts = int(lib.aabr_conv_narrow_parts(bk.V_out))
        assert bf and nparts == (bk.V_out + 255) // 256          # workgroup j sums the rows [256 j, 256 (j + 1))
        stats = torch.full((nparts, 2, 32), float("nan"), dtype=torch.float64, device=DEV)
    if mode == "plain":
        _hip.check((lib.aabr_conv_forward_narrow_bf16 if bf else lib.aabr_conv_forward_narrow)(*a, _hip.stream()))
    elif mode == "stats":
        _hip.check(lib.aabr_conv_forward_narrow_bf16_stats(*a, _p(stats), _hip.stream()))
    else:
        bx, bo, mean, leak = bn
        _hip.check(lib.aabr_conv_forward_narrow_bf16_bwd_stats(*a, _p(stats), _p(bx), _p(bo), _p(mean), leak, _hip.stream()))
    return out, stats


def run_single(bk, x, W, b, r, flags, bf):
    assert not bf
    lib = _lib()
    n_in, n_out = _dims(W, flags)
    out, wp = _out(bk, n_out, False), _pack(bk, W, flags, False)
    _hip.check(lib.aabr_conv_forward_single(_p(x), n_in, bk.rows_in, _p(out), n_out, bk.V_out, _p(bk.pairs()), bk.vol, _p(b),
                                            flags, _p(wp), _p(r), _hip.stream()))
    return out, None


# ------------------------------------------------------------------------------------------------ the two properties
def _reference(bk, op, flags, bias):
    """float64 acc (+ bias) of the launch from the oracle's rule book"""
    if flags & 1:
        assert flags == 3 and bk.mirrored and op.transposed
        acc = E.ref_input_grad(op.x, op.W, bk.rb, bk.V_out, bk.in_col)
    else:
        acc = E.ref_forward(op.x, op.W, bk.rb, bk.V_out, in_col=bk.in_col)
    return acc + op.bias if bias else acc


def _operands(bk, n_in, n_out, flags, seed):
    k = ("op", bk.key, n_in, n_out, flags, seed)
    if k not in _cache:
        op = E.operands(seed, bk.rows_in, bk.V_out, bk.vol, n_in, n_out, transposed=bool(flags & 1))
        largest = E.require_exact_forward(op, bk.rb, bk.V_out, in_col=bk.in_col)     # (with bias and residual: the most)
        _cache[k] = (op, _reference(bk, op, flags, False), largest)
    return _cache[k]


def check_exact(family, run, bk, n_in, n_out, flags, bias, res, bf, seed=1, variant=None, prefix=None, **kw):
    """one launch on exact operands against the reference's bits; returns (operands, stored output, statistics)"""
    op, acc, largest = _operands(bk, n_in, n_out, flags, seed)
    _note(family, largest)
    dt = torch.bfloat16 if bf else torch.float32
    out, stats = run(bk, _t(E.f32(op.x), dt), _t(E.f32(op.W)), _t(E.f32(op.bias)) if bias else None,
                     _t(E.f32(op.residual), dt) if res else None, flags, bf, **kw)
    _ran(variant, prefix)
    ab = acc + op.bias if bias else acc
    what = "%s %s flags %d bias %d residual %d %d->%d V %d %s" % (family, "bf16" if bf else "fp32", flags, bias, res, n_in,
                                                                n_out, bk.V_out, {k: v for k, v in kw.items() if k != "bn"})
    if bf:
        want = E.expect_bf16(ab, op.residual if res else None)
        E.assert_bits(out, want, exact=None if res else E.to_f32_exact(ab), rules=bk.nrules, what=what)
        stored = E.bf16_value(want).astype(np.float64)
    else:
        want = E.to_f32_exact(ab + op.residual if res else ab)
        E.assert_bits(out.cpu().numpy(), want, rules=bk.nrules, what=what)
        stored = want.astype(np.float64)
    return op, stored, stats


def _poisons(bk, n_in):
    """[(input rows poisoned, {row: (channel or None, value)})]: row 0 and the last row with a NaN in one channel, then a
    seeded 3 % of the rows holding NaN, +inf or -inf in the whole row or in one channel"""
    rng = np.random.default_rng(11)
    last = bk.rows_in - 1
    cases = [{0: (3, np.nan)}, {last: (n_in - 1, np.nan)}]
    n = max(1, (3 * bk.rows_in + 99) // 100)
    rows = rng.choice(bk.rows_in, n, replace=False)
    vals = (np.nan, np.inf, -np.inf)
    cases.append({int(r): (None if rng.random() < 0.5 else int(rng.integers(n_in)), vals[int(rng.integers(3))]) for r in rows})
    return cases[:1] + cases[2:] if last == 0 else cases


def _affected(bk, poisoned):
    """output rows with a rule into a poisoned input row, from the oracle's rule book"""
    hit = np.zeros(bk.V_out, bool)
    bad = np.zeros(bk.rows_in, bool)
    bad[list(poisoned)] = True
    for k in range(bk.vol):
        i, o = E.rule_pairs(bk.rb, k, bk.in_col)
        hit[o[bad[i]]] = True
    return hit


def check_rules_only(family, run, bk, n_in, n_out, flags, bias, res, bf, stats_T=None, prefix=None, **kw):
    """clean run against poisoned runs: the rows a rule connects to a poisoned row are non-finite in every column,
    every other element keeps its bits; statistics (stats_T rows per part) likewise per part"""
    op, acc, _ = _operands(bk, n_in, n_out, flags, 1)
    dt = torch.bfloat16 if bf else torch.float32
    W, b = _t(E.f32(op.W)), _t(E.f32(op.bias)) if bias else None
    r = _t(E.f32(op.residual), dt) if res else None
    clean, cstats = run(bk, _t(E.f32(op.x), dt), W, b, r, flags, bf, **kw)
    _ran(prefix=prefix)
    assert torch.isfinite(clean.float()).all()
    cb = E.bits(clean if bf else clean.cpu().numpy())
    # (flags 3 on a submanifold book: the launch's input rows are the layer's output rows -- the book is its own mirror)
    for poison in _poisons(bk, n_in):
        x = E.f32(op.x).copy()
        for row, (ch, val) in poison.items():
            if ch is None:
                x[row, :] = val
            else:
                x[row, ch] = val
        got, gstats = run(bk, _t(x, dt), W, b, r, flags, bf, **kw)
        hit = _affected(bk, poison)
        assert not bk.mirrored or hit[list(poison)].all()          # (a submanifold row has a rule to itself)
        g = got.float().cpu().numpy()
        fin = np.isfinite(g)
        assert not fin[hit].any(), "%s: %d finite elements in rows a rule connects to a poisoned row" % (
            family, int(fin[hit].sum()))
        gb = E.bits(got if bf else got.cpu().numpy())
        assert np.array_equal(gb[~hit], cb[~hit]), "%s: %d elements of rows WITHOUT a rule to a poisoned row changed; rows %s" % (
            family, int((gb[~hit] != cb[~hit]).sum()), np.nonzero((gb != cb).any(1) & ~hit)[0][:8])
        if stats_T:
            cs, gs = cstats.cpu().numpy(), gstats.cpu().numpy()
            thit = np.array([hit[j * stats_T:(j + 1) * stats_T].any() for j in range(cs.shape[0])])
            assert np.array_equal(E.bits(gs[~thit]), E.bits(cs[~thit]))
            assert not np.isfinite(gs[thit]).any()


def _flag_cases(bk, res_ok):
    """flags 0 and (mirrored books) 3, with and without bias, with residual where the entry takes one"""
    out = []
    for flags in (0, 3) if bk.mirrored else (0,):
        for bias, res in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if res_ok else ()):
            out.append((flags, bias, res))
    return out


# ------------------------------------------------------------------------------------------------- 64-row tiles
@pytest.mark.parametrize("inst", [R.name(k) for k in TILE_INSTANCES])
def test_tile_instance_is_exact(request, inst):
    """every 64-row-tile instance of csrc/conv.hip but the > 2 GiB generic one, at the first (book, planes, knobs) of
    tests/test_gpu_conv_tiles.py that reaches it"""
    key = next(k for k in TILE_INSTANCES if R.name(k) == inst)
    book, n_in, n_out, knobs = TT._config(key)
    bf = R.KINDS[key[0]] == "bf16"
    _knobs(request, **{k: knobs.get(k) for k in R.KNOBS})
    bk = tiles_book(book)
    for flags, bias, _ in _flag_cases(bk, False):
        want = TT._decide(bf, n_in, n_out, bk.V_out, bk.vol, flags, TT._sizes(n_in, n_out, bk.V_out, bk.vol, bf, False), knobs)
        assert want[:7] == key
        check_exact("tiles", run_tiles, bk, n_in, n_out, flags, bias, 0, bf, variant=inst)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", ROWS)
@pytest.mark.parametrize("n_in,n_out", [(32, 64), (64, 32), (96, 256)])
def test_tiles_every_row_count_default_knobs(V, n_in, n_out, bf):
    bk = sub_book(V)
    for flags, bias, _ in _flag_cases(bk, False):
        want = TT._decide(bf, n_in, n_out, V, bk.vol, flags, TT._sizes(n_in, n_out, V, bk.vol, bf, False), {})
        check_exact("tiles", run_tiles, bk, n_in, n_out, flags, bias, 0, bf, variant=R.name(want))


@pytest.mark.parametrize("bf", [False, True])
def test_tiles_strided_and_transposed_books(bf):
    down, up, _ = stride2_books()
    for bk in (down, up):
        for bias in (0, 1):
            check_exact("tiles", run_tiles, bk, 64, 96, 0, bias, 0, bf, prefix="k_conv_blocks_mfma")


# Output planes that are no multiple of 4 (the epilogue's scalar stores) together with a last column slab that is only
# partly filled: (book, bf16, planes in, planes out, knobs, the instance the rule decides, the generic instance the same
# shape reaches under flags 8 << 8).  bf16 needs plane counts that are multiples of 32: its last slab is short, its
# stores stay vectors.
GENERIC = 8 << 8        # steers the decision to the flat-pointer kernel; none of that kernel's dbg & 1 / 2 / 4 branches
RAGGED = [("large", False, 96, 198, {}, "k_conv_blocks_mfma_wpipe<4,3,true,false>", "k_conv_blocks_mfma<4,3,true>"),
          ("large", False, 96, 134, {}, "k_conv_blocks_mfma_buf<2,4,true,true>", "k_conv_blocks_mfma<2,4,true>"),
          ("large", False, 96, 70, {}, "k_conv_blocks_mfma_buf<1,4,true,true>", "k_conv_blocks_mfma<1,4,true>"),
          ("large", False, 9, 6, {}, "k_conv_blocks_mfma_buf<1,4,true,false>", "k_conv_blocks_mfma<1,4,false>"),
          ("large", False, 48, 198, {}, "k_conv_blocks_mfma_wlds<1,2,false>", "k_conv_blocks_mfma<4,3,false>"),
          ("large", False, 96, 6, {}, "k_conv_blocks_mfma_small<16>", None),
          ("large", True, 96, 160, {}, "k_conv_blocks_mfma_bf16<2,4,4,true>", None),
          ("large", True, 64, 416, {}, "k_conv_blocks_mfma_bf16<4,2,2,true>", None),
          ("small", False, 32, 134, {"CONV_WLDS": 2}, "k_conv_blocks_mfma_wlds<2,1,true>", None),
          ("small", False, 96, 70, {"SMALL_WPB": 8}, "k_conv_blocks_mfma_small<8>", None),
          ("small", False, 48, 198, {"CONV_WLDS": 0}, "k_conv_blocks_mfma_buf<1,4,true,false>", None)]


def run_tiles_generic(bk, x, W, b, r, flags, bf):
    return run_tiles(bk, x, W, b, r, flags | GENERIC, bf)


@pytest.mark.parametrize("book,bf,n_in,n_out,knobs,inst,generic", RAGGED,
                         ids=["%s-%s%d-%d" % (c[0], "bf16-" if c[1] else "", c[2], c[3]) for c in RAGGED])
def test_tiles_ragged_columns_are_exact(request, book, bf, n_in, n_out, knobs, inst, generic):
    """every kernel body's epilogue where co % 4 != 0 and / or the last column slab is partly filled, flags 0 and 3 with
    bias; the launches of one shape share their operands and reference"""
    _knobs(request, **{k: knobs.get(k) for k in R.KNOBS})
    bk = tiles_book(book)
    sizes = TT._sizes(n_in, n_out, bk.V_out, bk.vol, bf, False)
    for flags in (0, 3):
        assert R.name(TT._decide(bf, n_in, n_out, bk.V_out, bk.vol, flags, sizes, knobs)) == inst
        check_exact("tiles", run_tiles, bk, n_in, n_out, flags, 1, 0, bf, variant=inst)
        if generic:
            assert R.name(TT._decide(bf, n_in, n_out, bk.V_out, bk.vol, flags | GENERIC, sizes, knobs)) == generic
            check_exact("tiles", run_tiles_generic, bk, n_in, n_out, flags, 1, 0, bf, variant=generic)


# -------------------------------------------------------------------------------------------------------- wide
@pytest.mark.parametrize("T", [64, 128])
@pytest.mark.parametrize("kg,nbuf,bf,ncb,split", TW._instance_cases())
def test_wide_instance_is_exact(request, kg, nbuf, bf, ncb, split, T):
    """every k_conv_cs instance of the table (and the split launches that run them too), 700 rows in tiles of 64 and
    128 rows: aabr_conv_forward_wide_res / _bf16_res / _split / _split_bf16_res"""
    bk = sub_book(700)
    n_in, n_out = (64 if bf else 32) * kg, 128 if ncb == 2 else 64
    _knobs(request, **{"SPLIT_NBUF" if split else "WIDE_NBUF": nbuf, "WIDE_NCB": ncb})
    name = RW.name((kg, 0, nbuf, bf, ncb), bool(split))
    for flags, bias, res in _flag_cases(bk, True):
        if split:
            check_exact("split", run_split, bk, n_in, n_out, flags, bias, res, bool(bf), variant=name, parts=3, T=T)
        else:
            check_exact("wide", run_wide, bk, n_in, n_out, flags, bias, res, bool(bf), variant=name, T=T)


WIDE_SHAPES = [(False, 32, 64), (False, 64, 128), (False, 128, 64), (False, 256, 128), (True, 64, 128), (True, 128, 64),
               (True, 256, 128)]


@pytest.mark.parametrize("V", ROWS)
@pytest.mark.parametrize("bf,n_in,n_out", WIDE_SHAPES)
def test_wide_every_row_count(V, bf, n_in, n_out):
    bk = sub_book(V)
    for T in (64, 128):
        for flags, bias, res in _flag_cases(bk, True):
            check_exact("wide", run_wide, bk, n_in, n_out, flags, bias, res, bf, prefix="k_conv_cs<", T=T)


@pytest.mark.parametrize("bf", [False, True])
def test_wide_strided_and_transposed_books(bf):
    down, up, _ = stride2_books()
    for bk in (down, up):
        for bias, res in ((0, 0), (1, 1)):
            check_exact("wide", run_wide, bk, 128, 64, 0, bias, res, bf, prefix="k_conv_cs<", T=64)


@pytest.mark.parametrize("V", (129, 700))
@pytest.mark.parametrize("bf,n_in,n_out", [(False, 32, 64), (False, 128, 128), (True, 64, 128), (True, 128, 64)])
def test_wide_forward_statistics_are_exact(V, bf, n_in, n_out):
    """aabr_conv_forward_wide_stats / _bf16_stats: the stored bits, and per tile the exact fp64 sums of the stored values
    and of their squares"""
    bk = sub_book(V)
    for T in (64, 128):
        for flags, bias, res in ((0, 1, 0), (3, 0, 0)) + (() if bf else ((0, 1, 1),)):
            op, stored, stats = check_exact("wide stats", run_wide, bk, n_in, n_out, flags, bias, res, bf,
                                            prefix="k_conv_cs<", T=T, mode="stats")
            E.require_exact_stats(stored, op.col, T)
            E.assert_bits(stats.cpu().numpy(), E.tile_stats(stored, T), what="statistics T %d" % T)


@pytest.mark.parametrize("parts", [2, 5, 27])
@pytest.mark.parametrize("bf,n_in,n_out", [(False, 64, 64), (False, 128, 128), (False, 256, 64), (True, 64, 64),
                                           (True, 128, 128), (True, 256, 64)])
def test_offset_split_is_exact(request, parts, bf, n_in, n_out):
    """aabr_conv_forward_wide_split, _split_bf16 and _split_bf16_res at 2, 5 and vol parts (an offset range may be empty
    for a tile: its partial tile is zeros), every row count"""
    _knobs(request, SPLIT_MIN_ITEMS=1)
    split = ",split>"
    for V in ROWS:
        bk = sub_book(V)
        for flags, bias, res in _flag_cases(bk, True):
            check_exact("split", run_split, bk, n_in, n_out, flags, bias, res, bf, parts=parts)
            assert _ran().endswith(split)
            if bf and not res:
                check_exact("split", run_split, bk, n_in, n_out, flags, bias, 0, True, parts=parts, plain=True)
                assert _ran().endswith(split)


# ------------------------------------------------------------------------------------------------------ narrow
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", ROWS)
def test_narrow_is_exact(V, bf):
    bk = sub_book(V)
    for flags, bias, _ in _flag_cases(bk, False):
        check_exact("narrow", run_narrow, bk, 32, 32, flags, bias, 0, bf, variant="k_conv_narrow<bf16>" if bf else None,
                    prefix="k_conv_narrow<")
    if V == 700:
        down, up, _ = stride2_books()
        for b2 in (down, up):
            check_exact("narrow", run_narrow, b2, 32, 32, 0, 1, 0, bf, prefix="k_conv_narrow<")


@pytest.mark.parametrize("V", ROWS)
def test_narrow_forward_statistics_are_exact(V):
    bk = sub_book(V)
    for flags, bias in ((0, 1), (3, 0)):
        op, stored, stats = check_exact("narrow stats", run_narrow, bk, 32, 32, flags, bias, 0, True,
                                        variant="k_conv_narrow<bf16,stats>", mode="stats")
        E.require_exact_stats(stored, op.col, 256)
        E.assert_bits(stats.cpu().numpy(), E.tile_stats(stored, 256), what="narrow statistics")


# ------------------------------------------------------------------------------------------------- single rule
@pytest.mark.parametrize("chunk", [256, 1024])
@pytest.mark.parametrize("n_in,n_out", [(32, 64), (64, 128), (128, 128), (96, 64)])
def test_single_rule_kernel_is_exact(request, chunk, n_in, n_out):
    """aabr_conv_forward_single against the reference itself (elsewhere it is only held equal to k_conv_cs): identity
    books (filter volume 1; forward and transposed), a permuted book, the deconvolution book (an empty offset, one of 16
    pairs, one of 37)"""
    _knobs(request, SINGLE_CHUNK=chunk)
    name = "k_conv_single<%d>" % (n_in // 32)
    books = [sub_book(V, 1) for V in ROWS] + [perm_book(700), stride2_books()[1]]
    for bk in books:
        for flags, bias, res in _flag_cases(bk, True):
            check_exact("single", run_single, bk, n_in, n_out, flags, bias, res, False, variant=name)


def test_single_rule_kernel_refuses_what_it_documents():
    lib = _lib()
    bk = sub_book(129, 1)
    for n_in, n_out, why in ((128, 32, "n_out must be a multiple of 64"), (48, 64, "n_in must be a multiple of 32"),
                             (256, 64, "n_in <= 128")):
        x, out = torch.zeros((129, n_in), device=DEV), torch.zeros((129, n_out), device=DEV)
        wp = torch.zeros(int(lib.aabr_conv_wpack_floats(1, n_in, n_out)), device=DEV)
        rc = lib.aabr_conv_forward_single(_p(x), n_in, 129, _p(out), n_out, 129, _p(bk.pairs()), 1, None, 0, _p(wp), None,
                                          _hip.stream())
        assert rc != 0 and why in lib.aabr_last_error().decode()
        assert not out.any()


# ---------------------------------------------------------------------------------- backward-statistics write-outs
def _bn_operands(V, n, seed, bf):
    """a BatchNorm whose recomputed activation is exact: integer x and mean, invstd and weight powers of two (weight of
    either sign), integer bias"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (V, n)).astype(np.float64)
    mean = rng.integers(-2, 3, n).astype(np.float64)
    invstd = np.exp2(rng.integers(-2, 3, n))
    gam = np.exp2(rng.integers(-2, 3, n)) * rng.choice([-1.0, 1.0], n)
    bet = rng.integers(-3, 4, n).astype(np.float64)
    o = (x - mean) * invstd * gam + bet                       # exact in fp32 in any association: small integers / 16
    if bf:                                                    # bf16 storage reads the STORED activation's sign
        o = rng.integers(-3, 4, (V, n)).astype(np.float64)
    return x, mean, invstd, gam, bet, o


def _bwd_stats_want(stored, x, mean, o, leak, T):
    d = np.where(o > 0, stored, stored * leak)
    nt = (stored.shape[0] + T - 1) // T
    want = np.zeros((nt, 2, stored.shape[1]))
    mag = np.zeros(stored.shape[1])
    for j in range(nt):
        sl = slice(j * T, (j + 1) * T)
        want[j, 0], want[j, 1] = d[sl].sum(0), ((x[sl] - mean) * d[sl]).sum(0)
        mag = np.maximum(mag, np.maximum(np.abs(d[sl]).sum(0), (np.abs(x[sl] - mean) * np.abs(d[sl])).sum(0)))
    return want, mag


@pytest.mark.parametrize("leak", [0.0, 0.25])
@pytest.mark.parametrize("bf,n_in,n_out", [(False, 64, 64), (False, 128, 128), (True, 64, 128), (True, 128, 64)])
def test_wide_backward_statistics_are_exact(bf, n_in, n_out, leak):
    """aabr_conv_forward_wide_bwd_stats / _bf16_bwd_stats: the written d_out is the plain launch's bits, and per tile
    sum d and sum (x - mean) d with d = d_out or leak * d_out by the activation's sign are the exact fp64 sums.  Every
    operand of both entries can be made exact (fp32: the activation o = x * (invstd * weight) + (bias - mean * invstd *
    weight) is recomputed in fp32 from integers and powers of two; bf16: the sign is read from the stored activation)."""
    for V in (129, 700):
        bk = sub_book(V)
        x, mean, invstd, gam, bet, o = _bn_operands(V, n_out, 3 + V, bf)
        for T in (64, 128):
            for flags, res in ((3, 0), (0, 0)) + (() if bf else ((3, 1),)):
                if bf:
                    bn = (_t(E.f32(x), torch.bfloat16), _t(E.f32(o), torch.bfloat16), _t(E.f32(mean)), leak)
                else:
                    bn = (_t(E.f32(x)), _t(E.f32(mean)), _t(E.f32(invstd)), _t(E.f32(gam)), _t(E.f32(bet)), leak)
                op, stored, stats = check_exact("wide bwd stats", run_wide, bk, n_in, n_out, flags, 0, res, bf,
                                                prefix="k_conv_cs<", T=T, mode="bwd", bn=bn)
                want, mag = _bwd_stats_want(stored, x, mean, o, leak, T)
                assert (mag / (op.col / 4)).max() < E.FP64_LIMIT     # (granule: leak * column scale)
                E.assert_bits(stats.cpu().numpy(), want, what="backward statistics T %d" % T)
    # the affine-free form of the fp32 entry (weight and bias NULL)
    if not bf:
        o1 = (x - mean) * invstd
        bn = (_t(E.f32(x)), _t(E.f32(mean)), _t(E.f32(invstd)), None, None, leak)
        op, stored, stats = check_exact("wide bwd stats", run_wide, bk, n_in, n_out, 3, 0, 0, False, T=64, mode="bwd", bn=bn)
        E.assert_bits(stats.cpu().numpy(), _bwd_stats_want(stored, x, mean, o1, leak, 64)[0])


@pytest.mark.parametrize("leak", [0.0, 0.25])
@pytest.mark.parametrize("V", ROWS)
def test_narrow_backward_statistics_are_exact(V, leak):
    bk = sub_book(V)
    x, mean, _, _, _, o = _bn_operands(V, 32, 5 + V, True)
    bn = (_t(E.f32(x), torch.bfloat16), _t(E.f32(o), torch.bfloat16), _t(E.f32(mean)), leak)
    for flags in (3, 0):
        op, stored, stats = check_exact("narrow bwd stats", run_narrow, bk, 32, 32, flags, 0, 0, True,
                                        variant="k_conv_narrow<bf16,bwd_stats>", mode="bwd", bn=bn)
        want, mag = _bwd_stats_want(stored, x, mean, o, leak, 256)
        assert (mag / (op.col / 4)).max() < E.FP64_LIMIT     # (granule: leak * column scale)
        E.assert_bits(stats.cpu().numpy(), want, what="narrow backward statistics")


# -------------------------------------------------------------------------------------------------- weight gradient
def _dw_book(name):
    if name == "s2":
        return stride2_books()[0]
    return sub_book(int(name))


def _run_dw(bk, x, g, bf):
    """aabr_conv_backward_weight[_bf16] over the book's pair lists; max_chunks = the bound for rule counts unknown on
    the host, ceil(vol V / c) + vol"""
    lib = _lib()
    n_in, n_out = x.shape[1], g.shape[1]
    cp = lib.aabr_conv_dw_chunk_pairs(bk.V_out, bk.vol, n_in, n_out)
    mc = (bk.vol * bk.V_out + cp - 1) // cp + bk.vol
    scratch = torch.full((int(lib.aabr_conv_dw_scratch_floats(mc, n_in, n_out)),), float("nan"), device=DEV)
    dW = torch.full((bk.vol, n_in, n_out), float("nan"), device=DEV)
    db = torch.full((n_out,), float("nan"), device=DEV)
    fn = lib.aabr_conv_backward_weight_bf16 if bf else lib.aabr_conv_backward_weight
    _hip.check(fn(_p(x), n_in, _p(g), n_out, bk.V_out, _p(bk.pairs()), bk.vol, mc, _p(dW), _p(db), _p(scratch),
                  _hip.stream()))
    return dW, db, cp


# (book, planes in, planes out, chunk pairs, form): 17 sites leave most offsets without a rule, the stride-2 book one
DW_CASES = [("17", 64, 64, 256, "direct"), ("129", 64, 64, 256, "direct"), ("700", 64, 64, 256, "reduce"),
            ("s2", 32, 64, 256, "reduce"), ("700", 32, 32, 256, "reduce"), ("700", 128, 128, 1024, "direct"),
            ("700", 64, 128, 1024, "direct"), ("1500", 64, 128, 1024, "reduce"), ("1500", 96, 64, 1024, "reduce"),
            ("1500", 128, 128, 1024, "full"), ("1500", 256, 128, 1024, "full")]


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("book,n_in,n_out,chunk,form", DW_CASES)
def test_weight_gradient_is_exact(request, book, n_in, n_out, chunk, form, bf):
    """aabr_conv_backward_weight / _bf16 with d_bias: the 64 x 64-block kernels at 256- and 1024-pair chunks, direct
    (V <= chunk) and chunked + reduce, and the full-tile kernels (DW_FULL_MIN = 8; they need more rows than one
    1024-pair chunk, hence the 1500-site book); offsets without a rule are exact zeros (the reference's are +0.0)"""
    _knobs(request, DW_FULL_MIN=8)
    bk = _dw_book(book)
    rng = np.random.default_rng(n_in * 7 + n_out + bk.V_out)
    x, g = E.rows(rng, bk.rows_in, n_in), E.rows(rng, bk.V_out, n_out)
    _note("weight gradient", E.require_exact_weight_grad(x, g, bk.rb, bk.in_col))
    dt = torch.bfloat16 if bf else torch.float32
    dW, db, cp = _run_dw(bk, _t(E.f32(x), dt), _t(E.f32(g), dt), bf)
    v = _ran(prefix="k_conv_dw_")
    assert cp == chunk and (bk.V_out <= cp) == (form == "direct") and ("k_conv_dw_full" in v) == (form == "full"), (v, cp)
    rW, rb_ = E.ref_weight_grad(x, g, bk.rb, bk.in_col)
    assert any(int(c) == 0 for c in bk.rb.counts) or book not in ("17", "s2")
    E.assert_bits(dW.cpu().numpy(), E.to_f32_exact(rW), what="dW %s" % v)
    E.assert_bits(db.cpu().numpy(), E.to_f32_exact(rb_), what="d_bias")


# planes per side by blocks of 16 (cb / nb): the smallest that select the instance; the scalar bf16 kernel at counts
# that are no multiple of 32 (the MFMA form is not taken), none a multiple of 128 (nor is the full-tile path)
DW_PLANES = {("pairs", 0): {1: 16, 2: 32, 4: 64}, ("pairs", 1): {1: 16, 2: 48, 4: 80}, ("pairs_mfma", 1): {2: 32, 4: 64}}


def _dw_exact_operands(bk, n_in, n_out):
    """integer-valued rows and output gradients of one launch with the reference's dW and d_bias (float64), shared by
    the storage types and instances that use the shape"""
    k = ("dw", bk.key, n_in, n_out)
    if k not in _cache:
        rng = np.random.default_rng(n_in * 7 + n_out + bk.V_out)
        x, g = E.rows(rng, bk.rows_in, n_in), E.rows(rng, bk.V_out, n_out)
        largest = E.require_exact_weight_grad(x, g, bk.rb, bk.in_col)
        _cache[k] = (x, g, largest) + E.ref_weight_grad(x, g, bk.rb, bk.in_col)
    return _cache[k]


@pytest.mark.parametrize("inst", [RD.name(k) for k in DW_INSTANCES])
def test_weight_gradient_instance_is_exact(request, inst):
    """every row of the instance tables of csrc/conv_dw.hip through the C ABI with d_bias: the 64 x 64-block kernels
    direct (129 sites: V <= 256, the kernel writes dW) and chunked + reduce (1500 sites: V > 1024), the full-tile
    kernels at 128 -> 128 planes on the 1500-site book (DW_FULL_MIN = 8); the name reported is the row's, dW and d_bias
    are the reference's bits"""
    key = next(k for k in DW_INSTANCES if RD.name(k) == inst)
    kind, bf = RD.KINDS[key[0]], bool(key[1])
    knobs = {}
    if kind == "full":
        knobs = {"DW_FULL_MIN": 8}
        launches = [("1500", 128, 128, "ranges")]
    else:
        planes = DW_PLANES[(kind, key[1])]
        launches = [(book, planes[key[2]], planes[key[3]], reduce) for book, reduce in (("129", "none"), ("1500", "chunks"))]
    _knobs(request, **knobs)
    dt = torch.bfloat16 if bf else torch.float32
    for book, n_in, n_out, reduce in launches:
        bk = _dw_book(book)
        x, g, largest, rW, rb_ = _dw_exact_operands(bk, n_in, n_out)
        _note("weight gradient", largest)
        dW, db, cp = _run_dw(bk, _t(E.f32(x), dt), _t(E.f32(g), dt), bf)
        _ran(expect=inst)
        mc = (bk.vol * bk.V_out + cp - 1) // cp + bk.vol
        want = RD.decide(bf, n_in, n_out, bk.V_out, bk.vol, mc, True, tuple(knobs.get(k, RD.UNSET) for k in RD.KNOBS))
        assert want[:4] == key and RD.REDUCES[want[9]] == reduce and want[4] == cp, (want, key, reduce, cp)
        what = "%s %s %d->%d V %d" % (inst, reduce, n_in, n_out, bk.V_out)
        E.assert_bits(dW.cpu().numpy(), E.to_f32_exact(rW), what="dW " + what)
        E.assert_bits(db.cpu().numpy(), E.to_f32_exact(rb_), what="d_bias " + what)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("book,n_in,n_out", [("129", 64, 64), ("700", 64, 64), ("1500", 128, 128), ("1500", 64, 128)])
def test_weight_gradient_rules_only(request, book, n_in, n_out, bf):
    """a non-finite channel c of input row r: dW[k][c][:] is non-finite for exactly the offsets k at which r has a rule,
    everything else (and d_bias) keeps its bits"""
    _knobs(request, DW_FULL_MIN=8)
    bk = _dw_book(book)
    rng = np.random.default_rng(n_in + n_out)
    x, g = E.f32(E.rows(rng, bk.rows_in, n_in)), E.f32(E.rows(rng, bk.V_out, n_out))
    dt = torch.bfloat16 if bf else torch.float32
    gd = _t(g, dt)
    cW, cb_, _ = _run_dw(bk, _t(x, dt), gd, bf)
    _ran(prefix="k_conv_dw_")
    assert torch.isfinite(cW).all()
    for r, c, val in ((0, 5, np.nan), (bk.rows_in - 1, n_in - 1, np.inf), (bk.rows_in // 2, 0, -np.inf)):
        xp = x.copy()
        xp[r, c] = val
        dW, db, _ = _run_dw(bk, _t(xp, dt), gd, bf)
        hit = np.zeros((bk.vol, n_in), bool)
        for k in range(bk.vol):
            i, _o = E.rule_pairs(bk.rb, k, bk.in_col)
            hit[k, c] = bool((i == r).any())
        assert hit.any()
        got = dW.cpu().numpy()
        assert not np.isfinite(got[hit]).any()
        assert np.array_equal(E.bits(got)[~hit], E.bits(cW.cpu().numpy())[~hit])
        assert torch.equal(db, cb_)


# ------------------------------------------------------------------------------------------------ rules-only property
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", (129, 700))
def test_rules_only_tiles(V, bf):
    bk = sub_book(V)
    for n_in, n_out in ((32, 64), (96, 256)):
        for flags in (0, 3):
            check_rules_only("tiles", run_tiles, bk, n_in, n_out, flags, 1, 0, bf, prefix="k_conv_blocks_mfma")
    down, up, _ = stride2_books()
    for b2 in (down, up):
        check_rules_only("tiles", run_tiles, b2, 64, 96, 0, 0, 0, bf, prefix="k_conv_blocks_mfma")


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", (129, 700))
def test_rules_only_wide_and_its_statistics(V, bf):
    bk = sub_book(V)
    for n_in, n_out in ((64, 128), (128, 64)) + (() if bf else ((32, 64),)):
        for T in (64, 128):
            for flags in (0, 3):
                check_rules_only("wide", run_wide, bk, n_in, n_out, flags, 1, 1, bf, prefix="k_conv_cs<", T=T)
            check_rules_only("wide stats", run_wide, bk, n_in, n_out, 0, 1, 0, bf, stats_T=T, prefix="k_conv_cs<", T=T,
                             mode="stats")
    down, up, _ = stride2_books()
    for b2 in (down, up):
        check_rules_only("wide", run_wide, b2, 128, 64, 0, 0, 1, bf, prefix="k_conv_cs<", T=64)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", (129, 700))
def test_rules_only_offset_split(request, V, bf):
    _knobs(request, SPLIT_MIN_ITEMS=1)
    bk = sub_book(V)
    for parts in (2, 5, 27):
        for flags in (0, 3):
            check_rules_only("split", run_split, bk, 128, 64, flags, 1, 1, bf, parts=parts)
            assert _ran().endswith(",split>")


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("V", (17, 129, 700))
def test_rules_only_narrow_and_its_statistics(V, bf):
    bk = sub_book(V)
    for flags in (0, 3):
        check_rules_only("narrow", run_narrow, bk, 32, 32, flags, 1, 0, bf, prefix="k_conv_narrow<")
    if bf:
        check_rules_only("narrow stats", run_narrow, bk, 32, 32, 0, 1, 0, True, stats_T=256, prefix="k_conv_narrow<",
                         mode="stats")
    for b2 in stride2_books()[:2]:
        check_rules_only("narrow", run_narrow, b2, 32, 32, 0, 0, 0, bf, prefix="k_conv_narrow<")


@pytest.mark.parametrize("chunk", [256, 1024])
def test_rules_only_single(request, chunk):
    _knobs(request, SINGLE_CHUNK=chunk)
    for bk in (sub_book(129, 1), sub_book(700, 1), perm_book(700), stride2_books()[1]):
        for flags in (0, 3) if bk.mirrored else (0,):
            check_rules_only("single", run_single, bk, 64, 128, flags, 1, 1, False, prefix="k_conv_single<")


# ------------------------------------------------------------------------------------------------ through the layers
def _int_weights(layer, seed):
    rng = np.random.default_rng(seed)
    W = rng.integers(-4, 5, tuple(layer.weight.shape)).astype(np.float32)
    b = rng.integers(-4, 5, tuple(layer.bias.shape)).astype(np.float32)
    with torch.no_grad():
        layer.weight.copy_(_t(W))
        layer.bias.copy_(_t(b))
    vol = W.shape[0]
    return W.reshape(vol, W.shape[2], W.shape[3]).astype(np.float64), b.astype(np.float64)


def _layer_pass(layer, x_like, feats, grad, dt):
    import sparseconvnet as scn
    xs = scn.SparseConvNetTensor()
    xs.metadata, xs.spatial_size = x_like.metadata, x_like.spatial_size
    xs.features = _t(E.f32(feats), dt).requires_grad_(True)
    layer.zero_grad()
    y = layer(xs)
    fwd = _ran(prefix="k_conv")
    with torch.autograd.set_multithreading_enabled(False):       # (aabr_conv_last_variant is per thread)
        y.features.backward(_t(E.f32(grad), dt))
    _ran(prefix="k_conv")
    return y, xs.features.grad, layer.weight.grad, layer.bias.grad, fwd


def _check_layer(what, bk_fwd, W, b, feats, grad, y, d_in, dW, db, bf):
    """forward over bk_fwd's rules; the backward pass reads the same rules the other way round"""
    rb, ic = bk_fwd.rb, bk_fwd.in_col
    op = E.Operands(feats, W, b, np.zeros((bk_fwd.V_out, W.shape[2])), np.ones(W.shape[2]), False)
    _note("layers", E.require_exact_forward(op, rb, bk_fwd.V_out, residual=False, in_col=ic))
    ot = E.Operands(grad, W, None, None, np.ones(W.shape[1]), True)
    _note("layers", E.require_exact_forward(ot, rb, bk_fwd.rows_in, bias=False, residual=False, in_col=ic))
    _note("layers", E.require_exact_weight_grad(feats, grad, rb, ic))
    acc = E.ref_forward(feats, W, rb, bk_fwd.V_out, b, in_col=ic)
    gin = E.ref_input_grad(grad, W, rb, bk_fwd.rows_in, ic)
    rW, rdb = E.ref_weight_grad(feats, grad, rb, ic)
    if bf:
        E.assert_bits(y.features.detach(), E.expect_bf16(acc), exact=E.to_f32_exact(acc), what=what + " forward")
        E.assert_bits(d_in, E.expect_bf16(gin), exact=E.to_f32_exact(gin), what=what + " input gradient")
    else:
        E.assert_bits(y.features.detach().cpu().numpy(), E.to_f32_exact(acc), what=what + " forward")
        E.assert_bits(d_in.cpu().numpy(), E.to_f32_exact(gin), what=what + " input gradient")
    E.assert_bits(dW.float().cpu().numpy().reshape(rW.shape), E.to_f32_exact(rW), what=what + " dW")
    E.assert_bits(db.float().cpu().numpy(), E.to_f32_exact(rdb), what=what + " d_bias")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_in,n_out", [(64, 64), (32, 32), (128, 64)])
def test_layers_are_exact_under_default_dispatch(dt, n_in, n_out):
    """one autograd pass each of SubmanifoldConvolution, Convolution and Deconvolution with integer weights (no column
    scale: the input gradient sums over the output columns): forward, input gradient, dW and d_bias are the reference's
    bits, whatever kernels the default dispatch picks"""
    import sparseconvnet as scn
    bf = dt == torch.bfloat16
    rng = np.random.default_rng(n_in + 2 * n_out)
    sub = sub_book(700)
    down, up, x2 = stride2_books()
    cases = [("SubmanifoldConvolution", scn.SubmanifoldConvolution(3, n_in, n_out, 3, True), sub, sub.x),
             ("Convolution", scn.Convolution(3, n_in, n_out, 2, 2, True), down, x2)]
    for what, layer, bk, x_like in cases:
        layer = layer.to(DEV)
        W, b = _int_weights(layer, n_in)
        feats, grad = E.rows(rng, bk.rows_in, n_in), E.rows(rng, bk.V_out, n_out)
        y, d_in, dW, db, _ = _layer_pass(layer, x_like, feats, grad, dt)
        _check_layer(what, bk, W, b, feats, grad, y, d_in, dW, db, bf)
    # the Deconvolution reads the Convolution's output tensor: run the Convolution again for its metadata
    conv = scn.Convolution(3, n_in, n_out, 2, 2, False).to(DEV)
    xs = scn.SparseConvNetTensor()
    xs.metadata, xs.spatial_size = x2.metadata, x2.spatial_size
    xs.features = torch.zeros((down.rows_in, n_in), dtype=dt, device=DEV)
    with torch.no_grad():
        mid = conv(xs)
    dec = scn.Deconvolution(3, n_out, n_in, 2, 2, True).to(DEV)
    W, b = _int_weights(dec, n_out)
    feats, grad = E.rows(rng, up.rows_in, n_out), E.rows(rng, up.V_out, n_in)
    y, d_in, dW, db, fwd = _layer_pass(dec, mid, feats, grad, dt)
    _check_layer("Deconvolution", up, W, b, feats, grad, y, d_in, dW, db, bf)


# ---------------------------------------------------------------------------------------------------------- coverage
def test_zz_the_names_seen_cover_the_launch_tables():
    """reads only what the cases above collected (it runs last in this file): every 64-row-tile instance but the generic
    one, every k_conv_cs instance and split launch, the narrow forms, the single-rule kernel, every weight-gradient instance"""
    want = {R.name(k) for k in TILE_INSTANCES}
    want |= {RW.name(k) for k in RW.compiled_instances()} | {RW.name(k, True) for k in RW.split_instances()}
    want |= {"k_conv_narrow<bf16>", "k_conv_narrow<bf16,stats>", "k_conv_narrow<bf16,bwd_stats>", "k_conv_single<1>",
             "k_conv_single<2>", "k_conv_single<3>", "k_conv_single<4>"}
    want |= {RD.name(k) for k in DW_INSTANCES}
    print("largest sum |x||w| / granule per family:",
          {k: "2^%.2f" % np.log2(v) for k, v in sorted(LARGEST.items()) if v > 0})
    missing = sorted(want - SEEN)
    assert not missing, missing
    assert any(v.startswith("k_conv_narrow<") and "bf16" not in v for v in SEEN)
