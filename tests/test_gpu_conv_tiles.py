"""Every 64-row-tile kernel instance csrc/conv.hip compiles, launched through the C ABI (aabr_conv_forward /
aabr_conv_forward_bf16, bypassing SCN.conv_route) on real submanifold rule books, with the tuning knobs that reach
it: the instance the library reports must be the one csrc/conv_tiles.h decides (restated in
tests/conv_tiles_rule.py) and the output must match the oracle (SCN/CPU/Convolution.cpp:117-185), plain and in the
transposed + flipped input-gradient form.  The generic kernel (flat 64-bit addressing) runs on a table whose rows lie
in an input of more than 2 GiB, half of them beyond the 2 GiB mark."""
import itertools

import numpy as np
import pytest
import torch

import conv_tiles_rule as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# rule books: sites, cube edge the sites are drawn from, filter size
BOOKS = {"small": (700, 12, 3), "large": (9000, 40, 3), "one": (700, 12, 1)}
BIG_FLOATS = (1 << 29) + (1 << 20)                   # the generic kernel's input: 2 GiB + 4 MiB
KNOB_SETS = ([{}, {"CONV_WLDS": 2}, {"CONV_WLDS": 4}, {"SMALL_WPB": 8}] +
             [{"CONV_WPB": w} for w in (2, 3, 4)] +
             [{"CONV_NBW": n, "CONV_WPB": w} for n in (1, 2, 4) for w in (2, 3, 4)])
_cache = {}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _sizes(n_in, n_out, V, vol, bf16, big):
    import _hip
    rows_in, elem = BIG_FLOATS // n_in if big else V, 2 if bf16 else 4
    return (rows_in * n_in * elem, R.ceil_div(n_in, 32) * R.ceil_div(n_out, 16) * vol * 512 * elem,
            _hip.load().aabr_tile_blocks_words(V, vol) * 4)


def _decide(bf16, n_in, n_out, V, vol, flags, sizes, knobs):
    kn = tuple(knobs.get(k, R.UNSET) for k in R.KNOBS)
    return (R.bf16 if bf16 else R.fp32)(n_in, n_out, V, vol, flags, *sizes, kn)


def _config(key):
    """the first (book, planes in, planes out, knobs) whose launch is instance `key`"""
    bf16 = R.KINDS[key[0]] == "bf16"
    big = R.KINDS[key[0]] == "generic"
    books = ("large",) if big else ("small", "large", "one")
    planes = (32, 64, 96) if bf16 else (32, 48) if big else (32, 64, 16, 48, 96, 80)
    for book, knobs, n_in, n_out in itertools.product(books, KNOB_SETS, planes, (64, 256, 32)):
        V, vol = BOOKS[book][0], BOOKS[book][2] ** 3
        t = _decide(bf16, n_in, n_out, V, vol, 0, _sizes(n_in, n_out, V, vol, bf16, big), knobs)
        if t[:7] == key:
            return book, n_in, n_out, knobs
    raise AssertionError("no configuration reaches " + R.name(key))


def _book(name):
    if name not in _cache:
        import sparseconvnet as scn
        n, edge, fs = BOOKS[name]
        rng = np.random.default_rng(n + fs)
        cells = np.stack(np.meshgrid(*[np.arange(edge)] * 3, indexing="ij"), -1).reshape(-1, 3)
        coords = np.concatenate([cells[rng.choice(len(cells), n, replace=False)], np.zeros((n, 1), np.int64)], 1)
        zeros = np.zeros((n, 1), np.float32)
        x = scn.InputLayer(3, [64, 64, 64], mode=4)([_t(coords), _t(zeros)])
        tb = x.metadata.getSubmanifoldRuleBook(x.spatial_size, torch.LongTensor([fs] * 3))
        il = O.input_layer(coords, zeros, 4)
        assert tb.V_out == il["V"] == n and tb.vol == fs ** 3
        _cache[name] = (tb.out, O.submanifold_rules(il["coords"], [fs] * 3))
    return _cache[name]


def _big_input():
    """one input buffer of more than 2 GiB for every generic launch"""
    if "big" not in _cache:
        _cache["big"] = torch.zeros(BIG_FLOATS, device=DEV)
    return _cache["big"]


def _oracle(book, n_in, n_out, bf16, flags):
    """features, weights [vol, a, b] as the entry point reads them, bias, and the oracle's output"""
    k = (book, n_in, n_out, bf16, flags)
    if k not in _cache:
        ga, rb = _book(book)
        V, vol = ga.rows, ga.vol
        rng = np.random.default_rng(n_in * 1000 + n_out + vol)
        f = rng.standard_normal((V, n_in)).astype(np.float32)
        W = (rng.standard_normal((vol, n_in, n_out)) * 0.1).astype(np.float32)
        b = rng.standard_normal(n_out).astype(np.float32)
        if bf16:
            f = torch.as_tensor(f).bfloat16().float().numpy()
        Wr = torch.as_tensor(W).bfloat16().float().numpy() if bf16 else W
        # flags 3 (transposed, flipped): the weights are stored [vol][n_out][n_in] and offset k uses W[vol - 1 - k]^T
        Wk = np.ascontiguousarray(W[::-1].transpose(0, 2, 1)) if flags & 1 else W
        ref, _ = O.conv_fwd(f, Wr, rb, V, b)
        _cache[k] = (f, Wk, b, ref)
    return _cache[k]


@pytest.mark.parametrize("inst", [R.name(k) for k in R.compiled_instances()])
def test_every_tile_instance_matches_oracle(request, inst):
    import _hip
    from _hip import ptr, stream, check
    lib = _hip.load()
    key = next(k for k in R.compiled_instances() if R.name(k) == inst)
    book, n_in, n_out, knobs = _config(key)
    bf16, big = R.KINDS[key[0]] == "bf16", R.KINDS[key[0]] == "generic"
    ga, _ = _book(book)
    V, vol = ga.rows, ga.vol
    for name in R.KNOBS:
        _hip.set_knob(name, knobs.get(name))
    request.addfinalizer(lambda: [_hip.set_knob(name, None) for name in R.KNOBS])
    blocks = ga.blocks()
    rows_in = V
    if big:     # the book's rows at the bottom and the top of a > 2 GiB input; the table names only those
        rows_in = BIG_FLOATS // n_in
        assert rows_in * n_in * 4 >= (1 << 31) and rows_in < (1 << 25)   # (a block entry holds a 25-bit row)
        where = torch.arange(V, device=DEV, dtype=torch.int32)
        where[V // 2:] += rows_in - V
        assert int(where[-1]) * n_in * 4 > (1 << 31)
        lut = torch.cat([where, torch.full((1,), -1, dtype=torch.int32, device=DEV)])
        table = lut[ga.table.long()].contiguous()                       # -1 stays -1
        blocks = torch.empty(max(lib.aabr_tile_blocks_words(V, vol), 1), dtype=torch.int32, device=DEV)
        check(lib.aabr_build_tile_blocks(ptr(table), V, vol, ptr(blocks), stream()))
    for flags in (0, 3):
        f, Wk, b, ref = _oracle(book, n_in, n_out, bf16, flags)
        want = _decide(bf16, n_in, n_out, V, vol, flags, _sizes(n_in, n_out, V, vol, bf16, big), knobs)
        assert want[:7] == key
        Wd, bd = _t(Wk), _t(b)
        if bf16:
            fd = _t(f).bfloat16()
            out = torch.full((V, n_out), float("nan"), dtype=torch.bfloat16, device=DEV)
            wp = torch.empty(int(lib.aabr_conv_wpack_bf16_elems(vol, n_in, n_out)), dtype=torch.bfloat16, device=DEV)
            check(lib.aabr_conv_forward_bf16(ptr(fd), n_in, V, ptr(out), n_out, V, ptr(blocks), vol, ptr(Wd), ptr(bd),
                                             flags, ptr(wp), stream()))
        else:
            fd = _t(f)
            if big:
                x = _big_input()[: rows_in * n_in].view(rows_in, n_in)
                x[where.long()] = fd
                fd = x
            out = torch.full((V, n_out), float("nan"), device=DEV)
            wp = torch.empty(int(lib.aabr_conv_wpack_floats(vol, n_in, n_out)), device=DEV)
            check(lib.aabr_conv_forward(ptr(fd), n_in, rows_in, ptr(out), n_out, V, ptr(blocks), vol, ptr(Wd), ptr(bd),
                                        flags, ptr(wp), stream()))
        assert lib.aabr_conv_last_variant().decode() == inst
        got = out.float().cpu().numpy()
        if bf16:
            np.testing.assert_allclose(got, ref, rtol=2 ** -7, atol=2 ** -7 * np.abs(ref).max())
        else:
            np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * np.abs(f).max() * n_in)
