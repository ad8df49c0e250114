"""csrc/conv_single_tiles.h, the decision of the single-rule convolution route (k_conv_single: shape conditions, least row
count, pairs per chunk, grid), compiled for the host with g++ and compared over a grid of shapes with a plain restatement
below; then the loaded library's query and entry point against the header, the CONV_SINGLE knob, and SCN.conv_route,
which the route must leave as it was.  g++ and the library, no GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _hip
from sparseconvnet import SCN

HERE = os.path.dirname(os.path.abspath(__file__))
U = -(1 << 31)                       # conv_tiles.h kKnobUnset
G2 = 1 << 31
N_IN = (0, 16, 32, 48, 64, 96, 128, 160, 256)
N_OUT = (32, 64, 96, 128, 192)
VOLS = (1, 2, 8, 27)
NO_KNOBS = (U, U, U)


def want_unsupported(bf16, stats, n_in, n_out, rows_in, rows_out, vol):
    if bf16:
        return "fp32 storage only"
    if stats:
        return "no BatchNorm statistics"
    if not (n_in > 0 and n_out > 0 and 0 < vol <= 65535 and rows_in >= 0 and rows_out >= 0):
        return "bad sizes"
    if n_in > 128:
        return "n_in <= 128"
    if n_out % 64:
        return "n_out must be a multiple of 64"
    if n_in % 32:
        return "n_in must be a multiple of 32"
    if rows_in >= 1 << 23 or rows_in * n_in * 4 >= G2:
        return "input rows must be"
    if rows_out >= 1 << 25:
        return "too many output rows"
    if vol * (n_in // 32) * (n_out // 16) * 2048 >= G2:
        return "packed weights must be < 2 GiB"
    return None


def want_chunk(n_out, rows_out, vol, knobs):
    return 1024 if knobs[2] == 1024 else 256


def want_route(bf16, stats, n_in, n_out, rows_in, rows_out, vol, knobs, min_rows, default_on):
    """(refusal or None, chunk)"""
    if knobs[0] == 0 or (knobs[0] == U and not default_on):
        return "CONV_SINGLE is off", 0
    m = want_unsupported(bf16, stats, n_in, n_out, rows_in, rows_out, vol)
    if m:
        return m, 0
    if rows_out == 0:
        return "no output rows", 0
    if rows_out < (min_rows if knobs[1] == U else knobs[1]):
        return "too few output rows", 0
    return None, want_chunk(n_out, rows_out, vol, knobs)


def want_launch(n_in, n_out, rows_in, rows_out, vol, flags, knobs):
    """(refusal or None, kg, chunk, grid_x, grid_y, lds_bytes, wflip, wp_bytes)"""
    zero = (0,) * 7
    m = want_unsupported(0, 0, n_in, n_out, rows_in, rows_out, vol)
    if m:
        return (m,) + zero
    if rows_out == 0:
        return (None,) + zero
    if rows_in <= 0:
        return ("null pointer / empty input",) + zero
    chunk = want_chunk(n_out, rows_out, vol, knobs)
    gx, gy = rows_out // chunk + vol, n_out // 64           # the offsets share rows_out pairs; one partial chunk each
    if gx * gy >= G2:
        return ("too many workgroups",) + zero
    return (None, n_in // 32, chunk, gx, gy, 2 * 32 * n_in * 4, (flags >> 1) & 1, vol * (n_in // 32) * (n_out // 16) * 2048)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("single") / "libhostsingle.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "conv_single_host_harness.cpp")])
    lib = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.host_single.argtypes = [p, C.c_int64, p, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]
    lib.host_single_min_rows.restype = C.c_int64
    return lib


def _run(lib, cases):
    a = np.ascontiguousarray(cases, np.int64).reshape(len(cases), 11)
    out = np.zeros((len(cases), 10), np.int64)
    msgs = np.zeros((len(cases), 2, 128), np.uint8)
    lib.host_single(a, len(cases), out, msgs)
    text = [[bytes(m).split(b"\0")[0].decode() for m in pair] for pair in msgs]
    return out.tolist(), text


def _rows(min_rows):
    rows = {-1, 0, 1, 15, 16, 17, 255, 256, 257, 1000, 1023, 1024, 1025, 84077, 309589, (1 << 25) - 1, 1 << 25,
            min_rows - 1, min_rows, min_rows + 1}
    return sorted(r for r in rows if r >= -1)


def _cases(min_rows):
    out = []
    for bf16, stats, n_in, n_out, vol, r in itertools.product((0, 1), (0, 1), N_IN, N_OUT, VOLS, _rows(min_rows)):
        for rows_in in (max(r, 1), 0):
            out.append((bf16, stats, n_in, n_out, rows_in, r, vol, 2 * (len(out) % 2)) + NO_KNOBS)
    for kn in ((0, U, U), (1, U, U), (2, U, U), (U, 0, U), (U, 100000, U), (1, 0, 256), (U, U, 1024), (U, 0, 512)):
        for n_in, n_out, vol, r in itertools.product((32, 64, 128, 160), (64, 128), (1, 8), (0, 16, 5000, 84077, 600000)):
            out.append((0, 0, n_in, n_out, r + 3, r, vol, 0) + kn)
    for n_in in (32, 128):                                          # the 2^23-row and 2 GiB input limits, one step either side
        for rows_in in ((1 << 23) - 1, 1 << 23, G2 // (n_in * 4) - 1, G2 // (n_in * 4)):
            out.append((0, 0, n_in, 64, rows_in, 50000, 8, 0) + NO_KNOBS)
    for vol in (8191, 8192):                                        # packed weights around 2 GiB (128 -> 512: 256 KiB per offset)
        out.append((0, 0, 128, 512, 1000, 50000, vol, 0) + NO_KNOBS)
    return out


def test_single_decision_matches_the_restatement(host):
    min_rows, default_on = host.host_single_min_rows(), host.host_single_default_on()
    cases = _cases(min_rows)
    got, text = _run(host, cases)
    refusals, taken, chunks = set(), 0, set()
    for c, g, (m_route, m_launch) in zip(cases, got, text):
        wr, wchunk = want_route(*c[:7], knobs=c[8:], min_rows=min_rows, default_on=default_on)
        assert g[0] == (wr is not None) and g[1] == wchunk and (wr is None) == (m_route == ""), (c, g, m_route, wr)
        if wr is not None:
            assert wr in m_route, (c, m_route, wr)
            refusals.add(wr)
        else:
            taken += 1
            chunks.add(wchunk)
        wl = want_launch(c[2], c[3], c[4], c[5], c[6], c[7], c[8:])
        assert g[2] == (wl[0] is not None) and tuple(g[3:]) == wl[1:], (c, g, wl)
        assert (wl[0] or "") in m_launch and (wl[0] is None) == (m_launch == ""), (c, m_launch, wl)
    # every refusal the issue lists was reached, and both chunk lengths
    for m in ("no BatchNorm statistics", "fp32 storage only", "n_in <= 128", "n_out must be a multiple of 64",
              "n_in must be a multiple of 32", "too few output rows", "no output rows", "CONV_SINGLE is off"):
        assert m in refusals, m
    assert taken > 100 and chunks == {256, 1024}


def test_library_query_and_entry_point_follow_the_header(host):
    lib = _hip.load()
    min_rows, default_on = host.host_single_min_rows(), host.host_single_default_on()
    shapes = [(bf16, stats, n_in, n_out, r + 5, r, vol) for bf16, stats, n_in, n_out, vol, r in
              itertools.product((0, 1), (0, 1), (32, 48, 64, 128, 160), (32, 64, 128), (1, 8),
                                (0, 1, 1000, min_rows - 1, min_rows, 309589))]
    for knobs in (NO_KNOBS, (1, U, U), (0, U, U), (1, 0, U), (1, 0, 1024), (U, 0, 256)):
        try:
            for name, v in zip(("CONV_SINGLE", "SINGLE_ROWS", "SINGLE_CHUNK"), knobs):
                _hip.set_knob(name, None if v == U else v)
            for s in shapes:
                wr, wchunk = want_route(*s, knobs=knobs, min_rows=min_rows, default_on=default_on)
                q = (s[2], s[3], s[4], s[5], s[6], s[0], s[1])
                assert lib.aabr_conv_single_chunk(*q) == wchunk, (s, knobs)
                assert (wr or "") in lib.aabr_conv_single_refusal(*q).decode(), (s, knobs)
                r = SCN.single_route(s[2], s[3], s[4], s[5], s[6], bool(s[0]), stats=bool(s[1]))
                assert (r is None) == (wchunk == 0) and (r is None or (r.kind, r.takes_residual, r.stats_parts(s[5]))
                                                         == ("single", True, 0))
        finally:
            for name in ("CONV_SINGLE", "SINGLE_ROWS", "SINGLE_CHUNK"):
                _hip.set_knob(name)
    # the entry point words the header's refusals before any HIP call; nothing to do is no error
    one = 4096

    def fn(n_in=64, n_out=64, rows=170, V=150, vol=8, res=None):
        return lib.aabr_conv_forward_single(one, n_in, rows, one, n_out, V, one, vol, None, 0, one, res, None)

    for kw, text in ((dict(n_in=160), b"n_in <= 128"), (dict(n_out=32), b"n_out must be a multiple of 64"),
                     (dict(n_in=48), b"n_in must be a multiple of 32"), (dict(rows=0), b"null pointer / empty input"),
                     (dict(rows=1 << 23), b"input rows must be"), (dict(vol=0), b"bad sizes"),
                     (dict(res=one + 4), b"16-byte aligned")):
        rc = fn(**kw)
        assert rc == -1 and text in lib.aabr_last_error(), (kw, rc, lib.aabr_last_error())
    assert b"aabr_conv_forward_single:" in lib.aabr_last_error()
    assert fn(V=0) == 0
    assert lib.aabr_conv_forward_single(None, 64, 0, None, 64, 0, None, 8, None, 0, None, None, None) == 0


def test_knob_turns_the_route_off():
    args = (128, 128, 400000, 309589, 8, False)
    _hip.set_knob("CONV_SINGLE", 1)
    try:
        assert SCN.single_route(*args).kind == "single"
        assert SCN.single_route(*args, stats=True) is None and SCN.single_route(128, 128, 4000, 3000, 8, True) is None
        _hip.set_knob("CONV_SINGLE", 0)
        assert SCN.single_route(*args) is None
    finally:
        _hip.set_knob("CONV_SINGLE")


class _Gather(object):
    def __init__(self, rows, vol):
        self.rows, self.vol, self.table, self.built = rows, vol, "table", []

    def blocks(self):
        self.built.append("blocks")

    def blocks_wide(self, tile_rows):
        self.built.append(("wide", tile_rows))

    def pairs(self):
        self.built.append("pairs")


def test_compile_streams_builds_the_pairs_for_a_single_launch():
    import torch
    _hip.set_knob("CONV_SINGLE", 1)
    try:
        g = _Gather(309589, 8)
        SCN.compile_streams(g, 40000, 128, 128, torch.float32, single=True)
        assert g.built == ["pairs"]
        g = _Gather(309589, 8)
        SCN.compile_streams(g, 40000, 128, 128, torch.bfloat16, single=True)        # bf16 storage: not this route
        assert len(g.built) == 1 and g.built[0] != "pairs"
        g = _Gather(309589, 8)
        SCN.compile_streams(g, 40000, 128, 128, torch.float32)                      # default arguments: as before
        assert len(g.built) == 1 and g.built[0] != "pairs"
    finally:
        _hip.set_knob("CONV_SINGLE")


@pytest.mark.parametrize("single", (None, 0, 1))
def test_conv_route_is_unchanged(single):
    """SCN.conv_route cannot see a book's structure and must not move: its own grid check, with the route's knob either way"""
    import test_conv_route_host as T
    _hip.set_knob("CONV_SINGLE", single)
    try:
        kinds = T.check_grid()
    finally:
        _hip.set_knob("CONV_SINGLE")
    assert set(kinds) == {None, "narrow", "wide", "split", "tiles"}, kinds
