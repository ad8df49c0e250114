"""csrc/conv_single_tiles.h, the decision and launch description of the single-rule convolution's BACKWARD-STATISTICS form
(k_conv_single<KG, true>: `single_bwd_stats_refusal`, `single_bwd_stats_launch`), compiled for the host with g++ and
compared over a grid of shapes with a plain restatement below: every refusal, the part counts, the size of the fp64
buffer, and that the plain route's queries still refuse statistics; the same header as a stand-alone program under
-fsanitize=address,undefined; then the loaded library's queries, entry point and SCN's route query against the header.
g++ and the library, no GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _hip
from sparseconvnet import SCN

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "conv_single_bwd_stats_host_harness.cpp")
U = -(1 << 31)                       # conv_tiles.h kKnobUnset
G2 = 1 << 31
NO_KNOBS = (U, U, U, U)
ON = (U, U, U, 1)                    # SINGLE_BWD_STATS = 1: the decision behind the switch, whatever the shipped default
KNOB_NAMES = ("CONV_SINGLE", "SINGLE_ROWS", "SINGLE_CHUNK", "SINGLE_BWD_STATS")


def want_unsupported(bf16, n_in, n_out, rows_in, rows_out, vol):
    """every condition of the plain route's `single_unsupported` but the statistics one, in its order"""
    if bf16:
        return "fp32 storage only"
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


def want_route(bf16, n_in, n_out, rows_in, rows_out, vol, knobs, min_rows, default_on, bwd_default_on):
    """(refusal or None, chunk)"""
    if knobs[3] == 0 or (knobs[3] == U and not bwd_default_on):
        return "SINGLE_BWD_STATS is off", 0
    if knobs[0] == 0 or (knobs[0] == U and not default_on):
        return "CONV_SINGLE is off", 0
    m = want_unsupported(bf16, n_in, n_out, rows_in, rows_out, vol)
    if m:
        return m, 0
    if rows_out == 0:
        return "no output rows", 0
    if rows_out < (min_rows if knobs[1] == U else knobs[1]):
        return "too few output rows", 0
    return None, 1024 if knobs[2] == 1024 else 256


def want_launch(n_in, n_out, rows_in, rows_out, vol, flags, knobs):
    """(refusal or None, kg, chunk, grid_x, grid_y, lds_bytes, wflip, wp_bytes, parts, stats_doubles)"""
    zero = (0,) * 9
    m = want_unsupported(0, n_in, n_out, rows_in, rows_out, vol)
    if m:
        return (m,) + zero
    if rows_out == 0:
        return (None,) + zero
    if rows_in <= 0:
        return ("null pointer / empty input",) + zero
    chunk = 1024 if knobs[2] == 1024 else 256
    parts, gy = rows_out // chunk + vol, n_out // 64       # one part per chunk: the offsets share rows_out pairs, one partial chunk each
    if parts * gy >= G2:
        return ("too many workgroups",) + zero
    lds = max(2 * 32 * n_in * 4, 256 * 8 * 8)               # the stage, reused for the workgroup's 256 x 8 fp64 sums
    return (None, n_in // 32, chunk, parts, gy, lds, (flags >> 1) & 1, vol * (n_in // 32) * (n_out // 16) * 2048, parts,
            parts * 2 * n_out)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("single_bwd") / "libhostsinglebwd.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.host_single_bwd_stats.argtypes = [p, C.c_int64, p, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]
    lib.host_single_min_rows.restype = C.c_int64
    return lib


def _run(lib, cases):
    a = np.ascontiguousarray(cases, np.int64).reshape(len(cases), 11)
    out = np.zeros((len(cases), 13), np.int64)
    msgs = np.zeros((len(cases), 3, 128), np.uint8)
    lib.host_single_bwd_stats(a, len(cases), out, msgs)
    text = [[bytes(m).split(b"\0")[0].decode() for m in three] for three in msgs]
    return out.tolist(), text


def _cases(min_rows):
    rows = sorted({-1, 0, 1, 255, 256, 257, 1000, 1023, 1024, 1025, 84077, 200652, 281622, (1 << 25) - 1, 1 << 25,
                   min_rows - 1, min_rows, min_rows + 1})
    out = []
    for bf16, n_in, n_out, vol, r in itertools.product((0, 1), (0, 16, 32, 48, 64, 96, 128, 160, 256),
                                                       (32, 64, 96, 128, 192), (1, 2, 8, 27), rows):
        for rows_in in (max(r, 1), 0):
            out.append((bf16, n_in, n_out, rows_in, r, vol, 2 * (len(out) % 2)) + ON)
    for kn in ((0, U, U, U), (1, U, U, U), (U, U, U, 0), (U, U, U, 1), (0, U, U, 1), (1, 0, U, 0), (U, 0, U, U),
               (U, 100000, U, 1), (1, 0, 256, 1), (U, U, 1024, 1), (U, 0, 512, 1), (U, U, 1024, U)):
        for n_in, n_out, vol, r in itertools.product((32, 64, 128, 160), (64, 128), (1, 8), (0, 16, 5000, 84077, 600000)):
            out.append((0, n_in, n_out, r + 3, r, vol, 0) + kn)
    for n_in in (32, 128):                                          # the 2^23-row and 2 GiB input limits, one step either side
        for rows_in in ((1 << 23) - 1, 1 << 23, G2 // (n_in * 4) - 1, G2 // (n_in * 4)):
            out.append((0, n_in, 64, rows_in, 50000, 8, 0) + ON)
    for vol in (8191, 8192, 65535, 65536):                          # packed weights around 2 GiB; the largest filter volume
        out.append((0, 128, 512, 1000, 50000, vol, 0) + ON)
    return out


def test_bwd_stats_decision_matches_the_restatement(host):
    min_rows, default_on = host.host_single_min_rows(), host.host_single_default_on()
    bwd_on = host.host_single_bwd_stats_default_on()
    cases = _cases(min_rows)
    got, text = _run(host, cases)
    refusals, taken, chunks = set(), 0, set()
    for c, g, (m_route, m_launch, m_old) in zip(cases, got, text):
        wr, wchunk = want_route(*c[:6], knobs=c[7:], min_rows=min_rows, default_on=default_on, bwd_default_on=bwd_on)
        assert g[0] == (wr is not None) and g[1] == wchunk and (wr is None) == (m_route == ""), (c, g, m_route, wr)
        wl = want_launch(c[1], c[2], c[3], c[4], c[5], c[6], c[7:])
        assert g[2] == (wl[0] is not None) and tuple(g[3:12]) == wl[1:], (c, g, wl)
        assert (wl[0] or "") in m_launch and (wl[0] is None) == (m_launch == ""), (c, m_launch, wl)
        if wr is not None:
            assert wr in m_route, (c, m_route, wr)
            refusals.add(wr)
        else:                            # routed: the launch exists, one part per workgroup column, the buffer holds them
            taken += 1
            chunks.add(wchunk)
            if c[3] > 0:                 # (the route does not look at rows_in; without input rows the launch refuses)
                assert wl[0] is None and g[10] == g[5] == c[4] // wchunk + c[5] and g[11] == g[10] * 2 * c[2] == wl[9]
            if c[3] > 0 and c[4] >= min_rows and c[5] <= 27:             # what lets the parts share the wide kernel's workspace
                assert g[10] <= c[4] // 64 + 1, c
        # the plain route, asked for statistics, refuses as before -- with its own text unless an earlier condition speaks
        assert g[12] == 1 and m_old != "", c
        if not c[0] and not (c[7] == 0 or (c[7] == U and not default_on)):
            assert "no BatchNorm statistics" in m_old, (c, m_old)
    for m in ("SINGLE_BWD_STATS is off", "CONV_SINGLE is off", "fp32 storage only", "bad sizes", "n_in <= 128",
              "n_out must be a multiple of 64", "n_in must be a multiple of 32", "input rows must be",
              "too many output rows", "packed weights must be < 2 GiB", "no output rows", "too few output rows"):
        assert m in refusals, m
    assert taken > 100 and chunks == {256, 1024}


def test_bench_books_part_counts_and_buffer_sizes(host):
    """the three statistics-carrying books of the training step: parts = rows / 256 + 8, all inside the workspace the
    wide kernel's per-tile parts use ((rows / 64 + 1) x 2 x planes doubles)"""
    books = ((128, 128, 12000, 84077), (128, 64, 84077, 200652), (64, 64, 200652, 281622))
    got, text = _run(host, [(0, n_in, n_out, rows_in, rows, 8, 2) + NO_KNOBS for n_in, n_out, rows_in, rows in books])
    for (n_in, n_out, _, rows), g, t in zip(books, got, text):
        if not host.host_single_bwd_stats_default_on():
            assert g[0] == 1 and "SINGLE_BWD_STATS is off" in t[0]
        else:
            assert g[0] == 0 and g[1] == 256
        assert g[2] == 0 and g[3] == n_in // 32 and g[5] == g[10] == rows // 256 + 8 and g[6] == n_out // 64 and g[8] == 1
        assert g[11] == g[10] * 2 * n_out <= (rows // 64 + 1) * 2 * n_out


def test_header_under_the_sanitizers(tmp_path):
    """the pure C++ harness as a stand-alone program: address and undefined-behaviour sanitizers over the header's sweep"""
    exe = str(tmp_path / "single_bwd_host")
    subprocess.check_call(["g++", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DHARNESS_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "routed" in r.stdout, r.stdout


def test_library_queries_and_entry_point_follow_the_header(host):
    lib = _hip.load()
    min_rows, default_on = host.host_single_min_rows(), host.host_single_default_on()
    bwd_on = host.host_single_bwd_stats_default_on()
    shapes = [(bf16, n_in, n_out, r + 5, r, vol) for bf16, n_in, n_out, vol, r in
              itertools.product((0, 1), (32, 48, 64, 128, 160), (32, 64, 128), (1, 8),
                                (0, 1, 1000, min_rows - 1, min_rows, 281622))]
    for knobs in (NO_KNOBS, (1, U, U, 1), (0, U, U, 1), (1, 0, U, U), (1, 0, 1024, 1), (U, 0, 256, 0), (U, U, U, 0)):
        try:
            for name, v in zip(KNOB_NAMES, knobs):
                _hip.set_knob(name, None if v == U else v)
            for s in shapes:
                wr, wchunk = want_route(*s, knobs=knobs, min_rows=min_rows, default_on=default_on, bwd_default_on=bwd_on)
                q = (s[1], s[2], s[3], s[4], s[5], s[0])
                assert lib.aabr_conv_single_bwd_stats_chunk(*q) == wchunk, (s, knobs)
                assert (wr or "") in lib.aabr_conv_single_bwd_stats_refusal(*q).decode(), (s, knobs)
                assert (lib.aabr_conv_single_bwd_stats_refusal(*q) == b"") == (wchunk != 0)
                r = SCN.single_bwd_stats_route(s[1], s[2], s[3], s[4], s[5], bool(s[0]))
                assert (r is None) == (wchunk == 0), (s, knobs)
                if r is not None:
                    parts = s[4] // wchunk + s[5]
                    assert (r.kind, r.takes_residual, r.parts, r.stats_parts(s[4])) == ("single", True, parts, parts)
                    assert lib.aabr_conv_single_bwd_stats_parts(s[4], s[5], wchunk) == parts
                # the plain queries keep refusing statistics, whatever the new knob says
                assert lib.aabr_conv_single_chunk(*q, 1) == 0 and lib.aabr_conv_single_refusal(*q, 1) != b""
                assert SCN.single_route(s[1], s[2], s[3], s[4], s[5], bool(s[0]), stats=True) is None
        finally:
            for name in KNOB_NAMES:
                _hip.set_knob(name)
    assert lib.aabr_conv_single_bwd_stats_parts(1000, 8, 512) == 0 and lib.aabr_conv_single_bwd_stats_parts(0, 8, 256) == 0
    # the entry point words the header's refusals and its own pointer checks before any HIP call; nothing to do is no error
    one = 4096

    def fn(n_in=64, n_out=64, rows=170, V=150, vol=8, res=None, stats=one, x=one, mean=one, invstd=one, leak=0.0):
        return lib.aabr_conv_forward_single_bwd_stats(one, n_in, rows, one, n_out, V, one, vol, None, 3, one, res, stats, x,
                                                      mean, invstd, None, None, leak, None)

    for kw, text in ((dict(n_in=160), b"n_in <= 128"), (dict(n_out=32), b"n_out must be a multiple of 64"),
                     (dict(n_in=48), b"n_in must be a multiple of 32"), (dict(rows=0), b"null pointer / empty input"),
                     (dict(rows=1 << 23), b"input rows must be"), (dict(vol=0), b"bad sizes"),
                     (dict(res=one + 4), b"16-byte aligned"), (dict(x=one + 8), b"16-byte aligned"),
                     (dict(stats=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(mean=None), b"null pointer"),
                     (dict(invstd=None), b"null pointer"), (dict(stats=one + 4), b"8-byte aligned"),
                     (dict(leak=-0.5), b"leakiness >= 0")):
        rc = fn(**kw)
        assert rc == -1 and text in lib.aabr_last_error(), (kw, rc, lib.aabr_last_error())
    assert b"aabr_conv_forward_single_bwd_stats:" in lib.aabr_last_error()
    assert fn(V=0) == 0


def test_plan_record_reaches_the_new_entry_point():
    """an AABR_PLAN_CONV_SINGLE record with i32[5] == 1 is handed to aabr_conv_forward_single_bwd_stats (its refusal names
    it: no launch happens), without it to aabr_conv_forward_single; a bf16 record is refused"""
    import struct
    lib = _hip.load()
    op = struct.Struct("<2i6i4f4q12Q")
    assert op.size == 176
    one = 4096
    for i5, flags, text in ((1, 0, b"aabr_conv_forward_single_bwd_stats: n_in must be a multiple of 32"),
                            (0, 0, b"aabr_conv_forward_single: n_in must be a multiple of 32"),
                            (1, 1, b"fp32 storage only")):
        rec = op.pack(11, flags, 48, 64, 8, 3, 0, i5, 0.0, 0.0, 0.0, 0.0, 170, 150, 0, 0, one, one, one, 0, 0, one, one, one,
                      one, one, 0, 0)
        assert lib.aabr_plan_run(rec, 1, None) == -1
        assert text in lib.aabr_last_error(), lib.aabr_last_error()
