"""csrc/conv_wide_tiles.h, the launch decision of the wide kernel k_conv_cs (rows per tile, offset split, instance, grid,
LDS bytes, wflip word), compiled for the host and compared field by field with the rule as conv_wide.hip wrote it before
(tests/conv_wide_rule.py) over a grid of shapes, parts, tile rows, flags and tuning knobs; the grid must reach every
instance conv_wide.hip compiles, and the decision must return no other.  Then the loaded library's four queries against
the header, and the entry points' refusals.  g++ and the library, no GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import conv_wide_rule as R

HERE = os.path.dirname(os.path.abspath(__file__))
U, G2 = R.UNSET, R.G2
N_IN = sorted({v + d for v in (32, 64, 96, 128, 192, 256, 384, 512, 768) for d in (-32, 0, 32)})   # 0 .. 800
N_OUT = (64, 128, 192, 256)
VOLS = (1, 2, 8, 27, 63, 64)
PARTS = (0, 1, 2, 27, 32, 33)
TILE_ROWS = (0, 16, 48, 64, 96, 112, 128, 240, 256, 100)
KNOB_VALUES = {"WIDE_ROWS": (0, 16, 100, 112, 240, 256), "CONV_WIDE": (0, 1, 2), "CONV_WIDE_BF16": (0, 1, 2),
               "WIDE_SPLIT": (0, 1, 2, 5, 32, 33), "SPLIT_ROWS": (48, 64, 96, 100, 128, 144),
               "SPLIT_MIN_ITEMS": (0, 1, 8, 9, 100), "SPLIT_TARGET": (0, 1, 512, 768, 1280, 100000),
               "WIDE_NBUF": (0, 1, 2, 3), "SPLIT_NBUF": (1, 2, 3), "WIDE_NCB": (0, 1, 2), "WIDE_PRIO": (0, 1, 2)}


def _threshold_rows():
    """V_out around every workgroup-count threshold: tiles x slabs at 319 / 320 / 321 and 511 / 512 / 513 for every tile
    size and slab count the rules produce, V_out 1023 / 1024, (tile, slab) items at 7 / 8"""
    rows = {-1, 0, 1, 63, 64, 65, 150, 1023, 1024, 1025, 5565}
    for T, slabs, items in itertools.product((64, 80, 96, 112, 128), (1, 2, 3, 4), (7, 8, 319, 320, 321, 511, 512, 513)):
        tiles = -(-items // slabs)
        rows |= {(tiles - 1) * T, tiles * T, tiles * T + 1}
    return sorted(rows)


def _knobs(**kw):
    return tuple(kw.get(k, U) for k in R.KNOBS)


def _case(storage, parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, stats, knobs=R.NO_KNOBS):
    return (storage, parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, stats) + tuple(knobs)


def _limit_cases():
    """the 2^23-row limit and each 2 GiB limit (input bytes, block words, packed weights), one step either side"""
    out = []
    for st, elem in ((0, 4), (1, 2)):
        for rows in ((1 << 23) - 1, 1 << 23):
            out.append(_case(st, 0, 64, 64, rows, 4096, 64, 8, 0, 0))
        for n_in in (128, 256):
            for rows in (G2 // (n_in * elem) - 1, G2 // (n_in * elem)):
                out.append(_case(st, 0, n_in, 128, rows, 70000, 128, 27, 0, 0))
        for T, vol in ((64, 27), (96, 27), (128, 63), (112, 8)):
            per = (vol + 1) * 4 + (T // 16) * vol * 64                  # bytes of block words per tile
            tiles = (G2 - 1) // per                                    # the most tiles below 2 GiB
            for n_in, n_out in ((64, 64), (128, 128), (256, 256)):
                for V in (tiles * T, tiles * T + 1):
                    out.append(_case(st, 0, n_in, n_out, 1000, V, T, vol, 0, 0, _knobs(WIDE_ROWS=T)))
                    out.append(_case(st, 2, n_in, n_out, 1000, V, T, vol, 0, 0, _knobs(SPLIT_ROWS=T, WIDE_SPLIT=2)))
        for n_out in ((2048, 2112) if elem == 4 else (4160, 4224)):      # 63 x 4096 x n_out x elem around 2^31
            for V in (150, 100000):
                out.append(_case(st, 0, 4096, n_out, 1000, V, 64, 63, 0, 0))
                out.append(_case(st, 2, 4096, n_out, 1000, V, 64, 63, 0, 0))
    return out


def _cases(dev):
    rows = _threshold_rows()
    out = []
    # the queries' grid: every shape at every threshold (parts, tile_rows, flags, statistics do not enter them)
    queries = [_case(st, 0, n_in, n_out, max(V, 1), V, 64, vol, 0, 0)
               for st, n_in, n_out, vol, V in itertools.product((0, 1), N_IN, N_OUT, VOLS, rows)]
    # the launches' grid: the full product of what picks the message and the instance; V_out, flags, rows_in and statistics cycle
    # with pairwise coprime periods (9, 7 or 11, 13, 17; the innermost axis has 10 values), so that every tile size meets
    # every V_out, every flag word, an empty input and statistics
    few = (0, 150, 150, 4097, 150, 64 * 321, 1, 150, 4097)
    flags = (0, 2, 0, 256, 512, 768, 1024, 1280 | 2, 1536, 1792, 2048) if dev else (0, 2, 0, 2, 256, 1024 | 2, 2)
    assert len(TILE_ROWS) == 10 and len(few) == 9 and len(flags) in (7, 11)
    launches = []
    for i, (st, parts, n_in, n_out, vol, T) in enumerate(itertools.product((0, 1), PARTS, N_IN, N_OUT, VOLS, TILE_ROWS)):
        launches.append(_case(st, parts, n_in, n_out, 170 if i % 13 else 0, few[i % 9], T, vol, flags[i % len(flags)],
                              int(parts == 0 and i % 17 < 6)))
    for st, n_in, n_out, T, f, stats in itertools.product((0, 1), (32, 64, 128, 192, 256, 512), (64, 128), (48, 64, 128),
                                                          flags, (0, 1)):
        launches.append(_case(st, 0, n_in, n_out, 170, 150, T, 8, f, stats))
    launches += [_case(0, 0, 64, 64, -1, 150, 64, 8, 0, 0), _case(1, 2, 64, 64, 170, -1, 64, 8, 0, 0)]
    # each knob alone at the values its code distinguishes
    knobbed = []
    for k, values in KNOB_VALUES.items():
        for v in values:
            kn = _knobs(**{k: v})
            for st, n_in, n_out, V in itertools.product((0, 1), (32, 64, 96, 128, 192, 256, 512), (64, 128, 192),
                                                        (150, 600, 1024, 5565, 20480, 64 * 321, 200000)):
                knobbed.append(_case(st, 0, n_in, n_out, V, V, 64, 27, 0, 0, kn))
                knobbed.append(_case(st, 3, n_in, n_out, V, V, 96, 27, 2, 0, kn))
                knobbed.append(_case(st, 0, n_in, n_out, V, V, 64, 2, 0, 0, kn))
    limits = _limit_cases()
    return queries + knobbed + limits, launches + knobbed + limits


def _harness(tmp_path, dev):
    so = str(tmp_path / ("libhostwide%d.so" % dev))
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared"] + (["-DAABR_DEV"] if dev else []) +
                          ["-o", so, os.path.join(HERE, "conv_wide_host_harness.cpp")])
    lib = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.host_wide.argtypes = [C.c_int, p, C.c_int64, p, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]
    assert lib.host_wide_dev() == dev
    return lib


def _run(lib, what, cases):
    a = np.ascontiguousarray(cases, np.int64).reshape(len(cases), 21)
    out = np.zeros((len(cases), 14), np.int64)
    msgs = np.zeros((len(cases), 128), np.uint8)
    lib.host_wide(what, a, len(cases), out, msgs)
    return out, [bytes(m).split(b"\0")[0].decode() for m in msgs] if what == 2 else None


SPLIT32_MSG = "the fp32 offset split needs n_in >= 64"


@pytest.mark.parametrize("dev", (0, 1), ids=("release", "dev"))
def test_wide_decision_matches_rule_and_reaches_every_compiled_instance(tmp_path, dev):
    lib = _harness(tmp_path, dev)
    queries, launches = _cases(dev)
    for what, f32, bf16 in ((0, R.tile_rows_f32, R.tile_rows_bf16), (1, R.split_f32, R.split_bf16)):
        got = _run(lib, what, queries)[0][:, 0].tolist()
        for c, g in zip(queries, got):
            want = (bf16 if c[0] else f32)(c[2], c[3], c[4], c[5], c[7], c[10:])
            assert g == want, (what, c, g, want)
    got, msgs = _run(lib, 2, launches)
    reached, split_reached, refusals = set(), set(), set()
    for c, g, m in zip(launches, got.tolist(), msgs):
        want = R.launch(*c[:10], knobs=c[10:], dev=bool(dev))
        if want[0] is None and c[0] == 0 and c[1] != 0 and c[2] == 32 and want[1] == 4:
            # the one intended change: the parent ran the 128-channel instance on 32-channel rows here
            assert g[0] == 1 and m == SPLIT32_MSG and not any(g[1:]), (c, g, m)
            continue
        if want[0] is not None and want[0].startswith("128-column slabs"):
            raise AssertionError("the parent's 128-column check cannot fire: %r" % (c,))
        assert (m or None) == want[0] and g[0] == (want[0] is not None) and tuple(g[1:]) == want[1:], (c, g, m, want)
        if want[0] is not None:
            refusals.add(want[0])
        elif want[8]:                                   # a launch (V_out > 0)
            (split_reached if want[6] else reached).add(want[1:6])
    compiled = R.compiled_instances(dev)
    assert len(compiled) == len(set(compiled)) == (30 if dev else 20)
    assert reached == set(compiled) - set(R.never_launched(dev)), (sorted(set(compiled) ^ reached))
    assert split_reached == set(R.split_instances()), sorted(split_reached ^ set(R.split_instances()))
    assert len(refusals) >= 12                          # every message of the launchers was exercised


def test_instance_names_are_the_ones_profiles_key_on():
    names = {R.name(k) for k in R.compiled_instances()} | {R.name(k, True) for k in R.split_instances()}
    for n in ("k_conv_cs<4,0,1>", "k_conv_cs<3,0,2>", "k_conv_cs<2,0,1,split>", "k_conv_cs<4,0,2,split>",
              "k_conv_cs<2,0,1,bf16>", "k_conv_cs<1,0,2,bf16,x128>", "k_conv_cs<4,0,1,bf16,split>"):
        assert n in names, n
    assert len(names) == 30
    # and conv_wide.hip's table carries exactly these strings
    src = open(os.path.join(os.path.dirname(HERE), "automatic-as-built-reconstruction_amd", "csrc", "conv_wide.hip")).read()
    table = src[src.index("static const WideInst kWide[]"):src.index("constexpr int kWideCount")]
    release = table[:table.index("#ifdef AABR_DEV")]
    import re
    assert set(re.findall(r'"(k_conv_cs<[^"]*)"', release)) == names
    dev_names = {R.name(k) for k in R.compiled_instances(True)} | names
    assert set(re.findall(r'"(k_conv_cs<[^"]*)"', table)) == dev_names


def test_library_queries_equal_the_header(tmp_path):
    """the loaded library's four queries against the header over the WHOLE query grid and the limit cases: knobs unset,
    then each of CONV_WIDE, WIDE_ROWS, SPLIT_MIN_ITEMS and WIDE_SPLIT at every value (this pins wide_knobs()'s field order
    and the storage each extern "C" query hands on).  The harness loops the library's functions natively."""
    import _hip
    lib, host = _hip.load(), _harness(tmp_path, 0)
    fns = (C.c_void_p * 4)(*[C.cast(getattr(lib, n), C.c_void_p) for n in
                             ("aabr_conv_wide_tile_rows", "aabr_conv_wide_tile_rows_bf16", "aabr_conv_wide_split",
                              "aabr_conv_wide_split_bf16")])
    host.host_library_queries.argtypes = [C.c_void_p] + host.host_wide.argtypes[1:4]
    base = np.array([c for c in _cases(0)[0] if c[10:] == R.NO_KNOBS] + _limit_cases(), np.int64)
    base[:, 10:] = U
    assert len(base) > 200000
    knobs = [{}] + [{k: v} for k in ("CONV_WIDE", "WIDE_ROWS", "SPLIT_MIN_ITEMS", "WIDE_SPLIT") for v in KNOB_VALUES[k]]
    for kw in knobs:
        cases = base.copy()
        for k, v in kw.items():
            cases[:, 10 + R.KNOBS.index(k)] = v
        got = np.zeros((len(cases), 2), np.int64)
        try:
            for k, v in kw.items():
                _hip.set_knob(k, v)
            host.host_library_queries(fns, cases, len(cases), got)
        finally:
            for k in kw:
                _hip.set_knob(k, None)
        for what in (0, 1):
            want = _run(host, what, cases)[0][:, 0]
            bad = np.nonzero(got[:, what] != want)[0]
            assert not len(bad), (what, kw, cases[bad[0]].tolist(), int(got[bad[0], what]), int(want[bad[0]]))


def test_entry_points_refuse_with_the_decisions_messages():
    """every message of wide_launch once per family, through the real entry points, before any HIP call"""
    import _hip
    lib = _hip.load()
    one, E = 4096, -1                                    # a non-null, 16-byte aligned pointer nobody follows

    def f32(n_in=64, n_out=64, rows=170, V=150, T=64, vol=8, flags=0, stats=None):
        return lib.aabr_conv_forward_wide_stats(one, n_in, rows, one, n_out, V, one, T, vol, None, flags, one, None, stats,
                                                None)

    def f32s(n_in=64, n_out=64, rows=170, V=150, T=64, vol=8, flags=0, parts=3, scratch=one):
        return lib.aabr_conv_forward_wide_split(one, n_in, rows, one, n_out, V, one, T, vol, None, flags, one, None, parts,
                                                scratch, None)

    def b16(n_in=64, n_out=64, rows=170, V=150, T=64, vol=8, flags=0, stats=None):
        return lib.aabr_conv_forward_wide_bf16_stats(one, n_in, rows, one, n_out, V, one, T, vol, None, flags, one, stats,
                                                     None)

    def b16s(n_in=64, n_out=64, rows=170, V=150, T=64, vol=8, flags=0, parts=3, scratch=one):
        return lib.aabr_conv_forward_wide_split_bf16(one, n_in, rows, one, n_out, V, one, T, vol, None, flags, one, parts,
                                                     scratch, None)

    def refused(rc, text):
        assert rc == E and text in lib.aabr_last_error(), (rc, text, lib.aabr_last_error())

    for fn, bf, split in ((f32, 0, 0), (f32s, 0, 1), (b16, 1, 0), (b16s, 1, 1)):
        refused(fn(n_in=48), b"plane counts: n_in % 64" if bf else b"plane counts: n_in % 32")
        refused(fn(n_out=96), b"plane counts")
        refused(fn(vol=64), b"bad sizes")
        refused(fn(V=-1), b"bad sizes")
        refused(fn(T=100), b"tile_rows: multiple of 16, <= 240")
        refused(fn(T=256), b"tile_rows")
        refused(fn(rows=0), b"null pointer / empty input")
        refused(fn(rows=1 << 23), b"too many input rows")
        refused(fn(n_in=512, rows=G2 // (512 * (2 if bf else 4))), b"buffers must be < 2 GiB")
        refused(fn(V=((G2 - 1) // (28 * 4 + 8 * 27 * 64) + 1) * 128, T=128, vol=27, parts=3) if split else
                fn(V=((G2 - 1) // (28 * 4 + 8 * 27 * 64) + 1) * 128, T=128, vol=27), b"buffers must be < 2 GiB")
        refused(fn(n_in=4096, n_out=4224 if bf else 2112, vol=63), b"packed weights must be < 2 GiB")
        refused(fn(n_in=320 if bf else 160), b"n_in above 256 must be" if bf else b"n_in above 128 must be")
        if split:
            for parts in (0, 1, 33, 9):
                refused(fn(parts=parts), b"2 <= parts <= min(32, vol)")
            refused(fn(scratch=None), b"16-byte aligned scratch")
            refused(fn(scratch=one + 4), b"16-byte aligned scratch")
            assert fn(V=0, parts=3) == 0                 # nothing to do
        else:
            refused(fn(T=48, stats=one), b"statistics need tiles of >= 64 rows")
            refused(fn(stats=one + 4), b"statistics need")
            assert fn(V=0) == 0
    refused(f32s(n_in=32), SPLIT32_MSG.encode())         # the new refusal: no 32-channel split instance
    assert b"aabr_conv_forward_wide_split:" in lib.aabr_last_error()
    if not lib.aabr_build_flags() & 1:
        refused(f32(n_in=128, flags=256), b"`make DEV=1` build only")
    else:
        refused(f32(n_in=64, flags=256), b"debug variants exist for n_in >= 128 only")
    # null pointers are no error when there is nothing to do, and an error otherwise
    assert lib.aabr_conv_forward_wide(None, 64, 0, None, 64, 0, None, 64, 8, None, 0, None, None) == 0
    refused(lib.aabr_conv_forward_wide(None, 64, 170, one, 64, 150, one, 64, 8, None, 0, one, None), b"null pointer")
    refused(lib.aabr_conv_forward_wide(one + 4, 64, 170, one, 64, 150, one, 64, 8, None, 0, one, None), b"16-byte aligned")
    refused(lib.aabr_conv_forward_wide_res(one, 64, 170, one, 64, 150, one, 64, 8, None, 0, one, one + 8, None),
            b"residual must be 16-byte aligned")
    refused(lib.aabr_conv_forward_wide_split_bf16_res(one, 64, 170, one, 64, 150, one, 64, 8, None, 0, one, 3, one, one + 4,
                                                      None), b"residual must be 8-byte aligned")
