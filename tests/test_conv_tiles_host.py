"""csrc/conv_tiles.h, the 64-row-tile launch decision of aabr_conv_forward / aabr_conv_forward_bf16, compiled for the
host and compared field by field with the rule as the entry points wrote it before (tests/conv_tiles_rule.py) over a
grid of shapes, flags, buffer sizes and tuning knobs; the grid must reach every kernel instance conv.hip compiles, and
the decision must return no other.  Host only: g++, no GPU, no library."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import conv_tiles_rule as R

HERE = os.path.dirname(os.path.abspath(__file__))
U = R.UNSET
NO_KNOBS = (U,) * 6
KNOB_VALUES = {0: (0, 1, 2, 3, 4), 1: (0, 1), 2: (8, 12, 16), 3: (0, 100, 4096), 4: (1, 2, 3, 4), 5: (1, 2, 3, 4, 5)}
TILES = (1, 2, 7, 8, 16, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
         2049, 4095, 4096, 4097, 8191, 8192, 8193)           # 64-row tiles: workgroup counts around 512 / 1024 / 8192
ROWS = sorted({1, 63} | {64 * t + d for t in TILES for d in (-1, 0, 1)})
FP32_PLANES_IN = (9, 16, 32, 33, 48, 64, 80, 96, 128, 256)   # aligned or not; 1, 2 and >= 3 K-chunks
FP32_PLANES_OUT = (9, 16, 32, 48, 64, 96, 256)               # 1, 2, 3 and >= 4 column blocks
BF16_PLANES = (32, 64, 96, 128, 256)
FLAGS = (0, 1, 2, 3, 4, 256, 512 | 3)                        # transpose, flip, prepacked, timing-experiment bits


def _harness(tmp_path):
    so = str(tmp_path / "libhosttiles.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "conv_tiles_host_harness.cpp")])
    lib = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.host_conv_tile_launch.argtypes = [p, C.c_int64, p]
    return lib


def _sizes(n_in, n_out, V, vol, elem, big=None):
    """(in, packed weight, tile block) bytes of a submanifold launch; `big` puts one of them at 2 GiB"""
    b = [V * n_in * elem, vol * R.ceil_div(n_in, 32) * R.ceil_div(n_out, 16) * 512 * elem, V * vol * 4 + 4096]
    if big is not None:
        b[big] = R.G2 + (big == 0)          # exactly 2^31 (and one byte more for the input)
    return tuple(b)


def _cases():
    out = []
    for n_in, n_out, V, vol, flags in itertools.product(FP32_PLANES_IN, FP32_PLANES_OUT, ROWS, (1, 8, 27), FLAGS):
        out.append((0, n_in, n_out, V, vol, flags) + _sizes(n_in, n_out, V, vol, 4) + NO_KNOBS)
    for n_in, n_out, V, vol in itertools.product(BF16_PLANES, BF16_PLANES, ROWS, (1, 8, 27)):
        out.append((1, n_in, n_out, V, vol, 3 * (V & 1)) + _sizes(n_in, n_out, V, vol, 2) + NO_KNOBS)
    few_rows = ROWS[::4] + [64 * 128, 64 * 512, 64 * 2048]
    for n_in, n_out, V, vol, flags in itertools.product((16, 32, 48, 64, 96), (16, 32, 48, 64, 256), few_rows, (1, 27),
                                                        (0, 256)):
        for big in range(3):                # each buffer at 2 GiB
            out.append((0, n_in, n_out, V, vol, flags) + _sizes(n_in, n_out, V, vol, 4, big) + NO_KNOBS)
        out.append((0, n_in, n_out, V, vol, flags) + (R.G2 - 1, R.G2 - 1, R.G2 - 1) + NO_KNOBS)
        for k, values in KNOB_VALUES.items():
            for v in values:
                knobs = tuple(v if i == k else U for i in range(6))
                out.append((0, n_in, n_out, V, vol, flags) + _sizes(n_in, n_out, V, vol, 4) + knobs)
                if n_in % 32 == 0 and n_out % 32 == 0 and not flags:
                    out.append((1, n_in, n_out, V, vol, 3) + _sizes(n_in, n_out, V, vol, 2) + knobs)
    return out


def test_tile_decision_matches_rule_and_reaches_every_compiled_instance(tmp_path):
    lib = _harness(tmp_path)
    cases = _cases()
    a = np.array(cases, np.int64)
    got = np.zeros((len(cases), 11), np.int64)
    lib.host_conv_tile_launch(a, len(cases), got)
    reached = {}
    for c, g in zip(cases, got.tolist()):
        want = (R.bf16 if c[0] else R.fp32)(*c[1:9], c[9:])
        assert tuple(g) == want, (c, R.name(g), R.name(want), g, want)
        reached[want[:7]] = reached.get(want[:7], 0) + 1
    compiled = R.compiled_instances()
    assert len(compiled) == len(set(compiled)) == 61
    missing = set(compiled) - set(reached)
    assert not missing, sorted(R.name(k) for k in missing)
    extra = set(reached) - set(compiled)
    assert not extra, sorted(R.name(k) for k in extra)


def test_instance_names_are_the_ones_profiles_key_on():
    """spot checks of the name format (bench.py and the committed PMC records look kernels up by these strings)"""
    names = {R.name(k) for k in R.compiled_instances()}
    for n in ("k_conv_blocks_mfma_small<16>", "k_conv_blocks_mfma_small<8>", "k_conv_blocks_mfma_buf<1,4,true,true>",
              "k_conv_blocks_mfma_buf<2,4,true,false>", "k_conv_blocks_mfma_bf16<2,4,4,true>",
              "k_conv_blocks_mfma_bf16<4,2,1,true>", "k_conv_blocks_mfma_wpipe<4,3,true,false>",
              "k_conv_blocks_mfma_wlds<1,2,true>", "k_conv_blocks_mfma<2,4,false>", "k_conv_blocks_mfma<4,3,true>"):
        assert n in names, n
