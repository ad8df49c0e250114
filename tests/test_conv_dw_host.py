"""csrc/conv_dw_tiles.h, the weight-gradient launch decision of aabr_conv_backward_weight / aabr_conv_backward_weight_bf16,
compiled for the host and compared field by field with the rule as the entry point wrote it before
(tests/conv_dw_rule.py) over a grid of storage types, plane counts, rule-book sizes, scratch bounds, pointer alignments
and tuning knobs; the grid must reach every kernel instance conv_dw.hip compiles, and the decision must return no other.
Host only: g++, no GPU, no library."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import conv_dw_rule as R

HERE = os.path.dirname(os.path.abspath(__file__))
U = R.UNSET
NO_KNOBS = (U,) * 3
KNOB_VALUES = (0, 1, 8, 300, 512)
PLANES = (9, 16, 32, 33, 48, 64, 80, 96, 128, 256)      # 1, 2 and >= 4 blocks of 16; multiples of 32 / 128 or not
KNOB_PLANES = (96, 128, 256)                             # the knobs steer the full-tile kernels (multiples of 128) only
VOLS = (1, 8, 27)
RULE_ESTIMATES = (150000, 250000, 600000)                # bf16 / fp32 threshold of the full-tile kernels, two workgroups per CU


def _harness(tmp_path):
    so = str(tmp_path / "libhostdw.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "conv_dw_host_harness.cpp")])
    lib = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.host_conv_dw_launch.argtypes = [p, C.c_int64, p]
    return lib


def _r_est(V, vol):
    return V if vol == 1 else vol * V // 3


def _rows(vol):
    """V_out on both sides of every boundary of the rule: direct (V = chunk), the chunk size (vol V = 2^21), the rule
    estimates (the smallest V that reaches each, one below, one above)"""
    vs = {1, 255, 256, 257, 1023, 1024, 1025, (1 << 21) // vol - 1, (1 << 21) // vol, (1 << 21) // vol + 1}
    for t in RULE_ESTIMATES:
        v = t if vol == 1 else 3 * t // vol
        while _r_est(v, vol) < t:
            v += 1
        while _r_est(v - 1, vol) >= t:
            v -= 1
        assert _r_est(v - 1, vol) < t <= _r_est(v, vol)
        vs |= {v - 1, v, v + 1}
    return sorted(vs)


def _max_chunks(V, vol, n_in, n_out):
    """the geometric bound of SCN._Gather.max_chunks, then bounds that leave few or no slots beside the vol spare ones
    (n > slots, n_wg = 0)"""
    c = R.chunk_pairs(V, vol, n_in, n_out)
    return [R.ceil_div(vol * V, c) + vol] + [vol + s for s in (0, 1, 7, 8, 63, 64, 255, 256, 300, 512)]


def _cases():
    out = []
    for bf, n_in, n_out, vol, al in itertools.product((0, 1), PLANES, PLANES, VOLS, (0, 1)):
        knobbed = n_in in KNOB_PLANES and n_out in KNOB_PLANES
        for V in _rows(vol):
            for mc in _max_chunks(V, vol, n_in, n_out):
                out.append((bf, n_in, n_out, V, vol, mc, al) + NO_KNOBS)
                if knobbed:
                    for k, v in itertools.product(range(3), KNOB_VALUES):
                        out.append((bf, n_in, n_out, V, vol, mc, al) + tuple(v if i == k else U for i in range(3)))
            if knobbed:                       # the precedence: DW_FULL = 0 over all, DW_FULL_WGS over DW_FULL_MIN
                mc = _max_chunks(V, vol, n_in, n_out)[0]
                for kn in ((0, 8, 8), (1, 8, 300), (U, 8, 300), (U, 300, 8), (1, 1, U), (0, U, 8)):
                    out.append((bf, n_in, n_out, V, vol, mc, al) + kn)
    return out


def test_dw_decision_matches_rule_and_reaches_every_compiled_instance(tmp_path):
    lib = _harness(tmp_path)
    cases = _cases()
    a = np.array(cases, np.int64)
    got = np.zeros((len(cases), 12), np.int64)
    lib.host_conv_dw_launch(a, len(cases), got)
    reached = {}
    for c, g in zip(cases, got.tolist()):
        want = R.decide(*c[:7], c[7:])
        assert tuple(g) == want, (c, R.name(g), R.name(want), g, want)
        reached[want[:4]] = reached.get(want[:4], 0) + 1
    compiled = R.compiled_instances()
    assert len(compiled) == len(set(compiled)) == 24
    missing = set(compiled) - set(reached)
    assert not missing, sorted(R.name(k) for k in missing)
    extra = set(reached) - set(compiled)
    assert not extra, sorted(R.name(k) for k in extra)
    # every form of the launch was reached too: direct, chunked + reduce at both chunk sizes, ranges with 1 and 2 per CU
    forms = {(g[4], g[5], g[9]) for g in got.tolist()}
    assert forms == {(256, 1, 0), (1024, 1, 0), (256, 0, 1), (1024, 0, 1), (1024, 0, 2)}, forms
    assert {256, 512} <= {g[8] * g[7] for g in got.tolist() if g[0] == R.KINDS.index("full")}


def test_instance_names_are_the_ones_profiles_key_on():
    """the name format (bench.py and the committed profiles look kernels up by these strings)"""
    names = [R.name(k) for k in R.compiled_instances()]
    assert len(set(names)) == 24
    for n in ("k_conv_dw_pairs<4,2,float>", "k_conv_dw_pairs<2,1,bf16>", "k_conv_dw_pairs_bf16<2,4>", "k_conv_dw_full_f32",
              "k_conv_dw_full_bf16", "k_conv_dw_pairs<1,1,float>", "k_conv_dw_pairs<4,4,bf16>", "k_conv_dw_pairs_bf16<4,4>"):
        assert n in names, n
