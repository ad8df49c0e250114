"""csrc/conv_dw_tiles.h, the gather form of the weight gradient's 64 x 64-block kernel (dw_vec_operands: which operand rows
k_conv_dw_pairs<cb, nb, float> loads with one 16- / 8-byte instruction per lane) and the maps from an accumulator register
back to its channel (dw_tile_row / dw_tile_col), compiled for the host and compared with the rule restated here.
Host only: g++, no GPU, no library."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "conv_dw_vec_host_harness.cpp")
UNSET = -2147483647 - 1
PLANES = (9, 16, 32, 33, 48, 64, 80, 96, 128, 256)
OFFSETS = (0, 4, 8, 16)                                   # bytes off a 16-byte boundary (16: aligned again)
BASE = 0x7F0000001000


def _blocks(planes):
    n = (planes + 15) // 16
    return 4 if n >= 4 else (2 if n >= 2 else 1)


def _rule(bf, n_in, n_out, addr_in, addr_dout, knob):
    """bit 0: input features, bit 1: output gradients.  fp32 storage only; an operand qualifies when every tile of its cb
    (nb) blocks of 16 is full and its address is a multiple of the load's 4 cb (4 nb) bytes; one block: the scalar form"""
    if bf or knob == 0:
        return 0
    cb, nb = _blocks(n_in), _blocks(n_out)
    m = 0
    if cb > 1 and n_in % (16 * cb) == 0 and addr_in % (4 * cb) == 0:
        m |= 1
    if nb > 1 and n_out % (16 * nb) == 0 and addr_dout % (4 * nb) == 0:
        m |= 2
    return m


def _lib(tmp_path):
    so = str(tmp_path / "libhostdwvec.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    p64 = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    p32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.host_dw_vec_operands.argtypes = [p64, C.c_int64, p64]
    lib.host_dw_tile_maps.argtypes = [C.c_int, C.c_int, C.c_int, p32, p32]
    return lib


def test_vec_operands_match_the_rule(tmp_path):
    lib = _lib(tmp_path)
    cases = [(bf, ci, co, BASE + oi, 2 * BASE + oo, kn)
             for bf, ci, co, oi, oo, kn in itertools.product((0, 1), PLANES, PLANES, OFFSETS, OFFSETS, (UNSET, 0, 1))]
    a = np.array(cases, np.int64)
    got = np.zeros((len(cases), 3), np.int64)
    lib.host_dw_vec_operands(a, len(cases), got)
    seen = set()
    for c, g in zip(cases, got.tolist()):
        assert (g[0], g[1]) == (_blocks(c[1]), _blocks(c[2])), (c, g)
        assert g[2] == _rule(*c), (c, g)
        seen.add(g[2])
    assert seen == {0, 1, 2, 3}
    by = {c: g[2] for c, g in zip(cases, got.tolist())}
    # the cases the rule is written around
    assert by[(0, 64, 64, BASE, 2 * BASE, UNSET)] == 3 and by[(0, 128, 128, BASE, 2 * BASE, UNSET)] == 3
    assert by[(0, 32, 32, BASE, 2 * BASE, UNSET)] == 3 and by[(0, 32, 32, BASE + 8, 2 * BASE + 8, UNSET)] == 3   # dwordx2
    assert by[(0, 9, 32, BASE, 2 * BASE, UNSET)] == 2 and by[(0, 96, 64, BASE, 2 * BASE, UNSET)] == 2
    assert by[(0, 48, 80, BASE, 2 * BASE, UNSET)] == 0 and by[(0, 16, 16, BASE, 2 * BASE, UNSET)] == 0
    assert by[(0, 64, 64, BASE + 4, 2 * BASE, UNSET)] == 2 and by[(0, 64, 64, BASE, 2 * BASE + 8, UNSET)] == 1
    assert by[(0, 64, 64, BASE + 16, 2 * BASE + 16, UNSET)] == 3
    assert by[(1, 64, 64, BASE, 2 * BASE, UNSET)] == 0 and by[(0, 64, 64, BASE, 2 * BASE, 0)] == 0


def test_tile_maps_reach_every_channel_once(tmp_path):
    """(g, r, a) -> row and (c16, b) -> column of the tile are bijections in both forms, the scalar form is the MFMA's own
    layout (block a rows 16 a + 4 g + r, block b columns 16 b + c16) and the vector form the loads' (cb (4 g + r) + a,
    nb c16 + b): a lane's nb values of one register are nb consecutive columns"""
    lib = _lib(tmp_path)
    for vec, cb, nb in itertools.product((0, 1), (1, 2, 4), (1, 2, 4)):
        rows, cols = np.full(16 * cb, -1, np.int32), np.full(16 * nb, -1, np.int32)
        lib.host_dw_tile_maps(vec, cb, nb, rows, cols)
        assert sorted(rows.tolist()) == list(range(16 * cb)), (vec, cb, rows)
        assert sorted(cols.tolist()) == list(range(16 * nb)), (vec, nb, cols)
        rows, cols = rows.reshape(4, 4, cb), cols.reshape(16, nb)
        for g, r, a in itertools.product(range(4), range(4), range(cb)):
            assert rows[g, r, a] == (cb * (4 * g + r) + a if vec else 16 * a + 4 * g + r)
        for c16, b in itertools.product(range(16), range(nb)):
            assert cols[c16, b] == (nb * c16 + b if vec else 16 * b + c16)
        if vec:
            assert (np.diff(cols, axis=1) == 1).all()


def test_harness_alone_under_address_and_undefined_sanitizers(tmp_path):
    """the same header through a program of its own (its own main, no Python in the process), built with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "dw_vec_host")
    subprocess.check_call(["g++", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DDW_VEC_HOST_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert "0 violations" in r.stdout, r.stdout
