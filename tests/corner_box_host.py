"""csrc/corner_box.h compiled for the host (tests/corner_box_host_harness.cpp) and its four functions on numpy arrays:
shared by tests/test_corner_box_host.py (against the reference's vectors) and tests/test_gpu_corner_head.py (bit-equal to
the list kernels)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLIP = 10000.0


def build_harness(tmp_path):
    """csrc/corner_box.h for the host, as a shared library """
    so = str(tmp_path / "libhostcorner.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so,
                           os.path.join(HERE, "corner_box_host_harness.cpp")])
    L = C.CDLL(so)
    p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    L.host_box_to_2corners.argtypes = [p, C.c_int64, p]
    L.host_box_from_2corners.argtypes = [p, C.c_int64, p]
    L.host_box_encode_corner.argtypes = [p, p, C.c_int64, p, p]
    L.host_box_decode_corner.argtypes = [p, p, C.c_int64, C.c_int, p, C.c_float, p]
    return L


class Host(object):
    """the four functions on numpy arrays"""

    def __init__(self, lib):
        self.lib = lib

    def to_2corners(self, b):
        b = np.ascontiguousarray(b, np.float32)
        out = np.empty_like(b)
        self.lib.host_box_to_2corners(b, b.shape[0], out)
        return out

    def from_2corners(self, c):
        c = np.ascontiguousarray(c, np.float32)
        out = np.empty_like(c)
        self.lib.host_box_from_2corners(c, c.shape[0], out)
        return out

    def encode(self, t, a, w):
        t, a = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(a, np.float32)
        out = np.empty_like(t)
        self.lib.host_box_encode_corner(t, a, t.shape[0], np.ascontiguousarray(w, np.float32), out)
        return out

    def decode(self, e, a, w, clip=CLIP):
        e, a = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(a, np.float32)
        out = np.empty_like(e)
        self.lib.host_box_decode_corner(e, a, e.shape[0], e.shape[1] // 7, np.ascontiguousarray(w, np.float32), clip, out)
        return out
