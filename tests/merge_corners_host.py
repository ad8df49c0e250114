"""csrc/merge_corners.h compiled for the host (tests/merge_corners_host_harness.cpp) on numpy arrays, and the hand-built
scenes that tests/test_merge_corners_host.py (harness against restatement) and tests/test_gpu_merge_corners.py (kernel
against restatement) share.

A wall is built from its two end points: yx_zb [xc, yc, z_bottom, thickness, length, height, yaw - pi/2], a wall along +x
has yaw - pi/2 = -pi/2 (the unrotated branch of yxzb_to_2corners), one along +y has 0.  Its top corners sit half a thickness
inside the end points, so k wall ends meeting at one point give k corners on a circle of radius thickness / 2 around it:
with the thickness 0.08 used here every pair is at most 0.08 apart, 0.02 under the threshold 0.1."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
TH = 0.08


def build_harness(tmp_path):
    so = str(tmp_path / "libhostmerge.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so,
                           os.path.join(HERE, "merge_corners_host_harness.cpp")])
    L = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.host_merge_scene.restype = C.c_int64
    L.host_merge_scene.argtypes = [fp, C.c_void_p, C.c_int64, C.c_int64, C.c_float, fp, ip, ip]
    return L


class Host(object):
    def __init__(self, lib):
        self.lib = lib
        self.max_walls = int(lib.host_merge_max_walls())

    def merge_scene(self, boxes, labels=None, threshold=0.1, wall_label=1):
        """-> (boxes out [n, 7], merged [n, 2], |S| of the merging steps [2 W]); ValueError beyond the built limit"""
        boxes = np.ascontiguousarray(boxes, F).reshape(-1, 7)
        n = boxes.shape[0]
        lab = None if labels is None else np.ascontiguousarray(labels, np.int64)
        out, merged, steps = np.empty_like(boxes), np.zeros((n, 2), np.int32), np.zeros(2 * n + 1, np.int32)
        W = self.lib.host_merge_scene(boxes, None if lab is None else lab.ctypes.data, n, wall_label, threshold, out,
                                      merged, steps)
        if W < 0:
            raise ValueError("scene beyond the built limit of %d walls" % self.max_walls)
        return out, merged, steps[:2 * W if W > 1 else 0]


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def wall(p, q, th=TH, z0=0.0, h=2.5):
    """the wall whose bottom centre line runs from p to q"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    d = q - p
    if d[1] == 0:
        yaw = -np.pi / 2                                     # along x: the unrotated branch
    elif d[0] == 0:
        yaw = 0.0
    else:
        yaw = (-np.arctan2(d[1], d[0])) % np.pi - np.pi / 2
    c = (p + q) / 2
    return np.array([c[0], c[1], z0, th, np.hypot(*d), h, yaw], F)


def wall_between_top_corners(u, v, th=TH, **kw):
    """the wall whose two top corners, pulled in by half the thickness, sit at u and v"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    e = (v - u) / np.hypot(*(v - u))
    return wall(u - e * th / 2, v + e * th / 2, th, **kw)


def star(centre, k, length=3.0, phase=0.1, **kw):
    """k walls that end at one point, evenly spread: one group of k corners"""
    c = np.asarray(centre, np.float64)
    return [wall(c, c + length * np.array([np.cos(phase + 2 * np.pi * j / k), np.sin(phase + 2 * np.pi * j / k)]), **kw)
            for j in range(k)]


def rooms(gx, gy, size=4.0, jitter=0.0, seed=0, **kw):
    """the south and the west wall of every room of a gx x gy grid: 2 gx gy walls, L, T and cross joints"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(gx):
        for j in range(gy):
            o = np.array([size * i, size * j])
            for e in (np.array([size, 0.0]), np.array([0.0, size])):
                b = wall(o, o + e, **kw)
                b[0:2] += rng.uniform(-jitter, jitter, 2).astype(F)
                out.append(b)
    return out


def _scene(walls, others=(), order=None, seed=0):
    """walls (label 1) and other rows (labels 2, 3) -> (boxes [n, 7], labels [n]); order: a permutation, None: walls first"""
    rows = [np.asarray(w, F) for w in walls] + [np.asarray(o, F) for o in others]
    labels = [1] * len(walls) + [2 + (k % 2) for k in range(len(others))]
    if order is not None:
        rows, labels = [rows[k] for k in order], [labels[k] for k in order]
    return np.array(rows, F).reshape(-1, 7), np.array(labels, np.int64)


def other_rows(n, seed):
    rng = np.random.default_rng(seed)
    b = rng.uniform(-5, 5, (n, 7)).astype(F)
    b[:, 3:6] = np.abs(b[:, 3:6]) + F(0.1)
    return b


def hand_built_scenes():
    """name -> (boxes, labels) in a fixed order; every scene keeps each distance it meets >= 1e-3 off the threshold 0.1"""
    S = {}
    S["no rows"] = (np.zeros((0, 7), F), np.zeros(0, np.int64))
    S["no wall"] = _scene([], other_rows(5, 1))
    S["one wall"] = _scene([wall((0, 0), (3, 1), z0=0.3)], other_rows(2, 2), order=[1, 0, 2])
    S["L"] = _scene([wall((0, 0), (4, 0)), wall((0, 0), (0, 3), z0=0.02)])
    S["T"] = _scene([wall((-3, 0), (0, 0)), wall((0, 0), (4, 0)), wall((0, 0), (0, -3), h=2.52)])
    S["cross"] = _scene([wall((-3, 1), (0, 1)), wall((0, 1), (4, 1)), wall((0, 1), (0, -3)), wall((0, 1), (0.5, 5))])
    S["six"] = _scene(star((1, 2), 6, z0=0.1))
    # the skip: two short walls beside the end of a long one.  Every step at one of the five near corners meets a WHOLE
    # other wall, so none merges although every S has more than one member
    e = np.array([2.0, 0.0])
    S["skip"] = _scene([wall_between_top_corners((-2, 0), e), wall_between_top_corners(e + (0.02, 0.03), e + (0.05, 0.04)),
                        wall_between_top_corners(e + (0.02, -0.03), e + (0.05, -0.04))])
    # the chain: top corners a, b, c on a line at 0, 0.08, 0.16 -- |ab|, |bc| < 0.1 < |ac|.  The walls leave in three
    # directions; the step at a moves a and b to 0.04, which puts b 0.12 from c
    S["chain"] = _scene([wall_between_top_corners((0, 0), (-1, 3)), wall_between_top_corners((0.08, 0), (0.5, -3)),
                         wall_between_top_corners((0.16, 0), (1.5, 3))])
    n_w = len(rooms(3, 2))
    order = np.random.default_rng(5).permutation(n_w + 9)
    others = other_rows(9, 3)
    others[0, 0], others[1, 6] = F(-0.0), F(np.nan)         # copied bit for bit whatever they hold
    S["interleaved"] = _scene([np.concatenate([w[:2], [0.002 * k], w[3:]]) for k, w in enumerate(rooms(3, 2, jitter=0.003))],
                              others, order=order)
    S["300 walls"] = _scene(rooms(15, 10, jitter=0.003, seed=7), other_rows(4, 4))
    return S


def limit_scene(max_walls):
    """a scene of exactly max_walls rows, all of them walls (a 32 x 32 grid of rooms for 2048)"""
    g = int(round((max_walls / 2) ** 0.5))
    assert 2 * g * g == max_walls
    return _scene(rooms(g, g, jitter=0.003, seed=9))
