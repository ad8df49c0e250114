"""Generate tests/golden/merge_corners_golden.npz by RUNNING the reference's own merge_walls_by_corners
(maskrcnn_benchmark/structures/bounding_box_3d.py:850-923) on the CPU, on the reference's own BoxList3D.  Build container
only (needs /root/reference); the committed fixture is data only: the inputs and what the reference computed.

The module file is loaded on its own, with the placeholders of gen_corner_golden.py (numba / spconv decorator-only modules,
open3d, open3d_util, `np.float = float`).  Its line 863, `mask - torch.eye(n, dtype=torch.uint8)`, subtracts from a bool
tensor, which the torch of this container refuses; the value is never read afterwards.  The module's `torch` name is
therefore a stand-in that forwards every attribute to torch except
  * `eye`, which returns an object whose reflected subtraction gives back the left operand: the dead statement then has
    no effect, and
  * `nonzero`, which records what it returns: inside merge_walls_by_corners that is S of every step in order (line 871)
    and, last, the merged corners (line 900).
While the function runs, torch.Tensor.norm records the result of every call on a [n, 3] tensor over dim 1: the distances
of every step (line 867).  Nothing of the reference is edited or copied.

Two sets of scenes (one BoxList3D of walls each, threshold 0.1):
  A  every merged group has at most 4 corners: the means are then bit-equal to an ascending fp32 sum.  Walls along x and y
     only, so that yx_zb -> two corners is the same fp32 operations in the reference and in csrc/corner_box.h (a rotated
     wall goes through fp32 sin / cos in the one and fp64 in the other); z_bottom and height are small dyadic numbers, so
     that the scene's z0 mean (torch's own summation order over W values) is exact in any order.
  B  groups of 5 to 8 corners (stars of walls), any yaw.
Asserted for both: no distance met during the loop lies within 1e-4 of the threshold; no wall collapses to a point (its
two corners stay at least 0.5 apart); set A has no group above 4 and set B has one of every size 5 .. 8."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_iou_golden as G  # noqa: E402
import merge_corners_host as H  # noqa: E402  (scene builders only)

REF = "/root/reference"
THRESHOLD = 0.1
F = np.float32


class _Absorb(object):
    def __rsub__(self, other):
        return other


class _TorchStandIn(object):
    def __init__(self):
        self.nonzero_results = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def eye(self, *a, **k):
        return _Absorb()

    def nonzero(self, *a, **k):
        r = torch.nonzero(*a, **k)
        self.nonzero_results.append(r.reshape(-1).numpy().copy())
        return r


def load_reference():
    G._install_placeholders()
    np.float = float
    sys.modules["open3d"] = types.ModuleType("open3d")
    o3u = types.ModuleType("open3d_util")
    o3u.draw_cus = o3u.gen_animation = None
    sys.modules["open3d_util"] = o3u
    sys.path.insert(0, REF)
    importlib.import_module("utils3d.bbox3d_ops_torch")
    spec = importlib.util.spec_from_file_location("ref_bounding_box_3d",
                                                  os.path.join(REF, "maskrcnn_benchmark/structures/bounding_box_3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stand_in = _TorchStandIn()
    mod.torch = stand_in
    return mod, stand_in


def run_reference(mod, stand_in, walls):
    """-> (input rows as the reference's list holds them, rebuilt rows, S per step, merged corners, distances per step)"""
    bl = mod.BoxList3D(torch.from_numpy(walls.copy()), None, "yx_zb", None, {})
    inp = bl.bbox3d.numpy().copy()
    del stand_in.nonzero_results[:]
    dists = []
    norm0 = torch.Tensor.norm

    def norm(self, *a, **k):
        r = norm0(self, *a, **k)
        if self.dim() == 2 and self.shape[1] == 3 and k.get("dim") == 1:
            dists.append(r.numpy().copy())
        return r

    torch.Tensor.norm = norm
    try:
        out = mod.merge_walls_by_corners(bl, threshold=THRESHOLD)
    finally:
        torch.Tensor.norm = norm0
    W = len(walls)
    assert len(stand_in.nonzero_results) == 2 * W + 1 and len(dists) == 2 * W
    return inp, out.bbox3d.numpy().copy(), stand_in.nonzero_results[:-1], stand_in.nonzero_results[-1], dists


def dyadic(walls, rng):
    """z_bottom a multiple of 1/64 in [0, 1/16], height 2.5 + a multiple of 1/64 in [0, 1/16]"""
    out = []
    for w in walls:
        w = np.array(w, F)
        w[2] = rng.integers(0, 5) / 64.0
        w[5] = 2.5 + rng.integers(0, 5) / 64.0
        out.append(w)
    return np.array(out, F)


def scenes_a():
    rng = np.random.default_rng(31)
    S = [dyadic(H.rooms(3, 3, jitter=0.004, seed=1), rng), dyadic(H.rooms(2, 4, size=3.0, jitter=0.004, seed=2), rng),
         dyadic([H.wall((0, 0), (4, 0)), H.wall((0, 0), (0, 3))], rng),
         dyadic([H.wall((-3, 0), (0, 0)), H.wall((0, 0), (4, 0)), H.wall((0, 0), (0, -3))], rng),
         dyadic([H.wall((0, 0), (5, 0))], rng)]
    return S


def scenes_b():
    S = []
    for k, (k1, k2) in enumerate(((5, 8), (6, 7))):
        walls = H.star((0.3 * k, 1.0), k1, phase=0.1 + 0.2 * k, z0=0.1) + H.star((20.0, -3.0), k2, phase=0.25, z0=0.13)
        walls += [H.wall((8, 8), (12, 8), z0=0.1), H.wall((8, 8), (8, 11), z0=0.1)]
        order = np.random.default_rng(40 + k).permutation(len(walls))
        S.append(np.array([walls[j] for j in order], F))
    return S


def main():
    mod, stand_in = load_reference()
    out = {"threshold": np.float64(THRESHOLD)}
    for name, scenes in (("a", scenes_a()), ("b", scenes_b())):
        out["%s_scenes" % name] = np.int64(len(scenes))
        sizes = set()
        for si, walls in enumerate(scenes):
            inp, res, steps, merged, dists = run_reference(mod, stand_in, walls)
            W = len(walls)
            assert np.isfinite(res).all()
            for i, d in enumerate(dists):                 # the conditions under which the comparison's rounding cannot matter
                d = np.delete(d.astype(np.float64), i ^ 1)
                assert (np.abs(d - THRESHOLD) > 1e-4).all(), "a distance within 1e-4 of the threshold"
            assert (res[:, 4] > 0.5).all(), "a wall collapsed"
            flags = np.zeros(2 * W, np.int32)
            flags[merged] = 1
            for s in steps:
                if len(s) > 1:
                    sizes.add(len(s))
            key = "%s%d_" % (name, si)
            out[key + "in"], out[key + "out"], out[key + "merged"] = inp, res, flags.reshape(W, 2)
            out[key + "step_len"] = np.array([len(s) for s in steps], np.int64)
            out[key + "step_ids"] = np.concatenate(steps).astype(np.int64) if steps else np.zeros(0, np.int64)
        print("set", name, "group sizes met", sorted(sizes))
        if name == "a":
            assert max(sizes) <= 4 and {2, 3, 4} <= sizes
        else:
            assert {5, 6, 7, 8} <= sizes
    np.savez_compressed(os.path.join(HERE, "merge_corners_golden.npz"), **out)
    print("wrote merge_corners_golden.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
