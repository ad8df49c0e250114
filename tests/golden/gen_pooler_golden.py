"""Generate tests/golden/pooler_golden.npz by IMPORTING the reference's own pooler code and running it on seeded boxes
(build container only; needs the reference tree, /root/reference or $AABR_REFERENCE):

  * maskrcnn_benchmark/modeling/poolers_3d.py:57-69     LevelMapper_3d.__call__
  * maskrcnn_benchmark/modeling/poolers_3d.py:107-124   Pooler.convert_to_roi_format
  * maskrcnn_benchmark/structures/bounding_box_3d.py    BoxList3D.__init__ (limit_yaw) and .convert('standard')
  * utils3d/geometric_torch.py:4-10,88-97               limit_period, OBJ_DEF.limit_yaw

`maskrcnn_benchmark.layers` (compiled extensions) does not import here: an empty placeholder module with a name
`ROIAlignRotated3D` stands in, which nothing below calls.  The multiplication of convert_metric_to_pixel
(roi_box_feature_extractors.py:112, `prop.bbox3d[:, 0:6] *= self.voxel_scale`) is that one line on the reference's BoxList3D;
its class needs a config and the compiled layers.  The boxes are stored AFTER the yx_zb BoxList3D constructor wrapped
their yaws into [-pi/2, pi/2): they are what the pooler receives.  The committed fixture is data only.
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AABR_REFERENCE", "/root/reference")


def _boxes(rng, n, lo, hi):
    """yx_zb boxes whose sqrt(max size) spreads evenly over [sqrt(lo), sqrt(hi)]"""
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-2, 50, (n, 2))
    b[:, 2] = rng.uniform(-1, 10, n)
    big = rng.uniform(math.sqrt(lo), math.sqrt(hi), n) ** 2
    small = rng.uniform(lo, big)
    swap = rng.random(n) < 0.5
    b[:, 3], b[:, 4] = np.where(swap, small, big), np.where(swap, big, small)
    b[:, 5] = rng.uniform(0.5, 8, n)
    b[:, 6] = rng.uniform(-4, 4, n)                                   # the constructor wraps these
    return b


def main():
    sys.path.insert(0, REF)
    importlib.import_module("maskrcnn_benchmark")
    layers = types.ModuleType("maskrcnn_benchmark.layers")
    layers.ROIAlignRotated3D = None
    sys.modules["maskrcnn_benchmark.layers"] = layers
    pool = importlib.import_module("maskrcnn_benchmark.modeling.poolers_3d")
    bb = importlib.import_module("maskrcnn_benchmark.structures.bounding_box_3d")
    assert pool.__file__.startswith(REF) and bb.__file__.startswith(REF)

    def run(scenes, box_scale, scales, canonical_size):
        """scenes: list of [n, 7] arrays -> (boxes as the pooler receives them, rois, levels)"""
        lists = [bb.BoxList3D(torch.from_numpy(s.copy()), None, "yx_zb", None, {"prediction": True}) for s in scenes]
        received = [l.bbox3d.numpy().copy() for l in lists]
        scaled = []
        for l in lists:
            p = bb.BoxList3D(l.bbox3d.clone(), None, "yx_zb", None, {"prediction": True})
            p.bbox3d[:, 0:6] *= box_scale                             # convert_metric_to_pixel
            scaled.append(p)
        rois = pool.Pooler.convert_to_roi_format(None, scaled)
        levels = pool.LevelMapper_3d(scales, canonical_size)(scaled)
        return received, rois.numpy(), levels.numpy().astype(np.int64)

    out = {}
    rng = np.random.default_rng(23)
    h = np.float32(math.pi / 2)
    # a: three levels, canonical size 10, box_scale 1; two scenes and an empty one between them
    s0, s1 = _boxes(rng, 150, 1, 36), _boxes(rng, 100, 1, 36)
    s0[:8, 6] = [0.0, h, -h, np.nextafter(h, np.float32(0)), np.nextafter(-h, np.float32(0)), 2 * h, -2 * h, 1e-7]
    # b: the exact tie (scaled size 9 -> sqrt 3 -> rate 0.375, |0.5 - 0.375| == |0.25 - 0.375|: level 0), a NaN and a
    # negative size (both: every dif is NaN, argmin takes index 0), sizes under both orders of (x, y)
    s2 = _boxes(rng, 60, 1, 30)
    s2[0, 3:5] = (9.0, 4.0)
    s2[1, 3:5] = (2.0, 9.0)
    s2[2, 3:5] = (np.nan, 3.0)
    s2[3, 3:5] = (3.0, np.nan)
    s2[4, 3:5] = (-4.0, -1.0)
    s2[5, 3:5] = (-4.0, 25.0)
    # c: metric boxes and box_scale 50 (SPARSE3D.VOXEL_SCALE)
    s3 = _boxes(rng, 90, 1, 36)
    s3[:, 0:6] /= 50
    s3[:3, 6] = [0.0, h, -h]
    sets = {"a": ([s0, np.zeros((0, 7), np.float32), s1], 1.0, (0.5, 0.25, 0.125), 10),
            "b": ([s2], 1.0, (0.5, 0.25), 8),
            "c": ([s3, s3[::-1][:40].copy()], 50.0, (0.5, 0.25, 0.125), 10.0)}
    for k, (scenes, box_scale, scales, cs) in sets.items():
        received, rois, levels = run(scenes, box_scale, scales, cs)
        out[k + "_boxes"] = np.concatenate(received)
        out[k + "_counts"] = np.array([len(s) for s in scenes], np.int64)
        out[k + "_box_scale"] = np.array(box_scale, np.float64)
        out[k + "_scales"] = np.array(scales, np.float64)
        out[k + "_canonical_size"] = np.array(cs, np.float64)
        out[k + "_rois"], out[k + "_levels"] = rois, levels
        assert set(levels.tolist()) == set(range(len(scales))), (k, np.bincount(levels))
    assert (out["b_levels"][[0, 1, 2, 3, 4]] == 0).all()
    np.savez_compressed(os.path.join(HERE, "pooler_golden.npz"), **out)
    print("wrote pooler_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
