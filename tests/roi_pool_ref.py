"""The multi-level ROI pooler's box arithmetic restated with torch on the CPU in float32, and the per-level composition on
numpy index sets.  The yardstick of tests/test_roi_pool_host.py and tests/test_gpu_roi_pool.py for k_roi_pool_prepare
(csrc/roi_pool.hip); tests/golden/pooler_golden.npz (made by the reference's own classes) pins this restatement.

The expressions are the reference's, in its order, with its Python scalars (CPU torch divides by a scalar as a true
division in float32):
  FPN2MLPFeatureExtractor.convert_metric_to_pixel   modeling/roi_heads/box_head_3d/roi_box_feature_extractors.py:108-114
  BoxList3D.convert('standard')                     structures/bounding_box_3d.py:293-312
  BoxList3D.__init__ -> OBJ_DEF.limit_yaw           structures/bounding_box_3d.py:203, utils3d/geometric_torch.py:4-10,88-97
  Pooler.convert_to_roi_format                      modeling/poolers_3d.py:107-124
  LevelMapper_3d.__call__                           modeling/poolers_3d.py:57-69
The pooling itself is not restated here: tests/roi_align_ref.py is its fp64 yardstick, applied per level."""
import math

import numpy as np
import torch

F = np.float32


def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


def rois_and_levels(boxes, box_scale, scales, canonical_size):
    """boxes: list over scenes of [n_b, 7] float32 arrays (yx_zb) -> (rois [N, 8] float32, levels [N] int64)"""
    props = []
    for b in boxes:
        t = torch.from_numpy(np.ascontiguousarray(b, F).reshape(-1, 7)).clone()
        t[:, 0:6] *= box_scale                                            # convert_metric_to_pixel
        props.append(t)
    std = []
    for bbox3d0 in props:                                                 # convert('standard')
        bbox3d1 = bbox3d0[:, [0, 1, 2, 4, 3, 5, 6]]
        bbox3d1[:, 2] += bbox3d0[:, 5] * 0.5
        bbox3d1[:, -1] += math.pi * 0.5
        bbox3d1[:, -1] = limit_period(bbox3d1[:, -1], 0, math.pi)        # the constructor's limit_yaw, standard mode
        std.append(bbox3d1)
    concat = torch.cat(std, dim=0)
    ids = torch.cat([torch.full((len(b), 1), i, dtype=concat.dtype) for i, b in enumerate(std)], dim=0)
    rois = torch.cat([ids, concat], dim=1)
    rois = rois[:, [0, 2, 1, 3, 5, 4, 6, 7]]
    rois[:, -1] *= 180.0 / math.pi
    size = torch.sqrt(torch.cat([b[:, 3:5].max(dim=1)[0] for b in props]))  # LevelMapper_3d
    rate = size / canonical_size
    dif = torch.abs(torch.tensor(scales)[None, :] - rate[:, None])
    levels = torch.argmin(dif, 1)
    return rois.numpy(), levels.numpy().astype(np.int64)


def level_sets(levels, n_levels):
    """the rows of each level, ascending: what torch.nonzero(levels == l) yields in the reference's loop"""
    levels = np.asarray(levels)
    return [np.nonzero(levels == l)[0] for l in range(n_levels)]


def compose(levels, per_level, n_levels, tail_shape, dtype=F):
    """the reference's indexed writes: result[idx_l] = per_level[l] into a zero-filled [N, ...]"""
    out = np.zeros((len(levels),) + tuple(tail_shape), dtype)
    for idx, part in zip(level_sets(levels, n_levels), per_level):
        out[idx] = part
    return out


# ------------------------------------------------------------------------------------------------ inputs of the GPU cases
# shared by the host test (the fp64 yardstick's undecided share per level) and tests/test_gpu_roi_pool.py
FRAME = (48, 40, 12)                     # the box frame (x, y, z) the three levels' scales refer to
EXTENTS = ((24, 20, 6), (12, 10, 3), (6, 5, 2))
SCALES = (0.5, 0.25, 0.125)
CANONICAL = 10.0
BATCH = 2


def _sizes(rng, n):
    """two sizes in [1, 36] per box; the larger one is u * u, u uniform in [1, 6], so that sqrt(max) / CANONICAL is uniform
    over [0.1, 0.6] and lands on all three scales (about 45 / 37 / 17 %)"""
    big = rng.uniform(1.0, 6.0, n) ** 2
    small = rng.uniform(1.0, big)
    swap = rng.random(n) < 0.5
    return np.where(swap, small, big).astype(F), np.where(swap, big, small).astype(F)


def random_boxes(rng, n, skip_level=None, z_inside=False):
    """n yx_zb boxes over FRAME: centres inside it with a small margin outside, sizes as _sizes draws them.
    `skip_level`: redraw the sizes until no box maps to that level.  `z_inside`: bottoms in [0, 6] and heights in [1, 4],
    so that on every level of EXTENTS no sample lies above the map (level 0: top <= 10 * 0.5 <= 6 cells; levels 1 and 2:
    the height is raised to one cell, top <= 8 * 0.25 + 0.5 <= 3 and 8 * 0.125 + 0.5 <= 2)."""
    b = np.zeros((n, 7), F)
    b[:, 0] = rng.uniform(-2, FRAME[0] + 2, n)
    b[:, 1] = rng.uniform(-2, FRAME[1] + 2, n)
    b[:, 2] = rng.uniform(-1, FRAME[2] - 2, n)
    b[:, 3], b[:, 4] = _sizes(rng, n)
    b[:, 5] = rng.uniform(1.0, 8.0, n)
    b[:, 6] = rng.uniform(-math.pi / 2, math.pi / 2, n)
    if z_inside:
        b[:, 2] = rng.uniform(0.0, 6.0, n)
        b[:, 5] = rng.uniform(1.0, 4.0, n)
    if skip_level is not None:
        for _ in range(100):
            _, lv = rois_and_levels([b], 1.0, SCALES, CANONICAL)
            bad = lv == skip_level
            if not bad.any():
                break
            b[bad, 3], b[bad, 4] = _sizes(rng, int(bad.sum()))
        assert not bad.any()
    return b


class PoolCase(object):
    """one input set: per-level sites / features (numpy, built like roi_align_ref.make_sites), the scenes' boxes"""

    def __init__(self, name, seed, C, out_size, sampling, counts, skip_level=None, z_inside=False):
        import roi_align_ref as R
        self.name, self.seed, self.C, self.out_size, self.sampling = name, seed, C, tuple(out_size), sampling
        self.counts, self.skip_level = tuple(counts), skip_level
        rng = np.random.default_rng(seed)
        self.sites = [R.make_sites(rng, BATCH, h, w, z, 1.0 / 6) for (h, w, z) in EXTENTS]
        self.feats = [rng.standard_normal((len(s), C)).astype(F) for s in self.sites]
        self.boxes = [random_boxes(rng, n, skip_level=skip_level, z_inside=z_inside) for n in counts]
        self.rois, self.levels = rois_and_levels(self.boxes, 1.0, SCALES, CANONICAL)
        self._ref = None

    @property
    def n(self):
        return sum(self.counts)

    def grad(self):
        return np.random.default_rng(self.seed + 1000).standard_normal((self.n, self.C) + self.out_size).astype(F)

    def dense(self, l):
        h, w, z = EXTENTS[l]
        d = np.zeros((BATCH, self.C, h, w, z), F)
        s = self.sites[l]
        d[s[:, 3], :, s[:, 0], s[:, 1], s[:, 2]] = self.feats[l]
        return d

    def reference(self):
        """per level (index set, forward Result, backward Result) of roi_align_ref on that level's ROI subset; computed once"""
        import roi_align_ref as R
        if self._ref is None:
            g = self.grad()
            ref = []
            for l, idx in enumerate(level_sets(self.levels, len(SCALES))):
                h, w, z = EXTENTS[l]
                rf = R.forward(self.dense(l), self.rois[idx], SCALES[l], self.out_size, self.sampling)
                rb = R.backward(g[idx], self.rois[idx], SCALES[l], self.out_size, (BATCH, self.C, h, w, z), self.sampling)
                ref.append((idx, rf, rb))
            self._ref = ref
        return self._ref


_CASES = None


def gpu_cases():
    """C in {5, 130}; outputs (4, 6, 5) = 120 bins (two LDS passes, the second partial) and (2, 3, 2); sampling 2 and 0;
    scene counts (23, 17) and (0, 9); one case where no ROI maps to the middle level.  Built once per process."""
    global _CASES
    if _CASES is None:
        _CASES = [
            PoolCase("c5_120bins_s2", 311, 5, (4, 6, 5), 2, (23, 17)),
            PoolCase("c130_12bins_s2", 312, 130, (2, 3, 2), 2, (23, 17)),
            PoolCase("c130_120bins_adaptive", 313, 130, (4, 6, 5), 0, (0, 9)),
            PoolCase("c5_12bins_adaptive_empty_scene", 314, 5, (2, 3, 2), 0, (0, 9)),
            PoolCase("c5_no_middle_level", 315, 5, (2, 3, 2), 2, (23, 17), skip_level=1),
        ]
    return _CASES


_ADJOINT = None


def adjoint_case():
    """the adjoint identity's inputs: no sample above the map (there the forward pass reads the last slice and the backward
    pass adds nothing, so the pair is not adjoint by definition)"""
    global _ADJOINT
    if _ADJOINT is None:
        _ADJOINT = PoolCase("adjoint", 330, 7, (3, 2, 2), 2, (14, 10), z_inside=True)
    return _ADJOINT
