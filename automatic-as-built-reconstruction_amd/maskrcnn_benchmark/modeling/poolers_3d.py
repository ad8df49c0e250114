"""Multi-level ROI pooler of the box head (reference: maskrcnn_benchmark/modeling/poolers_3d.py:57-168, LevelMapper_3d
and Pooler; its FPN-paper LevelMapper ends in a breakpoint, is unused, and is not part of this package).

`Pooler.forward(x, boxes)`: x = one SparseConvNetTensor per level, boxes = one list of proposals per scene, duck-typed as
in PostProcessor.forward (`.bbox3d` [n, 7] yx_zb).  `fused = True` (the default) is roi_glue.pool_rois: ROI rows and
levels in one launch, every level's gather in a second one, no host read.  `fused = False` is the reference's loop --
torch expressions for the ROI rows and the levels, then per level nonzero / ROIAlignRotated3D / indexed write into a
zero-filled result -- kept as the yardstick and the A/B switch, like ROIAlignRotated3D.fused.
`pooled_dtype` (torch.float32, the default, or torch.bfloat16) is the storage of the result: the fused form writes bf16
from its gather launch (roi_glue.pool_rois(pooled_dtype=...)), the loop casts its fp32 result once -- the same bytes.

`box_scale` is an extension: the reference multiplies the boxes by SPARSE3D.VOXEL_SCALE in the feature extractor
(convert_metric_to_pixel) before it calls the pooler; here the pooler can take the metric boxes and do it in the same
launch.  1.0 (the default) is the reference's Pooler."""
import math

import torch
from torch import nn

import roi_glue
from maskrcnn_benchmark.layers.roi_align_rotated_3d import ROIAlignRotated3D


def _bbox3d(boxes):
    return [b.bbox3d for b in boxes]


def torch_rois_and_levels(bbox3d, scales, canonical_size, box_scale=1.0):
    """the reference's torch expressions on whichever device the boxes live on: convert_metric_to_pixel,
    BoxList3D.convert('standard') + limit_yaw, Pooler.convert_to_roi_format, LevelMapper_3d.__call__.  The two divisors are
    0-dim tensors on the boxes' device, so that a GPU evaluates true divisions as the CPU does (it multiplies by the
    reciprocal of a Python scalar)."""
    dev = bbox3d[0].device
    boxes = []
    for b in bbox3d:
        b = b.detach().to(torch.float32).clone()
        b[:, 0:6] *= box_scale
        boxes.append(b)
    std = []
    for b in boxes:
        s = b[:, [0, 1, 2, 4, 3, 5, 6]]
        s[:, 2] += b[:, 5] * 0.5
        s[:, -1] += math.pi * 0.5
        period = torch.tensor(math.pi, dtype=torch.float32, device=dev)
        s[:, -1] = s[:, -1] - torch.floor(s[:, -1] / period + 0) * period
        std.append(s)
    concat = torch.cat(std, dim=0)
    ids = torch.cat([torch.full((len(b), 1), i, dtype=concat.dtype, device=dev) for i, b in enumerate(std)], dim=0)
    rois = torch.cat([ids, concat], dim=1)
    rois = rois[:, [0, 2, 1, 3, 5, 4, 6, 7]]
    rois[:, -1] *= 180.0 / math.pi
    size = torch.sqrt(torch.cat([b[:, 3:5].max(dim=1)[0] for b in boxes]))
    rate = size / torch.tensor(float(canonical_size), dtype=torch.float32, device=dev)
    dif = torch.abs(torch.tensor(scales, dtype=torch.float32, device=dev)[None, :] - rate[:, None])
    return rois, torch.argmin(dif, 1)


class LevelMapper_3d(object):
    def __init__(self, scales, canonical_size):
        self.scales = torch.tensor(scales)
        self.canonical_size = canonical_size

    def __call__(self, boxlists):
        _rois, levels = roi_glue.roi_rows_and_levels(_bbox3d(boxlists), self.scales.tolist(), self.canonical_size)
        return levels.to(torch.int64)


class Pooler(nn.Module):
    def __init__(self, output_size, scales, sampling_ratio, canonical_size, canonical_level=None, box_scale=1.0):
        super(Pooler, self).__init__()
        if not 1 <= len(scales) <= roi_glue.POOL_MAX_LEVELS:
            raise ValueError("1 .. %d levels, got %d" % (roi_glue.POOL_MAX_LEVELS, len(scales)))
        self.poolers = nn.ModuleList([ROIAlignRotated3D(output_size, spatial_scale=scale, sampling_ratio=sampling_ratio)
                                      for scale in scales])
        self.output_size = output_size
        self.scales = tuple(float(s) for s in scales)
        self.sampling_ratio = sampling_ratio
        self.canonical_size = canonical_size
        self.box_scale = box_scale
        self.map_levels = LevelMapper_3d(scales, canonical_size)
        self.fused = True   # False: the reference's loop (torch ROI rows / levels, per-level nonzero + ROIAlignRotated3D)
        self.pooled_dtype = torch.float32   # torch.bfloat16: the pooled tensor (and its gradient) in bf16 storage

    def convert_to_roi_format(self, boxes):
        """[N, 8] ROI rows (scene, center_w, center_h, center_z, width, height, zsize, theta in degrees)"""
        if self.fused:
            return roi_glue.roi_rows_and_levels(_bbox3d(boxes), self.scales, self.canonical_size, self.box_scale)[0]
        return torch_rois_and_levels(_bbox3d(boxes), self.scales, self.canonical_size, self.box_scale)[0]

    def forward(self, x, boxes, pooled_dtype=None):
        """`pooled_dtype`: this call's storage of the result; None = the module's own `pooled_dtype`"""
        pooled_dtype = self.pooled_dtype if pooled_dtype is None else pooled_dtype
        if len(x) != len(self.poolers):
            raise ValueError("%d feature levels for a pooler of %d" % (len(x), len(self.poolers)))
        if pooled_dtype not in roi_glue.POOLED_DTYPES:
            raise TypeError("Pooler: pooled_dtype must be torch.float32 or torch.bfloat16, got %r" % (pooled_dtype,))
        bbox3d = _bbox3d(boxes)
        if len(self.poolers) == 1 and pooled_dtype == torch.float32:
            return self.poolers[0](x[0], self.convert_to_roi_format(boxes))
        if self.fused:
            return roi_glue.pool_rois(x, bbox3d, self.output_size, self.scales, self.sampling_ratio, self.canonical_size,
                                      self.box_scale, pooled_dtype=pooled_dtype)
        rois, levels = torch_rois_and_levels(bbox3d, self.scales, self.canonical_size, self.box_scale)
        feats0 = x[0].features
        # bf16 levels are gathered into an fp32 result, as the fused form gives it
        result = torch.zeros((len(rois), feats0.shape[1]) + tuple(self.output_size), device=feats0.device,
                             dtype=torch.float32 if feats0.dtype == torch.bfloat16 else feats0.dtype)
        for level, (per_level_feature, pooler) in enumerate(zip(x, self.poolers)):
            idx_in_level = torch.nonzero(levels == level).squeeze(1)
            result[idx_in_level] = pooler(per_level_feature, rois[idx_in_level])
        return result.to(pooled_dtype)               # bf16: one rounding of the loop's fp32 result
