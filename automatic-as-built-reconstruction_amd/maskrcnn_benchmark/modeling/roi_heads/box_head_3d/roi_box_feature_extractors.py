"""Feature extractor of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/
roi_box_feature_extractors.py:46-176): FPN2MLPFeatureExtractor, centroid form.  The parameters live in the reference's
modules under the reference's names -- `conv3d` = nn.Sequential(nn.Conv3d, nn.BatchNorm3d, nn.ReLU), `fc6`, `fc7` -- so
`state_dict()` keys, shapes and initialisation are the reference's and checkpoints load by name.  `fused = True` (the
default) computes with roi_glue.box_head_mlp (csrc/roi_mlp.hip: dense fp32 MFMA GEMMs reading the pooled tensor in place)
on those parameters; `fused = False` runs the torch modules themselves, the yardstick and the A/B switch, as Pooler.fused.
The pooler takes the metric proposals and SPARSE3D.VOXEL_SCALE (`box_scale`): convert_metric_to_pixel in its own launch.
Not part of this package: the corner-ROI form (cfg.MODEL.CORNER_ROI) and ResNet50Conv5ROIFeatureExtractor."""
import torch.nn.functional as F
from torch import nn

import roi_glue
from maskrcnn_benchmark.modeling.poolers_3d import Pooler


class FPN2MLPFeatureExtractor(nn.Module):
    """pooler, then Conv3d([1, 1, pz]) + BatchNorm3d + ReLU, fc6 and fc7: proposals -> one feature row per ROI"""

    def __init__(self, cfg):
        super(FPN2MLPFeatureExtractor, self).__init__()
        self.corner_roi = cfg.MODEL.CORNER_ROI
        if self.corner_roi:
            raise ValueError("cfg.MODEL.CORNER_ROI: the corner-ROI form of the box head is not part of this package")
        resolution = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.voxel_scale = cfg.SPARSE3D.VOXEL_SCALE
        self.pooler = Pooler(output_size=(resolution[0], resolution[1], resolution[2]),
                             scales=cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES_SPATIAL,
                             sampling_ratio=cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO,
                             canonical_size=cfg.MODEL.ROI_BOX_HEAD.CANONICAL_SIZE, canonical_level=None,
                             box_scale=self.voxel_scale)
        representation_size = cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM
        conv3d_ = nn.Conv3d(cfg.SPARSE3D.nPlaneMap, representation_size, kernel_size=[1, 1, resolution[2]],
                            stride=[1, 1, 1])
        bn = nn.BatchNorm3d(representation_size, track_running_stats=cfg.SOLVER.TRACK_RUNNING_STATS)
        self.conv3d = nn.Sequential(conv3d_, bn, nn.ReLU(inplace=True))
        self.fc6 = nn.Linear(representation_size * resolution[0] * resolution[1], representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        for l in [self.fc6, self.fc7]:
            # the reference's initialisation: uniform Kaiming with a = 1, zero bias
            nn.init.kaiming_uniform_(l.weight, a=1)
            nn.init.constant_(l.bias, 0)
        self.fused = True    # False: the torch modules themselves (rocBLAS / MIOpen), the yardstick

    def head(self, x1_):
        """pooled [N, C, ph, pw, pz] -> x4 [N, MLP_HEAD_DIM]"""
        if not self.fused:
            x1 = self.conv3d(x1_)
            x2 = x1.view(x1.size(0), -1)
            x3 = F.relu(self.fc6(x2))
            return F.relu(self.fc7(x3))
        conv, bn = self.conv3d[0], self.conv3d[1]
        state = {"eps": bn.eps, "momentum": bn.momentum, "training": bn.training,
                 "track_running_stats": bn.track_running_stats, "running_mean": bn.running_mean,
                 "running_var": bn.running_var}
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        return roi_glue.box_head_mlp(x1_, conv.weight, conv.bias, bn.weight, bn.bias, state, self.fc6.weight,
                                     self.fc6.bias, self.fc7.weight, self.fc7.bias)

    def forward(self, x0, proposals):
        return self.head(self.pooler(x0, proposals))


_ROI_BOX_FEATURE_EXTRACTORS = {"FPN2MLPFeatureExtractor": FPN2MLPFeatureExtractor}


def make_roi_box_feature_extractor(cfg):
    name = cfg.MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR
    if name not in _ROI_BOX_FEATURE_EXTRACTORS:
        raise ValueError("cfg.MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR = %r: only %s is part of this package"
                         % (name, sorted(_ROI_BOX_FEATURE_EXTRACTORS)))
    return _ROI_BOX_FEATURE_EXTRACTORS[name](cfg)
