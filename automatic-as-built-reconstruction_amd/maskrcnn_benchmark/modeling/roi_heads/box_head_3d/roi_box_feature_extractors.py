"""Feature extractor of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/
roi_box_feature_extractors.py:46-176): FPN2MLPFeatureExtractor, centroid and corner form.  The parameters live in the
reference's modules under the reference's names -- `conv3d` = nn.Sequential(nn.Conv3d, nn.BatchNorm3d, nn.ReLU), then
`fc6`, `fc7` (centroid) or `fc6_cor`, `fc6_body`, `fc7_cor`, `fc7_body` (cfg.MODEL.CORNER_ROI) -- so `state_dict()` keys,
shapes and initialisation are the reference's and checkpoints load by name.  `fused = True` (the default) computes with
roi_glue.box_head_mlp / box_head_mlp_corner (csrc/roi_mlp.hip: dense fp32 MFMA GEMMs reading the pooled tensor, and in
the corner form the windows of the convolution rows, in place) on those parameters; `fused = False` runs the torch
modules themselves, the yardstick and the A/B switch, as Pooler.fused.
`pooled_dtype` (torch.float32, the default, or torch.bfloat16) is handed to the pooler with every call -- it decides
for the extractor's calls whatever `pooler.pooled_dtype` says, and the pooler's own attribute is left as it is --: the
pooled tensor and its gradient in bf16 storage, read and written in place by the convolution's GEMMs; everything behind
it stays fp32.  The torch modules are fp32, so `fused = False` refuses a bf16 pooled tensor.
The pooler takes the metric proposals and SPARSE3D.VOXEL_SCALE (`box_scale`): convert_metric_to_pixel in its own launch.
Not part of this package: ResNet50Conv5ROIFeatureExtractor."""
import torch
import torch.nn.functional as F
from torch import nn

import roi_glue
from maskrcnn_benchmark.modeling.poolers_3d import Pooler


class CornerFeatures(list):
    """what the corner form returns: the list [x_cor0, x_cor1, x_body] of the reference, its first two entries being
    row views of `x_cor` [2 N, R] -- the predictor runs its corner GEMM on the stacked rows without a copy"""

    def __init__(self, x_cor, x_body):
        n = int(x_body.shape[0])
        super(CornerFeatures, self).__init__([x_cor[:n], x_cor[n:], x_body])
        self.x_cor = x_cor


class FPN2MLPFeatureExtractor(nn.Module):
    """pooler, then Conv3d([1, 1, pz]) + BatchNorm3d + ReLU, fc6 and fc7: proposals -> one feature row per ROI; in the
    corner form three rows per ROI: the two corner windows and the body window of the 11-wide axis, each through its
    own fc6 / fc7 (the corners share theirs)"""

    def __init__(self, cfg):
        super(FPN2MLPFeatureExtractor, self).__init__()
        self.corner_roi = cfg.MODEL.CORNER_ROI
        roi_glue.corner_roi_check(cfg)       # resolution[1] == 11 (the reference asserts it), no corner-connection loss
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
        if not self.corner_roi:
            self.fc6 = nn.Linear(representation_size * resolution[0] * resolution[1], representation_size)
            self.fc7 = nn.Linear(representation_size, representation_size)
            layers = [self.fc6, self.fc7]
        else:
            cor, body = roi_glue.CORNER_WINDOWS[1], roi_glue.BODY_WINDOW[1]          # roi_all_cor_body = [11, 3, 7]
            self.fc6_cor = nn.Linear(representation_size * resolution[0] * cor, representation_size)
            self.fc6_body = nn.Linear(representation_size * resolution[0] * body, representation_size)
            self.fc7_cor = nn.Linear(representation_size, representation_size)
            self.fc7_body = nn.Linear(representation_size, representation_size)
            layers = [self.fc6_cor, self.fc6_body, self.fc7_cor, self.fc7_body]
        for l in layers:
            # the reference's initialisation: uniform Kaiming with a = 1, zero bias
            nn.init.kaiming_uniform_(l.weight, a=1)
            nn.init.constant_(l.bias, 0)
        self.fused = True    # False: the torch modules themselves (rocBLAS / MIOpen), the yardstick
        self.pooled_dtype = torch.float32    # torch.bfloat16: the pooler's result in bf16 storage (fused only)

    @staticmethod
    def roi_separate(roi_2d):
        assert roi_2d.shape[3] == 11
        return [roi_2d[:, :, :, 0:3], roi_2d[:, :, :, 8:11], roi_2d[:, :, :, 2:9]]

    def head(self, x1_):
        """pooled [N, C, ph, pw, pz] -> x4 [N, MLP_HEAD_DIM]; corner form: [x_cor0, x_cor1, x_body], each that shape"""
        if not self.fused:
            if x1_.dtype == torch.bfloat16:
                raise TypeError("FPN2MLPFeatureExtractor.fused = False runs the torch modules on float32 parameters: a "
                                "bfloat16 pooled tensor (pooled_dtype) needs fused = True")
            x1 = self.conv3d(x1_)
            if self.corner_roi:
                # the reference's statements; squeeze(-1) where it has squeeze(), which also drops the ROI axis at N = 1
                x4s = []
                for i, x1i in enumerate(self.roi_separate(x1.squeeze(-1))):
                    x2 = x1i.contiguous().view(x1i.size(0), -1)
                    fc6, fc7 = (self.fc6_cor, self.fc7_cor) if i < 2 else (self.fc6_body, self.fc7_body)
                    x4s.append(F.relu(fc7(F.relu(fc6(x2)))))
                return x4s
            x2 = x1.view(x1.size(0), -1)
            x3 = F.relu(self.fc6(x2))
            return F.relu(self.fc7(x3))
        conv, bn = self.conv3d[0], self.conv3d[1]
        state = {"eps": bn.eps, "momentum": bn.momentum, "training": bn.training,
                 "track_running_stats": bn.track_running_stats, "running_mean": bn.running_mean,
                 "running_var": bn.running_var}
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        if self.corner_roi:
            return CornerFeatures(*roi_glue.box_head_mlp_corner(
                x1_, conv.weight, conv.bias, bn.weight, bn.bias, state, self.fc6_cor.weight, self.fc6_cor.bias,
                self.fc6_body.weight, self.fc6_body.bias, self.fc7_cor.weight, self.fc7_cor.bias, self.fc7_body.weight,
                self.fc7_body.bias))
        return roi_glue.box_head_mlp(x1_, conv.weight, conv.bias, bn.weight, bn.bias, state, self.fc6.weight,
                                     self.fc6.bias, self.fc7.weight, self.fc7.bias)

    def forward(self, x0, proposals):
        # the extractor's attribute is the knob for its own calls: handed over per call, the pooler module is not changed
        return self.head(self.pooler(x0, proposals, pooled_dtype=self.pooled_dtype))


_ROI_BOX_FEATURE_EXTRACTORS = {"FPN2MLPFeatureExtractor": FPN2MLPFeatureExtractor}


def make_roi_box_feature_extractor(cfg):
    name = cfg.MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR
    if name not in _ROI_BOX_FEATURE_EXTRACTORS:
        raise ValueError("cfg.MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR = %r: only %s is part of this package"
                         % (name, sorted(_ROI_BOX_FEATURE_EXTRACTORS)))
    return _ROI_BOX_FEATURE_EXTRACTORS[name](cfg)
