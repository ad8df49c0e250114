"""Predictor of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/roi_box_predictors.py:34-120):
FPNPredictor, centroid and corner form.  `cls_score` and `bbox_pred` are the reference's nn.Linear modules (names, shapes
and initialisation); `fused = True` (the default) computes both as one GEMM over the two weights
(roi_glue.box_predictions), `fused = False` runs the modules.  With cfg.MODEL.CORNER_ROI the modules are the reference's
`cls_score_body`, `bbox_pred_body` (z0, z1, thickness), `bbox_pred_cor` (x, y of a corner), `bbox_corner_semantic` and
`score_pred_cor`, default-initialised as there; the input is the extractor's [x_cor0, x_cor1, x_body] and the fused form
is two GEMMs, one over the body rows and one over both corners' rows (roi_glue.box_predictions_corner).  `score_pred_cor`
keeps its parameters and is not computed: the reference never uses its result.  Not part of this package:
FastRCNNPredictor."""
import torch
from torch import nn

import roi_glue


class FPNPredictor(nn.Module):
    def __init__(self, cfg):
        super(FPNPredictor, self).__init__()
        num_classes = len(cfg.INPUT.CLASSES)
        representation_size = cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM
        separate_classes = cfg.MODEL.SEPARATE_CLASSES
        if len(separate_classes) > 0:
            num_classes += len(separate_classes)
        self.num_classes = num_classes
        self.corner_roi = cfg.MODEL.CORNER_ROI
        roi_glue.corner_roi_check(cfg)       # the three-part input exists only at POOLER_RESOLUTION[1] == 11
        self.class_specific = cfg.MODEL.CLASS_SPECIFIC
        per = num_classes if self.class_specific else 1
        if not self.corner_roi:
            self.cls_score = nn.Linear(representation_size, num_classes)
            self.bbox_pred = nn.Linear(representation_size, per * 7)
            nn.init.normal_(self.cls_score.weight, std=0.01)
            nn.init.normal_(self.bbox_pred.weight, std=0.001)
            for l in [self.cls_score, self.bbox_pred]:
                nn.init.constant_(l.bias, 0)
        else:
            self.cls_score_body = nn.Linear(representation_size, num_classes)
            self.bbox_pred_body = nn.Linear(representation_size, per * 3)     # z0, z1, thickness
            self.bbox_pred_cor = nn.Linear(representation_size, per * 2)      # x, y
            self.bbox_corner_semantic = nn.Linear(representation_size, 8)     # connection along four directions
            self.score_pred_cor = nn.Linear(representation_size, 1)
        self.fused = True    # False: the nn.Linear modules themselves, the yardstick

    def forward_corner_box(self, x):
        """x = [x_cor0, x_cor1, x_body] -> (scores [n, C], bbox_regression_corners [n, 7 C] or [n, 7], corner_semantics
        [n, 16]); the regression is [cor0 xy, cor1 xy, z0 z1 thickness] per class"""
        x_cor0, x_cor1, x_body = x
        if self.fused:
            x_cor = getattr(x, "x_cor", None)
            if x_cor is None:
                x_cor = torch.cat([x_cor0, x_cor1])
            return roi_glue.box_predictions_corner(
                x_cor, x_body, self.cls_score_body.weight, self.cls_score_body.bias, self.bbox_pred_body.weight,
                self.bbox_pred_body.bias, self.bbox_pred_cor.weight, self.bbox_pred_cor.bias,
                self.bbox_corner_semantic.weight, self.bbox_corner_semantic.bias, bool(self.class_specific))
        scores = self.cls_score_body(x_body)
        bbox_body = self.bbox_pred_body(x_body)
        bbox_cor0 = self.bbox_pred_cor(x_cor0)
        bbox_cor1 = self.bbox_pred_cor(x_cor1)
        if self.class_specific:
            n = bbox_body.shape[0]
            bbox_cor0 = bbox_cor0.view([n, self.num_classes, 2])
            bbox_cor1 = bbox_cor1.view([n, self.num_classes, 2])
            bbox_body = bbox_body.view([n, self.num_classes, 3])
            bbox_regression_corners = torch.cat([bbox_cor0, bbox_cor1, bbox_body], 2).view([n, -1])
        else:
            bbox_regression_corners = torch.cat([bbox_cor0, bbox_cor1, bbox_body], 1)
        corner_semantics = torch.cat([self.bbox_corner_semantic(x_cor0), self.bbox_corner_semantic(x_cor1)], 1)
        return scores, bbox_regression_corners, corner_semantics

    def forward(self, x):
        if self.corner_roi:
            return self.forward_corner_box(x)
        if not self.fused:
            return self.cls_score(x), self.bbox_pred(x)
        return roi_glue.box_predictions(x, self.cls_score.weight, self.cls_score.bias, self.bbox_pred.weight,
                                        self.bbox_pred.bias)


_ROI_BOX_PREDICTOR = {"FPNPredictor": FPNPredictor}


def make_roi_box_predictor(cfg):
    name = cfg.MODEL.ROI_BOX_HEAD.PREDICTOR
    if name not in _ROI_BOX_PREDICTOR:
        raise ValueError("cfg.MODEL.ROI_BOX_HEAD.PREDICTOR = %r: only %s is part of this package"
                         % (name, sorted(_ROI_BOX_PREDICTOR)))
    return _ROI_BOX_PREDICTOR[name](cfg)
