"""Predictor of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/roi_box_predictors.py:34-120):
FPNPredictor, centroid form.  `cls_score` and `bbox_pred` are the reference's nn.Linear modules (names, shapes and
initialisation); `fused = True` (the default) computes both as one GEMM over the two weights (roi_glue.box_predictions),
`fused = False` runs the modules.  Not part of this package: the corner-ROI form and FastRCNNPredictor."""
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
        if self.corner_roi:
            raise ValueError("cfg.MODEL.CORNER_ROI: the corner-ROI form of the box head is not part of this package")
        self.class_specific = cfg.MODEL.CLASS_SPECIFIC
        self.cls_score = nn.Linear(representation_size, num_classes)
        self.bbox_pred = nn.Linear(representation_size, num_classes * 7 if self.class_specific else 7)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in [self.cls_score, self.bbox_pred]:
            nn.init.constant_(l.bias, 0)
        self.fused = True    # False: the two nn.Linear modules themselves, the yardstick

    def forward(self, x):
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
