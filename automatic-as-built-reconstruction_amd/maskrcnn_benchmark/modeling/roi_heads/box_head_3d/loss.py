"""FastRCNNLossComputation of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/loss.py:137-382,
577-606), the non-separated path: `subsample` matches, labels, encodes and samples the proposals of a batch in one library
call (roi_glue.box_head_targets, csrc/roi_loss.hip), `__call__` computes the cross-entropy and the per-class smooth-L1 loss
with autograd (roi_glue.box_head_loss).  `proposals` / `targets` are duck-typed (`.bbox3d` [n, 7] yx_zb, `.size3d`,
`len()`; targets also `get_field("labels")`); the sampled lists are DetectionList3D objects (box_head_3d/inference.py).
The coder may be the centroid or the corner form (MODEL.CORNER_ROI): the target kernel encodes in the form of the
BoxCoder3D it is given, and in `Diff` mode the losses treat element 6 (yaw difference / thickness) as an ordinary
difference either way.  Not part of this path, and refused: the separated-classifier groups
(SeperateClassifier.need_seperate) and the corner-connection losses (`corners_semantic`, MODEL.LOSS.WEIGHTS[4:7])."""
import torch

import roi_glue
from rpn_glue import parse_yaw_loss_mode
from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
from maskrcnn_benchmark.modeling.matcher import Matcher
from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D


class FastRCNNLossComputation(object):
    """
    Computes the loss for Faster R-CNN.
    """

    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, yaw_loss_mode, add_gt_proposals, aug_thickness,
                 seperate_classifier, class_specific):
        """proposal_matcher (Matcher), fg_bg_sampler (BalancedPositiveNegativeSampler), box_coder (BoxCoder3D);
        aug_thickness: dict target_Y / target_Z / anchor_Y / anchor_Z; seperate_classifier: None or an object whose
        `need_seperate` is false.  `add_gt_proposals` is kept as the reference keeps it (unused by this class: the RPN
        appends the ground truth, callers pass the lists they want matched)."""
        if seperate_classifier is not None and getattr(seperate_classifier, "need_seperate", False):
            raise ValueError("the separated-classifier groups (need_seperate) are not part of this path")
        roi_glue.coder_args(box_coder)       # ValueError unless it carries seven weights
        parse_yaw_loss_mode(yaw_loss_mode)   # 'Diff' / 'Diff_<w>'; 'SinDiff' cannot run in the reference's box_loss either
        self.proposal_matcher = proposal_matcher
        self.fg_bg_sampler = fg_bg_sampler
        self.box_coder = box_coder
        self.yaw_loss_mode = yaw_loss_mode
        self.high_threshold = proposal_matcher.high_threshold
        self.low_threshold = proposal_matcher.low_threshold
        self.add_gt_proposals = add_gt_proposals
        self.aug_thickness = aug_thickness
        self.seperate_classifier = seperate_classifier
        self.need_seperate = False
        self.class_specific = class_specific
        self.last_flag = None

    def subsample(self, proposals, targets):
        """proposals / targets: one list object per scene.  Returns one DetectionList3D per scene holding the sampled
        proposals in ascending row, with fields `labels`, `regression_targets` and `rows` (the scene's proposal row of
        each).  Keeps the state `__call__` needs."""
        s = self.fg_bg_sampler
        dets = roi_glue.box_head_targets(
            [p.bbox3d for p in proposals], [t.bbox3d for t in targets], [t.get_field("labels") for t in targets],
            fg_iou=self.high_threshold, bg_iou=self.low_threshold, aug_thickness=self.aug_thickness,
            batch_size_per_image=s.batch_size_per_image, positive_fraction=s.positive_fraction,
            box_coder=self.box_coder, seed=getattr(s, "seed", None))
        out = [DetectionList3D(d["bbox3d"], p.size3d, {"labels": d["labels"], "regression_targets": d["regression_targets"],
                                                       "rows": d["rows"]}) for d, p in zip(dets, proposals)]
        self._proposals = out
        return out

    def __call__(self, class_logits, box_regression, corners_semantic, targets=None):
        """class_logits [n, C], box_regression [n, 7 C] (class specific) or [n, 7], n = the rows `subsample` returned over
        the batch.  Returns (classification_loss, box_loss, {}) -- the corner loss of the reference is {} when
        corners_semantic is None, the only case of this path.  `self.last_flag` is left holding the 0-dim int32 device
        tensor of roi_glue.box_head_loss (1 = some label lay outside [0, C): that row was skipped); reading it is a
        host read, so it is the caller's to do, with the losses."""
        if corners_semantic is not None:
            raise ValueError("the corner-connection losses (corners_semantic; MODEL.LOSS.WEIGHTS[4:7] != 0) are not part "
                             "of this path")
        if not hasattr(self, "_proposals"):
            raise RuntimeError("subsample needs to be called before")
        props = self._proposals
        if not props:
            raise RuntimeError("subsample returned no scene")
        labels = torch.cat([p.get_field("labels") for p in props])
        regression_targets = torch.cat([p.get_field("regression_targets") for p in props])
        assert class_logits.shape[0] == box_regression.shape[0] == labels.shape[0]
        cls_loss, box_loss, self.last_flag = roi_glue.box_head_loss(
            class_logits, box_regression, labels, regression_targets, class_specific=bool(self.class_specific),
            yaw_loss_mode=self.yaw_loss_mode, return_flag=True)
        return cls_loss, box_loss, {}


def make_roi_box_loss_evaluator(cfg):
    """loss.py:577-606.  Returns (loss_evaluator, seperate_classifier); the second is None: cfg.MODEL.SEPARATE_CLASSES_ID
    must be empty here.  With MODEL.CORNER_ROI the coder is the corner form and MODEL.LOSS.WEIGHTS[4:7] must be 0
    (roi_glue.corner_roi_check)."""
    roi_glue.corner_roi_check(cfg)
    matcher = Matcher(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, cfg.MODEL.ROI_HEADS.BG_IOU_THRESHOLD,
                      allow_low_quality_matches=False)
    box_coder = BoxCoder3D(is_corner_roi=cfg.MODEL.CORNER_ROI, weights=cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    fg_bg_sampler = BalancedPositiveNegativeSampler(cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
                                                    cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
    ay = cfg.MODEL.ROI_HEADS.LABEL_AUG_THICKNESS_Y_TAR_ANC
    az = cfg.MODEL.ROI_HEADS.LABEL_AUG_THICKNESS_Z_TAR_ANC
    aug_thickness = {"target_Y": ay[0], "anchor_Y": ay[1], "target_Z": az[0], "anchor_Z": az[1]}
    if len(cfg.MODEL.SEPARATE_CLASSES_ID) > 0:
        raise ValueError("cfg.MODEL.SEPARATE_CLASSES_ID is not empty: the separated-classifier groups are not part of "
                         "this path")
    loss_evaluator = FastRCNNLossComputation(matcher, fg_bg_sampler, box_coder, cfg.MODEL.LOSS.YAW_MODE,
                                             cfg.MODEL.RPN.ADD_GT_PROPOSALS, aug_thickness, None,
                                             class_specific=cfg.MODEL.CLASS_SPECIFIC)
    return loss_evaluator, None
