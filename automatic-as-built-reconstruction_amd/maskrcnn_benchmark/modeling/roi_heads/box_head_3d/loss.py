"""FastRCNNLossComputation of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/loss.py:137-382,
577-606): `subsample` matches, labels, encodes and samples the proposals of a batch in one library
call (roi_glue.box_head_targets, csrc/roi_loss.hip), `__call__` computes the cross-entropy and the per-class smooth-L1 loss
with autograd (roi_glue.box_head_loss).  `proposals` / `targets` are duck-typed (`.bbox3d` [n, 7] yx_zb, `.size3d`,
`len()`; targets also `get_field("labels")`); the sampled lists are DetectionList3D objects (box_head_3d/inference.py).
The coder may be the centroid or the corner form (MODEL.CORNER_ROI): the target kernel encodes in the form of the
BoxCoder3D it is given, and in `Diff` mode the losses treat element 6 (yaw difference / thickness) as an ordinary
difference either way.  With separated-classifier groups (MODEL.SEPARATE_CLASSES_ID, class-agnostic regression) both
methods take the grouped path of the SeperateClassifier (modeling/seperate_classifier.py): one grouped call each, the
losses coming back as lists of one value per group.  With `corner_loss=True` (MODEL.LOSS.CORNER_CONNECTION, corner form
only) `subsample` also keeps the corner-connection tables of the sample (roi_glue.box_head_targets(corner_groups=True))
and `__call__` / `box_loss` turn `corners_semantic` into the reference's three corner losses
(roi_glue.corner_connection_loss, csrc/corner_loss.hip; loss.py:384-499).  Not part of this path, and refused: groups
together with MODEL.CLASS_SPECIFIC or with the corner losses, and `corners_semantic` without `corner_loss`."""
import torch

import roi_glue
from rpn_glue import parse_yaw_loss_mode
from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
from maskrcnn_benchmark.modeling.matcher import Matcher
from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier


class FastRCNNLossComputation(object):
    """
    Computes the loss for Faster R-CNN.
    """

    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, yaw_loss_mode, add_gt_proposals, aug_thickness,
                 seperate_classifier, class_specific, corner_loss=False):
        """proposal_matcher (Matcher), fg_bg_sampler (BalancedPositiveNegativeSampler), box_coder (BoxCoder3D);
        aug_thickness: dict target_Y / target_Z / anchor_Y / anchor_Z; seperate_classifier: None, an object whose
        `need_seperate` is false, or a SeperateClassifier with groups (then `class_specific` must be false).
        `add_gt_proposals` is kept as the reference keeps it (unused by this class: the RPN
        appends the ground truth, callers pass the lists they want matched).  `corner_loss`: compute the
        corner-connection losses from `corners_semantic` (needs a corner coder and no groups)."""
        need_seperate = seperate_classifier is not None and bool(getattr(seperate_classifier, "need_seperate", False))
        if need_seperate and (class_specific or not isinstance(seperate_classifier, SeperateClassifier)):
            raise ValueError("separated-classifier groups (need_seperate) need this package's SeperateClassifier and "
                             "class-agnostic box regression (MODEL.CLASS_SPECIFIC = False)")
        if corner_loss and (need_seperate or not roi_glue.coder_args(box_coder)[2]):
            raise ValueError("the corner-connection losses (corner_loss) need the corner form of the coder "
                             "(MODEL.CORNER_ROI) and no separated-classifier groups")
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
        self.need_seperate = need_seperate
        self.class_specific = class_specific
        self.corner_loss = bool(corner_loss)
        self.last_flag = None

    def subsample(self, proposals, targets):
        """proposals / targets: one list object per scene.  Returns one DetectionList3D per scene holding the sampled
        proposals in ascending row, with fields `labels`, `regression_targets` and `rows` (the scene's proposal row of
        each).  Keeps the state `__call__` needs.  With groups: SeperateClassifier.seperate_subsample (the proposals carry
        `sep_id`; the lists come back with `sep_id` and group-local `labels`).  With `corner_loss` the corner-connection
        tables of the sample are kept too (`_corner_tables`: per scene pos_pos, connect_ids, corner_xyz)."""
        if self.need_seperate:
            self._proposals = self.seperate_classifier.seperate_subsample(proposals, targets, self.subsample_standard)
            return self._proposals
        return self.subsample_standard(proposals, targets)

    def subsample_standard(self, proposals, targets):
        """the single-group form of `subsample`"""
        s = self.fg_bg_sampler
        dets = roi_glue.box_head_targets(
            [p.bbox3d for p in proposals], [t.bbox3d for t in targets], [t.get_field("labels") for t in targets],
            fg_iou=self.high_threshold, bg_iou=self.low_threshold, aug_thickness=self.aug_thickness,
            batch_size_per_image=s.batch_size_per_image, positive_fraction=s.positive_fraction,
            box_coder=self.box_coder, seed=getattr(s, "seed", None), corner_groups=self.corner_loss)
        out = [DetectionList3D(d["bbox3d"], p.size3d, {"labels": d["labels"], "regression_targets": d["regression_targets"],
                                                       "rows": d["rows"]}) for d, p in zip(dets, proposals)]
        self._proposals = out
        self._corner_tables = ([{k: d[k] for k in ("pos_pos", "connect_ids", "corner_xyz")} for d in dets]
                               if self.corner_loss else None)
        return out

    def corner_connection_loss(self, corners_semantic):
        """loss.py:384-499 on the tables `subsample` kept: {"geometric_pull_loss", "semantic_pull_loss",
        "semantic_push_loss"}, 0-dim device tensors (roi_glue.corner_connection_loss)."""
        if not self.corner_loss:
            raise ValueError("the corner-connection losses (corners_semantic) are not part of this path")
        if getattr(self, "_corner_tables", None) is None:
            raise RuntimeError("subsample needs to be called before")
        tabs = self._corner_tables
        return roi_glue.corner_connection_loss(
            corners_semantic, [len(q) for q in self._proposals], [d["pos_pos"] for d in tabs],
            [d["connect_ids"] for d in tabs], [d["corner_xyz"] for d in tabs])

    def box_loss(self, labels, box_regression, regression_targets, pro_bbox3ds=None, corners_semantic=None):
        """the box term of `__call__` alone (loss.py:343-382), single-group form: (box_loss, {}), or with `corner_loss` and
        corners_semantic (box_loss, the three corner losses).  It is the `box_loss_fn`
        SeperateClassifier.roi_box_loss_seperated is handed; `__call__` itself computes both losses in one call."""
        if corners_semantic is not None and not self.corner_loss:
            raise ValueError("the corner-connection losses (corners_semantic) are not part of this path")
        n, width = int(box_regression.shape[0]), int(box_regression.shape[1])
        zeros = box_regression.new_zeros((n, width // 7 if self.class_specific else roi_glue.SEP_MAX_COLS))
        _cls, box = roi_glue.box_head_loss(zeros, box_regression, labels, regression_targets,
                                           class_specific=bool(self.class_specific), yaw_loss_mode=self.yaw_loss_mode)
        return box, ({} if corners_semantic is None else self.corner_connection_loss(corners_semantic))

    def __call__(self, class_logits, box_regression, corners_semantic, targets=None):
        """class_logits [n, C], box_regression [n, 7 C] (class specific) or [n, 7], n = the rows `subsample` returned over
        the batch.  Returns (classification_loss, box_loss, corner_loss): the third is {} when corners_semantic is None,
        as in the reference, else (with `corner_loss`; corners_semantic fp32 [n, 16]) the dict of the three
        corner-connection losses.  `self.last_flag` is left holding the 0-dim int32 device
        tensor of roi_glue.box_head_loss (1 = some label lay outside [0, C): that row was skipped); reading it is a
        host read, so it is the caller's to do, with the losses.  With groups the two losses are lists of G 0-dim
        tensors (one grouped call, SeperateClassifier.roi_losses_seperated), box_regression is [n, 7] and class_logits
        [n, C_tot]."""
        if corners_semantic is not None and not self.corner_loss:
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
        if self.need_seperate:
            cls_loss, box_loss, self.last_flag = self.seperate_classifier.roi_losses_seperated(
                class_logits, box_regression, labels, regression_targets, props, yaw_loss_mode=self.yaw_loss_mode)
            return list(cls_loss.unbind(0)), list(box_loss.unbind(0)), {}
        cls_loss, box_loss, self.last_flag = roi_glue.box_head_loss(
            class_logits, box_regression, labels, regression_targets, class_specific=bool(self.class_specific),
            yaw_loss_mode=self.yaw_loss_mode, return_flag=True)
        return cls_loss, box_loss, ({} if corners_semantic is None else self.corner_connection_loss(corners_semantic))


def make_roi_box_loss_evaluator(cfg):
    """loss.py:577-606.  Returns (loss_evaluator, seperate_classifier); the second is None when
    cfg.MODEL.SEPARATE_CLASSES_ID is empty, else the SeperateClassifier built from it (ValueError together with
    MODEL.CLASS_SPECIFIC).  With MODEL.CORNER_ROI the coder is the corner form and MODEL.LOSS.WEIGHTS[4:7] must be 0
    unless MODEL.LOSS.CORNER_CONNECTION switches the corner-connection losses on (roi_glue.corner_roi_check)."""
    roi_glue.corner_roi_check(cfg)
    matcher = Matcher(cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD, cfg.MODEL.ROI_HEADS.BG_IOU_THRESHOLD,
                      allow_low_quality_matches=False)
    box_coder = BoxCoder3D(is_corner_roi=cfg.MODEL.CORNER_ROI, weights=cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    fg_bg_sampler = BalancedPositiveNegativeSampler(cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
                                                    cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
    ay = cfg.MODEL.ROI_HEADS.LABEL_AUG_THICKNESS_Y_TAR_ANC
    az = cfg.MODEL.ROI_HEADS.LABEL_AUG_THICKNESS_Z_TAR_ANC
    aug_thickness = {"target_Y": ay[0], "anchor_Y": ay[1], "target_Z": az[0], "anchor_Z": az[1]}
    seperate_classifier = None
    if len(cfg.MODEL.SEPARATE_CLASSES_ID) > 0:
        seperate_classifier = SeperateClassifier(cfg.MODEL.SEPARATE_CLASSES_ID, len(cfg.INPUT.CLASSES),
                                                 cfg.MODEL.CLASS_SPECIFIC, "ROI_LOSS")
    loss_evaluator = FastRCNNLossComputation(matcher, fg_bg_sampler, box_coder, cfg.MODEL.LOSS.YAW_MODE,
                                             cfg.MODEL.RPN.ADD_GT_PROPOSALS, aug_thickness, seperate_classifier,
                                             class_specific=cfg.MODEL.CLASS_SPECIFIC,
                                             corner_loss=roi_glue.corner_loss_on(cfg))
    return loss_evaluator, seperate_classifier
