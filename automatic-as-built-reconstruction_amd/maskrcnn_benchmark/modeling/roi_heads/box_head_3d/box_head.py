"""The box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/box_head.py:41-257), centroid form
(forward_centroid_box, :168-248) and corner form (cfg.MODEL.CORNER_ROI, forward_corner_box, :78-165): feature extractor,
predictor, loss evaluator and post-processor in the reference's order.  `proposals` is one duck-typed list per scene
(`.bbox3d` [n, 7] yx_zb, `.size3d`), or an object whose `seperate_examples()` returns that.  The corner form runs with the
default loss weights, cfg.MODEL.LOSS.WEIGHTS[4:7] == 0, where the reference drops `corners_semantic` (:121-122); nonzero
corner-connection loss weights need cfg.MODEL.LOSS.CORNER_CONNECTION = True, which passes `corners_semantic` to the loss
evaluator and adds `geometric_pull_loss`, `semantic_pull_loss`, `semantic_push_loss` to the loss dict (without the key
they are refused).  With separated-classifier groups (MODEL.SEPARATE_CLASSES /
SEPARATE_CLASSES_ID, class-agnostic regression) the proposals carry `sep_id`, the loss evaluator and the post-processor go
through the SeperateClassifier (modeling/seperate_classifier.py) and the losses come out per group, as
`loss_classifier_roi_{g}` / `loss_box_reg_roi_{g}` (:149-157).  Not part of this package: cfg.DEBUG.eval_in_train (its rm_gt_from_proposals_ reads an `is_gt` field the sampled lists here do not carry)."""
import torch

import roi_glue
from .inference import make_roi_box_post_processor
from .loss import make_roi_box_loss_evaluator
from .roi_box_feature_extractors import make_roi_box_feature_extractor
from .roi_box_predictors import make_roi_box_predictor


class ROIBoxHead3D(torch.nn.Module):
    """extractor + predictor + loss evaluator (training) or post-processor (evaluation)"""

    def __init__(self, cfg):
        super(ROIBoxHead3D, self).__init__()
        roi_glue.corner_roi_check(cfg)       # POOLER_RESOLUTION[1] == 11; LOSS.WEIGHTS[4:7] == 0 or LOSS.CORNER_CONNECTION
        if cfg.DEBUG.eval_in_train > 0:
            raise ValueError("cfg.DEBUG.eval_in_train > 0 is not part of this package")
        self.feature_extractor = make_roi_box_feature_extractor(cfg)
        self.predictor = make_roi_box_predictor(cfg)
        self.post_processor_ = make_roi_box_post_processor(cfg)
        self.loss_evaluator, self.seperate_classifier = make_roi_box_loss_evaluator(cfg)
        self.need_seperate = self.seperate_classifier is not None and self.seperate_classifier.need_seperate
        self.eval_in_train = cfg.DEBUG.eval_in_train
        self.add_gt_proposals = cfg.MODEL.RPN.ADD_GT_PROPOSALS
        self.detections_per_img = cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG
        self.corner_roi = cfg.MODEL.CORNER_ROI
        # box_head.py:57-58: the reference drops corners_semantic when the three weights sum to 0
        self.no_corner_loss = not (roi_glue.corner_loss_on(cfg) and sum(cfg.MODEL.LOSS.WEIGHTS[4:7]) != 0)
        self.cfg = cfg

    def post_processor(self, log_reg, proposals):
        if not self.need_seperate:
            return self.post_processor_(log_reg, proposals)
        class_logits, box_regression, corners_semantic = log_reg
        return self.seperate_classifier.post_processor(class_logits, box_regression, corners_semantic=corners_semantic,
                                                       proposals=proposals, post_processor_fn=self.post_processor_)

    def _roi_losses(self, loss_classifier, loss_box_reg):
        """the loss dict of a training pass: one pair, or one pair per separated group (box_head.py:149-157)"""
        if not self.need_seperate:
            return {"loss_classifier_roi": loss_classifier, "loss_box_reg_roi": loss_box_reg}
        roi_loss = {}
        for gi in range(len(loss_classifier)):
            roi_loss["loss_classifier_roi_%d" % gi] = loss_classifier[gi]
            roi_loss["loss_box_reg_roi_%d" % gi] = loss_box_reg[gi]
        return roi_loss

    def forward(self, features, proposals, targets=None):
        """features: one SparseConvNetTensor per level; proposals: per-scene lists; targets: per-scene ground truth
        (training).  Returns (x, proposals, losses): training -- the sampled proposals and {"loss_classifier_roi",
        "loss_box_reg_roi"} (with groups: one pair of keys per group, suffixed _0 .. _{G-1}); evaluation -- the detections
        and {}.  In the corner form x is the list [x_cor0, x_cor1,
        x_body] and box_regression holds two-corner encodings."""
        if self.corner_roi:
            return self.forward_corner_box(features, proposals, targets)
        if hasattr(proposals, "seperate_examples"):
            proposals = proposals.seperate_examples()
        if self.training:
            # training runs on the balanced sample of the proposals, not on all of them
            with torch.no_grad():
                proposals = self.loss_evaluator.subsample(proposals, targets)
        x = self.feature_extractor(features, proposals)
        class_logits, box_regression = self.predictor(x)
        if not self.training:
            result = self.post_processor((class_logits, box_regression, None), proposals)
            return x, result, {}
        loss_classifier, loss_box_reg, _ = self.loss_evaluator(class_logits, box_regression, corners_semantic=None,
                                                               targets=targets)
        return x, proposals, self._roi_losses(loss_classifier, loss_box_reg)


    def forward_corner_box(self, features, proposals, targets=None):
        if hasattr(proposals, "seperate_examples"):
            proposals = proposals.seperate_examples()
        if self.training:
            with torch.no_grad():
                proposals = self.loss_evaluator.subsample(proposals, targets)
        x = self.feature_extractor(features, proposals)
        class_logits, box_regression, corners_semantic = self.predictor(x)
        if self.no_corner_loss:
            corners_semantic = None
        if not self.training:
            result = self.post_processor((class_logits, box_regression, corners_semantic), proposals)
            return x, result, {}
        loss_classifier, loss_box_reg, loss_corner_grouping = self.loss_evaluator(
            class_logits, box_regression, corners_semantic, targets=targets)
        roi_loss = self._roi_losses(loss_classifier, loss_box_reg)
        roi_loss.update(loss_corner_grouping)
        return x, proposals, roi_loss


def build_roi_box_head(cfg):
    """the factory the reference's model builder calls"""
    return ROIBoxHead3D(cfg)
