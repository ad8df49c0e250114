"""PostProcessor of the box head (reference: maskrcnn_benchmark/modeling/roi_heads/box_head_3d/inference.py:17-189):
class logits, box regression and the proposals of a batch -> per scene the final labelled, scored, NMS-filtered boxes.
The reference loops over scenes and classes in Python; here the whole batch is one call of roi_glue.box_detections
(csrc/roi_post.hip).  `boxes` is duck-typed (`.bbox3d` [n, 7] yx_zb, `.size3d`, `len()`); the result is a small list
object with the surface structures/boxlist_ops_3d.py names -- not a port of BoxList3D.  The coder may be the centroid or
the corner form (MODEL.CORNER_ROI): the kernel decodes in the form of the BoxCoder3D it is given.  `merge_by_corner=True`
(the reference's MERGE_BY_CORNER switch, inference.py:15,82-83; here the optional key MODEL.ROI_HEADS.MERGE_BY_CORNER, off by
default) passes the detections of the whole batch through roi_glue.merge_by_corners (csrc/merge_corners.hip), one more
launch, before the lists are built."""
import torch
from torch import nn

import roi_glue
from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D


class DetectionList3D(object):
    """What PostProcessor.forward returns per scene: `.bbox3d` [m, 7], `.mode == "yx_zb"`, `.size3d`, `get_field`,
    `fields()`, `len()`, `__getitem__` with a LongTensor / mask; fields `scores`, `labels` (int64) and, as an extension,
    `rows` (the scene's proposal row each detection came from)."""
    mode = "yx_zb"

    def __init__(self, bbox3d, size3d, extra_fields=None):
        self.bbox3d = bbox3d
        self.size3d = size3d
        self.extra_fields = dict(extra_fields or {})

    def add_field(self, name, value):
        self.extra_fields[name] = value

    def get_field(self, name):
        return self.extra_fields[name]

    def has_field(self, name):
        return name in self.extra_fields

    def fields(self):
        return list(self.extra_fields.keys())

    def __len__(self):
        return int(self.bbox3d.shape[0])

    def __getitem__(self, item):
        return DetectionList3D(self.bbox3d[item], self.size3d, {k: v[item] for k, v in self.extra_fields.items()})

    def __repr__(self):
        return "DetectionList3D(num_boxes=%d, mode=%s, fields=%s)" % (len(self), self.mode, self.fields())


class PostProcessor(nn.Module):
    def __init__(self, score_thresh=0.05, nms=0.5, nms_aug_thickness=None, detections_per_img=100, box_coder=None,
                 class_specific=True, merge_by_corner=False):
        super(PostProcessor, self).__init__()
        self.score_thresh = score_thresh
        self.nms = nms
        self.detections_per_img = detections_per_img
        if box_coder is None:
            # (the reference's default, BoxCoder3D(weights=(10., 10., 5., 5.)), cannot be constructed: the 3-D coder
            # takes is_corner_roi and 7 weights; every caller passes a coder)
            box_coder = BoxCoder3D(is_corner_roi=False, weights=None)
        roi_glue.coder_args(box_coder)       # ValueError unless it carries seven weights
        self.box_coder = box_coder
        self.nms_aug_thickness = nms_aug_thickness
        self.class_specific = class_specific
        self.merge_by_corner = bool(merge_by_corner)

    def forward(self, x, boxes):
        """x = (class_logits [N, C], box_regression [N, 7 C] or [N, 7], corners_semantic (unused, as upstream));
        boxes: one list of proposals per scene.  Returns one DetectionList3D per scene."""
        class_logits, box_regression, _corners_semantic = x
        dets = roi_glue.box_detections(
            class_logits, box_regression, [b.bbox3d for b in boxes], score_thresh=self.score_thresh, nms=self.nms,
            nms_aug_thickness=self.nms_aug_thickness, detections_per_img=self.detections_per_img,
            class_specific=bool(self.class_specific), box_coder=self.box_coder)
        if self.merge_by_corner:
            merged = roi_glue.merge_by_corners([d["bbox3d"] for d in dets], [d["labels"] for d in dets])
            for d, m in zip(dets, merged):
                d["bbox3d"] = m
        return [DetectionList3D(d["bbox3d"], b.size3d, {"scores": d["scores"], "labels": d["labels"], "rows": d["rows"]})
                for d, b in zip(dets, boxes)]


def make_roi_box_post_processor(cfg):
    roi_glue.corner_roi_check(cfg)
    box_coder = BoxCoder3D(is_corner_roi=cfg.MODEL.CORNER_ROI, weights=cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    return PostProcessor(cfg.MODEL.ROI_HEADS.SCORE_THRESH, cfg.MODEL.ROI_HEADS.NMS,
                         nms_aug_thickness=cfg.MODEL.ROI_HEADS.NMS_AUG_THICKNESS_Y_Z,
                         detections_per_img=cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG, box_coder=box_coder,
                         class_specific=cfg.MODEL.CLASS_SPECIFIC,
                         merge_by_corner=bool(getattr(cfg.MODEL.ROI_HEADS, "MERGE_BY_CORNER", False)))
