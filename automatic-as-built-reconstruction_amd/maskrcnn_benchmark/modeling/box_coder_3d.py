"""BoxCoder3D -- regression-target encode / box decode on the device (reference:
maskrcnn_benchmark/modeling/box_coder_3d.py:12-122).  The centroid form is the RPN's: `encode` is what
RPNLossComputation.prepare_targets calls per image (modeling/rpn/loss_3d.py:186-196), `decode` what RPNPostProcessor
calls on the selected anchors (modeling/rpn/inference_3d.py:124-127); in the training step both are fused into the label /
proposal kernels (rpn_glue.rpn_label_matches(regression_targets=True), rpn_glue.rpn_proposals).  The corner form
(`is_corner_roi`, MODEL.CORNER_ROI) is the ROI heads': boxes go through their two-corner form [x0, y0, x1, y1, z0, z1,
thickness] (csrc/corner_box.h); in the box head it is fused into the target and detection kernels
(roi_glue.box_head_targets / box_detections given this coder).  This class is the list form of both; nothing here reads
back to the host (the reference's corner coder walks the boxes in a Python loop on the host)."""
import torch

import _hip
from _hip import check, ptr, stream


class BoxCoder3D(object):
    def __init__(self, is_corner_roi, weights):
        self.is_corner_roi = bool(is_corner_roi)
        self.smooth_dim = True
        self.weights = torch.tensor((1.0,) * 7 if weights is None else weights, dtype=torch.float32).view(1, 7)
        self.bbox_xform_clip = 10000. / 1

    def _w(self):
        return _hip.f32xn(self.weights.view(7).tolist())

    def encode(self, targets, anchors):
        if self.is_corner_roi:
            return self.encode_corner_box(targets, anchors)
        return self.encode_centroid_box(targets, anchors)

    def decode(self, box_encodings, anchors):
        if self.is_corner_roi:
            return self.decode_corner_box(box_encodings, anchors)
        return self.decode_centroid_box(box_encodings, anchors)

    def encode_centroid_box(self, targets, anchors):
        assert targets.shape == anchors.shape and anchors.shape[1] == 7
        t = targets.to(torch.float32).contiguous()
        a = anchors.to(device=t.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(t)
        check(_hip.load().aabr_box_encode(ptr(t), ptr(a), t.shape[0], self._w(), ptr(out), stream()))
        return out

    def decode_centroid_box(self, box_encodings, anchors):
        assert box_encodings.shape[0] == anchors.shape[0]
        assert anchors.shape[1] == 7
        num_classes = int(box_encodings.shape[1] / 7)
        e = box_encodings.to(torch.float32).contiguous()
        a = anchors.to(device=e.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(e)
        check(_hip.load().aabr_box_decode(ptr(e), ptr(a), e.shape[0], num_classes, self._w(),
                                          float(self.bbox_xform_clip), ptr(out), stream()))
        return out

    def encode_corner_box(self, targets_yxzb, anchors_yxzb):
        """box_coder_3d.py:82-91: both lists yx_zb [n, 7]; the encodings are between their two-corner forms"""
        assert targets_yxzb.shape == anchors_yxzb.shape and anchors_yxzb.shape[1] == 7
        t = targets_yxzb.to(torch.float32).contiguous()
        a = anchors_yxzb.to(device=t.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(t)
        check(_hip.load().aabr_box_encode_corner(ptr(t), ptr(a), t.shape[0], self._w(), ptr(out), stream()))
        return out

    def decode_corner_box(self, box_encodings_2corners, proposals_yxzb):
        """box_coder_3d.py:93-122: two-corner encodings [n, 7 * num_classes] against yx_zb proposals [n, 7] -> yx_zb boxes"""
        assert box_encodings_2corners.shape[0] == proposals_yxzb.shape[0]
        assert proposals_yxzb.shape[1] == 7
        num_classes = int(box_encodings_2corners.shape[1] / 7)
        e = box_encodings_2corners.to(torch.float32).contiguous()
        a = proposals_yxzb.to(device=e.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(e)
        check(_hip.load().aabr_box_decode_corner(ptr(e), ptr(a), e.shape[0], num_classes, self._w(),
                                                 float(self.bbox_xform_clip), ptr(out), stream()))
        return out
