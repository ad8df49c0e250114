"""Box3D_Torch -- the conversions between the yx_zb box form and the two-corner form of the ROI heads, on the device
(reference: utils3d/bbox3d_ops_torch.py:21-135).

    yx_zb       [xc, yc, z_bottom, thickness, length, height, yaw - pi/2]
    two corners [x0, y0, x1, y1, z0, z1, thickness]      end points of the bottom centre line along the length

The reference's from_yxzb_to_2corners copies the boxes to the host, loops over them in numpy (Bbox3D.bbox_corners) and
copies back; here each direction is one launch with a thread per box (csrc/corner_box.h through aabr_box_to_2corners /
aabr_box_from_2corners) and nothing is read back."""
import torch

import _hip
from _hip import check, ptr, stream


def _rows(boxes, fn):
    b = boxes.detach().to(torch.float32).contiguous()
    _hip.require_gpu(b)
    out = torch.empty_like(b)
    check(fn(ptr(b), b.numel() // 7, ptr(out), stream()))
    return out


class Box3D_Torch():
    @staticmethod
    def from_yxzb_to_2corners(boxes_in):
        """[n, 7] yx_zb -> [n, 7] two corners; corner 0 is the end whose offset from the centroid has a positive
        component sum (adjust_corner_order: a tie swaps)"""
        assert boxes_in.dim() == 2 and boxes_in.shape[1] == 7
        if boxes_in.shape[0] == 0:
            return boxes_in
        return _rows(boxes_in, _hip.load().aabr_box_to_2corners)

    @staticmethod
    def from_2corners_to_yxzb(boxes, debug=0):
        """[n, 7 k] two corners -> [n, 7 k] yx_zb, yaw in [-pi/2, pi/2)"""
        assert boxes.dim() == 2
        assert boxes.shape[-1] % 7 == 0
        if boxes.shape[0] == 0:
            return boxes.clone()
        return _rows(boxes, _hip.load().aabr_box_from_2corners)
