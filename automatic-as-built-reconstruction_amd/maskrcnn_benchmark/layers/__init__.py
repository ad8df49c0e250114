"""reference: maskrcnn_benchmark/layers/__init__.py (the 3-D path imports `nms` only,
structures/boxlist_ops_3d.py:7; the RPN loss imports `smooth_l1_loss`, modeling/rpn/loss_3d.py:13)."""
from .nms import nms
from .roi_align_rotated_3d import ROIAlignRotated3D, roi_align_rotated_3d
from .smooth_l1_loss import smooth_l1_loss

__all__ = ["nms", "ROIAlignRotated3D", "roi_align_rotated_3d", "smooth_l1_loss"]
