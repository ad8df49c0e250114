"""Base anchors of the RPN (reference: maskrcnn_benchmark/modeling/rpn/anchor_generator_sparse3d.py:46-79, 184-241).
Only the per-location ("cell") anchors are built here: the per-site anchors are generated inside the device kernels from
the maps' site lists (rpn_glue.grid_anchors is their torch form).  A cell anchor is a yx_zb box
[xc, yc, z_bot, y_size, x_size, z_size, yaw] at the origin: with USE_YAWS one box of the level's size per yaw, otherwise
one box per ratio with the size scaled by it and yaw 0.  Values are float32 throughout, as the reference's numpy arrays are."""
import numpy as np
import torch


def generate_anchors_3d(size, yaws, ratios, use_yaw):
    """size (3), yaws (n), ratios [r, 3] -> float32 tensor [n or r, 7]"""
    size = np.asarray(size, np.float32).reshape(3)
    if use_yaw:
        yaws = np.asarray(yaws, np.float32).reshape(-1)
        rows = [[0.0, 0.0, 0.0] + list(size) + [y] for y in yaws]
    else:
        ratios = np.asarray(ratios, np.float32).reshape(-1, 3)
        rows = [[0.0, 0.0, 0.0] + list(size * r) + [0.0] for r in ratios]
    return torch.from_numpy(np.asarray(rows, np.float32).reshape(-1, 7))


class AnchorGenerator(object):
    """the constants of the reference's AnchorGenerator: `cell_anchors[m]` [A, 7], `strides[m]` (3), `voxel_scale`, and
    A = the number of yaws (one size per location)"""

    def __init__(self, voxel_scale, sizes_3d, yaws, ratios, use_yaws, anchor_strides):
        sizes_3d = np.asarray(sizes_3d, np.float32)
        strides = np.asarray(anchor_strides, np.float32)
        if sizes_3d.ndim != 2 or sizes_3d.shape[1] != 3 or strides.shape != sizes_3d.shape:
            raise ValueError("ANCHOR_SIZES_3D and ANCHOR_STRIDE must both be [levels, 3]")
        if len(use_yaws) != len(sizes_3d):
            raise ValueError("USE_YAWS needs one entry per level")
        self.cell_anchors = [generate_anchors_3d(s, yaws, ratios, u) for s, u in zip(sizes_3d, use_yaws)]
        self.anchor_num_per_loc = len(yaws)
        if any(int(c.shape[0]) != self.anchor_num_per_loc for c in self.cell_anchors):
            raise ValueError("every level needs as many anchors per location as there are yaws")
        self.voxel_scale = voxel_scale
        self.strides = [[float(v) for v in s] for s in strides]

    def num_anchors_per_location(self):
        return self.anchor_num_per_loc


def make_anchor_generator(config):
    rpn = config.MODEL.RPN
    return AnchorGenerator(config.SPARSE3D.VOXEL_SCALE, rpn.ANCHOR_SIZES_3D, rpn.YAWS, rpn.RATIOS, rpn.USE_YAWS,
                           rpn.ANCHOR_STRIDE)
