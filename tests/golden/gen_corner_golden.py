"""Generate tests/golden/corner_golden.npz by IMPORTING the reference's corner-box code and running it on the CPU on
seeded inputs (build container only; needs /root/reference):

  * maskrcnn_benchmark/modeling/box_coder_3d.py:82-122   BoxCoder3D(True, w).encode / decode
  * utils3d/bbox3d_ops_torch.py:8-19,29-55,93-135        adjust_corner_order, Box3D_Torch.from_2corners_to_yxzb /
                                                          from_yxzb_to_2corners
    -> utils3d/bbox3d_ops.py:127-157,524-559,623-653     the numpy loop over boxes (convert_from_yx_zb_boxes, bbox_corners)
    -> utils3d/geometric_util.py:27-36                   Rz
  * second/pytorch/core/box_torch_ops.py:14-79           second_corner_box_encode / second_corner_box_decode

numba / spconv are absent: the decorator-only placeholder modules of gen_iou_golden.py let the modules import (Rz then
runs as plain numpy).  utils3d/bbox3d_ops.py additionally imports `open3d` and `open3d_util` (drawing only: empty
placeholder modules with the two imported names) and uses `np.float`, removed from numpy 1.24 on: `np.float = float`
restores the alias it was.  The reference runs unedited; no vector of the fixture comes from a restatement.

No box sits on the adjust_corner_order tie: the component sum of (corner 0 - centroid) is at least 1e-3 x length in
magnitude for every box that goes through from_yxzb_to_2corners (asserted below), so no comparison of the tests leaves
a case out.  The committed fixture is data only (inputs + expected outputs).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_iou_golden as G  # noqa: E402

REF = "/root/reference"
W2 = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 2.0)


def wall_boxes(rng, n):
    """yx_zb walls [xc, yc, z_bottom, thickness, length, height, yaw]: the yaw column cycles through 0, +-pi/2 (-pi/2 is
    the reference's unrotated branch: yaw + pi/2 == 0), +-(pi/4 +- 0.05) (-pi/4 is the corner-order tie: 0.05 rad off it)
    and uniform draws"""
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-8.0, 8.0, (n, 2))
    b[:, 2] = rng.uniform(0.0, 0.5, n)
    b[:, 3] = rng.uniform(0.05, 0.3, n)
    b[:, 4] = rng.uniform(0.8, 6.0, n)
    b[:, 5] = rng.uniform(1.0, 3.0, n)
    fixed = [0.0, np.pi / 2, -np.pi / 2, np.pi / 4 + 0.05, np.pi / 4 - 0.05, -np.pi / 4 + 0.05, -np.pi / 4 - 0.05]
    yaw = rng.uniform(-np.pi / 2, np.pi / 2, n)
    for i in range(n):
        if i % 10 < len(fixed):
            yaw[i] = fixed[i % 10]
        while abs(np.cos(yaw[i] + np.pi / 2) - np.sin(yaw[i] + np.pi / 2)) < 0.02:   # random draws: keep off the tie
            yaw[i] = rng.uniform(-np.pi / 2, np.pi / 2)
    b[:, 6] = yaw
    b[:, 6] = np.clip(b[:, 6], np.float32(-np.pi / 2), np.float32(np.pi / 2))
    return b


def assert_off_tie(c):
    """c: two-corner boxes [n, 7]"""
    c = c.astype(np.float64)
    cen = (c[:, 0:2] + c[:, 2:4]) / 2
    length = np.hypot(c[:, 2] - c[:, 0], c[:, 3] - c[:, 1])
    assert (np.abs((c[:, 0:2] - cen).sum(1)) >= 1e-3 * length).all(), "a box sits on the adjust_corner_order tie"


def main():
    G._install_placeholders()
    import collections
    import collections.abc
    collections.Iterable = collections.abc.Iterable     # torchplus/train/optim.py:1, as in gen_box_golden.py
    np.float = float                                    # utils3d/bbox3d_ops.py:538 (alias removed in numpy 1.24)
    sys.modules["open3d"] = types.ModuleType("open3d")
    o3u = types.ModuleType("open3d_util")
    o3u.draw_cus = o3u.gen_animation = None
    sys.modules["open3d_util"] = o3u
    sys.path.insert(0, REF)
    bto = importlib.import_module("second.pytorch.core.box_torch_ops")
    coder_mod = importlib.import_module("maskrcnn_benchmark.modeling.box_coder_3d")
    b3t = importlib.import_module("utils3d.bbox3d_ops_torch")
    T = b3t.Box3D_Torch

    out = {}
    rng = np.random.default_rng(11)
    n = 240
    boxes = wall_boxes(rng, n)
    anchors = wall_boxes(rng, n)
    # targets near their anchors, as matched proposals are: the anchor moved, stretched and turned a little
    targets = anchors.copy()
    targets[:, 0:3] += rng.normal(0, 0.2, (n, 3)).astype(np.float32)
    targets[:, 3:6] *= rng.uniform(0.8, 1.25, (n, 3)).astype(np.float32)
    for i in range(n):
        while True:                                      # the turned target keeps off the tie too
            y = float(np.clip(anchors[i, 6] + rng.normal(0, 0.1), -np.pi / 2, np.pi / 2))
            if abs(np.cos(y + np.pi / 2) - np.sin(y + np.pi / 2)) >= 0.02:
                break
        targets[i, 6] = y
    targets[::7] = boxes[::7]                            # and some far from them
    t = torch.from_numpy

    out["boxes"] = boxes.copy()
    out["corners"] = T.from_yxzb_to_2corners(t(boxes.copy())).numpy()
    out["boxes_back"] = T.from_2corners_to_yxzb(t(out["corners"].copy())).numpy()
    assert_off_tie(out["corners"])

    out["anchors"], out["targets"] = anchors.copy(), targets.copy()
    a2c = T.from_yxzb_to_2corners(t(anchors.copy()))
    t2c = T.from_yxzb_to_2corners(t(targets.copy()))
    assert_off_tie(a2c.numpy())
    assert_off_tie(t2c.numpy())
    out["enc_raw"] = bto.second_corner_box_encode(t2c.clone(), a2c.clone(), smooth_dim=True).numpy()

    enc = (rng.standard_normal((n, 7)) * np.array([0.15, 0.15, 0.15, 0.15, 0.2, 0.2, 0.4])).astype(np.float32)
    enc[5, 3:6] = 20000.0                                # beyond bbox_xform_clip (smooth_dim: 10000) at unit weights
    out["dec_enc"] = enc.copy()
    out["dec_raw"] = bto.second_corner_box_decode(t(enc.copy()), a2c.clone(), smooth_dim=True).numpy()
    for name, w in (("w1", None), ("w2", W2)):
        coder = coder_mod.BoxCoder3D(True, w)
        out["weights_%s" % name] = coder.weights.numpy().reshape(7).astype(np.float32)
        out["enc_%s" % name] = coder.encode(t(targets.copy()), t(anchors.copy())).numpy()
        out["dec_%s" % name] = coder.decode(t(enc.copy()), t(anchors.copy())).numpy()
    # the 3-class layout: [n, 7 * num_classes] (box_coder_3d.py:106-111,119-120)
    enc3 = (rng.standard_normal((64, 21)) * 0.15).astype(np.float32)
    out["dec3_enc"] = enc3.copy()
    out["dec3_w2"] = coder_mod.BoxCoder3D(True, W2).decode(t(enc3.copy()), t(anchors[:64].copy())).numpy()
    for k, v in out.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(HERE, "corner_golden.npz"), **out)
    print("wrote corner_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
