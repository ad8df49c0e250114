"""The RPN head and RPNModule (reference: maskrcnn_benchmark/modeling/rpn/rpn_sparse3d.py: SingleConvRPNHead_Sparse3D
:81-131, RPNModule :134-303) composed from the device paths of rpn_glue: rpn_head (csrc/rpn_head.hip: one launch per
forward for all maps, two per backward), rpn_proposals, rpn_label_matches and rpn_loss.  Containers are duck-typed: a
scene's proposals are a DetectionList3D (`.bbox3d` [n, 7] yx_zb, `.size3d`, field `objectness`), which ROIBoxHead3D
consumes; targets are objects with `.bbox3d` or plain [G, 7] tensors.  Not part of this package: the separated-classifier
RPN groups (SEPARATE_RPN with SEPARATE_CLASSES) and the SHOW_* debug paths."""
import torch
import torch.nn.functional as F
from torch import nn

import rpn_glue
from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
from .anchor_generator_sparse3d import make_anchor_generator


def _rows(x):
    """one map as feature rows [n, C]: a SparseConvNetTensor, rows, or the reference's [1, C, n, 1]"""
    if hasattr(x, "features"):
        return x.features
    if x.dim() == 4:
        if x.shape[0] != 1 or x.shape[3] != 1:
            raise ValueError("RPNHead: a 4-D input must be [1, C, n, 1], got %s" % (tuple(x.shape),))
        return x[0, :, :, 0].t()
    if x.dim() != 2:
        raise ValueError("RPNHead: expected [n, C] rows, [1, C, n, 1] or a SparseConvNetTensor")
    return x


class RPNHead(nn.Module):
    """SingleConvRPNHead_Sparse3D: a 1 x 1 convolution + ReLU, then the objectness and box heads.  The reference's three
    nn.Conv2d parameters under their names, shapes and initialisation, so its state_dict loads.  `fused` (default True):
    rpn_glue.rpn_head, 1 library launch forward and 2 backward for all maps; False: the torch convolutions of the
    reference, the yardstick."""
    fused = True

    def __init__(self, cfg, in_channels, num_anchors_per_location):
        super(RPNHead, self).__init__()
        self.num_anchors_per_location = num_anchors_per_location
        self.seperate_rpn = int(len(cfg.MODEL.SEPARATE_CLASSES) * cfg.MODEL.SEPARATE_RPN) + 1
        if self.seperate_rpn != 1:
            raise ValueError("cfg.MODEL.SEPARATE_RPN with SEPARATE_CLASSES: the separated RPN groups are not part of this "
                             "package")
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors_per_location, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors_per_location * 7, kernel_size=1, stride=1)
        for l in (self.conv, self.cls_logits, self.bbox_pred):
            torch.nn.init.normal_(l.weight, std=0.01)
            torch.nn.init.constant_(l.bias, 0)

    def forward_flat(self, x):
        """(objectness[m] [n A], box_regression[m] [n A, 7]): the [site, yaw] order the rpn_glue consumers read"""
        rows = [_rows(f) for f in x]
        if self.fused:
            return rpn_glue.rpn_head(rows, self.conv.weight, self.conv.bias, self.cls_logits.weight, self.cls_logits.bias,
                                     self.bbox_pred.weight, self.bbox_pred.bias)
        obj, reg = [], []
        for f in rows:
            if f.shape[0] == 0:         # torch's convolution refuses an empty map: the same layers as matrix products,
                t = F.relu(F.linear(f, self.conv.weight.flatten(1), self.conv.bias))    # which keep it in the graph
                obj.append(F.linear(t, self.cls_logits.weight.flatten(1), self.cls_logits.bias).reshape(-1))
                reg.append(F.linear(t, self.bbox_pred.weight.flatten(1), self.bbox_pred.bias).reshape(-1, 7))
                continue
            t = F.relu(self.conv(f.t().unsqueeze(0).unsqueeze(3)))              # [1, C, n, 1]
            obj.append(self.cls_logits(t).permute(0, 2, 1, 3).reshape(-1))      # [1, n, A, 1]
            reg.append(self.bbox_pred(t).permute(0, 2, 1, 3).reshape(-1, 7))    # [1, n, 7 A, 1] -> (site, yaw) rows
        return obj, reg

    def forward(self, x):
        """x: a list over maps of [1, C, n, 1] tensors (the reference), [n, C] rows or SparseConvNetTensors (no
        transpose).  Returns (logits[m] [1, n, A, 1], bbox_reg[m] [1, n, A, 7])"""
        obj, reg = self.forward_flat(x)
        A = self.num_anchors_per_location
        return [o.view(1, o.numel() // A, A, 1) for o in obj], [r.view(1, r.shape[0] // A, A, 7) for r in reg]


def _boxes_of(t):
    return t.bbox3d if hasattr(t, "bbox3d") else t


class RPNModule(torch.nn.Module):
    """head -> proposals (and, in training, labels -> losses), all on the device.  forward returns (boxes, losses):
    boxes = one DetectionList3D per scene with the field `objectness` (None in training with RPN__ONLY: the reference
    returns its undecoded anchors there, which this path never materialises); losses = {"loss_objectness",
    "loss_rpn_box_reg"} in training, {} in evaluation."""

    def __init__(self, cfg):
        super(RPNModule, self).__init__()
        self.cfg = cfg.clone() if hasattr(cfg, "clone") else cfg
        rpn = cfg.MODEL.RPN
        if rpn.RPN_HEAD != "SingleConvRPNHead_Sparse3D":
            raise ValueError("cfg.MODEL.RPN.RPN_HEAD %r: only SingleConvRPNHead_Sparse3D is part of this package" % (rpn.RPN_HEAD,))
        self.anchor_generator = make_anchor_generator(cfg)
        self.head = RPNHead(cfg, cfg.SPARSE3D.nPlaneMap, self.anchor_generator.num_anchors_per_location())
        self.add_gt_proposals = rpn.ADD_GT_PROPOSALS
        self.rpn_only = cfg.MODEL.RPN__ONLY
        ay, az = rpn.LABEL_AUG_THICKNESS_Y_TAR_ANC, rpn.LABEL_AUG_THICKNESS_Z_TAR_ANC
        self.label_aug = {"target_Y": ay[0], "anchor_Y": ay[1], "target_Z": az[0], "anchor_Z": az[1]}
        self.seed = None          # tests: a fixed seed for the loss's anchor sample (None: drawn from torch's generator)

    def _proposals(self, maps, obj, reg, nb, train):
        rpn = self.cfg.MODEL.RPN
        gen = self.anchor_generator
        pre = rpn.FPN_PRE_NMS_TOP_N_TRAIN if train else rpn.FPN_PRE_NMS_TOP_N_TEST
        post = rpn.FPN_POST_NMS_TOP_N_TRAIN if train else rpn.FPN_POST_NMS_TOP_N_TEST
        with torch.no_grad():
            return rpn_glue.rpn_proposals(maps, [o.detach() for o in obj], [r.detach() for r in reg], gen.cell_anchors,
                                          gen.strides, gen.voxel_scale, pre, post, rpn.NMS_THRESH,
                                          tuple(rpn.NMS_AUG_THICKNESS_Y_Z), batch_size=nb)

    def forward(self, inputs_sparse, features_sparse, targets=None):
        maps = list(features_sparse)
        obj, reg = self.head.forward_flat(maps)
        gt = [_boxes_of(t) for t in targets] if targets is not None else None
        nb = len(gt) if gt is not None else None
        if not self.training:
            props = self._proposals(maps, obj, reg, nb, False)
            boxes = [DetectionList3D(b, None, {"objectness": s}) for b, s in props]
            if self.rpn_only:                                   # the final output: high-to-low confidence
                boxes = [b[b.get_field("objectness").sort(descending=True)[1]] for b in boxes]
            return boxes, {}
        if gt is None:
            raise ValueError("RPNModule: training needs targets")
        rpn, gen = self.cfg.MODEL.RPN, self.anchor_generator
        boxes = None
        if not self.rpn_only:
            props = self._proposals(maps, obj, reg, nb, True)
            if self.add_gt_proposals:
                props = [(torch.cat([b, g.to(b.dtype)]), torch.cat([s, torch.ones(g.shape[0], dtype=s.dtype, device=s.device)]))
                         for (b, s), g in zip(props, gt)]
            boxes = [DetectionList3D(b, None, {"objectness": s}) for b, s in props]
        labels = rpn_glue.rpn_label_matches(maps, gen.cell_anchors, gen.strides, gen.voxel_scale, gt, self.label_aug,
                                            self.cfg.MODEL.IOU_CRITERIA, rpn.FG_IOU_THRESHOLD, rpn.BG_IOU_THRESHOLD,
                                            batch_size=nb, yaw_threshold=rpn.YAW_THRESHOLD, regression_targets=True)
        loss_objectness, loss_rpn_box_reg = rpn_glue.rpn_loss(maps, obj, reg, labels, gen.cell_anchors,
                                                              rpn.BATCH_SIZE_PER_IMAGE, rpn.POSITIVE_FRACTION,
                                                              self.cfg.MODEL.LOSS.YAW_MODE, seed=self.seed)
        return boxes, {"loss_objectness": loss_objectness, "loss_rpn_box_reg": loss_rpn_box_reg}


def build_rpn(cfg):
    """the factory the reference's model builder calls"""
    return RPNModule(cfg)
