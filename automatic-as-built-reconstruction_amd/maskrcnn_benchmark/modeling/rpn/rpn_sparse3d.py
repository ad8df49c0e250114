"""The RPN head and RPNModule (reference: maskrcnn_benchmark/modeling/rpn/rpn_sparse3d.py: SingleConvRPNHead_Sparse3D
:81-131, RPNModule :134-303) composed from the device paths of rpn_glue: rpn_head (csrc/rpn_head.hip: one launch per
forward for all maps, two per backward), rpn_proposals, rpn_label_matches and rpn_loss.  Containers are duck-typed: a
scene's proposals are a DetectionList3D (`.bbox3d` [n, 7] yx_zb, `.size3d`, field `objectness`), which ROIBoxHead3D
consumes; targets are objects with `.bbox3d` or plain [G, 7] tensors.  With MODEL.SEPARATE_CLASSES and SEPARATE_RPN (and
SEPARATE_CLASSES_ID, the class ids of each entry) the head has G = len(SEPARATE_CLASSES) + 1 branches (rpn_head_grouped,
the reference's parameter shapes) and RPNModule runs every stage per group as single grouped calls through its
SeperateClassifier: `boxes` is then a list over groups of lists over scenes, the losses are `loss_objectness_{g}` /
`loss_rpn_box_reg_{g}`, and the targets must carry the field `labels`.  Not part of this package: the SHOW_* debug
paths."""
import torch
import torch.nn.functional as F
from torch import nn

import rpn_glue
from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
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
    reference, the yardstick.  Fused, maps in bf16 storage are read in place: fp32 outputs, bf16 gradients to the maps."""
    fused = True

    def __init__(self, cfg, in_channels, num_anchors_per_location):
        super(RPNHead, self).__init__()
        self.num_anchors_per_location = num_anchors_per_location
        self.seperate_rpn = int(len(cfg.MODEL.SEPARATE_CLASSES) * cfg.MODEL.SEPARATE_RPN) + 1
        G = self.seperate_rpn
        if G != 1:
            group_class_ids(cfg)
            if not rpn_glue.rpn_head_group_limits_ok(in_channels, num_anchors_per_location, G):
                raise ValueError("RPNHead with separated RPN groups: C = %d, A = %d, G = %d; supported: %s"
                                 % (in_channels, num_anchors_per_location, G, rpn_glue.RPN_HEAD_GROUP_LIMITS))
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors_per_location * G, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors_per_location * 7 * G, kernel_size=1, stride=1)
        for l in (self.conv, self.cls_logits, self.bbox_pred):
            torch.nn.init.normal_(l.weight, std=0.01)
            torch.nn.init.constant_(l.bias, 0)

    def forward_flat(self, x):
        """(objectness[m] [n A], box_regression[m] [n A, 7]): the [site, yaw] order the rpn_glue consumers read.  With G > 1
        groups: [G, n A] and [G, n A, 7], group-major, each group's slice in that order"""
        rows = [_rows(f) for f in x]
        A, G = self.num_anchors_per_location, self.seperate_rpn
        # fused: bf16 rows are read in place (rpn_glue's feature_dtype); the glue refuses a mix of storages
        storage = torch.bfloat16 if rows and rows[0].dtype == torch.bfloat16 else torch.float32
        if G != 1:
            if self.fused:
                return rpn_glue.rpn_head_grouped(rows, self.conv.weight, self.conv.bias, self.cls_logits.weight,
                                                 self.cls_logits.bias, self.bbox_pred.weight, self.bbox_pred.bias, G,
                                                 feature_dtype=storage)
            logits, bbox = self._forward_reference(rows)
            return ([l.reshape(-1, A, G).permute(2, 0, 1).reshape(G, -1) for l in logits],
                    [b.reshape(-1, A, G, 7).permute(2, 0, 1, 3).reshape(G, -1, 7) for b in bbox])
        if self.fused:
            return rpn_glue.rpn_head(rows, self.conv.weight, self.conv.bias, self.cls_logits.weight, self.cls_logits.bias,
                                     self.bbox_pred.weight, self.bbox_pred.bias, feature_dtype=storage)
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

    def _forward_reference(self, rows):
        """the reference's forward with groups (rpn_sparse3d.py:114-131) on torch's layers: (logits[m] [1, n, A, G],
        bbox_reg[m] [1, n, A, 7 G])"""
        A, G = self.num_anchors_per_location, self.seperate_rpn
        logits, bbox = [], []
        for f in rows:
            if f.shape[0] == 0:         # torch's convolution refuses an empty map
                t = F.relu(F.linear(f, self.conv.weight.flatten(1), self.conv.bias))
                logits.append(F.linear(t, self.cls_logits.weight.flatten(1), self.cls_logits.bias).reshape(1, 0, A, G))
                bbox.append(F.linear(t, self.bbox_pred.weight.flatten(1), self.bbox_pred.bias).reshape(1, 0, A, 7 * G))
                continue
            t = F.relu(self.conv(f.t().unsqueeze(0).unsqueeze(3)))
            lo = self.cls_logits(t).permute(0, 2, 1, 3)
            logits.append(lo.reshape(1, lo.shape[1], A, G))
            rg = self.bbox_pred(t).permute(0, 2, 1, 3)
            bbox.append(rg.reshape(1, rg.shape[1], A, 7 * G))
        return logits, bbox

    def forward(self, x):
        """x: a list over maps of [1, C, n, 1] tensors (the reference), [n, C] rows or SparseConvNetTensors (no
        transpose).  Returns (logits[m] [1, n, A, 1], bbox_reg[m] [1, n, A, 7]); with G > 1 groups the reference's
        [1, n, A, G] and [1, n, A, 7 G] (fused: a permuted view of the group-major result)"""
        A, G = self.num_anchors_per_location, self.seperate_rpn
        if G != 1:
            if not self.fused:
                return self._forward_reference([_rows(f) for f in x])
            obj, reg = self.forward_flat(x)
            return ([o.view(G, -1, A).permute(1, 2, 0).unsqueeze(0) for o in obj],
                    [r.view(G, -1, A, 7).permute(1, 2, 0, 3).reshape(1, -1, A, 7 * G) for r in reg])
        obj, reg = self.forward_flat(x)
        return [o.view(1, o.numel() // A, A, 1) for o in obj], [r.view(1, r.shape[0] // A, A, 7) for r in reg]


def group_class_ids(cfg):
    """cfg.MODEL.SEPARATE_CLASSES_ID of a configuration with separated RPN groups: one list of class ids per entry of
    SEPARATE_CLASSES"""
    names = cfg.MODEL.SEPARATE_CLASSES
    ids = getattr(cfg.MODEL, "SEPARATE_CLASSES_ID", None)
    if ids is None or len(ids) != len(names):
        raise ValueError("cfg.MODEL.SEPARATE_RPN with SEPARATE_CLASSES %r needs cfg.MODEL.SEPARATE_CLASSES_ID, one list of "
                         "class ids per entry, got %r" % (list(names), ids))
    return [list(g) for g in ids]


def _boxes_of(t):
    return t.bbox3d if hasattr(t, "bbox3d") else t


class RPNModule(torch.nn.Module):
    """head -> proposals (and, in training, labels -> losses), all on the device.  forward returns (boxes, losses):
    boxes = one DetectionList3D per scene with the field `objectness` (None in training with RPN__ONLY: the reference
    returns its undecoded anchors there, which this path never materialises); losses = {"loss_objectness",
    "loss_rpn_box_reg"} in training, {} in evaluation.  With separated-classifier groups: see _forward_grouped."""

    def __init__(self, cfg):
        super(RPNModule, self).__init__()
        self.cfg = cfg.clone() if hasattr(cfg, "clone") else cfg
        rpn = cfg.MODEL.RPN
        if rpn.RPN_HEAD != "SingleConvRPNHead_Sparse3D":
            raise ValueError("cfg.MODEL.RPN.RPN_HEAD %r: only SingleConvRPNHead_Sparse3D is part of this package" % (rpn.RPN_HEAD,))
        self.anchor_generator = make_anchor_generator(cfg)
        G = int(len(cfg.MODEL.SEPARATE_CLASSES) * cfg.MODEL.SEPARATE_RPN) + 1
        ids = group_class_ids(cfg) if G != 1 else []
        self.seperate_classifier = SeperateClassifier(ids, len(cfg.INPUT.CLASSES) if G != 1 else 0,
                                                      getattr(cfg.MODEL, "CLASS_SPECIFIC", False), "RPN")
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

    def _forward_grouped(self, maps, targets):
        """forward with separated-classifier groups: `boxes` is a list over groups of lists over scenes (what
        SeperateClassifier.cat_boxlist_3d_seperated accepts), the losses are keyed per group"""
        sc = self.seperate_classifier
        obj, reg = self.head.forward_flat(maps)
        nb = len(targets) if targets is not None else None
        if not self.training:
            boxes = sc.seperate_rpn_selector(self, maps, obj, reg, None, False, train=False, batch_size=nb)
            if self.rpn_only:                                   # the final output: high-to-low confidence
                boxes = [[b[b.get_field("objectness").sort(descending=True)[1]] for b in scenes] for scenes in boxes]
            return boxes, {}
        if targets is None:
            raise ValueError("RPNModule: training needs targets")
        tg = sc.seperate_rpn_assin(list(targets))
        boxes = None
        if not self.rpn_only:
            boxes = sc.seperate_rpn_selector(self, maps, obj, reg, tg, self.add_gt_proposals, train=True, batch_size=nb)
        lo, lb = sc.seperate_rpn_loss_evaluator(self, maps, obj, reg, tg)
        losses = {}
        for g in range(sc.group_num):
            losses["loss_objectness_%d" % g] = lo[g]
            losses["loss_rpn_box_reg_%d" % g] = lb[g]
        return boxes, losses

    def forward(self, inputs_sparse, features_sparse, targets=None):
        maps = list(features_sparse)
        if self.seperate_classifier.need_seperate:
            return self._forward_grouped(maps, targets)
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
