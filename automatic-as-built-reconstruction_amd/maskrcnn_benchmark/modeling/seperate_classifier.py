"""SeperateClassifier, the "separated classifier" of MODEL.SEPARATE_CLASSES (reference:
maskrcnn_benchmark/modeling/seperate_classifier.py), for the box head.  Some classes get a classifier group of their own:
group 0 keeps every class not named (background 0 included), group g >= 1 is one entry of `seperate_classes` behind a
background column of its own, appended after the input classes.  Every proposal carries a `sep_id`, the group whose RPN
branch produced it, and takes part only in its own group's ground truth, logit columns, losses and NMS.

The reference runs its single-group code once per group and scene (nonzero, gathers, one subsample / cross-entropy /
post-processor pass each).  Here each ROI method is ONE grouped call of roi_glue (csrc/roi_loss.hip, csrc/roi_post.hip,
csrc/sep_groups.h): `seperate_subsample`, `roi_cross_entropy_seperated`, `roi_box_loss_seperated`, `post_processor`.
Box regression is class agnostic with groups: the reference's class-specific branch stops in a debugger
(seperate_classifier.py:264-267), so CLASS_SPECIFIC with groups is refused.

Proposals are the duck-typed per-scene lists used everywhere in this package (`.bbox3d` [n, 7], `.size3d`,
`get_field`), with an int field `sep_id`.  Host reads: a per-scene list may carry the HOST attribute `sep_counts` (its G
group sizes; its rows are then group-major) -- `cat_boxlist_3d_seperated` and `seperate_subsample` set it -- and then no
method reads the device.  Without it, `seperate_subsample` and `seperate_proposals` order the batch by one stable sort
and read the per-group counts of the whole batch in ONE read.  The losses and `post_processor` never need the sizes.

The RPN half (MODEL.SEPARATE_RPN: G objectness / regression groups per anchor) works on the instance RPNModule builds,
whose flag is 'RPN' -- the reference builds one instance per role: `seperate_targets`, `seperate_rpn_assin`,
`seperate_rpn_selector` and `seperate_rpn_loss_evaluator` are each ONE grouped call of rpn_glue (rpn_group_targets,
rpn_proposals_grouped, rpn_label_matches_grouped + rpn_loss_grouped).  On an instance of any other flag they raise
NotImplementedError.  `group_id_include_wall`, which only the corner-connection losses read, is left out."""
import torch

import _hip
import roi_glue


def _owner(fn, cls, what):
    """the object behind a bound method (or the object itself), which must be this package's `cls`"""
    obj = fn if isinstance(fn, cls) else getattr(fn, "__self__", None)
    if not isinstance(obj, cls):
        raise TypeError("%s must be a bound method of this package's %s (its thresholds, sampler and coder are read "
                        "from their owner), got %r" % (what, cls.__name__, fn))
    return obj


class SeperateClassifier(object):
    def __init__(self, seperate_classes, num_input_classes, class_specific, flag):
        """seperate_classes: list of lists of original class ids (none 0; each list is sorted ascending here, as the
        reference sorts it); num_input_classes counts the background."""
        self.need_seperate = len(seperate_classes) > 0
        if not self.need_seperate:
            return
        if class_specific:
            raise ValueError("MODEL.CLASS_SPECIFIC with separated-classifier groups is not part of this package: box "
                             "regression is class agnostic whenever groups are on")
        if not all(isinstance(g, (list, tuple)) and len(g) > 0 for g in seperate_classes):
            raise ValueError("seperate_classes must be a list of non-empty lists of class ids, got %r" % (seperate_classes,))
        sep = [sorted(int(c) for c in g) for g in seperate_classes]
        flat = [c for g in sep for c in g]
        if 0 in flat:
            raise ValueError("the background (0) cannot be a separated class: %r" % (seperate_classes,))
        if any(not 0 < c < num_input_classes for c in flat) or len(set(flat)) != len(flat):
            raise ValueError("separated class ids must be distinct and in [1, %d), got %r" % (num_input_classes, seperate_classes))
        self.flag = flag
        self.class_specific = class_specific
        self.num_input_classes = int(num_input_classes)
        remaining = [c for c in range(self.num_input_classes) if c not in flat]
        self.grouped_classes = [remaining] + [[self.num_input_classes + g] + s for g, s in enumerate(sep)]
        self.group_num = len(self.grouped_classes)
        self.seperated_num_classes_total = self.num_input_classes + self.group_num - 1
        self.class_nums = [len(gc) for gc in self.grouped_classes]
        roi_glue.sep_group_tables(self)          # ValueError beyond 8 groups / 32 columns
        self.org_labels_to_sep_labels = torch.full((self.seperated_num_classes_total, 2), -1, dtype=torch.int32)
        self.sep_labels_to_org_labels = [torch.full((n,), -1, dtype=torch.int32) for n in self.class_nums]
        for g, gc in enumerate(self.grouped_classes):
            for i, c in enumerate(gc):
                self.org_labels_to_sep_labels[c] = torch.tensor([g, i], dtype=torch.int32)
                self.sep_labels_to_org_labels[g][i] = c
        self._lut = {}

    # ---- the RPN half: only on the instance RPNModule builds (flag 'RPN'; the reference builds one instance per role) -----
    def _rpn(self, *_a, **_k):
        raise NotImplementedError("the RPN half of the separated classifier (MODEL.SEPARATE_RPN: per-group objectness, "
                                  "label generation and proposals) is a later change; only the box head runs with groups")

    def _rpn_role(fn):
        def method(self, *a, **k):
            if getattr(self, "flag", None) != "RPN":
                self._rpn()
            return fn(self, *a, **k)
        method.__name__, method.__doc__ = fn.__name__, fn.__doc__
        return method

    @_rpn_role
    def seperate_targets(self, targets):
        """a batch's ground truth by group, one call (rpn_glue.rpn_group_targets; ONE host read, none when the labels are
        host tensors): targets = per scene an object with `.bbox3d` [n, 7] and the field `labels` (ORIGINAL ids).
        Returns (boxes[b][g] [n, 7], local_labels[b][g], rows[b][g], counts[b][g]), each group's boxes in the order
        (group-local label, row) in which the reference concatenates them; a label no group owns is dropped.  A value
        this method returned is passed through, so a step splits its targets once."""
        import rpn_glue
        if isinstance(targets, tuple) and len(targets) == 4:
            return targets
        if any(not (hasattr(t, "bbox3d") and hasattr(t, "get_field")) for t in targets):
            raise ValueError("the separated RPN groups need targets that carry their classes (`.bbox3d` and the field "
                             "`labels`); plain box tensors cannot be split by group")
        return rpn_glue.rpn_group_targets([t.bbox3d for t in targets], [t.get_field("labels") for t in targets], self)

    @_rpn_role
    def seperate_targets_and_update_labels(self, targets):
        """-> list over groups of lists over scenes of the group's targets, `labels` GROUP-LOCAL"""
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
        boxes, local, _rows, _counts = self.seperate_targets(targets)
        size = [getattr(t, "size3d", None) for t in targets] if not isinstance(targets, tuple) else [None] * len(boxes)
        return [[DetectionList3D(boxes[b][g], size[b], {"labels": local[b][g]}) for b in range(len(boxes))]
                for g in range(self.group_num)]

    @_rpn_role
    def seperate_rpn_assin(self, targets):
        """splits the step's targets once; the value goes to seperate_rpn_selector / seperate_rpn_loss_evaluator"""
        self.targets_groups = self.seperate_targets(targets)
        return self.targets_groups

    @_rpn_role
    def seperate_rpn_selector(self, rpn, maps, objectness, box_regression, targets, add_gt_proposals, train=True,
                              batch_size=None):
        """RPNPostProcessor with groups, one stage (rpn_glue.rpn_proposals_grouped; ONE host read): `rpn` = this package's
        RPNModule, whose anchors and thresholds apply; objectness / box_regression group-major (RPNHead.forward_flat).
        With `add_gt_proposals` (training) a group gets ITS OWN ground truth with objectness 1.  Returns a list over groups
        of lists over scenes of DetectionList3D with the field `objectness`: what cat_boxlist_3d_seperated accepts."""
        import rpn_glue
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
        from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNModule
        rpn = _owner(rpn, RPNModule, "rpn")
        c, gen = rpn.cfg.MODEL.RPN, rpn.anchor_generator
        pre = c.FPN_PRE_NMS_TOP_N_TRAIN if train else c.FPN_PRE_NMS_TOP_N_TEST
        post = c.FPN_POST_NMS_TOP_N_TRAIN if train else c.FPN_POST_NMS_TOP_N_TEST
        tg = self.seperate_targets(targets) if add_gt_proposals and train else None
        if batch_size is None and tg is not None:
            batch_size = len(tg[0])
        with torch.no_grad():
            props = rpn_glue.rpn_proposals_grouped(maps, [o.detach() for o in objectness],
                                                   [r.detach() for r in box_regression], self.group_num, gen.cell_anchors,
                                                   gen.strides, gen.voxel_scale, pre, post, c.NMS_THRESH,
                                                   tuple(c.NMS_AUG_THICKNESS_Y_Z), batch_size=batch_size)
            out = []
            for g, scenes in enumerate(props):
                row = []
                for b, (box, score) in enumerate(scenes):
                    if tg is not None:
                        gt = tg[0][b][g].to(box.dtype)
                        box = torch.cat([box, gt])
                        score = torch.cat([score, torch.ones(gt.shape[0], dtype=score.dtype, device=score.device)])
                    row.append(DetectionList3D(box, None, {"objectness": score}))
                out.append(row)
        return out

    @_rpn_role
    def seperate_rpn_loss_evaluator(self, rpn, maps, objectness, box_regression, targets):
        """RPNLossComputation with groups: the labels of every (scene, group) segment in one library call per 16
        segments (rpn_glue.rpn_label_matches_grouped), both losses of every group in one grouped call
        (rpn_glue.rpn_loss_grouped).  `rpn` = this package's RPNModule, whose anchors, thresholds and seed apply.
        Returns (list of G objectness losses, list of G box losses), 0-dim each."""
        import rpn_glue
        from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNModule
        rpn = _owner(rpn, RPNModule, "rpn")
        c, gen, G = rpn.cfg.MODEL.RPN, rpn.anchor_generator, self.group_num
        boxes = self.seperate_targets(targets)[0]
        nb = len(boxes)
        flat = [boxes[b][g] for b in range(nb) for g in range(G)]
        labels = rpn_glue.rpn_label_matches_grouped(maps, gen.cell_anchors, gen.strides, gen.voxel_scale, flat, G,
                                                    rpn.label_aug, rpn.cfg.MODEL.IOU_CRITERIA, c.FG_IOU_THRESHOLD,
                                                    c.BG_IOU_THRESHOLD, batch_size=nb, yaw_threshold=c.YAW_THRESHOLD,
                                                    regression_targets=True)
        lo, lb = rpn_glue.rpn_loss_grouped(maps, objectness, box_regression, labels, gen.cell_anchors, G,
                                           c.BATCH_SIZE_PER_IMAGE, c.POSITIVE_FRACTION, rpn.cfg.MODEL.LOSS.YAW_MODE,
                                           seed=rpn.seed)
        return list(lo.unbind(0)), list(lb.unbind(0))

    del _rpn_role

    # ---- utilities ---------------------------------------------------------------------------------------------------
    def update_labels_to_seperated_id(self, labels_seperated_org):
        """list of tensors of ORIGINAL labels -> list of int64 tensors of group-local labels (one table lookup each;
        -1 for a label no group owns)"""
        assert isinstance(labels_seperated_org, list)
        out = []
        for ls in labels_seperated_org:
            lut = self._lut.get(ls.device)
            if lut is None:
                lut = self._lut[ls.device] = self.org_labels_to_sep_labels[:, 1].to(device=ls.device, dtype=torch.int64)
            out.append(lut[ls.long()])
        return out

    def cat_boxlist_3d_seperated(self, bboxes_ls):
        """bboxes_ls: one entry per group, each a list over scenes of that group's proposals -> a list over scenes of
        the groups' proposals one after the other, with the field `sep_id` (int32) and the host attribute `sep_counts`.
        One torch.cat per field and scene; no host read."""
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
        if len(bboxes_ls) != self.group_num:
            raise ValueError("%d groups of proposals, the classifier has %d" % (len(bboxes_ls), self.group_num))
        per_group = [b.seperate_examples() if hasattr(b, "seperate_examples") else list(b) for b in bboxes_ls]
        nb = len(per_group[0])
        out = []
        for b in range(nb):
            parts = [per_group[g][b] for g in range(self.group_num)]
            counts = [len(p) for p in parts]
            dev = parts[0].bbox3d.device
            fields = {k: torch.cat([p.get_field(k) for p in parts])
                      for k in (parts[0].fields() if hasattr(parts[0], "fields") else [])
                      if k != "sep_id" and all(p.has_field(k) for p in parts)}
            fields["sep_id"] = torch.cat([torch.full((n,), g, dtype=torch.int32, device=dev) for g, n in enumerate(counts)])
            d = DetectionList3D(torch.cat([p.bbox3d for p in parts]), parts[0].size3d, fields)
            d.sep_counts = counts
            out.append(d)
        return out

    def _group_major(self, proposals):
        """-> (per scene: bbox3d group-major, its G sizes, None or the int64 permutation that made it group-major).
        Lists with `sep_counts` are taken as they are; otherwise one stable sort over the batch and one host read."""
        G = self.group_num
        if all(getattr(p, "sep_counts", None) is not None for p in proposals):
            return [(p.bbox3d, [int(v) for v in p.sep_counts], None) for p in proposals]
        n_b = [len(p) for p in proposals]
        dev = proposals[0].bbox3d.device
        sid = torch.cat([p.get_field("sep_id").reshape(-1) for p in proposals]).to(torch.int64).clamp(0, G - 1)
        scene = torch.repeat_interleave(torch.arange(len(n_b)), torch.tensor(n_b)).to(dev)      # (host-known sizes)
        key = scene * G + sid
        _, perm = torch.sort(key, stable=True)
        counts = _hip.read_back(torch.bincount(key, minlength=len(n_b) * G).to(torch.int32))   # the one read
        out, r0 = [], 0
        for b, p in enumerate(proposals):
            pb = perm[r0:r0 + n_b[b]] - r0
            out.append((p.bbox3d[pb], [int(v) for v in counts[b * G:(b + 1) * G]], pb))
            r0 += n_b[b]
        return out

    def seperate_proposals(self, proposals):
        """-> (proposals_g, sep_ids_g): proposals_g[g][b] the rows of scene b in group g (ascending row), sep_ids_g[g]
        their indices in the batch's concatenated rows (int64)."""
        G = self.group_num
        gm = self._group_major(proposals)
        proposals_g = [[None] * len(proposals) for _ in range(G)]
        ids_g = [[None] * len(proposals) for _ in range(G)]
        r0 = 0
        for b, (p, (_box, counts, perm)) in enumerate(zip(proposals, gm)):
            if perm is None:
                perm = torch.arange(len(p), device=p.bbox3d.device)
            o = 0
            for g in range(G):
                idx = perm[o:o + counts[g]]
                proposals_g[g][b] = p[idx]
                ids_g[g][b] = idx + r0
                o += counts[g]
            r0 += len(p)
        return proposals_g, [torch.cat(i) for i in ids_g]

    # ---- the box head ------------------------------------------------------------------------------------------------
    def seperate_subsample(self, proposals, targets, subsample_fn):
        """FastRCNNLossComputation.subsample with groups, one call (roi_glue.box_head_targets_grouped).  `subsample_fn`:
        a bound method of the FastRCNNLossComputation whose matcher thresholds, sampler, coder and thickness clamps apply.
        targets keep their ORIGINAL labels; they are filtered by group on the device.  Returns one list per scene: the
        groups' samples one after the other (each in ascending row), fields `labels` (GROUP-LOCAL), `regression_targets`,
        `rows` (the scene's proposal row of each), `sep_id`; host attribute `sep_counts`."""
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss import FastRCNNLossComputation
        ev = _owner(subsample_fn, FastRCNNLossComputation, "subsample_fn")
        s = ev.fg_bg_sampler
        gm = self._group_major(proposals)
        dets = roi_glue.box_head_targets_grouped(
            [g[0] for g in gm], [g[1] for g in gm], [t.bbox3d for t in targets], [t.get_field("labels") for t in targets],
            self, fg_iou=ev.high_threshold, bg_iou=ev.low_threshold, aug_thickness=ev.aug_thickness,
            batch_size_per_image=s.batch_size_per_image, positive_fraction=s.positive_fraction, box_coder=ev.box_coder,
            seed=getattr(s, "seed", None))
        out = []
        for d, p, (_box, _counts, perm) in zip(dets, proposals, gm):
            rows = d["rows"] if perm is None else perm[d["rows"]]
            o = DetectionList3D(d["bbox3d"], p.size3d, {"labels": d["labels"], "regression_targets": d["regression_targets"],
                                                        "rows": rows, "sep_id": d["sep_id"]})
            o.sep_counts = d["sep_counts"]
            out.append(o)
        return out

    def roi_losses_seperated(self, class_logits, box_regression, labels, regression_targets, proposals,
                             yaw_loss_mode="Diff"):
        """both losses of every group in one call (2 launches): (cls_loss [G], box_loss [G], flag), what
        FastRCNNLossComputation.__call__ uses; `proposals` carry `sep_id`."""
        sep_id = torch.cat([p.get_field("sep_id").reshape(-1) for p in proposals])
        return roi_glue.box_head_loss_grouped(class_logits, box_regression, sep_id, labels, regression_targets, self,
                                              yaw_loss_mode=yaw_loss_mode, return_flag=True)

    def roi_cross_entropy_seperated(self, class_logits, labels, proposals):
        """class_logits [n, C_tot], labels [n] group-local, proposals with `sep_id` -> list of G 0-dim losses, group g's
        F.cross_entropy over its rows and columns.  One grouped call (the box term runs on zeros); the rows' groups are
        kept for roi_box_loss_seperated, as the reference keeps `sep_ids_g_roi`."""
        n = int(class_logits.shape[0])
        self._sep_id_roi = torch.cat([p.get_field("sep_id").reshape(-1) for p in proposals])
        zeros = class_logits.new_zeros((n, 7))
        cls, _box = roi_glue.box_head_loss_grouped(class_logits, zeros, self._sep_id_roi, labels, zeros.float(), self)
        return list(cls.unbind(0))

    def roi_box_loss_seperated(self, box_loss_fn, labels, box_regression, regression_targets, pro_bbox3ds, corners_semantic):
        """-> (list of G 0-dim box losses, []) after roi_cross_entropy_seperated.  `box_loss_fn`: a bound method of the
        FastRCNNLossComputation whose yaw mode applies.  The corner-connection losses are not part of this package:
        corners_semantic must be None, and the second value, their list, is empty."""
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss import FastRCNNLossComputation
        ev = _owner(box_loss_fn, FastRCNNLossComputation, "box_loss_fn")
        if corners_semantic is not None:
            raise ValueError("the corner-connection losses (corners_semantic) are not part of this package")
        if getattr(self, "_sep_id_roi", None) is None:
            raise RuntimeError("roi_cross_entropy_seperated needs to be called before")
        zeros = box_regression.new_zeros((int(box_regression.shape[0]), self.seperated_num_classes_total))
        _cls, box = roi_glue.box_head_loss_grouped(zeros, box_regression, self._sep_id_roi, labels, regression_targets,
                                                   self, yaw_loss_mode=ev.yaw_loss_mode)
        return list(box.unbind(0)), []

    def post_processor(self, class_logits, box_regression, corners_semantic, proposals, post_processor_fn):
        """PostProcessor.forward with groups, one call (roi_glue.box_detections_grouped).  `post_processor_fn`: this
        package's PostProcessor (or its bound forward), whose thresholds and coder apply.  Returns one list per scene:
        the groups in ascending order, `labels` ORIGINAL ids (never a background column), `scores`, `rows`."""
        from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D, PostProcessor
        pp = _owner(post_processor_fn, PostProcessor, "post_processor_fn")
        sep_id = torch.cat([p.get_field("sep_id").reshape(-1) for p in proposals])
        dets = roi_glue.box_detections_grouped(
            class_logits, box_regression, [p.bbox3d for p in proposals], sep_id, self, score_thresh=pp.score_thresh,
            nms=pp.nms, nms_aug_thickness=pp.nms_aug_thickness, detections_per_img=pp.detections_per_img,
            box_coder=pp.box_coder)
        return [DetectionList3D(d["bbox3d"], p.size3d, {"scores": d["scores"], "labels": d["labels"], "rows": d["rows"]})
                for d, p in zip(dets, proposals)]
