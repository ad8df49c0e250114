"""Box-head glue on the device: class logits + box regression + proposals -> final detections
(csrc/roi_post.hip, aabr_roi_post_detections).  The counterpart of rpn_glue.rpn_proposals for the second stage:
PostProcessor.forward of the reference (maskrcnn_benchmark/modeling/roi_heads/box_head_3d/inference.py:44-162)
without its Python loops over scenes and classes.  And the training half (csrc/roi_loss.hip): `box_head_targets`
(proposals -> matched, labelled, encoded, sampled: FastRCNNLossComputation.subsample, box_head_3d/loss.py:163-293) and
`box_head_loss` (cross-entropy + per-class smooth-L1 with autograd: FastRCNNLossComputation.__call__, loss.py:295-382).
Between the two, `pool_rois` (csrc/roi_pool.hip): the FPN maps and the sampled proposals -> [N, C, ph, pw, pz] features,
Pooler.forward (modeling/poolers_3d.py:126-168) without its per-level nonzero / index / indexed write.  And what turns
the pooled tensor into the other two (csrc/roi_mlp.hip, a dense fp32 MFMA GEMM family): `dense_linear`, `box_head_mlp`
(FPN2MLPFeatureExtractor after its pooler, roi_box_feature_extractors.py:149-157) and `box_predictions` (FPNPredictor,
roi_box_predictors.py:105-109).  The corner form of the head (MODEL.CORNER_ROI): `box_head_mlp_corner` (fc6 over windows
of the convolution rows, forward_corner_box, roi_box_feature_extractors.py:122-147) and `box_predictions_corner`
(roi_box_predictors.py:79-103); `box_head_targets` / `box_detections` take the coder's form from the BoxCoder3D they are
given."""
import itertools

import torch

import _hip
import _nms
from _hip import check, ptr
from rpn_glue import _Cfg, draw_seed, parse_yaw_loss_mode

def coder_args(box_coder):
    """(weights [7 floats], bbox_xform_clip, corner form 0 / 1) of a BoxCoder3D-like object: what the target and the
    detection kernels need of it.  ValueError for an object that does not carry seven weights."""
    w = getattr(box_coder, "weights", None)
    if not torch.is_tensor(w) or w.numel() != 7:
        raise ValueError("box_coder must be a BoxCoder3D: `weights` holding 7 values, got %r" % (w,))
    return ([float(v) for v in w.reshape(-1).tolist()], float(getattr(box_coder, "bbox_xform_clip", 10000.0)),
            int(bool(getattr(box_coder, "is_corner_roi", False))))


def corner_loss_on(cfg):
    """MODEL.LOSS.CORNER_CONNECTION: the switch of the corner-connection losses (absent = off)"""
    return bool(getattr(getattr(cfg.MODEL, "LOSS", None), "CORNER_CONNECTION", False))


def corner_roi_check(cfg):
    """What MODEL.CORNER_ROI = True asks of the rest of a config, checked wherever a module of the corner box head is
    made (ValueError otherwise; a config that lacks one of the keys is refused the same way):
      MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION[1] == 11 -- the extractor cuts that axis into the corner windows 0..2 and 8..10
        and the body window 2..8 (roi_box_feature_extractors.py:93-94,122-127);
      MODEL.LOSS.WEIGHTS[4:7] == 0 -- with these weights the reference drops corners_semantic (box_head.py:121-122) --
        unless MODEL.LOSS.CORNER_CONNECTION = True switches the corner-connection losses on (`corner_connection_loss`;
        a reference `*_corsem.yaml` needs that one additional line).
    The switch itself is refused without MODEL.CORNER_ROI (there are no corners_semantic) and together with
    separated-classifier groups (MODEL.SEPARATE_CLASSES_ID: in the reference's grouped corner loss each group's subsample
    overwrites the state of the one before, so there is no behaviour to match)."""
    on = corner_loss_on(cfg)
    if on and not cfg.MODEL.CORNER_ROI:
        raise ValueError("MODEL.LOSS.CORNER_CONNECTION needs MODEL.CORNER_ROI = True: the centroid box head has no "
                         "corners_semantic")
    if on and len(getattr(cfg.MODEL, "SEPARATE_CLASSES_ID", None) or ()) > 0:
        raise ValueError("MODEL.LOSS.CORNER_CONNECTION together with separated-classifier groups "
                         "(MODEL.SEPARATE_CLASSES_ID) is not part of this package")
    if not cfg.MODEL.CORNER_ROI:
        return
    res = getattr(getattr(cfg.MODEL, "ROI_BOX_HEAD", None), "POOLER_RESOLUTION", None)
    if res is None or len(res) != 3 or int(res[1]) != 11:
        raise ValueError("MODEL.CORNER_ROI needs MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION[1] == 11 (corner windows 0..2 and "
                         "8..10, body window 2..8), got %r" % (res,))
    lw = getattr(getattr(cfg.MODEL, "LOSS", None), "WEIGHTS", None)
    if lw is None or len(lw) < 7 or (not on and any(float(v) != 0.0 for v in lw[4:7])):
        raise ValueError("MODEL.CORNER_ROI: the corner-connection losses are not part of this path -- "
                         "MODEL.LOSS.WEIGHTS[4:7] must be given and be 0, got MODEL.LOSS.WEIGHTS = %r"
                         "%s" % (lw, "" if on else " (MODEL.LOSS.CORNER_CONNECTION = True switches them on)"))


PRE_NMS, POST_NMS = 2000, 500      # boxlist_nms_3d(flag='roi_post'): rotate_nms_3d(pre_max_size=2000, post_max_size=500)
INFO_WORDS = 8


def box_detections(class_logits, box_regression, proposals, score_thresh=0.05, nms=0.5, nms_aug_thickness=None,
                   detections_per_img=100, weights=None, class_specific=None, defer=False, debug=None,
                   bbox_xform_clip=10000.0, box_coder=None):
    """class_logits [N, C] (class 0 = background), box_regression [N, 7 C] or [N, 7], proposals: list over scenes of
    [n_b, 7] yx_zb tensors whose rows, concatenated, are the N rows of the other two.

    Per scene: softmax, BoxCoder3D.decode, per class the rows above `score_thresh`, rotated NMS the way
    boxlist_nms_3d(flag='roi_post') runs it (2000 best, `nms_aug_thickness` clamps on an NMS-only copy, 500
    survivors), the classes concatenated in ascending order and the `detections_per_img` cut of the reference
    (kthvalue: ties at the cut all stay).  Equal scores inside a class are ordered by ascending proposal row.

    `class_specific`: None = told from the regression's width (7 C: one box per class; 7: one box per row).
    `box_coder`: a BoxCoder3D; given, its weights, clip and form replace `weights` / `bbox_xform_clip` -- with a corner
    coder (`is_corner_roi`) box_regression holds two-corner encodings and the decode is BoxCoder3D.decode_corner_box.
    Returns a list over scenes of dicts: bbox3d [m, 7], scores [m], labels [m] int64, rows [m] int64 (the scene's
    proposal row each detection came from).  All launches go out without a host read; the one read (the counts) is at
    the end -- `defer=True` returns the function that does it, as rpn_glue.rpn_proposals does.  `debug` (a dict)
    receives `prob` [N, C] and `boxes` [N, C, 7]."""
    return _detections(class_logits, box_regression, proposals, None, None, class_specific, score_thresh, nms,
                       nms_aug_thickness, detections_per_img, weights, bbox_xform_clip, box_coder, defer, debug)


def _detections(class_logits, box_regression, proposals, sep_id, tables, class_specific, score_thresh, nms,
                nms_aug_thickness, detections_per_img, weights, bbox_xform_clip, box_coder, defer, debug):
    """box_detections (`tables` None) and box_detections_grouped (`tables` = (G, C_tot, class_nums, cols) of
    sep_group_tables, `sep_id` [N]; class-agnostic regression) as one path: casts and shape checks, the proposals
    concatenated, the empty case, the coder's arguments, scratch, outputs and debug buffers, the one library call and the
    finish()"""
    lib = _hip.load()
    _hip.require_gpu(class_logits)
    dev = class_logits.device
    logits = class_logits.to(torch.float32).contiguous()
    reg = box_regression.to(device=dev, dtype=torch.float32).contiguous()
    N, nc = int(logits.shape[0]), int(logits.shape[1])
    if tables is not None:
        if nc != tables[1]:
            raise ValueError("class_logits must be [N, %d] (C_tot of the groups), got %s" % (tables[1], tuple(logits.shape)))
        if tuple(reg.shape) != (N, 7):
            raise ValueError("box_regression must be [%d, 7] (class agnostic with groups), got %s" % (N, tuple(reg.shape)))
    else:
        if class_specific is None:
            class_specific = reg.shape[1] == 7 * nc and nc != 1
        if reg.shape[0] != N or reg.shape[1] != (7 * nc if class_specific else 7):
            raise ValueError("box_regression must be [N, %d], got %s" % (7 * nc if class_specific else 7, tuple(reg.shape)))
    n_b = [int(p.shape[0]) for p in proposals]
    nb = len(n_b)
    if nb == 0 and N == 0:
        return (lambda: []) if defer else []
    if tables is not None and (sum(n_b) != N or sep_id.numel() != N):
        raise ValueError("the proposals have %d rows, sep_id %d, class_logits %d" % (sum(n_b), sep_id.numel(), N))
    if sum(n_b) != N:
        raise ValueError("the proposals have %d rows, class_logits %d" % (sum(n_b), N))
    props = torch.cat([p.reshape(-1, 7) for p in proposals]).to(device=dev, dtype=torch.float32).contiguous()
    if tables is not None:
        sid = sep_id.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        fn, limits = "box_detections_grouped", "(1 <= scenes <= 16): C_tot=%d nb=%d"
        entry = lib.aabr_roi_post_detections_grouped
        head = (ptr(logits), ptr(reg), ptr(props), ptr(sid), nb, _hip.i64xn(n_b)) + tuple(tables)
        cap, boxes_shape = (nc - tables[0]) * POST_NMS, (N, 7)
    else:
        fn, limits = "box_detections", "(2 <= classes <= 32, 1 <= scenes <= 16): C=%d nb=%d"
        entry = lib.aabr_roi_post_detections_coder
        head = (ptr(logits), ptr(reg), ptr(props), nb, _hip.i64xn(n_b), nc, int(bool(class_specific)))
        cap, boxes_shape = (nc - 1) * POST_NMS, (N, nc, 7)
    aug = (0.0, 0.0) if nms_aug_thickness is None else nms_aug_thickness
    w = (1.0,) * 7 if weights is None else [float(v) for v in torch.as_tensor(weights).reshape(-1).tolist()]
    corner = 0
    if box_coder is not None:
        w, bbox_xform_clip, corner = coder_args(box_coder)
    words = int(lib.aabr_roi_post_scratch_words(nb, max(n_b) if n_b else 0, nc, PRE_NMS))
    if words < 0:
        raise _hip.AabrError("%s: unsupported shape %s" % (fn, limits % (nc, nb)))
    scratch = _hip.workspace("roi_post", words + 2, torch.int32, dev)
    off = (-scratch.data_ptr() // 4) % 2                                  # 8-byte alignment of the first word
    prob = boxes = None
    if debug is not None:
        prob = torch.empty((N, nc), dtype=torch.float32, device=dev)
        boxes = torch.empty(boxes_shape, dtype=torch.float32, device=dev)
    det_rows = torch.empty((nb, cap), dtype=torch.int64, device=dev)
    det_labels = torch.empty((nb, cap), dtype=torch.int64, device=dev)
    det_scores = torch.empty((nb, cap), dtype=torch.float32, device=dev)
    det_boxes = torch.empty((nb, cap, 7), dtype=torch.float32, device=dev)
    info = torch.empty((nb, INFO_WORDS), dtype=torch.int32, device=dev)
    check(entry(
        *head, _hip.f32xn(w), corner, float(bbox_xform_clip), float(score_thresh), float(nms), float(aug[0]), float(aug[1]),
        int(_nms.REFERENCE_DEBUG_ONLY_XY), PRE_NMS, POST_NMS, int(detections_per_img), ptr(prob), ptr(boxes),
        ptr(det_rows), ptr(det_labels), ptr(det_scores), ptr(det_boxes), ptr(info), scratch.data_ptr() + 4 * off,
        _hip.stream()))
    if debug is not None:
        debug["prob"], debug["boxes"] = prob, boxes

    def finish():
        counts = _hip.read_back(info)                                     # the one read of the stage
        if debug is not None:
            debug["info"] = counts
        out = []
        for b in range(nb):
            m = counts[b][0]
            out.append({"bbox3d": det_boxes[b, :m], "scores": det_scores[b, :m], "labels": det_labels[b, :m],
                        "rows": det_rows[b, :m]})
        return out

    return finish if defer else finish()


def merge_corners_max_walls():
    """walls (and, the wall count being known on the device only, rows) per scene that csrc/merge_corners.hip is built for"""
    return int(_hip.load().aabr_merge_corners_max_walls())


def merge_by_corners(bbox3d_list, labels_list=None, threshold=0.1, wall_label=1, return_merged=False):
    """merge_by_corners of the reference (maskrcnn_benchmark/structures/bounding_box_3d.py:843-923) for a list of scenes in
    ONE launch (csrc/merge_corners.hip, aabr_merge_walls_by_corners; the definition is in include/aabr_hip.h).

    bbox3d_list: per scene [n_b, 7] yx_zb; labels_list: per scene [n_b] labels -- the rows with `wall_label` are the
    scene's walls -- or None: every row is a wall (merge_walls_by_corners).  Wall ends closer than `threshold` are
    snapped to their mean in the reference's sequential order and the walls rebuilt from the snapped corners; every wall
    of a scene takes the scene's mean z0, as upstream.  Returns the list of new [n_b, 7] tensors (other rows: the
    input's bits); with return_merged also the list of [n_b, 2] int32 flags (1: that corner of the wall was merged).
    No host read.  ValueError before any device call for lists of different length, a shape that is not [n, 7], labels
    that do not match their boxes, or a scene with more rows than merge_corners_max_walls()."""
    bbox3d_list = list(bbox3d_list)
    if labels_list is not None:
        labels_list = list(labels_list)
        if len(labels_list) != len(bbox3d_list):
            raise ValueError("merge_by_corners: %d box lists and %d label lists" % (len(bbox3d_list), len(labels_list)))
    n_b = []
    for b, boxes in enumerate(bbox3d_list):
        if boxes.dim() != 2 or boxes.shape[1] != 7:
            raise ValueError("merge_by_corners: scene %d: boxes must be [n, 7] yx_zb, got %s" % (b, tuple(boxes.shape)))
        if labels_list is not None and labels_list[b].numel() != boxes.shape[0]:
            raise ValueError("merge_by_corners: scene %d has %d boxes and %d labels"
                             % (b, boxes.shape[0], labels_list[b].numel()))
        n_b.append(int(boxes.shape[0]))
    limit = merge_corners_max_walls()
    if n_b and max(n_b) > limit:
        raise ValueError("merge_by_corners: scene %d has %d rows; the kernel is built for at most %d walls per scene, and "
                         "a scene's wall count is known on the device only, so its row count is held to that limit"
                         % (n_b.index(max(n_b)), max(n_b), limit))
    if not n_b:
        return ([], []) if return_merged else []
    _hip.require_gpu(bbox3d_list[0])
    dev = bbox3d_list[0].device
    N = sum(n_b)
    boxes = torch.cat([b.reshape(-1, 7) for b in bbox3d_list]).to(device=dev, dtype=torch.float32).contiguous()
    labels = None
    if labels_list is not None:
        labels = torch.cat([l.reshape(-1) for l in labels_list]).to(device=dev, dtype=torch.int64).contiguous()
    out = torch.empty_like(boxes)
    merged = torch.empty((N, 2), dtype=torch.int32, device=dev) if return_merged else None
    if N > 0:
        begin = torch.tensor([0] + list(itertools.accumulate(n_b)), dtype=torch.int64).to(dev)   # host lengths: no read
        check(_hip.load().aabr_merge_walls_by_corners(ptr(boxes), ptr(labels), N, ptr(begin), len(n_b), max(n_b),
                                                      int(wall_label), float(threshold), ptr(out), ptr(merged),
                                                      _hip.stream()))
    outs = list(torch.split(out, n_b))
    return (outs, list(torch.split(merged, n_b))) if return_merged else outs


def _targets_inputs(proposals, targets, target_labels, aug_thickness, weights, box_coder, seed):
    """the prologue box_head_targets and box_head_targets_grouped share (at least one scene): the scenes' rows
    concatenated and cast, the clamp list, the coder's arguments and the seed ->
    (dev, n_b, g_b, props, tg, tl, aug, w, corner, seed)"""
    _hip.require_gpu(proposals[0])
    dev = proposals[0].device
    n_b = [int(p.shape[0]) for p in proposals]
    g_b = [int(t.shape[0]) for t in targets]
    if any(int(l.numel()) != g for l, g in zip(target_labels, g_b)):
        raise ValueError("target_labels do not match the targets")
    props = torch.cat([p.reshape(-1, 7) for p in proposals]).to(device=dev, dtype=torch.float32).contiguous()
    tg = torch.cat([t.reshape(-1, 7) for t in targets]).to(device=dev, dtype=torch.float32).contiguous()
    tl = torch.cat([l.reshape(-1) for l in target_labels]).to(device=dev, dtype=torch.int64).contiguous()
    aug = aug_thickness or {}
    aug = [float(aug.get(k, 0.0)) for k in ("target_Y", "target_Z", "anchor_Y", "anchor_Z")]
    w = (1.0,) * 7 if weights is None else [float(v) for v in torch.as_tensor(weights).reshape(-1).tolist()]
    corner = 0
    if box_coder is not None:
        w, _clip, corner = coder_args(box_coder)
    return dev, n_b, g_b, props, tg, tl, aug, w, corner, int(draw_seed() if seed is None else seed) & 0xffffffff


def _targets_run(entry, head, iou, N, S, B, words, dev, aug, fg_iou, bg_iou, w, corner, seed, positive_fraction, info):
    """the library call of box_head_targets and box_head_targets_grouped, `entry(*head, <what both take alike>)`: the
    per-proposal arrays over N rows and the padded samples of S segments, keyed as `debug` receives them (and in the order
    the library takes them), the aligned scratch of `words` words, `iou` = the arguments between the two sets (the plain
    entry's matrix, nothing for the grouped one) -> the arrays"""
    scratch = _hip.workspace("roi_targets", words + 2, torch.int32, dev)
    off = (-scratch.data_ptr() // 4) % 2                                  # 8-byte alignment of the first word
    i64, f32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)
    bufs = {"matched_idx": torch.empty(N, **i64), "matched_val": torch.empty(N, **f32),
            "labels": torch.empty(N, **i64), "regression_targets": torch.empty((N, 7), **f32),
            "samp_rows": torch.empty((S, B), **i64), "samp_labels": torch.empty((S, B), **i64),
            "samp_targets": torch.empty((S, B, 7), **f32), "samp_boxes": torch.empty((S, B, 7), **f32)}
    per_row, samples = list(bufs.values())[:4], list(bufs.values())[4:]
    check(entry(*head, _hip.f32x4(aug), -1, int(_nms.REFERENCE_DEBUG_ONLY_XY), float(fg_iou), float(bg_iou), _hip.f32xn(w),
                corner, seed, B, int(B * positive_fraction), *[ptr(t) for t in per_row], *iou, *[ptr(t) for t in samples],
                ptr(info), scratch.data_ptr() + 4 * off, _hip.stream()))
    return bufs


def _targets_finish(infos, debug, defer, scenes):
    """the one host read of a target stage: `infos` int32 [k, S, 8] (block 0: the samples' counts, `debug`'s `info`);
    scenes(<the blocks read>) -> the list over scenes.  `defer`: the function that does it is returned instead."""
    def finish():
        read = _hip.read_back(infos)                                      # the one read of the stage
        if debug is not None:
            debug["info"] = read[0]
        return scenes(read)

    return finish if defer else finish()


def box_head_targets(proposals, targets, target_labels, fg_iou=0.5, bg_iou=0.5, aug_thickness=None,
                     batch_size_per_image=500, positive_fraction=0.25, weights=None, seed=None, defer=False, debug=None,
                     box_coder=None, corner_groups=False):
    """proposals / targets: lists over scenes of [n_b, 7] / [G_b, 7] yx_zb device tensors, target_labels: list of int64
    [G_b].  Per scene what FastRCNNLossComputation.subsample does (box_head_3d/loss.py:163-293): IoU of every proposal
    with the scene's ground truth (`boxlist_iou_3d(target, proposal, aug_thickness, criterion=-1)`), Matcher(fg_iou,
    bg_iou, allow_low_quality_matches=False), labels (class of the match / 0 background / -1 ignored), regression targets
    `BoxCoder3D(weights).encode(target[matched.clamp(min=0)], proposal)`, BalancedPositiveNegativeSampler(
    batch_size_per_image, positive_fraction) by the library's hash rule (include/aabr_hip.h, aabr_sample_list), and the
    sampled rows in ascending proposal row.  A scene without ground truth has all its proposals background; a scene
    without proposals yields an empty sample (the reference raises there).

    `box_coder`: a BoxCoder3D; given, its weights and form replace `weights` -- with a corner coder (`is_corner_roi`)
    the regression targets are BoxCoder3D.encode_corner_box; matching, labels and the sample do not depend on it.
    `aug_thickness`: dict with target_Y / target_Z / anchor_Y / anchor_Z (None: no clamps).  `seed=None` draws one from
    torch's default CPU generator (rpn_glue.draw_seed).
    Returns a list over scenes of dicts: rows int64 [m] (scene-local proposal rows), bbox3d [m, 7], labels int64 [m],
    regression_targets fp32 [m, 7].  One library call (1 memset + 6 launches whatever the batch), no host read until the
    counts are read at the end -- `defer=True` returns the function that does it, as box_detections does.  `debug` (a
    dict) receives the per-proposal arrays `matched_idx`, `matched_val`, `labels`, `regression_targets` (scene-major
    concatenations), `iou` (list of [G_b, n_b] matrices), `info` (after the read) and the padded `samp_*` arrays.

    `corner_groups=True` (the label side of `corner_connection_loss`, csrc/corner_loss.hip: 3 more launches whatever the
    batch, the same one host read): each scene's dict also carries, over its p positives -- the sampled rows with a
    matched target, ordered by (matched target, row) --, `pos_pos` int64 [p] (positions in the scene's sample),
    `connect_ids` int32 [2 p, 8] and `corner_xyz` fp32 [2 p, 3]; `debug` also receives `tg_xyz`, `tg_connect` and
    `corner_info`.  The sample is the same with and without the flag."""
    lib = _hip.load()
    nb = len(proposals)
    if not (nb == len(targets) == len(target_labels)):
        raise ValueError("proposals, targets and target_labels differ in length")
    if nb == 0:
        return (lambda: []) if defer else []
    dev, n_b, g_b, props, tg, tl, aug, w, corner, seed = _targets_inputs(proposals, targets, target_labels, aug_thickness,
                                                                         weights, box_coder, seed)
    B = int(batch_size_per_image)
    words = int(lib.aabr_roi_targets_scratch_words(nb))
    if words < 0:
        raise _hip.AabrError("box_head_targets: 1 <= scenes <= 16, got %d" % nb)
    iou = torch.empty(sum(n * g for n, g in zip(n_b, g_b)), dtype=torch.float32, device=dev) if debug is not None else None
    infos = torch.empty((2 if corner_groups else 1, nb, INFO_WORDS), dtype=torch.int32, device=dev)
    bufs = _targets_run(lib.aabr_roi_targets_coder, (ptr(props), ptr(tg), ptr(tl), nb, _hip.i64xn(n_b), _hip.i64xn(g_b)),
                        (ptr(iou),), sum(n_b), nb, B, words, dev, aug, fg_iou, bg_iou, w, corner, seed, positive_fraction,
                        infos[0])
    midx, s_rows, s_labels, s_targets, s_boxes = (bufs[k] for k in ("matched_idx", "samp_rows", "samp_labels",
                                                                    "samp_targets", "samp_boxes"))
    if corner_groups:
        G = sum(g_b)
        tg_xyz = torch.empty((2 * G, 3), dtype=torch.float32, device=dev)
        tg_connect = torch.empty((2 * G, 3), dtype=torch.int32, device=dev)
        c_pos = torch.empty((nb, B), dtype=torch.int64, device=dev)
        c_ids = torch.empty((nb, 2 * B, 8), dtype=torch.int32, device=dev)
        c_xyz = torch.empty((nb, 2 * B, 3), dtype=torch.float32, device=dev)
        check(lib.aabr_corner_tables(ptr(tg), nb, _hip.i64xn(n_b), _hip.i64xn(g_b), ptr(midx), ptr(s_rows), ptr(s_boxes), B,
                                     ptr(tg_xyz), ptr(tg_connect), ptr(c_pos), ptr(c_ids), ptr(c_xyz), ptr(infos[1]),
                                     _hip.stream()))
        if debug is not None:
            debug.update(tg_xyz=tg_xyz, tg_connect=tg_connect)
    if debug is not None:
        debug.update(bufs, seed=seed)
        mats, o = [], 0
        for n, g in zip(n_b, g_b):
            mats.append(iou[o:o + n * g].view(g, n))
            o += n * g
        debug["iou"] = mats

    def scenes(both):
        if debug is not None and corner_groups:
            debug["corner_info"] = both[1]
        out = []
        for b in range(nb):
            m = both[0][b][0]
            out.append({"rows": s_rows[b, :m], "bbox3d": s_boxes[b, :m], "labels": s_labels[b, :m],
                        "regression_targets": s_targets[b, :m]})
            if corner_groups:
                p = both[1][b][0]
                out[b].update(pos_pos=c_pos[b, :p], connect_ids=c_ids[b, :2 * p], corner_xyz=c_xyz[b, :2 * p])
        return out

    return _targets_finish(infos, debug, defer, scenes)


CORNER_LOSS_KEYS = ("geometric_pull_loss", "semantic_pull_loss", "semantic_push_loss")    # loss.py:496-498


class _CornerLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sem, seg_rows, pos_pos, connect_ids, corner_xyz):
        lib = _hip.load()
        dev = sem.device
        sem_c = sem.contiguous()
        nb, n = len(seg_rows), int(sem.shape[0])
        tabs = ([t.contiguous() for t in pos_pos], [t.contiguous() for t in connect_ids],
                [t.contiguous() for t in corner_xyz])
        args = (n, nb, _hip.i64xn(seg_rows), _hip.i64xn([int(t.shape[0]) for t in pos_pos]), _hip.ptrs(tabs[0]),
                _hip.ptrs(tabs[1]), _hip.ptrs(tabs[2]))
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        counts = torch.empty((nb, 4), dtype=torch.int32, device=dev)
        scr = _hip.workspace("corner_loss", int(lib.aabr_corner_loss_scratch_words(nb)), torch.int32, dev)
        check(lib.aabr_corner_loss_forward(ptr(sem_c), *args, ptr(losses), ptr(counts), ptr(scr), _hip.stream()))
        ctx.save_for_backward(sem_c, counts, *(tabs[0] + tabs[1] + tabs[2]))
        ctx.args = args
        geo, pull, push = losses.unbind(0)
        ctx.mark_non_differentiable(geo, counts)              # the geometric loss depends on the proposals only
        return geo, pull, push, counts

    @staticmethod
    def backward(ctx, _g_geo, g_pull, g_push, _g_counts):
        lib = _hip.load()
        sem, counts = ctx.saved_tensors[:2]
        dev = sem.device
        g_pull = (g_pull if g_pull is not None else torch.zeros((), device=dev)).float().contiguous()
        g_push = (g_push if g_push is not None else torch.zeros((), device=dev)).float().contiguous()
        d_sem = torch.empty_like(sem)                                           # the kernel writes every element
        check(lib.aabr_corner_loss_backward(ptr(sem), *ctx.args, ptr(counts), ptr(g_pull), ptr(g_push), ptr(d_sem),
                                            _hip.stream()))
        return d_sem, None, None, None, None


def corner_connection_loss(corners_semantic, seg_rows, pos_pos, connect_ids, corner_xyz, return_counts=False):
    """FastRCNNLossComputation.corner_connection_loss (box_head_3d/loss.py:384-499) over the concatenated samples of a
    batch.  corners_semantic fp32 [n, 16] (corner 0's 8 values, then corner 1's; any other dtype raises TypeError: the
    predictor's output is fp32); the scenes are segments of its rows: seg_rows[b] = rows of scene b's sample, and pos_pos /
    connect_ids / corner_xyz are the per-scene lists `box_head_targets(corner_groups=True)` returns (int64 [p_b], int32
    [2 p_b, 8], fp32 [2 p_b, 3]).  The segments may differ in length; a scene without positives adds 0 to each loss and
    still counts in the batch divisor.  Returns {"geometric_pull_loss", "semantic_pull_loss", "semantic_push_loss"}: 0-dim
    fp32 device tensors, the semantic two with autograd to corners_semantic (the geometric one depends on the proposals
    only).  Forward 2 launches, backward 1, whatever the batch; no host read; bit-identical run to run.
    `return_counts=True` appends the int32 [nb, 4] device tensor of the per-scene counts (geometric entries below the
    threshold, connected pairs, push pairs, corners)."""
    lib = _hip.load()
    if not torch.is_tensor(corners_semantic) or corners_semantic.dtype != torch.float32:
        raise TypeError("corner_connection_loss: corners_semantic must be a float32 tensor, got %s"
                        % (getattr(corners_semantic, "dtype", type(corners_semantic)),))
    if corners_semantic.dim() != 2 or corners_semantic.shape[1] != 16:
        raise ValueError("corner_connection_loss: corners_semantic must be [n, 16], got %s" % (tuple(corners_semantic.shape),))
    seg_rows = [int(m) for m in seg_rows]
    nb = len(seg_rows)
    if not (nb == len(pos_pos) == len(connect_ids) == len(corner_xyz)):
        raise ValueError("corner_connection_loss: seg_rows, pos_pos, connect_ids and corner_xyz differ in length")
    if int(lib.aabr_corner_loss_scratch_words(nb)) < 0:
        raise _hip.AabrError("corner_connection_loss: 1 <= scenes <= 16, got %d" % nb)
    if sum(seg_rows) != int(corners_semantic.shape[0]):
        raise ValueError("corner_connection_loss: the scenes have %d sampled rows, corners_semantic %d"
                         % (sum(seg_rows), int(corners_semantic.shape[0])))
    for b in range(nb):
        p = int(pos_pos[b].shape[0])
        if (pos_pos[b].dtype != torch.int64 or connect_ids[b].dtype != torch.int32 or corner_xyz[b].dtype != torch.float32
                or tuple(connect_ids[b].shape) != (2 * p, 8) or tuple(corner_xyz[b].shape) != (2 * p, 3)):
            raise ValueError("corner_connection_loss: scene %d needs pos_pos int64 [p], connect_ids int32 [2 p, 8] and "
                             "corner_xyz float32 [2 p, 3]" % b)
        if p > seg_rows[b] or p > 512:
            raise ValueError("corner_connection_loss: scene %d has %d positives (at most its %d sampled rows and 512)"
                             % (b, p, seg_rows[b]))
    _hip.require_gpu(corners_semantic)
    geo, pull, push, counts = _CornerLoss.apply(corners_semantic, seg_rows, list(pos_pos), list(connect_ids),
                                                list(corner_xyz))
    out = dict(zip(CORNER_LOSS_KEYS, (geo, pull, push)))
    return (out, counts) if return_counts else out


class _BoxHeadLoss(torch.autograd.Function):
    """`tables` None: the plain entry points, 0-dim losses (`sep_id` None).  Else (G, C_tot, class_nums, cols) of
    sep_group_tables: the grouped entry points, losses [G], `sep_id` int32 [n], class-agnostic regression."""

    @staticmethod
    def forward(ctx, logits, reg, sep_id, labels, targets, tables, class_specific, beta):
        lib = _hip.load()
        dev = logits.device
        grouped = tables is not None
        logits_c, reg_c = logits.contiguous(), reg.contiguous()
        shape = (tables[0],) if grouped else ()
        cls_loss = torch.empty(shape, dtype=torch.float32, device=dev)
        box_loss = torch.empty(shape, dtype=torch.float32, device=dev)
        rows = torch.empty(shape, dtype=torch.int32, device=dev) if grouped else None      # n_g, for the backward
        flag = torch.empty((), dtype=torch.int32, device=dev)
        if grouped:
            entry, words = lib.aabr_roi_box_loss_grouped_forward, lib.aabr_roi_box_loss_grouped_scratch_floats()
        else:
            entry, words = lib.aabr_roi_box_loss_forward, lib.aabr_roi_box_loss_scratch_floats()
        scr = _hip.workspace("roi_box_loss_grouped" if grouped else "roi_box_loss", int(words), torch.float32, dev)
        # what the four entry points take between box_regression and labels; `rows` is an argument of the grouped two only
        ctx.form = (int(logits.dtype == torch.bfloat16), int(logits.shape[0])) + (
            tuple(tables) + (ptr(sep_id),) if grouped else (int(logits.shape[1]), int(class_specific)))
        check(entry(ptr(logits_c), ptr(reg_c), *ctx.form, ptr(labels), ptr(targets), beta, ptr(cls_loss), ptr(box_loss),
                    *([ptr(rows)] if grouped else []), ptr(flag), ptr(scr), _hip.stream()))
        ctx.save_for_backward(logits_c, reg_c, labels, targets, sep_id, rows)
        ctx.beta, ctx.shape = beta, shape
        ctx.mark_non_differentiable(flag)
        return cls_loss, box_loss, flag

    @staticmethod
    def backward(ctx, g_cls, g_box, _g_flag):
        lib = _hip.load()
        logits, reg, labels, targets, _sep_id, rows = ctx.saved_tensors   # (sep_id is kept alive: ctx.form holds its address)
        dev, grouped = logits.device, rows is not None
        g_cls = (g_cls if g_cls is not None else torch.zeros(ctx.shape, device=dev)).float().contiguous()
        g_box = (g_box if g_box is not None else torch.zeros(ctx.shape, device=dev)).float().contiguous()
        d_logits, d_reg = torch.empty_like(logits), torch.empty_like(reg)       # the kernel writes every element
        entry = lib.aabr_roi_box_loss_grouped_backward if grouped else lib.aabr_roi_box_loss_backward
        check(entry(ptr(logits), ptr(reg), *ctx.form, ptr(labels), ptr(targets), ctx.beta, *([ptr(rows)] if grouped else []),
                    ptr(g_cls), ptr(g_box), ptr(d_logits), ptr(d_reg), _hip.stream()))
        return d_logits, d_reg, None, None, None, None, None, None


BOX_LOSS_BETA = 1.0 / 5      # box_head_3d/loss.py:374


def _box_head_loss(class_logits, box_regression, sep_id, labels, regression_targets, tables, class_specific, return_flag):
    """the checks, the casts and the call of box_head_loss (`tables` None) and box_head_loss_grouped (`tables` of
    sep_group_tables and `sep_id`; class-agnostic regression)"""
    if class_logits.dim() != 2 or box_regression.dim() != 2:
        raise ValueError("class_logits and box_regression must be 2-D")
    n, nc = int(class_logits.shape[0]), int(class_logits.shape[1])
    if tables is not None and nc != tables[1]:
        raise ValueError("class_logits must be [n, %d] (C_tot of the groups), got %s" % (tables[1], tuple(class_logits.shape)))
    if class_logits.dtype not in (torch.float32, torch.bfloat16) or box_regression.dtype != class_logits.dtype:
        raise TypeError("class_logits and box_regression must both be float32, or both bfloat16")
    if tables is not None:
        if tuple(box_regression.shape) != (n, 7):
            raise ValueError("box_regression must be [%d, 7] (class agnostic with groups), got %s"
                             % (n, tuple(box_regression.shape)))
        if labels.numel() != n or regression_targets.numel() != 7 * n or sep_id.numel() != n:
            raise ValueError("sep_id / labels / regression_targets do not have %d rows" % n)
    else:
        if class_specific is None:
            class_specific = box_regression.shape[1] == 7 * nc and nc != 1
        width = 7 * nc if class_specific else 7
        if box_regression.shape[0] != n or box_regression.shape[1] != width:
            raise ValueError("box_regression must be [%d, %d], got %s" % (n, width, tuple(box_regression.shape)))
        if labels.numel() != n or regression_targets.numel() != 7 * n:
            raise ValueError("labels / regression_targets do not have %d rows" % n)
    _hip.require_gpu(class_logits)
    dev = class_logits.device
    sid = None if tables is None else sep_id.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    lab = labels.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    tgt = regression_targets.reshape(-1, 7).to(device=dev, dtype=torch.float32).contiguous()
    cls_loss, box_loss, flag = _BoxHeadLoss.apply(class_logits, box_regression, sid, lab, tgt, tables, bool(class_specific),
                                                  BOX_LOSS_BETA)
    return (cls_loss, box_loss, flag) if return_flag else (cls_loss, box_loss)


def box_head_loss(class_logits, box_regression, labels, regression_targets, class_specific=None, yaw_loss_mode="Diff",
                  return_flag=False):
    """FastRCNNLossComputation.__call__ (box_head_3d/loss.py:295-382, the non-separated path) on the sampled rows:
    class_logits [n, C], box_regression [n, 7 C] or [n, 7] (fp32 or bf16 alike), labels int64 [n] (0 = background),
    regression_targets fp32 [n, 7]:
      classification_loss = F.cross_entropy(class_logits, labels);
      box_loss = smooth_l1_loss(box_regression[pos, 7 l .. 7 l + 6], regression_targets[pos], beta=1/5, sum) / n
    (`labels.numel()`, not the positive count).  n == 0 gives NaN losses.  `class_specific`: None = told from the
    regression's width.  `yaw_loss_mode`: 'Diff' / 'Diff_<w>'; 'SinDiff' raises (rpn_glue.parse_yaw_loss_mode: the
    reference's box_loss passes a plain tensor where that mode reads `anchor.bbox3d`, so it cannot run there either).
    Returns (classification_loss, box_loss), 0-dim fp32 device tensors with autograd to both inputs; no host read.  A
    label outside [0, C) adds nothing, gets zero gradients and raises the flag: `return_flag=True` appends the 0-dim
    int32 device tensor (1 = some label was out of range) for the caller to read with the losses
    (FastRCNNLossComputation.__call__ keeps it as `last_flag`)."""
    parse_yaw_loss_mode(yaw_loss_mode)
    _hip.require_gpu(class_logits)
    return _box_head_loss(class_logits, box_regression, None, labels, regression_targets, None, class_specific, return_flag)


# ---- the separated-classifier groups (MODEL.SEPARATE_CLASSES; csrc/sep_groups.h) -------------------------------------------
SEP_MAX_GROUPS, SEP_MAX_COLS, SEP_MAX_SEGMENTS = 8, 32, 16


def sep_group_tables(groups):
    """`groups`: a SeperateClassifier (maskrcnn_benchmark/modeling/seperate_classifier.py) or its `grouped_classes`, a
    list over groups of column lists in group-local order, each group's background column first.  Returns
    (grouped_classes as lists of int, C_tot, class_nums int32 host array, cols int32 host array): the two host tables
    every grouped entry point of the library takes.  ValueError outside the library's limits (2 .. 8 groups, C_tot <= 32,
    every column below C_tot and in one group only) -- raised here, before the GPU is needed."""
    gc = getattr(groups, "grouped_classes", groups)
    gc = [[int(c) for c in g] for g in gc]
    if not 2 <= len(gc) <= SEP_MAX_GROUPS:
        raise ValueError("separated classifier: 2 .. %d groups, got %d" % (SEP_MAX_GROUPS, len(gc)))
    flat = [c for g in gc for c in g]
    c_tot = getattr(groups, "seperated_num_classes_total", None)
    c_tot = int(c_tot) if c_tot is not None else (max(flat) + 1 if flat else 0)
    if not 2 <= c_tot <= SEP_MAX_COLS:
        raise ValueError("separated classifier: 2 <= C_tot <= %d, got %d" % (SEP_MAX_COLS, c_tot))
    if any(len(g) < 1 for g in gc) or any(not 0 <= c < c_tot for c in flat) or len(set(flat)) != len(flat):
        raise ValueError("separated classifier: every group needs its background column, every column must lie in "
                         "[0, %d) and in one group only, got %r" % (c_tot, gc))
    return gc, c_tot, _hip.i32xn([len(g) for g in gc]), _hip.i32xn(flat)


def box_head_targets_grouped(proposals, sep_sizes, targets, target_labels, groups, fg_iou=0.5, bg_iou=0.5,
                             aug_thickness=None, batch_size_per_image=500, positive_fraction=0.25, weights=None, seed=None,
                             defer=False, debug=None, box_coder=None):
    """box_head_targets with separated-classifier groups (SeperateClassifier.seperate_subsample,
    seperate_classifier.py:134-161) as ONE pass instead of one per group.  proposals: list over scenes of [n_b, 7], the
    rows of a scene GROUP-MAJOR (all of group 0, then group 1, ...); sep_sizes: per scene the G host-known group sizes
    (their sum is n_b); targets / target_labels: each scene's whole ground truth with its ORIGINAL labels.

    Segment s = scene G + group is treated as box_head_targets treats a scene: its proposals meet only the scene's ground
    truth whose label lies in the group (none: all background, zero targets), the label is the GROUP-LOCAL id, and the
    sampler draws `batch_size_per_image` with the positive share per segment, its hash key over (seed, s, segment-local
    row).  The ground truth is filtered and ordered on the device: one launch writes a key per box
    (aabr_roi_gt_group_keys), ONE stable torch.sort of the keys orders every segment's boxes by (group-local label, row)
    -- the order in which the reference concatenates a group's targets, which decides ties -- and the target kernel finds
    each segment's run by binary search.  No host read of any per-group ground-truth count.  Library launches: 1 + 1 memset
    + 6, whatever the scenes and G; scenes x G <= 16.

    Returns a list over scenes of dicts: rows int64 [m] (scene-local proposal rows), bbox3d [m, 7], labels int64 [m]
    (group-local), regression_targets [m, 7], sep_id int32 [m] -- the groups' samples one after the other, each in
    ascending row.  `defer` / `debug` as box_head_targets; `debug` receives `matched_idx` (rows of the scene's own
    ground-truth list), `matched_val`, `labels`, `regression_targets`, the padded `samp_*` [scenes G, B, ...], `gt_keys`,
    `gt_perm`, `seed` and `info` [scenes G][8] after the read.  The IoU matrices are not stored in this form."""
    gc, _c_tot, class_nums, cols = sep_group_tables(groups)
    G = len(gc)
    nb = len(proposals)
    if not (nb == len(targets) == len(target_labels) == len(sep_sizes)):
        raise ValueError("proposals, sep_sizes, targets and target_labels differ in length")
    if nb == 0:
        return (lambda: []) if defer else []
    S = nb * G
    if S > SEP_MAX_SEGMENTS:
        raise _hip.AabrError("box_head_targets_grouped: scenes x groups <= %d, got %d x %d" % (SEP_MAX_SEGMENTS, nb, G))
    n_s = [int(v) for sz in sep_sizes for v in sz]
    if any(len(sz) != G for sz in sep_sizes) or any(v < 0 for v in n_s):
        raise ValueError("sep_sizes needs %d non-negative sizes per scene" % G)
    n_b = [int(p.shape[0]) for p in proposals]
    if any(sum(n_s[b * G:(b + 1) * G]) != n_b[b] for b in range(nb)):
        raise ValueError("sep_sizes do not add up to the scenes' proposal counts")
    lib = _hip.load()
    dev, n_b, g_b, props, tg, tl, aug, w, corner, seed = _targets_inputs(proposals, targets, target_labels, aug_thickness,
                                                                         weights, box_coder, seed)
    B = int(batch_size_per_image)
    keys = torch.empty(sum(g_b), dtype=torch.int64, device=dev)
    check(lib.aabr_roi_gt_group_keys(ptr(tl), nb, _hip.i64xn(g_b), G, _c_tot, class_nums, cols, ptr(keys), _hip.stream()))
    keys, perm = torch.sort(keys, stable=True)                            # the one sort: (segment, group-local label, row)
    infos = torch.empty((1, S, INFO_WORDS), dtype=torch.int32, device=dev)
    bufs = _targets_run(lib.aabr_roi_targets_grouped,
                        (ptr(props), ptr(tg), ptr(keys), ptr(perm), nb, G, _hip.i64xn(n_s), _hip.i64xn(g_b)), (), sum(n_b), S,
                        B, int(lib.aabr_roi_targets_scratch_words(S)), dev, aug, fg_iou, bg_iou, w, corner, seed,
                        positive_fraction, infos[0])
    s_rows, s_labels, s_targets, s_boxes = (bufs[k] for k in ("samp_rows", "samp_labels", "samp_targets", "samp_boxes"))
    if debug is not None:
        debug.update(bufs, seed=seed, gt_keys=keys, gt_perm=perm)

    def scenes(read):
        out = []
        for b in range(nb):
            ms = [read[0][b * G + g][0] for g in range(G)]
            first = [sum(n_s[b * G:b * G + g]) for g in range(G)]         # the segment's first row inside its scene
            seg = range(b * G, (b + 1) * G)
            out.append({"rows": torch.cat([s_rows[s, :m] + o for s, m, o in zip(seg, ms, first)]),
                        "bbox3d": torch.cat([s_boxes[s, :m] for s, m in zip(seg, ms)]),
                        "labels": torch.cat([s_labels[s, :m] for s, m in zip(seg, ms)]),
                        "regression_targets": torch.cat([s_targets[s, :m] for s, m in zip(seg, ms)]),
                        "sep_id": torch.cat([torch.full((m,), g, dtype=torch.int32, device=dev)
                                             for g, m in enumerate(ms)]),
                        "sep_counts": ms})
        return out

    return _targets_finish(infos, debug, defer, scenes)


def box_head_loss_grouped(class_logits, box_regression, sep_id, labels, regression_targets, groups, yaw_loss_mode="Diff",
                          return_flag=False):
    """box_head_loss with separated-classifier groups (SeperateClassifier.roi_cross_entropy_seperated and
    roi_box_loss_seperated, seperate_classifier.py:163-204) as one call: class_logits [n, C_tot], box_regression [n, 7]
    (class agnostic; fp32 or bf16 alike), sep_id [n] (each row's group), labels int64 [n] (GROUP-LOCAL, 0 = the group's
    background), regression_targets fp32 [n, 7].  For every group g over its n_g rows:
      cls_loss[g] = F.cross_entropy(class_logits[rows_g][:, grouped_classes[g]], labels[rows_g])
      box_loss[g] = smooth_l1_loss(box_regression[pos_g], regression_targets[pos_g], beta=1/5, sum) / n_g
    n_g is counted on the device; a group without rows gives NaN for that group only.  Returns (cls_loss [G], box_loss [G]),
    fp32 device tensors with autograd to both inputs -- the gradient of a column outside a row's group is an exact 0; no
    host read; 2 launches forward, 1 backward; bit-identical run to run.  A sep_id outside [0, G) or a label outside the
    group's range adds nothing, gets zero gradients and raises the flag (`return_flag=True` appends it)."""
    parse_yaw_loss_mode(yaw_loss_mode)
    gc, c_tot, class_nums, cols = sep_group_tables(groups)
    return _box_head_loss(class_logits, box_regression, sep_id, labels, regression_targets,
                          (len(gc), c_tot, class_nums, cols), False, return_flag)


def box_detections_grouped(class_logits, box_regression, proposals, sep_id, groups, score_thresh=0.05, nms=0.5,
                           nms_aug_thickness=None, detections_per_img=100, weights=None, defer=False, debug=None,
                           bbox_xform_clip=10000.0, box_coder=None):
    """box_detections with separated-classifier groups (SeperateClassifier.post_processor, seperate_classifier.py:342-364)
    as one call: class_logits [N, C_tot], box_regression [N, 7] (class agnostic), proposals: list over scenes of [n_b, 7],
    sep_id [N] (each row's group; the rows of a scene may come in any order -- no per-group sizes are needed).

    Per row the softmax over its group's columns only; per scene and foreground column the rows of that column's group
    above `score_thresh` through the NMS of box_detections; per scene the groups in ascending order, each group's
    columns in group-local order (ascending original label), the `detections_per_img` cut per (scene, group) with ties at
    the cut staying.  `labels` are original labels (the column index; never a background column).  5 launches, one read
    of the counts at the end (`defer` as box_detections).  `debug` receives `prob` [N, C_tot] (exact zeros outside the
    row's group), `boxes` [N, 7] and `info` (word 5 of a scene: some sep_id was outside [0, G))."""
    gc, c_tot, class_nums, cols = sep_group_tables(groups)
    return _detections(class_logits, box_regression, proposals, sep_id, (len(gc), c_tot, class_nums, cols), False,
                       score_thresh, nms, nms_aug_thickness, detections_per_img, weights, bbox_xform_clip, box_coder, defer,
                       debug)


POOL_MAX_LEVELS = 8          # csrc/roi_pool.hip kPoolMaxLevels: the level table travels in the kernel arguments


def _pool_check(features, proposals, output_size, scales):
    """the argument errors of pool_rois, raised before the GPU is needed"""
    if len(features) != len(scales):
        raise ValueError("%d feature levels, %d scales" % (len(features), len(scales)))
    if not 1 <= len(features) <= POOL_MAX_LEVELS:
        raise ValueError("1 .. %d levels, got %d" % (POOL_MAX_LEVELS, len(features)))
    if len(tuple(output_size)) != 3:
        raise ValueError("output_size must be (ph, pw, pz)")
    dtypes = set(x.features.dtype for x in features)
    if len(dtypes) != 1 or not dtypes <= {torch.float32, torch.bfloat16}:
        raise TypeError("pool_rois gathers float32 or bfloat16 features, every level in the same storage; got %s"
                        % sorted(str(d) for d in dtypes))
    for x in features:
        if x.features.dim() != 2:
            raise ValueError("features must be [V, C]")
    chans = set(int(x.features.shape[1]) for x in features)
    if len(chans) != 1:
        raise ValueError("the levels differ in channel count: %s" % sorted(chans))
    for p in proposals:
        if p.dim() != 2 or p.shape[1] != 7:
            raise ValueError("proposals must be [n, 7] yx_zb boxes, got %s" % (tuple(p.shape),))


def roi_rows_and_levels(proposals, scales, canonical_size, box_scale=1.0):
    """list over scenes of [n_b, 7] yx_zb device tensors -> (rois [N, 8] fp32, levels [N] int32), one launch
    (k_roi_pool_prepare): convert_metric_to_pixel + Pooler.convert_to_roi_format + LevelMapper_3d of the reference"""
    lib = _hip.load()
    if len(proposals) == 0:
        raise ValueError("no scenes")
    _hip.require_gpu(proposals[0])
    dev = proposals[0].device
    n_b = [int(p.shape[0]) for p in proposals]
    boxes = (torch.cat([p.reshape(-1, 7) for p in proposals]) if len(proposals) > 1 else proposals[0].reshape(-1, 7))
    boxes = boxes.detach().to(device=dev, dtype=torch.float32).contiguous()
    N = sum(n_b)
    rois = torch.empty((N, 8), dtype=torch.float32, device=dev)
    levels = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib.aabr_roi_pool_prepare(ptr(boxes), len(n_b), _hip.i64xn(n_b), float(box_scale), len(scales),
                                    _hip.f32xn(scales), float(canonical_size), ptr(rois), ptr(levels), _hip.stream()))
    return rois, levels


def _level_table(descs):
    tab = (_hip.AabrRoiLevel * len(descs))()
    for t, (feats, cm, ext, V, off, scale) in zip(tab, descs):
        t.feats, t.cellmap = ptr(feats) if V else None, ptr(cm) if V else None
        t.height, t.width, t.zsize, t.nb = ext
        t.V, t.row_offset, t.spatial_scale = V, off, scale
    return tab


class _PoolRois(torch.autograd.Function):
    """every level's gather in one launch; backward: one gradient allocation for all levels, one memset, one launch.
    bf16 levels are gathered in place; their gradients are summed in an fp32 buffer and rounded once into one bf16
    allocation (one more launch), sliced per level the same way.  A bf16 pooled tensor (cfg's fourth entry) is written by
    the same launch, rounded once on its store; its bf16 gradient is widened by the backward's staging loads"""

    @staticmethod
    def forward(ctx, rois, levels, geom, cfg, *feats):
        lib = _hip.load()
        output_size, sampling, nb, pooled_dtype = cfg
        feats = [f.contiguous() for f in feats]
        C_ = int(feats[0].shape[1])
        descs, off = [], 0
        for f, (cm, ext, scale) in zip(feats, geom):
            V = int(f.shape[0])
            descs.append((f, cm, ext, V, off, scale))
            off += V
        N = int(rois.shape[0])
        out = torch.empty((N, C_) + tuple(output_size), dtype=pooled_dtype, device=rois.device)    # every element is written
        bf16 = feats[0].dtype == torch.bfloat16
        out16 = pooled_dtype == torch.bfloat16
        args = (_level_table(descs), len(descs), C_, nb, ptr(rois), ptr(levels), N, output_size[0], output_size[1],
                output_size[2], sampling)
        if out16:
            check(lib.aabr_roi_pool_forward_pooled_bf16(*args, int(bf16), ptr(out), _hip.stream()))
        else:
            forward = lib.aabr_roi_pool_forward_bf16 if bf16 else lib.aabr_roi_pool_forward
            check(forward(*args, ptr(out), _hip.stream()))
        ctx.descs, ctx.total = [(None,) + d[1:] for d in descs], off
        ctx.cfg = (tuple(output_size), sampling, nb, C_, bf16, out16)
        ctx.save_for_backward(rois, levels, *feats)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        lib = _hip.load()
        rois, levels = ctx.saved_tensors[:2]
        descs = [(f,) + d[1:] for f, d in zip(ctx.saved_tensors[2:], ctx.descs)]
        output_size, sampling, nb, C_, bf16, out16 = ctx.cfg
        g = grad_output.contiguous()
        if g.dtype != (torch.bfloat16 if out16 else torch.float32):
            raise TypeError("pool_rois backward: the gradient must have the pooled tensor's dtype, got %s" % g.dtype)
        d_all = torch.empty((ctx.total, C_), dtype=torch.float32, device=g.device)                 # zeroed by the library
        head = (_level_table(descs), len(descs), C_, nb, ptr(rois), ptr(levels), int(rois.shape[0]), output_size[0],
                output_size[1], output_size[2], sampling)
        args = head + (ptr(g), ptr(d_all))
        if out16:                                       # the bf16 gradient is widened on load; sums as below
            d_f32 = d_all
            if bf16:
                d_all = torch.empty((ctx.total, C_), dtype=torch.bfloat16, device=g.device)
            check(lib.aabr_roi_pool_backward_pooled_bf16(*head, int(bf16), ptr(g), ptr(d_f32), ptr(d_all) if bf16 else None,
                                                         ctx.total, _hip.stream()))
        elif bf16:                                      # d_all: the fp32 sums; one rounding into the bf16 rows
            d_f32, d_all = d_all, torch.empty((ctx.total, C_), dtype=torch.bfloat16, device=g.device)
            check(lib.aabr_roi_pool_backward_bf16(*args, ptr(d_all), ctx.total, _hip.stream()))
        else:
            check(lib.aabr_roi_pool_backward(*args, ctx.total, _hip.stream()))
        grads = tuple(d_all[off:off + V] for (_f, _cm, _ext, V, off, _s) in ctx.descs)
        return (None, None, None, None) + grads


POOLED_DTYPES = (torch.float32, torch.bfloat16)      # storage of the pooled tensor and of its gradient


def pool_rois(features, proposals, output_size, scales, sampling_ratio, canonical_size, box_scale=1.0, debug=None,
              pooled_dtype=torch.float32):
    """features: list over levels of SparseConvNetTensor ([V_l, C] features, all fp32 or all bf16 storage -- bf16 rows are
    gathered in place, the result stays fp32, each level's gradient is bf16: fp32 sums rounded once); proposals: list over scenes of [n_b, 7]
    yx_zb device tensors; scales: each level's spatial scale relative to the box frame after `box_scale` (the
    reference's POOLER_SCALES; `box_scale` its SPARSE3D.VOXEL_SCALE, convert_metric_to_pixel).

    What Pooler.forward computes (modeling/poolers_3d.py:126-168): ROI rows from the boxes, a level per box
    (LevelMapper_3d: the scale closest to sqrt(max(size_x, size_y)) / canonical_size), and each box's rotated 3-D ROI-align
    from its level's map, gathered straight from the sparse feature rows (ROIAlignRotated3D's fused form, bit-identical).
    Returns [N, C, ph, pw, pz] fp32 with autograd to every level's features; a level no ROI maps to, and a level without
    sites, get an all-zero gradient of their own shape.  Two launches forward, a memset and one launch backward, whatever
    the level count; no host read once each grid's occupied extent and cell map are cached on its metadata (the first
    call per grid reads 16 bytes, as ROIAlignRotated3D does).  At most 8 levels and 16 scenes.  `debug` (a dict) receives
    `rois` [N, 8] and `levels` [N] int32.

    `pooled_dtype=torch.bfloat16` (fp32 or bf16 levels alike; any dtype but these two raises TypeError): the result is
    stored in bf16, each element the fp32 value rounded once (nearest even) by the same launch, and the backward takes a
    bf16 gradient, widened on load -- the sums, the atomics and the levels' gradients are as above."""
    from maskrcnn_benchmark.layers.roi_align_rotated_3d import _cellmap, _occupied_extent
    if pooled_dtype not in POOLED_DTYPES:
        raise TypeError("pool_rois: pooled_dtype must be torch.float32 or torch.bfloat16, got %r" % (pooled_dtype,))
    _pool_check(features, proposals, output_size, scales)
    if len(proposals) == 0:
        raise ValueError("no scenes")
    _hip.require_gpu(proposals[0])
    rois, levels = roi_rows_and_levels(proposals, scales, canonical_size, box_scale)
    if debug is not None:
        debug["rois"], debug["levels"] = rois, levels
    geom = []
    for x, scale in zip(features, scales):
        _hip.require_gpu(x.features)
        if int(x.features.shape[0]) == 0:
            geom.append((None, (0, 0, 0, 0), float(scale)))
            continue
        ext = _occupied_extent(x)                                       # (x, y, z, batch), cached per grid
        geom.append((_cellmap(x, ext), tuple(int(v) for v in ext), float(scale)))
    nb = max([len(proposals)] + [g[1][3] for g in geom])             # scenes: the proposals' or the maps', whichever is more
    cfg = (tuple(int(v) for v in output_size), int(sampling_ratio), nb, pooled_dtype)
    return _PoolRois.apply(rois, levels, geom, cfg, *[x.features for x in features])


class _Mlp(torch.autograd.Function):
    """one dense layer act(A W^T + bias) over csrc/roi_mlp.hip.  `pooled` = (hw, pz): A is the pooler's [n, C, ..., pz]
    tensor read in place (rows n hw + s, columns c pz + z).  `perm_hw` > 0: `weight` is fc6's [N, R hw] in the reference's
    column order r hw + s while A's columns are s R + r -- the weight is packed once (one launch), both GEMMs that read it
    run on the packed copy, and the weight gradient is stored through the inverse permutation.  A bf16 `a` (pooled
    only) is read in place by the _pooled_bf16 entry points and its gradient is written in bf16; all else stays fp32."""

    @staticmethod
    def forward(ctx, a, weight, bias, relu, pooled, perm_hw):
        lib = _hip.load()
        dev = a.device
        a16 = a.dtype == torch.bfloat16
        if a16 and pooled is None:
            raise TypeError("a bfloat16 operand is taken in the pooled layout only")
        a, weight = a.contiguous(), weight.contiguous()
        bias = bias.contiguous() if bias is not None else None
        N, K = int(weight.shape[0]), int(weight.shape[1])
        if pooled is None:
            layout, hw, pz, M = _hip.MLP_ROWS, 0, 0, int(a.shape[0])
        else:
            layout, (hw, pz) = _hip.MLP_POOLED, pooled
            M = int(a.shape[0]) * hw
        w_used = weight
        if perm_hw:
            w_used = torch.empty_like(weight)
            check(lib.aabr_roi_mlp_pack_fc6(ptr(weight), N, K // perm_hw, perm_hw, ptr(w_used), _hip.stream()))
        y = torch.empty((M, N), dtype=torch.float32, device=dev)                      # every element is written
        if a16:
            check(lib.aabr_roi_mlp_forward_pooled_bf16(ptr(a), hw, pz, ptr(w_used), ptr(bias), int(relu), M, N, K, ptr(y),
                                                       _hip.stream()))
        else:
            check(lib.aabr_roi_mlp_forward(ptr(a), layout, hw, pz, ptr(w_used), ptr(bias), int(relu), M, N, K, ptr(y),
                                           _hip.stream()))
        ctx.save_for_backward(a, w_used, y if relu else None)
        ctx.cfg = (layout, hw, pz, M, N, K, int(perm_hw), bias is not None, a16)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        lib = _hip.load()
        a, w_used, y = ctx.saved_tensors
        layout, hw, pz, M, N, K, perm_hw, has_bias, a16 = ctx.cfg
        dy = dy.contiguous()
        dev = dy.device
        d_a = d_w = d_b = None
        if ctx.needs_input_grad[0]:
            d_a = torch.empty_like(a)                                                  # every element is written
            if a16:
                check(lib.aabr_roi_mlp_backward_input_pooled_bf16(ptr(dy), ptr(y), ptr(w_used), M, N, K, hw, pz, ptr(d_a),
                                                                  _hip.stream()))
            else:
                check(lib.aabr_roi_mlp_backward_input(ptr(dy), ptr(y), ptr(w_used), M, N, K, layout, hw, pz, ptr(d_a),
                                                      _hip.stream()))
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            d_w = torch.empty((N, K), dtype=torch.float32, device=dev)
            d_b = torch.empty(N, dtype=torch.float32, device=dev) if has_bias else None
            floats = int(lib.aabr_roi_mlp_dw_scratch_floats(M, N, K))
            scr = _hip.workspace("roi_mlp_dw", floats, torch.float32, dev) if floats else None
            if a16:
                check(lib.aabr_roi_mlp_backward_weight_pooled_bf16(ptr(dy), ptr(y), ptr(a), hw, pz, M, N, K, perm_hw,
                                                                   ptr(d_w), ptr(d_b), ptr(scr), _hip.stream()))
            else:
                check(lib.aabr_roi_mlp_backward_weight(ptr(dy), ptr(y), ptr(a), layout, hw, pz, M, N, K, perm_hw, ptr(d_w),
                                                       ptr(d_b), ptr(scr), _hip.stream()))
        return d_a, d_w, d_b, None, None, None


def _mlp_f32(name, **tensors):
    for k, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s (bf16 is not part of this path)" % (name, k, t.dtype))


def _pooled_f32_or_bf16(name, pooled):
    """the one tensor of the head that may be bf16: the device pooler's result (pool_rois(pooled_dtype=torch.bfloat16)).
    A bf16 tensor that is not on the device is no such result and is refused as a dtype error, before the GPU is needed.
    This is a device condition reported as a TypeError on purpose: without it a host bf16 tensor would get as far as
    require_gpu and fail there with a RuntimeError, as a host fp32 tensor does, and the package's rule that bf16 outside
    the device path is a dtype error raised before the GPU is needed (tests/test_roi_mlp_host.py) would no longer hold"""
    if pooled.dtype not in POOLED_DTYPES:
        raise TypeError("%s: pooled must be float32 or bfloat16, got %s" % (name, pooled.dtype))
    if pooled.dtype == torch.bfloat16 and not pooled.is_cuda:
        raise TypeError("%s: a bfloat16 pooled tensor is taken from the device pooler only "
                        "(pool_rois(pooled_dtype=torch.bfloat16)); got one on %s" % (name, pooled.device))


def dense_linear(x, weight, bias=None, relu=False):
    """act(x W^T + bias): x [M, K] fp32, weight [N, K] (nn.Linear.weight), bias [N] or None, relu: ReLU fused into the
    write-out (and its mask into both gradients' operand loads).  Autograd to x, weight and bias; the weight and bias
    gradients are deterministic (no atomics).  K % 4 == 0 and K >= 4, any M >= 0 and N >= 1.  One launch forward; backward
    one for the input gradient and one (two when the reduction over M is split: aabr_roi_mlp_dw_splits) for the weight
    and bias gradients."""
    _mlp_f32("dense_linear", x=x, weight=weight, bias=bias)
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError("dense_linear: x [M, K] and weight [N, K], got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError("dense_linear: bias must be [%d]" % weight.shape[0])
    _hip.require_gpu(x)
    return _Mlp.apply(x, weight, bias, bool(relu), None, 0)


def box_head_mlp(pooled, conv_w, conv_b, bn_w, bn_b, bn_state, fc6_w, fc6_b, fc7_w, fc7_b):
    """FPN2MLPFeatureExtractor.forward_centroid_box after its pooler (roi_box_feature_extractors.py:152-157):
      pooled [N, C, ph, pw, pz] -> Conv3d([1, 1, pz]) -> BatchNorm3d -> ReLU -> view(N, -1) -> fc6, ReLU -> fc7, ReLU
    and returns x4 [N, R].  Parameters in the reference's layouts: conv_w [R, C, 1, 1, pz], fc6_w [R, R ph pw] (columns in
    the (r, h, w) order of the view), fc7_w [R, R].  The convolution reads the pooled tensor in place and keeps its result
    as rows [N ph pw, R]; BatchNorm + ReLU is the library's aabr_bn_forward / _backward over those rows (leakiness 0, the
    statistics in fp64); fc6 reads them as [N, ph pw R] against its weight packed to that column order.

    bn_state: dict with `eps`, `momentum` (torch's: the share of the NEW statistic; the library multiplies the running
    value, so it receives 1 - momentum), `training`, `track_running_stats`, and `running_mean` / `running_var` (updated
    in place in training; None without tracking).  Without tracking the batch statistics serve in both modes.
    6 launches forward (GEMM, BatchNorm 2, pack, GEMM, GEMM; box_predictions adds a seventh and two torch.cat copies),
    whatever N.  `pooled` may be bf16 (pool_rois(pooled_dtype=torch.bfloat16)): the convolution's GEMMs read it and write
    its gradient in place in bf16; every other tensor, the parameters and the result stay fp32."""
    _mlp_f32("box_head_mlp", conv_w=conv_w, conv_b=conv_b, bn_w=bn_w, bn_b=bn_b, fc6_w=fc6_w, fc6_b=fc6_b,
             fc7_w=fc7_w, fc7_b=fc7_b)
    _pooled_f32_or_bf16("box_head_mlp", pooled)
    n, ph, pw, R = _conv_shape(pooled, conv_w)
    hw = ph * pw
    if tuple(fc6_w.shape) != (int(fc6_w.shape[0]), R * hw):
        raise ValueError("fc6_w must be [*, %d], got %s" % (R * hw, tuple(fc6_w.shape)))
    x2 = _conv_bn_rows(pooled, conv_w, conv_b, bn_w, bn_b, bn_state)
    x3 = _Mlp.apply(x2.view(n, hw * R), fc6_w, fc6_b, True, None, hw)
    return _Mlp.apply(x3, fc7_w, fc7_b, True, None, 0)


def _conv_shape(pooled, conv_w):
    """(N, ph, pw, R) of a pooled tensor and the head's convolution weight, after checking them"""
    if pooled.dim() != 5:
        raise ValueError("pooled must be [N, C, ph, pw, pz], got %s" % (tuple(pooled.shape),))
    _hip.require_gpu(pooled)
    n, c, ph, pw, pz = (int(v) for v in pooled.shape)
    R = int(conv_w.shape[0])
    if tuple(conv_w.shape) != (R, c, 1, 1, pz):
        raise ValueError("conv_w must be [R, %d, 1, 1, %d], got %s" % (c, pz, tuple(conv_w.shape)))
    return n, ph, pw, R


def _conv_bn_rows(pooled, conv_w, conv_b, bn_w, bn_b, bn_state):
    """Conv3d([1, 1, pz]) + BatchNorm3d + ReLU of the head on the pooled tensor, kept as rows [N ph pw, R] (3 launches)"""
    from sparseconvnet.batchNormalization import BatchNormFunction
    n, c, ph, pw, pz = (int(v) for v in pooled.shape)
    R, hw = int(conv_w.shape[0]), ph * pw
    if bn_state.get("momentum") is None:
        raise ValueError("BatchNorm momentum None (cumulative average) is not part of this path")
    x1 = _Mlp.apply(pooled, conv_w.reshape(R, c * pz), conv_b, False, (hw, pz), 0)            # [N hw, R]
    track = bool(bn_state["track_running_stats"])
    train = bool(bn_state["training"]) or not track
    if track:
        rm, rv = bn_state["running_mean"], bn_state["running_var"]
    else:                                                  # the kernel's running-statistics update lands in scratch
        rm = _hip.workspace("roi_mlp_bn", 2 * R, torch.float32, pooled.device)
        rm, rv = rm[:R], rm[R:2 * R]
    empty = x1.new_empty(0)
    return BatchNormFunction.apply(x1, empty if bn_w is None else bn_w, empty if bn_b is None else bn_b, rm, rv,
                                   (float(bn_state["eps"]), 1.0 - float(bn_state["momentum"]), train, 0))


CORNER_PW = 11                                   # roi_box_feature_extractors.py:93-94: roi_all_cor_body = [11, 3, 7]
CORNER_WINDOWS = ((0, 8), 3)                     # cor0 = w 0..2 and cor1 = w 8..10: the two row blocks of one GEMM
BODY_WINDOW = ((2,), 7)                          # body = w 2..8
CORNER_OVERLAP = (2, 8)                          # the w positions both a corner and the body window hold


def _window(n, ph, pw, R, w0, wlen):
    win = _hip.AabrMlpWindow()
    win.n_rois, win.ph, win.pw, win.R, win.wlen, win.blocks = n, ph, pw, R, wlen, len(w0)
    win.w0[0], win.w0[1] = w0[0], w0[-1]
    return win


class _CornerFc6(torch.autograd.Function):
    """fc6_cor over both corner windows (one GEMM, M = 2 n) and fc6_body over the body window of the convolution rows
    x2 [n ph pw, R], each with ReLU: the windows are read in place (csrc/roi_mlp.hip, the window layout), the weights
    packed once per call to the rows' column order, their gradients stored through the inverse permutation.
    Backward: the input gradient is written by the body GEMM (w 2..8, stores) and then, on the same stream, by the
    corner GEMM (w 0, 1, 9, 10 stores; w 2 and 8 added to the body's value): every element written, no zero fill, no
    atomics."""

    @staticmethod
    def forward(ctx, x2, cor_w, cor_b, body_w, body_b, geom):
        lib = _hip.load()
        n, ph, pw, R = geom
        x2 = x2.contiguous()
        dev = x2.device
        parts = []
        for (w0, wlen), w, b in ((CORNER_WINDOWS, cor_w, cor_b), (BODY_WINDOW, body_w, body_b)):
            w = w.contiguous()
            N = int(w.shape[0])
            wp = torch.empty_like(w)
            check(lib.aabr_roi_mlp_pack_fc6(ptr(w), N, R, ph * wlen, ptr(wp), _hip.stream()))
            y = torch.empty((len(w0) * n, N), dtype=torch.float32, device=dev)       # every element is written
            win = _window(n, ph, pw, R, w0, wlen)
            check(lib.aabr_roi_mlp_forward_window(ptr(x2), win, ptr(wp), ptr(b.contiguous() if b is not None else None),
                                                  1, N, ptr(y), _hip.stream()))
            parts.append((wp, y))
        ctx.save_for_backward(x2, parts[0][0], parts[0][1], parts[1][0], parts[1][1])
        ctx.cfg = (geom, cor_b is not None, body_b is not None)
        return parts[0][1], parts[1][1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy_cor, dy_body):
        lib = _hip.load()
        x2, wp_cor, y_cor, wp_body, y_body = ctx.saved_tensors
        (n, ph, pw, R), has_cb, has_bb = ctx.cfg
        dev = x2.device
        st = _hip.stream()
        body = (BODY_WINDOW, wp_body, y_body, dy_body.contiguous(), has_bb, (-1, -1))
        cor = (CORNER_WINDOWS, wp_cor, y_cor, dy_cor.contiguous(), has_cb, CORNER_OVERLAP)
        d_x = None
        if ctx.needs_input_grad[0]:
            d_x = torch.empty_like(x2)                                               # body then corner write all of it
            for (w0, wlen), wp, y, dy, _hb, acc in (body, cor):                     # this order: see the class docstring
                win = _window(n, ph, pw, R, w0, wlen)
                check(lib.aabr_roi_mlp_backward_input_window(ptr(dy), ptr(y), ptr(wp), win, int(wp.shape[0]), acc[0],
                                                             acc[1], ptr(d_x), st))
        grads = {}
        for name, ((w0, wlen), wp, y, dy, has_b, _acc) in (("cor", cor), ("body", body)):
            N, K, M = int(wp.shape[0]), int(wp.shape[1]), len(w0) * n
            d_w = torch.empty((N, K), dtype=torch.float32, device=dev)
            d_b = torch.empty(N, dtype=torch.float32, device=dev) if has_b else None
            floats = int(lib.aabr_roi_mlp_dw_scratch_floats(M, N, K))
            scr = _hip.workspace("roi_mlp_dw", floats, torch.float32, dev) if floats else None
            win = _window(n, ph, pw, R, w0, wlen)
            check(lib.aabr_roi_mlp_backward_weight_window(ptr(dy), ptr(y), ptr(x2), win, N, ph * wlen, ptr(d_w), ptr(d_b),
                                                          ptr(scr), st))
            grads[name] = (d_w, d_b)
        return d_x, grads["cor"][0], grads["cor"][1], grads["body"][0], grads["body"][1], None


def box_head_mlp_corner(pooled, conv_w, conv_b, bn_w, bn_b, bn_state, fc6_cor_w, fc6_cor_b, fc6_body_w, fc6_body_b,
                        fc7_cor_w, fc7_cor_b, fc7_body_w, fc7_body_b):
    """FPN2MLPFeatureExtractor.forward_corner_box after its pooler (roi_box_feature_extractors.py:122-147):
      pooled [N, C, ph, 11, pz] -> Conv3d([1, 1, pz]) -> BatchNorm3d -> ReLU -> the three windows of the 11-wide axis
      (cor0 = w 0..2, body = w 2..8, cor1 = w 8..10) -> fc6_cor / fc7_cor on both corners, fc6_body / fc7_body on the body
    and returns (x_cor [2 N, R'], x_body [N, R']): rows 0 .. N-1 of x_cor are corner 0, rows N .. 2N-1 corner 1.
    Parameters in the reference's layouts: fc6_cor_w [R', R ph 3], fc6_body_w [R', R ph 7] (columns in the (r, h, w) order
    of `.contiguous().view(N, -1)`).  Convolution and BatchNorm as box_head_mlp; the windows are never made contiguous.
    9 launches forward (GEMM, BatchNorm 2, pack 2, fc6 2, fc7 2), whatever N; N = 1 is the unsqueezed case (the
    reference's squeeze() drops the ROI axis there)."""
    _mlp_f32("box_head_mlp_corner", conv_w=conv_w, conv_b=conv_b, bn_w=bn_w, bn_b=bn_b,
             fc6_cor_w=fc6_cor_w, fc6_cor_b=fc6_cor_b, fc6_body_w=fc6_body_w, fc6_body_b=fc6_body_b, fc7_cor_w=fc7_cor_w,
             fc7_cor_b=fc7_cor_b, fc7_body_w=fc7_body_w, fc7_body_b=fc7_body_b)
    _pooled_f32_or_bf16("box_head_mlp_corner", pooled)
    n, ph, pw, R = _conv_shape(pooled, conv_w)
    if pw != CORNER_PW:
        raise ValueError("the corner windows need pw == %d, got pooled %s" % (CORNER_PW, tuple(pooled.shape)))
    for name, w, wlen in (("fc6_cor_w", fc6_cor_w, CORNER_WINDOWS[1]), ("fc6_body_w", fc6_body_w, BODY_WINDOW[1])):
        if w.dim() != 2 or int(w.shape[1]) != R * ph * wlen:
            raise ValueError("%s must be [*, %d], got %s" % (name, R * ph * wlen, tuple(w.shape)))
    x2 = _conv_bn_rows(pooled, conv_w, conv_b, bn_w, bn_b, bn_state)
    y_cor, y_body = _CornerFc6.apply(x2, fc6_cor_w, fc6_cor_b, fc6_body_w, fc6_body_b, (n, ph, pw, R))
    return (_Mlp.apply(y_cor, fc7_cor_w, fc7_cor_b, True, None, 0), _Mlp.apply(y_body, fc7_body_w, fc7_body_b, True, None, 0))


def box_predictions(x, cls_w, cls_b, reg_w, reg_b):
    """FPNPredictor.forward_centroid_box (roi_box_predictors.py:105-109): (cls_score(x), bbox_pred(x)) as ONE GEMM over
    the two weights concatenated along N, returned as two column views of its result.  Device work per call: the one
    GEMM launch, plus torch's own 2 copies (torch.cat of the two weights and of the two biases); backward 2 or 3 library
    launches (input gradient, weight + bias gradient, its second stage when split) plus torch's 5 small kernels for the
    two column views (two zero fills, two copies, one add)."""
    _mlp_f32("box_predictions", x=x, cls_w=cls_w, cls_b=cls_b, reg_w=reg_w, reg_b=reg_b)
    if x.dim() != 2 or cls_w.dim() != 2 or reg_w.dim() != 2 or cls_w.shape[1] != x.shape[1] or reg_w.shape[1] != x.shape[1]:
        raise ValueError("box_predictions: x [n, R], cls_w [C, R], reg_w [7 C or 7, R]")
    if (cls_b is None) != (reg_b is None):
        raise ValueError("box_predictions: both biases or neither")
    _hip.require_gpu(x)
    nc = int(cls_w.shape[0])
    w = torch.cat([cls_w, reg_w])
    b = torch.cat([cls_b, reg_b]) if cls_b is not None else None
    y = _Mlp.apply(x, w, b, False, None, 0)
    return y[:, :nc], y[:, nc:]


def box_predictions_corner(x_cor, x_body, cls_w, cls_b, body_w, body_b, cor_w, cor_b, sem_w, sem_b, class_specific):
    """FPNPredictor.forward_corner_box (roi_box_predictors.py:79-103) as two GEMMs: x_body [n, R] against cls_score_body
    and bbox_pred_body concatenated along N, x_cor [2 n, R] (corner 0 rows, then corner 1 rows) against bbox_pred_cor
    and bbox_corner_semantic concatenated.  Returns (scores [n, C], bbox_regression_corners, corner_semantics [n, 16]):
    the regression is [cor0 xy, cor1 xy, body z0 z1 thickness] per class, [n, 7 C] when class specific, else [n, 7];
    the semantics are corner 0's 8 then corner 1's 8.  score_pred_cor is not computed: the reference drops its result."""
    _mlp_f32("box_predictions_corner", x_cor=x_cor, x_body=x_body, cls_w=cls_w, cls_b=cls_b, body_w=body_w, body_b=body_b,
             cor_w=cor_w, cor_b=cor_b, sem_w=sem_w, sem_b=sem_b)
    if x_cor.dim() != 2 or x_body.dim() != 2 or x_cor.shape[0] != 2 * x_body.shape[0] or x_cor.shape[1] != x_body.shape[1]:
        raise ValueError("box_predictions_corner: x_cor [2 n, R] and x_body [n, R], got %s and %s"
                         % (tuple(x_cor.shape), tuple(x_body.shape)))
    _hip.require_gpu(x_body)
    n, nc = int(x_body.shape[0]), int(cls_w.shape[0])
    k = nc if class_specific else 1
    if tuple(body_w.shape)[0] != 3 * k or tuple(cor_w.shape)[0] != 2 * k:
        raise ValueError("box_predictions_corner: bbox_pred_body [%d, R] and bbox_pred_cor [%d, R]" % (3 * k, 2 * k))
    yb = _Mlp.apply(x_body, torch.cat([cls_w, body_w]), torch.cat([cls_b, body_b]), False, None, 0)
    yc = _Mlp.apply(x_cor, torch.cat([cor_w, sem_w]), torch.cat([cor_b, sem_b]), False, None, 0)
    scores, bbox_body = yb[:, :nc], yb[:, nc:]
    bbox_cor0, bbox_cor1 = yc[:n, :2 * k], yc[n:, :2 * k]
    if class_specific:
        reg = torch.cat([bbox_cor0.reshape(n, nc, 2), bbox_cor1.reshape(n, nc, 2), bbox_body.reshape(n, nc, 3)],
                        2).view(n, -1)
    else:
        reg = torch.cat([bbox_cor0, bbox_cor1, bbox_body], 1)
    return scores, reg, torch.cat([yc[:n, 2 * k:], yc[n:, 2 * k:]], 1)


def box_head_cfg(C=8, resolution=(2, 3, 2), R=12, classes=("background", "wall", "door"), class_specific=True, separate=(),
                 corner=False, track=False, scales=(0.5, 0.25, 0.125), canonical=10.0, sampling=2, voxel_scale=1.0,
                 extractor="FPN2MLPFeatureExtractor", predictor="FPNPredictor", eval_in_train=0, detections=20,
                 loss_weights=(1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0), separate_ids=(), corner_loss=False):
    """a plain attribute tree with the cfg keys the box head's modules read, named as in the reference's
    config/defaults.py -- for smoke(), the timing tool and the tests, which have no yacs config.  `separate` are the
    separated groups' class names (MODEL.SEPARATE_CLASSES: the predictor adds one column per entry), `separate_ids` the
    same groups as lists of class ids (MODEL.SEPARATE_CLASSES_ID: the loss evaluator builds its SeperateClassifier from
    them); `corner_loss` sets MODEL.LOSS.CORNER_CONNECTION, the switch of the corner-connection losses (corner_roi_check)"""
    box_head = _Cfg(POOLER_RESOLUTION=tuple(resolution), POOLER_SCALES_SPATIAL=tuple(scales),
                    POOLER_SAMPLING_RATIO=sampling, CANONICAL_SIZE=canonical, MLP_HEAD_DIM=R, FEATURE_EXTRACTOR=extractor,
                    PREDICTOR=predictor)
    heads = _Cfg(FG_IOU_THRESHOLD=0.5, BG_IOU_THRESHOLD=0.5, BBOX_REG_WEIGHTS=(10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0),
                 BATCH_SIZE_PER_IMAGE=16, POSITIVE_FRACTION=0.25, LABEL_AUG_THICKNESS_Y_TAR_ANC=(0.0, 0.0),
                 LABEL_AUG_THICKNESS_Z_TAR_ANC=(0.0, 0.0), SCORE_THRESH=0.05, NMS=0.5, NMS_AUG_THICKNESS_Y_Z=(0.0, 0.0),
                 DETECTIONS_PER_IMG=detections)
    model = _Cfg(CORNER_ROI=corner, CLASS_SPECIFIC=class_specific, SEPARATE_CLASSES=list(separate),
                 SEPARATE_CLASSES_ID=[list(g) for g in separate_ids],
                 ROI_BOX_HEAD=box_head, ROI_HEADS=heads, LOSS=_Cfg(YAW_MODE="Diff", WEIGHTS=tuple(loss_weights), CORNER_CONNECTION=bool(corner_loss)),
                 RPN=_Cfg(ADD_GT_PROPOSALS=False))
    return _Cfg(MODEL=model, SPARSE3D=_Cfg(VOXEL_SCALE=voxel_scale, nPlaneMap=C), SOLVER=_Cfg(TRACK_RUNNING_STATS=track),
                INPUT=_Cfg(CLASSES=list(classes)), DEBUG=_Cfg(eval_in_train=eval_in_train))
