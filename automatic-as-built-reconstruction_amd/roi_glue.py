"""Box-head glue on the device: class logits + box regression + proposals -> final detections
(csrc/roi_post.hip, aabr_roi_post_detections).  The counterpart of rpn_glue.rpn_proposals for the second stage:
PostProcessor.forward of the reference (maskrcnn_benchmark/modeling/roi_heads/box_head_3d/inference.py:44-162)
without its Python loops over scenes and classes."""
import ctypes as C

import torch

import _hip
import _nms
from _hip import check, ptr

PRE_NMS, POST_NMS = 2000, 500      # boxlist_nms_3d(flag='roi_post'): rotate_nms_3d(pre_max_size=2000, post_max_size=500)
INFO_WORDS = 8


def box_detections(class_logits, box_regression, proposals, score_thresh=0.05, nms=0.5, nms_aug_thickness=None,
                   detections_per_img=100, weights=None, class_specific=None, defer=False, debug=None,
                   bbox_xform_clip=10000.0):
    """class_logits [N, C] (class 0 = background), box_regression [N, 7 C] or [N, 7], proposals: list over scenes of
    [n_b, 7] yx_zb tensors whose rows, concatenated, are the N rows of the other two.

    Per scene: softmax, BoxCoder3D.decode, per class the rows above `score_thresh`, rotated NMS the way
    boxlist_nms_3d(flag='roi_post') runs it (2000 best, `nms_aug_thickness` clamps on an NMS-only copy, 500
    survivors), the classes concatenated in ascending order and the `detections_per_img` cut of the reference
    (kthvalue: ties at the cut all stay).  Equal scores inside a class are ordered by ascending proposal row.

    `class_specific`: None = told from the regression's width (7 C: one box per class; 7: one box per row).
    Returns a list over scenes of dicts: bbox3d [m, 7], scores [m], labels [m] int64, rows [m] int64 (the scene's
    proposal row each detection came from).  All launches go out without a host read; the one read (the counts) is at
    the end -- `defer=True` returns the function that does it, as rpn_glue.rpn_proposals does.  `debug` (a dict)
    receives `prob` [N, C] and `boxes` [N, C, 7]."""
    lib = _hip.load()
    _hip.require_gpu(class_logits)
    dev = class_logits.device
    logits = class_logits.to(torch.float32).contiguous()
    reg = box_regression.to(device=dev, dtype=torch.float32).contiguous()
    N, nc = int(logits.shape[0]), int(logits.shape[1])
    if class_specific is None:
        class_specific = reg.shape[1] == 7 * nc and nc != 1
    if reg.shape[0] != N or reg.shape[1] != (7 * nc if class_specific else 7):
        raise ValueError("box_regression must be [N, %d], got %s" % (7 * nc if class_specific else 7, tuple(reg.shape)))
    n_b = [int(p.shape[0]) for p in proposals]
    nb = len(n_b)
    if nb == 0 and N == 0:
        return (lambda: []) if defer else []
    if sum(n_b) != N:
        raise ValueError("the proposals have %d rows, class_logits %d" % (sum(n_b), N))
    props = (torch.cat([p.reshape(-1, 7) for p in proposals]) if nb else logits.new_zeros((0, 7)))
    props = props.to(device=dev, dtype=torch.float32).contiguous()
    aug = (0.0, 0.0) if nms_aug_thickness is None else nms_aug_thickness
    w = (1.0,) * 7 if weights is None else [float(v) for v in torch.as_tensor(weights).reshape(-1).tolist()]
    cap = (nc - 1) * POST_NMS
    words = int(lib.aabr_roi_post_scratch_words(nb, max(n_b) if n_b else 0, nc, PRE_NMS))
    if words < 0:
        raise _hip.AabrError("box_detections: unsupported shape (2 <= classes <= 32, 1 <= scenes <= 16): C=%d nb=%d"
                             % (nc, nb))
    scratch = _hip.workspace("roi_post", words + 2, torch.int32, dev)
    off = (-scratch.data_ptr() // 4) % 2                                  # 8-byte alignment of the first word
    prob = boxes = None
    if debug is not None:
        prob = torch.empty((N, nc), dtype=torch.float32, device=dev)
        boxes = torch.empty((N, nc, 7), dtype=torch.float32, device=dev)
    det_rows = torch.empty((nb, cap), dtype=torch.int64, device=dev)
    det_labels = torch.empty((nb, cap), dtype=torch.int64, device=dev)
    det_scores = torch.empty((nb, cap), dtype=torch.float32, device=dev)
    det_boxes = torch.empty((nb, cap, 7), dtype=torch.float32, device=dev)
    info = torch.empty((nb, INFO_WORDS), dtype=torch.int32, device=dev)
    check(lib.aabr_roi_post_detections(
        ptr(logits), ptr(reg), ptr(props), nb, (C.c_int64 * nb)(*n_b), nc, int(bool(class_specific)), _hip.f32xn(w),
        float(bbox_xform_clip), float(score_thresh), float(nms), float(aug[0]), float(aug[1]),
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
