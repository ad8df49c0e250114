"""Device-resident RPN glue: from a sparse feature map's site list and the RPN
head outputs to NMS-ed proposals without a host round trip.

Restates, for one feature map, `RPNPostProcessor.forward_for_single_feature_map`
(maskrcnn_benchmark/modeling/rpn/inference_3d.py:82-163): per example sigmoid -> top-k ->
anchors of the selected indices (anchor_generator_sparse3d.py:88-104) -> BoxCoder3D.decode ->
boxlist_nms_3d (structures/boxlist_ops_3d.py:14-62).  sigmoid / top-k are torch plumbing; anchor
generation + decode are one fused HIP kernel; NMS is the device mask + scan.  Containers
(BoxList3D) are out of scope: plain tensors in, plain tensors out."""
import torch

import _hip
from sparseconvnet import SCN as _SCN
import _nms
from _hip import ptr, stream, check


def grid_anchors(site_coords, base_anchors, voxel_scale, stride):
    """all anchors of a map, flattened [site, yaw] like AnchorGenerator.grid_anchors: [V*A, 7]"""
    c = site_coords[:, 0:3].float() / voxel_scale * torch.as_tensor(stride, dtype=torch.float32,
                                                                    device=site_coords.device).view(1, 3)
    c = torch.cat([c, torch.zeros(c.shape[0], 4, device=c.device)], 1).view(-1, 1, 7)
    return (c + base_anchors.view(1, -1, 7).to(c.device)).reshape(-1, 7)


_anchor_cache = {}


def _device_anchors(base_anchors, A, dev):
    """the maps' base anchors as one [n_maps * A, 7] device tensor; constants of the config, uploaded once per
    (tensor objects, versions, device) -- a pageable host->device copy blocks the host until the stream gets there"""
    key = (tuple((id(b), b._version) for b in base_anchors), str(dev))
    hit = _anchor_cache.get(key)
    if hit is None or any(a is not b for a, b in zip(hit[0], base_anchors)):
        if len(_anchor_cache) > 64:
            _anchor_cache.clear()
        t = torch.cat([b.reshape(A, 7).to(torch.float32).cpu() for b in base_anchors], 0).to(dev).contiguous()
        hit = _anchor_cache[key] = (list(base_anchors), t)
    return hit[1]


def rpn_proposals_single_map(tensor, objectness, box_regression, base_anchors, voxel_scale, stride,
                             pre_nms_top_n=2000, post_nms_top_n=1000, nms_thresh=0.5,
                             nms_aug_thickness=(0.3, 0.3), weights=(1.0,) * 7, bbox_xform_clip=10000.0):
    """tensor: SparseConvNetTensor of the map (sites batch-contiguous); objectness [V*A] logits and
    box_regression [V*A,7] in the flatten order [site, yaw].  Returns a list over examples of
    (boxes [m,7] yx_zb, objectness [m]) after NMS, all on the device."""
    lib = _hip.load()
    g = tensor.metadata.grids[_SCN._key(tensor.spatial_size)]
    dev = objectness.device
    A = int(base_anchors.shape[0])
    ba = base_anchors.to(device=dev, dtype=torch.float32).contiguous()
    reg = box_regression.contiguous().float()
    batch = g.coords[:, 3]
    nb = int(batch[-1].item()) + 1 if g.V else 0
    counts = torch.bincount(batch.long(), minlength=nb).tolist()   # sites per example (one small read-back)
    out, s = [], 0
    for bi in range(nb):
        e = s + counts[bi]
        n_anchor = (e - s) * A
        if n_anchor == 0:
            out.append((torch.zeros(0, 7, device=dev), torch.zeros(0, device=dev)))
            continue
        obj = objectness[s * A:e * A].sigmoid()
        k = min(pre_nms_top_n, n_anchor)
        score, idx = obj.topk(k, dim=0, sorted=True)
        boxes = torch.empty((k, 7), dtype=torch.float32, device=dev)
        check(lib.aabr_rpn_decode(ptr(g.coords), s, ptr(idx), k, ptr(reg), s * A, ptr(ba), A, float(voxel_scale),
                                  _hip.f32xn(stride), _hip.f32xn(weights), float(bbox_xform_clip), ptr(boxes),
                                  stream()))
        # boxlist_nms_3d: thickness clamps, then rotated NMS on the (already sorted) list
        nb7 = boxes.clone()
        nb7[:, 3:5] = torch.clamp(nb7[:, 3:5], min=nms_aug_thickness[0])
        nb7[:, 5] = torch.clamp(nb7[:, 5], min=nms_aug_thickness[1])
        keep = _nms.rotate_nms_sorted(nb7, nms_thresh, post_nms_top_n, _nms.REFERENCE_DEBUG_ONLY_XY)
        out.append((boxes[keep], score[keep]))
        s = e
    return out


def _site_counts(grids, nb, dev):
    """sites per (map, example), counts[m][b]: the per-sample row offsets every grid got with its site-count read
    (SparseGrid::ctr, Metadata.h:24-33); only a grid built without them costs a read here"""
    counts = [g.sample_counts(nb) for g in grids]
    if any(c is None for c in counts):
        counts = torch.stack([torch.bincount(g.coords[:, 3].long(), minlength=nb)[:nb] if g.V else
                              torch.zeros(nb, dtype=torch.int64, device=dev) for g in grids]).tolist()
    return counts


def _anchor_tables(counts, A, b0=0, b1=None):
    """The two host tables of the examples' anchor lists (csrc/anchor_list.h) for examples b0 .. b1 (default: all), from
    counts[m][b] = sites of example b in map m.  Returns (seg, site, n_anchor): seg flat, n_maps + 1 per example, the
    first list index of every map and the list's length; site flat, n_maps per example, the example's first site row
    in every map (absolute: b0 > 0 starts behind the earlier examples); n_anchor[i] = the length of example b0 + i's
    list.  Plain Python on ints."""
    n_maps = len(counts)
    b1 = len(counts[0]) if b1 is None else b1
    row = [sum(c[:b0]) for c in counts]
    seg, site, n_anchor = [], [], []
    for b in range(b0, b1):
        seg.append(0)
        for m in range(n_maps):
            seg.append(seg[-1] + counts[m][b] * A)
            site.append(row[m])
            row[m] += counts[m][b]
        n_anchor.append(seg[-1])
    return seg, site, n_anchor


fused_topk = True      # aabr_rpn_topk_maps instead of torch.cat + torch.topk per example (False: the round-4 path, for A/B)
topk_stats = {"fallbacks": 0}
_trace = None     # tools/tools_step_timeline.py: called with a label at the stage's host-side boundaries
debug_nms_inputs = None   # tests: a list here receives (nms_boxes [k,7], scores [k]) of every example's NMS call


def rpn_proposals(maps, objectness, box_regression, base_anchors, strides, voxel_scale, pre_nms_top_n=2000,
                  post_nms_top_n=1000, nms_thresh=0.5, nms_aug_thickness=(0.3, 0.3), weights=(1.0,) * 7,
                  bbox_xform_clip=10000.0, batch_size=None, batched=False, defer=False):
    """Cross-scale proposals, the shape the reference runs in (RPNModule.forward, rpn_sparse3d.py:184-209):
    `cat_scales_obj_reg` regroups the scales example-major and RPNPostProcessor then does, per example, ONE
    sigmoid -> top-k(2000) -> decode -> boxlist_nms_3d(1000) over the anchors of all maps
    (rpn/inference_3d.py:95-149).

    maps: list of SparseConvNetTensor (sites batch-contiguous); objectness[m] [V_m*A] logits and
    box_regression[m] [V_m*A,7] in the flatten order [site, yaw]; base_anchors[m] [A,7]; strides[m] (3).
    Device-resident: neither the anchors nor the regrouped tensors are materialised -- the fused kernel maps a
    selected index of the example's concatenated list back to (map, site, yaw).  The top-k runs on the logits
    (sigmoid is monotone; it is applied to the k selected entries inside the kernel).  One small read-back
    (sites per example and map) sizes the slices.  Returns a list over examples of (boxes [m,7], scores [m])."""
    lib = _hip.load()
    n_maps = len(maps)
    assert n_maps == len(objectness) == len(box_regression) == len(base_anchors) == len(strides)
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    dev = objectness[0].device
    A = int(base_anchors[0].shape[0])
    ba = _device_anchors(base_anchors, A, dev)
    obj = [o.reshape(-1).contiguous().float() for o in objectness]
    reg = [r.reshape(-1, 7).contiguous().float() for r in box_regression]
    # `batch_size` (extension): the number of examples when the caller knows it -- saves the read of the last site's
    # batch index.  `batched` (extension): one top-k over a padded [examples, anchors] matrix and one library call for
    # every example's decode + NMS (aabr_rpn_gather_logits / aabr_rpn_proposals_batch) when every example has at
    # least pre_nms_top_n anchors; same selections unless logits tie exactly at the cut
    if batch_size is not None:
        nb = int(batch_size)
    else:
        nb = max((int(g.coords[-1, 3].item()) + 1 if g.V else 0) for g in grids[:1])
    counts = _site_counts(grids, nb, dev)
    segs, sites, n_anchor = _anchor_tables(counts, A, 0, nb)
    if batched and 1 <= nb <= 16 and n_maps <= 8:
        if min(n_anchor) >= pre_nms_top_n:
            k = int(pre_nms_top_n)
            lmax = max(n_anchor)
            seg_h, site_h = _hip.i32xn(segs), _hip.i32xn(sites)
            padded = torch.empty((nb, lmax), dtype=torch.float32, device=dev)
            check(lib.aabr_rpn_gather_logits(n_maps, _hip.ptrs(obj), nb, seg_h, site_h, A, lmax, ptr(padded), stream()))
            _, sel = padded.topk(k, dim=1, sorted=True)
            boxes = torch.empty((nb, k, 7), dtype=torch.float32, device=dev)
            nms_boxes = torch.empty((nb, k, 7), dtype=torch.float32, device=dev)
            scores = torch.empty((nb, k), dtype=torch.float32, device=dev)
            cb = (k + 63) // 64
            mask = torch.empty(nb * k * cb, dtype=torch.int64, device=dev)
            keep = torch.empty((nb, k), dtype=torch.int64, device=dev)
            meta = torch.empty((nb, _hip.META_WORDS), dtype=torch.int32, device=dev)
            check(lib.aabr_rpn_proposals_batch(
                n_maps, _hip.ptrs([g.coords for g in grids]), _hip.ptrs(obj), _hip.ptrs(reg), nb, seg_h, site_h,
                _hip.f32xn([v for st in strides for v in st]), ptr(ba), A, float(voxel_scale), _hip.f32xn(weights),
                float(bbox_xform_clip), float(nms_aug_thickness[0]), float(nms_aug_thickness[1]), ptr(sel), k,
                ptr(boxes), ptr(nms_boxes), ptr(scores), float(nms_thresh), int(_nms.REFERENCE_DEBUG_ONLY_XY),
                int(post_nms_top_n), ptr(mask), ptr(keep), ptr(meta), stream()))
            kept = _hip.read_back(meta[:, 0])       # the one read of the stage
            out = []
            for bi in range(nb):
                kk = keep[bi, :kept[bi]]
                out.append((boxes[bi][kk], scores[bi][kk]))
            return out
    coords_p, obj_p, reg_p = _hip.ptrs([g.coords for g in grids]), _hip.ptrs(obj), _hip.ptrs(reg)
    strides_h = _hip.f32xn([v for st in strides for v in st])
    weights_h = _hip.f32xn(weights)
    # fused cross-scale top-k (csrc/iou_nms.hip aabr_rpn_topk_maps): every example's selection in four launches, nothing
    # concatenated; torch.topk per example (a chain of ~9 rocprim launches each, on a concatenated copy) stays as the
    # fallback for shapes the kernel does not take and for the (reported) case of > 4096 exactly tied logits at the cut
    sel_all = topk_info = None
    if fused_topk and 1 <= nb <= 16 and n_maps <= 8 and pre_nms_top_n <= 2048:
        ks = [min(pre_nms_top_n, n) for n in n_anchor]
        kmax = max(max(ks), 1)
        sel_all = torch.empty((nb, kmax), dtype=torch.int64, device=dev)
        topk_info = torch.empty((nb, 2), dtype=torch.int32, device=dev)
        tscr = _hip.workspace("rpn_topk", int(lib.aabr_rpn_topk_scratch_words(nb)) + 2, torch.int32, dev)
        tso = (-tscr.data_ptr() // 4) % 2
        check(lib.aabr_rpn_topk_maps(n_maps, obj_p, nb, _hip.i32xn(segs), _hip.i32xn(sites), A, _hip.i32xn(ks), ptr(sel_all),
                                     kmax, ptr(topk_info), tscr.data_ptr() + 4 * tso, stream()))

    def rows_of(bi):
        """example bi's rows of the two tables"""
        return segs[bi * (n_maps + 1):(bi + 1) * (n_maps + 1)], sites[bi * n_maps:(bi + 1) * n_maps]

    def logits_of(bi):
        """example bi's logits, concatenated in map order (the torch.topk paths)"""
        seg, st0 = rows_of(bi)
        return torch.cat([obj[m][st0[m] * A:st0[m] * A + (seg[m + 1] - seg[m])] for m in range(n_maps)])

    def decode(bi, sel, boxes, scores):
        """example bi's selected anchors decoded into `boxes` / `scores`; returns the thickness-clamped copy for the NMS"""
        k = boxes.shape[0]
        seg, st0 = rows_of(bi)
        nms_boxes = torch.empty((k, 7), dtype=torch.float32, device=dev)
        check(lib.aabr_rpn_decode_maps(n_maps, coords_p, obj_p, reg_p, _hip.i32xn(seg), _hip.i32xn(st0), strides_h,
                                       ptr(ba), A, float(voxel_scale), weights_h, float(bbox_xform_clip),
                                       float(nms_aug_thickness[0]), float(nms_aug_thickness[1]), ptr(sel), k,
                                       ptr(boxes), ptr(nms_boxes), ptr(scores), stream()))
        return nms_boxes

    out, pending = [], []
    for bi in range(nb):
        if n_anchor[bi] == 0:
            out.append((torch.zeros(0, 7, device=dev), torch.zeros(0, device=dev)))
            continue
        k = min(pre_nms_top_n, n_anchor[bi])
        if sel_all is not None:
            sel = sel_all[bi, :k]
        else:
            _, sel = logits_of(bi).topk(k, dim=0, sorted=True)
        boxes = torch.empty((k, 7), dtype=torch.float32, device=dev)
        scores = torch.empty(k, dtype=torch.float32, device=dev)
        nms_boxes = decode(bi, sel, boxes, scores)
        if debug_nms_inputs is not None:
            debug_nms_inputs.append((nms_boxes, scores))
        # every example's launches go out first; the numbers kept are read once, after the last one
        keep, meta = _nms.rotate_nms_sorted(nms_boxes, nms_thresh, post_nms_top_n, _nms.REFERENCE_DEBUG_ONLY_XY,
                                            lazy=True)
        pending.append((len(out), boxes, scores, keep, meta, bi))
        out.append(None)

    def finish():
        if pending:
            if _trace is not None:
                _trace("proposal launches enqueued")
            words = [p[4][0:1] for p in pending]
            if topk_info is not None:
                words.append(topk_info[:, 1])
            vals = _hip.read_back(torch.cat(words))                             # the one read of the stage
            kept, over = vals[:len(pending)], vals[len(pending):]
            if _trace is not None:
                _trace("proposal counts read")
            for (i, boxes, scores, keep, meta, bi), nk in zip(pending, kept):
                if over and over[bi]:
                    # > 4096 exactly tied logits at the cut: this example again, selected by a full torch.topk
                    topk_stats["fallbacks"] += 1
                    _, sel = logits_of(bi).topk(boxes.shape[0], dim=0, sorted=True)
                    nms_boxes = decode(bi, sel, boxes, scores)
                    kp = _nms.rotate_nms_sorted(nms_boxes, nms_thresh, post_nms_top_n, _nms.REFERENCE_DEBUG_ONLY_XY)
                    out[i] = (boxes[kp], scores[kp])
                    continue
                k = keep[:nk]
                out[i] = (boxes[k], scores[k])
        return out

    # `defer` (extension): every launch of the stage is out; the caller gets the function that does the one read and
    # slices the lists, to be called (on the same stream) when it wants the result -- e.g. after it has enqueued
    # other work that does not depend on the proposals
    return finish if defer else finish()


def rpn_label_matches(maps, base_anchors, strides, voxel_scale, targets, aug_thickness, criterion=6,
                      fg_iou=0.55, bg_iou=0.2, batch_size=None, return_matrix=False, yaw_threshold=0.7,
                      allow_low_quality_matches=True, regression_targets=False, weights=(1.0,) * 7):
    """The label-generation half of the RPN's training step on the device: per example the IoU of its ground-truth
    boxes against the anchors of ALL maps, `boxlist_iou_3d(target, anchor, aug_thickness, criterion,
    flag='rpn_label_generation')` (RPNLossComputation.match_targets_to_anchors, modeling/rpn/loss_3d.py:91-100;
    criterion = cfg.MODEL.IOU_CRITERIA = 6, config/defaults.py:44), followed by `Matcher.__call__` as
    make_rpn_loss_evaluator builds it (loss_3d.py:338-344, modeling/matcher.py:50-196): entries whose |yaw
    difference| is not below `yaw_threshold` (cfg.MODEL.RPN.YAW_THRESHOLD = 0.7, defaults.py:153; > 1.58 = no mask)
    are zeroed, best ground truth per anchor, BELOW_LOW_THRESHOLD (-1) / BETWEEN_THRESHOLDS (-2) by the two IoU
    thresholds (defaults.py:147,151), then -- `allow_low_quality_matches`, True for the RPN -- set_low_quality_matches_
    and its ignore-nearby pass.  The `cendis` argument the reference also passes is dead there (`if cendis is None or
    True`, matcher.py:130).  The sampler and the losses are plain torch in the reference and are not part of this path.
    `matched_vals` / the returned matrix: the masked maximum / the UNMASKED `boxlist_iou_3d` matrix.

    maps / base_anchors / strides as in `rpn_proposals`; targets[b] = [G_b, 7] yx_zb boxes of example b (device).
    ONE library call for the whole batch (`aabr_rpn_label_generation`): anchors are generated inside the kernel from
    the maps' site lists (AnchorGenerator.grid_anchors, anchor_generator_sparse3d.py:88-104, example-major like
    `cat_scales_anchor`), the per-example row ranges come from the grids' per-sample offsets (no host read), the
    [G_b, N_b] matrices are written only with `return_matrix`.
    `regression_targets` True: the same launch also writes what RPNLossComputation.prepare_targets computes next
    (loss_3d.py:186-196) -- `box_coder.encode(target[matched_idxs.clamp(min=0)], anchor)` for every anchor, BoxCoder3D's
    centroid form with `weights` (box_coder_3d.py:46-51; an example without ground truth encodes its anchors against
    themselves, loss_3d.py:91-94) -- and every tuple gets it as a fourth entry, fp32 [N_b, 7].
    Returns a list over examples of (matched_idxs int64 [N_b], matched_vals fp32 [N_b], iou [G_b, N_b] or None
    [, regression targets])."""
    from utils3d import rotate_nms_3d_torch as R
    lib = _hip.load()
    n_maps = len(maps)
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    dev = grids[0].coords.device
    A = int(base_anchors[0].shape[0])
    ba = _device_anchors(base_anchors, A, dev)
    nb = int(batch_size) if batch_size is not None else len(targets)
    assert aug_thickness["anchor_Y"] == 0 and aug_thickness["target_Y"] >= 0.3     # rotate_nms_3d_torch.py:34-36
    counts = _site_counts(grids, nb, dev)
    out = []
    for b0 in range(0, nb, 16):            # the library takes up to 16 examples per call
        b1 = min(nb, b0 + 16)
        seg, site, n_anch = _anchor_tables(counts, A, b0, b1)
        tg = [targets[bi].to(device=dev, dtype=torch.float32).contiguous() for bi in range(b0, b1)]
        total = sum(n_anch)
        midx = torch.empty(total, dtype=torch.int64, device=dev)
        mval = torch.empty(total, dtype=torch.float32, device=dev)
        mat = torch.empty(sum(n * int(t.shape[0]) for n, t in zip(n_anch, tg)), dtype=torch.float32,
                          device=dev) if return_matrix else None
        aug = (aug_thickness["target_Y"], aug_thickness["target_Z"], aug_thickness["anchor_Y"],
               aug_thickness["anchor_Z"])
        n_gt = sum(int(t.shape[0]) for t in tg)
        rowmax = torch.empty(max(n_gt, 1), dtype=torch.int32, device=dev) if allow_low_quality_matches else None
        regt = torch.empty((total, 7), dtype=torch.float32, device=dev) if regression_targets else None
        check(lib.aabr_rpn_label_generation_targets(
            n_maps, _hip.ptrs([g.coords for g in grids]), b1 - b0, _hip.i32xn(seg), _hip.i32xn(site),
            _hip.f32xn([v for st in strides for v in st]), ptr(ba), A, float(voxel_scale), _hip.ptrs(tg),
            _hip.i32xn([int(t.shape[0]) for t in tg]), _hip.f32x4(aug), int(criterion), int(bool(R.DEBUG)),
            float(fg_iou), float(bg_iou), float(yaw_threshold), int(bool(allow_low_quality_matches)), ptr(midx),
            ptr(mval), ptr(mat), ptr(rowmax), _hip.f32xn(weights), ptr(regt), stream()))
        o = mo = 0
        for n, t in zip(n_anch, tg):
            G = int(t.shape[0])
            row = (midx[o:o + n], mval[o:o + n], mat[mo:mo + G * n].view(G, n) if return_matrix else None)
            out.append(row + (regt[o:o + n],) if regression_targets else row)
            o += n
            mo += G * n
    return out


_stride_cache = {}


def _stride_t(stride, dev):
    key = (tuple(float(v) for v in stride), str(dev))
    t = _stride_cache.get(key)
    if t is None:
        t = _stride_cache[key] = torch.tensor(key[0], dtype=torch.float32).to(dev).view(1, 3)
    return t


def cat_scales_obj_reg(objectness, rpn_box_regression, examples_idxscope):
    """`cat_scales_obj_reg` (modeling/rpn/rpn_sparse3d.py:19-77) on plain tensors: the RPN head emits, per
    scale, the objectness / regression rows of all examples back to back; the loss and the post-processor
    want them regrouped example-major ([example][scale][row]).  `objectness[s]` reshapes to [rows_s, sep],
    `rpn_box_regression[s]` to [rows_s, 7*sep]; `examples_idxscope[s][b] = (begin, end)` is the row range
    of example b at scale s (the reference keeps it on its anchor BoxList3D).  Stays on the device; the
    regrouping is two `torch.cat`s of views."""
    scale_num = len(objectness)
    assert scale_num == len(rpn_box_regression) == len(examples_idxscope)
    batch_size = len(examples_idxscope[0])
    obj_new = [[] for _ in range(batch_size)]
    reg_new = [[] for _ in range(batch_size)]
    for s in range(scale_num):
        assert objectness[s].shape[0] == 1 and rpn_box_regression[s].shape[0] == 1
        sep = objectness[s].shape[-1]
        assert rpn_box_regression[s].shape[-1] == 7 * sep
        obj_s = objectness[s].reshape(-1, sep)
        reg_s = rpn_box_regression[s].reshape(-1, 7 * sep)
        for b in range(batch_size):
            begin, end = examples_idxscope[s][b]
            obj_new[b].append(obj_s[begin:end])
            reg_new[b].append(reg_s[begin:end])
    obj = torch.cat([torch.cat(o, 0) for o in obj_new], 0)
    reg = torch.cat([torch.cat(r, 0) for r in reg_new], 0)
    return obj, reg


def parse_yaw_loss_mode(yaw_loss_mode):
    """`'Diff'` / `'Diff_<w>'` (layers/smooth_l1_loss.py:7-14,19-25: the weight of 'Diff' is parsed and never applied, so
    every column is the plain smooth L1 of |pred - target|).  `'SinDiff'` is refused: the reference reads
    `anchor.bbox3d` in it (smooth_l1_loss.py:27) while RPNLossComputation passes a plain tensor as `anchor`
    (loss_3d.py:238-241), so that mode can never run through the RPN loss."""
    mode = str(yaw_loss_mode).split("_")[0]
    if mode == "SinDiff":
        raise ValueError("yaw_loss_mode %r: 'SinDiff' is not supported (the reference's RPN loss cannot run it: it passes a "
                         "tensor where smooth_l1_loss reads anchor.bbox3d)" % (yaw_loss_mode,))
    if mode != "Diff":
        raise ValueError("yaw_loss_mode %r: expected 'Diff' or 'Diff_<weight>'" % (yaw_loss_mode,))
    return mode


def draw_seed():
    """one 31-bit seed from torch's default CPU generator: no device work, reproduced by torch.manual_seed"""
    return int(torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64).item())


_BF16_OR_F32 = (torch.float32, torch.bfloat16)


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, *tensors):
        lib = _hip.load()
        n_maps = cfg["n_maps"]
        obj, reg = tensors[:n_maps], tensors[n_maps:]
        dev = obj[0].device
        bf16 = int(obj[0].dtype == torch.bfloat16)
        nb, B = cfg["nb"], cfg["B"]
        obj_c = [o.reshape(-1).contiguous() for o in obj]
        reg_c = [r.reshape(-1, 7).contiguous() for r in reg]
        sel = torch.empty((nb, B), dtype=torch.int64, device=dev)
        info = torch.empty((nb, 8), dtype=torch.int32, device=dev)
        obj_loss = torch.empty((), dtype=torch.float32, device=dev)
        box_loss = torch.empty((), dtype=torch.float32, device=dev)
        scr = _hip.workspace("rpn_loss", int(lib.aabr_rpn_loss_scratch_words(nb)) + 2, torch.int32, dev)
        so = (-scr.data_ptr() // 4) % 2
        check(lib.aabr_rpn_loss_forward(
            n_maps, _hip.ptrs(cfg["coords"]), _hip.ptrs(obj_c), _hip.ptrs(reg_c), bf16, cfg["A"], nb, cfg["seg"],
            cfg["site"], _hip.ptrs(cfg["labels"]), _hip.ptrs(cfg["targets"]), cfg["seed"], B, cfg["num_pos"], cfg["beta"],
            ptr(sel), ptr(info), ptr(obj_loss), ptr(box_loss), scr.data_ptr() + 4 * so, stream()))
        ctx.cfg = cfg
        ctx.save_for_backward(sel, info, *obj_c, *reg_c)
        ctx.shapes = [t.shape for t in tensors]
        ctx.mark_non_differentiable(sel, info)
        return obj_loss, box_loss, sel, info

    @staticmethod
    def backward(ctx, g_obj, g_box, _g_sel, _g_info):
        lib = _hip.load()
        cfg = ctx.cfg
        n_maps = cfg["n_maps"]
        saved = ctx.saved_tensors
        sel, info, obj_c, reg_c = saved[0], saved[1], saved[2:2 + n_maps], saved[2 + n_maps:]
        dev, dt = obj_c[0].device, obj_c[0].dtype
        g_obj = (g_obj if g_obj is not None else torch.zeros((), device=dev)).float().contiguous()
        g_box = (g_box if g_box is not None else torch.zeros((), device=dev)).float().contiguous()
        sizes = [o.numel() for o in obj_c] + [r.numel() for r in reg_c]
        flat = torch.zeros(sum(sizes), dtype=dt, device=dev)       # one fill for every gradient
        grads = list(torch.split(flat, sizes))
        check(lib.aabr_rpn_loss_backward(
            n_maps, _hip.ptrs(obj_c), _hip.ptrs(reg_c), int(dt == torch.bfloat16), cfg["A"], cfg["nb"], cfg["seg"],
            cfg["site"], _hip.ptrs(cfg["targets"]), cfg["B"], cfg["beta"], ptr(sel), ptr(info), ptr(g_obj), ptr(g_box),
            _hip.ptrs(grads[:n_maps]), _hip.ptrs(grads[n_maps:]), stream()))
        return (None,) + tuple(g.view(s) for g, s in zip(grads, ctx.shapes))


def rpn_loss(maps, objectness, box_regression, labels, base_anchors, batch_size_per_image=256, positive_fraction=0.5,
             yaw_loss_mode="Diff", seed=None, return_samples=False):
    """The RPN loss of the training step, RPNLossComputation.__call__ (modeling/rpn/loss_3d.py:201-251) for one objectness
    group, on the device with no host read: per example BalancedPositiveNegativeSampler(batch_size_per_image,
    positive_fraction) over the labels (matched index >= 0 positive, -1 negative, -2 ignored; loss_3d.py:180-187), then
    `smooth_l1_loss(box_regression[pos], regression_targets[pos], ., beta=1/9, size_average=False) / N_s` and
    `binary_cross_entropy_with_logits(objectness[sampled], labels[sampled])` (mean), N_s = the anchors sampled over the
    batch.  An empty sample gives NaN losses (the reference's mean of nothing) and zero gradients.

    maps / base_anchors as in `rpn_proposals` (base_anchors gives A); objectness[m] [V_m*A] (any shape of that size) and
    box_regression[m] [V_m*A, 7], fp32 or bf16, read where they lie (nothing concatenated, `cat_scales_obj_reg` is not
    called); labels = the list `rpn_label_matches(..., regression_targets=True)` returns.  The random subset is the one
    of the rule in include/aabr_hip.h (aabr_rpn_loss_forward): a hash of (seed, example, map, x, y, z, anchor) -- the same
    anchors whatever the grid's row order; `seed=None` draws one from torch's default CPU generator.
    `yaw_loss_mode`: 'Diff' / 'Diff_<w>' ('SinDiff' raises ValueError, see parse_yaw_loss_mode).
    Returns (objectness_loss, box_loss), 0-dim fp32 device tensors with autograd to objectness / box_regression; with
    `return_samples` also the int64 [nb, batch_size_per_image] selected indices into the concatenated label lists
    (example-major), positives then negatives, -1 padded."""
    parse_yaw_loss_mode(yaw_loss_mode)
    n_maps = len(maps)
    if not (n_maps == len(objectness) == len(box_regression) == len(base_anchors)):
        raise ValueError("maps, objectness, box_regression and base_anchors differ in length")
    nb = len(labels)
    if nb == 0:
        raise ValueError("no examples")
    if any(len(l) < 4 or l[3] is None for l in labels):
        raise ValueError("labels need the regression targets: rpn_label_matches(..., regression_targets=True)")
    dt = objectness[0].dtype
    if dt not in _BF16_OR_F32 or any(t.dtype != dt for t in list(objectness) + list(box_regression)):
        raise TypeError("objectness and box_regression must all be float32, or all bfloat16")
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    dev = objectness[0].device
    A = int(base_anchors[0].shape[0])
    counts = _site_counts(grids, nb, dev)
    for m in range(n_maps):
        V = sum(counts[m])
        if objectness[m].numel() != V * A or box_regression[m].numel() != V * A * 7:
            raise ValueError("map %d: objectness / box_regression do not hold %d sites x %d anchors" % (m, V, A))
    seg, site, n_anchor = _anchor_tables(counts, A, 0, nb)
    for bi in range(nb):
        if labels[bi][0].numel() != n_anchor[bi] or labels[bi][3].shape[0] != n_anchor[bi]:
            raise ValueError("example %d: the labels do not match the maps' anchors" % bi)
    lab = [l[0] if l[0].dtype == torch.int64 else l[0].long() for l in labels]
    tgt = [l[3].float().contiguous() for l in labels]
    cfg = {"n_maps": n_maps, "nb": nb, "A": A, "B": int(batch_size_per_image),
           "num_pos": int(batch_size_per_image * positive_fraction), "beta": 1.0 / 9,
           "seed": int(draw_seed() if seed is None else seed) & 0xffffffff,
           "coords": [g.coords for g in grids], "seg": _hip.i32xn(seg), "site": _hip.i32xn(site),
           "labels": [l.contiguous() for l in lab], "targets": tgt}
    obj_loss, box_loss, sel, _ = _RpnLoss.apply(cfg, *objectness, *box_regression)
    return (obj_loss, box_loss, sel) if return_samples else (obj_loss, box_loss)


# ---------------------------------------------------------------------------------------------------- the RPN head
RPN_HEAD_MAX_MAPS, RPN_HEAD_MAX_ANCHORS = 8, 4
RPN_HEAD_CHANNELS = (32, 64, 96, 128)


class _RpnHead(torch.autograd.Function):
    """SingleConvRPNHead_Sparse3D over every map in one launch (csrc/rpn_head.hip); the hidden activation is written to
    memory only when some input requires a gradient"""

    @staticmethod
    def forward(ctx, A, W1, b1, Wc, bc, Wr, br, *feats):
        lib = _hip.load()
        dev = W1.device
        C, n_maps = int(W1.shape[0]), len(feats)
        params = [p.contiguous() for p in (W1, b1, Wc, bc, Wr, br)]
        feats = [f.contiguous() for f in feats]
        rows = [int(f.shape[0]) for f in feats]
        obj = [torch.empty(v * A, dtype=torch.float32, device=dev) for v in rows]       # every element is written
        reg = [torch.empty((v * A, 7), dtype=torch.float32, device=dev) for v in rows]
        need = any(ctx.needs_input_grad)
        hidden = torch.empty((sum(rows), C), dtype=torch.float32, device=dev) if need else None
        tab = (_hip.AabrRpnMap * n_maps)()
        for m in range(n_maps):
            tab[m].features, tab[m].rows = ptr(feats[m]), rows[m]
            tab[m].objectness, tab[m].box_regression = ptr(obj[m]), ptr(reg[m])
        check(lib.aabr_rpn_head_forward(tab, n_maps, C, A, *[ptr(p) for p in params], ptr(hidden), stream()))
        if need:
            ctx.save_for_backward(hidden, params[0], params[2], params[4], *feats)
        ctx.cfg = (A, C, n_maps, rows)
        return tuple(obj) + tuple(reg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        lib = _hip.load()
        A, C, n_maps, rows = ctx.cfg
        hidden, W1, Wc, Wr = ctx.saved_tensors[:4]
        feats = ctx.saved_tensors[4:]
        dev = W1.device
        g_obj = [g.contiguous() if g is not None else None for g in grads[:n_maps]]
        g_reg = [g.contiguous() if g is not None else None for g in grads[n_maps:]]
        d_all = torch.empty((sum(rows), C), dtype=torch.float32, device=dev)           # every element is written
        d_f = list(torch.split(d_all, rows))
        sizes = (C * C, C, A * C, A, 7 * A * C, 7 * A)
        d_p = list(torch.split(torch.empty(sum(sizes), dtype=torch.float32, device=dev), sizes))
        t_rows = lib.aabr_rpn_head_tile_rows(C)
        tiles = sum(-(-v // t_rows) for v in rows)
        floats = int(lib.aabr_rpn_head_scratch_floats(tiles, C, A))
        scr = _hip.workspace("rpn_head", floats, torch.float32, dev) if floats else None
        tab = (_hip.AabrRpnMap * n_maps)()
        for m in range(n_maps):
            tab[m].features, tab[m].rows, tab[m].d_features = ptr(feats[m]), rows[m], ptr(d_f[m])
            tab[m].objectness, tab[m].box_regression = ptr(g_obj[m]), ptr(g_reg[m])
        check(lib.aabr_rpn_head_backward(tab, n_maps, C, A, ptr(W1), ptr(Wc), ptr(Wr), ptr(hidden),
                                         *[ptr(p) for p in d_p], ptr(scr), stream()))
        return (None, d_p[0].view(C, C), d_p[1], d_p[2].view(A, C), d_p[3], d_p[4].view(7 * A, C), d_p[5]) + tuple(d_f)


def _as_out_in(name, w):
    """a Conv2d weight [out, in, 1, 1] or a Linear weight [out, in] -> [out, in]"""
    if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
        return w.reshape(w.shape[0], w.shape[1])
    if w.dim() != 2:
        raise ValueError("rpn_head: %s must be [out, in] or [out, in, 1, 1], got %s" % (name, tuple(w.shape)))
    return w


def rpn_head(features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b):
    """SingleConvRPNHead_Sparse3D.forward (modeling/rpn/rpn_sparse3d.py:109-131) for all maps at once:
      t = relu(f conv_w^T + conv_b), objectness = t cls_w^T + cls_b, box_regression = t reg_w^T + reg_b
    features: a list (1..8 maps) of SparseConvNetTensors or of [V_m, C] fp32 tensors; the weights as [out, in] or the
    reference's Conv2d [out, in, 1, 1]: conv_w [C, C], cls_w [A, C], reg_w [7 A, C] (channel a 7 + j, 'box_toghter').
    C in {32, 64, 96, 128}, 1 <= A <= 4.  Returns (objectness, box_regression): lists over the maps of [V_m A] and
    [V_m A, 7] in the [site, yaw] flatten order rpn_proposals, rpn_label_matches and rpn_loss read.
    Device work: forward 1 library launch whatever the number of maps (nothing concatenated, the hidden activation
    reaches memory only when a gradient is required); backward 2 (the fused main kernel and the in-order reduction of its
    per-workgroup partials: deterministic, no atomics).  No host read."""
    feats = [f.features if hasattr(f, "features") else f for f in features]
    if not 1 <= len(feats) <= RPN_HEAD_MAX_MAPS:
        raise ValueError("rpn_head: 1 to %d maps, got %d" % (RPN_HEAD_MAX_MAPS, len(feats)))
    w1, wc, wr = _as_out_in("conv_w", conv_w), _as_out_in("cls_w", cls_w), _as_out_in("reg_w", reg_w)
    for k, t in [("conv_w", w1), ("conv_b", conv_b), ("cls_w", wc), ("cls_b", cls_b), ("reg_w", wr), ("reg_b", reg_b)] + \
            [("features[%d]" % i, f) for i, f in enumerate(feats)]:
        if t.dtype != torch.float32:
            raise TypeError("rpn_head: %s must be float32, got %s (bf16 feature storage is not part of this path)"
                            % (k, t.dtype))
    C, A = int(w1.shape[1]), int(wc.shape[0])
    if C not in RPN_HEAD_CHANNELS:
        raise ValueError("rpn_head: C = %d; supported: a multiple of 32 from 32 to 128" % C)
    if not 1 <= A <= RPN_HEAD_MAX_ANCHORS:
        raise ValueError("rpn_head: A = %d anchors per site; supported: 1 to %d" % (A, RPN_HEAD_MAX_ANCHORS))
    if tuple(w1.shape) != (C, C) or tuple(wc.shape) != (A, C) or tuple(wr.shape) != (7 * A, C):
        raise ValueError("rpn_head: conv_w [C, C], cls_w [A, C], reg_w [7 A, C]; got %s, %s, %s"
                         % (tuple(w1.shape), tuple(wc.shape), tuple(wr.shape)))
    if tuple(conv_b.shape) != (C,) or tuple(cls_b.shape) != (A,) or tuple(reg_b.shape) != (7 * A,):
        raise ValueError("rpn_head: the biases must be [C], [A] and [7 A]")
    for i, f in enumerate(feats):
        if f.dim() != 2 or int(f.shape[1]) != C:
            raise ValueError("rpn_head: features[%d] must be [V, %d], got %s" % (i, C, tuple(f.shape)))
    _hip.require_gpu(feats[0])
    out = _RpnHead.apply(A, w1, conv_b, wc, cls_b, wr, reg_b, *feats)
    return list(out[:len(feats)]), list(out[len(feats):])


class _Cfg(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def clone(self):
        return self


def rpn_cfg(C=32, anchor_sizes=((0.4, 1.5, 1.5), (1.5, 1.5, 1.0)), yaws=(0, -1.57), strides=((8, 8, 8), (16, 16, 16)),
            voxel_scale=20.0, pre_nms_top_n=(200, 200), post_nms_top_n=(50, 50), nms_thresh=0.5, rpn_only=False,
            add_gt_proposals=False, separate=(), separate_rpn=True, batch_size_per_image=256, positive_fraction=0.5,
            classes=("background", "wall", "door")):
    """a plain attribute tree with the cfg keys the RPN modules read, named as in the reference's config/defaults.py
    (pre / post_nms_top_n: (train, test)) -- for smoke(), the timing tool and the tests, which have no yacs config"""
    rpn = _Cfg(ANCHOR_SIZES_3D=[list(s) for s in anchor_sizes], YAWS=tuple(yaws), RATIOS=[[1, 1, 1]] * len(yaws),
               USE_YAWS=[1] * len(anchor_sizes), ANCHOR_STRIDE=[list(s) for s in strides], USE_FPN=True,
               FG_IOU_THRESHOLD=0.55, BG_IOU_THRESHOLD=0.2, YAW_THRESHOLD=0.7, BATCH_SIZE_PER_IMAGE=batch_size_per_image,
               POSITIVE_FRACTION=positive_fraction, NMS_THRESH=nms_thresh, NMS_AUG_THICKNESS_Y_Z=[0.3, 0.3],
               LABEL_AUG_THICKNESS_Y_TAR_ANC=[0.4, 0], LABEL_AUG_THICKNESS_Z_TAR_ANC=[0.8, 0],
               FPN_PRE_NMS_TOP_N_TRAIN=pre_nms_top_n[0], FPN_PRE_NMS_TOP_N_TEST=pre_nms_top_n[1],
               FPN_POST_NMS_TOP_N_TRAIN=post_nms_top_n[0], FPN_POST_NMS_TOP_N_TEST=post_nms_top_n[1],
               RPN_HEAD="SingleConvRPNHead_Sparse3D", ADD_GT_PROPOSALS=add_gt_proposals)
    model = _Cfg(RPN=rpn, RPN__ONLY=rpn_only, SEPARATE_CLASSES=list(separate), SEPARATE_RPN=separate_rpn, IOU_CRITERIA=6,
                 LOSS=_Cfg(YAW_MODE="Diff"))
    return _Cfg(MODEL=model, SPARSE3D=_Cfg(VOXEL_SCALE=voxel_scale, nPlaneMap=C), INPUT=_Cfg(CLASSES=list(classes)))
