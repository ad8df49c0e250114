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
            if debug_nms_inputs is not None:
                debug_nms_inputs.extend((nms_boxes[bi], scores[bi]) for bi in range(nb))
            kept = _hip.read_back(meta[:, 0])       # the one read of the stage
            out = []
            for bi in range(nb):
                kk = keep[bi, :kept[bi]]
                out.append((boxes[bi][kk], scores[bi][kk]))
            return out
    segments = [(segs[bi * (n_maps + 1):(bi + 1) * (n_maps + 1)], sites[bi * n_maps:(bi + 1) * n_maps],
                 sites[bi * n_maps:(bi + 1) * n_maps], obj, reg) for bi in range(nb)]
    return _proposals_of_segments(lib, dev, [g.coords for g in grids], obj, segments, ba, A, strides, voxel_scale,
                                  pre_nms_top_n, post_nms_top_n, nms_thresh, nms_aug_thickness, weights, bbox_xform_clip,
                                  False, defer)


def _proposals_of_segments(lib, dev, coords, topk_obj, segments, ba, A, strides, voxel_scale, pre_nms_top_n,
                           post_nms_top_n, nms_thresh, nms_aug_thickness, weights, bbox_xform_clip, chunked, defer):
    """top-k -> decode -> NMS of every segment, then the one read.  A segment is an example of rpn_proposals, or a
    (group, scene) pair of rpn_proposals_grouped: (seg, site, topk_site, obj, reg) = its rows of the two anchor tables,
    the site row the fused top-k uses against the allocations `topk_obj` (for a group: offset to the group's slice), and
    the per-map logits / regressions the decode reads with `site`.  `chunked`: more than 16 segments go to the fused top-k
    16 at a time (False: they take the torch.topk path, as rpn_proposals always did)."""
    n_maps, n_seg = len(coords), len(segments)
    n_anchor = [sg[0][n_maps] for sg in segments]
    coords_p = _hip.ptrs(coords)
    strides_h = _hip.f32xn([v for st in strides for v in st])
    weights_h = _hip.f32xn(weights)
    ptr_cache = {}

    def ptrs_of(ts):
        hit = ptr_cache.get(id(ts))
        if hit is None:
            hit = ptr_cache[id(ts)] = (ts, _hip.ptrs(ts))
        return hit[1]
    # fused cross-scale top-k (csrc/iou_nms.hip aabr_rpn_topk_maps): every example's selection in four launches, nothing
    # concatenated; torch.topk per example (a chain of ~9 rocprim launches each, on a concatenated copy) stays as the
    # fallback for shapes the kernel does not take and for the (reported) case of > 4096 exactly tied logits at the cut
    sel_of = over_words = None
    if fused_topk and n_seg >= 1 and (n_seg <= 16 or chunked) and n_maps <= 8 and pre_nms_top_n <= 2048:
        sel_of, over_words = [], []
        topk_p = ptrs_of(topk_obj)
        for e0 in range(0, n_seg, 16):
            chunk = segments[e0:e0 + 16]
            ks = [min(pre_nms_top_n, n) for n in n_anchor[e0:e0 + 16]]
            kmax = max(max(ks), 1)
            sel_all = torch.empty((len(chunk), kmax), dtype=torch.int64, device=dev)
            topk_info = torch.empty((len(chunk), 2), dtype=torch.int32, device=dev)
            tscr = _hip.workspace("rpn_topk", int(lib.aabr_rpn_topk_scratch_words(len(chunk))) + 2, torch.int32, dev)
            tso = (-tscr.data_ptr() // 4) % 2
            check(lib.aabr_rpn_topk_maps(n_maps, topk_p, len(chunk), _hip.i32xn([v for sg in chunk for v in sg[0]]),
                                         _hip.i32xn([v for sg in chunk for v in sg[2]]), A, _hip.i32xn(ks), ptr(sel_all),
                                         kmax, ptr(topk_info), tscr.data_ptr() + 4 * tso, stream()))
            sel_of.extend((sel_all, i) for i in range(len(chunk)))
            over_words.append(topk_info[:, 1])

    def logits_of(bi):
        """segment bi's logits, concatenated in map order (the torch.topk paths).  torch.topk on the device selects a NaN
        whatever its sign bit but sorts one with the sign bit set last among the selected: every NaN goes in as
        float('nan') (sign bit clear), which it puts first -- where the fused top-k puts a NaN (csrc/iou_nms.hip
        topk_order_key; aabr_rpn_gather_logits does the same for the batched form)"""
        seg, st0, _, obj, _reg = segments[bi]
        cat = torch.cat([obj[m][st0[m] * A:st0[m] * A + (seg[m + 1] - seg[m])] for m in range(n_maps)])
        return torch.where(cat != cat, torch.full_like(cat, float("nan")), cat)

    def decode(bi, sel, boxes, scores):
        """segment bi's selected anchors decoded into `boxes` / `scores`; returns the thickness-clamped copy for the NMS"""
        k = boxes.shape[0]
        seg, st0, _, obj, reg = segments[bi]
        nms_boxes = torch.empty((k, 7), dtype=torch.float32, device=dev)
        check(lib.aabr_rpn_decode_maps(n_maps, coords_p, ptrs_of(obj), ptrs_of(reg), _hip.i32xn(seg), _hip.i32xn(st0),
                                       strides_h, ptr(ba), A, float(voxel_scale), weights_h, float(bbox_xform_clip),
                                       float(nms_aug_thickness[0]), float(nms_aug_thickness[1]), ptr(sel), k,
                                       ptr(boxes), ptr(nms_boxes), ptr(scores), stream()))
        return nms_boxes

    out, pending = [], []
    for bi in range(n_seg):
        if n_anchor[bi] == 0:
            out.append((torch.zeros(0, 7, device=dev), torch.zeros(0, device=dev)))
            continue
        k = min(pre_nms_top_n, n_anchor[bi])
        if sel_of is not None:
            sel = sel_of[bi][0][sel_of[bi][1], :k]
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
            if over_words is not None:
                words.extend(over_words)
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


def rpn_proposals_grouped(maps, objectness, box_regression, G, base_anchors, strides, voxel_scale, pre_nms_top_n=2000,
                          post_nms_top_n=1000, nms_thresh=0.5, nms_aug_thickness=(0.3, 0.3), weights=(1.0,) * 7,
                          bbox_xform_clip=10000.0, batch_size=None, defer=False):
    """rpn_proposals for every separated-classifier group (SeperateClassifier.seperate_rpn_selector,
    seperate_classifier.py:68-88) as one stage: objectness[m] [G, V_m A] and box_regression[m] [G, V_m A, 7] are the
    group-major outputs of rpn_head_grouped; per (group, scene) the same top-k of `pre_nms_top_n` over the anchors of
    all maps, decode, rotated NMS and `post_nms_top_n` cut that rpn_proposals does on the group's slices -- the same
    results.  The top-k of all segments is ONE aabr_rpn_topk_maps call per at most 16 segments: it reads logits only,
    so a site table offset by g V_m addresses group g's slice of the allocation; the decode is per segment and takes
    the slice's pointers.  ONE host read for the whole stage (the counts kept, with the top-k's tie flags).
    Returns a list over groups of lists over scenes of (boxes [m, 7], scores [m]); `defer`: the function that does the
    read and returns that."""
    lib = _hip.load()
    n_maps, G = len(maps), int(G)
    assert n_maps == len(objectness) == len(box_regression) == len(base_anchors) == len(strides)
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    dev = objectness[0].device
    A = int(base_anchors[0].shape[0])
    ba = _device_anchors(base_anchors, A, dev)
    obj = [o.reshape(G, -1).contiguous().float() for o in objectness]
    reg = [r.reshape(G, -1, 7).contiguous().float() for r in box_regression]
    if batch_size is not None:
        nb = int(batch_size)
    else:
        nb = max((int(g.coords[-1, 3].item()) + 1 if g.V else 0) for g in grids[:1])
    counts = _site_counts(grids, nb, dev)
    V = [sum(c) for c in counts]
    for m in range(n_maps):
        if obj[m].shape[1] != V[m] * A or reg[m].shape[1] != V[m] * A:
            raise ValueError("map %d: objectness / box_regression do not hold %d groups x %d sites x %d anchors"
                             % (m, G, V[m], A))
    segs, sites, _n = _anchor_tables(counts, A, 0, nb)
    segments = []
    for g in range(G):
        obj_g, reg_g = [o[g] for o in obj], [r[g] for r in reg]
        for bi in range(nb):
            site = sites[bi * n_maps:(bi + 1) * n_maps]
            segments.append((segs[bi * (n_maps + 1):(bi + 1) * (n_maps + 1)], site,
                             [site[m] + g * V[m] for m in range(n_maps)], obj_g, reg_g))
    fin = _proposals_of_segments(lib, dev, [g.coords for g in grids], obj, segments, ba, A, strides, voxel_scale,
                                 pre_nms_top_n, post_nms_top_n, nms_thresh, nms_aug_thickness, weights, bbox_xform_clip,
                                 True, True)

    def finish():
        flat = fin()
        return [flat[g * nb:(g + 1) * nb] for g in range(G)]
    return finish if defer else finish()


def rpn_label_matches(maps, base_anchors, strides, voxel_scale, targets, aug_thickness, criterion=6,
                      fg_iou=0.55, bg_iou=0.2, batch_size=None, return_matrix=False, yaw_threshold=0.7,
                      allow_low_quality_matches=True, regression_targets=False, weights=(1.0,) * 7, groups=1):
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
    [, regression targets]).  `groups`: see rpn_label_matches_grouped."""
    from utils3d import rotate_nms_3d_torch as R
    lib = _hip.load()
    n_maps = len(maps)
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    dev = grids[0].coords.device
    A = int(base_anchors[0].shape[0])
    ba = _device_anchors(base_anchors, A, dev)
    nb = int(batch_size) if batch_size is not None else len(targets) // int(groups)
    assert aug_thickness["anchor_Y"] == 0 and aug_thickness["target_Y"] >= 0.3     # rotate_nms_3d_torch.py:34-36
    counts = _site_counts(grids, nb, dev)
    # the examples of the library call: the scenes, or with `groups` (rpn_label_matches_grouped) the (scene, group)
    # segments, a scene's rows of the two tables repeated for its groups
    seg_all, site_all, n_all = _anchor_tables(counts, A, 0, nb)
    ne = nb * int(groups)
    scene = [e // int(groups) for e in range(ne)] if ne != nb else None
    out = []
    for b0 in range(0, ne, 16):            # the library takes up to 16 examples per call
        b1 = min(ne, b0 + 16)
        if ne == nb:
            seg, site, n_anch = seg_all[b0 * (n_maps + 1):b1 * (n_maps + 1)], site_all[b0 * n_maps:b1 * n_maps], n_all[b0:b1]
        else:
            seg = [v for e in range(b0, b1) for v in seg_all[scene[e] * (n_maps + 1):(scene[e] + 1) * (n_maps + 1)]]
            site = [v for e in range(b0, b1) for v in site_all[scene[e] * n_maps:(scene[e] + 1) * n_maps]]
            n_anch = [n_all[scene[e]] for e in range(b0, b1)]
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


def rpn_label_matches_grouped(maps, base_anchors, strides, voxel_scale, targets, G, aug_thickness, criterion=6,
                              fg_iou=0.55, bg_iou=0.2, batch_size=None, yaw_threshold=0.7, allow_low_quality_matches=True,
                              regression_targets=True, weights=(1.0,) * 7):
    """rpn_label_matches for the separated-classifier groups (the label half of
    SeperateClassifier.seperate_rpn_loss_evaluator, seperate_classifier.py:90-109): targets = the flat list of nb G
    ground-truth tensors [n, 7], entry b G + g the boxes of scene b whose class lies in group g (rpn_group_targets);
    segment (scene, group) is an example of the same aabr_rpn_label_generation_targets call, a scene's rows of the anchor
    tables repeated for its groups, at most 16 segments per call.  A segment without ground truth: every anchor
    negative, as an example without ground truth.  Returns the flat list of nb G tuples rpn_label_matches returns,
    exactly what it returns for each group's filtered targets."""
    G = int(G)
    nb = int(batch_size) if batch_size is not None else len(targets) // G
    if len(targets) != nb * G:
        raise ValueError("rpn_label_matches_grouped: %d target lists, expected %d scenes x %d groups" % (len(targets), nb, G))
    return rpn_label_matches(maps, base_anchors, strides, voxel_scale, list(targets), aug_thickness, criterion, fg_iou,
                             bg_iou, batch_size=nb, yaw_threshold=yaw_threshold,
                             allow_low_quality_matches=allow_low_quality_matches, regression_targets=regression_targets,
                             weights=weights, groups=G)


def rpn_group_targets(targets, labels, sc):
    """A batch's ground truth split by separated-classifier group (SeperateClassifier.seperate_targets,
    seperate_classifier.py:111-132), ordered by (scene, group, group-local label, row): the order in which the reference
    concatenates a group's targets, which decides ties in the label generation.  targets: list over scenes of [n_b, 7];
    labels: list over scenes of [n_b] ORIGINAL class ids; sc: the SeperateClassifier (or its grouped_classes).  One key
    per box (aabr_roi_gt_group_keys: (b G + g) 32 + group-local label, behind every segment when no group owns the
    label -- such a box is dropped), ONE stable torch.sort, one gather.  The per-segment sizes cost ONE host read -- none
    when the labels are host tensors: the keys are then formed on the host by the same rule.
    Returns (boxes, local_labels, rows, counts): boxes[b][g] [n, 7] and local_labels[b][g] / rows[b][g] int64 [n] (the
    group-local label and the scene's ground-truth row of each) are views of three tensors; counts[b][g] = n."""
    import roi_glue
    gc, c_tot, class_nums, cols = roi_glue.sep_group_tables(sc)
    G, nb = len(gc), len(targets)
    if nb != len(labels):
        raise ValueError("rpn_group_targets: targets and labels differ in length")
    g_b = [int(t.shape[0]) for t in targets]
    if any(int(l.numel()) != n for l, n in zip(labels, g_b)):
        raise ValueError("rpn_group_targets: labels do not match the targets")
    dev = targets[0].device if nb else torch.device("cpu")
    S = nb * G
    if all(not l.is_cuda for l in labels):
        lut = torch.full((c_tot,), -1, dtype=torch.int64)
        for g, cs in enumerate(gc):
            for i, c in enumerate(cs):
                lut[c] = g * 32 + i
        tl = torch.cat([l.reshape(-1).long() for l in labels]) if nb else torch.zeros(0, dtype=torch.int64)
        scene = torch.repeat_interleave(torch.arange(nb), torch.tensor(g_b, dtype=torch.int64)) if nb else tl
        owned = (tl >= 0) & (tl < c_tot)
        code = torch.where(owned, lut[tl.clamp(0, c_tot - 1)], torch.full_like(tl, -1))
        keys = torch.where(code >= 0, scene * (G * 32) + code, torch.full_like(tl, S * 32))
        keys, perm = torch.sort(keys, stable=True)
        counts = torch.bincount(keys // 32, minlength=S + 1)[:S].tolist()
        keys, perm = keys.to(dev), perm.to(dev)
    else:
        lib = _hip.load()
        tl = torch.cat([l.reshape(-1) for l in labels]).to(device=dev, dtype=torch.int64).contiguous()
        keys = torch.empty(sum(g_b), dtype=torch.int64, device=dev)
        per, o = max(16 // G, 1), 0                                       # the key kernel takes up to 16 segments per call
        for b0 in range(0, nb, per):
            gc_b = g_b[b0:b0 + per]
            part = keys[o:o + sum(gc_b)]
            if part.numel() == 0:
                continue
            check(lib.aabr_roi_gt_group_keys(ptr(tl[o:]), len(gc_b), _hip.i64xn(gc_b), G, c_tot, class_nums, cols, ptr(part),
                                             stream()))
            if nb > per:                                                  # a later chunk's segments follow the earlier ones
                part.copy_(torch.where(part < len(gc_b) * G * 32, part + b0 * G * 32, torch.full_like(part, S * 32)))
            o += sum(gc_b)
        keys, perm = torch.sort(keys, stable=True)                        # the one sort: (segment, group-local label, row)
        counts = _hip.read_back(torch.bincount(keys // 32, minlength=S + 1)[:S].to(torch.int32))      # the one read
        counts = [int(v) for v in counts]
    tg = torch.cat([t.reshape(-1, 7) for t in targets]).to(device=dev, dtype=torch.float32)[perm]
    first = [0]
    for n in g_b:
        first.append(first[-1] + n)
    local = keys % 32
    scene_of = torch.repeat_interleave(torch.arange(nb), torch.tensor(g_b, dtype=torch.int64)).to(dev) if nb else perm
    rows = perm - torch.tensor(first[:-1] + [0], dtype=torch.int64).to(dev)[scene_of[perm]] if nb else perm
    boxes, loc, rws, cnt, o = [], [], [], [], 0
    for b in range(nb):
        cb = counts[b * G:(b + 1) * G]
        boxes.append([]), loc.append([]), rws.append([]), cnt.append(cb)
        for n in cb:
            boxes[b].append(tg[o:o + n]), loc[b].append(local[o:o + n]), rws[b].append(rows[o:o + n])
            o += n
    return boxes, loc, rws, cnt


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
    """aabr_rpn_loss_*: one segment per example, losses 0-dim; with cfg["G"] (aabr_rpn_loss_grouped_*) one segment per
    (scene, group), the inputs group-major, losses [G]"""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        lib = _hip.load()
        n_maps, G = cfg["n_maps"], cfg["G"]
        obj, reg = tensors[:n_maps], tensors[n_maps:]
        dev = obj[0].device
        bf16 = int(obj[0].dtype == torch.bfloat16)
        nb, B = cfg["nb"], cfg["B"]
        lead, ns = ((), nb) if G is None else ((G,), nb * G)
        obj_c = [o.reshape(lead + (-1,)).contiguous() for o in obj]
        reg_c = [r.reshape(lead + (-1, 7)).contiguous() for r in reg]
        sel = torch.empty((ns, B), dtype=torch.int64, device=dev)
        info = torch.empty((ns, 8), dtype=torch.int32, device=dev)
        obj_loss = torch.empty(lead, dtype=torch.float32, device=dev)
        box_loss = torch.empty(lead, dtype=torch.float32, device=dev)
        words = lib.aabr_rpn_loss_scratch_words(nb) if G is None else lib.aabr_rpn_loss_grouped_scratch_words(nb, G)
        scr = _hip.workspace("rpn_loss", int(words) + 2, torch.int32, dev)
        so = (-scr.data_ptr() // 4) % 2
        forward = lib.aabr_rpn_loss_forward if G is None else lib.aabr_rpn_loss_grouped_forward
        check(forward(
            n_maps, _hip.ptrs(cfg["coords"]), _hip.ptrs(obj_c), _hip.ptrs(reg_c), *cfg["rows"], bf16, cfg["A"], nb, *lead,
            cfg["seg"], cfg["site"], _hip.ptrs(cfg["labels"]), _hip.ptrs(cfg["targets"]), cfg["seed"], B, cfg["num_pos"],
            cfg["beta"], ptr(sel), ptr(info), ptr(obj_loss), ptr(box_loss), scr.data_ptr() + 4 * so, stream()))
        ctx.cfg = cfg
        ctx.save_for_backward(sel, info, *obj_c, *reg_c)
        ctx.shapes = [t.shape for t in tensors]
        ctx.mark_non_differentiable(sel, info)
        return obj_loss, box_loss, sel, info

    @staticmethod
    def backward(ctx, g_obj, g_box, _g_sel, _g_info):
        lib = _hip.load()
        cfg = ctx.cfg
        n_maps, G = cfg["n_maps"], cfg["G"]
        saved = ctx.saved_tensors
        sel, info, obj_c, reg_c = saved[0], saved[1], saved[2:2 + n_maps], saved[2 + n_maps:]
        dev, dt = obj_c[0].device, obj_c[0].dtype
        lead = () if G is None else (G,)
        g_obj = (g_obj if g_obj is not None else torch.zeros(lead, device=dev)).float().contiguous()
        g_box = (g_box if g_box is not None else torch.zeros(lead, device=dev)).float().contiguous()
        sizes = [o.numel() for o in obj_c] + [r.numel() for r in reg_c]
        flat = torch.zeros(sum(sizes), dtype=dt, device=dev)       # one fill for every gradient
        grads = list(torch.split(flat, sizes))
        backward = lib.aabr_rpn_loss_backward if G is None else lib.aabr_rpn_loss_grouped_backward
        check(backward(
            n_maps, _hip.ptrs(obj_c), _hip.ptrs(reg_c), *cfg["rows"], int(dt == torch.bfloat16), cfg["A"], cfg["nb"], *lead,
            cfg["seg"], cfg["site"], _hip.ptrs(cfg["targets"]), cfg["B"], cfg["beta"], ptr(sel), ptr(info), ptr(g_obj),
            ptr(g_box), _hip.ptrs(grads[:n_maps]), _hip.ptrs(grads[n_maps:]), stream()))
        return (None,) + tuple(g.view(s) for g, s in zip(grads, ctx.shapes))


def _rpn_loss_cfg(maps, objectness, box_regression, labels, base_anchors, G, batch_size_per_image, positive_fraction,
                  yaw_loss_mode, seed):
    """the checks and tables rpn_loss (G None: a segment is an example) and rpn_loss_grouped (a segment is (scene,
    group), len(labels) a multiple of G) share -> _RpnLoss's cfg"""
    parse_yaw_loss_mode(yaw_loss_mode)
    n_maps, ng = len(maps), G or 1
    if not (n_maps == len(objectness) == len(box_regression) == len(base_anchors)):
        raise ValueError("maps, objectness, box_regression and base_anchors differ in length")
    nb = len(labels) // ng
    if any(len(l) < 4 or l[3] is None for l in labels):
        raise ValueError("labels need the regression targets: rpn_label_matches%s(..., regression_targets=True)"
                         % ("" if G is None else "_grouped"))
    dt = objectness[0].dtype
    if dt not in _BF16_OR_F32 or any(t.dtype != dt for t in list(objectness) + list(box_regression)):
        raise TypeError("objectness and box_regression must all be float32, or all bfloat16")
    grids = [t.metadata.grids[_SCN._key(t.spatial_size)] for t in maps]
    A = int(base_anchors[0].shape[0])
    counts = _site_counts(grids, nb, objectness[0].device)
    V = [sum(c) for c in counts]
    for m in range(n_maps):
        if objectness[m].numel() != ng * V[m] * A or box_regression[m].numel() != ng * V[m] * A * 7:
            raise ValueError("map %d: objectness / box_regression do not hold %s%d sites x %d anchors"
                             % (m, "" if G is None else "%d groups x " % G, V[m], A))
    seg, site, n_anchor = _anchor_tables(counts, A, 0, nb)
    for e in range(nb * ng):
        if labels[e][0].numel() != n_anchor[e // ng] or labels[e][3].shape[0] != n_anchor[e // ng]:
            raise ValueError("%s %d: the labels do not match the maps' anchors" % ("example" if G is None else "segment", e))
    lab = [l[0] if l[0].dtype == torch.int64 else l[0].long() for l in labels]
    return {"n_maps": n_maps, "nb": nb, "G": G, "A": A, "B": int(batch_size_per_image),
            "num_pos": int(batch_size_per_image * positive_fraction), "beta": 1.0 / 9,
            "seed": int(draw_seed() if seed is None else seed) & 0xffffffff,
            "rows": () if G is None else (_hip.i64xn(V),),                 # the grouped entries' rows_host argument
            "coords": [g.coords for g in grids], "seg": _hip.i32xn(seg), "site": _hip.i32xn(site),
            "labels": [l.contiguous() for l in lab], "targets": [l[3].float().contiguous() for l in labels]}


def rpn_loss(maps, objectness, box_regression, labels, base_anchors, batch_size_per_image=256, positive_fraction=0.5,
             yaw_loss_mode="Diff", seed=None, return_samples=False, return_info=False):
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
    (example-major), positives then negatives, -1 padded; with `return_info` then the int32 [nb, 8] info words of
    aabr_rpn_loss_forward (num_pos, num_neg, P, N, candidates, overflow, N_s)."""
    if len(labels) == 0:
        raise ValueError("no examples")
    cfg = _rpn_loss_cfg(maps, objectness, box_regression, labels, base_anchors, None, batch_size_per_image,
                        positive_fraction, yaw_loss_mode, seed)
    obj_loss, box_loss, sel, info = _RpnLoss.apply(cfg, *objectness, *box_regression)
    out = (obj_loss, box_loss) + ((sel,) if return_samples else ()) + ((info,) if return_info else ())
    return out


def rpn_loss_grouped(maps, objectness, box_regression, labels, base_anchors, G, batch_size_per_image=256,
                     positive_fraction=0.5, yaw_loss_mode="Diff", seed=None, return_samples=False):
    """rpn_loss for every separated-classifier group in one call (SeperateClassifier.seperate_rpn_loss_evaluator,
    seperate_classifier.py:90-109, which runs the loss evaluator once per group).  objectness[m] [G, V_m A] and
    box_regression[m] [G, V_m A, 7]: the group-major outputs of rpn_head_grouped, fp32 or bf16, read where they lie;
    labels: the flat list of nb G tuples of rpn_label_matches_grouped (entry b G + g: scene b against group g's ground
    truth).  Segment (scene, group) is sampled as rpn_loss samples a scene -- the key hashes the scene, so with the same
    seed group g's selection, N_s, losses and gradients are the bits rpn_loss gives on the group's slices and labels.
    `seed=None` draws ONE seed for the call.  An empty group sample gives NaN losses and zero gradients.
    Device work: 1 memset + 4 launches per 16 segments + 1 forward, 1 launch per 16 segments backward; no host read.
    Returns (objectness_losses [G], box_losses [G]) with autograd to objectness / box_regression; with `return_samples`
    also the int64 [nb G, batch_size_per_image] selected indices (into group g's scene-major label lists) and the int32
    [nb G, 8] info words."""
    G = int(G)
    if G < 2 or len(labels) == 0 or len(labels) % G:
        raise ValueError("rpn_loss_grouped: G >= 2 and one label tuple per (scene, group), got G = %d, %d tuples"
                         % (G, len(labels)))
    cfg = _rpn_loss_cfg(maps, objectness, box_regression, labels, base_anchors, G, batch_size_per_image,
                        positive_fraction, yaw_loss_mode, seed)
    obj_loss, box_loss, sel, info = _RpnLoss.apply(cfg, *objectness, *box_regression)
    return (obj_loss, box_loss, sel, info) if return_samples else (obj_loss, box_loss)


# ---------------------------------------------------------------------------------------------------- the RPN head
RPN_HEAD_MAX_MAPS, RPN_HEAD_MAX_ANCHORS = 8, 4
RPN_HEAD_CHANNELS = (32, 64, 96, 128)


class _RpnHead(torch.autograd.Function):
    """SingleConvRPNHead_Sparse3D over every map in one launch (csrc/rpn_head.hip); the hidden activation is written to
    memory only when some input requires a gradient.  G None: aabr_rpn_head_*, outputs [V A] and [V A, 7]; with G
    separated-classifier groups: aabr_rpn_head_grouped_*, Wc [A G, C], Wr [7 A G, C] in the reference's layout, the
    outputs group-major [G, V A] and [G, V A, 7].  `bf16`: the maps are bf16 rows (aabr_rpn_head_*_bf16): the outputs
    and parameter gradients stay fp32, the maps' gradients come back as bf16 views of one allocation"""

    @staticmethod
    def forward(ctx, A, G, bf16, W1, b1, Wc, bc, Wr, br, *feats):
        lib = _hip.load()
        dev = W1.device
        C, n_maps = int(W1.shape[0]), len(feats)
        params = [p.contiguous() for p in (W1, b1, Wc, bc, Wr, br)]
        feats = [f.contiguous() for f in feats]
        rows = [int(f.shape[0]) for f in feats]
        lead = () if G is None else (G,)
        obj = [torch.empty(lead + (v * A,), dtype=torch.float32, device=dev) for v in rows]     # every element is written
        reg = [torch.empty(lead + (v * A, 7), dtype=torch.float32, device=dev) for v in rows]
        need = any(ctx.needs_input_grad)
        hidden = torch.empty((sum(rows), C), dtype=torch.float32, device=dev) if need else None
        tab = (_hip.AabrRpnMap * n_maps)()
        for m in range(n_maps):
            tab[m].features, tab[m].rows = ptr(feats[m]), rows[m]
            tab[m].objectness, tab[m].box_regression = ptr(obj[m]), ptr(reg[m])
        forward = getattr(lib, "aabr_rpn_head%s_forward%s" % ("" if G is None else "_grouped", "_bf16" if bf16 else ""))
        check(forward(tab, n_maps, C, A, *lead, *[ptr(p) for p in params], ptr(hidden), stream()))
        if need:
            ctx.save_for_backward(hidden, params[0], params[2], params[4], *feats)
        ctx.cfg = (A, G, C, n_maps, rows, bf16)
        return tuple(obj) + tuple(reg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        lib = _hip.load()
        A, G, C, n_maps, rows, bf16 = ctx.cfg
        hidden, W1, Wc, Wr = ctx.saved_tensors[:4]
        feats = ctx.saved_tensors[4:]
        dev = W1.device
        g_obj = [g.contiguous() if g is not None else None for g in grads[:n_maps]]
        g_reg = [g.contiguous() if g is not None else None for g in grads[n_maps:]]
        d_all = torch.empty((sum(rows), C), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)  # all written
        d_f = list(torch.split(d_all, rows))
        AG = A * (G or 1)
        sizes = (C * C, C, AG * C, AG, 7 * AG * C, 7 * AG)
        d_p = list(torch.split(torch.empty(sum(sizes), dtype=torch.float32, device=dev), sizes))
        t_rows = lib.aabr_rpn_head_tile_rows(C)
        tiles = sum(-(-v // t_rows) for v in rows)
        lead = () if G is None else (G,)
        key = "rpn_head" if G is None else "rpn_head_grouped"
        floats = getattr(lib, "aabr_%s_scratch_floats" % key)
        backward = getattr(lib, "aabr_%s_backward%s" % (key, "_bf16" if bf16 else ""))
        floats = int(floats(tiles, C, A, *lead))
        scr = _hip.workspace(key, floats, torch.float32, dev) if floats else None
        tab = (_hip.AabrRpnMap * n_maps)()
        for m in range(n_maps):
            tab[m].features, tab[m].rows, tab[m].d_features = ptr(feats[m]), rows[m], ptr(d_f[m])
            tab[m].objectness, tab[m].box_regression = ptr(g_obj[m]), ptr(g_reg[m])
        check(backward(tab, n_maps, C, A, *lead, ptr(W1), ptr(Wc), ptr(Wr), ptr(hidden), *[ptr(p) for p in d_p],
                       ptr(scr), stream()))
        return (None, None, None, d_p[0].view(C, C), d_p[1], d_p[2].view(AG, C), d_p[3], d_p[4].view(7 * AG, C), d_p[5]) + tuple(d_f)


def _as_out_in(name, w):
    """a Conv2d weight [out, in, 1, 1] or a Linear weight [out, in] -> [out, in]"""
    if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
        return w.reshape(w.shape[0], w.shape[1])
    if w.dim() != 2:
        raise ValueError("rpn_head: %s must be [out, in] or [out, in, 1, 1], got %s" % (name, tuple(w.shape)))
    return w


RPN_HEAD_MAX_GROUPS, RPN_HEAD_MAX_COLUMNS = 8, 16
RPN_HEAD_GROUP_LIMITS = ("C in %s, 1 <= A <= %d anchors per site, 2 <= G <= %d groups, A G <= %d"
                         % (RPN_HEAD_CHANNELS, RPN_HEAD_MAX_ANCHORS, RPN_HEAD_MAX_GROUPS, RPN_HEAD_MAX_COLUMNS))


def rpn_head_group_limits_ok(C, A, G):
    return (C in RPN_HEAD_CHANNELS and 1 <= A <= RPN_HEAD_MAX_ANCHORS and 2 <= G <= RPN_HEAD_MAX_GROUPS
            and A * G <= RPN_HEAD_MAX_COLUMNS)


def _rpn_head(fn, G, features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b, feature_dtype=torch.float32):
    """the checks and the launch of rpn_head (G None) and rpn_head_grouped; `fn`: the caller's name, for the messages"""
    if feature_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("%s: feature_dtype must be torch.float32 or torch.bfloat16, got %s" % (fn, feature_dtype))
    feats = [f.features if hasattr(f, "features") else f for f in features]
    if not 1 <= len(feats) <= RPN_HEAD_MAX_MAPS:
        raise ValueError("%s: 1 to %d maps, got %d" % (fn, RPN_HEAD_MAX_MAPS, len(feats)))
    w1, wc, wr = _as_out_in("conv_w", conv_w), _as_out_in("cls_w", cls_w), _as_out_in("reg_w", reg_w)
    for k, t in [("conv_w", w1), ("conv_b", conv_b), ("cls_w", wc), ("cls_b", cls_b), ("reg_w", wr), ("reg_b", reg_b)]:
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s (the parameters are fp32 in either feature storage)"
                            % (fn, k, t.dtype))
    for i, f in enumerate(feats):                       # every map in the one storage the caller names
        if f.dtype != feature_dtype:
            want = "float32" if feature_dtype == torch.float32 else "bfloat16 (feature_dtype=torch.bfloat16)"
            raise TypeError("%s: features[%d] must be %s, got %s; bf16 maps are read in place with the keyword "
                            "feature_dtype=torch.bfloat16 (default float32), all maps in one storage"
                            % (fn, i, want, f.dtype))
    C, AG = int(w1.shape[1]), int(wc.shape[0])          # AG: the rows of cls_w, A without groups
    if G is None:
        A = AG
        if C not in RPN_HEAD_CHANNELS:
            raise ValueError("%s: C = %d; supported: a multiple of 32 from 32 to 128" % (fn, C))
        if not 1 <= A <= RPN_HEAD_MAX_ANCHORS:
            raise ValueError("%s: A = %d anchors per site; supported: 1 to %d" % (fn, A, RPN_HEAD_MAX_ANCHORS))
    else:
        A = AG // G if G > 0 and AG % G == 0 else 0
        if not rpn_head_group_limits_ok(C, A, G):
            raise ValueError("%s: C = %d, cls_w with %d rows, G = %d; supported: %s" % (fn, C, AG, G, RPN_HEAD_GROUP_LIMITS))
    n = "A" if G is None else "A G"
    if tuple(w1.shape) != (C, C) or tuple(wc.shape) != (AG, C) or tuple(wr.shape) != (7 * AG, C):
        raise ValueError("%s: conv_w [C, C], cls_w [%s, C], reg_w [7 %s, C]; got %s, %s, %s"
                         % (fn, n, n, tuple(w1.shape), tuple(wc.shape), tuple(wr.shape)))
    if tuple(conv_b.shape) != (C,) or tuple(cls_b.shape) != (AG,) or tuple(reg_b.shape) != (7 * AG,):
        raise ValueError("%s: the biases must be [C], [%s] and [7 %s]" % (fn, n, n))
    for i, f in enumerate(feats):
        if f.dim() != 2 or int(f.shape[1]) != C:
            raise ValueError("%s: features[%d] must be [V, %d], got %s" % (fn, i, C, tuple(f.shape)))
    _hip.require_gpu(feats[0])
    out = _RpnHead.apply(A, G, feature_dtype == torch.bfloat16, w1, conv_b, wc, cls_b, wr, reg_b, *feats)
    return list(out[:len(feats)]), list(out[len(feats):])


def rpn_head(features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b, feature_dtype=torch.float32):
    """SingleConvRPNHead_Sparse3D.forward (modeling/rpn/rpn_sparse3d.py:109-131) for all maps at once:
      t = relu(f conv_w^T + conv_b), objectness = t cls_w^T + cls_b, box_regression = t reg_w^T + reg_b
    features: a list (1..8 maps) of SparseConvNetTensors or of [V_m, C] fp32 tensors; the weights as [out, in] or the
    reference's Conv2d [out, in, 1, 1]: conv_w [C, C], cls_w [A, C], reg_w [7 A, C] (channel a 7 + j, 'box_toghter').
    C in {32, 64, 96, 128}, 1 <= A <= 4.  Returns (objectness, box_regression): lists over the maps of [V_m A] and
    [V_m A, 7] in the [site, yaw] flatten order rpn_proposals, rpn_label_matches and rpn_loss read.
    Device work: forward 1 library launch whatever the number of maps (nothing concatenated, the hidden activation
    reaches memory only when a gradient is required); backward 2 (the fused main kernel and the in-order reduction of its
    per-workgroup partials: deterministic, no atomics).  No host read.
    `feature_dtype=torch.bfloat16`: every map is bf16 storage, read in place (no widened copy); the parameters and both
    outputs stay fp32 and are the bits of the fp32 call on `f.float()`; autograd delivers bf16 gradients to the maps, the
    fp32 call's values rounded once.  The keyword is explicit: a bf16 map without it raises TypeError."""
    return _rpn_head("rpn_head", None, features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b, feature_dtype)


def rpn_head_grouped(features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b, G, feature_dtype=torch.float32):
    """SingleConvRPNHead_Sparse3D.forward with MODEL.SEPARATE_CLASSES and SEPARATE_RPN (rpn_sparse3d.py:95-131), G =
    len(SEPARATE_CLASSES) + 1 branches on one hidden layer, for all maps at once.  The weights in the reference's layout
    ([out, in] or Conv2d [out, in, 1, 1]): cls_w [A G, C] with row a G + g, reg_w [7 A G, C] with row a 7 G + 7 g + k.
    C in {32, 64, 96, 128}, 1 <= A <= 4, 2 <= G <= 8, A G <= 16.
    Returns (objectness, box_regression): lists over the maps of [G, V_m A] and [G, V_m A, 7]: group g's slice is a
    contiguous tensor in the [site, yaw] order of rpn_head, and holds the bits rpn_head gives on that group's weight rows.
    Device work as rpn_head: forward 1 library launch, backward 2; nothing is permuted or copied.  No host read.
    `feature_dtype` as in rpn_head."""
    return _rpn_head("rpn_head_grouped", int(G), features, conv_w, conv_b, cls_w, cls_b, reg_w, reg_b, feature_dtype)


class _Cfg(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def clone(self):
        return self


def rpn_cfg(C=32, anchor_sizes=((0.4, 1.5, 1.5), (1.5, 1.5, 1.0)), yaws=(0, -1.57), strides=((8, 8, 8), (16, 16, 16)),
            voxel_scale=20.0, pre_nms_top_n=(200, 200), post_nms_top_n=(50, 50), nms_thresh=0.5, rpn_only=False,
            add_gt_proposals=False, separate=(), separate_rpn=True, batch_size_per_image=256, positive_fraction=0.5,
            classes=("background", "wall", "door"), separate_ids=None):
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
    if separate_ids is not None:
        model.SEPARATE_CLASSES_ID = [list(g) for g in separate_ids]
    return _Cfg(MODEL=model, SPARSE3D=_Cfg(VOXEL_SCALE=voxel_scale, nPlaneMap=C), INPUT=_Cfg(CLASSES=list(classes)))
