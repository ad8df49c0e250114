"""The RPN head on the device (csrc/rpn_head.hip, rpn_glue.rpn_head, the RPNHead / RPNModule modules) against the fp64
definition of tests/rpn_head_ref.py: every element inside its derived bound, the device's t > 0 mask against the
definition's outside the undecidable units (counted, capped at 1 %).  Shapes are the smallest that reach each path:
T = aabr_rpn_head_tile_rows(C) rows per tile, maps that cross a tile edge by one row, an empty map, a one-row map, more
tiles than workgroups, a single tile."""
import numpy as np
import pytest
import torch

import rpn_head_ref as R
import synth_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
NAN = float("nan")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lib():
    import _hip
    return _hip.load()


def _ok(what, got, ref):
    w, bad = R.worst(got, ref)
    print("%s: max |device - fp64| / bound = %.4g" % (what, w))
    assert bad == 0, (what, w)


class _Run(object):
    """one case through the C ABI: every output buffer is pre-filled with NaN"""

    def __init__(self, C, A, rows, seed):
        self.C, self.A, self.rows = C, A, list(rows)
        self.p, self.f, self.g_obj, self.g_reg = R.make_case(C, A, rows, seed)
        self.pd = {k: _t(v) for k, v in self.p.items()}
        self.fd = [_t(f) for f in self.f]
        self.god, self.grd = [_t(g) for g in self.g_obj], [_t(g) for g in self.g_reg]
        T = _lib().aabr_rpn_head_tile_rows(C)
        self.tiles = sum(-(-n // T) for n in rows)
        self.tag = "C %d A %d rows %s" % (C, A, self.rows)

    def table(self, o, r, d=None):
        import _hip
        tab = (_hip.AabrRpnMap * len(self.rows))()
        for m, n in enumerate(self.rows):
            tab[m].features, tab[m].rows = _hip.ptr(self.fd[m]), n
            tab[m].objectness = _hip.ptr(o[m]) if o is not None else None
            tab[m].box_regression = _hip.ptr(r[m]) if r is not None else None
            tab[m].d_features = _hip.ptr(d[m]) if d is not None else None
        return tab

    def forward(self, with_hidden=True):
        from _hip import check, ptr, stream
        C, A, pd = self.C, self.A, self.pd
        obj = [torch.full((n, A), NAN, device=DEV) for n in self.rows]
        reg = [torch.full((n, 7 * A), NAN, device=DEV) for n in self.rows]
        hidden = torch.full((sum(self.rows), C), NAN, device=DEV) if with_hidden else None
        check(_lib().aabr_rpn_head_forward(self.table(obj, reg), len(self.rows), C, A, ptr(pd["conv_w"]), ptr(pd["conv_b"]),
                                           ptr(pd["cls_w"]), ptr(pd["cls_b"]), ptr(pd["reg_w"]), ptr(pd["reg_b"]),
                                           ptr(hidden), stream()))
        return obj, reg, hidden

    def backward(self, hidden, null_obj=False, null_reg=False, zero_obj=False, zero_reg=False):
        from _hip import check, ptr, stream
        lib = _lib()
        C, A, pd = self.C, self.A, self.pd
        d_f = [torch.full((n, C), NAN, device=DEV) for n in self.rows]
        grads = {k: torch.full(tuple(v.shape), NAN, device=DEV) for k, v in pd.items()}
        floats = lib.aabr_rpn_head_scratch_floats(self.tiles, C, A)
        scr = torch.full((max(floats, 1),), NAN, device=DEV)
        go = None if null_obj else [torch.zeros_like(g) for g in self.god] if zero_obj else self.god
        gr = None if null_reg else [torch.zeros_like(g) for g in self.grd] if zero_reg else self.grd
        check(lib.aabr_rpn_head_backward(self.table(go, gr, d_f), len(self.rows), C, A, ptr(pd["conv_w"]), ptr(pd["cls_w"]),
                                         ptr(pd["reg_w"]), ptr(hidden), ptr(grads["conv_w"]), ptr(grads["conv_b"]),
                                         ptr(grads["cls_w"]), ptr(grads["cls_b"]), ptr(grads["reg_w"]),
                                         ptr(grads["reg_b"]), ptr(scr), stream()))
        return d_f, grads

    def check_against_definition(self):
        """forward, the mask, and all gradients; returns the device outputs"""
        obj, reg, hidden = self.forward()
        f_all = np.concatenate(self.f)
        fwd = R.forward(f_all, self.p)
        t_dev = hidden.cpu().numpy()
        _ok("objectness " + self.tag, torch.cat(obj).cpu().numpy(), fwd["obj"])
        _ok("box regression " + self.tag, torch.cat(reg).cpu().numpy(), fwd["reg"])
        _ok("hidden " + self.tag, t_dev, fwd["t"])
        und = R.undecided(fwd)
        share = float(und.mean()) if und.size else 0.0
        print("undecidable hidden units: %d of %d" % (int(und.sum()), und.size))
        assert share < R.MAX_UNDECIDED
        assert (((t_dev > 0) == (fwd["pre"].v > 0)) | und).all()                 # the mask, outside the undecidable units
        d_f, grads = self.backward(hidden)
        bwd = R.backward(f_all, self.p, np.concatenate(self.g_obj), np.concatenate(self.g_reg), t_dev, fwd)
        d_all = torch.cat(d_f).cpu().numpy()
        assert not np.isnan(d_all).any()                                       # every d_f element is written
        _ok("d_f " + self.tag, d_all, bwd["d_f"])
        for k in self.p:
            _ok("d_%s %s" % (k, self.tag), grads[k].cpu().numpy(), bwd["d_" + k])
        return obj, reg, hidden, d_f, grads


def _bits(ts):
    return b"".join(t.cpu().numpy().tobytes() for t in ts)


# ------------------------------------------------------------------------------------------------ 1 and 3
def test_entry_points_against_the_definition():
    T = _lib().aabr_rpn_head_tile_rows(128)
    assert T == _lib().aabr_rpn_head_tile_rows(32)
    for C, A, rows, seed in R.entry_cases(T):
        _Run(C, A, rows, seed).check_against_definition()


def test_outputs_do_not_depend_on_storing_the_hidden_activation():
    T = _lib().aabr_rpn_head_tile_rows(128)
    for C, A, rows, seed in R.hidden_cases(T):
        run = _Run(C, A, rows, seed)
        o1, r1, hidden, _, _ = run.check_against_definition()
        o0, r0, none = run.forward(with_hidden=False)
        assert none is None and _bits(o0 + r0) == _bits(o1 + r1)
        assert not torch.isnan(hidden).any()


# ------------------------------------------------------------------------------------------------ 2
def test_more_tiles_than_groups_and_a_single_tile_are_deterministic():
    lib = _lib()
    T, gmax = lib.aabr_rpn_head_tile_rows(32), lib.aabr_rpn_head_groups(2 ** 40)
    many = _Run(32, 2, ((gmax + 1) * T + 5,), 5)
    assert many.tiles == gmax + 2 and lib.aabr_rpn_head_groups(many.tiles) == gmax
    one = _Run(32, 2, (7,), 6)
    assert one.tiles == 1 and lib.aabr_rpn_head_groups(1) == 1
    for run in (many, one):
        _, _, hidden, d_f, grads = run.check_against_definition()
        d_f2, grads2 = run.backward(hidden)
        assert _bits(d_f) == _bits(d_f2)
        assert all(_bits([grads[k]]) == _bits([grads2[k]]) for k in grads)


# ------------------------------------------------------------------------------------------------ 4 and all maps empty
def test_null_gradients_equal_zeros_bit_for_bit():
    T = _lib().aabr_rpn_head_tile_rows(32)
    run = _Run(32, 2, (T + 3, 0, 2), 7)
    _, _, hidden = run.forward()
    for kw_null, kw_zero in (({"null_obj": True}, {"zero_obj": True}), ({"null_reg": True}, {"zero_reg": True}),
                             ({"null_obj": True, "null_reg": True}, {"zero_obj": True, "zero_reg": True})):
        d_n, g_n = run.backward(hidden, **kw_null)
        d_z, g_z = run.backward(hidden, **kw_zero)
        assert _bits(d_n) == _bits(d_z) and not np.isnan(torch.cat(d_n).cpu().numpy()).any()
        assert all(_bits([g_n[k]]) == _bits([g_z[k]]) for k in g_n)
    d, g = run.backward(hidden, null_obj=True, null_reg=True)
    assert not torch.cat(d).any() and not any(v.any() for v in g.values())


def test_all_maps_empty_launch_nothing_and_zero_the_weight_gradients():
    run = _Run(64, 4, (0, 0), 8)
    obj, reg, hidden = run.forward()
    assert all(o.numel() == 0 for o in obj + reg)
    _, grads = run.backward(hidden)
    assert all(not v.any() and not torch.isnan(v).any() for v in grads.values())


# ------------------------------------------------------------------------------------------------ 5
def test_glue_autograd_against_the_torch_modules_in_every_input_form():
    import rpn_glue
    import sparseconvnet as scn
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    C, A, rows = 64, 4, (70, 0, 9)
    p, f, g_obj, g_reg = R.make_case(C, A, rows, 9)
    head = RPNHead(rpn_glue.rpn_cfg(C=C), C, A).to(DEV)
    with torch.no_grad():
        for mod, k in ((head.conv, "conv"), (head.cls_logits, "cls"), (head.bbox_pred, "reg")):
            mod.weight.copy_(_t(p[k + "_w"]).view_as(mod.weight))
            mod.bias.copy_(_t(p[k + "_b"]))
    go = [_t(g).view(1, n, A, 1) for g, n in zip(g_obj, rows)]
    gr = [_t(g).view(1, n, A, 7) for g, n in zip(g_reg, rows)]

    def run(form, fused):
        head.fused = fused
        head.zero_grad()
        leaves = [_t(x).requires_grad_(True) for x in f]
        if form == "rows":
            xs = leaves
        elif form == "sparse":
            xs = [scn.SparseConvNetTensor(x, None, None) for x in leaves]
        else:
            xs = [x.t().unsqueeze(0).unsqueeze(3) for x in leaves]
        logits, bbox = head(xs)
        assert all(tuple(l.shape) == (1, n, A, 1) and tuple(b.shape) == (1, n, A, 7) for l, b, n in zip(logits, bbox, rows))
        loss = sum((l * g).sum() for l, g in zip(logits, go)) + sum((b * g).sum() for b, g in zip(bbox, gr))
        loss.backward()
        grads = [q.grad.clone() for q in head.parameters()] + [x.grad.clone() for x in leaves]
        return [l.detach() for l in logits] + [b.detach() for b in bbox], grads
    out_f, grad_f = run("rows", True)
    for form in ("sparse", "nchw"):
        o, g = run(form, True)
        assert _bits(o) == _bits(out_f) and _bits(g) == _bits(grad_f), form
    assert [tuple(g.shape) for g in grad_f[:6]] == [tuple(q.shape) for q in head.parameters()]
    # against the definition (the bound) and against the torch modules (both within the bound of the definition)
    f_all = np.concatenate(f)
    fwd = R.forward(f_all, p)
    t_dev = np.maximum(f_all.astype(np.float64) @ p["conv_w"].astype(np.float64).T + p["conv_b"], 0)
    out_t, grad_t = run("nchw", False)
    names = ["conv_w", "conv_b", "cls_w", "cls_b", "reg_w", "reg_b"]
    for tag, outs, grads in (("fused", out_f, grad_f), ("torch", out_t, grad_t)):
        _ok(tag + " logits", torch.cat([o.reshape(-1, A) for o in outs[:3]]).cpu().numpy(), fwd["obj"])
        _ok(tag + " bbox", torch.cat([o.reshape(-1, 7 * A) for o in outs[3:]]).cpu().numpy(), fwd["reg"])
    und = R.undecided(fwd)
    assert und.mean() < R.MAX_UNDECIDED
    if not und.any():                                                            # the masks of both sides are the definition's
        bwd = R.backward(f_all, p, np.concatenate(g_obj), np.concatenate(g_reg), t_dev, fwd)
        for tag, grads in (("fused", grad_f), ("torch", grad_t)):
            for k, g in zip(names, grads[:6]):
                _ok("%s d_%s" % (tag, k), g.reshape(p[k].shape).cpu().numpy(), bwd["d_" + k])
            _ok(tag + " d_f", torch.cat(grads[6:]).cpu().numpy(), bwd["d_f"])
    # no gradient required: the hidden activation is not kept, the outputs are the same bits
    head.fused = True
    with torch.no_grad():
        logits, bbox = head([_t(x) for x in f])
    assert _bits(logits + bbox) == _bits(out_f)


# ------------------------------------------------------------------------------------------------ 6
class _Target(object):
    def __init__(self, b):
        self.bbox3d = b


def _small_maps():
    """2 scenes, 2 maps of a few hundred sites, 32 channels: a strided convolution chain, no FPN"""
    import sparseconvnet as scn
    torch.manual_seed(2)
    locs, feats = S.make_batch(2, 1500, 31, 20)
    layer = scn.InputLayer(3, list(S.FULL_SCALE), mode=4)
    c1 = scn.Convolution(3, 9, 32, 2, 2, False).to(DEV)
    c2 = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
    c3 = scn.Convolution(3, 32, 32, 2, 2, False).to(DEV)
    with torch.no_grad():
        x = layer([torch.as_tensor(locs).to(DEV), torch.as_tensor(feats).to(DEV)])
        m0 = c2(c1(x))
        m1 = c3(m0)
    return [m0, m1], [[4.0] * 3, [8.0] * 3]


def test_rpn_module_equals_the_explicit_sequence():
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import build_rpn
    maps, strides = _small_maps()
    assert all(50 <= m.features.shape[0] <= 3000 for m in maps), [m.features.shape for m in maps]
    gts = [_t(S.make_gt_boxes(6, 3)), _t(S.make_gt_boxes(4, 4))]
    targets = [_Target(g) for g in gts]
    kw = dict(C=32, strides=strides, voxel_scale=20.0, pre_nms_top_n=(300, 200), post_nms_top_n=(60, 40))
    cfg = rpn_glue.rpn_cfg(**kw)
    torch.manual_seed(5)
    mod = build_rpn(cfg).to(DEV)
    with torch.no_grad():
        for q in mod.parameters():
            q.normal_(std=0.3)
    mod.seed = 77
    h, gen, rpn = mod.head, mod.anchor_generator, cfg.MODEL.RPN
    A = gen.num_anchors_per_location()
    aug = {"target_Y": 0.4, "anchor_Y": 0, "target_Z": 0.8, "anchor_Z": 0}

    def explicit(train):
        obj, reg = rpn_glue.rpn_head(maps, h.conv.weight, h.conv.bias, h.cls_logits.weight, h.cls_logits.bias,
                                     h.bbox_pred.weight, h.bbox_pred.bias)
        assert all(o.shape == (m.features.shape[0] * A,) and r.shape == (m.features.shape[0] * A, 7)
                   for o, r, m in zip(obj, reg, maps))
        pre, post = (300, 60) if train else (200, 40)
        with torch.no_grad():
            props = rpn_glue.rpn_proposals(maps, [o.detach() for o in obj], [r.detach() for r in reg], gen.cell_anchors,
                                           strides, 20.0, pre, post, 0.5, (0.3, 0.3), batch_size=2)
        if not train:
            return props, None
        labels = rpn_glue.rpn_label_matches(maps, gen.cell_anchors, strides, 20.0, gts, aug, 6, 0.55, 0.2, batch_size=2,
                                            yaw_threshold=0.7, regression_targets=True)
        return props, rpn_glue.rpn_loss(maps, obj, reg, labels, gen.cell_anchors, 256, 0.5, "Diff", seed=77)

    mod.train()
    boxes, losses = mod(None, maps, targets)
    props, (lo, lb) = explicit(True)
    assert set(losses) == {"loss_objectness", "loss_rpn_box_reg"}
    assert torch.equal(losses["loss_objectness"], lo) and torch.equal(losses["loss_rpn_box_reg"], lb)
    assert torch.isfinite(lo) and torch.isfinite(lb)
    assert len(boxes) == 2
    for b, (pb, ps) in zip(boxes, props):
        assert torch.equal(b.bbox3d, pb) and torch.equal(b.get_field("objectness"), ps) and 0 < len(b) <= 60
    (losses["loss_objectness"] + losses["loss_rpn_box_reg"]).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in mod.parameters())
    assert float(h.conv.weight.grad.abs().max()) > 0

    mod.add_gt_proposals = True                                                  # ADD_GT_PROPOSALS: the ground truth behind
    with_gt, _ = mod(None, maps, targets)
    for b, (pb, ps), g in zip(with_gt, props, gts):
        assert torch.equal(b.bbox3d, torch.cat([pb, g])) and len(b) == len(pb) + len(g)
        assert torch.equal(b.get_field("objectness"), torch.cat([ps, torch.ones(len(g), device=DEV)]))
    mod.add_gt_proposals = False

    mod.rpn_only = True                                                          # RPN__ONLY in training: no decode
    none, only = mod(None, maps, targets)
    assert none is None and torch.equal(only["loss_objectness"], lo)
    mod.rpn_only = False

    mod.eval()
    ev, no_loss = mod(None, maps)
    props_e, _ = explicit(False)
    assert no_loss == {}
    for b, (pb, ps) in zip(ev, props_e):
        assert torch.equal(b.bbox3d, pb) and torch.equal(b.get_field("objectness"), ps) and 0 < len(b) <= 40
    mod.rpn_only = True                                                          # RPN-only evaluation: sorted by confidence
    srt, _ = mod(None, maps)
    for b in srt:
        s = b.get_field("objectness")
        assert (s[:-1] >= s[1:]).all()


# ------------------------------------------------------------------------------------------------ 7
def test_head_forward_and_backward_enqueue_without_a_host_read():
    import rpn_glue
    C, A, rows = 32, 2, (130, 0, 5)
    p, f, g_obj, g_reg = R.make_case(C, A, rows, 12)
    pd = {k: _t(v).requires_grad_(True) for k, v in p.items()}
    fd = [_t(x).requires_grad_(True) for x in f]
    go, gr = [_t(g).reshape(-1) for g in g_obj], [_t(g).reshape(-1, 7) for g in g_reg]

    def run():
        for q in list(pd.values()) + fd:
            q.grad = None
        obj, reg = rpn_glue.rpn_head(fd, pd["conv_w"], pd["conv_b"], pd["cls_w"], pd["cls_b"], pd["reg_w"], pd["reg_b"])
        torch.autograd.backward(obj + reg, go + gr)
        return [o.detach().clone() for o in obj + reg] + [q.grad.clone() for q in list(pd.values()) + fd]
    a = run()                                                                    # also sizes the scratch workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _bits(a) == _bits(b)
