"""The RPN head with separated-classifier groups on the device (aabr_rpn_head_grouped_*, rpn_glue.rpn_head_grouped, the
RPNHead module with MODEL.SEPARATE_CLASSES) against the fp64 definition of tests/rpn_head_grouped_ref.py: every element
inside its derived bound, every buffer NaN-filled beforehand, the device's t > 0 mask against the definition's outside
the undecidable units; and against the plain head on each group's weight rows, bit for bit.  Shapes are the smallest that
reach each path: 16 to 128 output columns (one padded tile to four), both ends of C, a map that crosses a tile edge by one
row, an empty map, a one-row map, more tiles than workgroups, a single tile."""
import numpy as np
import pytest
import torch

import rpn_head_grouped_ref as GR
import rpn_head_ref as R

pytestmark = pytest.mark.gpu
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


def _bits(ts):
    return b"".join(t.cpu().numpy().tobytes() for t in ts)


def _table(fd, rows, o, r, d=None):
    import _hip
    tab = (_hip.AabrRpnMap * len(rows))()
    for m, n in enumerate(rows):
        tab[m].features, tab[m].rows = _hip.ptr(fd[m]), n
        tab[m].objectness = _hip.ptr(o[m]) if o is not None else None
        tab[m].box_regression = _hip.ptr(r[m]) if r is not None else None
        tab[m].d_features = _hip.ptr(d[m]) if d is not None else None
    return tab


class _Run(object):
    """one case through the C ABI: every output buffer is pre-filled with NaN"""

    def __init__(self, C, A, G, rows, seed):
        self.C, self.A, self.G, self.rows = C, A, G, list(rows)
        self.p, self.f, self.g_obj, self.g_reg = GR.make_case(C, A, G, rows, seed)      # gradients: packed order
        self.pd = {k: _t(v) for k, v in self.p.items()}
        self.fd = [_t(f) for f in self.f]
        self.god = [_t(GR.to_groups(g, A, G, 1)) for g in self.g_obj]                   # the device's: group-major
        self.grd = [_t(GR.to_groups(g, A, G, 7)) for g in self.g_reg]
        T = _lib().aabr_rpn_head_tile_rows(C)
        self.tiles = sum(-(-n // T) for n in rows)
        self.tag = "C %d A %d G %d rows %s" % (C, A, G, self.rows)

    def forward(self, with_hidden=True):
        from _hip import check, ptr, stream
        C, A, G, pd = self.C, self.A, self.G, self.pd
        obj = [torch.full((G, n, A), NAN, device=DEV) for n in self.rows]
        reg = [torch.full((G, n, A, 7), NAN, device=DEV) for n in self.rows]
        hidden = torch.full((sum(self.rows), C), NAN, device=DEV) if with_hidden else None
        check(_lib().aabr_rpn_head_grouped_forward(_table(self.fd, self.rows, obj, reg), len(self.rows), C, A, G,
                                                   ptr(pd["conv_w"]), ptr(pd["conv_b"]), ptr(pd["cls_w"]), ptr(pd["cls_b"]),
                                                   ptr(pd["reg_w"]), ptr(pd["reg_b"]), ptr(hidden), stream()))
        return obj, reg, hidden

    def plain_forward(self, g):
        """the plain head on group g's weight rows"""
        from _hip import check, ptr, stream
        C, A = self.C, self.A
        pg = {k: _t(v) for k, v in GR.group_params(self.p, A, self.G, g).items()}
        obj = [torch.full((n, A), NAN, device=DEV) for n in self.rows]
        reg = [torch.full((n, A, 7), NAN, device=DEV) for n in self.rows]
        hidden = torch.full((sum(self.rows), C), NAN, device=DEV)
        check(_lib().aabr_rpn_head_forward(_table(self.fd, self.rows, obj, reg), len(self.rows), C, A, ptr(pg["conv_w"]),
                                           ptr(pg["conv_b"]), ptr(pg["cls_w"]), ptr(pg["cls_b"]), ptr(pg["reg_w"]),
                                           ptr(pg["reg_b"]), ptr(hidden), stream()))
        return obj, reg, hidden

    def backward(self, hidden, null_obj=False, null_reg=False, zero_obj=False, zero_reg=False):
        from _hip import check, ptr, stream
        lib = _lib()
        C, A, G, pd = self.C, self.A, self.G, self.pd
        d_f = [torch.full((n, C), NAN, device=DEV) for n in self.rows]
        grads = {k: torch.full(tuple(v.shape), NAN, device=DEV) for k, v in pd.items()}
        floats = lib.aabr_rpn_head_grouped_scratch_floats(self.tiles, C, A, G)
        scr = torch.full((max(floats, 1),), NAN, device=DEV)
        go = None if null_obj else [torch.zeros_like(g) for g in self.god] if zero_obj else self.god
        gr = None if null_reg else [torch.zeros_like(g) for g in self.grd] if zero_reg else self.grd
        check(lib.aabr_rpn_head_grouped_backward(_table(self.fd, self.rows, go, gr, d_f), len(self.rows), C, A, G,
                                                 ptr(pd["conv_w"]), ptr(pd["cls_w"]), ptr(pd["reg_w"]), ptr(hidden),
                                                 ptr(grads["conv_w"]), ptr(grads["conv_b"]), ptr(grads["cls_w"]),
                                                 ptr(grads["cls_b"]), ptr(grads["reg_w"]), ptr(grads["reg_b"]), ptr(scr),
                                                 stream()))
        return d_f, grads

    def check_against_definition(self):
        """forward, the mask, and all gradients; returns the device outputs"""
        A, G = self.A, self.G
        obj, reg, hidden = self.forward()
        f_all = np.concatenate(self.f)
        fwd = R.forward(f_all, self.p)
        t_dev = hidden.cpu().numpy()
        _ok("objectness " + self.tag, torch.cat(obj, 1).cpu().numpy(), GR.v_to_groups(fwd["obj"], A, G, 1))
        _ok("box regression " + self.tag, torch.cat(reg, 1).cpu().numpy(), GR.v_to_groups(fwd["reg"], A, G, 7))
        _ok("hidden " + self.tag, t_dev, fwd["t"])
        und = R.undecided(fwd)
        share = float(und.mean()) if und.size else 0.0
        print("undecidable hidden units: %d of %d" % (int(und.sum()), und.size))
        assert share < R.MAX_UNDECIDED
        assert (((t_dev > 0) == (fwd["pre"].v > 0)) | und).all()                 # the mask, outside the undecidable units
        d_f, grads = self.backward(hidden)
        bwd = GR.backward(f_all, self.p, np.concatenate(self.g_obj), np.concatenate(self.g_reg), t_dev, fwd, A, G)
        d_all = torch.cat(d_f).cpu().numpy()
        assert not np.isnan(d_all).any()                                       # every d_f element is written
        _ok("d_f " + self.tag, d_all, bwd["d_f"])
        for k in self.p:
            _ok("d_%s %s" % (k, self.tag), grads[k].cpu().numpy(), bwd["d_" + k])
        return obj, reg, hidden, d_f, grads


# ------------------------------------------------------------------------------------------------ 1 and 2
def test_entry_points_against_the_definition_and_the_plain_head_on_sliced_weights():
    T = _lib().aabr_rpn_head_tile_rows(128)
    for C, A, G, rows, seed in GR.entry_cases(T):
        run = _Run(C, A, G, rows, seed)
        obj, reg, hidden, _, _ = run.check_against_definition()
        for g in range(G):
            po, pr, ph = run.plain_forward(g)
            assert _bits([ph]) == _bits([hidden]), (run.tag, g)
            assert _bits(po) == _bits([o[g] for o in obj]), (run.tag, g)
            assert _bits(pr) == _bits([r[g] for r in reg]), (run.tag, g)


# ------------------------------------------------------------------------------------------------ 3
def test_outputs_do_not_depend_on_storing_the_hidden_activation():
    T = _lib().aabr_rpn_head_tile_rows(128)
    for C, A, G, rows, seed in GR.hidden_cases(T):
        run = _Run(C, A, G, rows, seed)
        o1, r1, hidden, _, _ = run.check_against_definition()
        o0, r0, none = run.forward(with_hidden=False)
        assert none is None and _bits(o0 + r0) == _bits(o1 + r1)
        assert not torch.isnan(hidden).any()


def test_more_tiles_than_workgroups_and_a_single_tile_are_deterministic():
    lib = _lib()
    T, gmax = lib.aabr_rpn_head_tile_rows(32), lib.aabr_rpn_head_groups(2 ** 40)
    many, one = [_Run(*c) for c in GR.determinism_cases(T, gmax)]
    assert many.tiles == gmax + 1 == 257 and lib.aabr_rpn_head_groups(many.tiles) == gmax
    assert one.tiles == 1
    for run in (many, one):
        o, r, hidden, d_f, grads = run.check_against_definition()
        o2, r2, h2 = run.forward()
        d_f2, grads2 = run.backward(hidden)
        assert _bits(o + r + [hidden]) == _bits(o2 + r2 + [h2])
        assert _bits(d_f) == _bits(d_f2)
        assert all(_bits([grads[k]]) == _bits([grads2[k]]) for k in grads)


# ------------------------------------------------------------------------------------------------ 4 and all maps empty
def test_null_gradients_equal_zeros_bit_for_bit():
    T = _lib().aabr_rpn_head_tile_rows(32)
    run = _Run(32, 2, 3, (T + 3, 0, 2), 7)
    _, _, hidden = run.forward()
    for kw_null, kw_zero in (({"null_obj": True}, {"zero_obj": True}), ({"null_reg": True}, {"zero_reg": True}),
                             ({"null_obj": True, "null_reg": True}, {"zero_obj": True, "zero_reg": True})):
        d_n, g_n = run.backward(hidden, **kw_null)
        d_z, g_z = run.backward(hidden, **kw_zero)
        assert _bits(d_n) == _bits(d_z) and not np.isnan(torch.cat(d_n).cpu().numpy()).any()
        assert all(_bits([g_n[k]]) == _bits([g_z[k]]) for k in g_n)
        assert not any(torch.isnan(v).any() for v in g_n.values())
    d, g = run.backward(hidden, null_obj=True, null_reg=True)
    assert not torch.cat(d).any() and not any(v.any() for v in g.values())


def test_all_maps_empty_launch_nothing_and_zero_the_weight_gradients():
    run = _Run(64, 4, 3, (0, 0), 8)
    obj, reg, hidden = run.forward()
    assert all(o.numel() == 0 for o in obj + reg)
    _, grads = run.backward(hidden)
    assert all(not v.any() and not torch.isnan(v).any() for v in grads.values())


# ------------------------------------------------------------------------------------------------ 5
def _head(C, A, G, p):
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    names = ["c%d" % i for i in range(G - 1)]
    cfg = rpn_glue.rpn_cfg(C=C, separate=names, separate_ids=[[i + 1] for i in range(G - 1)],
                           classes=["background"] + names)
    head = RPNHead(cfg, C, A).to(DEV)
    with torch.no_grad():
        for mod, k in ((head.conv, "conv"), (head.cls_logits, "cls"), (head.bbox_pred, "reg")):
            mod.weight.copy_(_t(p[k + "_w"]).view_as(mod.weight))
            mod.bias.copy_(_t(p[k + "_b"]))
    return head


def test_glue_autograd_against_the_unfused_module():
    C, A, G, rows = 64, 4, 3, (70, 0, 9)
    p, f, g_obj, g_reg = GR.make_case(C, A, G, rows, 9)
    head = _head(C, A, G, p)
    assert head.seperate_rpn == G
    go = [_t(g).view(1, n, A, G) for g, n in zip(g_obj, rows)]                   # the reference's shapes: packed order
    gr = [_t(g).view(1, n, A, 7 * G) for g, n in zip(g_reg, rows)]

    def run(fused):
        head.fused = fused
        head.zero_grad()
        leaves = [_t(x).requires_grad_(True) for x in f]
        logits, bbox = head(leaves)
        assert all(tuple(l.shape) == (1, n, A, G) and tuple(b.shape) == (1, n, A, 7 * G)
                   for l, b, n in zip(logits, bbox, rows))
        loss = sum((l * g).sum() for l, g in zip(logits, go)) + sum((b * g).sum() for b, g in zip(bbox, gr))
        loss.backward()
        grads = [q.grad.clone() for q in head.parameters()] + [x.grad.clone() for x in leaves]
        return [l.detach() for l in logits] + [b.detach() for b in bbox], grads
    out_f, grad_f = run(True)
    out_t, grad_t = run(False)
    assert [tuple(g.shape) for g in grad_f[:6]] == [tuple(q.shape) for q in head.parameters()]
    f_all = np.concatenate(f)
    fwd = R.forward(f_all, p)
    t_def = np.maximum(f_all.astype(np.float64) @ p["conv_w"].astype(np.float64).T + p["conv_b"], 0)
    names = ["conv_w", "conv_b", "cls_w", "cls_b", "reg_w", "reg_b"]
    for tag, outs in (("fused", out_f), ("torch", out_t)):
        _ok(tag + " logits", torch.cat([o.reshape(-1, A * G) for o in outs[:3]]).cpu().numpy(), fwd["obj"])
        _ok(tag + " bbox", torch.cat([o.reshape(-1, 7 * A * G) for o in outs[3:]]).cpu().numpy(), fwd["reg"])
    und = R.undecided(fwd)
    assert und.mean() < R.MAX_UNDECIDED
    if not und.any():                                                            # the masks of both sides are the definition's
        bwd = GR.backward(f_all, p, np.concatenate(g_obj), np.concatenate(g_reg), t_def, fwd, A, G)
        for tag, grads in (("fused", grad_f), ("torch", grad_t)):
            for k, g in zip(names, grads[:6]):
                _ok("%s d_%s" % (tag, k), g.reshape(p[k].shape).cpu().numpy(), bwd["d_" + k])
            _ok(tag + " d_f", torch.cat(grads[6:]).cpu().numpy(), bwd["d_f"])
    # forward_flat: group-major slices of the same values, fused and unfused
    for fused in (True, False):
        head.fused = fused
        with torch.no_grad():
            flat_o, flat_r = head.forward_flat([_t(x) for x in f])
            logits, bbox = head([_t(x) for x in f])
        for o, r, l, b, n in zip(flat_o, flat_r, logits, bbox, rows):
            assert tuple(o.shape) == (G, n * A) and tuple(r.shape) == (G, n * A, 7)
            for g in range(G):
                assert torch.equal(o[g], l[0, :, :, g].reshape(-1))
                assert torch.equal(r[g], b[0, :, :, 7 * g:7 * g + 7].reshape(-1, 7))
    head.fused = True
    with torch.no_grad():                                                        # no gradient required: the same bits
        logits, bbox = head([_t(x) for x in f])
    assert _bits(logits + bbox) == _bits(out_f)


# ------------------------------------------------------------------------------------------------ 6
def test_head_forward_and_backward_enqueue_without_a_host_read():
    import rpn_glue
    C, A, G, rows = 32, 2, 3, (130, 0, 5)
    p, f, g_obj, g_reg = GR.make_case(C, A, G, rows, 12)
    pd = {k: _t(v).requires_grad_(True) for k, v in p.items()}
    fd = [_t(x).requires_grad_(True) for x in f]
    go = [_t(GR.to_groups(g, A, G, 1)).reshape(G, -1) for g in g_obj]
    gr = [_t(GR.to_groups(g, A, G, 7)).reshape(G, -1, 7) for g in g_reg]

    def run():
        for q in list(pd.values()) + fd:
            q.grad = None
        obj, reg = rpn_glue.rpn_head_grouped(fd, pd["conv_w"], pd["conv_b"], pd["cls_w"], pd["cls_b"], pd["reg_w"],
                                             pd["reg_b"], G)
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
