"""k_rpn_label_maps (csrc/iou_nms.hip) where its suite did not reach: more than one ground-truth chunk (kLabelTgtChunk =
128), exact ties between ground truths and between anchors, row maxima of +-0, thresholds equal to attained values,
lists of 255 / 256 / 257 anchors, 16 ragged examples in one call, 17 through the glue, the z factor (only_xy off),
criterion -1, and NaN entries.  Everything goes through the C ABI (aabr_rpn_label_generation_targets) on hand-built site
lists; the definition is tests/label_ref.py (plain numpy, nothing of the package), the conditions every case has to
meet are checked without a GPU in tests/test_label_ref_host.py.

Per call: every output buffer is pre-filled with a sentinel and has 64 guard elements on either side; per example the
matrix against the definition (criterion 6 with only_xy: at most 1 fp32 ulp, the entries that are not bit-equal are
counted and printed; z factor: the bound derived in label_ref; criterion -1: 2e-5 against the C oracle), labels and
matched values EXACTLY the reference Matcher's (oracle/box_oracle.py, pinned by matcher_golden.npz) on the device's own
matrix, regression targets torch.equal to BoxCoder3D.encode on the materialised anchors, the call without the matrix
and a second call bit-equal to the first."""
import numpy as np
import pytest
import torch

import label_ref as L
import oracle_lib as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.int64: -77, torch.float32: -12345.5, torch.int32: 0x5a5a5a5a}
STATS = {"entries": 0, "not_bit_equal": 0}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _OnDevice(object):
    """a case's inputs in device memory"""

    def __init__(self, case, coords=None):
        self.case = case
        self.coords = coords if coords is not None else [_t(m[0]) for m in case.maps]
        self.base = _t(np.concatenate([m[2] for m in case.maps], 0))
        self.strides = [v for m in case.maps for v in m[1]]
        self.targets = [_t(t) for t in case.targets]


class _Guarded(object):
    def __init__(self, n, dtype):
        self.n, self.fill = n, SENTINEL[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        self.body = self.buf[GUARD:GUARD + n]

    def check(self, name, all_written=True):
        assert (self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.n:] == self.fill).all(), name + ": guard"
        assert not all_written or not (self.body == self.fill).any(), name + ": an element was not written"


def _call(dev, b0, b1, allow, ythr, fg, bg, matrix=True):
    """one library call for examples b0 .. b1 - 1; returns per example (idx, vals, matrix or None, regression targets)"""
    import _hip
    import rpn_glue
    case, lib = dev.case, _hip.load()
    seg, site, n_anch = rpn_glue._anchor_tables(case.counts, case.A, b0, b1)
    n_gt = [len(case.targets[b]) for b in range(b0, b1)]
    total = sum(n_anch)
    idx, val = _Guarded(total, torch.int64), _Guarded(total, torch.float32)
    reg = _Guarded(total * 7, torch.float32)
    mat = _Guarded(sum(n * g for n, g in zip(n_anch, n_gt)), torch.float32) if matrix else None
    row = _Guarded(sum(n_gt), torch.int32) if allow else None
    _hip.check(lib.aabr_rpn_label_generation_targets(
        len(case.maps), _hip.ptrs(dev.coords), b1 - b0, _hip.i32xn(seg), _hip.i32xn(site), _hip.f32xn(dev.strides),
        _hip.ptr(dev.base), case.A, float(L.VOXEL_SCALE), _hip.ptrs(dev.targets[b0:b1]), _hip.i32xn(n_gt),
        _hip.f32x4(case.aug), case.criterion, case.only_xy, float(fg), float(bg), float(ythr), int(allow), idx.ptr, val.ptr,
        mat.ptr if matrix else None, row.ptr if allow else None, _hip.f32xn(case.weights), reg.ptr, _hip.stream()))
    torch.cuda.synchronize()
    for name, g in (("matched_idx", idx), ("matched_val", val), ("regression_targets", reg), ("matrix", mat)):
        if g is not None:
            g.check(name)
    if row is not None:
        row.check("row-maximum scratch", all_written=False)
    out, o, mo = [], 0, 0
    for n, g in zip(n_anch, n_gt):
        out.append((idx.body[o:o + n], val.body[o:o + n], mat.body[mo:mo + g * n].view(g, n) if matrix else None,
                    reg.body[7 * o:7 * (o + n)].view(n, 7)))
        o += n
        mo += g * n
    return out


def _same(x, y):
    """bit-equal outputs of two calls (NaN payloads included)"""
    return all((a is None and b is None) or torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                        b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(x, y))


def _equal_nan(a, b):
    return bool((torch.isnan(a) == torch.isnan(b)).all() and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)))


def _check_example(case, b, out, allow, ythr, fg, bg, nan_targets=False):
    """one example's outputs against the definition"""
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    an, tg = L.anchors(case, b), case.targets[b]
    idx, val, mat, reg = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(), out[3]
    N, G = an.shape[0], tg.shape[0]
    assert idx.shape == (N,) and val.shape == (N,) and mat.shape == (G, N) and reg.shape == (N, 7)
    coder = BoxCoder3D(False, case.weights)
    if N == 0:
        return
    if G == 0:                # no ground truth: background, the anchors encoded against themselves (loss_3d.py:91-94)
        assert (idx == -1).all() and (val == 0).all()
        assert torch.equal(reg, coder.encode(_t(an), _t(an)))
        return
    ref = L.matrix(case, b)
    if ref["ref32"] is not None:
        d = L.ulp_distance(mat, ref["ref32"])
        STATS["entries"] += d.size
        STATS["not_bit_equal"] += int((d != 0).sum())
        assert d.max() <= 1, "%s[%d]: %d entries beyond 1 ulp, worst %d" % (case.name, b, (d > 1).sum(), d.max())
    elif case.criterion == 6:
        nan = np.isnan(ref["ref"])
        assert np.array_equal(np.isnan(mat), nan)
        err = np.abs(mat.astype(np.float64) - ref["ref"])
        print("%s[%d]: z factor, worst error / bound %.3f" % (case.name, b, (err[~nan] / np.maximum(ref["bound"][~nan], 1e-300)).max()))
        assert (err[~nan] <= ref["bound"][~nan]).all()
    else:
        want = O.boxes_iou_3d(tg, an, case.aug, case.criterion, bool(case.only_xy))
        print("%s[%d]: criterion %d, worst |device - oracle| %.3g" % (case.name, b, case.criterion, np.abs(mat - want).max()))
        np.testing.assert_allclose(mat, want, atol=2e-5, rtol=0)
    with np.errstate(invalid="ignore"):
        lab, mv = L.labels(mat, tg, an, fg, bg, allow, ythr)               # the reference's Matcher on the device's matrix
    np.testing.assert_array_equal(val, mv)
    np.testing.assert_array_equal(idx, lab)
    for _, later in case.duplicates:
        assert not (idx == later).any()
    want = coder.encode(_t(tg)[out[0].clamp(min=0)], _t(an))
    assert _equal_nan(reg, want) if nan_targets else torch.equal(reg, want)


def _check_call(dev, b0, b1, allow, ythr, fg=None, bg=None, nan_targets=False):
    """the call with the matrix against the definition; the call without it and a second call bit-equal to it"""
    case = dev.case
    fg, bg = case.fg if fg is None else fg, case.bg if bg is None else bg
    full = _call(dev, b0, b1, allow, ythr, fg, bg)
    lean = _call(dev, b0, b1, allow, ythr, fg, bg, matrix=False)
    again = _call(dev, b0, b1, allow, ythr, fg, bg)
    for i, b in enumerate(range(b0, b1)):
        _check_example(case, b, full[i], allow, ythr, fg, bg, nan_targets)
        assert lean[i][2] is None and _same(lean[i][:2] + lean[i][3:], full[i][:2] + full[i][3:]), (case.name, b)
        assert _same(again[i], full[i]), (case.name, b)
    print("%s: criterion-6 entries compared so far %d, not bit-equal %d" % (case.name, STATS["entries"], STATS["not_bit_equal"]))
    return full


@pytest.fixture(scope="module")
def on_device():
    return {name: _OnDevice(case) for name, case in L.cases().items()}


@pytest.mark.parametrize("allow", [True, False])
@pytest.mark.parametrize("G", L.CHUNK_G)
def test_chunk_edges(on_device, G, allow):
    """204 anchors against 1 / 127 / 128 / 129 / 256 / 257 ground truths: one chunk, a full one, one box into the second,
    two full ones, one box into the third.  Boxes 200 and 128 copy boxes 5 and 127: never a label."""
    dev = on_device["chunk_G%d" % G]
    out = _check_call(dev, 0, 1, allow, 0.7)
    idx = out[0][0].cpu().numpy()
    for first, later in dev.case.duplicates:
        assert (idx == first).any() and not (idx == later).any()
    assert G < 256 or (idx >= 128).any()


@pytest.mark.parametrize("name", ["ragged_a", "ragged_b"])
def test_sixteen_ragged_examples_in_one_call(on_device, name):
    """(N, G) from (4, 129) over (0, 3) and (1100, 0) to (1100, 257), lists of 255 / 256 / 257 anchors, a map empty for
    one example, an example empty in every map: gt_begin, out_begin and iou_begin all irregular"""
    _check_call(on_device[name], 0, 16, True, 0.7)
    _check_call(on_device[name], 0, 16, False, 3.0)


def test_seventeen_examples_through_the_glue(on_device):
    """nb > 16: rpn_glue.rpn_label_matches makes two library calls and stitches them; every example's tuple must equal
    the one of a single-example call, and the definition"""
    import sparseconvnet as scn
    import rpn_glue
    case = L.cases()["batch17"]
    extents = ((20, 12, 2), (8, 8, 2))
    maps, new_maps = [], []
    for (coords, stride, base), ext in zip(case.maps, extents):
        x = scn.InputLayer(3, list(ext), mode=3)([_t(coords.astype(np.int64)), _t(np.zeros((coords.shape[0], 1), np.float32))])
        sc = x.get_spatial_locations().numpy()
        assert (np.diff(sc[:, 3]) >= 0).all() and sc.shape == coords.shape
        maps.append(x)
        new_maps.append((sc.astype(np.int32), stride, base))
    counts = [[int((m[0][:, 3] == b).sum()) for b in range(case.nb)] for m in new_maps]
    assert counts == case.counts                    # the same sites per example, in the grid's row order
    grid_case = L.Case("batch17_grid", new_maps, counts, case.targets, weights=case.weights)
    dev = _OnDevice(grid_case)
    aug = dict(zip(("target_Y", "target_Z", "anchor_Y", "anchor_Z"), L.LABEL_AUG))
    for allow in (True, False):
        res = rpn_glue.rpn_label_matches(maps, [torch.as_tensor(m[2]) for m in new_maps], [m[1] for m in new_maps],
                                         L.VOXEL_SCALE, dev.targets, aug, 6, return_matrix=True, allow_low_quality_matches=allow,
                                         regression_targets=True, weights=case.weights)
        assert len(res) == 17
        for b in range(17):
            single = _call(dev, b, b + 1, allow, 0.7, 0.55, 0.2)[0]
            assert _same(res[b], single), b
            _check_example(grid_case, b, res[b], allow, 0.7, 0.55, 0.2)


@pytest.mark.parametrize("allow", [False, True])
def test_thresholds_on_attained_values(on_device, allow):
    """fg_iou and bg_iou are two values read from the device's own best values: `<` is strict on both, an anchor whose
    best equals fg is matched, one whose best equals bg lies between the thresholds"""
    dev = on_device["chunk_G129"]
    vals = _call(dev, 0, 1, False, 0.7, 0.55, 0.2)[0][1].cpu().numpy()
    fg, bg = L.attained_thresholds(vals)
    assert (vals == np.float32(fg)).any() and (vals == np.float32(bg)).any() and bg < fg
    out = _check_call(dev, 0, 1, allow, 0.7, fg, bg)
    idx, val = out[0][0].cpu().numpy(), out[0][1].cpu().numpy()
    assert (idx[val == np.float32(fg)] >= 0).all()
    if not allow:
        assert (idx[val == np.float32(bg)] == -2).all()
    else:
        assert (idx[val == np.float32(bg)] != -1).all()          # -2, or matched by the low-quality pass


@pytest.mark.parametrize("ythr,allow", [(0.7, True), (0.7, False), (3.0, True), (3.0, False)])
def test_yaw_mask(on_device, ythr, allow):
    """ground-truth yaws 3.0 and -2.5, one ground truth masked against every anchor (its row maximum is +-0 and every
    anchor ties with it), and yaw_threshold 3.0 = no mask"""
    out = _check_call(on_device["yaw"], 0, 1, allow, ythr)
    if ythr == 0.7 and allow:
        assert (out[0][0] >= 0).all()


@pytest.mark.parametrize("name", ["z_clamped", "z_plain"])
def test_z_factor(on_device, name):
    """only_xy off: overlapping, touching and disjoint z intervals (a negative factor), clamps on and at 0"""
    _check_call(on_device[name], 0, 1, True, 0.7)
    _check_call(on_device[name], 0, 1, False, 3.0)


def test_criterion_minus_one(on_device):
    """the rotated IoU itself, 2e-5 against the C oracle; labels exactly the Matcher's on the device's matrix, and equal to
    the Matcher's on the oracle's matrix unless a value lies within rounding distance of a decision"""
    dev = on_device["iou"]
    case = dev.case
    _check_call(dev, 0, 1, True, 0.7)
    out = _check_call(dev, 0, 1, False, 0.7)
    an, tg = L.anchors(case, 0), case.targets[0]
    idx = out[0][0].cpu().numpy()
    assert {-2, -1} <= set(idx.tolist()) and (idx >= 0).any()
    want = O.boxes_iou_3d(tg, an, case.aug, -1, True)
    lab, vals = L.labels(want, tg, an, case.fg, case.bg, False, 0.7)
    differ = np.nonzero(lab != idx)[0]
    mm = L.masked(want, tg, an, 0.7)
    for n in differ:                                          # razor edge: a threshold, or the two best ground truths
        top = np.sort(mm[:, n])[::-1]
        gap = top[0] - top[1] if len(top) > 1 else np.inf
        assert abs(vals[n] - case.fg) < 2e-5 or abs(vals[n] - case.bg) < 2e-5 or gap < 4e-5, (n, vals[n], gap)


@pytest.mark.parametrize("allow", [True, False])
def test_nan_entries(on_device, allow):
    """0 / 0 in the z factor (a zero-height ground truth at the z of zero-height anchors): as in torch.max a NaN wins,
    the first one by index, matched_val is NaN and the anchor is matched; a NaN row maximum ties with nothing.  (The
    anchors' zero height also puts NaN and inf into the regression targets: compared with NaN == NaN.)"""
    dev = on_device["nan"]
    out = _check_call(dev, 0, 1, allow, 0.7, nan_targets=True)
    idx, val, mat = [t.cpu().numpy() for t in out[0][:3]]
    nan = np.isnan(mat)
    assert nan.any() and np.array_equal(np.isnan(val), nan.any(0))
    assert (idx[nan[1]] == 1).all() and (idx[nan[4] & ~nan[1]] == 4).all()
