"""The proposal stage's selection and suppression where their suite did not reach (csrc/iou_nms.hip aabr_rpn_topk_maps,
csrc/nms_shared.h nms_scan_block): logits that are NaN (both sign bits), infinite, +-0, denormal or spread over 60 decades;
cuts on the edges of the two 12-bit histograms and of topk_find_bin's 16-bin thread groups; 4096 / 4097 candidates for the
4096-entry buffer; a list longer than the capped grid walks in 8 steps; the full 16-example x 8-map table; and NMS lists
of 34 and more column blocks, where a kept row's suppression words beyond the 32 prefetched ones come from the scan's far
loop.  The definitions and inputs are tests/proposal_ref.py (plain numpy); tests/test_proposal_ref_host.py checks without
a GPU that every input reaches its edge.

Every device call goes through the C ABI; every output buffer is pre-filled with a sentinel and has 64 guard elements on
either side, checked after the call; a second call must be bit-equal to the first.  Every comparison is exact: indices,
flags, torch.equal.

What these tests found (MI355X).  With the bare float_order_key as the top-k's key the special-value, signed-zero and
all-NaN cases, the histogram sweeps whose cut lies in the zeros, and the glue test failed: a NaN with the sign bit set
ranked below -inf, a +0 before a -0 of lower index.  The three ranking passes now share topk_order_key.  The glue test
then still failed on the torch.topk paths: on the device torch.topk selects a NaN whatever its sign bit but sorts one with
the sign bit set last among the selected, so those paths now hand it float('nan') for every NaN (rpn_glue logits_of,
aabr_rpn_gather_logits).  The scan's far loop, the bin search, the candidate buffer and the capped grid were right."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import proposal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.int64: -77, torch.int32: 0x5a5a5a5a}
CASES = R.topk_cases()


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Guarded(object):
    def __init__(self, n, dtype):
        self.n, self.fill = n, SENTINEL[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 8 == 0 and (GUARD * self.buf.element_size()) % 8 == 0
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        self.body = self.buf[GUARD:GUARD + n]

    def check(self, name):
        assert (self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.n:] == self.fill).all(), name + ": guard"


# ---------------------------------------------------------------- selection
def _upload(arrays):
    """logit buffers in device memory, the same bits as on the host (NaN sign bits and payloads, -0, denormals)"""
    out = [_t(m) for m in arrays]
    for m, d in zip(arrays, out):
        assert np.array_equal(d.view(torch.int32).cpu().numpy().view(np.uint32), R.bits_of(m))
    return out


def _topk_call(case, maps):
    """one aabr_rpn_topk_maps call over the whole case: (selected [nb, stride], info [nb, 2], scratch)"""
    import _hip
    lib = _hip.load()
    stride = max(max(case.ks), 1) + 3                           # rows do not touch
    sel = _Guarded(case.nb * stride, torch.int64)
    info = _Guarded(case.nb * 2, torch.int32)
    scr = _Guarded(int(lib.aabr_rpn_topk_scratch_words(case.nb)), torch.int32)
    _hip.check(lib.aabr_rpn_topk_maps(case.n_maps, _hip.ptrs(maps), case.nb, _hip.i32xn([v for s in case.seg for v in s]),
                                      _hip.i32xn([v for s in case.site for v in s]), case.A, _hip.i32xn(case.ks), sel.ptr,
                                      stride, info.ptr, scr.ptr, _hip.stream()))
    torch.cuda.synchronize()
    for name, g in (("selected", sel), ("info", info), ("scratch", scr)):
        g.check("%s: %s" % (case.name, name))
    return sel.body.view(case.nb, stride), info.body.view(case.nb, 2), scr.body


def _run_topk(case, overflow=()):
    """the call twice (bit-equal), then every example against the definition: selected[b][:k] index for index, nothing
    written past k, no overflow flag, the documented number of candidates -- or, for the examples in `overflow`, the flag and every
    entry inside the list"""
    maps = _upload(case.maps)
    sel, info, scr = _topk_call(case, maps)
    sel2, info2, _ = _topk_call(case, maps)
    assert torch.equal(info, info2), case.name
    sel_h, info_h = sel.cpu().numpy(), info.cpu().numpy()
    for b in range(case.nb):
        k = case.ks[b]
        assert (sel_h[b, k:] == SENTINEL[torch.int64]).all(), (case.name, b, "written past k")
        if b in overflow:
            assert info_h[b, 1] == 1, (case.name, b)
            assert ((sel_h[b, :k] >= 0) & (sel_h[b, :k] < case.n(b))).all(), (case.name, b)
            continue
        assert torch.equal(sel[b], sel2[b]), (case.name, b)
        # info[2b]: the logits whose 24-bit key prefix is at or above the k-th logit's, as the header documents it
        assert info_h[b].tolist() == [R.candidate_count(case.logits(b), k), 0], (case.name, b, info_h[b].tolist())
        np.testing.assert_array_equal(sel_h[b, :k], case.expected(b), err_msg="%s[%d], k = %d" % (case.name, b, k))
    return sel_h, info_h


def test_topk_special_values():
    """NaN of either sign bit above +inf, both by ascending index; infinities, zeros, denormals and 60 decades of
    magnitudes in their value order; k = 1 / 50 / 600 / 2048 over 3 maps with 2 anchors per site"""
    case = CASES["special"]
    sel, _ = _run_topk(case)
    v = case.logits(0)
    assert R.bits_of(v[sel[0, :1]])[0] == R.NAN_NEG and np.isnan(v[sel[1, :48]]).all() and np.isposinf(v[sel[2, 48:72]]).all()


def test_topk_signed_zeros_at_the_cut():
    """-0 and +0 compare equal: inside the run of zeros the cut takes them by ascending index, whatever their sign"""
    _run_topk(CASES["signed_zeros"])


def test_topk_all_nan_and_all_minus_infinity():
    """3,000 equal keys fit the candidate buffer: indices 0 .. 1999 in order, no overflow"""
    case = CASES["uniform"]
    sel, info = _run_topk(case)
    for b in (0, 1):
        assert sel[b, :2000].tolist() == list(range(2000)) and info[b].tolist() == [3000, 0]


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("hist_")))
def test_topk_cuts_on_histogram_bin_edges(name):
    """k = P and P + 1 for every prefix sum P <= 2047 of the level-1 bins, 16 k per call: the cut is the last element of
    a bin, then the first of the next; first and last bins of topk_find_bin's 16-bin groups, both sides of zero"""
    _run_topk(CASES[name])


def test_topk_candidate_buffer_boundary():
    """4096 candidates fit (and are sorted: the selection equals the definition), 4097 raise the flag"""
    case = CASES["boundary"]
    _, info = _run_topk(case, overflow=(1,))
    assert info[0].tolist() == [4096, 0] and info[1].tolist() == [4097, 1]


def test_topk_list_longer_than_the_capped_grid():
    _run_topk(CASES["grid_cap"])


def test_topk_smallest_and_largest_sizes():
    """n = 1, k = n, k = 0 with n > 0, k = n = 2048, over aliased rows of one buffer"""
    _run_topk(CASES["sizes"])


def test_topk_sixteen_examples_by_eight_maps():
    """the real layout: empty maps, one-logit maps, an example empty in every map between two full ones"""
    _run_topk(CASES["ragged"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_glue_selects_alike_on_all_three_paths():
    """rpn_glue.rpn_proposals over objectness with both NaN sign bits and both zeros inside the top k (no two selected
    logits equal): the boxes and scores handed to NMS, and the proposals, are the same bits with the fused top-k, with
    torch.topk per example and with the batched torch.topk"""
    import sparseconvnet as scn
    import rpn_glue
    s = R.GlueScene()
    maps = []
    for coords, sp in zip(s.coords, s.SPATIAL):
        x = scn.InputLayer(3, list(sp), mode=3)([_t(coords), _t(np.zeros((coords.shape[0], 1), np.float32))])
        sc = x.get_spatial_locations().numpy()
        assert sc.shape == coords.shape and (np.diff(sc[:, 3]) >= 0).all()
        assert [int((sc[:, 3] == b).sum()) for b in (0, 1)] == [int((coords[:, 3] == b).sum()) for b in (0, 1)]
        maps.append(x)
    obj = _upload(s.obj)
    reg = [_t(r) for r in s.reg]
    args = (maps, obj, reg, [torch.as_tensor(b) for b in s.base], list(s.STRIDES), 20.0, s.K, s.POST, 0.5, (0.3, 0.3),
            (1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5), 10000.0)
    seen, out = {}, {}
    assert rpn_glue.debug_nms_inputs is None and rpn_glue.fused_topk is True
    f0 = rpn_glue.topk_stats["fallbacks"]
    try:
        for path, fused, kw in (("fused", True, {}), ("torch", False, {}), ("batched", True, {"batched": True})):
            rpn_glue.fused_topk = fused
            rpn_glue.debug_nms_inputs = seen[path] = []
            out[path] = rpn_glue.rpn_proposals(*args, batch_size=2, **kw)
    finally:
        rpn_glue.fused_topk = True
        rpn_glue.debug_nms_inputs = None
    assert rpn_glue.topk_stats["fallbacks"] == f0
    for path in ("fused", "torch", "batched"):
        assert len(seen[path]) == len(out[path]) == 2
        for b in (0, 1):
            boxes, scores = seen[path][b]
            assert boxes.shape == (s.K, 7) and scores.shape == (s.K,)
            print("%s[%d]: NaN scores at %s, first scores %s" % (path, b, torch.isnan(scores).nonzero().flatten().tolist(),
                                                                 scores[:3].tolist()))
            assert bool(torch.isnan(scores[0])) and not bool(torch.isnan(scores[1:]).any())       # the NaN logit leads
            assert (scores[1:] == 0.5).sum() == 1                                                  # the zero is inside
            assert torch.equal(_bits(boxes), _bits(seen["fused"][b][0])), (path, b)
            assert torch.equal(_bits(scores), _bits(seen["fused"][b][1])), (path, b)
            assert out[path][b][0].shape[0] > 10
            assert torch.equal(_bits(out[path][b][0]), _bits(out["fused"][b][0])), (path, b)
            assert torch.equal(_bits(out[path][b][1]), _bits(out["fused"][b][1])), (path, b)


# ---------------------------------------------------------------- suppression
def _nms_call(kind, boxes, thr, post):
    """aabr_rotate_nms_sorted (kind 0) / aabr_nms_sorted (kind 1) on a sorted list in device memory: (keep, meta, mask)"""
    import _hip
    lib = _hip.load()
    n = boxes.shape[0]
    cb = (n + 63) // 64
    mask, keep, meta = _Guarded(n * cb, torch.int64), _Guarded(n, torch.int64), _Guarded(_hip.META_WORDS, torch.int32)
    if kind == 0:
        _hip.check(lib.aabr_rotate_nms_sorted(_hip.ptr(boxes), n, float(thr), 1, int(post), mask.ptr, keep.ptr, meta.ptr,
                                              _hip.stream()))
    else:
        _hip.check(lib.aabr_nms_sorted(_hip.ptr(boxes), n, float(thr), mask.ptr, keep.ptr, meta.ptr, _hip.stream()))
    torch.cuda.synchronize()
    for name, g in (("mask", mask), ("keep", keep), ("meta", meta)):
        g.check(name)
    assert not (mask.body == SENTINEL[torch.int64]).any()             # every word of the mask is written
    return keep.body, meta.body, mask.body


def _check_nms(kind, boxes, thr, post, want):
    d = _t(boxes)
    keep, meta, mask = _nms_call(kind, d, thr, post)
    keep2, meta2, mask2 = _nms_call(kind, d, thr, post)
    assert torch.equal(keep, keep2) and torch.equal(meta, meta2) and torch.equal(mask, mask2)
    nk = int(meta[0].item())
    assert nk == len(want) and (meta[1:] == 0).all()
    np.testing.assert_array_equal(keep[:nk].cpu().numpy(), want)
    assert (keep[nk:] == SENTINEL[torch.int64]).all()                 # nothing written past the kept positions
    return keep[:nk]


@pytest.fixture(scope="module")
def rotated_inputs():
    return dict(((n, seed), R.nms_rotated_inputs(n, seed)) for _, n, seed, _, _, _ in R.NMS_ROTATED)


@pytest.mark.parametrize("name,n,seed,thr,post,far", R.NMS_ROTATED)
def test_rotated_nms_scan_past_33_column_blocks(rotated_inputs, name, n, seed, thr, post, far):
    """the keep list of the oracle (Sutherland-Hodgman decision, its own pre-filter) position for position; no pair of
    these lists lies within 1e-9 of the threshold (host test), so there is nothing to be lenient about"""
    import _nms
    b, sc = rotated_inputs[(n, seed)]
    want = O.rotate_nms_3d(b, sc, None, post, thr)
    got = _check_nms(0, b, thr, post, want)
    assert torch.equal(_nms.rotate_nms_sorted(_t(b), thr, post), got)            # the wrapper every caller goes through


def test_axis_aligned_nms_scan_past_33_column_blocks():
    n, _, thr = R.NMS_AXIS
    d, sc = R.nms_axis_inputs()
    import _nms
    got = _check_nms(1, d, thr, n, O.nms_axis_aligned(d, sc, thr))
    assert torch.equal(_nms.nms_sorted(_t(d), thr), got)
