"""tests/proposal_ref.py without a GPU: every input of tests/test_gpu_proposal_limits.py checked for what its name claims
-- the special values are there bit for bit, the cuts fall where the kernel's histograms and candidate buffer have their
edges, the NMS lists hold boxes that only the scan's far loop can suppress and no pair stands on the threshold -- so an
input that does not reach its edge fails here, before a GPU is used."""
import numpy as np
import pytest

import oracle_lib as O
import proposal_ref as R

CASES = R.topk_cases()


def _rank_key(v):
    """what two logits must share to be equal in the order: NaN with NaN, -0 with +0"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        val = np.where(np.isposinf(v), 1e300, v.astype(np.float64))       # +inf below the NaN, above every finite float32
    return np.where(np.isnan(v), np.inf, np.where(v == 0, 0.0, val))


def test_topk_order_is_torch_topk_plus_the_index_rule():
    import torch
    v = R.f32_from_bits([0x3F800000, R.NAN_NEG, 0x80000000, 0, 0x7F800000, R.NAN_POS, 0xFF800000, 0x3F800000, 0x80000000])
    assert R.topk_order(v, 9).tolist() == [1, 5, 4, 0, 7, 2, 3, 8, 6]
    assert R.topk_order(v, 3).tolist() == [1, 5, 4] and R.topk_order(v, 0).size == 0
    rng = np.random.default_rng(1)
    w = CASES["special"].logits(0)
    for k in (1, 50, 600, 2048):
        got = w[R.topk_order(w, k)]
        tv = torch.as_tensor(w).topk(k, sorted=True)[0].numpy()
        assert np.array_equal(np.isnan(got), np.isnan(tv)) and np.array_equal(got[~np.isnan(got)], tv[~np.isnan(tv)])
    # the key that places the inputs orders as the definition does, and only ties what the definition ties
    u = rng.permutation(w)[:3000]
    key, order = R.order_key(u), R.topk_order(u, u.size)
    assert (np.diff(key[order].astype(np.int64)) <= 0).all()
    rk = _rank_key(u)[order]
    assert np.array_equal(key[order][1:] == key[order][:-1], rk[1:] == rk[:-1])
    assert R.order_key(R.f32_from_bits([R.NAN_NEG, R.NAN_POS, 0x7FC00001])).tolist() == [0xFFFFFFFF] * 3
    assert R.order_key(R.f32_from_bits([0x80000000])) == R.order_key(R.f32_from_bits([0])) == 0x80000000


def test_every_case_is_a_valid_call():
    for c in CASES.values():
        assert 1 <= c.nb <= 16 and 1 <= c.n_maps <= 8
        for b in range(c.nb):
            assert c.logits(b).size == c.n(b) and 0 <= c.ks[b] <= min(c.n(b), R.K_MAX)
            assert c.expected(b).size == c.ks[b]


def test_special_values_case():
    c = CASES["special"]
    v = c.logits(0)
    assert c.A == 2 and c.n_maps == 3 and v.size == 20000 and c.ks == [1, 50, 600, 2048]
    bits = R.bits_of(v)
    for word in (R.NAN_POS, R.NAN_NEG, 0x7F800000, 0xFF800000, 0, 0x80000000, R.word_of(1e-42),
                 R.word_of(-1e-42)):
        assert (bits == word).sum() == R.SPECIAL_EACH
    den = R.f32_from_bits([R.word_of(1e-42)])
    assert 0 < den[0] < np.finfo(np.float32).tiny
    fin = v[np.isfinite(v) & (v != 0)]
    mag = np.abs(fin[np.abs(fin) > 1e-40]).astype(np.float64)
    assert np.log10(mag.max() / mag.min()) > 55                        # many exponents
    nan = np.nonzero(np.isnan(v))[0]
    assert bits[nan[0]] == R.NAN_NEG                                   # k = 1 selects a NaN with the sign bit set
    for k in c.ks:
        sel = R.topk_order(v, k)
        assert np.isnan(v[sel[:min(k, 48)]]).all() and np.array_equal(sel[:min(k, 48)], nan[:min(k, 48)])
    sel = R.topk_order(v, 600)
    assert np.isposinf(v[sel[48:72]]).all() and np.isfinite(v[sel[72:]]).all()
    # the key of the un-canonical rule (a NaN with the sign bit set at the bottom) selects differently for every k
    raw = np.where(bits & 0x80000000, ~bits, bits | 0x80000000)
    for k in c.ks:
        other = np.lexsort((np.arange(v.size), -raw.astype(np.int64)))[:k]
        assert not np.array_equal(other, R.topk_order(v, k))


def test_signed_zeros_case():
    c = CASES["signed_zeros"]
    v = c.logits(0)
    bits = R.bits_of(v)
    neg0, pos0 = np.nonzero(bits == 0x80000000)[0], np.nonzero(bits == 0)[0]
    assert len(neg0) >= 100 and len(pos0) >= 100 and neg0[0] < pos0[0]
    assert (v > 0).sum() == R.ZEROS_POSITIVE and (v < 0).sum() > v.size // 2
    first, last = R.ZEROS_POSITIVE + 1, R.ZEROS_POSITIVE + len(neg0) + len(pos0)
    inside = [k for k in c.ks if first <= k < last]
    assert len(inside) >= 8 and first in c.ks and last in c.ks and last + 1 in c.ks
    zeros = np.sort(np.concatenate([neg0, pos0]))
    raw = np.where(bits & 0x80000000, ~bits, bits | 0x80000000)
    differ = 0
    for k in inside:
        sel = R.topk_order(v, k)
        assert np.array_equal(sel[R.ZEROS_POSITIVE:], zeros[:k - R.ZEROS_POSITIVE])      # the zeros by index, both signs
        differ += not np.array_equal(sel, np.lexsort((np.arange(v.size), -raw.astype(np.int64)))[:k])
    assert differ == len(inside)                                       # a key with -0 below +0 selects differently


def test_uniform_lists_case():
    c = CASES["uniform"]
    a, b = c.logits(0), c.logits(1)
    assert a.size == b.size == 3000 and np.isnan(a).all() and np.isneginf(b).all() and c.ks == [2000, 2000]
    assert {R.NAN_POS, R.NAN_NEG} <= set(R.bits_of(a).tolist())
    for e in (0, 1):
        assert np.array_equal(c.expected(e), np.arange(2000))
        assert R.candidate_count(c.logits(e), 2000) == 3000 <= R.CAND


def test_histogram_edges_cases():
    v = R.histogram_edges_list()
    cnt = R.bin_counts(v)
    used = np.nonzero(cnt)[0]
    pos_bins, neg_bins = used[used > 0x800], used[used < 0x800]
    assert len(pos_bins) == len(neg_bins) == 64 and cnt[0x800] == 50             # the zeros of both signs share one bin
    assert (np.diff(pos_bins) == 1).all() and (np.diff(neg_bins) == 1).all()
    assert cnt[used].min() >= 15 and len(set(cnt[pos_bins].tolist())) > 5
    for b in used[used != 0x800]:                                      # inside a bin the values differ in the next 12 bits
        nxt = (R.order_key(v[R.prefix12(v) == b]) >> 8) & 4095
        assert len(set(nxt.tolist())) == cnt[b]
    ks = R.histogram_sweep_ks(v)
    cases = [c for name, c in sorted(CASES.items()) if name.startswith("hist_")]
    assert sorted(k for c in cases for k in c.ks) == ks and all(np.array_equal(c.logits(0), v) for c in cases)
    P = np.cumsum(cnt[::-1][cnt[::-1] > 0])
    assert set(P[P <= 2047].tolist()) | set((P[P <= 2047] + 1).tolist()) == set(ks) and max(ks) > 1900
    order = R.topk_order(v, v.size)
    cut_bin = {k: int(R.prefix12(v[order[k - 1:k]])[0]) for k in ks}
    # thread t of topk_find_bin owns bins 4095 - 16 t - 15 .. 4095 - 16 t, top first: bin % 16 == 15 is a group's first
    last_of_bin = [k for k in ks if k in set(P.tolist())]
    first_of_bin = [k for k in ks if k - 1 in set(P.tolist())]
    for group in (last_of_bin, first_of_bin):
        assert {15, 0} <= {cut_bin[k] % 16 for k in group}
    assert any(v[order[k - 1]] < 0 for k in last_of_bin) and any(v[order[k - 1]] < 0 for k in first_of_bin)
    assert any(v[order[k - 1]] == 0 for k in ks)
    assert len({cut_bin[k] // 16 for k in ks}) > 4                     # more than one 16-bin thread group


def test_boundary_case():
    c = CASES["boundary"]
    assert c.ks == [R.BOUNDARY_K] * 2
    for e, T, cand in ((0, R.BOUNDARY_FITS, 4096), (1, R.BOUNDARY_OVER, 4097)):
        v = c.logits(e)
        assert v.size == 100 + T + 5000 and (v >= 2).sum() == 100 and ((v >= -1) & (v < 0.5)).sum() == 5000
        tied = (R.bits_of(v) >> 8) == (0x3F800000 >> 8)
        assert tied.sum() == T and len(set(R.bits_of(v[tied]).tolist())) == 256
        assert R.candidate_count(v, R.BOUNDARY_K) == cand
        where = np.nonzero(tied)[0]
        assert where.min() < 50 and where.max() > v.size - 50          # interleaved, not a block
    assert R.CAND == 4096


def test_size_cases():
    c = CASES["grid_cap"]
    assert c.n(0) == 600000 > 256 * 256 * 8 and c.n_maps == 2 and 2048 in c.ks
    c = CASES["sizes"]
    shape = [(c.n(b), c.ks[b]) for b in range(c.nb)]
    assert {(1, 1), (1, 0), (1500, 1500), (900, 0), (2048, 2048), (4000, 2048)} <= set(shape)
    c = CASES["ragged"]
    assert c.nb == 16 and c.n_maps == 8
    ln = np.array([[c.seg[b][m + 1] - c.seg[b][m] for m in range(8)] for b in range(16)])
    assert (ln == 0).any(1).sum() >= 8 and (ln == 1).sum() >= 8        # empty maps and one-logit maps in between
    assert c.n(5) == 0 and c.n(4) >= 2048 and c.n(6) >= 2048 and c.ks[4] == c.ks[6] == 2048 and c.ks[5] == 0
    assert c.n(9) == 1 and c.ks[9] == 1
    assert any(c.ks[b] == c.n(b) > 1 for b in range(16)) and any(c.ks[b] == 0 < c.n(b) for b in range(16))
    for b in range(16):                                                # the real layout: rows example after example
        assert c.site[b] == [int(c.counts[m][:b].sum()) for m in range(8)]


def test_glue_scene():
    s = R.GlueScene()
    for m, cnt in enumerate(s.COUNTS):
        cc = s.coords[m]
        assert len(set(map(tuple, cc.tolist()))) == len(cc) == sum(cnt) and (np.diff(cc[:, 3]) >= 0).all()
        assert (cc[:, :3] < np.array(s.SPATIAL[m])).all()
    all_bits = np.concatenate([R.bits_of(o) for o in s.obj])
    for word in (R.NAN_POS, R.NAN_NEG, 0, 0x80000000):
        assert (all_bits == word).sum() == 1
    for b, (nan_word, zero_word) in enumerate(((R.NAN_POS, 0x80000000), (R.NAN_NEG, 0))):
        v = s.logits(b)
        assert v.size >= s.K                                           # the batched path takes the scene
        top = v[R.topk_order(v, s.K)]
        assert R.bits_of(top[:1])[0] == nan_word and not np.isnan(top[1:]).any()
        assert (R.bits_of(top) == zero_word).sum() == 1 and (top == 0).sum() == 1 and top[-1] < 0
        assert len(set(_rank_key(top).tolist())) == s.K                # no two of the top k logits are equal


# ---------------------------------------------------------------- suppression
@pytest.fixture(scope="module")
def rotated_matrices():
    out = {}
    for _, n, seed, _, _, _ in R.NMS_ROTATED:
        if (n, seed) not in out:
            b, sc = R.nms_rotated_inputs(n, seed)
            assert (np.diff(sc) <= 0).all()
            out[(n, seed)] = (b, sc, O.boxes_iou_3d(b, b, (0, 0, 0, 0), -1, True), O.clip_iou_matrix(b))
    return out


# kept, only-far suppressed: the oracle's figures (CPU)
ROTATED_FIGURES = {"n3000_t05": (901, 260), "n3000_t03": (420, 352), "n3000_post700": (700, 260), "n2176": (693, 2),
                   "n2113": (711, 0)}


@pytest.mark.parametrize("name,n,seed,thr,post,far", R.NMS_ROTATED)
def test_rotated_nms_lists_reach_the_far_loop(rotated_matrices, name, n, seed, thr, post, far):
    b, sc, pre, dec = rotated_matrices[(n, seed)]
    assert (n + 63) // 64 >= 34 and (name != "n2113" or n == 33 * 64 + 1)       # 2113: the first size with a far word
    want = O.rotate_nms_3d(b, sc, None, post, thr)
    upper = np.triu(np.ones((n, n), bool), 1)
    sup = (pre > 0) & (dec >= np.float64(np.float32(thr))) & upper
    keep = R.greedy(sup)
    assert np.array_equal(keep[:post], want)                           # the oracle's loop, restated on its two matrices
    only_far = R.only_far_suppressed(sup, keep)
    assert (len(want), len(only_far)) == ROTATED_FIGURES[name]
    assert (len(only_far) > 0) == far or name == "n3000_post700"
    if name == "n3000_post700":                                        # the scan stops at post_max, rows before the end
        assert np.array_equal(want, keep[:700]) and len(keep) > 700 and (keep[699] >> 6) < (n >> 6) - 1
    # no pair stands on the threshold, no suppressing pair on the pre-filter's
    assert np.abs(dec[upper] - np.float64(np.float32(thr))).min() > 1e-9
    assert pre[(dec >= np.float64(np.float32(thr))) & upper].min() > 1e-3
    # a scan without the far words keeps more
    near = sup & ((np.arange(n)[None, :] >> 6) - (np.arange(n)[:, None] >> 6) <= R.SCAN_NEAR)
    assert far == (not np.array_equal(R.greedy(near)[:post], want)) or name == "n3000_post700"


def test_axis_aligned_nms_list_reaches_the_far_loop():
    n, _, thr = R.NMS_AXIS
    d, sc = R.nms_axis_inputs()
    assert d.shape == (n, 4) and (np.diff(sc) <= 0).all()
    assert (d[:, :2] >= 0).all() and (d[:, :2] <= 400).all()
    wh = d[:, 2:] - d[:, :2]
    assert (wh > 4.99).all() and (wh < 40.01).all()
    want = O.nms_axis_aligned(d, sc, thr)
    iou = R.axis_iou_matrix(d)
    sup = np.triu(iou >= np.float32(thr), 1)
    keep = R.greedy(sup)
    assert np.array_equal(keep, want)
    only_far = R.only_far_suppressed(sup, keep)
    # the CPU oracle's figures for this draw order (xy, then wh, then scores, from default_rng(5))
    assert (len(want), len(only_far)) == (1857, 107)
    assert np.abs(iou[np.triu_indices(n, 1)] - np.float32(thr)).min() > 1e-6     # both sides evaluate the same fp32 expression


def test_only_far_suppressed_counts_what_it_says():
    n = 64 * 40
    sup = np.zeros((n, n), bool)
    sup[0, 64 * 33] = True             # 33 blocks to the right: far
    sup[0, 64 * 32 + 5] = True         # 32 blocks: the prefetch covers it
    sup[0, 64 * 35] = sup[64 * 10, 64 * 35] = True        # far and near suppressor: not only-far
    sup[64 * 33, 64 * 39] = True       # its suppressor is itself suppressed: kept
    keep = R.greedy(sup)
    assert R.only_far_suppressed(sup, keep).tolist() == [64 * 33]
    assert 64 * 39 in keep.tolist() and 64 * 35 not in keep.tolist()
