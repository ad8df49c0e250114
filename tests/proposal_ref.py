"""The proposal stage's selection and suppression, defined in plain numpy, and the inputs of tests/test_gpu_proposal_limits.py
(nothing of the package is imported here; tests/test_proposal_ref_host.py checks without a GPU that every input reaches
the edge its name claims).

Selection (aabr_rpn_topk_maps, csrc/iou_nms.hip): `topk_order` is the definition -- torch.topk's value order (a NaN of
either sign above +inf, then descending value, -0 equal to +0) made total by the library's documented index rule (equal
logits, and NaN among themselves, by ascending list index).  `order_key` restates the documented 32-bit key (sign,
exponent, mantissa; canonical for NaN and zero) ONLY to place inputs on the edges of the kernel's two 12-bit histograms
and of its 4096-entry candidate buffer; no expected output comes from it.

Suppression (aabr_rotate_nms_sorted / aabr_nms_sorted, csrc/nms_shared.h nms_scan_block): a kept row's suppression words
right of the diagonal are OR-ed in two parts, the 32 words next to the diagonal from a prefetch and every later word by a
strided loop that only exists from 34 column blocks (2113 boxes) on.  `only_far_suppressed` counts the boxes that only
that loop can suppress."""
import numpy as np

import synth_scenes as S

NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000
K_MAX, CAND, BINS = 2048, 4096, 4096          # the entry's k limit, its candidate buffer, bins of one histogram level
SCAN_NEAR = 32                                # column blocks right of the diagonal that the scan's prefetch covers


def f32_from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits_of(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def word_of(x):
    """the 32 bits of float32(x)"""
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------- selection: the definition
def topk_order(v, k):
    """indices of the k first logits of v: NaN (either sign) first, then descending value compared in float64 (-0 == +0),
    then ascending index"""
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        val = np.where(nan, 0.0, v.astype(np.float64))
    return np.lexsort((np.arange(v.size), -val, ~nan))[:k]


def order_key(v):
    """the documented key of a logit (uint32, larger = earlier): sign flipped into an unsigned order, every NaN the
    topmost key, -0 the key of +0.  For input construction only."""
    u = bits_of(v).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    mag = u & 0x7FFFFFFF
    key = np.where(mag > 0x7F800000, 0xFFFFFFFF, key)
    key = np.where(mag == 0, 0x80000000, key)
    return key.astype(np.uint32)


def prefix12(v):
    """leading 12 bits of the key: sign, exponent, top 3 mantissa bits -- the level-1 histogram bin"""
    return (order_key(v) >> 20).astype(np.int64)


def bin_counts(v):
    return np.bincount(prefix12(v), minlength=BINS)


def candidate_count(v, k):
    """logits whose 24-bit key prefix is at or above that of the k-th logit in the order: what the kernel gathers"""
    if k == 0:
        return int((order_key(v) >> 8 == 0xFFFFFF).sum())
    p = order_key(v) >> 8
    return int((p >= p[topk_order(v, k)[-1]]).sum())


class TopkCase(object):
    """maps: the logit buffers; seg[b]: n_maps + 1 list indices, the first of every map and the list's length; site[b]:
    the example's first site row in every map; ks[b].  Examples may alias the same rows."""

    def __init__(self, name, A, maps, seg, site, ks):
        self.name, self.A, self.maps = name, A, [np.ascontiguousarray(m, np.float32) for m in maps]
        self.seg, self.site, self.ks = [list(s) for s in seg], [list(s) for s in site], list(ks)
        self.nb, self.n_maps = len(ks), len(maps)
        assert 1 <= self.nb <= 16 and 1 <= self.n_maps <= 8 and len(seg) == len(site) == self.nb
        for b in range(self.nb):
            s = self.seg[b]
            assert len(s) == self.n_maps + 1 and s[0] == 0 and len(self.site[b]) == self.n_maps
            for m in range(self.n_maps):
                ln = s[m + 1] - s[m]
                assert ln >= 0 and ln % A == 0 and self.site[b][m] * A + ln <= self.maps[m].size
            assert 0 <= self.ks[b] <= min(s[-1], K_MAX)

    def n(self, b):
        return self.seg[b][-1]

    def logits(self, b):
        """example b's list, maps end to end"""
        s, st, A = self.seg[b], self.site[b], self.A
        parts = [self.maps[m][st[m] * A:st[m] * A + s[m + 1] - s[m]] for m in range(self.n_maps)]
        return np.concatenate(parts) if parts else np.zeros(0, np.float32)

    def expected(self, b):
        return topk_order(self.logits(b), self.ks[b])


def _aliased(name, A, maps, ks):
    """every example the whole of every map, one k each"""
    seg = [0]
    for m in maps:
        seg.append(seg[-1] + len(m))
    return TopkCase(name, A, maps, [seg] * len(ks), [[0] * len(maps)] * len(ks), ks)


SPECIAL_KINDS = ("nan_neg", "nan_pos", "+inf", "-inf", "+0", "-0", "+denormal", "-denormal")
SPECIAL_EACH = 24


def special_values_case():
    """20,000 logits over 60 decades with a few dozen each of both NaN sign bits, both infinities, both zeros and both
    signs of a denormal; the NaN of lowest index has the sign bit set.  3 maps, A = 2, k = 1 / 50 / 600 / 2048."""
    rng = np.random.default_rng(401)
    n = 20000
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    assert np.isfinite(v).all() and (np.abs(v) > 1e-37).all()
    pos = np.sort(rng.choice(n, SPECIAL_EACH * len(SPECIAL_KINDS), replace=False))
    bits = bits_of(v).copy()
    word = {"nan_neg": NAN_NEG, "nan_pos": NAN_POS, "+inf": 0x7F800000, "-inf": 0xFF800000, "+0": 0, "-0": 0x80000000,
            "+denormal": word_of(1e-42), "-denormal": word_of(-1e-42)}
    for i, p in enumerate(pos):
        bits[p] = word[SPECIAL_KINDS[i % len(SPECIAL_KINDS)]]
    v = f32_from_bits(bits)
    return _aliased("special", 2, [v[:7000], v[7000:13000], v[13000:]], [1, 50, 600, 2048])


ZEROS_EACH, ZEROS_POSITIVE = 130, 40


def signed_zeros_case():
    """3,000 logits, 40 positive, 130 -0 and 130 +0 interleaved (a -0 before the first +0), the rest negative; 16 values of
    k, most of them inside the run of zeros"""
    rng = np.random.default_rng(402)
    n = 3000
    v = (-np.abs(rng.standard_normal(n)) - 0.125).astype(np.float32)
    pos = rng.choice(n, ZEROS_POSITIVE + 2 * ZEROS_EACH, replace=False)
    v[pos[:ZEROS_POSITIVE]] = (0.5 + rng.random(ZEROS_POSITIVE)).astype(np.float32)
    zeros = np.sort(pos[ZEROS_POSITIVE:])
    sign = np.zeros(2 * ZEROS_EACH, bool)
    sign[0] = True                                    # the zero of lowest index is -0
    sign[1:] = rng.permutation(np.arange(1, 2 * ZEROS_EACH) % 2 == 0)
    v[zeros] = np.where(sign, np.float32(-0.0), np.float32(0.0))
    ks = [1, 40, 41, 42, 45, 60, 100, 170, 171, 200, 299, 300, 301, 302, 400, 2048]
    return _aliased("signed_zeros", 1, [v[:1700], v[1700:]], ks)


def uniform_lists_case():
    """3,000 NaN (both sign bits, several payloads) and 3,000 -inf, k = 2000: every logit has one key, all fit the
    candidate buffer, the order is the index"""
    rng = np.random.default_rng(403)
    payload = np.array([NAN_POS, NAN_NEG, 0x7FC00001, 0xFFFFFFFF, 0x7F800001], np.uint32)
    nan = f32_from_bits(payload[rng.integers(0, len(payload), 3000)])
    assert np.isnan(nan).all()
    ninf = np.full(3000, -np.inf, np.float32)
    return TopkCase("uniform", 1, [nan, ninf], [[0, 3000, 3000], [0, 0, 3000]], [[0, 0], [0, 0]], [2000, 2000])


def histogram_edges_list():
    """+-2**e (1 + m / 8)(1 + s), e = -4 .. 3, m = 0 .. 7: 64 consecutive level-1 bins on either side of zero, 15 .. 25
    values in each that differ in the next 12 bits, 50 zeros of both signs between the sides; shuffled"""
    rng = np.random.default_rng(404)
    vals = []
    for sign in (1.0, -1.0):
        for e in range(-4, 4):
            for m in range(8):
                cnt = 15 + (5 * e + 3 * m + (0 if sign > 0 else 4)) % 11
                s = (np.arange(cnt) + 1) * (0.06 / 25)
                vals.append(sign * 2.0 ** e * (1 + m / 8.0) * (1 + s))
    vals.append(np.where(np.arange(50) % 3 == 0, -0.0, 0.0))
    v = np.concatenate(vals).astype(np.float32)
    return v[rng.permutation(v.size)]


def histogram_sweep_ks(v):
    """k = P and P + 1 for every prefix sum P <= 2047 of the level-1 bin counts from the top"""
    c = bin_counts(v)[::-1]
    P = np.cumsum(c[c > 0])
    P = P[P <= K_MAX - 1]
    return sorted(set(P.tolist()) | set((P + 1).tolist()))


def histogram_edges_cases():
    v = histogram_edges_list()
    ks = histogram_sweep_ks(v)
    return [_aliased("hist_%d" % i, 1, [v[:1000], v[1000:]], ks[i:i + 16]) for i in range(0, len(ks), 16)]


def boundary_list(T):
    """100 values >= 2, T values of bits 0x3F800000 + (i % 256) (one 24-bit prefix), 5,000 in [-1, 0.5); interleaved"""
    rng = np.random.default_rng(405)
    top = (2.0 + 10.0 * rng.random(100)).astype(np.float32)
    tied = f32_from_bits(0x3F800000 + (np.arange(T) % 256).astype(np.uint32))
    low = (-1.0 + 1.5 * rng.random(5000)).astype(np.float32)
    low = np.minimum(low, np.float32(0.49999997))
    v = np.concatenate([top, tied, low])
    return v[rng.permutation(v.size)]


BOUNDARY_K, BOUNDARY_FITS, BOUNDARY_OVER = 150, 3996, 3997


def boundary_case():
    """example 0: 4096 candidates (fits), example 1: 4097 (overflow)"""
    a, b = boundary_list(BOUNDARY_FITS), boundary_list(BOUNDARY_OVER)
    return TopkCase("boundary", 1, [a, b], [[0, a.size, a.size], [0, 0, b.size]], [[0, 0], [0, 0]],
                    [BOUNDARY_K, BOUNDARY_K])


def grid_cap_case():
    """600,000 logits in 2 maps: more than 256 workgroups x 256 threads x 8, so the grid is capped and a thread walks
    more than 8 entries"""
    rng = np.random.default_rng(406)
    v = (rng.standard_normal(600000) * 2.0 ** rng.integers(-3, 4, 600000)).astype(np.float32)
    return _aliased("grid_cap", 1, [v[:350000], v[350000:]], [2048, 7])


def sizes_case():
    """n = 1 (k = 1 and k = 0), k = n, k = 0 with n > 0, k = n = 2048, over aliased rows of one buffer"""
    rng = np.random.default_rng(407)
    v = rng.standard_normal(4000).astype(np.float32)
    rows = [(0, 1, 1), (5, 1, 0), (10, 1500, 1500), (100, 900, 0), (1000, 2048, 2048), (1, 2, 2), (0, 4000, 2048)]
    return TopkCase("sizes", 1, [v], [[0, n] for _, n, _ in rows], [[s] for s, _, _ in rows], [k for _, _, k in rows])


def ragged_case():
    """16 examples x 8 maps in the real layout (every map's rows example after example): empty maps, one-logit maps, an
    example empty in every map between two full ones"""
    rng = np.random.default_rng(408)
    nb, n_maps = 16, 8
    counts = rng.integers(0, 700, (n_maps, nb))
    counts[rng.random((n_maps, nb)) < 0.25] = 0
    counts[rng.random((n_maps, nb)) < 0.15] = 1
    counts[:, 5] = 0                                  # empty between two full ones
    counts[:, 4] = np.maximum(counts[:, 4], 300)
    counts[:, 6] = np.maximum(counts[:, 6], 300)
    counts[:, 9] = 0
    counts[3, 9] = 1                                  # a one-logit example
    maps = []
    for m in range(n_maps):
        v = rng.standard_normal(int(counts[m].sum())).astype(np.float32)
        v[rng.integers(0, max(v.size, 1), v.size // 40)] = 0.25     # exact ties
        maps.append(v)
    seg, site, row = [], [], [0] * n_maps
    for b in range(nb):
        s = [0]
        for m in range(n_maps):
            s.append(s[-1] + int(counts[m][b]))
        seg.append(s)
        site.append(list(row))
        row = [row[m] + int(counts[m][b]) for m in range(n_maps)]
    want = [2048, 1, 600, 0, 2048, 0, 2048, 300, 2048, 1, 17, 2048, 999, 2048, 64, 2048]
    ks = [min(want[b], seg[b][-1], K_MAX) for b in range(nb)]
    case = TopkCase("ragged", 1, maps, seg, site, ks)
    case.counts = counts
    return case


def topk_cases():
    cases = [special_values_case(), signed_zeros_case(), uniform_lists_case(), boundary_case(), grid_cap_case(),
             sizes_case(), ragged_case()] + histogram_edges_cases()
    return dict((c.name, c) for c in cases)


# ---------------------------------------------------------------- selection through the glue
class GlueScene(object):
    """two examples over two maps, A = 2: example 0's objectness holds NaN 0x7FC00000 and a -0, example 1's NaN 0xFFC00000
    and a +0, each zero inside its example's top k; every other logit is distinct"""
    A, K, POST = 2, 300, 100
    SPATIAL = ((24, 24, 4), (12, 12, 2))
    STRIDES = ((4.0, 4.0, 4.0), (8.0, 8.0, 8.0))
    COUNTS = ((400, 380), (60, 50))                   # sites per (map, example)

    def __init__(self):
        rng = np.random.default_rng(409)
        self.coords, self.obj, self.reg, self.base = [], [], [], []
        for mi, (sp, cnt) in enumerate(zip(self.SPATIAL, self.COUNTS)):
            cc = []
            for b, c in enumerate(cnt):
                cells = rng.permutation(sp[0] * sp[1] * sp[2])[:c]
                cc.append(np.stack([cells // (sp[1] * sp[2]), cells // sp[2] % sp[1], cells % sp[2], np.full(c, b)], 1))
            self.coords.append(np.concatenate(cc).astype(np.int64))
            V = sum(cnt)
            self.obj.append((rng.standard_normal(V * self.A) - 1.0).astype(np.float32))
            self.reg.append((rng.standard_normal((V * self.A, 7)) * 0.3).astype(np.float32))
            base = np.zeros((self.A, 7), np.float32)
            base[:, 3:6] = [0.2 * (mi + 1), 1.5 * (mi + 1), 2.6]
            base[:, 6] = [0.0, -1.57]
            self.base.append(base)
        A = self.A
        o0, o1 = bits_of(self.obj[0]).copy(), bits_of(self.obj[1]).copy()
        o0[123] = NAN_POS                             # example 0, map 0
        o1[7] = 0x80000000                            # example 0, map 1: -0
        o1[self.COUNTS[1][0] * A + 31] = NAN_NEG      # example 1, map 1
        o0[self.COUNTS[0][0] * A + 200] = 0           # example 1, map 0: +0
        self.obj = [f32_from_bits(o0), f32_from_bits(o1)]

    def logits(self, b):
        A, out = self.A, []
        for m, cnt in enumerate(self.COUNTS):
            r0 = sum(cnt[:b])
            out.append(self.obj[m][r0 * A:(r0 + cnt[b]) * A])
        return np.concatenate(out)


# ---------------------------------------------------------------- suppression
def nms_rotated_inputs(n, seed):
    """synth_scenes.make_nms_boxes in descending-score order (stable): what aabr_rotate_nms_sorted takes"""
    b7, sc = S.make_nms_boxes(n, seed)
    order = np.argsort(-sc, kind="stable")
    return np.ascontiguousarray(b7[order]), np.ascontiguousarray(sc[order])


# (name, boxes, seed, threshold, post_max, only-far suppressed boxes must exist).  2113 boxes are 34 column blocks, the first
# size with a far word (row block 0, word 33); 2176 fill those 34 blocks to the last column; 3000 are 47 blocks.  With
# post_max = 700 the scan stops at row block 28, after far words have been OR-ed in but before any is read.
NMS_ROTATED = (("n3000_t05", 3000, 3013, 0.5, 3000, True), ("n3000_t03", 3000, 3013, 0.3, 3000, True),
               ("n3000_post700", 3000, 3013, 0.5, 700, False), ("n2176", 2176, 7, 0.5, 2176, True),
               ("n2113", 2113, 7, 0.5, 2113, False))
NMS_AXIS = (3000, 5, 0.4)


def nms_axis_inputs():
    n, seed, _ = NMS_AXIS
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 400, (n, 2))
    wh = rng.uniform(5, 40, (n, 2))
    sc = rng.random(n).astype(np.float32)
    d = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    order = np.argsort(-sc, kind="stable")
    return np.ascontiguousarray(d[order]), np.ascontiguousarray(sc[order])


def axis_iou_matrix(d):
    """the fp32 expression of maskrcnn_benchmark's nms (the +1 pixel convention), operation by operation"""
    d = np.asarray(d, np.float32)
    one = np.float32(1)
    area = (d[:, 2] - d[:, 0] + one) * (d[:, 3] - d[:, 1] + one)
    xx1, yy1 = np.maximum(d[:, None, 0], d[None, :, 0]), np.maximum(d[:, None, 1], d[None, :, 1])
    xx2, yy2 = np.minimum(d[:, None, 2], d[None, :, 2]), np.minimum(d[:, None, 3], d[None, :, 3])
    w, h = np.maximum(np.float32(0), xx2 - xx1 + one), np.maximum(np.float32(0), yy2 - yy1 + one)
    inter = w * h
    return inter / (area[:, None] + area[None, :] - inter)


def greedy(sup):
    """keep list of a sorted list under the boolean matrix sup[i, j] = `i suppresses j` (read for i < j only)"""
    n = sup.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= sup[i, i + 1:]
    return np.array(keep, np.int64)


def only_far_suppressed(sup, keep):
    """boxes that are not kept and whose EVERY kept suppressor lies more than SCAN_NEAR column blocks (of 64) to their
    left: only the scan's far loop can suppress them"""
    n = sup.shape[0]
    keep = np.asarray(keep, np.int64)
    kept = np.zeros(n, bool)
    kept[keep] = True
    blk = np.arange(n) >> 6
    by = np.triu(sup, 1) & kept[:, None]                       # by[i, j]: kept i suppresses j
    far = (blk[None, :] - blk[:, None]) > SCAN_NEAR
    return np.nonzero(~kept & by.any(0) & ~(by & ~far).any(0))[0]
