"""Definition of the RPN label generation (csrc/iou_nms.hip k_rpn_label_maps, reference: rpn/loss_3d.py:91-100 ->
boxlist_iou_3d + Matcher), written without the package: plain numpy, fp64 wherever the kernel computes in double.  The
labels go through oracle/box_oracle.py `matcher` / `angle_dif`, which tests/golden/matcher_golden.npz pins to the
reference's own Matcher.

What is defined here
  anchors      AnchorGenerator.grid_anchors of an example: `coords / voxel_scale * stride + base`, fp32, the maps laid
               end to end ([map][site][yaw]).
  criterion 6  as rotate_iou (csrc/iou_math.h) evaluates it: the reference's fp32 thickness clamps, fp32 differences
               widened to double, `1 - ((|dw| + |dl|) + sqrt(d0^2 + d1^2)) / 0.7` in double, ONE narrowing to fp32, and
               the `same_box -> 1.0` patch of iou_eval_entry.
  z factor     `overlap / common` of the two z intervals in fp64 from the fp32 interval ends (only_xy off).
  criterion -1 the exact polygon IoU of the two rectangles (Sutherland-Hodgman clip in fp64), the figure the
               vertex-collection IoU of the reference approximates.

Bounds on the device's distance from these values, u = 2^-24 (unit roundoff of fp32, round to nearest)
  criterion 6, only_xy on: every fp32 subtraction is correctly rounded on both sides (and exact on the builders'
    lattice), sqrt / + / / / - are IEEE double on both sides (the library is built with -ffp-contract=off) and there is
    one narrowing: the device value is the correctly rounded fp32 of the same double unless a double operation differs
    in its last bit, which moves the fp32 result by at most one ulp.  Bound: 1 ulp; bit-equality is expected.
  z factor: the builders keep every interval end on the lattice, so `overlap` and `common` are exact in fp32
    (tests/test_label_ref_host.py checks it).  The device then rounds three times: v = fl(v64), q = fl(overlap / common),
    result = fl(v q).  Each rounding multiplies by (1 + e), |e| <= u, while nothing is subnormal (|q| is 0 or at least
    2^-14 on the lattice, |v| at least 2^-20 or exactly 0), so |device - v64 q64| <= ((1 + u)^3 - 1) |v64 q64|.  Where
    the device's double differs from numpy's in its last bit (see above) v moves by one more fp32 ulp at most: the bound
    used is ((1 + u)^3 (1 + 2u) - 1) |v64 q64|, about 5 u relative.  0 / 0 (two zero heights at one z) is NaN on both sides.
  criterion -1: the project's figure for this kernel against the oracle, atol 2e-5 (tests/test_gpu_labels.py).

Case builders: integer site coordinates, voxel_scale 16, strides 4 and 8, base sizes and ground-truth centres / sizes on
multiples of 1/16 with magnitudes far below 2^10, anchor yaws 0, -1.5, -0.75, 0.75 -- every fp32 subtraction of the
kernel is then exact.  Ground-truth yaws come from a list whose wrapped differences to the anchor yaws all lie further
than 0.05 from the yaw threshold 0.7, so the mask is the same in fp32 and fp64."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import box_oracle as BO  # noqa: E402

F = np.float32
U = 2.0 ** -24
VOXEL_SCALE = 16.0
STRIDES = ((4.0, 4.0, 4.0), (8.0, 8.0, 8.0), (4.0, 4.0, 8.0))
YAWS = (0.0, -1.5, -0.75, 0.75)
GT_YAWS = (0.0, 0.25, -0.25, 1.5, -1.25, 3.0, -2.5, 0.5)       # 3.0 and -2.5 lie outside (-pi/2, pi/2]
MASKED_YAW = 0.8125               # against anchor yaws 0 and -1.5: |wrapped difference| 0.8125 and 0.829, both >= 0.7
LABEL_AUG = (0.4, 0.8, 0.0, 0.0)  # target_Y, target_Z, anchor_Y, anchor_Z (config/defaults.py:161-162)
Z_FACTOR_REL = (1 + U) ** 3 * (1 + 2 * U) - 1


class Case(object):
    """maps: per map (coords int32 [V, 4] with the example in column 3, rows example-contiguous; stride (3); base [A, 7]);
    counts[m][b] sites of example b in map m; targets[b] fp32 [G_b, 7] yx_zb"""

    def __init__(self, name, maps, counts, targets, aug=LABEL_AUG, criterion=6, only_xy=1, fg=0.55, bg=0.2,
                 yaw_threshold=0.7, weights=(1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 1.5), duplicates=()):
        self.name, self.maps, self.counts, self.targets = name, maps, counts, targets
        self.aug, self.criterion, self.only_xy = tuple(float(v) for v in aug), int(criterion), int(only_xy)
        self.fg, self.bg, self.yaw_threshold, self.weights = fg, bg, yaw_threshold, tuple(weights)
        self.duplicates = tuple(duplicates)            # (earlier, later) pairs of identical ground-truth boxes
        self.A = int(maps[0][2].shape[0])
        self.nb = len(targets)
        assert all(len(c) == self.nb for c in counts) and len(counts) == len(maps)
        for (coords, _, base), c in zip(maps, counts):
            assert coords.shape == (sum(c), 4) and coords.dtype == np.int32 and base.shape == (self.A, 7)
            assert (coords[:, 3] == np.repeat(np.arange(self.nb), c)).all()

    def n_anchors(self, b):
        return sum(c[b] for c in self.counts) * self.A


# ------------------------------------------------------------------------------------------------------ the definition
def anchors(case, b):
    """the materialised anchors of example b, fp32 [N_b, 7], map-major, rows [site, yaw]"""
    return _anchors(case.maps, case.counts, b)


def _anchors(maps, counts, b):
    out = []
    for (coords, stride, base), c in zip(maps, counts):
        rows = coords[sum(c[:b]):sum(c[:b + 1])]
        cen = rows[:, :3].astype(F) / F(VOXEL_SCALE) * np.asarray(stride, F).reshape(1, 3)
        a = np.zeros((rows.shape[0], base.shape[0], 7), F)
        a[:, :, :3] = cen[:, None, :] + base[None, :, :3].astype(F)
        a[:, :, 3:] = F(0) + base[None, :, 3:].astype(F)
        out.append(a.reshape(-1, 7))
    return np.concatenate(out, 0) if out else np.zeros((0, 7), F)


def _clamped(b7, min_y, min_z):
    """(x, y, size along column 3 clamped, size along column 4, yaw), z0, z1 -- fp32, rotate_nms_3d_torch.py:59-66"""
    b7 = np.asarray(b7, F).reshape(-1, 7)
    th = np.where(b7[:, 3] < F(min_y), F(min_y), b7[:, 3]).astype(F)
    h = np.where(b7[:, 5] < F(min_z), F(min_z), b7[:, 5]).astype(F)
    return np.stack([b7[:, 0], b7[:, 1], th, b7[:, 4], b7[:, 6]], 1).astype(F), b7[:, 2].astype(F), (b7[:, 2] + h).astype(F)


def _same_box(t5, a5):
    d = np.abs(t5[:, None, :] - a5[None, :, :]).astype(F)
    return (d < F(1e-6)).all(2)


def criterion6(targets, anch, aug=LABEL_AUG):
    """[G, N]: (fp32 value, the double before the narrowing)"""
    t5, _, _ = _clamped(targets, aug[0], aug[1])
    a5, _, _ = _clamped(anch, aug[2], aug[3])
    diff = [(a5[None, :, d] - t5[:, None, d]).astype(F).astype(np.float64) for d in range(4)]
    dc = np.sqrt(diff[0] * diff[0] + diff[1] * diff[1])
    m = (np.abs(diff[2]) + np.abs(diff[3])) + dc
    v64 = 1 - m / 0.7
    v64 = np.where(_same_box(t5, a5), 1.0, v64)
    return v64.astype(F), v64


def z_factor(targets, anch, aug):
    """[G, N] fp64 `overlap / common`, and whether both fp32 subtractions of the kernel are exact for every pair"""
    _, t0, t1 = _clamped(targets, aug[0], aug[1])
    _, a0, a1 = _clamped(anch, aug[2], aug[3])
    lo32, hi32 = np.maximum(a0[None, :], t0[:, None]), np.minimum(a1[None, :], t1[:, None])
    LO32, HI32 = np.minimum(a0[None, :], t0[:, None]), np.maximum(a1[None, :], t1[:, None])
    overlap = hi32.astype(np.float64) - lo32.astype(np.float64)
    common = HI32.astype(np.float64) - LO32.astype(np.float64)
    exact = bool(((hi32 - lo32).astype(np.float64) == overlap).all() and ((HI32 - LO32).astype(np.float64) == common).all())
    with np.errstate(invalid="ignore", divide="ignore"):
        return overlap / common, exact


def _corners(r):
    c, s = math.cos(r[4]), math.sin(r[4])
    hx, hy = r[2] / 2, r[3] / 2
    return [(x * c + y * s + r[0], -x * s + y * c + r[1]) for x, y in ((-hx, -hy), (-hx, hy), (hx, hy), (hx, -hy))]


def _area2(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))


def _clip(subject, clipper):
    """Sutherland-Hodgman: `subject` cut down to the inside of the counter-clockwise convex `clipper`"""
    out = subject
    for i in range(len(clipper)):
        a, b = clipper[i], clipper[(i + 1) % len(clipper)]
        inp, out = out, []
        if not inp:
            break
        side = [(b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) for p in inp]
        for j, p in enumerate(inp):
            k = (j + 1) % len(inp)
            if side[j] >= 0:
                out.append(p)
            if (side[j] >= 0) != (side[k] >= 0):
                t = side[j] / (side[j] - side[k])
                out.append((p[0] + t * (inp[k][0] - p[0]), p[1] + t * (inp[k][1] - p[1])))
    return out


def polygon_iou(targets, anch, aug=LABEL_AUG):
    """criterion -1, [G, N] fp64: intersection over union of the two (clamped) rectangles, exact clip"""
    t5, _, _ = _clamped(targets, aug[0], aug[1])
    a5, _, _ = _clamped(anch, aug[2], aug[3])
    same = _same_box(t5, a5)
    out = np.zeros((t5.shape[0], a5.shape[0]))
    polys = []
    for r in list(t5.astype(np.float64)) + list(a5.astype(np.float64)):
        p = _corners(r)
        polys.append(p if _area2(p) > 0 else p[::-1])
    for g in range(t5.shape[0]):
        for n in range(a5.shape[0]):
            inter = abs(_area2(_clip(polys[g], polys[t5.shape[0] + n]))) / 2
            uni = abs(_area2(polys[g])) / 2 + abs(_area2(polys[t5.shape[0] + n])) / 2 - inter
            out[g, n] = 1.0 if same[g, n] else inter / uni
    return out


def matrix(case, b):
    """example b's [G, N] match-quality matrix as defined above: dict with `ref` fp64, `ref32` (criterion 6 with only_xy:
    the value the device must reach within one ulp; None otherwise) and `bound` (absolute, fp64; None with ref32)"""
    an, tg = anchors(case, b), case.targets[b]
    if case.criterion == 6:
        v32, v64 = criterion6(tg, an, case.aug)
        if case.only_xy:
            return {"ref": v64, "ref32": v32, "bound": None}
        q, exact = z_factor(tg, an, case.aug)
        assert exact, "%s: a z interval leaves the lattice" % case.name
        with np.errstate(invalid="ignore"):
            ref = v64 * q
            return {"ref": ref, "ref32": None, "bound": Z_FACTOR_REL * np.abs(ref)}
    assert case.criterion == -1 and case.only_xy
    ref = polygon_iou(tg, an, case.aug)
    return {"ref": ref, "ref32": None, "bound": np.full(ref.shape, 2e-5)}


def yaw_abs_diff(targets, anch):
    """|angle_dif(anchor yaw, target yaw)| fp32 [G, N], what the loss hands the Matcher (rpn/loss_3d.py:96-97)"""
    return np.abs(BO.angle_dif(np.asarray(anch, F)[:, 6].reshape(1, -1), np.asarray(targets, F)[:, 6].reshape(-1, 1)))


def yaw_margin(targets, anch, yaw_threshold):
    """the smallest distance of a |wrapped yaw difference| (fp64) from the threshold"""
    d = np.asarray(targets, np.float64)[:, 6].reshape(-1, 1) - np.asarray(anch, np.float64)[:, 6].reshape(1, -1)
    w = d - np.floor(d / math.pi + 0.5) * math.pi
    return float(np.abs(np.abs(w) - yaw_threshold).min()) if w.size else float("inf")


def labels(mq, targets, anch, fg, bg, allow_low, yaw_threshold):
    """(matched_idxs int64 [N], matched_vals fp32 [N]) of the reference's Matcher on the fp32 matrix `mq`"""
    with np.errstate(invalid="ignore"):                 # NaN entries are legitimate input
        return BO.matcher(mq, yaw_abs_diff(targets, anch), fg, bg, allow_low, yaw_threshold)


def masked(mq, targets, anch, yaw_threshold):
    """the matrix the Matcher takes its maxima on (matcher.py:51-56)"""
    mq = np.asarray(mq, F)
    if yaw_threshold > 1.58:
        return mq
    with np.errstate(invalid="ignore"):
        return (mq * (yaw_abs_diff(targets, anch) < F(yaw_threshold)).astype(F)).astype(F)


def ulp_distance(a, b):
    """distance in fp32 steps (-0 and +0 coincide); both arrays finite"""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------------ case builders
def _base(sizes, yaws, offset=(0.0, 0.0, 0.0)):
    return np.array([list(offset) + list(sizes) + [y] for y in yaws], F)


def _sites(rng, counts, extent):
    """counts[b] distinct integer sites per example inside `extent`, example-contiguous"""
    rows = []
    for b, n in enumerate(counts):
        flat = rng.permutation(extent[0] * extent[1] * extent[2])[:n]
        assert flat.size == n
        x, rest = np.divmod(flat, extent[1] * extent[2])
        y, z = np.divmod(rest, extent[2])
        rows.append(np.stack([x, y, z, np.full(n, b)], 1))
    return np.concatenate(rows, 0).astype(np.int32).reshape(-1, 4)


def _wrapped(d):
    return d - math.floor(d / math.pi + 0.5) * math.pi


def _targets(rng, G, anch, x_limit, yaws=GT_YAWS, z=(-4, 5), dh=(-2, 3)):
    """G ground-truth boxes on the lattice, each next to one anchor of `anch` whose centre has x <= x_limit: centre within
    2/16 per axis, sizes within 2/16, a yaw of `yaws` the mask lets through for that anchor -- so every box has a
    positive entry in its row of the masked matrix (a row without one has maximum +-0 and ties with EVERY masked anchor,
    matcher.py:126-128), and the anchors beyond x_limit stay without a match"""
    t = np.zeros((G, 7), F)
    if G == 0:
        return t
    pool = anch[anch[:, 0] <= x_limit] if len(anch) else anch
    pool = pool if len(pool) else anch
    if len(pool) == 0:                                # an example without sites: any boxes do
        pool = np.array([[1.0, 1.0, 0.0, 0.5, 1.5, 1.5, 0.0]], F)
    a = pool[rng.integers(0, len(pool), G)].astype(np.float64)
    t[:, 0:2] = a[:, 0:2] + rng.integers(-2, 3, (G, 2)) / 16.0
    t[:, 2] = a[:, 2] + rng.integers(z[0], z[1], G) / 16.0
    t[:, 3:5] = a[:, 3:5] + rng.integers(-2, 3, (G, 2)) / 16.0
    t[:, 5] = a[:, 5] + rng.integers(dh[0], dh[1], G) / 16.0
    for g in range(G):
        ok = [y for y in yaws if abs(_wrapped(y - a[g, 6])) < 0.65]
        t[g, 6] = ok[rng.integers(0, len(ok))]
    thin = rng.random(G) < 0.1
    t[thin, 3] = a[thin, 3] - 0.25                    # 0.5 -> 0.25, below target_Y: the clamp acts
    return t.astype(F)


SIZES2 = ((0.5, 1.5, 1.5), (1.5, 1.5, 1.0))
DUPLICATES = ((5, 200), (127, 128))


def chunk_case(G, seed=5):
    """one example, two maps, 204 anchors (one workgroup), the first G of 257 ground-truth boxes; boxes 200 and 128 are
    copies of boxes 5 and 127, which are copies of two anchors: those anchors' best value, 1.0, is reached twice -- for
    G >= 129 on both sides of index 128"""
    rng = np.random.default_rng(seed)
    m0 = _sites(rng, [35], (7, 5, 2))                # c / 16 * 4: a 0.25 grid over 1.5 x 1.0
    m1 = _sites(rng, [16], (8, 8, 1))                # c / 16 * 8: a 0.5 grid over 3.5 x 3.5, the boxes keep to x <= 1
    maps = [(m0, STRIDES[0], _base(SIZES2[0], YAWS, (0.0625, 0.0, 0.125))), (m1, STRIDES[1], _base(SIZES2[1], YAWS))]
    t = _targets(rng, 257, _anchors(maps, [[35], [16]], 0), 1.0)
    an = _anchors(maps, [[35], [16]], 0)
    t[5], t[127] = an[0], an[35 * 4]               # two anchors themselves (yaw 0): their best value is 1.0
    for first, later in DUPLICATES:
        t[later] = t[first]
    dup = tuple(p for p in DUPLICATES if p[1] < G)
    return Case("chunk_G%d" % G, maps, [[35], [16]], [t[:G].copy()], duplicates=dup)


CHUNK_G = (1, 127, 128, 129, 256, 257)


def _ragged(name, A, sites, n_gt, seed):
    """sites[b] = sites per map of example b; n_gt[b] ground-truth boxes"""
    rng = np.random.default_rng(seed)
    n_maps = len(sites[0])
    extents = ((20, 12, 2), (8, 8, 2), (6, 6, 1))
    sizes = ((0.5, 1.5, 1.5), (1.5, 1.5, 1.0), (0.75, 2.0, 1.5))
    counts = [[s[m] for s in sites] for m in range(n_maps)]
    maps = [(_sites(rng, counts[m], extents[m]), STRIDES[m], _base(sizes[m], YAWS[:A], (0.0, 0.0625 * m, 0.0)))
            for m in range(n_maps)]
    targets = [_targets(rng, g, _anchors(maps, counts, b), 2.0) for b, g in enumerate(n_gt)]
    return Case(name, maps, counts, targets)


def ragged_case_a():
    """16 examples, three maps, A = 4: one site against 129 boxes, no site at all, 1100 anchors (five workgroups) without
    any box and against 257, one site against one box, a map empty for one example"""
    sites = [(1, 0, 0), (0, 0, 0), (200, 60, 15), (200, 60, 15), (0, 1, 0), (40, 0, 11), (7, 3, 1), (3, 0, 2), (64, 0, 0),
             (0, 0, 5), (12, 9, 1), (1, 1, 1), (0, 33, 0), (5, 5, 5), (2, 0, 0), (100, 20, 8)]
    n_gt = [129, 3, 0, 257, 1, 130, 2, 0, 128, 5, 1, 31, 64, 3, 129, 12]
    return _ragged("ragged_a", 4, sites, n_gt, 11)


def ragged_case_b():
    """16 examples, two maps, A = 1: lists of exactly 255, 256 and 257 anchors among shorter and longer ones"""
    sites = [(200, 55), (3, 0), (200, 56), (0, 0), (201, 56), (1, 0), (0, 64), (240, 64), (0, 1), (130, 0), (17, 5), (0, 0),
             (210, 47), (2, 2), (63, 1), (64, 0)]
    n_gt = [129, 2, 128, 4, 257, 0, 7, 130, 1, 127, 256, 0, 3, 200, 1, 64]
    return _ragged("ragged_b", 1, sites, n_gt, 12)


def batch17_case():
    """17 examples over two maps (more than one library call takes), for rpn_glue.rpn_label_matches"""
    sites = [(9, 2), (4, 0), (0, 0), (12, 3), (1, 1), (7, 0), (3, 2), (0, 5), (5, 1), (2, 1), (8, 0), (1, 4), (6, 2), (10, 3),
             (3, 1), (4, 0), (11, 6)]
    n_gt = [3, 1, 2, 130, 0, 5, 2, 1, 4, 0, 7, 1, 2, 129, 3, 1, 6]
    return _ragged("batch17", 4, sites, n_gt, 17)


def yaw_case():
    """A = 2 (yaws 0 and -1.5): ground-truth yaws outside (-pi/2, pi/2], and box 3 masked against every anchor -- its
    row of the masked matrix holds only +-0, so every anchor ties with its maximum"""
    rng = np.random.default_rng(21)
    m0 = _sites(rng, [30], (7, 5, 2))
    m1 = _sites(rng, [10], (4, 4, 1))
    maps = [(m0, STRIDES[0], _base(SIZES2[0], YAWS[:2])), (m1, STRIDES[1], _base(SIZES2[1], YAWS[:2]))]
    t = _targets(rng, 9, _anchors(maps, [[30], [10]], 0), 1.0)
    t[0, 6], t[1, 6], t[3, 6] = 3.0, -2.5, MASKED_YAW
    return Case("yaw", maps, [[30], [10]], [t])


def z_case(clamped):
    """only_xy off: z intervals that overlap, touch and lie apart (a negative factor); thickness clamps on (dyadic, so
    the interval ends stay on the lattice) or all 0"""
    rng = np.random.default_rng(31)
    m0 = _sites(rng, [30], (7, 5, 3))                # anchor z: 0, 0.25, 0.5 (+ base) -- height 1.5
    m1 = _sites(rng, [10], (4, 4, 2))
    maps = [(m0, STRIDES[0], _base(SIZES2[0], YAWS)), (m1, STRIDES[1], _base(SIZES2[1], YAWS))]
    t = _targets(rng, 24, _anchors(maps, [[30], [10]], 0), 1.0, z=(-8, 9))
    t[0, 2], t[0, 5] = 2.0, 1.0                      # touches the top of the anchors that start at 0.5 (0.5 + 1.5 = 2.0)
    t[1, 2], t[1, 5] = 3.0, 0.5                      # above every anchor: negative factor
    t[2, 2], t[2, 5] = -2.0, 0.25                    # below every anchor; height under the clamp
    aug = (0.5, 0.75, 0.25, 0.5) if clamped else (0.0, 0.0, 0.0, 0.0)
    return Case("z_clamped" if clamped else "z_plain", maps, [[30], [10]], [t], aug=aug, only_xy=0)


def nan_case():
    """only_xy off, no height clamp, base anchors of height 0: a zero-height ground truth at an anchor's z gives 0 / 0"""
    rng = np.random.default_rng(41)
    m0 = _sites(rng, [30], (7, 5, 2))                # anchor z: 0 and 0.25
    sizes = ((0.5, 1.5, 0.0),)
    maps = [(m0, STRIDES[0], _base(sizes[0], YAWS))]
    t = _targets(rng, 6, _anchors(maps, [[30]], 0), 1.0, z=(-2, 3), dh=(8, 17))
    t[1, 2], t[1, 5] = 0.0, 0.0                      # NaN against every anchor at z = 0
    t[4, 2], t[4, 5] = 0.25, 0.0                     # NaN against every anchor at z = 0.25
    t[2, 2], t[2, 5] = 0.0, 0.5                      # a finite neighbour at the same z
    return Case("nan", maps, [[30]], [t], aug=(0.4, 0.0, 0.0, 0.0), only_xy=0)


def iou_case():
    """criterion -1: rectangles in general position (centres and sizes off the lattice, no coinciding edges)"""
    rng = np.random.default_rng(51)
    m0 = _sites(rng, [25], (7, 5, 1))
    maps = [(m0, STRIDES[0], _base(SIZES2[0], YAWS))]
    t = _targets(rng, 12, _anchors(maps, [[25]], 0), 1.0, yaws=(0.25, -0.25, 0.5, -1.25, 1.5, 3.0))
    t[:, 0:2] += (rng.random((12, 2)) * 0.05 + 0.003).astype(F)
    t[:, 3:5] += (rng.random((12, 2)) * 0.05 + 0.003).astype(F)
    return Case("iou", maps, [[25]], [t], criterion=-1, fg=0.5, bg=0.15)


def attained_thresholds(matched_vals):
    """(fg, bg): the two values nearest to 0.55 and 0.2 among those the anchors' best values attain, bg < fg"""
    v = np.unique(np.asarray(matched_vals, F)[np.isfinite(matched_vals)])
    fg = v[np.argmin(np.abs(v - 0.55))]
    lo = v[v < fg]
    return float(fg), float(lo[np.argmin(np.abs(lo - 0.2))])


_cases = {}


def cases():
    """every case of tests/test_gpu_label_edges.py by name, built once"""
    if not _cases:
        for c in [chunk_case(G) for G in CHUNK_G] + [ragged_case_a(), ragged_case_b(), yaw_case(), z_case(True),
                                                     z_case(False), nan_case(), iou_case(), batch17_case()]:
            _cases[c.name] = c
    return _cases
