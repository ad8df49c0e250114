"""Cases that push the grid and rule-book builders (csrc/geometry.hip, csrc/geom.h, csrc/brick.hip) past everyday sizes,
and a second reference for the rule books.

The cases are sized from the kernels' own constants, read out of the sources, so that a case stays on the side of a
threshold its name says when a constant moves.  tests/test_geometry_edges_host.py asserts that every case is what its
name says (no GPU needed); tests/test_gpu_geometry_edges.py runs them on the device.

`brute_rules` restates the two rule books from the definitions -- the region calculators of the reference
(SCN/Metadata/RectangularRegions.h:95-119, SubmanifoldConvolutionRules.h:26-45, ConvolutionRules.h:11-34) and the order
contract at the top of csrc/geometry.hip -- over a plain dictionary.  It shares no code with oracle/scn_oracle.c; the host
twin holds the two against each other on the small cases before either judges the device.  Integer work throughout: every
comparison built on this module is exact."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "automatic-as-built-reconstruction_amd", "csrc")


# ---------------------------------------------------------------------------------------------------- the kernels' constants
def _constant(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, text)
    assert m is not None, "constant %s not found" % name
    return int(m.group(1))


def _read_constants():
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("geometry.hip", "brick.hip", "common.h")}
    k = {n: _constant(text["geometry.hip"], n) for n in ("kScanThreads", "kScanItems", "kInlinePrefixBlocks")}
    k.update({n: _constant(text["brick.hip"], n) for n in ("kBsThreads", "kBsItems")})
    k["kMaxCoord"] = _constant(text["common.h"], "kMaxCoord")
    return k


K = _read_constants()
SCAN_TILE = K["kScanThreads"] * K["kScanItems"]              # candidates per scan block
INLINE_LIMIT = K["kInlinePrefixBlocks"] * SCAN_TILE          # the last candidate count without k_scan_blockprefix
PREFIX_STEP = 1024                                           # blocks per trip of k_scan_blockprefix's loop (its block size)
BRICK_CHUNK = K["kBsThreads"] * K["kBsItems"]                # bricks per chunk of k_brick_scan
BRICK_LOOKBACK = 64 * BRICK_CHUNK                            # bricks one round of the look-back covers
MAX_COORD = K["kMaxCoord"]


def max_samples():
    """SCN.MAX_SAMPLES: a level keeps its per-sample offsets when its samples are 0 .. MAX_SAMPLES at the most"""
    from sparseconvnet import SCN
    return SCN.MAX_SAMPLES


def max_outputs(size, stride):
    """output sites one input site can reach (csrc/geom.h make_geom)"""
    n = 1
    for a, b in zip(size, stride):
        n *= (a + b - 1) // b
    return n


def conv_out_spatial(extent, size, stride):
    return tuple((e - f) // s + 1 for e, f, s in zip(extent, size, stride))


def scan_blocks(candidates):
    return (max(candidates, 1) + SCAN_TILE - 1) // SCAN_TILE


# ---------------------------------------------------------------------------------------------------- case builder
def draw_sites(seed, extent, counts):
    """counts[b] DISTINCT cells of `extent` for sample b, drawn without replacement (0 = an empty sample): int64 [V, 4]
    (x, y, z, sample), sample-major, the rows of a sample in random order.  V is exactly sum(counts)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod([int(e) for e in extent]))
    out = []
    for b, c in enumerate(counts):
        if c == 0:
            continue
        assert c <= n, "sample %d: %d sites do not fit %s" % (b, c, extent)
        pick = rng.choice(n, size=int(c), replace=False)
        x, r = np.divmod(pick, extent[1] * extent[2])
        y, z = np.divmod(r, extent[2])
        out.append(np.stack([x, y, z, np.full_like(x, b)], 1))
    coords = np.concatenate(out).astype(np.int64) if out else np.zeros((0, 4), np.int64)
    assert len(np.unique(site_key(coords))) == len(coords) == sum(counts)
    return coords


def _box(cells, room):
    """an extent with odd and even sides that holds about `room` times `cells` cells"""
    side = int(np.ceil((float(room) * cells) ** (1.0 / 3.0)))
    return (side + 3, side | 1, max(side - 2, 1))


def site_key(c):
    """one uint64 per (x, y, z, sample) row, 16 bits each: the whole key range (sample 65534 included) fits"""
    c = np.asarray(c, np.int64).reshape(-1, 4).astype(np.uint64)
    return (c[:, 3] << np.uint64(48)) | (c[:, 0] << np.uint64(32)) | (c[:, 1] << np.uint64(16)) | c[:, 2]


def _split(total, parts):
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


# A: the scan boundary.  Strided 3/2: eight candidates per input site; FullConvolution 3/2: twenty-seven.
A_SIZE, A_STRIDE = (3, 3, 3), (2, 2, 2)
A_MAXOUT = max_outputs(A_SIZE, A_STRIDE)
A_EDGE = INLINE_LIMIT // A_MAXOUT                     # input sites of the last inline case
A_STRIDED = {"last inline": A_EDGE, "first prefix": A_EDGE + 1, "prefix": A_EDGE + A_EDGE // 4}
A_FULL_VOL = int(np.prod(A_SIZE))
A_FULL_PER_SAMPLE = (INLINE_LIMIT // A_FULL_VOL) // 2 + 91      # two live samples: about 180 sites past the boundary

# B: filter volumes above 64 (the brick table builders' second pass of 64 offsets)
B_EXTENT = (23, 22, 21)
B_COUNTS = (1334, 1333, 1333)
B_SUBMANIFOLD = {"5x5x5": (5, 5, 5), "3x5x7": (3, 5, 7)}
B_STRIDED = {"5x5x5 / 3": ((5, 5, 5), (3, 3, 3)), "4x4x5 / 2": ((4, 4, 5), (2, 2, 2))}

# C: many samples
C_EXTENT = (12, 10, 8)
C_SIZE = C_STRIDE = (2, 2, 2)
C_POINTS = 3000

# D: the ends of the key range
D_SPATIAL = (MAX_COORD + 1,) * 3
_M = MAX_COORD
D_SITES = [(0, 0, 0), (1, 0, 0), (_M, _M, _M), (_M - 1, _M, _M), (_M, _M, _M - 1)]
D_STRIDED = {"2/2": ((2, 2, 2), (2, 2, 2)), "3/2": ((3, 3, 3), (2, 2, 2))}

# E: more occupied bricks than one round of the brick scan's look-back covers
E_EXTENT = (512, 512, 64)
E_SITES = BRICK_LOOKBACK + BRICK_LOOKBACK // 4

ORDERS = ("first_seen", "brick")


def c_case_names():
    m = max_samples()
    return ["%d samples%s" % (nb, tail) for nb in (m + 1, m + 2, m + 9) for tail in ("", ", three empty")]


def _c_counts(name):
    nb = int(name.split()[0])
    counts = [C_POINTS // nb + (b * 7) % 5 - 2 for b in range(nb)]
    if name.endswith("three empty"):
        for b in (1, nb // 2, nb - 1):
            counts[b] = 0
    return counts


_CASES = {}


def case(name):
    """dict(coords, extent, counts, ...) of a case; built once, never changed"""
    if name in _CASES:
        return _CASES[name]
    if name.startswith("A strided "):
        v = A_STRIDED[name[len("A strided "):]]
        counts = _split(v, 2)
        extent = _box(max(counts), 40)        # thin: new output sites keep turning up until the last scan block
        c = dict(coords=draw_sites(len(name) + v, extent, counts), extent=extent, counts=counts, size=A_SIZE,
                 stride=A_STRIDE, out_spatial=conv_out_spatial(extent, A_SIZE, A_STRIDE), maxout=A_MAXOUT)
    elif name == "A full":
        counts = [A_FULL_PER_SAMPLE, 0, A_FULL_PER_SAMPLE]       # the empty middle sample of test_gpu_full_conv.py
        extent = _box(A_FULL_PER_SAMPLE, 3)
        c = dict(coords=draw_sites(41, extent, counts), extent=extent, counts=counts, size=A_SIZE, stride=A_STRIDE,
                 out_spatial=tuple((e - 1) * s + f for e, f, s in zip(extent, A_SIZE, A_STRIDE)), maxout=A_FULL_VOL)
    elif name == "B":
        c = dict(coords=draw_sites(42, B_EXTENT, B_COUNTS), extent=B_EXTENT, counts=list(B_COUNTS))
    elif name.startswith("C "):
        counts = _c_counts(name[2:])
        c = dict(coords=draw_sites(43 + len(counts), C_EXTENT, counts), extent=C_EXTENT, counts=counts, size=C_SIZE,
                 stride=C_STRIDE, out_spatial=conv_out_spatial(C_EXTENT, C_SIZE, C_STRIDE))
    elif name == "D":
        rows = [p + (b,) for b in (0, 1) for p in D_SITES] + [D_SITES[0] + (_M,), D_SITES[2] + (_M,)]
        c = dict(coords=np.array(rows, np.int64), extent=D_SPATIAL, counts=None)
    elif name == "E":
        counts = _split(E_SITES, 2)
        c = dict(coords=draw_sites(44, E_EXTENT, counts), extent=E_EXTENT, counts=counts, size=(2, 2, 2), stride=(2, 2, 2),
                 out_spatial=conv_out_spatial(E_EXTENT, (2, 2, 2), (2, 2, 2)))
    else:
        raise KeyError(name)
    c["coords"].setflags(write=False)
    _CASES[name] = c
    return c


def occupied_bricks(coords):
    """number of 4 x 4 x 4 bricks (csrc/geom.h) that hold a site"""
    c = np.array(coords, np.int64).reshape(-1, 4)
    c[:, :3] >>= 2
    return len(np.unique(site_key(c)))


# ---------------------------------------------------------------------------------------------------- the second reference
def _offsets(size):
    return [(a, b, c) for a in range(size[0]) for b in range(size[1]) for c in range(size[2])]      # z fastest


def brute_rules(coords, size, stride=None, out_sp=None, kind="submanifold"):
    """(out_coords int64 [V_out, 4], rules) of a rule book over the sites `coords` (int [V, 4]: x, y, z, sample; distinct).
    rules = the set of (k, in_row, out_row), k = the filter offset with z fastest.

    "submanifold": the output sites are the input sites; site o at p gathers, at offset (dx, dy, dz), the site at
    p + (dx, dy, dz) - size // 2 of the same sample (InputRegionCalculator_Submanifold).
    "strided": input site u at p reaches the output points lb .. ub per axis, lb = max(0, (p - size + stride) / stride)
    with C's division, ub = min(out_sp - 1, p / stride) (OutputRegionCalculator); a point not seen before in the sample is
    the next output site -- input rows ascending, then the region with z fastest; the rule's offset is p - o * stride
    (InputRegionCalculator: the window of output o starts at o * stride)."""
    coords = [tuple(int(v) for v in r) for r in np.asarray(coords, np.int64).reshape(-1, 4)]
    rows = {}
    for i, (x, y, z, b) in enumerate(coords):
        assert (b, x, y, z) not in rows, "the sites must be distinct"
        rows[(b, x, y, z)] = i
    rules = set()
    if kind == "submanifold":
        h = [s // 2 for s in size]
        for o, (x, y, z, b) in enumerate(coords):
            for k, (dx, dy, dz) in enumerate(_offsets(size)):
                u = rows.get((b, x + dx - h[0], y + dy - h[1], z + dz - h[2]))
                if u is not None:
                    rules.add((k, u, o))
        return np.array(coords, np.int64).reshape(-1, 4), rules
    assert kind == "strided"

    def span(p, i):
        num = p - size[i] + stride[i]
        q = num // stride[i] if num >= 0 else -((-num) // stride[i])          # C division: toward zero
        return range(max(0, q), min(out_sp[i] - 1, p // stride[i]) + 1)
    out_rows = {}
    for u, (x, y, z, b) in enumerate(coords):
        for ox in span(x, 0):
            for oy in span(y, 1):
                for oz in span(z, 2):
                    o = out_rows.setdefault((b, ox, oy, oz), len(out_rows))
                    d = (x - ox * stride[0], y - oy * stride[1], z - oz * stride[2])
                    assert all(0 <= d[i] < size[i] for i in range(3))
                    rules.add(((d[0] * size[1] + d[1]) * size[2] + d[2], u, o))
    out = np.array([(k[1], k[2], k[3], k[0]) for k in out_rows], np.int64).reshape(-1, 4)     # dicts keep insertion order
    return out, rules


def rules_by_offset(rules, vol):
    """the set of brute_rules as a list over offsets of sorted int64 keys in_row << 32 | out_row"""
    per = [[] for _ in range(vol)]
    for k, u, o in rules:
        per[k].append((u << 32) | o)
    return [np.sort(np.array(p, np.int64)) for p in per]


def pair_keys(rows_in, rows_out):
    """sorted int64 keys in_row << 32 | out_row of a list of rules"""
    return np.sort((np.asarray(rows_in, np.int64) << 32) | np.asarray(rows_out, np.int64))
