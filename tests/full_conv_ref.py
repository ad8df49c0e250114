"""Plain-numpy restatement of the FullConvolution / TransposeConvolution geometry, written from
SCN/Metadata/FullConvolutionRules.h:11-57 (with InputRegionCalculator, RectangularRegions.h:95-105, and
RectangularRegion::offset, :30-38).

The reference walks the input sites of a sample, and for each the points `p * stride + q`, q in [0, size) with the last
axis fastest; a point not seen before in the sample becomes the next output site, and (input row, output row) is appended
to the rules of offset q.  Its input walk is the iteration order of a google::dense_hash_map, an artefact; here the input
rows are walked in ascending order and the output map is insertion-ordered (a dict), which gives the first-seen
convention the device path documents: input rows ascending, then offsets with z fastest, samples contiguous.  The second
half is the brick-major order rule of csrc/geom.h, as tests/test_gpu_brick.py states it."""
import numpy as np


def out_spatial(in_spatial, size, stride):
    return tuple((int(i) - 1) * int(s) + int(f) for i, f, s in zip(in_spatial, size, stride))


def offsets(size):
    """[vol, 3] filter offsets in rule order: z fastest"""
    return np.array([(a, b, c) for a in range(size[0]) for b in range(size[1]) for c in range(size[2])], np.int64)


class RuleBook(object):
    """rules[k] = int32 [n_k, 2] of (input row, output row); the interface tests/conv_exact.py reads (`vol`, `pairs`)"""

    def __init__(self, rules):
        self.rules = rules
        self.vol = len(rules)

    def pairs(self, k):
        return self.rules[k]

    def total(self):
        return sum(len(r) for r in self.rules)


def full_convolution_rules(in_coords, size, stride):
    """in_coords int [V_in, 4] (x, y, z, sample), samples contiguous and ascending.
    Returns (out_coords int64 [V_out, 4] in first-seen order, RuleBook)."""
    in_coords = np.asarray(in_coords, np.int64).reshape(-1, 4)
    assert (np.diff(in_coords[:, 3]) >= 0).all(), "samples must be contiguous and ascending"
    offs = offsets(size)
    stride = np.asarray(stride, np.int64)
    seen = {}                  # (sample, x, y, z) -> output row; one map with the sample in the key = one map per sample
    out = []                   # with a running counter (FullConvolutionRules.h:46-54)
    rules = [[] for _ in range(len(offs))]
    for u, (x, y, z, b) in enumerate(in_coords.tolist()):
        base = (x * stride[0], y * stride[1], z * stride[2])
        for k, (dx, dy, dz) in enumerate(offs.tolist()):
            key = (b, base[0] + dx, base[1] + dy, base[2] + dz)
            row = seen.get(key)
            if row is None:
                row = seen[key] = len(out)
                out.append((key[1], key[2], key[3], b))
            rules[k].append((u, row))
    out = np.array(out, np.int64).reshape(-1, 4)
    return out, RuleBook([np.array(r, np.int32).reshape(-1, 2) for r in rules])


def tables(rb, V_in, V_out):
    """the two gather tables of the book: t_out [vol, V_in] -- the new-level row input row u reaches at offset k (complete
    by construction) -- and t_in [vol, V_out] -- the input row that reaches new-level row o at offset k, or -1"""
    t_out = np.full((rb.vol, V_in), -1, np.int32)
    t_in = np.full((rb.vol, V_out), -1, np.int32)
    for k in range(rb.vol):
        r = rb.pairs(k)
        t_out[k, r[:, 0]] = r[:, 1]
        t_in[k, r[:, 1]] = r[:, 0]
    return t_out, t_in


def scatter(x, W, rb, V_out, bias=None):
    """out[o] (+)= x[i] @ W[k] over the rules, float64; W [vol, nIn, nOut]"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    out = np.zeros((V_out, W.shape[2]), np.float64)
    for k in range(rb.vol):
        r = rb.pairs(k)
        if len(r):
            np.add.at(out, r[:, 1].astype(np.int64), x[r[:, 0].astype(np.int64)] @ W[k])
    if bias is not None:
        out += np.asarray(bias, np.float64)
    return out


def densify(coords, feats, spatial, batch):
    """[batch, planes, X, Y, Z] float64"""
    feats = np.asarray(feats, np.float64)
    d = np.zeros((batch, feats.shape[1]) + tuple(spatial), np.float64)
    c = np.asarray(coords, np.int64)
    d[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]] = feats
    return d


# ---- brick-major order (csrc/geom.h; tests/test_gpu_brick.py _brick_major_key) -------------------------------------------
def brick_major_key(c):
    """batch, super-brick (x, y, z), brick in super-brick, cell in brick"""
    c = np.asarray(c, np.int64)
    x, y, z, b = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    sb = ((b * 5000 + (x >> 4)) * 5000 + (y >> 4)) * 5000 + (z >> 4)
    bit = (((x >> 2) & 3) << 4) | (((y >> 2) & 3) << 2) | ((z >> 2) & 3)
    cell = ((x & 3) << 4) | ((y & 3) << 2) | (z & 3)
    return (sb * 64 + bit) * 64 + cell


def coord_key(c):
    c = np.asarray(c, np.int64)
    return ((c[:, 3] * 70000 + c[:, 0]) * 70000 + c[:, 1]) * 70000 + c[:, 2]


def match_rows(dev_coords, ref_coords):
    """reference row of every device row; asserts that the two lists hold the same set of sites"""
    kd, kr = coord_key(dev_coords), coord_key(ref_coords)
    assert len(kd) == len(kr), "site counts differ: %d vs %d" % (len(kd), len(kr))
    assert len(np.unique(kd)) == len(kd), "a site is listed twice"
    if len(kd) == 0:
        return np.zeros(0, np.int64)
    order = np.argsort(kr)
    pos = np.minimum(np.searchsorted(kr[order], kd), len(kr) - 1)
    assert (kr[order][pos] == kd).all(), "site sets differ"
    return order[pos]


def input_sites(seed, spatial, samples, density):
    """distinct sites of a `spatial` grid for every sample of `samples` (a list of flags: False = an EMPTY sample),
    int64 [V, 4], sample-major, rows of a sample in random order"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(spatial))
    out = []
    for b, live in enumerate(samples):
        if not live:
            continue
        pick = rng.permutation(n)[:max(1, int(round(density * n)))]
        x, r = np.divmod(pick, spatial[1] * spatial[2])
        y, z = np.divmod(r, spatial[2])
        out.append(np.stack([x, y, z, np.full_like(x, b)], 1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 4), np.int64)
