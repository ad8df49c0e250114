"""Plain numpy restatement of the batched input layer (BLInputLayer / BLOutputLayer), written from its semantics:

  coords int64 [B, L, 3], features float32 [B, L, C]; point i is the flat row i = b * L + l.
  * A row is EMPTY if and only if its x is negative (y and z are not looked at).  It belongs to no site.
  * Sites are numbered sample by sample; inside a sample by first appearance in ascending l.  The same coordinate in two
    samples is two sites.  The layer has exactly B samples.
  * Every site keeps the ascending list of its points; what the rule book LISTS depends on the mode:
      0  every point (all rows present and unique is the caller's promise),   3, 4  every point,
      1  only the LAST point of a site,                                          2  only the FIRST.
  * forward (fp32): out[site] = sum over the listed points, ascending, of  mult * in[point]  -- multiply, then add, each
    rounded to fp32; mult = 1 / count (rounded to fp32) in mode 4, else 1.  Accumulation starts at 0.
  * backward: d_in[point] = 0 + mult * d_out[site] for every listed point, exactly zero for every other row.
  * BLOutputLayer: the backward pass with mult = 1 in every mode; its gradient is the forward pass with mult = 1.

Nothing here looks at the library: it is what the tests hold the kernels to."""
import numpy as np


def bl_rules(coords, mode):
    """coords int [B, L, 3] -> dict:
    site_coords int64 [V, 4] (x, y, z, b) in site order, sample_off [B + 1] (first site of every sample), point_site
    int64 [B * L] (-1: no site), points: per site the ascending flat indices of ALL its points, listed: per site the flat
    indices the mode's rule book lists, max_active: the longest listed row, rules int32 [V, 1 + max_active] = (count,
    listed points.., zero padded)"""
    assert mode in (0, 1, 2, 3, 4)
    coords = np.asarray(coords, np.int64)
    B, L = coords.shape[:2]
    site_coords, points, sample_off = [], [], [0]
    point_site = np.full(B * L, -1, np.int64)
    for b in range(B):
        seen = {}
        for l in range(L):
            x, y, z = (int(v) for v in coords[b, l])
            if x < 0:
                continue
            assert y >= 0 and z >= 0, "a present row with a negative y or z is an error, not a case of this model"
            v = seen.get((x, y, z))
            if v is None:
                v = seen[(x, y, z)] = len(site_coords)
                site_coords.append((x, y, z, b))
                points.append([])
            points[v].append(b * L + l)
            point_site[b * L + l] = v
        sample_off.append(len(site_coords))
    if mode == 1:
        listed = [p[-1:] for p in points]
    elif mode == 2:
        listed = [p[:1] for p in points]
    else:
        listed = [list(p) for p in points]
    V = len(points)
    max_active = max([len(p) for p in listed], default=0)
    rules = np.zeros((V, 1 + max_active), np.int32)
    for v, p in enumerate(listed):
        rules[v, 0] = len(p)
        rules[v, 1:1 + len(p)] = p
    return dict(B=B, L=L, V=V, mode=mode, site_coords=np.array(site_coords, np.int64).reshape(V, 4),
                sample_off=np.array(sample_off, np.int64), point_site=point_site, points=points, listed=listed,
                max_active=max_active, rules=rules)


def _mult(count, average):
    return np.float32(1.0) / np.float32(count) if average else np.float32(1.0)


def forward(rb, feats, average=None):
    """out float32 [V, C]; `average` defaults to (mode == 4)"""
    average = (rb["mode"] == 4) if average is None else average
    f = np.ascontiguousarray(feats, np.float32).reshape(rb["B"] * rb["L"], -1)
    out = np.zeros((rb["V"], f.shape[1]), np.float32)
    for v, pts in enumerate(rb["listed"]):
        m = _mult(len(pts), average)
        acc = np.zeros(f.shape[1], np.float32)
        for p in pts:
            acc = (acc + (m * f[p]).astype(np.float32)).astype(np.float32)
        out[v] = acc
    return out


def backward(rb, d_out, average=None):
    """d_in float32 [B, L, C]"""
    average = (rb["mode"] == 4) if average is None else average
    d_out = np.ascontiguousarray(d_out, np.float32)
    C = d_out.shape[1]
    d_in = np.zeros((rb["B"] * rb["L"], C), np.float32)
    for v, pts in enumerate(rb["listed"]):
        m = _mult(len(pts), average)
        for p in pts:
            d_in[p] = (np.float32(0.0) + (m * d_out[v]).astype(np.float32)).astype(np.float32)
    return d_in.reshape(rb["B"], rb["L"], C)


def output_layer(rb, site_feats):
    """BLOutputLayer: float32 [B, L, C]"""
    return backward(rb, site_feats, average=False)


def output_layer_grad(rb, d_out):
    """gradient of BLOutputLayer with respect to the site rows: float32 [V, C]"""
    return forward(rb, np.asarray(d_out, np.float32), average=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
