"""numpy restatement of the six pooling passes (MaxPooling, AveragePooling, UnPooling; forward and backward) from
reference-format rule pairs: `rules[k]` = int array [n_k, 2] of (input row, output row) for filter offset k, as
`oracle_lib.convolution_rules(...).pairs(k)` gives them -- independent of the device's gather tables.

The semantics are the reference's CPU kernels' (SCN/CPU/MaxPooling.cpp, AveragePooling.cpp, UnPooling.cpp), offsets in
ascending order, every operation a single np.float32 operation (no float64 intermediate, no np.add.at): inside one offset
a row appears at most once on either side (asserted), so one offset is one vectorised fp32 statement.

  max      out starts at +0; `if out < x: out = x`        -> max(0, inputs); a NaN input is ignored
  average  out += x / float32(vol)                         (vol = number of offsets, empty ones included)
  unpool   fine += coarse                                  over the book (fine, coarse): pairs are (fine row, coarse row)
  max backward   dx[in] += dy[out] where y[out] == x[in]   (+0 == -0, NaN never matches), on the columns the forward read

`nFeaturesToDrop` (`drop`): the forward reads columns [drop, C); gradients are full width with zeros in the dropped columns.
`store="bf16"`: the inputs hold bf16-representable values, the arithmetic is the same fp32 arithmetic, and the result is
rounded ONCE, to nearest even, to a bf16-representable float32 (`round_bf16`)."""
import numpy as np


def round_bf16(a):
    """float32 -> the nearest bf16-representable float32 (ties to even); NaN stays a quiet NaN"""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    r = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    r = np.where(np.isnan(a), (bits >> 16) | 0x40, r)
    return (r.astype(np.uint32) << 16).view(np.float32).reshape(a.shape)


def _store(a, store):
    assert store in ("fp32", "bf16")
    return round_bf16(a) if store == "bf16" else a


def _pairs(rules):
    """per offset (first column, second column) as int64 index arrays, each free of repeats"""
    out = []
    for r in rules:
        r = np.asarray(r, np.int64).reshape(-1, 2)
        a, b = r[:, 0], r[:, 1]
        assert len(np.unique(a)) == len(a) and len(np.unique(b)) == len(b), "a row twice in one offset"
        out.append((a, b))
    return out


def max_forward(x, rules, n_out, drop=0, store="fp32"):
    x = np.asarray(x, np.float32)
    y = np.zeros((n_out, x.shape[1] - drop), np.float32)
    for i, o in _pairs(rules):
        xi, yo = x[i, drop:], y[o]
        y[o] = np.where(yo < xi, xi, yo)
    return _store(y, store)


def max_backward(x, y, dy, rules, drop=0, store="fp32"):
    x, y, dy = (np.asarray(a, np.float32) for a in (x, y, dy))
    dx = np.zeros_like(x)
    for i, o in _pairs(rules):
        hit = y[o] == x[i, drop:]
        cur = dx[i, drop:]
        dx[i, drop:] = np.where(hit, cur + dy[o], cur)
    return _store(dx, store)


def average_forward(x, rules, n_out, drop=0, store="fp32"):
    x = np.asarray(x, np.float32)
    vol = np.float32(len(rules))
    y = np.zeros((n_out, x.shape[1] - drop), np.float32)
    for i, o in _pairs(rules):
        y[o] = y[o] + x[i, drop:] / vol
    return _store(y, store)


def average_backward(dy, rules, n_in, drop=0, store="fp32"):
    dy = np.asarray(dy, np.float32)
    vol = np.float32(len(rules))
    dx = np.zeros((n_in, dy.shape[1] + drop), np.float32)
    for i, o in _pairs(rules):
        dx[i, drop:] = dx[i, drop:] + dy[o] / vol
    return _store(dx, store)


def unpool_forward(x, rules, n_fine, drop=0, store="fp32"):
    """x: coarse rows; rules: (fine row, coarse row) pairs of the book (fine -> coarse)"""
    x = np.asarray(x, np.float32)
    y = np.zeros((n_fine, x.shape[1] - drop), np.float32)
    for f, c in _pairs(rules):
        y[f] = y[f] + x[c, drop:]
    return _store(y, store)


def unpool_backward(dy, rules, n_coarse, drop=0, store="fp32"):
    dy = np.asarray(dy, np.float32)
    dx = np.zeros((n_coarse, dy.shape[1] + drop), np.float32)
    for f, c in _pairs(rules):
        dx[c, drop:] = dx[c, drop:] + dy[f]
    return _store(dx, store)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
