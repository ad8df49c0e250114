"""Exact-arithmetic yardstick of the sparse convolutions (SCN/CPU/Convolution.cpp:46-115, Deconvolution.cpp:7-77).

With integer-valued features, weights, bias, residual and gradients every product and every partial sum of a convolution
is exactly representable in fp32 -- in any summation order, through the MFMA, the LDS read-add-write, the split's partial
tiles and the weight gradient's reduce alike -- so a kernel must equal a float64 reference BIT FOR BIT, and a bf16 store
must be THE round-to-nearest-even bf16 of the exact sum.  This file holds the seeded operand generator, the float64
reference over the oracle's integer rule books (plain numpy), the exactness precondition (asserted, never measured: all
|terms| of an output element together stay below 2^24 granules), the expected stored values, and a comparison of bits
that reports what differs.  tests/test_conv_exact_host.py tests the yardstick itself; tests/test_gpu_conv_exact.py holds
every kernel family to it."""
import numpy as np
import torch

FP32_LIMIT = float(1 << 24)       # integers below it are exact in fp32, and so is every partial sum of terms whose
FP64_LIMIT = float(1 << 53)       # absolute values add up to less (the same with 2^53 for the fp64 statistics)


# ------------------------------------------------------------------------------------------------------- operands
class Operands(object):
    """x [rows_in, n_in] (features, or the gradient of a transposed launch), W [vol, a, b] as the layer stores it
    (a = the layer's input planes), bias / residual of the launch's output, col [n_out] the per-output-column power of
    two every term of a column is a multiple of (the granule), all float64 and all exactly representable in bf16"""

    def __init__(self, x, W, bias, residual, col, transposed):
        self.x, self.W, self.bias, self.residual, self.col, self.transposed = x, W, bias, residual, col, transposed


def rows(rng, n, planes, m_max=4, a_max=3):
    """[n, planes] of m * 2^a: integer m in [-m_max, m_max], one exponent a in {0..a_max} per row"""
    a = rng.integers(0, a_max + 1, (n, 1))
    return rng.integers(-m_max, m_max + 1, (n, planes)).astype(np.float64) * np.exp2(a)


def operands(seed, rows_in, V_out, vol, n_in, n_out, transposed=False, a_max=3, e_max=12):
    """operands of one forward-form launch n_in -> n_out planes.  `transposed`: the launch is the input-gradient form
    of a layer with n_out -> n_in planes, whose weight [vol, n_out, n_in] it reads transposed; the column scale follows
    the launch's output columns either way (columns never mix inside one sum)"""
    rng = np.random.default_rng(seed)
    x = rows(rng, rows_in, n_in, a_max=a_max)
    col = np.exp2(rng.integers(-e_max, e_max + 1, n_out))
    W = rng.integers(-4, 5, (vol, n_in, n_out)).astype(np.float64) * col
    if transposed:
        W = np.ascontiguousarray(W.transpose(0, 2, 1))
    bias = rng.integers(-4, 5, n_out) * col
    residual = rng.integers(-4, 5, (V_out, n_out)) * col
    op = Operands(x, W, bias, residual, col, transposed)
    for a in (x, W, bias, residual):
        assert np.array_equal(f32(a).astype(np.float64), a)
        assert np.array_equal(torch.from_numpy(f32(a)).bfloat16().float().numpy().astype(np.float64), a)
    return op


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def site_coords(n, seed, edge=12, batch=2):
    """[n, 4] int64 (x, y, z, sample): n distinct sites of an edge^3 cube over `batch` samples, sample-major"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(batch * edge ** 3, n, replace=False)
    b, c = pick // edge ** 3, pick % edge ** 3
    order = np.argsort(b, kind="stable")
    return np.stack([c // (edge * edge), (c // edge) % edge, c % edge, b], 1)[order].astype(np.int64)


def gather_table(rb, V_out, in_col=0):
    """[vol, V_out] int32: per offset and output row the input row of its rule, -1 where there is none"""
    t = np.full((rb.vol, V_out), -1, np.int32)
    for k in range(rb.vol):
        i, o = _pairs(rb, k, in_col)
        t[k, o] = i
    return t


# ------------------------------------------------------------------------------------------------------ reference
def _pairs(rb, k, in_col):
    p = rb.pairs(k)
    return p[:, in_col].astype(np.int64), p[:, 1 - in_col].astype(np.int64)


rule_pairs = _pairs       # (input rows, output rows) of offset k's rules


def _scatter_add(dst, idx, val):
    if len(np.unique(idx)) == len(idx):
        dst[idx] += val
    else:
        np.add.at(dst, idx, val)


def ref_forward(x, W, rb, V_out, bias=None, residual=None, in_col=0):
    """out[o] = bias + sum_k x[i] @ W[k] over offset k's rules (i, o) (+ residual), float64.  in_col = 1: the rule
    book's columns swapped (the Deconvolution reads a Convolution's book the other way round)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    out = np.zeros((V_out, W.shape[2]), np.float64)
    for k in range(rb.vol):
        i, o = _pairs(rb, k, in_col)
        if len(i):
            _scatter_add(out, o, x[i] @ W[k])
    if bias is not None:
        out += np.asarray(bias, np.float64)
    if residual is not None:
        out += np.asarray(residual, np.float64)
    return out


def ref_input_grad(g, W, rb, V_in, in_col=0):
    """d_in[i] = sum_k g[o] @ W[k]^T over offset k's rules (i, o), float64: the launch with transposed weights and (on a
    submanifold book, read from its output side) mirrored offsets -- `flags` 3"""
    g, W = np.asarray(g, np.float64), np.asarray(W, np.float64)
    d_in = np.zeros((V_in, W.shape[1]), np.float64)
    for k in range(rb.vol):
        i, o = _pairs(rb, k, in_col)
        if len(i):
            _scatter_add(d_in, i, g[o] @ W[k].T)
    return d_in


def ref_weight_grad(x, g, rb, in_col=0):
    """dW[k] = X[i]^T dY[o] over offset k's rules, d_bias = column sums of dY; float64"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    dW = np.zeros((rb.vol, x.shape[1], g.shape[1]), np.float64)
    for k in range(rb.vol):
        i, o = _pairs(rb, k, in_col)
        if len(i):
            dW[k] = x[i].T @ g[o]
    return dW, g.sum(0)


def rules_per_row(rb, V, in_col=0, side="out"):
    """number of rules of every output row (side "in": of every input row)"""
    n = np.zeros(V, np.int64)
    for k in range(rb.vol):
        i, o = _pairs(rb, k, in_col)
        np.add.at(n, o if side == "out" else i, 1)
    return n


def tile_stats(stored, T):
    """[ceil(V / T), 2, planes] float64: per tile of T rows the column sums of the stored values and of their squares"""
    s = np.asarray(stored, np.float64)
    nt = (s.shape[0] + T - 1) // T
    out = np.zeros((nt, 2, s.shape[1]), np.float64)
    for j in range(nt):
        blk = s[j * T:(j + 1) * T]
        out[j, 0], out[j, 1] = blk.sum(0), (blk * blk).sum(0)
    return out


# -------------------------------------------------------------------------------------------------- precondition
class NotExact(AssertionError):
    pass


def _require(largest, limit, what):
    if not largest < limit:
        raise NotExact("%s: the absolute terms of one sum reach %.4g granules (2^%.2f), not below 2^%d: shrink the "
                       "operand range" % (what, largest, np.log2(largest), int(np.log2(limit))))
    return float(largest)


def require_exact_forward(op, rb, V_out, bias=True, residual=True, in_col=0):
    """every output element's sum |x||w| (+ |bias| + |residual|) / granule < 2^24; returns the largest"""
    a = np.abs
    if op.transposed:
        mag = ref_input_grad(a(op.x), a(op.W), rb, V_out, in_col)
    else:
        mag = ref_forward(a(op.x), a(op.W), rb, V_out, in_col=in_col)
    if bias:
        mag = mag + a(op.bias)
    if residual:
        mag = mag + a(op.residual)
    return _require((mag / op.col).max() if mag.size else 0.0, FP32_LIMIT, "convolution")


def require_exact_weight_grad(x, g, rb, in_col=0):
    """integer x and dY: the granule is 1; sum |x||dY| per dW element and sum |dY| per column < 2^24"""
    assert np.array_equal(np.rint(x), x) and np.array_equal(np.rint(g), g)
    dW, db = ref_weight_grad(np.abs(x), np.abs(g), rb, in_col)
    return _require(max(dW.max() if dW.size else 0.0, db.max() if db.size else 0.0), FP32_LIMIT, "weight gradient")


def require_exact_stats(stored, col, T):
    """per tile: sum |v| / granule and sum v^2 / granule^2 < 2^53"""
    s = np.abs(np.asarray(stored, np.float64)) / col
    st = tile_stats(s, T)
    return _require(st.max() if st.size else 0.0, FP64_LIMIT, "statistics")


# ------------------------------------------------------------------------------------------- expected stored values
def bits(a):
    """the bit pattern of a float32 array (uint32), a torch bfloat16 tensor (uint16) or a float64 array (uint64)"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        if a.dtype == torch.bfloat16:
            return a.view(torch.int16).numpy().view(np.uint16)
        a = a.numpy()
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def to_f32_exact(ref):
    """the float64 reference narrowed to float32 -- exact under the precondition, and asserted to be"""
    r = np.asarray(ref, np.float64).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), ref), "the reference is not representable in fp32"
    return r


def bf16_rne(a32):
    """uint16 bits of torch's CPU float32 -> bfloat16 (round to nearest, ties to even)"""
    return bits(torch.from_numpy(np.ascontiguousarray(a32, np.float32)).bfloat16())


def bf16_trunc(a32):
    return (bits(np.ascontiguousarray(a32, np.float32)) >> 16).astype(np.uint16)


def bf16_ties_away(a32):
    """round to nearest, ties away from zero (finite values)"""
    return ((bits(np.ascontiguousarray(a32, np.float32)).astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)


def bf16_value(b16):
    """float32 values of bf16 bit patterns"""
    return (np.asarray(b16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def is_tie(a32):
    return (bits(np.ascontiguousarray(a32, np.float32)) & 0xffff) == 0x8000


def expect_bf16(acc_bias, residual=None):
    """bits of the stored bf16: one RNE of the exact acc + bias; with a residual the documented store-then-add form,
    bf16(float(bf16(acc + bias)) + float(residual)) -- two roundings"""
    b = bf16_rne(to_f32_exact(acc_bias))
    if residual is None:
        return b
    s = bf16_value(b).astype(np.float64) + np.asarray(residual, np.float64)
    return bf16_rne(to_f32_exact(s))      # (a bf16 plus a bf16 of the same granule: exact in fp32)


# ----------------------------------------------------------------------------------------------------- comparison
class ExactMismatch(AssertionError):
    """count: differing elements; first: [(row, column, got, want)]; truncated / other_neighbour: how many bf16
    elements are the truncation of the exact value / the neighbour of `want` on the other side; row_rules: for the first
    differing rows, how many rules they have"""

    def __init__(self, msg, count, first, truncated, other_neighbour, row_rules):
        AssertionError.__init__(self, msg)
        self.count, self.first, self.truncated, self.other_neighbour = count, first, truncated, other_neighbour
        self.row_rules = row_rules


def _as_bits(a):
    return a if isinstance(a, np.ndarray) and a.dtype.kind == "u" else bits(a)


def _value(b):
    return bf16_value(b) if b.dtype == np.uint16 else b.view(np.float32 if b.dtype == np.uint32 else np.float64)


def assert_bits(got, want, exact=None, rules=None, what="output"):
    """bit equality of every element (float32 / float64 arrays, bf16 tensors or uint16 bit patterns): no element
    skipped, no tolerance.  `exact`: the exact float32 values a bf16 `want` was rounded from; `rules`: rules per row"""
    g, w = _as_bits(got), _as_bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = g != w
    n = int(bad.sum())
    if n == 0:
        return
    g2, w2, bad2 = g.reshape(g.shape[0], -1), w.reshape(w.shape[0], -1), bad.reshape(bad.shape[0], -1)
    at = np.argwhere(bad2)[:6]
    gv, wv = _value(g2), _value(w2)
    first = [(int(r), int(c), float(gv[r, c]), float(wv[r, c])) for r, c in at]
    msg = ["%s: %d of %d elements differ in bits" % (what, n, g.size)]
    msg += ["  [%d, %d] got %r (0x%x) want %r (0x%x)" % (r, c, a, int(g2[r, c]), b, int(w2[r, c])) for r, c, a, b in first]
    trunc = other = 0
    if g.dtype == np.uint16 and exact is not None:
        t = bf16_trunc(np.asarray(exact, np.float32)).reshape(g2.shape)
        # the neighbour of `want` on the other side of the exact value: truncation when RNE rounded up, else one step up
        up = (t.astype(np.uint32) + 1).astype(np.uint16)
        neighbour = np.where(w2 == t, up, t)
        trunc = int((bad2 & (g2 == t)).sum())
        other = int((bad2 & (g2 == neighbour)).sum())
        msg.append("  of these, %d are the truncation of the exact value and %d the other neighbour of the RNE value; "
                   "%d exact values are ties" % (trunc, other, int((bad2 & is_tie(exact).reshape(g2.shape)).sum())))
    row_rules = []
    if rules is not None:
        for r in np.unique(np.argwhere(bad2)[:, 0])[:6]:
            row_rules.append((int(r), int(rules[r])))
        msg.append("  rules of the first differing rows: " + ", ".join("row %d: %d" % rr for rr in row_rules))
    raise ExactMismatch("\n".join(msg), n, first, trunc, other, row_rules)
