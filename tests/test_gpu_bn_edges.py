"""BatchNorm(+leaky ReLU) at the edges of its dispatch (csrc/bn.hip) against the fp64 yardstick of tests/fp64_yardstick.py,
in fp32 and bf16 storage, through the C ABI and through the module path.

Paths reached (bn_forward_t / bn_backward_t): the one-launch small kernels (rows 2..2048 by default, planes % 4 == 0,
16-byte aligned, own statistics) and the three-launch path (partials<·, 4|1>, finalize, apply{,1,4}); the partial count
bn_parts(rows, planes, vec) at 1, 31, 32, 33 and the 512 cap (32 planes, vector form: 128 rows per partial); plane tails
that are not a multiple of the finalize's 8 planes (12, 260) and a scalar count (9); unaligned views (a row buffer one
element in) that fall back to partials<·,1> / apply1; statistics given as fp64 partials (the convolution's epilogue
layout [nparts][2][planes]); the residual add of the backward; the mask recomputed from x (fp32) or read from the stored
output (bf16); rows 0 and 1; affine=False; leakiness 0, 0.333 and 1; negative weights; constant columns; a large common
offset; eval mode.

Bounds: fp32 outputs and input gradients within the per-element slack of the yardstick (and, where no large offset
makes the slack the only meaningful bound, within test_gpu_parity's 4e-7 / 2e-6 of the tensor's scale); parameter
gradients, saved and running statistics within their counted fp32 roundings of fp64 (<= ~1e-6 relative); bf16 stores
by assert_bf16_rounded.  n = 1 and constant columns are additionally held to the oracle (bit-equal to the reference)."""
import contextlib
import os

import numpy as np
import pytest
import torch

import fp64_yardstick as Y
import oracle_lib as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-4, 0.95
BF = torch.bfloat16
MARGINS = os.environ.get("AABR_BN_MARGINS")     # a file to append the measured err / slack ratios to


def _hip():
    import _hip
    return _hip


@contextlib.contextmanager
def _bn_small(v):
    """knob BN_SMALL: None = shipped default (2048-row cap), 0 = never the one-launch kernels, > 1 = that row cap"""
    h = _hip()
    if v is not None:
        h.set_knob("BN_SMALL", v)
    try:
        yield
    finally:
        h.set_knob("BN_SMALL", None)


def _dev(a, dtype, aligned=True):
    """a device copy in `dtype`; aligned=False: a view one element into a larger buffer (never 16-byte aligned)"""
    t = torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dtype)
    if aligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _f32(a):
    return None if a is None else _dev(a, torch.float32)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _margin(what, err, slack):
    m = slack > 0
    r = float((err[m] / slack[m]).max()) if m.any() else 0.0
    if MARGINS:
        with open(MARGINS, "a") as f:
            f.write("%s %.4f\n" % (what, r))
    return r


def _fwd(x, w, b, leak, train=True, rm=None, rv=None, parts=None, aligned=True):
    """C ABI forward: (y, save_mean, save_invstd, running_mean, running_var)"""
    h = _hip()
    lib, p = h.load(), h.ptr
    rows, planes = x.shape
    y = _dev(np.zeros(x.shape), x.dtype, aligned)
    sm, si = (torch.full((planes,), float("nan"), device=DEV) for _ in range(2))
    rm = torch.zeros(planes, device=DEV) if rm is None else _f32(rm)
    rv = torch.ones(planes, device=DEV) if rv is None else _f32(rv)
    ws = torch.empty(int(lib.aabr_bn_scratch_floats(planes)), device=DEV)
    a = (p(x), p(y), rows, planes, p(sm), p(si), p(rm), p(rv), p(w), p(b), EPS, MOM)
    bf = x.dtype == BF
    if parts is not None:
        pt = torch.as_tensor(parts).to(DEV)
        fn = lib.aabr_bn_forward_parts_bf16 if bf else lib.aabr_bn_forward_parts
        h.check(fn(*a, leak, p(pt), pt.shape[0], p(ws), h.stream()))
    else:
        fn = lib.aabr_bn_forward_bf16 if bf else lib.aabr_bn_forward
        h.check(fn(*a, int(train), leak, p(ws), h.stream()))
    torch.cuda.synchronize()
    return y, sm, si, rm, rv


def _bwd(x, y, g, sm, si, w, b, leak, add=None, parts=None, aligned=True):
    """C ABI backward: (d_in, d_weight, d_bias); d_weight / d_bias start as NaN (the kernel writes every element)"""
    h = _hip()
    lib, p = h.load(), h.ptr
    rows, planes = x.shape
    d_in = _dev(np.zeros(x.shape), x.dtype, aligned)
    dw, db = (torch.full((planes,), float("nan"), device=DEV) for _ in range(2))
    ws = torch.empty(int(lib.aabr_bn_scratch_floats(planes)), device=DEV)
    a = (p(x), p(d_in), p(y), p(g), rows, planes, p(sm), p(si), p(w), p(b), p(dw), p(db), leak)
    pt = None if parts is None else torch.as_tensor(parts).to(DEV)
    np_ = 0 if parts is None else parts.shape[0]
    if x.dtype == BF:
        if add is not None:
            h.check(lib.aabr_bn_backward_add_bf16(*a, p(pt), np_, p(ws), p(add), h.stream()))
        elif pt is not None:
            h.check(lib.aabr_bn_backward_parts_bf16(*a, p(pt), np_, p(ws), h.stream()))
        else:
            h.check(lib.aabr_bn_backward_bf16(*a, p(ws), h.stream()))
    else:
        if pt is not None:
            h.check(lib.aabr_bn_backward_parts(*a, p(pt), np_, p(ws), p(add), h.stream()))
        elif add is not None:
            h.check(lib.aabr_bn_backward_add(*a, p(ws), p(add), h.stream()))
        else:
            h.check(lib.aabr_bn_backward(*a, p(ws), h.stream()))
    torch.cuda.synchronize()
    return d_in, dw, db


def _check_fwd(what, x, y, sm, si, rm, rv, w, b, leak, train=True, rm0=None, rv0=None, parts=None, tight=True,
               undecided=0.05):
    """device forward against bn_forward_exact on the values the device read"""
    ex = Y.bn_forward_exact(_np(x), w, b, EPS, MOM, leak, train, rm0, rv0, parts)
    got = _np(y)
    if y.dtype == BF:
        Y.assert_bf16_rounded(y, ex["out"], ex["slack"], what + " out", undecided)
    else:
        err = np.abs(got - ex["out"])
        bad = err > ex["slack"]
        assert not bad.any(), "%s out: %d outside the slack, max err/slack %.3g" % (what, bad.sum(), _margin(
            what + " fwd", err, ex["slack"]))
        _margin(what + " fwd", err, ex["slack"])
        if tight and got.size:
            assert err.max() <= 4e-7 * np.abs(ex["out"]).max(), (what, err.max())
    for name, dv, want, tol in (("save_mean", sm, ex["mean"], ex["tol_mean"]), ("save_invstd", si, ex["invstd"],
                                                                                 ex["tol_invstd"]),
                                ("running_mean", rm, ex["running_mean"], ex["tol_rm"]),
                                ("running_var", rv, ex["running_var"], ex["tol_rv"])):
        d = _np(dv)
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(d), nan, err_msg="%s %s NaN pattern" % (what, name))
        e = np.abs(d - want)[~nan]
        assert (e <= tol[~nan] + 1e-30).all(), "%s %s: max err %.3g, tol %.3g" % (what, name, e.max(), tol[~nan].max())
    return ex


def _check_bwd(what, x, y, g, sm, si, w, leak, d_in, dw, db, parts=None, tight=True, undecided=0.05):
    """device backward against bn_backward_exact with the device's saved statistics and its stored output's signs"""
    ex = Y.bn_backward_exact(_np(x), _np(y), _np(g), _np(sm), _np(si), w, leak, parts)
    if d_in.dtype == BF:
        Y.assert_bf16_rounded(d_in, ex["d_in"], ex["slack"], what + " d_in", undecided)
    else:
        err = np.abs(_np(d_in) - ex["d_in"])
        r = _margin(what + " bwd", err, ex["slack"])
        assert (err <= ex["slack"]).all(), "%s d_in: max err/slack %.3g" % (what, r)
        if tight and err.size:
            assert err.max() <= 2e-6 * np.abs(ex["d_in"]).max(), (what, err.max())
    for name, dv, want, tol in (("d_weight", dw, ex["dw"], ex["tol_dw"]), ("d_bias", db, ex["db"], ex["tol_db"])):
        e = np.abs(_np(dv) - want)
        assert (e <= tol + 1e-30).all(), "%s %s: max err %.3g, tol %.3g" % (what, name, e.max(), tol.max())
    return ex


def _data(rng, rows, planes, kind="normal"):
    x = (rng.standard_normal((rows, planes)) * 1.7 + 0.4).astype(np.float32)
    if kind == "offset":              # |mean| >> std
        x = (rng.standard_normal((rows, planes)) + 300.0 * rng.choice([-1, 1], planes)).astype(np.float32)
    if kind == "constant":            # variance 0: a few exactly representable constants, every sum exact in fp32 too
        x = np.tile(np.array([0.75, -2.0, 0.0, 3.5], np.float32)[np.arange(planes) % 4], (rows, 1))
    return x


def _params(rng, planes, affine, neg):
    if not affine:
        return None, None
    w = rng.uniform(0.5, 1.5, planes).astype(np.float32)
    if neg:
        w *= rng.choice([-1, 1], planes).astype(np.float32)
    return w, rng.standard_normal(planes).astype(np.float32)


def _bn_parts(rows, planes, vec):
    """bn.hip's bn_parts"""
    pv = planes // vec
    tpr = min(pv, 256)
    rpi = 256 // tpr
    return int(min(max(-(-rows // (rpi * 4)), 1), 512))


# (rows, planes, BN_SMALL knob, aligned, data kind): the dispatch edges
CASES = [
    (1, 32, None, True, "normal"),        # n = 1: three-launch (the small kernels need rows > 1)
    (2, 32, None, True, "normal"),        # small
    (3, 12, None, True, "normal"),
    (3, 12, 0, True, "normal"),           # the same rows through the three-launch path
    (2048, 16, None, True, "normal"),     # the last row count of the small kernels
    (2048, 16, 0, True, "normal"),
    (2049, 16, None, True, "normal"),     # the first of the three-launch path
    (2049, 16, 4096, True, "normal"),     # ... and the same rows through the small kernels
    (100, 32, 0, True, "normal"),         # nparts 1
    (31 * 128, 32, None, True, "normal"),  # nparts 31
    (32 * 128, 32, None, True, "normal"),  # nparts 32 = kFinSlices
    (32 * 128 + 1, 32, None, True, "normal"),  # nparts 33
    (70000, 32, None, True, "normal"),    # nparts 547 -> the 512 cap
    (3000, 260, None, True, "normal"),    # 65 vector columns, tail of 4 planes past the finalize's 8-plane blocks
    (500, 260, None, True, "normal"),
    (3000, 9, None, True, "normal"),      # scalar forms
    (1000, 32, None, False, "normal"),    # unaligned: partials<1> / apply1 instead of the small kernels
    (5000, 12, None, False, "normal"),
    (1500, 8, None, True, "offset"),
    (5000, 8, None, True, "offset"),
    (1500, 8, None, True, "constant"),
    (5000, 8, None, True, "constant"),
]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,planes,small,aligned,kind", CASES)
def test_bn_c_abi_edges(dtype, rows, planes, small, aligned, kind):
    rng = np.random.default_rng(rows * 7 + planes + (small or 0))
    if rows == 32 * 128 + 1:
        assert [_bn_parts(r, 32, 4) for r in (100, 31 * 128, 32 * 128, 32 * 128 + 1, 70000)] == [1, 31, 32, 33, 512]
    x = _dev(_data(rng, rows, planes, kind), dtype, aligned)
    g = _dev(rng.standard_normal((rows, planes)).astype(np.float32), dtype, aligned)
    # the scale-relative bounds of test_gpu_parity hold where no cancellation makes the per-element slack the only
    # meaningful bound: not with a large offset, not at n <= 2 (two rows normalise to +-1 whatever x: d_in is ~0)
    tight = kind == "normal" and rows > 2
    undecided = 0.05 if tight else 1.0
    # cycle affine / leakiness / sign of the weights over the cases
    i = CASES.index((rows, planes, small, aligned, kind))
    affine, leak, neg = [(True, 0.0, False), (True, 0.333, True), (False, 1.0, False), (True, 1.0, True),
                         (False, 0.0, False), (True, 0.1, False)][i % 6]
    w, b = _params(rng, planes, affine, neg)
    wd, bd = _f32(w), _f32(b)
    what = "%s %dx%d small=%s aligned=%d %s affine=%d leak=%g" % (dtype, rows, planes, small, aligned, kind, affine, leak)
    with _bn_small(small):
        y, sm, si, rm, rv = _fwd(x, wd, bd, leak, aligned=aligned)
        _check_fwd(what, x, y, sm, si, rm, rv, w, b, leak, tight=tight, undecided=undecided)
        d_in, dw, db = _bwd(x, y, g, sm, si, wd, bd, leak, aligned=aligned)
        _check_bwd(what, x, y, g, sm, si, w, leak, d_in, dw, db, tight=tight, undecided=undecided)
        # the residual add folded into the backward's write-out == backward, then add, with its stated rounding
        add = _dev(rng.standard_normal((rows, planes)).astype(np.float32), dtype, aligned)
        d_sum, dw2, db2 = _bwd(x, y, g, sm, si, wd, bd, leak, add=add, aligned=aligned)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    if dtype == BF:   # bf16(bf16(gradient) + add): fp32 sum of the two stored bf16 values, then one RNE
        want = Y.bf16_rne((_np(d_in).astype(np.float32) + _np(add).astype(np.float32)).astype(np.float64))
    else:
        want = (_np(d_in).astype(np.float32) + _np(add).astype(np.float32)).astype(np.float64)
    np.testing.assert_array_equal(_np(d_sum), want, err_msg=what + " residual add")
    if kind == "constant" or rows == 1:
        _check_against_oracle(what, x, y, sm, si, rm, rv, w, b, leak, d_in, g)


def _check_against_oracle(what, x, y, sm, si, rm, rv, w, b, leak, d_in, g):
    """n = 1 and variance-0 columns: the device produces what the reference does (the oracle is bit-equal to it,
    tests/test_oracle_ref_kernels.py): the same saved and running statistics -- the 0 / 0 of n = 1 included --, the
    same output (bias where x == mean) and a zero input gradient at n = 1"""
    xs = _np(x).astype(np.float32)
    out, osm, osi, orm, orv = O.bn_fwd(xs, w, b, np.zeros(xs.shape[1]), np.ones(xs.shape[1]), EPS, MOM, True, leak)
    np.testing.assert_array_equal(_np(sm), osm, err_msg=what + " save_mean vs oracle")
    np.testing.assert_allclose(_np(si), osi, rtol=4 * 2.0 ** -24, err_msg=what + " save_invstd vs oracle")
    np.testing.assert_array_equal(_np(rm), orm, err_msg=what + " running_mean vs oracle")
    np.testing.assert_allclose(_np(rv), orv, rtol=2 * 2.0 ** -24, err_msg=what + " running_var vs oracle")  # NaN == NaN
    # the oracle does the device's fp32 operations in the same order: within both sides' slack of the exact value
    slack = Y.bn_forward_exact(xs, w, b, EPS, MOM, leak)["slack"]
    bound = 2 * slack + (2.0 ** -8 * np.abs(out) if y.dtype == BF else 0)
    assert (np.abs(_np(y) - out) <= bound).all(), what + " out vs oracle"
    if xs.shape[0] == 1:
        d_ref, *_ = O.bn_bwd(xs, _np(y).astype(np.float32), _np(g).astype(np.float32), osm, osi, w, leak)
        np.testing.assert_array_equal(d_ref, 0)
        np.testing.assert_array_equal(_np(d_in), 0)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_bn_rows_zero(dtype):
    """nActive == 0: the forward leaves everything untouched, the backward zeroes d_weight / d_bias"""
    planes = 16
    x = torch.empty((0, planes), dtype=dtype, device=DEV)
    w, b = torch.ones(planes, device=DEV), torch.zeros(planes, device=DEV)
    rm0, rv0 = np.full(planes, 0.25, np.float32), np.full(planes, 2.0, np.float32)
    y, sm, si, rm, rv = _fwd(x, w, b, 0.0, rm=rm0, rv=rv0)
    assert y.numel() == 0 and torch.isnan(sm).all() and torch.isnan(si).all()
    np.testing.assert_array_equal(_np(rm), rm0)
    np.testing.assert_array_equal(_np(rv), rv0)
    sm.fill_(0.0), si.fill_(1.0)
    _, dw, db = _bwd(x, x, x, sm, si, w, b, 0.0)
    assert (dw == 0).all() and (db == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,planes,nparts", [(3000, 32, 37), (1500, 12, 600), (900, 64, 1)])
def test_bn_given_partials(dtype, rows, planes, nparts):
    """aabr_bn_forward_parts[_bf16] / aabr_bn_backward_parts[_bf16]: the statistics as fp64 partial sums in the
    convolution epilogue's [nparts][2][planes] layout (tiles of consecutive rows; more than kMaxParts allowed), built by
    numpy; the partial count here wraps the finalize's 32 slices unevenly"""
    rng = np.random.default_rng(rows + nparts)
    xs = _data(rng, rows, planes)
    x = _dev(xs, dtype)
    x64 = _np(x)
    tiles = np.array_split(np.arange(rows), nparts)
    fparts = np.stack([np.stack([x64[t].sum(0), (x64[t] ** 2).sum(0)]) for t in tiles])
    w, b = _params(rng, planes, True, True)
    wd, bd = _f32(w), _f32(b)
    leak = 0.333
    y, sm, si, rm, rv = _fwd(x, wd, bd, leak, parts=fparts)
    what = "%s parts %dx%d/%d" % (dtype, rows, planes, nparts)
    _check_fwd(what, x, y, sm, si, rm, rv, w, b, leak, parts=fparts)
    g = _dev(rng.standard_normal((rows, planes)).astype(np.float32), dtype)
    d = np.where(_np(y) > 0, _np(g), _np(g) * float(np.float32(leak)))
    xm = x64 - _np(sm)
    bparts = np.stack([np.stack([d[t].sum(0), (xm[t] * d[t]).sum(0)]) for t in tiles])
    d_in, dw, db = _bwd(x, y, g, sm, si, wd, bd, leak, parts=bparts)
    _check_bwd(what, x, y, g, sm, si, w, leak, d_in, dw, db, parts=bparts)
    if dtype == BF:   # the residual form with given partials
        add = _dev(rng.standard_normal((rows, planes)).astype(np.float32), dtype)
        d_sum, _, _ = _bwd(x, y, g, sm, si, wd, bd, leak, add=add, parts=bparts)
        want = Y.bf16_rne((_np(d_in).astype(np.float32) + _np(add).astype(np.float32)).astype(np.float64))
        np.testing.assert_array_equal(_np(d_sum), want)


def _module_input(x):
    import sparseconvnet as scn
    t = scn.SparseConvNetTensor()
    t.features = x
    return t


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,rows,planes", [("BatchNormalization", 700, 32), ("BatchNormalization-noaffine", 3000, 12),
                                              ("BatchNormReLU", 2049, 64), ("BatchNormLeakyReLU", 1800, 260),
                                              ("BatchNormLeakyReLU", 6000, 10)])
def test_bn_module_train_and_eval(dtype, kind, rows, planes):
    """scn.BatchNormalization / BatchNormReLU / BatchNormLeakyReLU: training forward and backward (the saved statistics
    read back from the autograd node), the running statistics, then eval mode on them"""
    import sparseconvnet as scn
    rng = np.random.default_rng(rows + planes)
    if kind == "BatchNormReLU":
        bn, leak = scn.BatchNormReLU(planes, momentum=MOM), 0.0
    elif kind == "BatchNormLeakyReLU":
        bn, leak = scn.BatchNormLeakyReLU(planes, momentum=MOM, leakiness=0.2), 0.2
    else:
        bn, leak = scn.BatchNormalization(planes, momentum=MOM, affine=kind == "BatchNormalization"), 1.0
    bn = bn.to(DEV)
    rm0 = rng.standard_normal(planes).astype(np.float32) * 0.1
    bn.running_mean.copy_(torch.as_tensor(rm0))
    if bn.affine:
        w = rng.uniform(-1.5, 1.5, planes).astype(np.float32)
        b = rng.standard_normal(planes).astype(np.float32)
        bn.weight.data.copy_(torch.as_tensor(w))
        bn.bias.data.copy_(torch.as_tensor(b))
    else:
        w = b = None
    x = _dev(_data(rng, rows, planes), dtype).requires_grad_(True)
    y = bn(_module_input(x)).features
    assert y.dtype == dtype
    saved = y.grad_fn.saved_tensors
    sm, si = saved[6], saved[7]
    what = "module %s %s %dx%d" % (kind, dtype, rows, planes)
    _check_fwd(what, x, y, sm, si, bn.running_mean, bn.running_var, w, b, leak, rm0=rm0)
    g = _dev(rng.standard_normal((rows, planes)).astype(np.float32), dtype)
    y.backward(g)
    if bn.affine:
        _check_bwd(what, x, y, g, sm, si, w, leak, x.grad, bn.weight.grad, bn.bias.grad)
    else:
        _check_bwd_d_in_only(what, x, y, g, sm, si, leak)
    rm1, rv1 = _np(bn.running_mean), _np(bn.running_var)
    bn.eval()
    with torch.no_grad():
        ye = bn(_module_input(x.detach())).features
    ex = Y.bn_forward_exact(_np(x), w, b, EPS, MOM, leak, False, rm1, rv1)
    if dtype == BF:
        Y.assert_bf16_rounded(ye, ex["out"], ex["slack"], what + " eval")
    else:
        err = np.abs(_np(ye) - ex["out"])
        assert (err <= ex["slack"]).all(), (what, _margin(what + " eval", err, ex["slack"]))
        _margin(what + " eval", err, ex["slack"])


def _check_bwd_d_in_only(what, x, y, g, sm, si, leak):
    ex = Y.bn_backward_exact(_np(x), _np(y), _np(g), _np(sm), _np(si), None, leak)
    if x.grad.dtype == BF:
        Y.assert_bf16_rounded(x.grad, ex["d_in"], ex["slack"], what + " d_in")
    else:
        err = np.abs(_np(x.grad) - ex["d_in"])
        assert (err <= ex["slack"]).all(), (what, _margin(what + " bwd", err, ex["slack"]))
        _margin(what + " bwd", err, ex["slack"])
