"""Pins the NUMERICAL half of oracle/scn_oracle.c to the reference's OWN CPU kernels
(SCN/CPU/BatchNormalization.cpp, IOLayers.cpp, Convolution.cpp gather/scatter + at::matmul,
SparseToDense.cpp), through what those kernels returned on the inputs built below: tests/golden/ref_kernels_golden.npz,
written by tests/golden/gen_ref_golden.py from oracle/_ref/libref_kernels.so (the reference sources compiled where
they lie, recipe: oracle/Makefile, harness: oracle/ref_kernels_harness.cpp).  The tests read the stored vectors only.

Bars: BatchNorm fwd/bwd and InputLayer fwd/bwd BIT-EQUAL (same sequential fp32 arithmetic; compared by SHA-256 of the
reference's bits); conv / deconv fwd + bwd within 1e-5 relative (the reference contracts with at::matmul = MKL sgemm,
whose summation order is not specified; the oracle accumulates in double): the vectors keep, per array, the
reference's max |r| and its distance to the exact (float64) contraction on the same rule book, so that
|oracle - exact| < 1e-5 max|r| - |r - exact| implies |oracle - r| < 1e-5 max|r|; SparseToDense exact (SHA-256)."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O
import synth_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels_golden.npz")
STALE = "inputs differ from those the golden vectors were made from (tests/golden/gen_ref_golden.py)"


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------ inputs (shared with the generator)
BN_CASES = [(1, 4), (2, 32), (777, 32), (5000, 128), (66094, 32)]
INPUT_CASES = [(300, 4), (6000, 20), (79998, 20)]
SUBM_CASES = [(9, 32, 3), (32, 32, 3), (32, 64, 3), (64, 128, 1), (16, 16, (3, 1, 5))]
STRIDED_CASES = [((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((1, 1, 8), (1, 1, 1))]


def bn_cases(rows, planes, affine):
    """yields (train, x, weight, bias, running mean, running var, d_out)"""
    rng = np.random.default_rng(rows * 131 + planes)
    x = (rng.standard_normal((rows, planes)) * 2 + 0.3).astype(np.float32)
    w = rng.uniform(0.5, 1.5, planes).astype(np.float32) if affine else None
    b = rng.standard_normal(planes).astype(np.float32) if affine else None
    rm0 = rng.standard_normal(planes).astype(np.float32)
    rv0 = rng.uniform(0.5, 2, planes).astype(np.float32)
    for train in ([True, False] if rows > 1 else [False]):
        yield train, x, w, b, rm0, rv0, rng.standard_normal((rows, planes)).astype(np.float32)


def bn_key(rows, planes, affine, leak, train):
    return "bn/%dx%d/affine%d/leak%g/train%d/" % (rows, planes, affine, leak, train)


def input_layer_case(mode, npts, scale):
    locs, feats = S.make_batch(2 if npts < 50000 else 1, npts, 3, scale)
    il = O.input_layer(locs, feats, mode)
    d_out = np.random.default_rng(5).standard_normal((il["V"], feats.shape[1])).astype(np.float32)
    return locs, feats, il, d_out


def _scene(npts, scale, seed=0, bs=2):
    locs, feats = S.make_batch(bs, npts, seed, scale)
    il = O.input_layer(locs, feats, 4)
    return il


def subm_case(nin, nout, filt):
    """(V, rule book, x, W, d_out)"""
    il = _scene(4000, 20)
    V = il["V"]
    size = [filt] * 3 if isinstance(filt, int) else list(filt)
    rb = O.submanifold_rules(il["coords"], size)
    rng = np.random.default_rng(nin * 7 + nout)
    x = rng.standard_normal((V, nin)).astype(np.float32)
    W = (rng.standard_normal((rb.vol, nin, nout)) * np.sqrt(2.0 / (nin * rb.vol))).astype(np.float32)
    d_out = rng.standard_normal((V, nout)).astype(np.float32)
    return V, rb, x, W, d_out


def strided_case(size, stride):
    """(V, Vo, rule book, x, W, d_out, y, d_up): convolution fine -> coarse, deconvolution coarse -> fine"""
    il = _scene(3000, 10)
    V = il["V"]
    sp_in = np.array([64, 64, 8]) if size == (1, 1, 8) else np.array(S.FULL_SCALE)
    coords = il["coords"].copy()
    if size == (1, 1, 8):
        coords[:, :3] = coords[:, :3] % sp_in
        _, uniq = np.unique(coords, axis=0, return_index=True)
        coords = coords[np.sort(uniq)]
        V = coords.shape[0]
    out_sp = (sp_in - np.array(size)) // np.array(stride) + 1
    rb, out_coords = O.convolution_rules(coords, size, stride, out_sp)
    Vo = out_coords.shape[0]
    nin, nout = 32, 48
    rng = np.random.default_rng(11)
    x = rng.standard_normal((V, nin)).astype(np.float32)
    W = (rng.standard_normal((rb.vol, nin, nout)) * 0.1).astype(np.float32)
    d_out = rng.standard_normal((Vo, nout)).astype(np.float32)
    y = rng.standard_normal((Vo, nin)).astype(np.float32)
    d_up = rng.standard_normal((V, nout)).astype(np.float32)
    return V, Vo, rb, x, W, d_out, y, d_up


def rules_digest(rb):
    return digest(np.concatenate([rb.counts.astype(np.int64)] +
                                 [rb.rules[k, :int(rb.counts[k])].reshape(-1).astype(np.int64) for k in range(rb.vol)]))


def exact_fwd(x, W, rb, n_out_rows, in_col=0):
    """out[R[:, 1 - in_col]] += x[R[:, in_col]] @ W[k] per offset k, in float64"""
    out = np.zeros((n_out_rows, W.shape[2]))
    for k in range(rb.vol):
        r = rb.rules[k, :int(rb.counts[k])]
        np.add.at(out, r[:, 1 - in_col], x[r[:, in_col]].astype(np.float64) @ W[k].astype(np.float64))
    return out


def exact_bwd(x, d_out, W, rb, in_col=0):
    """(d_in, dW) of exact_fwd, in float64"""
    d_in, dW = np.zeros(x.shape), np.zeros(W.shape)
    for k in range(rb.vol):
        r = rb.rules[k, :int(rb.counts[k])]
        xi, do = x[r[:, in_col]].astype(np.float64), d_out[r[:, 1 - in_col]].astype(np.float64)
        dW[k] = xi.T @ do
        np.add.at(d_in, r[:, in_col], do @ W[k].T.astype(np.float64))
    return d_in, dW


def s2d_case():
    """(points, features, spatial size, batch, d_dense)"""
    rng = np.random.default_rng(2)
    sp = np.array([12, 10, 6], np.int64)
    B, planes = 3, 7
    pts = np.unique(np.stack([rng.integers(0, sp[0], 400), rng.integers(0, sp[1], 400), rng.integers(0, sp[2], 400),
                              np.sort(rng.integers(0, B, 400))], 1), axis=0)
    pts = pts[np.argsort(pts[:, 3], kind="stable")]
    feats = rng.standard_normal((pts.shape[0], planes)).astype(np.float32)
    d_dense = rng.standard_normal((B, planes) + tuple(int(v) for v in sp)).astype(np.float32)
    return pts, feats, sp, B, d_dense


def _close(ref, key, o, exact):
    """|o - r| < 1e-5 max|r| for the reference's r, from its stored max|r| and |r - exact|"""
    M, dev = float(ref[key + "max"]), float(ref[key + "dev"])
    err = float(np.abs(o.astype(np.float64) - exact).max()) if o.size else 0.0
    assert err < 1e-5 * M - dev, (key, err / M, dev / M)


# ------------------------------------------------------------------ BatchNorm: bit-equal
@pytest.mark.parametrize("rows,planes", BN_CASES)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("leak", [0.0, 0.333])
def test_bn_forward_backward_bit_equal(ref, rows, planes, affine, leak):
    for train, x, w, b, rm0, rv0, d_out in bn_cases(rows, planes, affine):
        key = bn_key(rows, planes, affine, leak, train)
        assert digest(x) + digest(d_out) == str(ref[key + "inputs"]), STALE
        o_out, o_sm, o_si, o_rm, o_rv = O.bn_fwd(x, w, b, rm0, rv0, 1e-4, 0.95, train, leak)
        for a, name in ((o_out, "out"), (o_sm, "saveMean"), (o_si, "saveInvStd"), (o_rm, "runningMean"),
                        (o_rv, "runningVar")):
            assert digest(a) == str(ref[key + name]), (name, train)
        # backward on the (bit-equal) forward state
        o_din, o_dw, o_db, o_dmask = O.bn_bwd(x, o_out, d_out, o_sm, o_si, w, leak)
        assert digest(o_din) == str(ref[key + "d_in"]), train
        assert digest(o_dmask) == str(ref[key + "d_out_masked"]), train   # in-place mask
        assert digest(o_dw) == str(ref[key + "d_weight"]), train
        assert digest(o_db) == str(ref[key + "d_bias"]), train


# ------------------------------------------------------------------ InputLayer: bit-equal
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("npts,scale", INPUT_CASES)
def test_input_layer_forward_backward_bit_equal(ref, mode, npts, scale):
    locs, feats, il, d_out = input_layer_case(mode, npts, scale)
    key = "input/mode%d/%d/%d/" % (mode, npts, scale)
    assert digest(feats.astype(np.float32)) + digest(il["rules"]) + digest(d_out) == str(ref[key + "inputs"]), STALE
    assert digest(il["out"]) == str(ref[key + "out"])
    assert digest(O.input_layer_bwd(il, d_out)) == str(ref[key + "d_in"])


def test_input_layer_empty(ref):
    """zero points: the reference's forward returned an empty [0, 9] output; so does the oracle's"""
    il = O.input_layer(np.zeros((0, 4), np.int64), np.zeros((0, 9), np.float32), 4)
    assert il["V"] == int(ref["input/empty/rows"]) == 0
    assert il["out"].shape == (0, 9) and digest(il["out"]) == str(ref["input/empty/out"])


# ------------------------------------------------------------------ conv / deconv: 1e-5
@pytest.mark.parametrize("nin,nout,filt", SUBM_CASES)
def test_submanifold_conv_matches_reference_kernels(ref, nin, nout, filt):
    V, rb, x, W, d_out = subm_case(nin, nout, filt)
    key = "subm/%d/%d/%s/" % (nin, nout, filt)
    assert rules_digest(rb) + digest(x) + digest(W) + digest(d_out) == str(ref[key + "inputs"]), STALE
    o_out, o_macs = O.conv_fwd(x, W, rb, V)
    assert o_macs == float(ref[key + "macs"]) == float(rb.total) * nin * nout
    _close(ref, key + "out/", o_out, exact_fwd(x, W, rb, V))
    o_din, o_dW, _ = O.conv_bwd(x, d_out, W, rb)
    e_din, e_dW = exact_bwd(x, d_out, W, rb)
    _close(ref, key + "d_in/", o_din, e_din)
    _close(ref, key + "dW/", o_dW, e_dW)


@pytest.mark.parametrize("size,stride", STRIDED_CASES)
def test_strided_conv_and_deconv_match_reference_kernels(ref, size, stride):
    V, Vo, rb, x, W, d_out, y, d_up = strided_case(size, stride)
    key = "strided/%s/%s/" % (size, stride)
    assert rules_digest(rb) + "".join(digest(a) for a in (x, W, d_out, y, d_up)) == str(ref[key + "inputs"]), STALE
    # Convolution: in rows = column 0, out rows = column 1
    o_out, _ = O.conv_fwd(x, W, rb, Vo)
    _close(ref, key + "out/", o_out, exact_fwd(x, W, rb, Vo))
    o_din, o_dW, _ = O.conv_bwd(x, d_out, W, rb)
    e_din, e_dW = exact_bwd(x, d_out, W, rb)
    _close(ref, key + "d_in/", o_din, e_din)
    _close(ref, key + "dW/", o_dW, e_dW)
    # Deconvolution (CPU/Deconvolution.cpp:15-16): same book, columns swapped: coarse rows in, fine rows out
    o_up, _ = O.conv_fwd(y, W, rb, V, in_col=1)
    _close(ref, key + "up/", o_up, exact_fwd(y, W, rb, V, in_col=1))
    o_dy, o_dW2, _ = O.conv_bwd(y, d_up, W, rb, in_col=1)
    e_dy, e_dW2 = exact_bwd(y, d_up, W, rb, in_col=1)
    _close(ref, key + "d_y/", o_dy, e_dy)
    _close(ref, key + "dW_up/", o_dW2, e_dW2)


# ------------------------------------------------------------------ SparseToDense: exact
def test_sparse_to_dense_matches_reference_kernels(ref):
    pts, feats, sp, B, d_dense = s2d_case()
    assert digest(pts) + digest(feats) + digest(d_dense) == str(ref["s2d/inputs"]), STALE
    o_dense = O.sparse_to_dense(pts, feats, sp, B)
    assert o_dense.shape == d_dense.shape
    assert digest(o_dense) == str(ref["s2d/dense"])
    assert digest(O.sparse_to_dense_bwd(pts, d_dense, feats.shape[1], sp)) == str(ref["s2d/d_in"])
