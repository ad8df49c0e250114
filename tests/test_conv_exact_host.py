"""The exact-arithmetic yardstick of tests/conv_exact.py, tested without a GPU: its float64 reference equals the oracle
(SCN/CPU/Convolution.cpp:46-185, fp32 accumulation -- exact on these operands) bit for bit; the precondition refuses
operands whose sums leave the exact range; every way a kernel is known to go subtly wrong (a lost rule, a lost channel,
swapped offsets, a truncating or ties-away store, one rounding where two are documented, statistics of unrounded values)
fails the comparison and is reported as what it is; and the generated bf16 outputs hold enough ties and enough values
where truncation and round-to-nearest-even differ for the GPU test to tell the rounding modes apart."""
import copy

import numpy as np
import pytest

import conv_exact as E
import oracle_lib as O


def _sites(n, seed):
    il = O.input_layer(E.site_coords(n, seed), np.zeros((n, 1), np.float32), 4)
    assert il["V"] == n
    return il["coords"]


def _book(kind, n=700):
    sites = _sites(n, 7 + n)
    if kind == "sub3":
        return O.submanifold_rules(sites, [3, 3, 3]), n, n
    if kind == "one":
        return O.submanifold_rules(sites, [1, 1, 1]), n, n
    rb, oc = O.convolution_rules(sites, [2, 2, 2], [2, 2, 2], [6, 6, 6])
    return rb, n, oc.shape[0]


@pytest.mark.parametrize("kind", ["sub3", "strided", "one"])
@pytest.mark.parametrize("n_in,n_out", [(32, 64), (128, 32)])
def test_reference_equals_the_oracle_bit_for_bit(kind, n_in, n_out):
    rb, V_in, V_out = _book(kind)
    op = E.operands(n_in + n_out, V_in, V_out, rb.vol, n_in, n_out)
    E.require_exact_forward(op, rb, V_out, residual=False)
    ref = E.ref_forward(op.x, op.W, rb, V_out, op.bias)
    got, _ = O.conv_fwd(E.f32(op.x), E.f32(op.W), rb, V_out, E.f32(op.bias))
    E.assert_bits(got, E.to_f32_exact(ref), rules=E.rules_per_row(rb, V_out))
    assert np.abs(ref).max() > 0
    # backward: integer gradients (granule 1 for dW and d_bias); the input gradient's columns are the layer's input
    # planes, so its operands are generated as a transposed launch n_out -> n_in
    ot = E.operands(n_in * 3 + n_out, V_out, V_in, rb.vol, n_out, n_in, transposed=True)
    E.require_exact_forward(ot, rb, V_in, bias=False, residual=False)
    rng = np.random.default_rng(5)
    xi = E.rows(rng, V_in, n_in)
    E.require_exact_weight_grad(xi, ot.x, rb)
    d_in, dW, db = O.conv_bwd(E.f32(xi), E.f32(ot.x), E.f32(ot.W), rb, want_bias=True)
    E.assert_bits(d_in, E.to_f32_exact(E.ref_input_grad(ot.x, ot.W, rb, V_in)))
    rW, rb_ = E.ref_weight_grad(xi, ot.x, rb)
    E.assert_bits(dW, E.to_f32_exact(rW))
    E.assert_bits(db, E.to_f32_exact(rb_))
    if kind == "strided":       # the transposed layer: the same book with its columns swapped (Deconvolution.cpp:15-16)
        od = E.operands(11, V_out, V_in, rb.vol, n_in, n_out)
        E.require_exact_forward(od, rb, V_in, residual=False, in_col=1)
        got, _ = O.conv_fwd(E.f32(od.x), E.f32(od.W), rb, V_in, E.f32(od.bias), in_col=1)
        E.assert_bits(got, E.to_f32_exact(E.ref_forward(od.x, od.W, rb, V_in, od.bias, in_col=1)))
        gt = E.operands(12, V_in, V_out, rb.vol, n_out, n_in, transposed=True)
        xc = E.rows(rng, V_out, n_in)
        d_in, dW, db = O.conv_bwd(E.f32(xc), E.f32(gt.x), E.f32(gt.W), rb, in_col=1, want_bias=True)
        E.assert_bits(d_in, E.to_f32_exact(E.ref_input_grad(gt.x, gt.W, rb, V_out, in_col=1)))
        E.assert_bits(dW, E.to_f32_exact(E.ref_weight_grad(xc, gt.x, rb, in_col=1)[0]))


def test_precondition_refuses_operands_outside_the_exact_range():
    rb, V_in, V_out = _book("sub3")
    ok = E.operands(1, V_in, V_out, rb.vol, 128, 64)
    assert E.require_exact_forward(ok, rb, V_out) < 2.0 ** 21
    wide = E.operands(1, V_in, V_out, rb.vol, 128, 64, a_max=20)          # rows up to 4 * 2^20: sums pass 2^24
    with pytest.raises(E.NotExact):
        E.require_exact_forward(wide, rb, V_out)
    rng = np.random.default_rng(2)
    x, g = E.rows(rng, V_in, 32, a_max=12), E.rows(rng, V_out, 32, a_max=12)
    with pytest.raises(E.NotExact):
        E.require_exact_weight_grad(x, g, rb)
    with pytest.raises(E.NotExact):
        E.require_exact_stats(np.full((64, 4), 2.0 ** 30), np.ones(4), 64)
    assert E.require_exact_stats(np.full((64, 4), 2.0 ** 20), np.ones(4), 64) == 64 * 2.0 ** 40


@pytest.fixture(scope="module")
def case():
    rb, V_in, V_out = _book("sub3")
    op = E.operands(3, V_in, V_out, rb.vol, 128, 64)
    E.require_exact_forward(op, rb, V_out)
    acc = E.ref_forward(op.x, op.W, rb, V_out, op.bias)
    return rb, V_out, op, acc


def _mismatch(got, want, **kw):
    with pytest.raises(E.ExactMismatch) as e:
        E.assert_bits(got, want, **kw)
    assert e.value.count > 0 and len(e.value.first) > 0 and "differ in bits" in str(e.value)
    return e.value


def test_a_lost_rule_a_lost_channel_and_swapped_offsets_are_rejected(case):
    rb, V, op, acc = case
    want = E.to_f32_exact(acc)
    nrules = E.rules_per_row(rb, V)
    E.assert_bits(E.to_f32_exact(E.ref_forward(op.x, op.W, rb, V, op.bias)), want)
    # one rule of one output row
    k = int(np.argmax(rb.counts > 3))
    row = int(rb.rules[k, 2, 1])
    less = copy.copy(rb)
    less.rules, less.counts = rb.rules.copy(), rb.counts.copy()
    less.rules[k, 2:rb.counts[k] - 1] = rb.rules[k, 3:rb.counts[k]]
    less.counts[k] -= 1
    e = _mismatch(E.to_f32_exact(E.ref_forward(op.x, op.W, less, V, op.bias)), want, rules=nrules)
    assert {r for r, _, _, _ in e.first} == {row} and e.row_rules == [(row, int(nrules[row]))]
    assert e.count <= want.shape[1]
    # one input channel of one offset
    W = op.W.copy()
    W[5, 17, :] = 0
    e = _mismatch(E.to_f32_exact(E.ref_forward(op.x, W, rb, V, op.bias)), want, rules=nrules)
    assert e.count > rb.counts[5]
    # two offsets' weight slices swapped
    W = op.W.copy()
    W[[3, 4]] = W[[4, 3]]
    _mismatch(E.to_f32_exact(E.ref_forward(op.x, W, rb, V, op.bias)), want, rules=nrules)
    # and in bf16 storage the lost rule still shows after the rounding
    _mismatch(E.expect_bf16(E.ref_forward(op.x, op.W, less, V, op.bias)), E.expect_bf16(acc))


def test_rounding_faults_are_rejected_and_named(case):
    rb, V, op, acc = case
    exact = E.to_f32_exact(acc)
    want = E.expect_bf16(acc)
    E.assert_bits(E.bf16_rne(exact), want, exact=exact)
    # one 64-row tile truncated instead of rounded
    got = want.copy()
    got[64:128] = E.bf16_trunc(exact[64:128])
    e = _mismatch(got, want, exact=exact)
    assert e.truncated == e.count and all(64 <= r < 128 for r, _, _, _ in e.first)
    assert "truncation" in str(e)
    # ties resolved away from even: exactly the ties whose even neighbour lies towards zero
    e = _mismatch(E.bf16_ties_away(exact), want, exact=exact)
    tie = E.is_tie(exact)
    assert e.count == int((tie & (E.bf16_trunc(exact) == want)).sum()) and e.other_neighbour == e.count
    # the residual: rounded once instead of twice
    two = E.expect_bf16(acc, op.residual)
    one = E.bf16_rne(E.to_f32_exact(acc + op.residual))
    e = _mismatch(one, two)
    assert e.count > 0.01 * two.size
    # statistics of the unrounded values
    stored = E.bf16_value(want)
    E.require_exact_stats(stored, op.col, 64)
    e = _mismatch(E.tile_stats(acc, 64), E.tile_stats(stored, 64), what="statistics")
    assert e.count > 0


@pytest.mark.parametrize("n_in", [32, 128, 256])
def test_generated_outputs_decide_the_rounding_mode(n_in):
    """at least 5 % of the exact sums lie on a bf16 tie and for at least 10 % truncation and RNE differ"""
    rb, V_in, V_out = _book("sub3")
    op = E.operands(40 + n_in, V_in, V_out, rb.vol, n_in, 64)
    E.require_exact_forward(op, rb, V_out)
    exact = E.to_f32_exact(E.ref_forward(op.x, op.W, rb, V_out, op.bias))
    ties = E.is_tie(exact).mean()
    differ = (E.bf16_rne(exact) != E.bf16_trunc(exact)).mean()
    print("n_in %d: ties %.3f, RNE != truncation %.3f" % (n_in, ties, differ))
    assert ties >= 0.05 and differ >= 0.10
