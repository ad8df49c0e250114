"""The bf16 rounding checker and the BatchNorm fp64 yardstick of tests/fp64_yardstick.py, on the CPU: the checker accepts
torch's bf16 conversion and rejects truncation and a one-ulp shift; the yardstick agrees with a plain restatement and
with torch's own batch norm."""
import numpy as np
import torch

import fp64_yardstick as Y


def _values(rng, n):
    """random fp64 values over many binades, both signs, plus exact bf16 values and exact midpoints"""
    v = rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))
    exact = Y.bf16_rne(v[: n // 8])
    mid = exact + np.sign(exact) * np.ldexp(1.0, np.frexp(exact)[1] - 9)
    return np.concatenate([v, exact, mid, [0.0, -0.0, 2.0 ** -130, -(2.0 ** -133) * 3]])


def _torch_bf16(v):
    return torch.as_tensor(v, dtype=torch.float64).to(torch.bfloat16).double().numpy()


def _truncate(v):
    """bf16 by dropping the low 16 bits of the fp32 pattern (round toward zero)"""
    b = np.asarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def test_bf16_rne_matches_torch_on_float32_values():
    """on values an fp32 register can hold, torch's conversion is one RNE: bf16_rne must reproduce it exactly"""
    rng = np.random.default_rng(0)
    v = _values(rng, 200000).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(Y.bf16_rne(v), _torch_bf16(v.astype(np.float32)))


def test_bf16_rne_ties_to_even():
    one = 1.0 + 2.0 ** -8                  # midpoint of 1 and 1 + 2^-7: 1 has the even significand
    three = 1.0 + 3 * 2.0 ** -8            # midpoint of 1 + 2^-7 and 1 + 2^-6: the latter is even
    np.testing.assert_array_equal(Y.bf16_rne([one, -one, three, -three]), [1.0, -1.0, 1 + 2.0 ** -6, -1 - 2.0 ** -6])
    # the largest value below 2 rounds up into the next binade
    assert Y.bf16_rne(2.0 - 2.0 ** -9) == 2.0
    # bf16 subnormals are spaced 2^-133
    assert Y.bf16_rne(2.0 ** -133 * 2.4) == 2.0 ** -133 * 2


def test_checker_accepts_torch_conversion_of_fp64():
    """torch converts fp64 through fp32: an fp32 computation of the value within u|v| of it, which is the slack"""
    rng = np.random.default_rng(1)
    v = _values(rng, 200000)
    ok, _ = Y.check_bf16_rounded(_torch_bf16(v), v, Y.U * np.abs(v))
    assert ok.all()
    _, undecided = Y.check_bf16_rounded(_torch_bf16(v[:200000]), v[:200000], Y.U * np.abs(v[:200000]))
    assert undecided < 1e-3                 # the random part (the rest are exact values and midpoints by construction)
    Y.assert_bf16_rounded(torch.as_tensor(v).to(torch.bfloat16), v, Y.U * np.abs(v), "torch", max_undecided=0.11)


def test_checker_rejects_truncation_and_one_ulp_shift():
    rng = np.random.default_rng(2)
    v = rng.standard_normal(100000) * np.exp2(rng.integers(-20, 20, 100000))
    slack = 4 * Y.U * np.abs(v)
    rne = _torch_bf16(v)
    trunc = _truncate(v)
    ok, _ = Y.check_bf16_rounded(trunc, v, slack)
    differs = trunc != rne
    assert differs.mean() > 0.4
    decided = Y.bf16_rne(v - slack) == Y.bf16_rne(v + slack)
    assert decided.mean() > 0.999
    assert not ok[differs & decided].any()  # every truncation that is not the RNE result is caught where decided
    rne = Y.bf16_rne(v)
    ulp = np.ldexp(1.0, np.frexp(rne)[1] - 8)
    for shifted in (rne + ulp, rne - ulp):
        ok, _ = Y.check_bf16_rounded(shifted, v, slack)
        assert not ok[decided].any()
    # a value that is not a bf16 at all (fp32 left unrounded)
    ok, _ = Y.check_bf16_rounded(v.astype(np.float32).astype(np.float64), v, slack)
    assert ok.mean() < 0.01
    # the assertion form reports the failure
    try:
        Y.assert_bf16_rounded(trunc, v, slack, "truncated")
    except AssertionError as e:
        assert "truncated" in str(e)
    else:
        raise AssertionError("truncation accepted")


def test_checker_straddling_slack_allows_both_neighbours_only():
    lo, hi = 1.0, 1.0 + 2.0 ** -7
    mid = 0.5 * (lo + hi)
    v = np.array([mid + 1e-9, mid - 1e-9])
    ok, undecided = Y.check_bf16_rounded([lo, hi], v, 2e-9)     # both sides of the midpoint within the slack
    assert ok.all() and undecided == 1.0
    ok, _ = Y.check_bf16_rounded([lo, lo], v, 1e-10)            # slack clear of the midpoint: RNE only
    assert list(ok) == [False, True]
    ok, _ = Y.check_bf16_rounded([hi + 2.0 ** -7], [mid], 2e-9)  # never two ulps away
    assert not ok.any()


def test_bn_yardstick_matches_restatement_and_torch():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((700, 12)) * 1.7 + 0.4).astype(np.float32)
    w = rng.uniform(-1.5, 1.5, 12).astype(np.float32)
    b = rng.standard_normal(12).astype(np.float32)
    leak = 0.333
    f = Y.bn_forward_exact(x, w, b, 1e-4, 0.95, leak)
    xt = torch.as_tensor(x, dtype=torch.float64).requires_grad_()
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_()
    bt = torch.as_tensor(b, dtype=torch.float64).requires_grad_()
    rm, rv = torch.zeros(12, dtype=torch.float64), torch.ones(12, dtype=torch.float64)
    y = torch.nn.functional.batch_norm(xt, rm, rv, wt, bt, True, 1 - float(np.float32(0.95)), float(np.float32(1e-4)))
    out = torch.nn.functional.leaky_relu(y, float(np.float32(leak)))
    np.testing.assert_allclose(f["out"], out.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f["running_mean"], rm.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(f["running_var"], rv.numpy(), rtol=1e-12)
    g = rng.standard_normal(x.shape)
    out.backward(torch.as_tensor(g))
    bwd = Y.bn_backward_exact(x, f["out"], g, f["mean"], f["invstd"], w, leak)
    # the yardstick reads the saved statistics at fp32; torch keeps them exact: agreement to that rounding
    np.testing.assert_allclose(bwd["d_in"], xt.grad.numpy(), rtol=0, atol=1e-5 * np.abs(bwd["d_in"]).max())
    np.testing.assert_allclose(bwd["dw"], wt.grad.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(bwd["db"], bt.grad.numpy(), rtol=1e-12, atol=1e-12)
    # partial sums in the convolution's [nparts][2][planes] layout give the same statistics
    x64 = x.astype(np.float64)
    parts = np.stack([np.stack([c.sum(0), (c * c).sum(0)]) for c in np.array_split(x64, 7)])
    fp = Y.bn_forward_exact(x, w, b, 1e-4, 0.95, leak, parts=parts)
    np.testing.assert_allclose(fp["out"], f["out"], rtol=1e-11, atol=1e-11)
    # eval mode normalises by the running statistics; affine=False is weight 1, bias 0
    e = Y.bn_forward_exact(x, None, None, 1e-4, 0.95, 1.0, train=False, running_mean=f["running_mean"],
                           running_var=f["running_var"])
    rm32, rv32 = Y.f32(f["running_mean"]), Y.f32(f["running_var"])
    np.testing.assert_allclose(e["out"], (x64 - rm32) / np.sqrt(rv32 + Y.f32(1e-4)), rtol=1e-12, atol=1e-12)
    # n == 1: the reference's 0 / 0 in the running variance
    one = Y.bn_forward_exact(x[:1], w, b, 1e-4, 0.95, leak)
    assert np.isnan(one["running_var"]).all() and (one["var"] == 0).all()
