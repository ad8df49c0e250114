"""fp64 yardsticks shared by the BatchNorm and RPN-loss tests, and the bf16 rounding checker.

BatchNorm (SCN/CPU/BatchNormalization.cpp:12-107, csrc/bn.hip): the exact forward / backward of the operation the kernel
performs, in float64, with every scalar parameter (eps, momentum, leakiness, weight, bias) taken at the float32 value the
kernel receives.  Each function also returns a per-element SLACK: a bound on how far the kernel's own fp32 arithmetic
(after its fp64 statistics) may move a result from the exact value.  The bounds are counted operation by operation below,
with u = 2^-24 (half an fp32 ulp, relative) and bn.hip compiled with -ffp-contract=off (no fused multiply-adds).

assert_bf16_rounded(got, exact64, slack): a bf16 store of a value the device holds in fp32 within `slack` of `exact64`
must be the round-to-nearest-even bf16 of SOME value in [exact64 - slack, exact64 + slack].  RNE is monotone, so the
allowed stores are the bf16 values from RNE(exact64 - slack) to RNE(exact64 + slack): where the slack stays clear of a
midpoint that is exactly RNE(exact64); where it straddles one, either bf16 neighbour.  Truncation, a double rounding
through an intermediate coarser than fp32, or a one-ulp shift is rejected wherever the slack is clear of a midpoint,
which is almost everywhere: the checker reports the fraction of elements where it could not decide, and the callers
assert that fraction is small.
"""
import numpy as np

U = 2.0 ** -24            # half an fp32 ulp, relative

# forward apply, y = x*a + c with a = invstd*w, c = bias - mean*a, then the activation.  Per element the kernel computes
#   mean_f = fl(mean)                                  |err| <= u |mean|
#   t = fl(fl(var) + eps)                              2u relative
#   invstd_f = powf(t, -0.5)                           u (from t) + 2 ulp of powf (4u)   -> 5u relative
#   w_f = fl(invstd_f * weight)                        6u relative                          (|a|)
#   c_f = fl(fl(-mean_f * w_f) + bias)                 (1 + 6 + 1) u |mean a| + u |c|
#   y_f = fl(fl(x * w_f) + c_f)                        (6 + 1) u |x a| + |c_f - c| + u |y|
#   out = y_f > 0 ? y_f : fl(y_f * leak)               + u |y leak|,  0 <= leak <= 1
# With |c| <= |mean a| + |bias| and |y| <= |x a| + |mean a| + |bias|:
#   |out_f - out| <= 11 u (|x a| + |mean a| + |bias|)
# plus what the fp64 statistics carry in: the sums' rounding, (n + 2) 2^-53 of sum |x| and sum x^2, which matters only
# for a large common offset (|mean| >> std: the one-pass variance cancels) -- added per plane as var_rel / mean_err.
K_FWD = 11
# backward apply, with the saved mean_f / invstd_f as given inputs (the reference's backward reads them too):
#   d = mask ? g : fl(g leak)                          u |d| where rounded (never for leakiness 0 or 1); R = their sum |d|
#   s = sum d (fp64), dp = sum fl(x - mean_f) d (fp64, the products exact)
#                                                      |ds| <= u R,  |ddp| <= 2u P,  P = sum |(x - mean) d|
#   gm = fl(s / n)                                     u |s|/n + u R/n
#   kk = fl(fl(fl(fl(dp) is) is) / n)                  4u |kk| + 2u is^2 P / n  <=  6u is^2 P / n
#   sw = fl(is * weight)                               u |sw|
#   r = fl(fl(fl(d - gm) - fl(fl(x - mean_f) kk)) sw)
#     inner: 3u |d| + 4u (|s| + R)/n + 9u |x - mean| is^2 P / n;  times sw: + 2u (|d| + |s|/n + |x - mean| is^2 P / n)
#   |r_f - r| <= 11 u |sw| (|d| + (|s| + R)/n + |x - mean| is^2 P / n)
K_BWD = 11
# parameter gradients: db = fl(s), dw = fl(fl(dp) is): |db_f - db| <= u |db| + u R; |dw_f - dw| <= 2u |dw| + 2u is P.
# Running statistics: fl(fl(m r) + fl(fl(1 - m) fl(stat))) <= 4u (|m r| + |(1 - m) stat|).  Saved mean: u; saved invstd: 5u.


def f32(v):
    """a scalar or array parameter at the float32 value the kernel receives, as float64"""
    return np.asarray(np.float32(v) if np.isscalar(v) else np.asarray(v, np.float32), np.float64)


def bn_forward_exact(x, weight=None, bias=None, eps=1e-4, momentum=0.9, leak=0.0, train=True, running_mean=None,
                     running_var=None, parts=None):
    """float64 BatchNorm(+leaky ReLU) forward of x [rows, planes] (the values the device read: bf16 inputs as their bf16
    values).  weight / bias None = affine=False.  train: batch statistics (from `parts` [nparts, 2, planes] fp64 sums of
    x and x*x when given, as the convolution's epilogue writes them), running-statistics update with momentum and
    n / (n - 1) (NaN at n == 1, as the reference: 0 / 0); eval: the running statistics.  Returns a dict: out, y (before
    the activation), mean, var (biased), invstd, a, c, running_mean, running_var, slack (per element of out) and the
    per-plane tolerances tol_mean, tol_invstd, tol_rm, tol_rv."""
    x = np.asarray(x, np.float64)
    n, C = x.shape
    w = np.ones(C) if weight is None else f32(weight)
    b = np.zeros(C) if bias is None else f32(bias)
    eps, mom, leak = float(f32(eps)), float(f32(momentum)), float(f32(leak))
    rm0 = np.zeros(C) if running_mean is None else f32(running_mean)
    rv0 = np.ones(C) if running_var is None else f32(running_var)
    r = {}
    var_err, mean_err = np.zeros(C), np.zeros(C)
    if train:
        if parts is not None:
            s, ss = parts[:, 0].sum(0), parts[:, 1].sum(0)
            mean = s / n
            var = np.maximum(ss / n - mean * mean, 0.0)
        else:
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
        # the kernel's one-pass fp64 statistics: var = (sum x^2 - mean^2 n) / n, summation error <= (n + 2) 2^-53 sum x^2
        var_err = (n + 2) * 2.0 ** -53 * (x * x).mean(0)
        mean_err = (n + 2) * 2.0 ** -53 * np.abs(x).mean(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            unb = var * n / (n - 1) if n > 1 else np.full(C, np.nan)
            unb_err = var_err * n / (n - 1) if n > 1 else np.zeros(C)
        r["running_mean"] = mom * rm0 + (1 - mom) * mean
        r["running_var"] = mom * rv0 + (1 - mom) * unb
        r["tol_rm"] = 4 * U * (np.abs(mom * rm0) + np.abs((1 - mom) * mean)) + (1 - mom) * mean_err
        r["tol_rv"] = 4 * U * (np.abs(mom * rv0) + np.abs((1 - mom) * unb)) + (1 - mom) * unb_err
    else:
        mean, var = rm0, rv0
        r["running_mean"], r["running_var"] = rm0, rv0
        r["tol_rm"] = r["tol_rv"] = np.zeros(C)
    invstd = (var + eps) ** -0.5
    var_rel = var_err / (2 * (var + eps))          # relative error of invstd it causes
    a = invstd * w
    c = b - mean * a
    y = x * a + c
    slack = (K_FWD * U + var_rel) * (np.abs(x * a) + np.abs(mean * a) + np.abs(b)) + np.abs(a) * mean_err
    # where y is negative beyond its slack the kernel's y is negative too, and out = fl(y leak) carries leak times it
    # (a ReLU's zeros stay exact zeros)
    r.update(mean=mean, var=var, invstd=invstd, a=a, c=c, y=y, out=np.where(y > 0, y, y * leak),
             slack=np.where(y < -slack, leak * slack, slack),
             tol_mean=U * np.abs(mean) + mean_err, tol_invstd=(5 * U + var_rel) * invstd)
    return r


def bn_backward_exact(x, out, d_out, mean, invstd, weight=None, leak=0.0, parts=None):
    """float64 BatchNorm(+leaky ReLU) backward (CPU/BatchNormalization.cpp:63-107) with the saved mean / invstd given (the
    device's own fp32 values), the activation mask from the given stored forward output `out` (`out > 0`, as the kernel
    reads it in bf16; in fp32 the kernel recomputes the same sign from x).  `parts` [nparts, 2, planes]: the statistics
    (sum of masked d_out, sum of (x - mean) * masked d_out) as given fp64 partial sums instead of the kernel's own.
    Returns a dict: d_in, dw, db, slack (per element of d_in), tol_dw, tol_db."""
    x, g = np.asarray(x, np.float64), np.asarray(d_out, np.float64)
    n, C = x.shape
    mean, invstd, leak = f32(mean), f32(invstd), float(f32(leak))
    w = np.ones(C) if weight is None else f32(weight)
    d = np.where(np.asarray(out) > 0, g, g * leak)
    xm = x - mean
    if parts is not None:
        s, dot = parts[:, 0].sum(0), parts[:, 1].sum(0)
    else:
        s, dot = d.sum(0), (xm * d).sum(0)
    # R: sum |d| over the products g * leak the kernel rounds (none for leakiness 0 or 1)
    R = np.abs(np.where(np.asarray(out) > 0, 0.0, d)).sum(0) if 0.0 < leak < 1.0 else np.zeros(C)
    P = np.abs(xm * d).sum(0)
    k = dot * invstd * invstd / n
    sw = invstd * w
    d_in = (d - s / n - xm * k) * sw
    return dict(d_in=d_in, dw=dot * invstd, db=s,
                slack=K_BWD * U * np.abs(sw) * (np.abs(d) + (np.abs(s) + R) / n + np.abs(xm) * invstd * invstd * P / n),
                tol_db=U * (np.abs(s) + R), tol_dw=2 * U * (np.abs(dot * invstd) + invstd * P))


# ------------------------------------------------------------------------------------------------ bf16 rounding
def bf16_rne(v):
    """round-to-nearest-even of float64 values to bf16 (8 significant bits, fp32's exponent range incl. its subnormals),
    directly -- no intermediate fp32 rounding; returned as float64"""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(v)
    ulp = np.ldexp(1.0, np.maximum(e, -125) - 8)
    k = np.floor(v / ulp)
    lo = k * ulp
    mid = lo + 0.5 * ulp
    up = (v > mid) | ((v == mid) & (np.mod(k, 2) == 1))
    return np.where(up, lo + ulp, lo)


def check_bf16_rounded(got, exact64, slack):
    """(ok mask, fraction of elements whose slack interval straddles a bf16 midpoint)"""
    got = np.asarray(got, np.float64)
    e = np.asarray(exact64, np.float64)
    s = np.broadcast_to(np.asarray(slack, np.float64), e.shape)
    lo, hi = bf16_rne(e - s), bf16_rne(e + s)
    ok = (got >= lo) & (got <= hi) & (bf16_rne(got) == got)
    return ok, float((lo != hi).mean()) if e.size else 0.0


def assert_bf16_rounded(got, exact64, slack, what="", max_undecided=0.05):
    """every element of `got` (a bf16 tensor or its float values) is the RNE bf16 of a value within `slack` of exact64;
    and at most `max_undecided` of the elements have a slack interval wide enough to allow two bf16 values"""
    if hasattr(got, "detach"):
        got = got.detach().float().cpu().numpy()
    exact64 = np.asarray(exact64, np.float64)
    assert np.asarray(got).shape == exact64.shape, (what, np.asarray(got).shape, exact64.shape)
    assert np.isfinite(exact64).all(), what
    ok, undecided = check_bf16_rounded(got, exact64, slack)
    if not ok.all():
        i = np.flatnonzero(~ok.ravel())[0]
        g_, e_ = np.asarray(got, np.float64).ravel()[i], exact64.ravel()[i]
        s_ = np.broadcast_to(slack, exact64.shape).ravel()[i]
        raise AssertionError("%s: %d of %d stores are not a round-to-nearest-even bf16 of the exact value within its "
                             "slack; first at flat index %d: got %.9g, exact %.12g (RNE %.9g), slack %.3g"
                             % (what, (~ok).sum(), ok.size, i, g_, e_, bf16_rne(e_), s_))
    assert undecided <= max_undecided, "%s: the slack leaves %.2f %% of the stores undecided" % (what, 100 * undecided)
    return undecided

