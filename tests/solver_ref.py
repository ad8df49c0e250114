"""numpy restatement of the fused SGD step (csrc/solver.hip, solver_glue.FusedSGD): one fp32 operation at a time, in the
kernel's order, plus the same step evaluated in float64 and the first-order bounds that follow from the operation
sequence.  The device must equal `step_f32` exactly (as values, NaNs in the same places); torch.optim.SGD on the CPU fuses
some of the operations and is held to the bounds instead.

    g  = widen(grad);  g = g * grad_scale      only when grad_scale != 1
    d  = g + wd * p                            only when wd != 0
    m' = mu * m + d                            only when mu != 0   (else no buffer; the step uses d)
    p' = p - lr * m'

Bounds against the float64 step from the same (p, m, g), u = 2^-24, S = mu |m| + |g| + wd |p| (g after the scale):
    m': up to 3 roundings on quantities of at most S (the product mu m, the product wd p and its sum, the last sum)
        -> B_m = 3 u S
    p': the error of m' scaled by lr, the product's rounding (u lr S) and the rounding of the difference
        (u (|p| + lr S)) -> B_p = u (|p| + 5 lr S)
each times (1 + 2^-10) for the higher-order terms."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
F = np.float32


def widen_bf16(bits):
    """uint16 bf16 bit patterns -> the float32 of the same value (exact)"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite values)"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def step_f32(p, m, g, lr, wd, mu, grad_scale=1.0):
    """one step on float32 arrays; lr, wd, mu, grad_scale are rounded to float32 once, as the entry point's arguments.
    Returns (p', m'); m' is `m` itself (unchanged) when mu == 0."""
    p, g = np.asarray(p, F), np.asarray(g, F)
    lr, wd, mu, gs = F(lr), F(wd), F(mu), F(grad_scale)
    with np.errstate(all="ignore"):
        if gs != F(1.0):
            g = (g * gs).astype(F)
        d = g
        if wd != F(0.0):
            t = (wd * p).astype(F)
            d = (g + t).astype(F)
        if mu != F(0.0):
            t = (mu * np.asarray(m, F)).astype(F)
            m = (t + d).astype(F)
            d = m
        t = (lr * d).astype(F)
        p = (p - t).astype(F)
    return p, m


def step_f64(p, m, g, lr, wd, mu, grad_scale=1.0):
    """the same step in float64 from the same float32 inputs and the same float32 scalars"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    lr, wd, mu, gs = (float(F(v)) for v in (lr, wd, mu, grad_scale))
    g = g * gs
    d = g + wd * p
    if mu != 0.0:
        m = mu * np.asarray(m, np.float64) + d
        d = m
    return p - lr * d, m


def bounds(p, m, g, lr, wd, mu, grad_scale=1.0):
    """(B_p, B_m) per element"""
    p, m, g = (np.abs(np.asarray(v, np.float64)) for v in (p, m, g))
    lr, wd, mu, gs = (abs(float(F(v))) for v in (lr, wd, mu, grad_scale))
    S = mu * m + g * gs + wd * p
    return U * (p + 5.0 * lr * S) * SLACK, 3.0 * U * S * SLACK


def same_values(a, b):
    """equal as values with NaNs in the same places (+0 == -0)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())
