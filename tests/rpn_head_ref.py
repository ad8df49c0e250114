"""fp64 definition of the RPN head (SingleConvRPNHead_Sparse3D, modeling/rpn/rpn_sparse3d.py:109-131) and of its
gradients, with a per-element bound on the device's distance from each result, derived from the kernel's operation
sequence (csrc/rpn_head.hip) as tests/roi_mlp_ref.py does for the box head.

Definition, for the rows f [n, C] of all maps (the weights are shared, so the maps are concatenated HERE only):
  pre = f W1^T + b1, t = relu(pre), out = t [Wc; Wr]^T + [bc; br]; objectness = out[:, :A] and box_regression =
  out[:, A:] viewed [n, A, 7] (channel a 7 + j).
  D = [d_obj | d_reg];  dt = (D [Wc; Wr]) . (t > 0);  d_f = dt W1;  dW1 = dt^T f, db1 = 1^T dt;
  d[Wc; Wr] = D^T t, d[bc; br] = 1^T D.

Bounds, u = 2^-24.  The fp32 MFMA is a bitwise fmaf chain, so a dot product of K terms plus a bias, in ANY order of
chains and partial sums, is within (K + 2) u (sum |a_k w_k| + |bias|) of exact (terms of order u^2 dropped):
  pre:  (C + 2) u (|f| |W1|^T + |b1|)                                              = s_t (ReLU adds nothing)
  out:  (C + 2) u (|t| |W2|^T + |b2|) + s_t |W2|^T
The backward pass takes the DEVICE's hidden activation as its input: the mask is the device's own t > 0 (the decision),
and d[Wc; Wr] multiplies the device's t, which is within s_t of the definition's.
  dt:   (32 + 2) u (|D| |W2|)      (8 A columns zero-padded to 32; zeros add nothing)              = s_dt, masked
  d_f:  (C + 2) u (|dt| |W1|) + s_dt |W1|
  dW1:  (M + 2) u (|dt|^T |f|) + s_dt^T |f|,   db1: (M + 2) u sum |dt| + sum s_dt        M = rows of all maps: the
  dW2:  (M + 2) u (|D|^T |t|) + |D|^T s_t,     db2: (M + 2) u sum |D|                    sums over sites run as
        per-workgroup chains whose partials are added in order -- any order of M terms is within (M + 2) u.
A hidden unit whose fp64 pre-activation lies within s_t of zero is UNDECIDABLE: the device may take either branch.  Such
units are left out of the comparison of the device's mask with the definition's, counted, and capped at 1 %.
"""
import numpy as np

U = 2.0 ** -24
F = np.float32
MAX_UNDECIDED = 0.01


class V(object):
    """a value in fp64 and the bound on the device's distance from it"""

    def __init__(self, v, s=None):
        self.v = np.asarray(v, np.float64)
        self.s = np.zeros_like(self.v) if s is None else np.asarray(s, np.float64)


def packed(p):
    """[Wc; Wr] and [bc; br] in fp64"""
    return (np.concatenate([p["cls_w"], p["reg_w"]]).astype(np.float64),
            np.concatenate([p["cls_b"], p["reg_b"]]).astype(np.float64))


def forward(f, p):
    """f [n, C] (exact fp32 input), p: fp32 parameters conv_w [C, C], conv_b, cls_w [A, C], cls_b, reg_w [7 A, C], reg_b.
    Returns dict of V: pre, t, obj [n, A], reg [n, 7 A]"""
    f = np.asarray(f, np.float64)
    w1, b1 = p["conv_w"].astype(np.float64), p["conv_b"].astype(np.float64)
    w2, b2 = packed(p)
    C, A = w1.shape[0], p["cls_w"].shape[0]
    pre = f @ w1.T + b1
    s_t = (C + 2) * U * (np.abs(f) @ np.abs(w1).T + np.abs(b1))
    t = np.maximum(pre, 0.0)
    out = t @ w2.T + b2
    s_o = (C + 2) * U * (t @ np.abs(w2).T + np.abs(b2)) + s_t @ np.abs(w2).T
    return {"pre": V(pre, s_t), "t": V(t, s_t), "obj": V(out[:, :A], s_o[:, :A]), "reg": V(out[:, A:], s_o[:, A:])}


def undecided(fwd):
    """bool [n, C]: hidden units whose branch the bound leaves open"""
    return np.abs(fwd["pre"].v) <= fwd["pre"].s


def backward(f, p, g_obj, g_reg, t_dev, fwd):
    """gradients with the device's hidden activation t_dev [n, C] as the input (mask and d[Wc; Wr] operand).
    g_obj [n, A], g_reg [n, 7 A] (zeros for an absent gradient).  Returns dict of V."""
    f = np.asarray(f, np.float64)
    w1 = p["conv_w"].astype(np.float64)
    w2, _ = packed(p)
    C, A = w1.shape[0], p["cls_w"].shape[0]
    M = f.shape[0]
    D = np.concatenate([g_obj, g_reg], 1).astype(np.float64)
    mask = np.asarray(t_dev) > 0
    dt = np.where(mask, D @ w2, 0.0)
    s_dt = np.where(mask, 34 * U * (np.abs(D) @ np.abs(w2)), 0.0)
    k = (M + 2) * U
    out = {"d_f": V(dt @ w1, (C + 2) * U * (np.abs(dt) @ np.abs(w1)) + s_dt @ np.abs(w1)),
           "d_conv_w": V(dt.T @ f, k * (np.abs(dt).T @ np.abs(f)) + s_dt.T @ np.abs(f)),
           "d_conv_b": V(dt.sum(0), k * np.abs(dt).sum(0) + s_dt.sum(0))}
    # the definition's t; the device's operand is within s_t of it
    t, s_t = fwd["t"].v, fwd["t"].s
    dw2 = V(D.T @ t, k * (np.abs(D).T @ np.abs(t)) + np.abs(D).T @ s_t)
    db2 = V(D.sum(0), k * np.abs(D).sum(0))
    out["d_cls_w"], out["d_reg_w"] = V(dw2.v[:A], dw2.s[:A]), V(dw2.v[A:], dw2.s[A:])
    out["d_cls_b"], out["d_reg_b"] = V(db2.v[:A], db2.s[:A]), V(db2.v[A:], db2.s[A:])
    return out


def worst(got, ref):
    """max |got - ref.v| / ref.s (0 / 0 = 0), and the count of elements outside the bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.v.shape, (got.shape, ref.v.shape)
    err = np.abs(got - ref.v)
    bad = ~(err <= ref.s)                       # a NaN is outside
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / ref.s)
    return (float(np.nanmax(ratio)) if ratio.size else 0.0), int(bad.sum())


# ------------------------------------------------------------------------------------------------ shared test inputs
def make_case(C, A, rows, seed):
    """seeded fp32 inputs: per-map feature rows and output gradients, and the parameters ([out, in] layouts)"""
    rng = np.random.default_rng(1000 * seed + 10 * C + A)
    p = {"conv_w": (rng.standard_normal((C, C)) / np.sqrt(C)).astype(F), "conv_b": (0.5 * rng.standard_normal(C)).astype(F),
         "cls_w": (rng.standard_normal((A, C)) / np.sqrt(C)).astype(F), "cls_b": rng.standard_normal(A).astype(F),
         "reg_w": (rng.standard_normal((7 * A, C)) / np.sqrt(C)).astype(F), "reg_b": rng.standard_normal(7 * A).astype(F)}
    f = [rng.standard_normal((n, C)).astype(F) for n in rows]
    g_obj = [rng.standard_normal((n, A)).astype(F) for n in rows]
    g_reg = [rng.standard_normal((n, 7 * A)).astype(F) for n in rows]
    return p, f, g_obj, g_reg


def entry_cases(T):
    """(C, A, rows per map, seed) of the entry-point test: every C, the padded-column case 8 A = 8, a map that
    crosses a tile edge by one row, an empty map, a one-row map"""
    return [(C, A, (T + 1, 0, 1), 3) for C in (32, 64, 96, 128) for A in (1, 2, 4)]


def hidden_cases(T):
    return [(C, A, (2 * T, T - 1, 3), 4) for C in (32, 64, 96, 128) for A in (1, 2, 4)]
