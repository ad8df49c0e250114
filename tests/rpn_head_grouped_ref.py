"""fp64 definition and bounds of the RPN head with separated-classifier groups (aabr_rpn_head_grouped_*,
csrc/rpn_head.hip; the reference's rpn_sparse3d.py:95-131) -- TEST INFRASTRUCTURE ONLY.

The grouped head IS the plain head of tests/rpn_head_ref.py with A G anchors' worth of output channels: cls_w [A G, C]
holds row a G + g, reg_w [7 A G, C] row a 7 G + 7 g + k.  So the definition and the bounds are rpn_head_ref's, on the
packed channel order, and only the channel permutation to and from the device's group-major tensors is restated here:
  objectness [n, A G]       -> [G, n, A]       (group g: channel a G + g)
  box_regression [n, 7 A G] -> [G, n, A, 7]    (group g: channel a 7 G + 7 g + k)
One bound differs: dt = (D [Wc; Wr]) . (t > 0) reduces over the 8 A G packed columns padded to whole 32-wide MFMA tiles
(zeros add nothing), so its chain has 32 ceil(8 A G / 32) terms and the bound is (32 ceil(8 A G / 32) + 2) u where
rpn_head_ref has 34 u.  backward() below is rpn_head_ref.backward with that one factor."""
import numpy as np

import rpn_head_ref as R

U = R.U
GROUPS = [(1, 2), (2, 3), (4, 2), (4, 3), (2, 8)]       # (A, G): 16, 48, 64, 96, 128 output columns


def to_groups(x, A, G, k):
    """packed channels [n, k A G] -> group-major [G, n, A] (k = 1) or [G, n, A, 7] (k = 7)"""
    x = np.asarray(x)
    n = x.shape[0]
    if k == 1:
        return np.ascontiguousarray(x.reshape(n, A, G).transpose(2, 0, 1))
    return np.ascontiguousarray(x.reshape(n, A, G, 7).transpose(2, 0, 1, 3))


def from_groups(x, A, G, k):
    """the inverse: group-major [G, n, A(, 7)] -> packed [n, k A G]"""
    x = np.asarray(x)
    n = x.shape[1]
    if k == 1:
        return np.ascontiguousarray(x.reshape(G, n, A).transpose(1, 2, 0)).reshape(n, A * G)
    return np.ascontiguousarray(x.reshape(G, n, A, 7).transpose(1, 2, 0, 3)).reshape(n, 7 * A * G)


def v_to_groups(v, A, G, k):
    return R.V(to_groups(v.v, A, G, k), to_groups(v.s, A, G, k))


def group_params(p, A, G, g):
    """the plain head's parameters of group g: rows a G + g of cls_w / cls_b, rows a 7 G + 7 g + k of reg_w / reg_b"""
    C = p["conv_w"].shape[0]
    return {"conv_w": p["conv_w"], "conv_b": p["conv_b"],
            "cls_w": np.ascontiguousarray(p["cls_w"].reshape(A, G, C)[:, g]),
            "cls_b": np.ascontiguousarray(p["cls_b"].reshape(A, G)[:, g]),
            "reg_w": np.ascontiguousarray(p["reg_w"].reshape(A, G, 7, C)[:, g]).reshape(7 * A, C),
            "reg_b": np.ascontiguousarray(p["reg_b"].reshape(A, G, 7)[:, g]).reshape(7 * A)}


def dt_terms(A, G):
    return 32 * (-(-8 * A * G // 32)) + 2


def backward(f, p, g_obj, g_reg, t_dev, fwd, A, G):
    """rpn_head_ref.backward on the packed channel order (g_obj [n, A G], g_reg [n, 7 A G]) with the dt bound of the
    padded 8 A G columns"""
    f = np.asarray(f, np.float64)
    w1 = p["conv_w"].astype(np.float64)
    w2, _ = R.packed(p)
    C, AG = w1.shape[0], p["cls_w"].shape[0]
    assert AG == A * G
    M = f.shape[0]
    D = np.concatenate([g_obj, g_reg], 1).astype(np.float64)
    mask = np.asarray(t_dev) > 0
    dt = np.where(mask, D @ w2, 0.0)
    s_dt = np.where(mask, dt_terms(A, G) * U * (np.abs(D) @ np.abs(w2)), 0.0)
    k = (M + 2) * U
    out = {"d_f": R.V(dt @ w1, (C + 2) * U * (np.abs(dt) @ np.abs(w1)) + s_dt @ np.abs(w1)),
           "d_conv_w": R.V(dt.T @ f, k * (np.abs(dt).T @ np.abs(f)) + s_dt.T @ np.abs(f)),
           "d_conv_b": R.V(dt.sum(0), k * np.abs(dt).sum(0) + s_dt.sum(0))}
    t, s_t = fwd["t"].v, fwd["t"].s
    dw2 = R.V(D.T @ t, k * (np.abs(D).T @ np.abs(t)) + np.abs(D).T @ s_t)
    db2 = R.V(D.sum(0), k * np.abs(D).sum(0))
    out["d_cls_w"], out["d_reg_w"] = R.V(dw2.v[:AG], dw2.s[:AG]), R.V(dw2.v[AG:], dw2.s[AG:])
    out["d_cls_b"], out["d_reg_b"] = R.V(db2.v[:AG], db2.s[:AG]), R.V(db2.v[AG:], db2.s[AG:])
    return out


# ------------------------------------------------------------------------------------------------ shared test inputs
def make_case(C, A, G, rows, seed):
    """rpn_head_ref.make_case(C, A G, rows, seed): its shapes are exactly the grouped ones.  The gradients are in the
    packed channel order; the device reads their group-major form (to_groups)."""
    return R.make_case(C, A * G, rows, seed)


def entry_cases(T):
    """(C, A, G, rows per map, seed): every C; a padded single tile, a group's columns across a tile edge, two full
    tiles, the reference's 3g6c, the limit; a map that crosses a tile edge by one row, an empty map, a one-row map"""
    return [(C, A, G, (T + 1, 0, 1), 3) for C in (32, 64, 96, 128) for A, G in GROUPS]


def hidden_cases(T):
    return [(C, A, G, (2 * T, T - 1, 3), 4) for C in (32, 64, 96, 128) for A, G in GROUPS]


def determinism_cases(T, gmax):
    """more tiles than workgroups (gmax + 1 tiles), and one tile"""
    return [(32, 2, 3, (gmax * T + 5,), 5), (32, 2, 3, (7,), 6)]
