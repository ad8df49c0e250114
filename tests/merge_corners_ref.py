"""numpy fp32 restatement of merge_walls_by_corners as this package defines it (include/aabr_hip.h,
aabr_merge_walls_by_corners; reference: maskrcnn_benchmark/structures/bounding_box_3d.py:843-923), operation by operation:
every product, sum and quotient is one np.float32 operation, written from the definition and from the reference's lines, not
from csrc/merge_corners.h.

  * yx_zb -> two corners (utils3d/bbox3d_ops_torch.py:115-135 and what it calls) follows the operation sequence that
    csrc/corner_box.h documents: the rotation in float64 with libm's sin / cos (math.sin / math.cos: the functions the
    host harness calls), rounded once to fp32.
  * the fused steps -- sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) of the distances and of the epilogue's norm,
    sqrt(fma(dy, dy, dx * dx)) of the wall's length -- are computed through float64: the product of two fp32 values is
    exact there, the sum with the fp32 partial result is rounded to float64 and then to fp32.
  * a mean is a sum from 0 in ascending index, one fp32 addition at a time, and one division.

`merge_scene` returns the rebuilt rows, the per-corner merged flags and, per step, the set S the step met (before its
skip / merge decision) and whether it merged; `margin` is the smallest |distance - threshold| any step met (the tests
keep it >= 1e-3: a condition on their inputs)."""
import math

import numpy as np

F = np.float32
PI = F(3.14159274101257324)
HALF_PI = F(1.57079637050628662)
MAX_WALLS = 2048


def _limit_period(v, offset):
    return F(v - F(np.floor(F(F(v / PI) + offset)) * PI))


def to_2corners(b):
    """one yx_zb box -> [x0, y0, x1, y1, z0, z1, thickness]"""
    b = [F(v) for v in b]
    h = F(0.5)
    zc = F(b[2] + F(b[5] * h))
    sx, sy, sz = b[4], b[3], b[5]
    yaw = _limit_period(F(b[6] + HALF_PI), F(0))
    hx, hy, hz = F(sx * h), F(sy * h), F(sz * h)
    zx, zy, zz = F(b[0] - hx), F(b[1] - hy), F(zc - hz)
    kx, ky = [None] * 4, [None] * 4
    if yaw != 0:
        cs, sn = math.cos(float(yaw)), math.sin(float(yaw))
        dhx, dhy, dhz = float(hx), float(hy), float(hz)
        for k in range(4):
            dx = (float(sx) if k & 1 else 0.0) - dhx
            dy = (float(sy) if k & 2 else 0.0) - dhy
            kx[k] = F(F((cs * dx + sn * dy) + dhx) + zx)
            ky[k] = F(F(((-sn) * dx + cs * dy) + dhy) + zy)
        zb = F(F((0.0 - dhz) + dhz) + zz)
        zt = F(F((float(sz) - dhz) + dhz) + zz)
    else:
        for k in range(4):
            kx[k] = F((sx if k & 1 else F(0)) + zx)
            ky[k] = F((sy if k & 2 else F(0)) + zy)
        zb = F(F(0) + zz)
        zt = F(sz + zz)
    two = F(2)
    ax, ay = F(F(kx[0] + kx[2]) / two), F(F(ky[0] + ky[2]) / two)
    bx, by = F(F(kx[1] + kx[3]) / two), F(F(ky[1] + ky[3]) / two)
    mx, my = F(F(ax + bx) / two), F(F(ay + by) / two)
    m = F(1) if F(F(ax - mx) + F(ay - my)) > 0 else F(0)
    n = F(F(1) - m)
    return [F(F(ax * m) + F(bx * n)), F(F(ay * m) + F(by * n)), F(F(bx * m) + F(ax * n)), F(F(by * m) + F(ay * n)),
            F(F(zb + zb) / two), F(F(zt + zt) / two), b[3]]


def top_offseted(c):
    """the two top corners of a two-corner box pulled towards their midpoint by half the thickness -> [2][3]"""
    p = [[c[0], c[1], c[5]], [c[2], c[3], c[5]]]
    cen = [F(F(p[0][d] + p[1][d]) / F(2)) for d in range(3)]
    out = []
    for k in range(2):
        off = [F(cen[d] - p[k][d]) for d in range(3)]
        nrm = np.sqrt(F(F(F(off[0] * off[0]) + F(off[1] * off[1])) + F(off[2] * off[2])))
        out.append([F(p[k][d] + F(F(F(off[d] / nrm) * c[6]) * F(0.5))) for d in range(3)])
    return out


def _fused_sq(v, acc):
    """fma(v, v, acc) of fp32 values through float64"""
    v = np.asarray(v, np.float64)
    return (v * v + np.asarray(acc, np.float64)).astype(F)


def norm3(dx, dy, dz):
    """sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) in fp32 (arrays or scalars)"""
    dx, dy, dz = (np.asarray(v, F) for v in (dx, dy, dz))
    return np.sqrt(_fused_sq(dz, _fused_sq(dy, dx * dx)))


def from_2corners(c):
    """one two-corner box back to yx_zb"""
    two = F(2)
    cx, cy, cz = F(F(c[0] + c[2]) / two), F(F(c[1] + c[3]) / two), F(F(c[4] + c[5]) / two)
    dx, dy = F(c[2] - c[0]), F(c[3] - c[1])
    ln = F(np.sqrt(_fused_sq(dy, F(dx * dx))))
    zs = F(c[5] - c[4])
    vx, vy = F(dx / ln), F(dy / ln)
    cr = F(F(F(1) * vy) - F(F(0) * vx))
    g = F(1) if abs(cr) > 1 else F(0)
    cr = F(cr * F(F(1) - F(g * F(1e-7))))
    ang = F(-F(math.asin(float(cr)))) if not np.isnan(cr) else F(np.nan)
    cosa = F(F(F(F(1) * vx) + F(F(0) * vy)) + F(F(0) * F(0)))
    m = F(1) if cosa >= 0 else F(0)
    ang = F(F(ang * m) + F(F(PI - ang) * F(F(1) - m)))
    ang = _limit_period(ang, F(0))
    return [cx, cy, F(cz - F(zs * F(0.5))), c[6], ln, zs, _limit_period(F(ang - HALF_PI), F(0.5))]


def _mean_from_zero(values):
    s = F(0)
    for v in values:
        s = F(s + v)
    return F(s / F(len(values)))


def step(x, y, z, i, threshold):
    """one step on the corner arrays (fp32, modified in place) -> (S ascending, merged?, distances)"""
    d = norm3(x[i] - x, y[i] - y, z[i] - z)
    mask = d < F(threshold)
    mask[i ^ 1] = False
    ids = np.nonzero(mask)[0]
    whole = bool((mask[0::2] & mask[1::2]).any())
    did = (not whole) and len(ids) > 1
    if did:
        mean = [_mean_from_zero(v[ids]) for v in (x, y, z)]
        x[ids], y[ids], z[ids] = mean
    return ids, did, d


def merge_walls(walls, threshold=0.1, trace=None):
    """walls [W, 7] yx_zb fp32 -> (rebuilt [W, 7], merged [W, 2] int32).  trace (a dict) receives `steps`: a list of
    (S, merged?) per step, `margin`, and `corners0` / `corners1`: the corner arrays before and after the loop."""
    walls = np.ascontiguousarray(walls, F).reshape(-1, 7)
    W = walls.shape[0]
    out, merged = np.empty((W, 7), F), np.zeros(2 * W, np.int32)
    if W == 0:
        return out, merged.reshape(0, 2)
    with np.errstate(all="ignore"):
        rows = [to_2corners(b) for b in walls]
        top = np.array([top_offseted(c) for c in rows], F).reshape(2 * W, 3)
        x, y, z = (np.ascontiguousarray(top[:, d]) for d in range(3))
        steps, margin = [], np.inf
        corners0 = np.stack([x, y, z], 1)
        if W > 1:
            for i in range(2 * W):
                ids, did, d = step(x, y, z, i, threshold)
                margin = min(margin, float(np.abs(np.delete(d, i ^ 1).astype(np.float64) - float(F(threshold))).min()))
                if did:
                    merged[ids] = 1
                steps.append((ids, did))
        z0_mean = _mean_from_zero([c[4] for c in rows])
        for w in range(W):
            th = rows[w][6]
            p = [[x[2 * w], y[2 * w], z[2 * w]], [x[2 * w + 1], y[2 * w + 1], z[2 * w + 1]]]
            cen = [F(F(F(F(0) + p[0][d]) + p[1][d]) / F(2)) for d in range(3)]
            q = []
            for k in range(2):
                off = [F(p[k][d] - cen[d]) for d in range(3)]
                nrm = F(norm3(off[0], off[1], off[2]))
                q.append([F(p[k][d] + F(F(F(off[d] / nrm) * th) * F(0.5))) for d in range(3)])
            z1 = F(F(F(F(0) + q[0][2]) + q[1][2]) / F(2))
            out[w] = from_2corners([q[0][0], q[0][1], q[1][0], q[1][1], z0_mean, z1, th])
    if trace is not None:
        trace.update(steps=steps, margin=margin, corners0=corners0, corners1=np.stack([x, y, z], 1))
    return out, merged.reshape(W, 2)


def merge_scene(boxes, labels=None, threshold=0.1, wall_label=1, trace=None):
    """boxes [n, 7], labels [n] (None: every row is a wall) -> (boxes out [n, 7], merged [n, 2] int32): the wall rows
    rebuilt, every other row the input's bits"""
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 7)
    sel = np.ones(len(boxes), bool) if labels is None else np.asarray(labels) == wall_label
    out, merged = boxes.copy(), np.zeros((len(boxes), 2), np.int32)
    if sel.any():
        out[sel], merged[sel] = merge_walls(boxes[sel], threshold, trace)
    elif trace is not None:
        trace.update(steps=[], margin=np.inf)
    return out, merged


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
