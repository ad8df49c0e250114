"""Rotated 3-D ROI-align in float64, written from the operation's definition, with a derived error bound.

The yardstick of tests/test_roi_align_host.py and tests/test_gpu_roi_align.py for both kernels of csrc/roi.hip (the dense
one and the fused gather through the cell map).  It is NOT a restatement of the kernel: oracle/roi_oracle.c is that (the
kernel's fp32 statements on the CPU), and the host test holds the two against each other.

Definition.  Input `inp` [B, C, H, W, Z] (layout [B, C, X(h), Y(w), Z]: the FIRST spatial axis is the one the ROI's `h`
and the coordinate `y` run along, the SECOND belongs to `w` and `x`).  An ROI is (b, cw, ch, cz, w, h, z, theta_deg).
With spatial scale s and output size (PH, PW, PZ):
  * centre (cw, ch, cz) s and sizes (w, h, z) s, in cells; coordinate i is the centre of cell i;
  * the box is cut into PH x PW x PZ bins along its own h, w, z axes, each bin into a grid of gh x gw x gz samples
    placed at the centres of the grid's sub-cells: along one axis, sample i of bin p sits at
    -size/2 + (p + (i + 1/2) / g) size / P  in the box's frame;
  * the box's frame is the map's frame turned by theta about z:  x = xx cos + yy sin + cw,  y = yy cos - xx sin + ch,
    z = zz + cz   (xx along the box's w, yy along its h: at +90 degrees h runs along +x and w along -y);
  * the value at a sample is the trilinear interpolant of plane c of sample b (product of three 1-D hat functions over
    the cell centres, the edge cells extended outwards);
  * out[n, c, ph, pw, pz] = sum over the bin's samples / (gh gw gz).
The backward pass is the transpose of that linear map, applied to the output gradient.

Documented quirks, each with the line of csrc/roi.hip that has it:
  Q1 sizes below one cell are raised to 1 after scaling                                        (roi.hip:86, fmaxf)
  Q2 sampling ratio <= 0: the grid is ceil(size / bins) per axis                              (roi.hip:88-90)
  Q3 a sample contributes nothing when y < -1, y > H, x < -1, x > W or z < -1; the forward pass has NO upper cut in z
     (the sample clamps to the last slice), the backward pass cuts z > Z                     (roi.hip:30-35, :111)
  Q4 coordinates in [-1, 0] clamp to 0; at or beyond the last cell centre the sample takes that cell with weight 1
                                                                                              (roi.hip:36-42)
  Q5 output [n, C, PH, PW, PZ]; theta = float32(deg * pi / 180 computed in double)            (roi.hip:85)
  Q6 a batch index outside [0, B) names an empty sample: zeros forward, nothing backward     (roi.hip:77-82, :322)
Inputs are taken at the float32 values the kernel receives (ROI fields, scale, theta as in Q5); all else is float64.

------------------------------------------------------------------------------------------------------------------------
The slack: how far the kernel's fp32 arithmetic may move a result.  u = 2^-24; round to nearest; the library is built with
-ffp-contract=off, so every * and + below rounds on its own.  fl(v) adds u |v| UNLESS everything before it was exact and
v is itself a float32 number, in which case it adds nothing (_fl below): hand-placed dyadic cases therefore get a
coordinate slack of exactly zero and are decided the same way in both arithmetics.

(a) coordinates.  Per axis (size S = r s, P bins, grid g, bin p, sample i), in the order the kernel computes:
      S_f = fl(r s); below 1 it becomes exactly 1                   e_S = fl
      a = -S_f / 2   (exact halving)                                e_a = e_S / 2
      B = fl(S_f / P)                                               e_B = e_S / P, fl
      t1 = fl(p B)                                                  e_t1 = p e_B, fl
      s1 = fl(a + t1)                                               e_s1 = e_a + e_t1, fl
      t2 = fl((i + .5) B),  t3 = fl(t2 / g)                         e_t3 = (i + .5) e_B / g, fl, fl
      t = fl(s1 + t3)                                               e_t = e_s1 + e_t3, fl
    cosf / sinf: within 1 ulp of the exact value of their float32 argument (the maximum error HIP's math API reference
    lists for sinf, cosf and sincosf), 1 ulp <= 2^-23 |value|: e_c = 2u |cos|, e_s = 2u |sin|; theta = 0 gives exactly
    1 and 0.  Then x = fl(fl(fl(xx c) + fl(yy s)) + fl(cw s)):
      e_x = |c| e_xx + |xx| e_c + e_xx e_c, fl;  the same for yy s;  their sum, fl;  + e_cw, fl
    and y likewise; z = fl(zz + fl(cz s)).
(b) value.  Away from the cuts of Q3 the interpolant is continuous and piecewise trilinear, so moving a sample by
    (e_y, e_x, e_z) moves its value by at most e_y L_y + e_x L_x + e_z L_z, L_a = the largest |difference of neighbouring
    cells along axis a| over the sample's 2x2x2 corner block and the cells one step further out (fp32 may put the sample
    into the neighbouring cell; the bound covers it as long as e < 1/2, otherwise the bin is undecided).
(c) weights and the eight-term sum.  ly = y - y_low is exact (Sterbenz); hy = fl(1 - ly): u; w = fl(fl(hy hx) hz): 3u
    from the factors + 2u; fl(w v): u; seven additions, left to right: 7u of sum |w v|.  Together 13u A, A = sum |w v|.
(d) bin.  The running sum over the S samples: (S - 1) u sum A; the division by the (exact) count: u |out|.
    forward slack = 1.01 (sum_s (b)_s + (13 + S - 1 + 1) u sum_s A_s) / count       (1.01: second-order terms)
Backward, per input cell: a contribution is fl(fl(g w) / count).  Along each axis the weight of a FIXED cell is a
1-Lipschitz function of the coordinate, so with exact axis weights (a, b, c) of that cell the fp32 weight is at most
(a + e_y)(b + e_x)(c + e_z) =: w_up (cells one step outside the exact 2x2x2 block have a, b or c = 0 and are included),
and |contribution - exact| <= |g| / count (w_up - a b c + 7u w_up)  (5u for the weight as in (c), one product, one
division).  m contributions arrive by atomics in any order: any order of m - 1 additions is within
gamma(m - 1) = (m - 1) u / (1 - (m - 1) u) of the sum of absolute contributions.
    backward slack = 1.01 (sum of the per-contribution errors + gamma(m - 1) sum |contribution|)
Nothing here comes from a device run or from the C oracle's output.

Undecided.  Across a cut of Q3 the operation jumps.  A sample with e > 0 within e of a cut (or with e >= 1/2) makes its
bin undecided; an ROI whose adaptive grid (Q2) has size / bins within its rounding error of an integer is undecided as a
whole.  Backward: every cell in the 4x4x4 neighbourhood of such a sample is undecided.
"""
import numpy as np

U = 2.0 ** -24
F = np.float32
K_SAMPLE = 13          # (c)
K_CONTRIB = 7          # backward, per contribution
SECOND_ORDER = 1.01

# deliberately wrong variants, for tests/test_roi_align_host.py's "the bound has teeth" only
VARIANTS = ("rot_sign", "swap_wh", "offset0", "fwd_zcut", "bin_order", "count_inside", "corner_swap", "theta_rad")


def _fl(v, e):
    """error after one fp32 rounding of the value v that carried error e: nothing is added where e == 0 and v is a
    float32 number (the fp32 computation then holds exactly v)"""
    v = np.asarray(v, np.float64)
    e = np.asarray(e, np.float64)
    with np.errstate(over="ignore"):
        exact = (e == 0) & (v.astype(F).astype(np.float64) == v)
    return e + np.where(exact, 0.0, U * np.abs(v))


class Geometry(object):
    """sample points of one ROI: flat arrays over S = (PH gh)(PW gw)(PZ gz) samples, bins in (ph, pw, pz) order"""


def _axis(r, scale, P, g, offset):
    """1-D sample positions of one box axis in the box's frame: (t [P g], e_t, bin index, size, grid, grid_undecided)"""
    raw = float(r) * float(scale)
    e_S = float(_fl(raw, 0.0))
    if raw < 1.0:
        S, e_S = 1.0, 0.0                                             # Q1
    else:
        S = raw
    und = False
    if g <= 0:                                                        # Q2
        q = S / P
        e_q = float(_fl(q, e_S / P))
        g = int(np.ceil(q))
        und = e_q > 0 and abs(q - np.rint(q)) <= e_q
    p = np.repeat(np.arange(P), g).astype(np.float64)
    i = np.tile(np.arange(g), P).astype(np.float64)
    t = -S / 2 + (p + (i + offset) / g) * (S / P)
    # (a), in the kernel's order of operations
    Bw = S / P
    e_B = _fl(Bw, e_S / P)
    e_t1 = _fl(p * Bw, p * e_B)
    e_s1 = _fl(-S / 2 + p * Bw, e_S / 2 + e_t1)
    e_t2 = _fl((i + offset) * Bw, (i + offset) * e_B)
    e_t3 = _fl((i + offset) * Bw / g, e_t2 / g)
    e_t = _fl(t, e_s1 + e_t3)
    return t, e_t, np.repeat(np.arange(P), g), S, g, und


def geometry(roi, scale, out_size, sampling, shape, backward, variant=None):
    """roi: 8 float32 values; shape = (H, W, Z).  Returns a Geometry with y, x, z, their slacks ey, ex, ez, `valid`
    (inside the cuts of Q3), `near` (undecided sample), `bin`, `count`, `grid_undecided`."""
    roi = np.asarray(roi, F).astype(np.float64)
    scale = float(F(scale))
    PH, PW, PZ = out_size
    H, W, Z = shape
    w_field, h_field = (roi[5], roi[4]) if variant == "swap_wh" else (roi[4], roi[5])
    off = 0.0 if variant == "offset0" else 0.5
    yy, e_yy, bh, _, gh, u1 = _axis(h_field, scale, PH, sampling, off)
    xx, e_xx, bw, _, gw, u2 = _axis(w_field, scale, PW, sampling, off)
    zz, e_zz, bz, _, gz, u3 = _axis(roi[6], scale, PZ, sampling, off)
    theta = float(F(roi[7] * np.pi / 180.0)) if variant != "theta_rad" else float(F(roi[7]))      # Q5
    c, s = np.cos(theta), np.sin(theta)
    e_c, e_s = (0.0, 0.0) if theta == 0.0 else (2 * U * abs(c), 2 * U * abs(s))
    if variant == "rot_sign":
        s = -s
    cw, ch, cz = roi[1] * scale, roi[2] * scale, roi[3] * scale
    e_cw, e_ch, e_cz = _fl(cw, 0.0), _fl(ch, 0.0), _fl(cz, 0.0)
    YY, XX = yy[:, None], xx[None, :]
    EYY, EXX = e_yy[:, None], e_xx[None, :]

    def rot(a, ea, fa, efa, b_, eb, fb, efb, centre, e_centre):
        """fl(fl(fl(a fa) + fl(b_ fb)) + centre) and its slack"""
        p1, p2 = a * fa, b_ * fb
        e1 = _fl(p1, abs(fa) * ea + np.abs(a) * efa + ea * efa)
        e2 = _fl(p2, abs(fb) * eb + np.abs(b_) * efb + eb * efb)
        e12 = _fl(p1 + p2, e1 + e2)
        v = p1 + p2 + centre
        return v, _fl(v, e12 + e_centre)

    x2, ex2 = rot(XX, EXX, c, e_c, YY, EYY, s, e_s, cw, e_cw)            # [PH gh, PW gw]
    y2, ey2 = rot(YY, EYY, c, e_c, XX, EXX, -s, e_s, ch, e_ch)
    z1 = zz + cz
    ez1 = _fl(z1, e_zz + e_cz)
    full = (len(yy), len(xx), len(zz))
    g = Geometry()
    g.y = np.broadcast_to(y2[:, :, None], full).ravel()
    g.x = np.broadcast_to(x2[:, :, None], full).ravel()
    g.z = np.broadcast_to(z1[None, None, :], full).ravel()
    g.ey = np.broadcast_to(ey2[:, :, None], full).ravel()
    g.ex = np.broadcast_to(ex2[:, :, None], full).ravel()
    g.ez = np.broadcast_to(ez1[None, None, :], full).ravel()
    g.bin = ((bh[:, None, None] * PW + bw[None, :, None]) * PZ + bz[None, None, :]).ravel()
    g.grid = (gh, gw, gz)
    g.count = float(gh * gw * gz)
    g.grid_undecided = bool(u1 or u2 or u3)
    zcut = backward or variant == "fwd_zcut"
    cut = (g.y < -1) | (g.y > H) | (g.x < -1) | (g.x > W) | (g.z < -1)                       # Q3
    near = ((g.ey > 0) & ((np.abs(g.y + 1) <= g.ey) | (np.abs(g.y - H) <= g.ey))) | \
           ((g.ex > 0) & ((np.abs(g.x + 1) <= g.ex) | (np.abs(g.x - W) <= g.ex))) | \
           ((g.ez > 0) & (np.abs(g.z + 1) <= g.ez))
    if zcut:
        cut |= g.z > Z
        near |= (g.ez > 0) & (np.abs(g.z - Z) <= g.ez)
    near |= (g.ey >= 0.5) | (g.ex >= 0.5) | (g.ez >= 0.5)
    g.valid = ~cut
    g.near = near
    g.coord_slack = float(max(g.ey.max(), g.ex.max(), g.ez.max()))
    return g


def _hat(t, n):
    """1-D linear interpolation over cell centres 0..n-1 with the edge cells extended (Q4): low cell, high cell, and the
    weight of the high cell"""
    tc = np.clip(t, 0.0, n - 1.0)
    lo = np.floor(tc).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    return lo, hi, tc - lo


def _window_max(a, axis, before, after):
    """out[i] = max(a[i - before .. i + after]) along `axis`, a >= 0, out-of-range entries skipped"""
    out = a.copy()
    n = a.shape[axis]
    for d in range(-before, after + 1):
        if d == 0 or abs(d) >= n:
            continue
        src = [slice(None)] * a.ndim
        dst = [slice(None)] * a.ndim
        src[axis] = slice(max(d, 0), n + min(d, 0))
        dst[axis] = slice(max(-d, 0), n + min(-d, 0))
        np.maximum(out[tuple(dst)], a[tuple(src)], out=out[tuple(dst)])
    return out


class Field(object):
    """the input in float64 and, built once, the three local Lipschitz maps of (b): L[a][b, c, y_low, x_low, z_low]"""

    def __init__(self, inp):
        self.v = np.asarray(inp, F).astype(np.float64)
        self._lip = None

    def lip(self):
        if self._lip is None:
            v = self.v
            maps = []
            for ax in (2, 3, 4):
                d = np.zeros_like(v)
                if v.shape[ax] > 1:
                    sl = [slice(None)] * 5
                    sl[ax] = slice(0, v.shape[ax] - 1)
                    d[tuple(sl)] = np.abs(np.diff(v, axis=ax))       # d[j] = |v[j + 1] - v[j]|
                for ax2 in (2, 3, 4):
                    # differences j = low - 1 .. low + 1 along their own axis; cells low - 1 .. low + 2 across
                    d = _window_max(d, ax2, 1, 1 if ax2 == ax else 2)
                maps.append(d)
            self._lip = maps
        return self._lip


class Result(object):
    pass


def forward(inp, rois, scale, out_size, sampling, variant=None):
    """-> Result: values [n, C, PH, PW, PZ] float64, slack (same shape), undecided (bool, same shape),
    coord_slack [n] (largest coordinate slack of the ROI's samples)"""
    fld = inp if isinstance(inp, Field) else Field(inp)
    v = fld.v
    B, C, H, W, Z = v.shape
    rois = np.asarray(rois, F).reshape(-1, 8)
    PH, PW, PZ = out_size
    n = rois.shape[0]
    r = Result()
    r.values = np.zeros((n, C, PH, PW, PZ))
    r.slack = np.zeros_like(r.values)
    r.undecided = np.zeros(r.values.shape, bool)
    r.coord_slack = np.zeros(n)
    for k in range(n):
        b = int(rois[k, 0])
        if b < 0 or b >= B:                                           # Q6
            continue
        g = geometry(rois[k], scale, out_size, sampling, (H, W, Z), False, variant)
        r.coord_slack[k] = g.coord_slack
        ok = g.valid
        ylo, yhi, fy = _hat(g.y[ok], H)
        xlo, xhi, fx = _hat(g.x[ok], W)
        zlo, zhi, fz = _hat(g.z[ok], Z)
        d = v[b].reshape(C, -1)
        val = np.zeros((C, ylo.size))
        mag = np.zeros((C, ylo.size))
        corners = [(yi, wy, xi, wx, zi, wz) for yi, wy in ((ylo, 1 - fy), (yhi, fy)) for xi, wx in ((xlo, 1 - fx), (xhi, fx))
                   for zi, wz in ((zlo, 1 - fz), (zhi, fz))]
        weights = [wy * wx * wz for (_, wy, _, wx, _, wz) in corners]
        if variant == "corner_swap":
            weights[2], weights[4] = weights[4], weights[2]           # (y_low, x_high, z_low) <-> (y_high, x_low, z_low)
        for (yi, _, xi, _, zi, _), wt in zip(corners, weights):
            cell = np.take(d, (yi * W + xi) * Z + zi, axis=1)
            val += wt * cell
            mag += wt * np.abs(cell)
        low = (ylo * W + xlo) * Z + zlo
        Ly, Lx, Lz = [np.take(m[b].reshape(C, -1), low, axis=1) for m in fld.lip()]
        move = g.ey[ok] * Ly + g.ex[ok] * Lx + g.ez[ok] * Lz
        nb = PH * PW * PZ
        bins = g.bin[ok]
        S = g.count
        count = S
        onehot = np.zeros((ylo.size, nb))
        onehot[np.arange(ylo.size), bins] = 1.0
        tot = val @ onehot
        if variant == "count_inside":
            count = np.maximum(onehot.sum(0), 1.0)
        out = tot / count
        slack = SECOND_ORDER * (move @ onehot + (K_SAMPLE + S) * U * (mag @ onehot)) / count
        und = np.zeros(nb, bool)
        und[g.bin[g.near]] = True
        if g.grid_undecided:
            und[:] = True
        shape3 = (C, PH, PW, PZ)
        if variant == "bin_order":
            out = out.reshape(C, PZ, PW, PH).transpose(0, 3, 2, 1).reshape(C, nb)
        r.values[k] = out.reshape(shape3)
        r.slack[k] = slack.reshape(shape3)
        r.undecided[k] = np.broadcast_to(und.reshape(1, PH, PW, PZ), shape3)
    return r


def _block(t, e, n):
    """per sample, the four cells low - 1 .. low + 2 along one axis: index [S, 4], in-range mask, exact weight, upper
    weight of the fp32 computation (a + e, at most 1; 0 out of range)"""
    lo, hi, f = _hat(t, n)
    idx = lo[:, None] + np.arange(-1, 3)[None, :]
    inr = (idx >= 0) & (idx < n)
    a = np.zeros(idx.shape)
    a[:, 1] = 1 - f
    a[:, 2] = f
    a = np.where(inr, a, 0.0)
    up = np.where(inr & ((a > 0) | (e[:, None] > 0)), np.minimum(a + e[:, None], 1.0), 0.0)
    return np.where(inr, idx, 0), inr, a, up


def backward(grad, rois, scale, out_size, shape, sampling, variant=None):
    """grad [n, C, PH, PW, PZ]; shape = (B, C, H, W, Z).  -> Result: values [B, C, H, W, Z] float64, slack (same shape),
    undecided [B, H, W, Z] (per cell, all planes alike), touched [B, H, W, Z] (cells with a non-zero exact weight),
    contributions [B, H, W, Z] (m of the derivation)"""
    B, C, H, W, Z = shape
    g64 = np.asarray(grad, F).astype(np.float64)
    rois = np.asarray(rois, F).reshape(-1, 8)
    PH, PW, PZ = out_size
    nb = PH * PW * PZ
    g64 = g64.reshape(rois.shape[0], C, nb)
    ncell = H * W * Z
    values = np.zeros((B, C, ncell))
    err = np.zeros((B, C, ncell))
    mag = np.zeros((B, C, ncell))
    m = np.zeros((B, ncell))
    und = np.zeros((B, ncell), bool)
    touched = np.zeros((B, ncell), bool)
    for k in range(rois.shape[0]):
        b = int(rois[k, 0])
        if b < 0 or b >= B:                                           # Q6
            continue
        ge = geometry(rois[k], scale, out_size, sampling, (H, W, Z), True, variant)
        gk = g64[k]
        if variant == "bin_order":
            gk = gk.reshape(C, PH, PW, PZ).transpose(0, 3, 2, 1).reshape(C, nb)
        use = ge.valid | ge.near
        iy, my, ay, uy = _block(ge.y[use], ge.ey[use], H)
        ix, mx, ax, ux = _block(ge.x[use], ge.ex[use], W)
        iz, mz, az, uz = _block(ge.z[use], ge.ez[use], Z)
        cells = ((iy[:, :, None, None] * W + ix[:, None, :, None]) * Z + iz[:, None, None, :]).reshape(-1)
        inr = (my[:, :, None, None] & mx[:, None, :, None] & mz[:, None, None, :]).reshape(-1)
        live = ge.valid[use].astype(np.float64)[:, None, None, None]
        w_ex = ay[:, :, None, None] * ax[:, None, :, None] * az[:, None, None, :] * live
        if variant == "corner_swap":
            w_ex = w_ex.copy()
            t = w_ex[:, 1, 2, 1].copy()
            w_ex[:, 1, 2, 1] = w_ex[:, 2, 1, 1]
            w_ex[:, 2, 1, 1] = t
        w_ex = w_ex.reshape(-1)
        w_up = (uy[:, :, None, None] * ux[:, None, :, None] * uz[:, None, None, :] * live).reshape(-1)
        if ge.near.any() or ge.grid_undecided:
            nearb = np.broadcast_to(ge.near[use][:, None, None, None] | ge.grid_undecided, (int(use.sum()), 4, 4, 4))
            und[b, cells[nearb.reshape(-1) & inr]] = True
        keep = inr & ((w_up > 0) | (w_ex > 0))
        cells, w_ex, w_up = cells[keep], w_ex[keep], w_up[keep]
        bins = np.broadcast_to(ge.bin[use][:, None, None, None], (int(use.sum()), 4, 4, 4)).reshape(-1)[keep]
        uniq, inv = np.unique(cells, return_inverse=True)
        K = uniq.size
        if K == 0:
            continue
        count = ge.count
        if variant == "count_inside":
            count = np.maximum(np.bincount(ge.bin[ge.valid], minlength=nb), 1.0)[:, None]
        flat = bins * K + inv
        M = np.bincount(flat, w_ex, nb * K).reshape(nb, K) / count
        M_up = np.bincount(flat, w_up, nb * K).reshape(nb, K) / count
        E = np.maximum(M_up - M, 0.0) + K_CONTRIB * U * M_up
        ga = np.abs(gk)
        values[b][:, uniq] += gk @ M
        mag[b][:, uniq] += ga @ M
        err[b][:, uniq] += ga @ E
        m[b, uniq] += np.bincount(inv, w_up > 0, K)
        touched[b, uniq] |= M.sum(0) > 0
    m1 = np.maximum(m - 1, 0) * U
    gamma = m1 / (1 - m1)
    r = Result()
    r.values = values.reshape(shape)
    r.slack = (SECOND_ORDER * (err + gamma[:, None, :] * mag)).reshape(shape)
    r.undecided = und.reshape(B, H, W, Z)
    r.touched = touched.reshape(B, H, W, Z)
    r.contributions = m.reshape(B, H, W, Z)
    return r


def linear_map(shape3, roi, scale, out_size, sampling, backward_cuts=False):
    """the operation of ONE ROI on one plane as an explicit matrix [PH PW PZ, H W Z], built by sending the unit fields
    through forward() (one plane per cell); backward_cuts: with the backward pass's upper cut in z (Q3)"""
    H, W, Z = shape3
    n = H * W * Z
    basis = np.eye(n, dtype=F).reshape(1, n, H, W, Z)
    roi = np.asarray(roi, F).copy()
    roi[0] = 0
    out = forward(basis, roi[None], scale, out_size, sampling, "fwd_zcut" if backward_cuts else None)
    return out.values[0].reshape(n, -1).T


# ------------------------------------------------------------------------------------------------ comparison
def compare(got, ref, what=""):
    """got against a Result on its decided entries -> (largest |got - exact| / slack, undecided share, count outside).
    An entry with zero slack must be met exactly (ratio inf otherwise)."""
    got = np.asarray(got, np.float64)
    und = ref.undecided if ref.undecided.shape == ref.values.shape else \
        np.broadcast_to(ref.undecided[:, None], ref.values.shape)
    dec = ~und
    diff = np.abs(got - ref.values)[dec]
    slack = ref.slack[dec]
    bad = int((diff > slack).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / slack)
    worst = float(ratio.max()) if ratio.size else 0.0
    return worst, float(und.mean()) if und.size else 0.0, bad


# ------------------------------------------------------------------------------------------------ case builders
# shared by the host test (oracle within the slack, undecided share) and the GPU test; nothing here reads a device


class Case(object):
    def __init__(self, name, shape, sites, feats, rois, scale, out_size, sampling, exact=False, seed=0):
        self.name, self.shape, self.sites, self.feats = name, tuple(shape), sites, feats
        self.rois, self.scale, self.out_size, self.sampling, self.exact = rois, scale, tuple(out_size), sampling, exact
        self.seed = seed

    def dense(self):
        """[B, C, H, W, Z] float32 over the case's extent (inactive cells zero)"""
        B, C, H, W, Z = self.shape
        d = np.zeros(self.shape, F)
        s = self.sites
        inside = (s[:, 0] < H) & (s[:, 1] < W) & (s[:, 2] < Z) & (s[:, 3] < B)
        s = s[inside]
        d[s[:, 3], :, s[:, 0], s[:, 1], s[:, 2]] = self.feats[inside]
        return d

    def grad(self):
        n = len(self.rois)
        return np.random.default_rng(self.seed + 1000).standard_normal((n, self.shape[1]) + self.out_size).astype(F)


def make_sites(rng, B, H, W, Z, occupancy, few_in=None):
    """unique active sites [V, 4] int32 (y, x, z, b), sorted by sample; the far corner of every sample is active so that
    the occupied extent is the whole map; `few_in`: that sample keeps only its corner and two more sites"""
    rows = []
    for b in range(B):
        if occupancy >= 1.0:
            m = np.ones((H, W, Z), bool)
        else:
            m = rng.random((H, W, Z)) < occupancy
        if few_in == b:
            m[:] = False
            m[0, 0, 0] = m[H // 2, W // 2, Z // 2] = True
        m[H - 1, W - 1, Z - 1] = True
        yxz = np.argwhere(m)
        rows.append(np.concatenate([yxz, np.full((len(yxz), 1), b)], 1))
    return np.concatenate(rows).astype(np.int32)


def random_rois(rng, n, B, H, W, Z, scale, spread=0.1, size=(1.0, 12.0), zsize=(0.5, 6.0)):
    """ROIs drawn like those of the fused-versus-dense test: centres over the map and a margin outside it"""
    r = np.zeros((n, 8), F)
    r[:, 0] = rng.integers(0, B, n)
    r[:, 1] = rng.uniform(-spread * W, (1 + spread) * W, n) / scale
    r[:, 2] = rng.uniform(-spread * H, (1 + spread) * H, n) / scale
    r[:, 3] = rng.uniform(-spread * Z, (1 + spread) * Z, n) / scale
    r[:, 4] = rng.uniform(size[0], size[1], n) / scale
    r[:, 5] = rng.uniform(size[0], size[1], n) / scale
    r[:, 6] = rng.uniform(zsize[0], zsize[1], n) / scale
    r[:, 7] = rng.uniform(-180, 180, n)
    return r


def _case(name, seed, B, C, H, W, Z, rois, scale, out_size, sampling, occupancy=1.0 / 6, few_in=None, exact=False,
          dyadic=False):
    rng = np.random.default_rng(seed)
    sites = make_sites(rng, B, H, W, Z, occupancy, few_in)
    if dyadic:
        feats = (rng.integers(-8, 9, (len(sites), C)) / 4.0).astype(F)
    else:
        feats = rng.standard_normal((len(sites), C)).astype(F)
    rois = rois(rng) if callable(rois) else np.asarray(rois, F)
    return Case(name, (B, C, H, W, Z), sites, feats, rois.reshape(-1, 8), scale, out_size, sampling, exact, seed)


def face_rois(H, W, Z):
    """one ROI straddling each of the six faces, one fully outside on each side, two fully inside; rotated a little so
    that no sample sits on a cut"""
    r = []
    for cw, ch, cz in ((0.3, H / 2, Z / 2), (W - 0.2, H / 2, Z / 2), (W / 2, -0.1, Z / 2), (W / 2, H - 0.4, Z / 2),
                       (W / 2, H / 2, -0.3), (W / 2, H / 2, Z - 0.2)):
        r.append([0, cw, ch, cz, 4.3, 3.7, 2.9, 17.0])
    for cw, ch, cz in ((-9.0, H / 2, Z / 2), (W + 9.0, H / 2, Z / 2), (W / 2, -9.0, Z / 2), (W / 2, H + 9.0, Z / 2),
                       (W / 2, H / 2, -7.0), (W / 2, H / 2, Z + 7.0)):
        r.append([0, cw, ch, cz, 4.3, 3.7, 2.9, -28.0])
    r.append([0, W / 2, H / 2, Z / 2, 3.1, 2.6, 1.7, 61.0])
    r.append([0, W / 2 + 0.4, H / 2 - 0.3, Z / 2, 0.3, 0.2, 0.4, -5.0])      # Q1: below one cell
    return np.array(r, F)


def boundary_case():
    """hand-placed samples ON the cuts, from values exact in fp32 (theta = 0, dyadic centres / sizes / scale 0.5, dyadic
    features): H, W, Z = 8, 6, 4, bins (2, 2, 2), two samples per axis.  After scaling every box is 4 x 4 x 4 cells, so
    its samples sit at centre + {-1.5, -0.5, 0.5, 1.5} per axis.  Boxes, by (centre_w, centre_h, centre_z) in cells:
      (2.5, 0.5, 1.5)  y = -1 exactly (kept: the cut is y < -1), then 0, 1, 2
      (2.5, 6.5, 1.5)  y = 5, 6, 7 and y = H = 8 exactly (kept: the cut is y > H)
      (0.5, 3.5, 1.5)  x = -1 exactly;   (4.5, 3.5, 1.5)  x = W = 6 exactly
      (2.5, 3.5, 0.5)  z = -1 exactly
      (2.5, 3.5, 3.5)  z = 2, 3, Z = 4 exactly, 5: forward reads the last slice for both, backward keeps 4 and cuts 5
      (2.5, 3.5, 4.5)  z = 3 .. 6
      (0, 0, 0) and (5, 7, 3)  a half step further out: samples at -1.5 (cut), at y = 8.5 and x = 6.5 (cut)
      (2.5, 3.5, 9.5)  every z sample above Z: last slice forward, nothing backward
    ROI fields are given before scaling (scale 0.5: twice the cell values)."""
    H, W, Z = 8, 6, 4

    def roi(cw, ch, cz, w=4.0, h=4.0, z=4.0):
        return [0, 2 * cw, 2 * ch, 2 * cz, 2 * w, 2 * h, 2 * z, 0.0]
    rois = [roi(2.5, 0.5, 1.5), roi(2.5, 6.5, 1.5), roi(0.5, 3.5, 1.5), roi(4.5, 3.5, 1.5), roi(2.5, 3.5, 0.5),
            roi(2.5, 3.5, 3.5), roi(2.5, 3.5, 4.5), roi(0.0, 0.0, 0.0), roi(5.0, 7.0, 3.0),
            roi(2.5, 3.5, 9.5)]
    return _case("boundary_exact", 501, 1, 3, H, W, Z, rois, 0.5, (2, 2, 2), 2, occupancy=1.0, exact=True, dyadic=True)


def gpu_cases():
    """every input set of tests/test_gpu_roi_align.py.  Sizes are small enough for the numpy reference; maps are
    non-cubic so that no two axes can be confused."""
    cs = []

    def rr(n, B, H, W, Z, scale, **kw):
        return lambda rng: random_rois(rng, n, B, H, W, Z, scale, **kw)
    # planes: the fused kernel's 128-plane groups, the c_ok tail, blockIdx.y > 0
    for C in (1, 127, 128, 129, 257):
        cs.append(_case("planes_%d" % C, 10 + C, 2, C, 11, 9, 5, rr(6, 2, 11, 9, 5, 1.0, size=(1.0, 7.0)), 1.0,
                        (2, 3, 2), 2))
    # bins per ROI: the 96-bin LDS passes and the odd / even split between the two half-workgroups
    for out_size in ((1, 1, 1), (5, 19, 1), (4, 6, 4), (1, 97, 1), (8, 6, 4), (193, 1, 1), (5, 6, 11)):
        cs.append(_case("bins_%dx%dx%d" % out_size, 40 + sum(out_size), 2, 5, 13, 10, 6,
                        rr(8, 2, 13, 10, 6, 1.0), 1.0, out_size, 1 if np.prod(out_size) > 150 else 2))
    # ROI counts 0 and 1
    cs.append(_case("rois_0", 60, 1, 4, 9, 7, 4, np.zeros((0, 8), F), 1.0, (2, 2, 2), 2))
    cs.append(_case("rois_1", 61, 1, 4, 9, 7, 4, [[0, 3.2, 4.1, 1.9, 4.4, 5.2, 2.1, 33.0]], 1.0, (2, 2, 2), 2))
    # more outputs than 8192 x 256: the dense kernel's grid-stride loop runs twice.  Few ROIs with many planes cost
    # the reference less than many ROIs with few planes (its Python loop is over ROIs): 112 x 128 x 147 > 2^21
    cs.append(_case("grid_stride", 62, 2, 128, 12, 10, 5, rr(112, 2, 12, 10, 5, 1.0, size=(2.0, 9.0)), 1.0, (7, 7, 3),
                    1, occupancy=0.5))
    # sampling ratio 1, 2, 3 and adaptive with three different grids (sizes 11 x 5.2 x 2.9 over 2 x 2 x 2 bins: 6, 3, 2)
    for s in (1, 2, 3):
        cs.append(_case("sampling_%d" % s, 70 + s, 2, 6, 14, 11, 6, rr(10, 2, 14, 11, 6, 1.0), 1.0, (3, 2, 2), s))
    cs.append(_case("sampling_adaptive", 74, 1, 6, 16, 13, 7,
                    [[0, 6.1, 7.9, 3.2, 5.2, 11.0, 2.9, 24.0], [0, 5.0, 8.0, 3.0, 9.3, 4.1, 5.7, -71.0],
                     [0, 7.7, 6.6, 2.0, 0.4, 13.1, 1.1, 140.0]], 1.0, (2, 2, 2), 0))
    # spatial scale 1, 0.5 and a non-dyadic one
    for i, sc in enumerate((0.5, 0.3)):
        cs.append(_case("scale_%g" % sc, 80 + i, 2, 6, 14, 11, 6, rr(10, 2, 14, 11, 6, sc), sc, (3, 3, 2), 2))
    # angles
    H, W, Z = 15, 12, 5
    ang = [0.0, 90.0, -90.0, 180.0, -180.0, 179.999, -179.999, 180.001, 89.9995, 360.0, 725.0, -1083.0, 45.0, 1e-3]
    cs.append(_case("angles", 90, 1, 6, H, W, Z, [[0, 5.6, 7.3, 2.4, 5.3, 7.1, 2.6, a] for a in ang], 1.0, (3, 2, 2), 2))
    # faces: inside, straddling each face, outside on each side, below one cell
    cs.append(_case("faces", 91, 1, 6, H, W, Z, face_rois(H, W, Z), 1.0, (2, 3, 2), 2, occupancy=1.0))
    cs.append(boundary_case())
    # batch of three, the middle sample with few sites; every valid batch index used
    cs.append(_case("batch3_thin_middle", 92, 3, 6, 12, 10, 5, rr(18, 3, 12, 10, 5, 1.0), 1.0, (2, 2, 2), 2, few_in=1))
    # a 1 along an axis: both corners of that axis are the same cell
    cs.append(_case("z_is_1", 93, 2, 6, 12, 9, 1, rr(10, 2, 12, 9, 1, 1.0, zsize=(0.5, 2.0)), 1.0, (3, 2, 2), 2))
    cs.append(_case("h_is_1", 94, 1, 6, 1, 9, 4, rr(8, 1, 1, 9, 4, 1.0, size=(1.0, 4.0)), 1.0, (2, 3, 2), 2))
    cs.append(_case("w_is_1", 95, 1, 6, 9, 1, 4, rr(8, 1, 9, 1, 4, 1.0, size=(1.0, 4.0)), 1.0, (2, 3, 2), 2))
    # occupancy: dense, typical, one active site
    cs.append(_case("occupancy_dense", 96, 2, 6, 12, 10, 5, rr(10, 2, 12, 10, 5, 1.0), 1.0, (3, 3, 2), 2, occupancy=1.0))
    cs.append(_case("occupancy_one_site", 97, 1, 6, 7, 5, 3, rr(10, 1, 7, 5, 3, 1.0, size=(2.0, 6.0)), 1.0, (3, 3, 2), 2,
                    occupancy=0.0))
    # backward contention: many identical ROIs on one spot
    cs.append(_case("contention", 98, 1, 4, 10, 8, 4, np.tile(np.array([[0, 3.7, 5.2, 1.6, 2.2, 1.9, 1.3, 21.0]], F),
                                                                (300, 1)), 1.0, (2, 2, 2), 2, occupancy=1.0))
    # the larger random set the undecided-share figure of the suite is about
    cs.append(_case("random_40x33x7", 99, 2, 3, 40, 33, 7, rr(60, 2, 40, 33, 7, 0.9), 0.9, (7, 7, 3), 2))
    return cs


def batch_index_case():
    """Q6: ROIs that name sample B (a trailing empty sample the module cropped away) and sample -1, among valid ones"""
    H, W, Z = 10, 8, 4
    rois = [[0, 3.2, 4.1, 1.9, 4.4, 5.2, 2.1, 33.0], [2, 3.2, 4.1, 1.9, 4.4, 5.2, 2.1, 33.0],
            [1, 4.0, 5.0, 2.0, 3.0, 3.0, 2.0, -12.0], [-1, 4.0, 5.0, 2.0, 3.0, 3.0, 2.0, -12.0],
            [2, 1.0, 1.0, 1.0, 9.0, 9.0, 9.0, 0.0], [1, 6.1, 2.2, 3.0, 2.0, 6.0, 1.5, 77.0]]
    return _case("batch_index", 120, 2, 130, H, W, Z, rois, 1.0, (2, 3, 2), 2)
