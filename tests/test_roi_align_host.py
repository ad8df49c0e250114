"""The rotated 3-D ROI-align yardstick (tests/roi_align_ref.py) checked without a GPU: against itself (transpose, adjoint),
against torch on cases with a closed form (these fix the conventions independently of any kernel text), and against
oracle/roi_oracle.c -- the kernel's fp32 statement sequence on the CPU -- which must lie within the derived slack on
every input set the GPU test uses and must be REJECTED by every deliberately wrong variant of the reference."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import roi_align_ref as R

F = np.float32
CASES = R.gpu_cases()
IDS = [c.name for c in CASES]
RANDOMISED = [c for c in CASES if not c.exact]


def _field(rng, C, H, W, Z, B=1):
    return rng.standard_normal((B, C, H, W, Z)).astype(F)


# ------------------------------------------------------------------------------------------ reference against itself
@pytest.mark.parametrize("sampling,theta,cz", [(2, 27.0, 1.4), (0, -64.0, 2.9), (1, 0.0, 3.6)])
def test_scatter_backward_equals_explicit_transpose(sampling, theta, cz):
    """backward() builds its weights by scatter-adds; linear_map() sends unit fields through forward().  Small map with
    the box partly outside, the last z case reaching above the map (the backward pass's own z cut)"""
    rng = np.random.default_rng(3)
    H, W, Z, C = 6, 5, 3, 2
    roi = np.array([0, 1.7, 2.9, cz, 4.6, 3.3, 2.7, theta], F)
    out_size = (2, 3, 2)
    M = R.linear_map((H, W, Z), roi, 1.0, out_size, sampling, backward_cuts=True)
    g = rng.standard_normal((1, C) + out_size)
    want = g.astype(F).astype(np.float64).reshape(C, -1) @ M
    got = R.backward(g, roi[None], 1.0, out_size, (1, C, H, W, Z), sampling)
    np.testing.assert_allclose(got.values.reshape(C, -1), want, rtol=0, atol=1e-14)
    assert (got.touched.reshape(-1) == (M.sum(0) > 0)).all()
    # and forward is that matrix on the field
    x = _field(rng, C, H, W, Z)
    Mf = R.linear_map((H, W, Z), roi, 1.0, out_size, sampling)
    np.testing.assert_allclose(R.forward(x, roi[None], 1.0, out_size, sampling).values.reshape(C, -1),
                               x.astype(np.float64).reshape(C, -1) @ Mf.T, rtol=0, atol=1e-13)


def test_adjoint_identity_in_fp64():
    """<g, F(x)> = <B(g), x>, with F taken with the backward pass's upper cut in z (Q3: the forward pass proper reads the
    last slice for samples above the map, the backward pass drops them, so the plain pair is adjoint only when no sample
    lies above the map; the GPU test's adjoint case is built that way)"""
    c = next(k for k in CASES if k.name == "sampling_2")
    x = c.dense()
    g = c.grad()
    f = R.forward(x, c.rois, c.scale, c.out_size, c.sampling, "fwd_zcut")
    b = R.backward(g, c.rois, c.scale, c.out_size, c.shape, c.sampling)
    lhs = float((g.astype(np.float64) * f.values).sum())
    rhs = float((b.values * x.astype(np.float64)).sum())
    scale = float(np.abs(g.astype(np.float64) * f.values).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale and scale > 1


# ------------------------------------------------------------------------------------------ closed forms (torch)
def test_integer_aligned_roi_is_indexing_and_average_pooling():
    """theta = 0; coordinate i is cell i, so a box that starts half a sample step before cell y0 samples cell centres"""
    rng = np.random.default_rng(5)
    H, W, Z = 12, 10, 7
    x = _field(rng, 3, H, W, Z, B=2)
    y0, x0, z0, PH, PW, PZ = 3, 2, 1, 4, 3, 2
    roi = np.array([[1, x0 + PW / 2 - .5, y0 + PH / 2 - .5, z0 + PZ / 2 - .5, PW, PH, PZ, 0.0]], F)
    out = R.forward(x, roi, 1.0, (PH, PW, PZ), 1)
    assert (out.values[0] == x[1, :, y0:y0 + PH, x0:x0 + PW, z0:z0 + PZ]).all()
    assert out.coord_slack[0] == 0.0 and not out.undecided.any()
    roi2 = np.array([[1, x0 + PW - .5, y0 + PH - .5, z0 + PZ - .5, 2 * PW, 2 * PH, 2 * PZ, 0.0]], F)
    out2 = R.forward(x, roi2, 1.0, (PH, PW, PZ), 2)
    crop = torch.from_numpy(x[1:2, :, y0:y0 + 2 * PH, x0:x0 + 2 * PW, z0:z0 + 2 * PZ]).double()
    want = torch.nn.functional.avg_pool3d(crop, 2)[0].numpy()
    np.testing.assert_allclose(out2.values[0], want, rtol=0, atol=1e-15)
    # the same through a spatial scale: fields twice as large at scale 0.5
    out3 = R.forward(x, roi2 * np.array([1, 2, 2, 2, 2, 2, 2, 1], F), 0.5, (PH, PW, PZ), 2)
    assert (out3.values == out2.values).all()


@pytest.mark.parametrize("theta", [90.0, -90.0, 180.0])
def test_quarter_turns_equal_the_unrotated_result_on_the_turned_map(theta):
    """x = xx cos + yy sin + cw, y = yy cos - xx sin + ch.  At +90 the box's h axis runs along +x of the map and its w
    axis along -y: on the map m'[i, j] = m[H - 1 - j, i] (first axis = old x, second = old y reversed) the same box is
    unrotated with centre (cw', ch') = (H - 1 - ch, cw).  At -90: h along -x, w along +y: m'[i, j] = m[j, W - 1 - i],
    centre (ch, W - 1 - cw).  At 180: both reversed.  Pins the rotation's sign and which axis w and h name."""
    rng = np.random.default_rng(7)
    H, W, Z = 16, 13, 5
    x = _field(rng, 2, H, W, Z)
    cw, ch = 6.3, 7.9
    box = [3.1, 5.7, 2.2]                                    # w != h, and PH != PW below
    out_size = (3, 2, 2)
    got = R.forward(x, np.array([[0, cw, ch, 2.1] + box + [theta]], F), 1.0, out_size, 2).values
    if theta == 90.0:
        turned, cw2, ch2 = x.transpose(0, 1, 3, 2, 4)[:, :, :, ::-1], H - 1 - ch, cw
    elif theta == -90.0:
        turned, cw2, ch2 = x.transpose(0, 1, 3, 2, 4)[:, :, ::-1, :], ch, W - 1 - cw
    else:
        turned, cw2, ch2 = x[:, :, ::-1, ::-1], W - 1 - cw, H - 1 - ch
    want = R.forward(np.ascontiguousarray(turned), np.array([[0, cw2, ch2, 2.1] + box + [0.0]], F), 1.0, out_size,
                     2).values
    # float32(pi / 2) is not pi / 2: cos = -4.4e-8, and the float32 centres differ by an ulp: 1e-5 covers both
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    wrong = R.forward(x, np.array([[0, cw, ch, 2.1] + box + [theta]], F), 1.0, out_size, 2, "rot_sign").values
    assert theta == 180.0 or np.abs(wrong - want).max() > 0.1


def test_affine_field_gives_the_field_at_the_bin_centre():
    rng = np.random.default_rng(9)
    H, W, Z = 40, 36, 12
    yy, xx, zz = np.meshgrid(np.arange(H), np.arange(W), np.arange(Z), indexing="ij")
    a = np.array([0.5, -1.25, 0.75, 2.0])
    x = (a[0] + a[1] * yy + a[2] * xx + a[3] * zz)[None, None].astype(F)      # exact in fp32
    PH, PW, PZ = 3, 4, 2
    for theta in (0.0, 31.0, -117.0, 200.0):
        w, h, z = 7.5, 5.25, 3.5
        cw, ch, cz = 17.5, 19.25, 5.5
        out = R.forward(x, np.array([[0, cw, ch, cz, w, h, z, theta]], F), 1.0, (PH, PW, PZ), 3).values[0, 0]
        t = float(F(theta * np.pi / 180))
        by = (-h / 2 + (np.arange(PH) + .5) * h / PH)[:, None, None]
        bx = (-w / 2 + (np.arange(PW) + .5) * w / PW)[None, :, None]
        bz = (-z / 2 + (np.arange(PZ) + .5) * z / PZ)[None, None, :]
        want = a[0] + a[1] * (by * np.cos(t) - bx * np.sin(t) + ch) + a[2] * (bx * np.cos(t) + by * np.sin(t) + cw) + \
            a[3] * (bz + cz)
        np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)


def test_constant_field_counts_the_samples_inside():
    H, W, Z = 8, 6, 4
    x = np.ones((1, 1, H, W, Z), F)
    inside = R.forward(x, np.array([[0, 2.6, 3.7, 1.8, 2.9, 3.3, 1.7, 40.0]], F), 1.0, (2, 2, 2), 2)
    np.testing.assert_allclose(inside.values, 1.0, rtol=0, atol=1e-15)
    # box 4 x 4 x 4 centred on (x, y, z) = (0, 0, 0), two samples per bin and axis at -1.5 (cut), -0.5, 0.5, 1.5
    out = R.forward(x, np.array([[0, 0, 0, 0, 4, 4, 4, 0.0]], F), 1.0, (2, 2, 2), 2).values[0, 0]
    k = np.array([1, 2])                                      # samples inside, per axis, of the low and the high bin
    want = k[:, None, None] * k[None, :, None] * k[None, None, :] / 8.0
    assert (out == want).all()


def test_small_roi_behaves_as_one_cell_and_z_overshoot():
    rng = np.random.default_rng(11)
    H, W, Z = 9, 8, 4
    x = _field(rng, 2, H, W, Z)
    small = np.array([[0, 3.3, 4.4, 1.6, 0.2, 0.4, 0.01, 25.0]], F)
    one = small.copy()
    one[0, 4:7] = 1.0
    assert (R.forward(x, small, 1.0, (2, 2, 2), 2).values == R.forward(x, one, 1.0, (2, 2, 2), 2).values).all()
    assert (R.forward(x, small * np.array([1, 2, 2, 2, 2, 2, 2, 1], F), 0.5, (2, 2, 2), 0).values ==
            R.forward(x, one, 1.0, (2, 2, 2), 1).values).all()
    # every z sample above Z: forward reads the last slice, backward adds nothing
    over = np.array([[0, 3.0, 4.0, 9.5, 2, 2, 2, 0.0]], F)          # samples at y 3.5 / 4.5, x 2.5 / 3.5, z 9 / 10
    out = R.forward(x, over, 1.0, (2, 2, 2), 1)
    xs = x.astype(np.float64)
    want = 0.25 * (xs[0, :, 3:5, 2:4, Z - 1][:, :-1, :-1] + xs[0, :, 3:5, 2:4, Z - 1][:, 1:, :-1] +
                   xs[0, :, 3:5, 2:4, Z - 1][:, :-1, 1:] + xs[0, :, 3:5, 2:4, Z - 1][:, 1:, 1:])
    want = 0.25 * (xs[0, :, 3:6, 2:5, Z - 1][:, :-1, :-1] + xs[0, :, 3:6, 2:5, Z - 1][:, 1:, :-1] +
                   xs[0, :, 3:6, 2:5, Z - 1][:, :-1, 1:] + xs[0, :, 3:6, 2:5, Z - 1][:, 1:, 1:])
    np.testing.assert_allclose(out.values[0], np.repeat(want[..., None], 2, -1), rtol=0, atol=1e-15)
    back = R.backward(np.ones((1, 2, 2, 2, 2), F), over, 1.0, (2, 2, 2), (1, 2, H, W, Z), 1)
    assert not back.values.any() and not back.touched.any()


def test_batch_index_outside_the_input_is_an_empty_sample():
    c = R.batch_index_case()
    f = R.forward(c.dense(), c.rois, c.scale, c.out_size, c.sampling)
    outside = (c.rois[:, 0] < 0) | (c.rois[:, 0] >= c.shape[0])
    assert outside.sum() == 3 and not f.values[outside].any() and not f.slack[outside].any()
    assert np.abs(f.values[~outside]).min(axis=(1, 2, 3, 4)).max() > 0
    b = R.backward(c.grad(), c.rois, c.scale, c.out_size, c.shape, c.sampling)
    b2 = R.backward(c.grad()[~outside], c.rois[~outside], c.scale, c.out_size, c.shape, c.sampling)
    assert (b.values == b2.values).all()


# ------------------------------------------------------------------------------------------ the slack and the oracle
_memo = {}


def _both(case):
    """fp64 reference and fp32 oracle, forward and backward, of one case (memoised: three tests read them)"""
    if case.name not in _memo:
        x, g = case.dense(), case.grad()
        ref_f = R.forward(x, case.rois, case.scale, case.out_size, case.sampling)
        ref_b = R.backward(g, case.rois, case.scale, case.out_size, case.shape, case.sampling)
        if len(case.rois):
            orc_f = O.roi_align_rot3d_fwd(x, case.rois, case.scale, case.out_size, case.sampling)
            orc_b = O.roi_align_rot3d_bwd(g, case.rois, case.scale, case.out_size, case.shape, case.sampling)
        else:
            orc_f, orc_b = np.zeros(ref_f.values.shape, F), np.zeros(case.shape, F)
        _memo[case.name] = (ref_f, ref_b, orc_f, orc_b)
    return _memo[case.name]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_lies_within_the_slack(case):
    """the bound is not too tight: the kernel's fp32 statement sequence, run on the CPU, meets it on every decided
    output of every input set the GPU test uses"""
    ref_f, ref_b, orc_f, orc_b = _both(case)
    wf, uf, bad_f = R.compare(orc_f, ref_f)
    wb, ub, bad_b = R.compare(orc_b, ref_b)
    print("%s: oracle |err| / slack forward %.3g backward %.3g; undecided %.4f / %.4f" % (case.name, wf, wb, uf, ub))
    assert bad_f == 0 and bad_b == 0, (wf, wb)
    assert np.isfinite(ref_f.slack).all() and np.isfinite(ref_b.slack).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_undecided_share_is_small(case):
    ref_f, ref_b = _both(case)[:2]
    fwd = ref_f.undecided.mean() if ref_f.undecided.size else 0.0
    bwd = (ref_b.undecided & ref_b.touched).sum() / max(ref_b.touched.sum(), 1)
    if case.exact:
        assert fwd == 0 and bwd == 0 and (ref_f.coord_slack == 0).all()
    else:
        assert fwd <= 0.01 and bwd <= 0.01, (fwd, bwd)


def test_boundary_case_sits_on_the_cuts():
    """the hand-placed case does what its docstring says: samples exactly on y = -1, y = H, x = -1, x = W, z = -1 and
    z = Z, kept; the ones a half step further out, cut"""
    c = R.boundary_case()
    H, W, Z = c.shape[2:]
    on = {"y-1": 0, "yH": 0, "x-1": 0, "xW": 0, "z-1": 0, "zZ": 0}
    for roi in c.rois:
        for backward in (False, True):
            g = R.geometry(roi, c.scale, c.out_size, c.sampling, (H, W, Z), backward)
            assert g.coord_slack == 0 and not g.near.any()
            on["y-1"] += int((g.valid & (g.y == -1)).sum())
            on["yH"] += int((g.valid & (g.y == H)).sum())
            on["x-1"] += int((g.valid & (g.x == -1)).sum())
            on["xW"] += int((g.valid & (g.x == W)).sum())
            on["z-1"] += int((g.valid & (g.z == -1)).sum())
            on["zZ"] += int((g.valid & (g.z == Z)).sum())
            assert not (g.valid & ((g.y < -1) | (g.y > H) | (g.x < -1) | (g.x > W) | (g.z < -1))).any()
            assert backward or g.valid[(g.z > Z) & (g.y >= 0) & (g.y <= H) & (g.x >= 0) & (g.x <= W)].all()
            assert not backward or not g.valid[g.z > Z].any()
    assert min(on.values()) > 0, on


TEETH = [c for c in CASES if c.name in ("random_40x33x7", "sampling_adaptive", "faces", "bins_4x6x4", "boundary_exact")]


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_variants_are_rejected(variant):
    """the bound has teeth: the oracle's output does NOT pass against a reference with one convention changed"""
    rejected_f, rejected_b = [], []
    for case in TEETH:
        x, g = case.dense(), case.grad()
        _, _, orc_f, orc_b = _both(case)
        bad = R.forward(x, case.rois, case.scale, case.out_size, case.sampling, variant)
        if R.compare(orc_f, bad)[2] > 0:
            rejected_f.append(case.name)
        if variant != "fwd_zcut":                           # (the backward pass has that cut by definition)
            badb = R.backward(g, case.rois, case.scale, case.out_size, case.shape, case.sampling, variant)
            if R.compare(orc_b, badb)[2] > 0:
                rejected_b.append(case.name)
    assert rejected_f, variant
    assert rejected_b or variant == "fwd_zcut", variant
    if variant not in ("fwd_zcut", "count_inside"):         # (those two need samples outside the map to show)
        assert "random_40x33x7" in rejected_f and "random_40x33x7" in rejected_b
