"""tests/label_ref.py without a GPU: its matrices against the C oracle, and every case of tests/test_gpu_label_edges.py
checked for what its name claims -- on the definition's own matrix, so a case that does not reach its edge fails here,
before a GPU is used."""
import numpy as np
import pytest

import label_ref as L
import oracle_lib as O

CASES = L.cases()


def _examples(case):
    return [b for b in range(case.nb) if case.n_anchors(b) and len(case.targets[b])]


def _mq32(case, b):
    m = L.matrix(case, b)
    with np.errstate(invalid="ignore"):
        return m["ref32"] if m["ref32"] is not None else m["ref"].astype(np.float32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matrices_agree_with_the_oracle(name):
    """criterion 6 (with and without the z factor) and criterion -1 against oracle/iou_oracle.c at the project's 2e-5"""
    case = CASES[name]
    seen = 0
    for b in _examples(case):
        an, tg = L.anchors(case, b), case.targets[b]
        want = O.boxes_iou_3d(tg, an, case.aug, case.criterion, bool(case.only_xy))
        got = L.matrix(case, b)["ref"]
        assert got.shape == want.shape == (len(tg), case.n_anchors(b))
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, atol=2e-5, rtol=0)           # NaN at the same places counts as equal
        seen += got.size
    assert seen > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_yaw_mask_is_decidable(name):
    """no |wrapped yaw difference| within 1e-3 of the yaw threshold in use (3.0 means no mask at all)"""
    case = CASES[name]
    for b in _examples(case):
        assert L.yaw_margin(case.targets[b], L.anchors(case, b), 0.7) > 1e-3


def test_lattice_keeps_the_kernels_subtractions_exact():
    for name, case in CASES.items():
        if case.criterion != 6:
            continue
        for b in _examples(case):
            an, tg = L.anchors(case, b).astype(np.float64), case.targets[b].astype(np.float64)
            assert (an * 16 == np.round(an * 16))[:, :6].all() and (tg * 16 == np.round(tg * 16))[:, :6].all(), name
            assert np.abs(an[:, :6]).max() < 1024 and np.abs(tg[:, :6]).max() < 1024


@pytest.mark.parametrize("G", L.CHUNK_G)
def test_chunk_cases_reach_their_edges(G):
    case = CASES["chunk_G%d" % G]
    an, tg = L.anchors(case, 0), case.targets[0]
    assert an.shape[0] == 204 and tg.shape[0] == G
    mq = _mq32(case, 0)
    lab, vals = L.labels(mq, tg, an, case.fg, case.bg, True, 0.7)
    plain, _ = L.labels(mq, tg, an, case.fg, case.bg, False, 0.7)
    if G >= 127:
        assert {-2, -1} <= set(lab.tolist()) and (lab >= 0).any()
        assert {-2, -1} <= set(plain.tolist()) and (plain >= 0).any()
        assert (lab != plain).any()                                    # the low-quality pass acts
    else:
        assert (lab >= 0).any() and (lab == -1).any()
    mm = L.masked(mq, tg, an, 0.7)
    tied_rows = ((mm == mm.max(1, keepdims=True)).sum(1) > 1).sum()
    assert tied_rows >= 1                                              # a row maximum attained by several anchors
    if G > 128:
        assert G == 129 or ((lab >= 128).any() and (plain >= 128).any())     # G = 129: box 128 is the later copy
        # an anchor whose best value is attained on both sides of index 128
        top = mm == mm.max(0, keepdims=True)
        both = top[:128].any(0) & top[128:].any(0)
        assert both.any()
        assert (lab[both] < 128).all() or (lab[both] < 0).any()
    for first, later in case.duplicates:
        assert (tg[first] == tg[later]).all()
        assert not (lab == later).any() and not (plain == later).any()
        assert (lab == first).any() and (plain == first).any()         # the earlier copy does get its anchor
        assert (mm[first] == 1.0).any() and (mm[first] == mm[later]).all()
    assert case.duplicates == tuple(p for p in L.DUPLICATES if p[1] < G)


def test_threshold_case_attains_both_thresholds():
    case = CASES["chunk_G129"]
    an, tg = L.anchors(case, 0), case.targets[0]
    mq = _mq32(case, 0)
    _, vals = L.labels(mq, tg, an, case.fg, case.bg, False, 0.7)
    fg, bg = L.attained_thresholds(vals)
    assert bg < fg and np.float32(fg) == fg and np.float32(bg) == bg
    lab, vals = L.labels(mq, tg, an, fg, bg, False, 0.7)
    assert (vals == fg).any() and (vals == bg).any()
    assert (lab[vals == fg] >= 0).all() and (lab[vals == bg] == -2).all()


def test_ragged_cases_reach_their_edges():
    a, b = CASES["ragged_a"], CASES["ragged_b"]
    assert a.nb == b.nb == 16 and a.A == 4 and b.A == 1
    shape = [(a.n_anchors(e), len(a.targets[e])) for e in range(16)]
    assert {(4, 129), (0, 3), (1100, 0), (1100, 257), (4, 1)} <= set(shape)
    assert len({g for _, g in shape}) > 8                              # the row-maximum prefix is not regular
    assert any(a.counts[m][e] == 0 and a.n_anchors(e) for m in range(3) for e in range(16))
    assert {255, 256, 257, 0} <= {b.n_anchors(e) for e in range(16)}
    for case in (a, b):
        lab = [L.labels(_mq32(case, e), case.targets[e], L.anchors(case, e), case.fg, case.bg, True, 0.7)[0]
               for e in _examples(case)]
        assert {-2, -1} <= set(np.concatenate(lab).tolist()) and any((v >= 128).any() for v in lab)


def test_yaw_case_masks_a_whole_row():
    case = CASES["yaw"]
    an, tg = L.anchors(case, 0), case.targets[0]
    assert case.A == 2 and (np.abs(tg[:, 6]) > np.pi / 2).sum() >= 2
    mq = _mq32(case, 0)
    mm = L.masked(mq, tg, an, 0.7)
    assert (mm[3] == 0).all() and mm[3].max() == 0 and np.signbit(mm[3]).any()      # a row maximum of +-0
    assert (mm.max(1)[[0, 1, 2, 4]] > 0).all()
    lab, _ = L.labels(mq, tg, an, case.fg, case.bg, True, 0.7)
    assert (lab >= 0).all()                    # every anchor ties with row 3's maximum (matcher.py:126-128)
    nomask, _ = L.labels(mq, tg, an, case.fg, case.bg, True, 3.0)
    off, _ = L.labels(mq, tg, an, case.fg, case.bg, False, 0.7)
    assert (nomask < 0).any() and {-2, -1} <= set(off.tolist()) and (off >= 0).any()
    assert (L.labels(mq, tg, an, case.fg, case.bg, False, 3.0)[0] != off).any()     # the mask acts


@pytest.mark.parametrize("name", ["z_clamped", "z_plain"])
def test_z_cases_overlap_touch_and_lie_apart(name):
    case = CASES[name]
    an, tg = L.anchors(case, 0), case.targets[0]
    q, exact = L.z_factor(tg, an, case.aug)
    assert exact and np.isfinite(q).all()
    assert (q > 0).any() and (q == 0).any() and (q < 0).any()
    ref = L.matrix(case, 0)["ref"]
    assert (ref[q < 0] > 0).any()              # a negative factor on a negative criterion-6 value: a positive entry
    lab, _ = L.labels(ref.astype(np.float32), tg, an, case.fg, case.bg, True, 0.7)
    assert {-2, -1} <= set(lab.tolist()) and (lab >= 0).any()


def test_nan_case_has_nan_beside_finite_entries():
    case = CASES["nan"]
    an, tg = L.anchors(case, 0), case.targets[0]
    mq = _mq32(case, 0)
    nan = np.isnan(mq)
    assert nan[1].any() and nan[4].any() and not nan[[0, 2, 3, 5]].any() and not nan.all(0).any()
    assert np.isfinite(mq[2][nan[1]]).all()                            # the finite neighbour at the same z
    for allow in (True, False):
        lab, vals = L.labels(mq, tg, an, case.fg, case.bg, allow, 0.7)
        assert np.array_equal(np.isnan(vals), nan.any(0))
        assert (lab[nan[1]] == 1).all() and (lab[nan[4] & ~nan[1]] == 4).all()      # NaN wins, the first one by index
        # a matcher in which NaN never wins labels these anchors differently
        never = np.where(nan, -np.inf, mq).astype(np.float32)
        other, _ = L.labels(never, tg, an, case.fg, case.bg, allow, 0.7)
        assert (other[nan.any(0)] != lab[nan.any(0)]).any()


def test_ulp_distance():
    a = np.array([1.0, -0.0, 0.0, -1.0, 0.55], np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), 0.0, np.float32(1e-45), -1.0, 0.55], np.float32)
    assert L.ulp_distance(a, b).tolist() == [1, 0, 1, 0, 0]
