"""The multi-level ROI pooler without a GPU: the restatement (tests/roi_pool_ref.py) against the golden the reference's own
classes produced (tests/golden/pooler_golden.npz), the C ABI's argument checks (each returns before any HIP call), the
Python surface's refusals, and the fp64 yardstick's undecided share on the inputs of tests/test_gpu_roi_pool.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import roi_pool_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("aabr_roi_pool_prepare", "aabr_roi_pool_forward", "aabr_roi_pool_backward")
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "pooler_golden.npz"))


def golden_set(k):
    counts = GOLDEN[k + "_counts"]
    scenes = np.split(GOLDEN[k + "_boxes"], np.cumsum(counts)[:-1])
    return (scenes, float(GOLDEN[k + "_box_scale"]), tuple(GOLDEN[k + "_scales"].tolist()),
            float(GOLDEN[k + "_canonical_size"]), GOLDEN[k + "_rois"], GOLDEN[k + "_levels"])


@pytest.mark.parametrize("k", ["a", "b", "c"])
def test_restatement_reproduces_the_reference_golden(k):
    scenes, box_scale, scales, cs, rois, levels = golden_set(k)
    got_rois, got_levels = P.rois_and_levels(scenes, box_scale, scales, cs)
    assert (got_levels == levels).all()
    assert got_rois.dtype == F and got_rois.shape == rois.shape
    assert got_rois.tobytes() == rois.tobytes()                     # bit for bit, the NaN sizes of set b included
    assert set(levels.tolist()) == set(range(len(scales)))          # sizes that land on every level


def test_golden_holds_the_edges_it_is_meant_to():
    scenes, _, scales, cs, rois, levels = golden_set("b")
    b = scenes[0]
    assert scales == (0.5, 0.25) and cs == 8.0
    assert b[0, 3] == 9.0 and b[1, 4] == 9.0 and levels[0] == 0 and levels[1] == 0           # the exact tie: level 0
    assert abs(0.5 - 3.0 / 8) == abs(0.25 - 3.0 / 8)
    assert np.isnan(b[2, 3]) and np.isnan(b[3, 4]) and (b[4, 3:5] < 0).all()
    assert (levels[2:5] == 0).all()                                                           # NaN / negative: level 0
    scenes, _, _, _, rois, _ = golden_set("a")
    assert [len(s) for s in scenes] == [150, 0, 100] and (rois[150:, 0] == 2).all()          # an empty scene between
    yaw = scenes[0][:8, 6]
    h = F(np.pi / 2)
    assert yaw[0] == 0 and (yaw == -h).sum() >= 2 and rois[0, 7] == 90.0 and 0.0 in rois[:8, 7] and 180.0 in rois[:8, 7]
    assert (rois[:, 7] >= 0).all() and (rois[:, 7] <= 180.0).all()


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, hdr) and name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name
    assert int(re.search(r"#define AABR_ABI_VERSION (\d+)", hdr).group(1)) == _hip.ABI_VERSION == lib.aabr_version() == 640
    # the record's layout as the header declares it: two pointers, four int32, two int64, a float and a pad
    assert C.sizeof(_hip.AabrRoiLevel) == 56 and _hip.AabrRoiLevel.V.offset == 32 and \
        _hip.AabrRoiLevel.spatial_scale.offset == 48
    src = open(os.path.join(REPO, "automatic-as-built-reconstruction_amd", "csrc", "Makefile")).read()
    assert "roi_pool.hip" in src and "roi_shared.h" in src


def _table(n, V=5, nb=2, ext=(4, 3, 2), feats=0x1000, cm=0x2000, off=None):
    import _hip
    tab = (_hip.AabrRoiLevel * max(n, 1))()
    for i in range(n):
        t = tab[i]
        t.feats, t.cellmap = feats, cm                               # never dereferenced: every call below is refused
        t.height, t.width, t.zsize = ext
        t.nb, t.V, t.row_offset, t.spatial_scale = nb, V, (i * V if off is None else off), 0.5
    return tab


def test_argument_validation_without_gpu():
    import _hip
    lib = _hip.load()
    err = lambda: lib.aabr_last_error()                              # noqa: E731
    n2 = _hip.i64xn([3, 4])
    sc = _hip.f32xn([0.5, 0.25, 0.125, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])

    def prepare(nb, n_host, n_levels):
        return lib.aabr_roi_pool_prepare(None, nb, n_host, 1.0, n_levels, sc, 10.0, None, None, None)
    assert prepare(2, n2, 0) == -1 and b"n_levels" in err()
    assert prepare(2, n2, 9) == -1 and b"n_levels" in err()
    assert prepare(0, n2, 3) == -1 and b"nb must be" in err()
    assert prepare(17, n2, 3) == -1 and b"nb must be" in err()
    assert prepare(2, _hip.i64xn([3, -1]), 3) == -1 and b"negative" in err()
    assert prepare(2, n2, 3) == -1 and b"null" in err()              # 7 boxes, no arrays
    assert prepare(2, _hip.i64xn([0, 0]), 3) == 0                    # N == 0: nothing to launch

    def forward(tab, n_levels, batch_size=2, num_rois=4, channels=8, out=(2, 2, 2)):
        return lib.aabr_roi_pool_forward(tab, n_levels, channels, batch_size, None, None, num_rois, out[0], out[1], out[2],
                                         2, None, None)

    def backward(tab, n_levels, batch_size=2, num_rois=4, channels=8, out=(2, 2, 2), total=10):
        return lib.aabr_roi_pool_backward(tab, n_levels, channels, batch_size, None, None, num_rois, out[0], out[1],
                                          out[2], 2, None, None, total, None)
    for call in (forward, backward):
        assert call(_table(2), 0) == -1 and b"n_levels" in err()
        assert call(_table(2), 9) == -1 and b"n_levels" in err()
        assert call(_table(2, nb=0), 2) == -1 and b"nb must be" in err()
        assert call(_table(2, nb=3), 2, batch_size=2) == -1 and b"nb must be" in err()
        assert call(_table(2), 2, num_rois=-1) == -1 and b"negative" in err()
        assert call(_table(2, V=-1), 2) == -1 and b"negative V" in err()
        assert call(_table(2, ext=(4, 0, 2)), 2) == -1 and b"extent" in err()
        assert call(_table(2), 2, out=(2, 0, 2)) == -1
        assert call(_table(2, feats=None), 2) == -1 and b"null" in err()
        assert call(None, 2) == -1 and b"null" in err()
        assert call(_table(2), 2) == -1 and b"null" in err()         # a valid table, but no rois / output arrays
    assert forward(_table(2), 2, num_rois=0) == 0                    # N == 0: nothing to launch
    assert backward(_table(2), 2, total=9) == -1 and b"row_offset" in err()
    assert backward(_table(2, off=-1), 2) == -1 and b"row_offset" in err()
    assert backward(_table(2, V=0), 2, num_rois=0, total=0) == 0


class _X(object):
    """a stand-in for a SparseConvNetTensor: the refusals read nothing but `.features`"""

    def __init__(self, v, c, dtype=torch.float32):
        self.features = torch.zeros((v, c), dtype=dtype)


class _Boxes(object):
    def __init__(self, n):
        self.bbox3d = torch.zeros((n, 7))


def test_python_surface_and_refusals():
    import roi_glue
    from maskrcnn_benchmark.layers.roi_align_rotated_3d import ROIAlignRotated3D
    from maskrcnn_benchmark.modeling.poolers_3d import LevelMapper_3d, Pooler
    p = Pooler((5, 11, 4), (0.5, 0.25), 2, 8, canonical_level=None)
    assert p.fused is True and len(p.poolers) == 2 and all(isinstance(m, ROIAlignRotated3D) for m in p.poolers)
    assert [m.spatial_scale for m in p.poolers] == [0.5, 0.25] and p.poolers[0].output_size == (5, 11, 4)
    assert "ROIAlignRotated3D(output_size=(5, 11, 4), spatial_scale=0.25, sampling_ratio=2)" in repr(p)
    assert list(p.state_dict().keys()) == [] and p.box_scale == 1.0
    assert isinstance(p.map_levels, LevelMapper_3d) and p.map_levels.scales.tolist() == [0.5, 0.25]
    boxes = [torch.zeros((3, 7)), torch.zeros((2, 7))]
    two = [_X(4, 8), _X(3, 8)]
    args = ((5, 11, 4), (0.5, 0.25), 2, 8)
    with pytest.raises(ValueError):
        roi_glue.pool_rois(two + [_X(2, 8)], boxes, *args)                       # three levels, two scales
    with pytest.raises(ValueError):
        roi_glue.pool_rois([_X(4, 8), _X(3, 16)], boxes, *args)                  # channel counts differ
    with pytest.raises(ValueError):
        roi_glue.pool_rois([_X(1, 8)] * 9, boxes, (5, 11, 4), (0.5,) * 9, 2, 8)  # more than 8 levels
    with pytest.raises(ValueError):
        roi_glue.pool_rois(two, [torch.zeros((3, 6))], *args)                    # not [n, 7]
    with pytest.raises(TypeError):
        roi_glue.pool_rois([_X(4, 8), _X(3, 8, torch.bfloat16)], boxes, *args)
    with pytest.raises(TypeError):
        p(two[:1] + [_X(3, 8, torch.float64)], [_Boxes(3), _Boxes(2)])
    with pytest.raises(ValueError):
        p(two + [_X(2, 8)], [_Boxes(3)])                                         # three maps for a two-level pooler
    with pytest.raises(ValueError):
        Pooler((2, 2, 2), (0.5,) * 9, 2, 8)


@pytest.mark.parametrize("case", P.gpu_cases(), ids=[c.name for c in P.gpu_cases()])
def test_undecided_share_of_the_gpu_cases_is_small(case):
    """the fp64 yardstick alone, per level: at most 1 % of the forward outputs and of the touched backward sites undecided
    (the cap of test_roi_align_host.py::test_undecided_share_is_small); the cases hit the levels they are meant to"""
    hit = [len(idx) for idx, _, _ in case.reference()]
    assert sum(hit) == case.n
    for l, (idx, rf, rb) in enumerate(case.reference()):
        fwd = rf.undecided.mean() if rf.undecided.size else 0.0
        bwd = (rb.undecided & rb.touched).sum() / max(rb.touched.sum(), 1)
        assert fwd <= 0.01 and bwd <= 0.01, (l, fwd, bwd)
    if case.skip_level is None:
        assert min(hit) > 0, hit
    else:
        assert hit[case.skip_level] == 0 and min(h for l, h in enumerate(hit) if l != case.skip_level) > 0
    assert (case.rois[:, 0] == np.repeat(np.arange(len(case.counts)), case.counts)).all()


def test_adjoint_case_has_nothing_undecided_and_nothing_above_the_map():
    import roi_align_ref as R
    case = P.adjoint_case()
    for l, (idx, rf, rb) in enumerate(case.reference()):
        assert len(idx) > 0 and not rf.undecided.any() and not (rb.undecided & rb.touched).any()
        for roi in case.rois[idx]:
            g = R.geometry(roi, P.SCALES[l], case.out_size, case.sampling, P.EXTENTS[l], True)
            assert (g.z <= P.EXTENTS[l][2]).all()
