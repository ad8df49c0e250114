"""Merging walls by their corners without a GPU.

  * tests/merge_corners_ref.py (the numpy fp32 restatement of the definition in include/aabr_hip.h) against
    tests/golden/merge_corners_golden.npz: the REFERENCE's own merge_walls_by_corners run on the CPU by
    tests/golden/gen_merge_corners_golden.py.  Set A (groups of at most 4 corners, walls along the axes): bit-equal.  Set B
    (groups of 5 to 8, any yaw): the same S at every step and the same merged flags, and every value within the bound
    derived below.
  * csrc/merge_corners.h compiled for the host (tests/merge_corners_host_harness.cpp) -- the statements the HIP kernel
    runs -- against the restatement: bit-equal on both sets, on the hand-built scenes of tests/merge_corners_host.py and on
    a scene at the built limit.
  * argument errors of the glue and of the C entry raise before any device call.

THE BOUND OF SET B.  u = 2^-24.  Two fp32 evaluations are compared (the restatement and the reference), which differ in
  (a) yx_zb -> two corners: fp64 sin / cos here, fp32 in the reference.  corner_box_ref.corner_bounds gives each side's
      bound E_xy (the reference's with its TRIG term) and E_z; a corner coordinate differs by at most their sum;
  (b) the summation order of a mean over more than 4 rows and of the scene's z0 mean over W walls.
Propagation, per axis, with e[k] the bound on corner k's coordinate difference:
  top corners     p + off / |off| * th / 2 with off = cen - p, |off| = L / 2: the pulled-in point moves with the end point
                  (e), its direction turns by at most 2 |d off| / |off| <= 4 sqrt(3) e / L, times th / 2; each side rounds
                  cen, off, the norm (3 u relative), the quotient, two products and the sum: <= u (2 |p| + 8 th / 2) each.
                  e_top = e (1 + 2 sqrt(3) th / L) + 2 u (2 |p| + 4 th)
  a merging step  the mean of values that differ by at most max e[S] differs by at most that; each side's own sum of n
                  terms and its division are off by at most n u sum|x| (the bound the issue of this feature states:
                  (n - 1) u sum|x| / n for the sum in any order, u |mean| for the division, rounded up):
                  e[S] <- max e[S] + 2 n u sum|x[S]|.  The steps and their S are the restatement's, equal to the
                  reference's (asserted first).
  epilogue        cen, off = p - cen (|d off| <= 2 max(e0, e1) per axis), q = p + off / |off| * th / 2 with |off| = L' / 2:
                  e_q = e + 4 sqrt(3) max(e0, e1) th / L' + 2 u (2 |p| + 4 th), L' the rebuilt length;
                  z1 = (q0z + q1z) / 2: max e_qz + 2 u |z1|; z0 mean: 2 W u sum|z0| (the walls' z0 themselves are the
                  same fp32 operations on both sides, up to E_z);
  corners_to_yxzb corner_box_ref.from_corner_bounds(c, e_xy, e_z) is the bound of ONE fp32 evaluation on corners that
                  carry e_xy / e_z; the other side's own rounding is from_corner_bounds(c, ref=True).  Yaw modulo pi.
None of these figures is taken from what the code gives."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import corner_box_ref as CR
import merge_corners_host as H
import merge_corners_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
U = 2.0 ** -24
SQ3 = np.sqrt(3.0)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "merge_corners_golden.npz")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return H.Host(H.build_harness(tmp_path_factory.mktemp("merge_host")))


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement on every scene of the fixture, once: key -> (out, merged, trace)"""
    res = {}
    for name in "ab":
        for si in range(int(golden[name + "_scenes"])):
            key = "%s%d_" % (name, si)
            tr = {}
            out, merged = R.merge_scene(golden[key + "in"], None, float(golden["threshold"]), trace=tr)
            res[key] = (out, merged, tr)
    return res


def _steps_of(golden, key):
    lens = golden[key + "step_len"].tolist()
    ids, o = golden[key + "step_ids"], 0
    out = []
    for n in lens:
        out.append(ids[o:o + n].tolist())
        o += n
    return out


def test_fixture_holds_what_the_tests_rely_on(golden):
    assert float(golden["threshold"]) == 0.1
    sizes = {n: set() for n in "ab"}
    for name in "ab":
        assert int(golden[name + "_scenes"]) >= 2
        for si in range(int(golden[name + "_scenes"])):
            key = "%s%d_" % (name, si)
            W = len(golden[key + "in"])
            assert golden[key + "out"].shape == (W, 7) and golden[key + "merged"].shape == (W, 2)
            assert len(golden[key + "step_len"]) == 2 * W
            sizes[name] |= {n for n in golden[key + "step_len"].tolist() if n > 1}
            assert (golden[key + "out"][:, 4] > 0.5).all()                       # no wall collapsed
    assert max(sizes["a"]) <= 4 and {2, 3, 4} <= sizes["a"] and {5, 6, 7, 8} <= sizes["b"]


def test_restatement_is_bit_equal_to_the_reference_on_set_a(golden, restated):
    for si in range(int(golden["a_scenes"])):
        key = "a%d_" % si
        out, merged, tr = restated[key]
        assert R.same_bits(out, golden[key + "out"]), key
        assert (merged == golden[key + "merged"]).all(), key
        if len(out) > 1:                                                         # (W = 1 runs no step here)
            assert [s.tolist() for s, _ in tr["steps"]] == _steps_of(golden, key), key
            assert tr["margin"] > 1e-4


def _set_b_bound(walls, tr, out):
    """[W, 7] bound on |restatement - reference| per element, by the derivation of the module docstring"""
    W = len(walls)
    exy = CR.corner_bounds(walls)[0] + CR.corner_bounds(walls, ref=True)[0]
    ez = CR.corner_bounds(walls)[1] + CR.corner_bounds(walls, ref=True)[1]
    th, L = np.abs(walls[:, 3]).astype(np.float64), np.abs(walls[:, 4]).astype(np.float64)
    p0 = np.abs(tr["corners0"].astype(np.float64))                                # [2W, 3]
    e = np.empty((2 * W, 3))
    for k in range(2 * W):
        w = k >> 1
        e[k, :2] = exy[w] * (1 + 2 * SQ3 * th[w] / L[w]) + 2 * U * (2 * p0[k, :2] + 4 * th[w])
        e[k, 2] = ez[w] * (1 + 2 * SQ3 * th[w] / L[w]) + 2 * U * (2 * p0[k, 2] + 4 * th[w])
    # replay the steps on the restatement's corners to know sum|x| of every mean
    x = tr["corners0"].astype(np.float64).copy()
    xf = [np.ascontiguousarray(tr["corners0"][:, d]).copy() for d in range(3)]
    for i, (ids, did) in enumerate(tr["steps"]):
        ids2, did2, _ = R.step(xf[0], xf[1], xf[2], i, 0.1)
        assert ids2.tolist() == ids.tolist() and did2 == did
        if did:
            n = len(ids)
            for d in range(3):
                e[ids, d] = e[ids, d].max() + 2 * n * U * np.abs(x[ids, d]).sum()
            x[ids] = np.stack([v[ids] for v in xf], 1)
    assert all((xf[d] == tr["corners1"][:, d]).all() for d in range(3))
    c1 = np.abs(tr["corners1"].astype(np.float64))
    rows = np.array([R.to_2corners(b) for b in walls], np.float64)
    z0_err = ez.max() + 2 * W * U * np.abs(rows[:, 4]).sum()
    bound = np.empty((W, 7))
    for w in range(W):
        Lr = float(out[w, 4])
        em = np.maximum(e[2 * w], e[2 * w + 1])
        eq = [e[2 * w + k] + 4 * SQ3 * em * th[w] / Lr + 2 * U * (2 * c1[2 * w + k] + 4 * th[w]) for k in range(2)]
        e_xy = max(eq[0][:2].max(), eq[1][:2].max())
        e_z1 = max(eq[0][2], eq[1][2]) + 2 * U * (c1[2 * w, 2] + th[w])
        c = CR.to_2corners(out[w:w + 1])                                         # the rebuilt wall's two-corner row
        bound[w] = (CR.from_corner_bounds(c, e_xy, max(e_z1, z0_err)) + CR.from_corner_bounds(c, ref=True))[0]
    return bound


def test_set_b_same_decisions_and_values_within_the_derived_bound(golden, restated):
    for si in range(int(golden["b_scenes"])):
        key = "b%d_" % si
        out, merged, tr = restated[key]
        assert [s.tolist() for s, _ in tr["steps"]] == _steps_of(golden, key), key   # the same S at every step
        assert (merged == golden[key + "merged"]).all(), key
        assert tr["margin"] > 1e-4
        bound = _set_b_bound(golden[key + "in"], tr, out)
        diff = CR.diff_rows(out, golden[key + "out"])
        print("%s worst |diff| per column %s\n   worst diff / bound per column %s" % (key, diff.max(0), (diff / np.maximum(bound, 1e-300)).max(0)))
        bad = np.argwhere(diff > bound)
        assert bad.size == 0, "%s: %d elements beyond their bound, first %s: %g > %g" % (
            key, len(bad), bad[0], diff[tuple(bad[0])], bound[tuple(bad[0])])
        assert (out[:, 3] == golden[key + "in"][:, 3]).all()                      # the thickness is a copy


def _same(a, b):
    """equal bits, or NaN on both sides (the sign of a NaN that 0 / 0 produces is the machine's)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_harness_is_bit_equal_to_the_restatement(golden, restated, host):
    for key, (out, merged, tr) in restated.items():
        h_out, h_merged, h_steps = host.merge_scene(golden[key + "in"], None, 0.1)
        assert R.same_bits(h_out, out) and (h_merged == merged).all(), key
        assert h_steps.tolist() == [len(s) if did else 0 for s, did in tr["steps"]], key
    for name, (boxes, labels) in H.hand_built_scenes().items():
        tr = {}
        out, merged = R.merge_scene(boxes, labels, 0.1, trace=tr)
        assert tr["margin"] >= 1e-3, name                                         # a condition on the inputs
        h_out, h_merged, h_steps = host.merge_scene(boxes, labels, 0.1)
        assert _same(h_out, out) and (h_merged == merged).all(), name
        assert h_steps.tolist() == [len(s) if did else 0 for s, did in tr["steps"]], name
        sel = labels == 1
        assert R.same_bits(out[~sel], boxes[~sel]) and not merged[~sel].any(), name   # other rows: the input's bits
        if sel.any():
            assert (out[sel, 2] == out[sel, 2][0]).all(), name                    # one z0 for every wall of the scene


def test_hand_built_scenes_test_what_they_are_named_for():
    S = H.hand_built_scenes()

    def run(name, **kw):
        tr = {}
        out, merged = R.merge_scene(S[name][0], S[name][1], 0.1, trace=tr, **kw)
        return out, merged, tr

    for name, size in (("L", 2), ("T", 3), ("cross", 4), ("six", 6)):
        _, merged, tr = run(name)
        assert max(len(s) for s, did in tr["steps"] if did) == size and merged.sum() == size, name
    # the skip: five steps meet more than one corner, each meets a whole other wall, nothing moves, no flag
    _, merged, tr = run("skip")
    big = [(s, did) for s, did in tr["steps"] if len(s) > 1]
    assert len(big) == 5 and not any(did for _, did in big) and not merged.any()
    assert R.same_bits(tr["corners0"], tr["corners1"])
    # the chain: on the corners as they were before the loop, the step at b would meet a, b AND c; sequentially the
    # step at a has moved b out of c's reach, and the results differ
    out, merged, tr = run("chain")
    c0 = tr["corners0"]
    x, y, z = (np.ascontiguousarray(c0[:, d]).copy() for d in range(3))
    frozen = [R.step(x.copy(), y.copy(), z.copy(), i, 0.1)[0].tolist() for i in range(len(c0))]
    sequential = [s.tolist() for s, _ in tr["steps"]]
    assert max(len(s) for s in frozen) == 3 and max(len(s) for s in sequential) == 2
    assert frozen != sequential and merged.sum() == 2
    a, b, c = sorted(np.argsort(np.abs(c0[:, 1]) + np.abs(c0[:, 0]))[:3], key=lambda k: c0[k, 0])
    d = lambda p, q, arr: float(np.linalg.norm(arr[p].astype(np.float64) - arr[q]))
    assert d(a, b, c0) < 0.099 and d(b, c, c0) < 0.099 and d(a, c, c0) > 0.101
    assert d(b, c, tr["corners1"]) > 0.101 and d(a, b, tr["corners1"]) == 0.0
    # interleaved: walls and other rows alternate irregularly
    lab = S["interleaved"][1]
    assert (lab == 1).sum() == 12 and len(set(np.diff(np.nonzero(lab == 1)[0]).tolist())) > 1
    assert (S["300 walls"][1] == 1).sum() == 300


def test_limit_scene_and_one_over(host):
    boxes, labels = H.limit_scene(host.max_walls)
    assert host.max_walls >= 2048 and len(boxes) == host.max_walls
    tr = {}
    out, merged = R.merge_scene(boxes, labels, 0.1, trace=tr)
    assert tr["margin"] >= 1e-3
    h_out, h_merged, _ = host.merge_scene(boxes, labels, 0.1)
    assert R.same_bits(h_out, out) and (h_merged == merged).all() and merged.sum() > host.max_walls
    with pytest.raises(ValueError, match=str(host.max_walls)):
        host.merge_scene(np.concatenate([boxes, boxes[:1]]), None, 0.1)


def test_collapsed_wall_gives_the_ieee_result(host):
    """two walls whose four corners all meet: each wall's corners are NOT merged with each other (the partner is left
    out, and the other wall is whole: a skip) -- so the collapse is built directly: a wall of zero length"""
    b = np.array([[1, 2, 0, 0.08, 0.0, 2.5, 0.0], [5, 5, 0, 0.08, 3.0, 2.5, 0.0]], np.float32)
    out, _ = R.merge_scene(b, None, 0.1)
    h_out, _, _ = host.merge_scene(b, None, 0.1)
    assert np.isnan(out[0]).any() and np.isfinite(out[1]).all() and _same(h_out, out)


def test_header_binding_and_library_agree():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    for name in ("aabr_merge_walls_by_corners", "aabr_merge_corners_max_walls"):
        assert name in _hip._SIGS and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert (0 if decl.strip() == "void" else decl.count(",") + 1) == len(_hip._SIGS[name][1]), name
    assert lib.aabr_merge_corners_max_walls() >= 2048
    mk = open(os.path.join(REPO, "automatic-as-built-reconstruction_amd", "csrc", "Makefile")).read()
    assert "merge_corners.hip" in mk and "merge_corners.h " in mk


def test_c_entry_refuses_before_any_launch():
    import _hip
    lib = _hip.load()
    f, one, E = lib.aabr_merge_walls_by_corners, 4096, -1                         # `one`: a pointer nobody follows
    limit = lib.aabr_merge_corners_max_walls()
    assert f(None, None, 0, None, 0, 0, 1, 0.1, None, None, None) == 0           # no scene: nothing to do
    assert f(one, None, -1, one, 1, 0, 1, 0.1, one + 64, None, None) == E
    assert f(one, None, 5, one, 1, 6, 1, 0.1, one + 64, None, None) == E         # max_scene_rows > rows
    assert f(one, None, 5, None, 1, 5, 1, 0.1, one + 64, None, None) == E and b"null" in lib.aabr_last_error()
    assert f(None, None, 5, one, 1, 5, 1, 0.1, one + 64, None, None) == E
    assert f(one, None, 5, one, 1, 5, 1, 0.1, one, None, None) == E and b"boxes_out" in lib.aabr_last_error()
    assert f(one, None, 5, one, 0, 5, 1, 0.1, one + 64, None, None) == E         # rows without a scene
    assert f(one, None, limit + 1, one, 1, limit + 1, 1, 0.1, one + 64, None, None) == E
    assert str(limit).encode() in lib.aabr_last_error()                          # the message names the limit


class _List(object):
    def __init__(self, bbox3d, labels=None, mode="yx_zb"):
        self.bbox3d, self.mode, self._labels = bbox3d, mode, labels

    def get_field(self, name):
        assert name == "labels"
        return self._labels


def test_glue_argument_errors_raise_before_any_device_call():
    import roi_glue
    from maskrcnn_benchmark.structures.bounding_box_3d import merge_by_corners, merge_walls_by_corners
    limit = roi_glue.merge_corners_max_walls()
    assert limit >= 2048
    b = torch.zeros(3, 7)
    with pytest.raises(ValueError, match="label lists"):
        roi_glue.merge_by_corners([b, b], [torch.ones(3)])
    with pytest.raises(ValueError, match="3 boxes and 2 labels"):
        roi_glue.merge_by_corners([b], [torch.ones(2)])
    with pytest.raises(ValueError, match=r"\[n, 7\]"):
        roi_glue.merge_by_corners([torch.zeros(3, 6)])
    with pytest.raises(ValueError, match="at most %d walls" % limit):
        roi_glue.merge_by_corners([b, torch.zeros(limit + 1, 7)])
    assert roi_glue.merge_by_corners([]) == [] and roi_glue.merge_by_corners([], [], return_merged=True) == ([], [])
    for fn in (merge_by_corners, merge_walls_by_corners):
        with pytest.raises(ValueError, match="standard"):
            fn(_List(b, torch.ones(3), mode="standard"))
        with pytest.raises(ValueError, match="standard"):
            fn([_List(b, torch.ones(3)), _List(b, torch.ones(3), mode="standard")])
    with pytest.raises(ValueError, match="at most %d walls" % limit):
        merge_walls_by_corners(_List(torch.zeros(limit + 1, 7)))


def test_post_processor_option_and_config_key():
    import roi_glue
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import PostProcessor, make_roi_box_post_processor
    assert PostProcessor().merge_by_corner is False and PostProcessor(merge_by_corner=True).merge_by_corner is True
    cfg = roi_glue.box_head_cfg()
    assert make_roi_box_post_processor(cfg).merge_by_corner is False              # the key is optional
    cfg.MODEL.ROI_HEADS.MERGE_BY_CORNER = True
    assert make_roi_box_post_processor(cfg).merge_by_corner is True


def test_harness_stand_alone_under_host_sanitizers(tmp_path):
    """the same header as a stand-alone program with AddressSanitizer and UBSan, on the host: a grid of rooms, a scene at
    the limit, one beyond it"""
    exe = str(tmp_path / "merge_harness_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-DMERGE_HARNESS_MAIN", "-o", exe,
                           os.path.join(HERE, "merge_corners_host_harness.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    assert b"walls 2048" in r.stdout and b"walls -1" in r.stdout
