"""Both rotated 3-D ROI-align kernels of csrc/roi.hip against the fp64 yardstick tests/roi_align_ref.py.

Every case of roi_align_ref.gpu_cases() (what each is for is said there, next to its construction) runs
  * the dense kernel, `_C.roi_align_rotated_3d_forward / _backward` on the dense tensor,
  * the fused gather through the C entry points aabr_roi_cellmap / aabr_roi_align_rotated_3d_sparse_forward / _backward,
  * the fused gather through the module ROIAlignRotated3D (fused = True, its default), forward and autograd backward,
and each result must lie within the reference's derived slack on every decided output; the undecided share is held to
the same 1 % cap as on the host (0 for the hand-placed boundary case).  tests/test_roi_align_host.py shows that the
slack is wide enough for the kernel's arithmetic and narrow enough to reject a changed convention.  Each test prints the
largest |device - fp64| / slack it saw.  Nothing outside the repository is read; no input is NaN or infinite."""
import numpy as np
import pytest
import torch

import roi_align_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
CASES = R.gpu_cases()


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _sparse(case):
    """the case's sites and features as a SparseConvNetTensor; returns (tensor, sites [V, 4] int32 in the device's row
    order, features [V, C] in that order)"""
    import sparseconvnet as scn
    B, C, H, W, Z = case.shape
    x = scn.InputLayer(3, [H + 3, W + 2, Z + 1], mode=4)([_t(case.sites.astype(np.int64)), _t(case.feats)])
    key = tuple(int(v) for v in x.spatial_size.tolist())
    grid = x.metadata.grids[key]
    sites = grid.coords.cpu().numpy().astype(np.int32)
    feats = x.features.detach().cpu().numpy()
    # the input layer only renumbers rows: same set of sites, same feature row at each
    order = np.lexsort(case.sites.T[::-1])
    order_dev = np.lexsort(sites.T[::-1])
    assert (case.sites[order] == sites[order_dev]).all() and (case.feats[order] == feats[order_dev]).all()
    return x, sites, feats


def _dense(case, sites, feats):
    B, C, H, W, Z = case.shape
    d = np.zeros(case.shape, F)
    d[sites[:, 3], :, sites[:, 0], sites[:, 1], sites[:, 2]] = feats
    return d


def _at_sites(a, sites):
    """[B, C, H, W, Z] (or [B, H, W, Z]) -> rows [V, C] (or [V]) at the sites"""
    if a.ndim == 5:
        return a[sites[:, 3], :, sites[:, 0], sites[:, 1], sites[:, 2]]
    return a[sites[:, 3], sites[:, 0], sites[:, 1], sites[:, 2]]


class _SiteResult(object):
    """a backward Result restricted to the active sites (what the fused form returns)"""

    def __init__(self, ref, sites):
        self.values, self.slack = _at_sites(ref.values, sites), _at_sites(ref.slack, sites)
        self.undecided = np.broadcast_to(_at_sites(ref.undecided, sites)[:, None], self.values.shape)


def _check(name, what, got, ref, exact_case):
    worst, und, bad = R.compare(got, ref)
    print("%s %s: max |device - fp64| / slack = %.4g (undecided share %.5f)" % (name, what, worst, und))
    assert bad == 0, (name, what, worst)
    return worst


def _cellmap(sites_dev, V, ext, B):
    import _hip
    from _hip import ptr, stream, check
    cm = torch.empty((B,) + tuple(ext), dtype=torch.int32, device=DEV)
    check(_hip.load().aabr_roi_cellmap(ptr(sites_dev), V, _hip.i32x3(ext), B, ptr(cm), stream()))
    return cm


def _run_all(case):
    """-> dict of the three paths' forward / backward results as numpy, and the reference's Results"""
    import _hip
    from _hip import ptr, stream, check
    from maskrcnn_benchmark.layers import _C
    from maskrcnn_benchmark.layers.roi_align_rotated_3d import ROIAlignRotated3D
    import sparseconvnet as scn
    B, C, H, W, Z = case.shape
    PH, PW, PZ = case.out_size
    x, sites, feats = _sparse(case)
    dense = _dense(case, sites, feats)
    rois, grad = case.rois, case.grad()
    n = len(rois)
    ref_f = R.forward(dense, rois, case.scale, case.out_size, case.sampling)
    ref_b = R.backward(grad, rois, case.scale, case.out_size, case.shape, case.sampling)
    fwd_und = ref_f.undecided.mean() if ref_f.undecided.size else 0.0
    bwd_und = (ref_b.undecided & ref_b.touched).sum() / max(ref_b.touched.sum(), 1)
    cap = 0.0 if case.exact else 0.01
    assert fwd_und <= cap and bwd_und <= cap, (fwd_und, bwd_und)
    res = {}
    rois_d, grad_d = _t(rois), _t(grad)
    # dense kernel
    res["dense_fwd"] = _C.roi_align_rotated_3d_forward(_t(dense), rois_d, case.scale, PH, PW, PZ, case.sampling)
    res["dense_bwd"] = _C.roi_align_rotated_3d_backward(grad_d, rois_d, case.scale, PH, PW, PZ, B, C, H, W, Z,
                                                        case.sampling)
    # fused gather, C entry points
    V = sites.shape[0]
    sites_d, feats_d = _t(sites), _t(feats)
    cm = _cellmap(sites_d, V, (H, W, Z), B)
    out = torch.full((n, C, PH, PW, PZ), 7.0, dtype=torch.float32, device=DEV)
    lib = _hip.load()
    check(lib.aabr_roi_align_rotated_3d_sparse_forward(ptr(feats_d), C, ptr(cm), B, H, W, Z, ptr(rois_d), n,
                                                       float(case.scale), PH, PW, PZ, int(case.sampling), ptr(out),
                                                       stream()))
    d_feats = torch.full((V, C), 7.0, dtype=torch.float32, device=DEV)
    check(lib.aabr_roi_align_rotated_3d_sparse_backward(ptr(grad_d), C, ptr(cm), B, H, W, Z, ptr(rois_d), n,
                                                        float(case.scale), PH, PW, PZ, int(case.sampling), V,
                                                        ptr(d_feats), stream()))
    res["cabi_fwd"], res["cabi_bwd"] = out, d_feats
    # fused gather, the module
    f = _t(feats).requires_grad_(True)
    layer = ROIAlignRotated3D(case.out_size, case.scale, case.sampling)
    assert layer.fused
    mo = layer(scn.SparseConvNetTensor(f, x.metadata, x.spatial_size), rois_d)
    assert tuple(mo.shape) == (n, C, PH, PW, PZ)
    if n:
        mo.backward(grad_d)
        res["module_bwd"] = f.grad
    res["module_fwd"] = mo.detach()
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in res.items()}
    return res, ref_f, ref_b, sites, dense, grad


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_both_kernels_within_the_slack(case):
    res, ref_f, ref_b, sites, _, _ = _run_all(case)
    site_b = _SiteResult(ref_b, sites)
    worst = {}
    for path in ("dense", "cabi", "module"):
        worst[path + "_fwd"] = _check(case.name, path + " forward", res[path + "_fwd"], ref_f, case.exact)
        if path + "_bwd" in res:
            worst[path + "_bwd"] = _check(case.name, path + " backward", res[path + "_bwd"],
                                          ref_b if path == "dense" else site_b, case.exact)
    # the fused forward runs the dense kernel's statements: bit-identical
    assert (res["cabi_fwd"] == res["dense_fwd"]).all() and (res["module_fwd"] == res["dense_fwd"]).all()
    print("RATIO %s forward %.4g backward %.4g" % (case.name, max(v for k, v in worst.items() if k.endswith("fwd")),
                                                   max([v for k, v in worst.items() if k.endswith("bwd")] + [0.0])))


def test_adjoint_identity_on_device_outputs():
    """<g, F(x)> = <B(g), x> with F(x) and B(g) from the device, accumulated on the host in fp64, within the sum of the
    two slacks.  No sample lies above the map (there the forward pass reads the last slice and the backward pass adds
    nothing, so the pair is not adjoint by definition) and nothing is undecided."""
    H, W, Z = 14, 11, 8

    def rois(rng):
        r = R.random_rois(rng, 24, 2, H, W, Z, 1.0, zsize=(0.5, 2.0))
        r[:, 3] = rng.uniform(1.5, Z - 2.5, len(r))
        return r
    case = R._case("adjoint", 130, 2, 9, H, W, Z, rois, 1.0, (3, 2, 2), 2, occupancy=0.3)
    res, ref_f, ref_b, sites, dense, grad = _run_all(case)
    assert not ref_f.undecided.any() and not (ref_b.undecided & ref_b.touched).any()
    g64, x64 = grad.astype(np.float64), dense.astype(np.float64)
    bound = (np.abs(g64) * ref_f.slack).sum() + (ref_b.slack * np.abs(x64)).sum()
    lhs = (g64 * res["dense_fwd"]).sum()
    rhs = (res["dense_bwd"].astype(np.float64) * x64).sum()
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    feats = _at_sites(dense, sites).astype(np.float64)
    lhs2 = (g64 * res["module_fwd"]).sum()
    rhs2 = (res["module_bwd"].astype(np.float64) * feats).sum()
    assert abs(lhs2 - rhs2) <= bound, (lhs2, rhs2, bound)
    print("adjoint: dense |diff| / bound %.4g, fused %.4g" % (abs(lhs - rhs) / bound, abs(lhs2 - rhs2) / bound))


def test_cellmap_exact_against_numpy():
    """aabr_roi_cellmap: site row or -1 per cell; sites outside the given extent (in any coordinate or in the batch
    index) are left out by its guard; V = 0 gives all -1; map + features reproduce the dense tensor exactly"""
    rng = np.random.default_rng(140)
    B, H, W, Z, C = 3, 9, 7, 4, 5
    sites = R.make_sites(rng, B, H, W, Z, 0.3)
    V = len(sites)
    feats = rng.standard_normal((V, C)).astype(F)
    for ext, nb in (((H, W, Z), B), ((H - 3, W, Z), B), ((H, W - 2, Z - 1), B), ((H, W, Z), B - 1)):
        cm = _cellmap(_t(sites), V, ext, nb).cpu().numpy()
        want = np.full((nb,) + ext, -1, np.int32)
        inside = (sites[:, 0] < ext[0]) & (sites[:, 1] < ext[1]) & (sites[:, 2] < ext[2]) & (sites[:, 3] < nb)
        assert 0 < inside.sum() and (inside.sum() < V or (ext == (H, W, Z) and nb == B))
        s = sites[inside]
        want[s[:, 3], s[:, 0], s[:, 1], s[:, 2]] = np.nonzero(inside)[0]
        assert (cm == want).all()
        if inside.all():
            dense = np.zeros((B, C, H, W, Z), F)
            dense[sites[:, 3], :, sites[:, 0], sites[:, 1], sites[:, 2]] = feats
            rebuilt = np.where(cm[:, None] >= 0, feats[np.maximum(cm, 0)].transpose(0, 4, 1, 2, 3), 0).astype(F)
            assert (rebuilt == dense).all()
    empty = _cellmap(None, 0, (H, W, Z), B).cpu().numpy()
    assert (empty == -1).all()


def test_module_reuses_its_cached_extent_and_cellmap():
    from maskrcnn_benchmark.layers.roi_align_rotated_3d import ROIAlignRotated3D
    import sparseconvnet as scn
    case = next(c for c in CASES if c.name == "batch3_thin_middle")
    x, sites, feats = _sparse(case)
    layer = ROIAlignRotated3D(case.out_size, case.scale, case.sampling)
    xin = scn.SparseConvNetTensor(_t(feats), x.metadata, x.spatial_size)
    a = layer(xin, _t(case.rois))
    key = tuple(int(v) for v in x.spatial_size.tolist())
    cm, ext = x.metadata._roi_cellmap[key], x.metadata._roi_extent[key]
    assert tuple(ext) == case.shape[2:] + (case.shape[0],) and tuple(cm.shape) == (case.shape[0],) + case.shape[2:]
    b = ROIAlignRotated3D(case.out_size, case.scale, case.sampling)(xin, _t(case.rois))
    assert x.metadata._roi_cellmap[key] is cm and x.metadata._roi_extent[key] is ext
    assert torch.equal(a, b)


def test_batch_index_outside_the_input_is_an_empty_sample_on_both_paths():
    """Q6 of roi_align_ref: ROIs naming sample B (a trailing sample without sites, cropped away by the module) and
    sample -1, among valid ones: zeros forward, nothing backward, the other ROIs unaffected -- the dense kernel
    (guarded by the batch size it is now told) and the fused one alike"""
    case = R.batch_index_case()
    res, ref_f, ref_b, sites, _, _ = _run_all(case)
    outside = (case.rois[:, 0] < 0) | (case.rois[:, 0] >= case.shape[0])
    assert outside.sum() == 3
    site_b = _SiteResult(ref_b, sites)
    for path in ("dense", "cabi", "module"):
        assert not res[path + "_fwd"][outside].any(), path
        _check(case.name, path + " forward", res[path + "_fwd"], ref_f, False)
        _check(case.name, path + " backward", res[path + "_bwd"], ref_b if path == "dense" else site_b, False)
