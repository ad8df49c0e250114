"""Device-side input pipeline: the reference dataset's host quantisation + `trainMerge` collate
(data3d/suncg_utils/suncg_dataset.py:126-188 test-time path, data3d/data.py:25-37) as one HIP
kernel per scene writing straight into the batch tensors the InputLayer consumes."""
import torch

import _hip
from _hip import ptr, stream, check


def quantize_scenes(xyz_list, extra_feats_list, voxel_scale, full_scale):
    """xyz_list: per-scene [n_i,3] float32/float64 DEVICE tensors (metres); extra_feats_list: per-scene
    [n_i, C-3] float32 (colour, normal, ...) or None.  Returns (locs int64 [sum n,4], feats float32
    [sum n, C]) in the trainMerge layout.  Points outside FULL_SCALE carry the (-1,-1,-1) sentinel
    the InputLayer skips (the reference drops them on the host)."""
    lib = _hip.load()
    dev = xyz_list[0].device
    _hip.require_gpu(xyz_list[0])
    ns = [int(x.shape[0]) for x in xyz_list]
    cx = 0 if extra_feats_list is None or extra_feats_list[0] is None else int(extra_feats_list[0].shape[1])
    C_ = 3 + cx
    tot = sum(ns)
    locs = torch.empty((tot, 4), dtype=torch.int64, device=dev)
    feats = torch.empty((tot, C_), dtype=torch.float32, device=dev)
    fs = torch.tensor([int(v) for v in full_scale], dtype=torch.int32, device=dev)
    o = 0
    for b, x in enumerate(xyz_list):
        n = ns[b]
        x = x.contiguous()
        assert x.dtype in (torch.float32, torch.float64) and x.shape[1] == 3
        amin = x.amin(0) if n else torch.zeros(3, dtype=x.dtype, device=dev)
        check(lib.aabr_quantize_points(ptr(x), int(x.dtype == torch.float64), n, float(voxel_scale), ptr(amin),
                                       ptr(fs), b, locs[o:].data_ptr() if n else None,
                                       feats[o:].data_ptr() if n else None, C_, stream()))
        if cx:
            feats[o:o + n, 3:] = extra_feats_list[b]
        o += n
    return locs, feats


def quantize_scenes_bl(xyz_list, extra_feats_list, voxel_scale, full_scale, length=None):
    """`quantize_scenes` for a PADDED batch, all scenes in one library call: returns (coords int64 [B, L, 3], feats float32
    [B, L, C]), the pair `sparseconvnet.BLInputLayer` consumes where it lies.  L is `length` or the largest scene
    (`length` below it: ValueError).  Per scene the arithmetic is quantize_scenes' exactly (a = xyz * scale - min * scale
    in double, keep 0 <= a < full_scale, trunc, feature xyz = float(a / scale)): coords[b, :n_b] are that scene's
    locs[:, :3] (a dropped point is (-1, -1, -1)), feats[b, :n_b] its feature rows (equal under ==: a -0.0 may come out as
    0.0 where the minimum is a signed zero); rows n_b .. L are -1 coordinates and zero features -- padding and dropped
    points are the same empty rows to the BLInputLayer.  The scenes' pointers and sizes travel in the kernel arguments, 32
    scenes per launch (csrc/geometry.hip k_qbl_*): one fill, one minimum launch and one quantise launch that also copies
    the extra features for B <= 32; no per-scene torch op, no host read.  The scenes share one dtype (float32 or
    float64) and one number of extra feature planes.  Inputs are finite: a NaN coordinate is out of scope (its point is
    dropped, and the scene's minimum ignores it, where torch.amin would return NaN)."""
    lib = _hip.load()
    B = len(xyz_list)
    if B == 0:
        raise ValueError("quantize_scenes_bl needs at least one scene")
    x0 = xyz_list[0]
    _hip.require_gpu(x0)
    dev = x0.device
    ns = [int(x.shape[0]) for x in xyz_list]
    extras = None if extra_feats_list is None or extra_feats_list[0] is None else extra_feats_list
    cx = 0 if extras is None else int(extras[0].shape[1])
    for b, x in enumerate(xyz_list):
        if x.dtype != x0.dtype or x.dtype not in (torch.float32, torch.float64) or x.dim() != 2 or x.shape[1] != 3:
            raise TypeError("scene %d: xyz must be [n, 3] %s like scene 0, got %s %s"
                            % (b, x0.dtype, tuple(x.shape), x.dtype))
        if extras is not None and (extras[b].dtype != torch.float32 or tuple(extras[b].shape) != (ns[b], cx)):
            raise TypeError("scene %d: extra features must be float32 [%d, %d], got %s %s"
                            % (b, ns[b], cx, tuple(extras[b].shape), extras[b].dtype))
    L = max(ns) if length is None else int(length)
    if L < max(ns):
        raise ValueError("length = %d is below the largest scene (%d points)" % (L, max(ns)))
    cont = lambda t: t if t.is_contiguous() else t.contiguous()
    xs = [cont(x) for x in xyz_list]
    es = [cont(e) for e in extras] if extras is not None else None
    coords = torch.empty((B, L, 3), dtype=torch.int64, device=dev)
    feats = torch.empty((B, L, 3 + cx), dtype=torch.float32, device=dev)
    keys = _hip.workspace("quantize_bl", 3 * B, torch.int64, dev)
    check(lib.aabr_quantize_scenes_bl(_hip.ptrs(xs), _hip.ptrs(es) if es is not None else None, _hip.i64xn(ns), B,
                                      int(x0.dtype == torch.float64), cx, float(voxel_scale),
                                      _hip.i32x3(full_scale), L, ptr(coords), ptr(feats), ptr(keys), stream()))
    return coords, feats
