"""bf16 storage of the pooled ROI tensor, without a GPU: the five new C-ABI symbols (header, binding, library, argument
counts, the argument checks that return before any HIP call), the ABI version and record size they leave alone, and the
dtype checks of roi_glue.pool_rois / dense_linear and of the two modules' `pooled_dtype` attribute."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# new symbol -> (the fp32 entry point it mirrors, arguments it has more (+) or fewer (-) than that one)
NEW_SYMBOLS = {
    "aabr_roi_pool_forward_pooled_bf16": ("aabr_roi_pool_forward", 1),             # + feats_bf16
    "aabr_roi_pool_backward_pooled_bf16": ("aabr_roi_pool_backward_bf16", 1),      # + feats_bf16
    "aabr_roi_mlp_forward_pooled_bf16": ("aabr_roi_mlp_forward", -1),              # - a_layout
    "aabr_roi_mlp_backward_input_pooled_bf16": ("aabr_roi_mlp_backward_input", -1),
    "aabr_roi_mlp_backward_weight_pooled_bf16": ("aabr_roi_mlp_backward_weight", -1),
}
E = -1
ONE = 4096                                                                       # a non-null, aligned pointer nobody follows


def _err(lib):
    return lib.aabr_last_error()


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640 and _hip.ABI_VERSION == 640 and "#define AABR_ABI_VERSION 640" in hdr
    for name, (mirror, extra) in NEW_SYMBOLS.items():
        assert name in _hip._SIGS and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name
        assert len(_hip._SIGS[name][1]) == len(_hip._SIGS[mirror][1]) + extra, name
        assert "bf16" in decl, name                                              # the bf16 operands are named as such
    assert ctypes.sizeof(_hip.AabrRoiLevel) == 56


def _levels(feats=ONE, V=4):
    import _hip
    tab = (_hip.AabrRoiLevel * 1)()
    tab[0].feats, tab[0].cellmap, tab[0].V, tab[0].nb = feats, ONE, V, 1
    tab[0].height = tab[0].width = tab[0].zsize = 2
    tab[0].spatial_scale = 1.0
    return tab


def test_pool_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()

    def pf(tab, n_levels=1, rois=ONE, lv=ONE, out=ONE, f16=0, n=3):
        return lib.aabr_roi_pool_forward_pooled_bf16(tab, n_levels, 8, 1, rois, lv, n, 2, 2, 2, 2, f16, out, None)

    def pb(tab, f16=1, g=ONE, acc=ONE, out=ONE, total=4, rois=ONE, n=3):
        return lib.aabr_roi_pool_backward_pooled_bf16(tab, 1, 8, 1, rois, ONE, n, 2, 2, 2, 2, f16, g, acc, out, total, None)

    for f16 in (0, 1):
        assert pf(None, f16=f16) == E and b"levels_desc_host" in _err(lib)
        assert pf(_levels(), rois=None, f16=f16) == E and b"rois" in _err(lib)
        assert pf(_levels(), lv=None, f16=f16) == E and b"levels" in _err(lib)
        assert pf(_levels(), out=None, f16=f16) == E and b"output_bf16" in _err(lib)
        assert pf(_levels(), out=ONE + 2, f16=f16) == E and b"output_bf16 must be 4-byte aligned" in _err(lib)
        assert pf(_levels(), n_levels=0, f16=f16) == E and b"n_levels" in _err(lib)
        assert pf(_levels(feats=None), f16=f16) == E and b"null feats" in _err(lib)
        assert pf(_levels(), n=0, rois=None, lv=None, out=None, f16=f16) == 0       # no ROIs: success, no launch
        assert lib.aabr_roi_pool_forward(_levels(), 1, 8, 1, None, None, 0, 2, 2, 2, 2, None, None) == 0   # as the fp32 form
    assert pf(_levels(feats=ONE + 2), f16=1) == E and b"feats must be 4-byte aligned" in _err(lib)
    for f16 in (0, 1):
        assert pb(None, f16=f16) == E and b"levels_desc_host" in _err(lib)
        assert pb(_levels(), f16=f16, rois=None) == E and b"rois" in _err(lib)
        assert pb(_levels(), f16=f16, g=None) == E and b"grad_output_bf16" in _err(lib)
        assert pb(_levels(), f16=f16, g=ONE + 2) == E and b"grad_output_bf16 must be 4-byte aligned" in _err(lib)
        assert pb(_levels(), f16=f16, acc=None) == E and b"accum_f32" in _err(lib)
        assert pb(_levels(), f16=f16, total=3) == E and b"row_offset" in _err(lib)  # V = 4 rows do not fit
        assert pb(_levels(V=0), f16=f16, acc=None, out=None, total=0) == 0          # nothing to do: success, no launch
    assert pb(_levels(), f16=1, out=None) == E and b"d_feats_all_bf16" in _err(lib)
    assert pb(_levels(), f16=1, out=ONE + 2) == E and b"d_feats_all_bf16 must be 4-byte aligned" in _err(lib)


def test_mlp_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()
    hw, pz, C = 6, 2, 4                                                          # M = 2 ROIs x hw rows, K = C pz

    def fw(A=ONE, W=ONE, Y=ONE, M=2 * hw, N=3, K=C * pz, hw_=hw, pz_=pz):
        return lib.aabr_roi_mlp_forward_pooled_bf16(A, hw_, pz_, W, None, 0, M, N, K, Y, None)

    def bi(dY=ONE, W=ONE, dA=ONE, M=2 * hw, N=3, K=C * pz, hw_=hw, pz_=pz):
        return lib.aabr_roi_mlp_backward_input_pooled_bf16(dY, None, W, M, N, K, hw_, pz_, dA, None)

    def bw(dY=ONE, A=ONE, dW=ONE, M=2 * hw, N=3, K=C * pz, hw_=hw, pz_=pz, perm=0):
        return lib.aabr_roi_mlp_backward_weight_pooled_bf16(dY, None, A, hw_, pz_, M, N, K, perm, dW, None, None, None)

    assert fw(A=None) == E and b"A_bf16" in _err(lib)
    assert fw(A=ONE + 2) == E and b"A_bf16 must be 4-byte aligned" in _err(lib)
    assert fw(W=None) == E and b"null W" in _err(lib)
    assert fw(Y=None) == E and b"null Y" in _err(lib)
    assert bi(dA=None) == E and b"dA_bf16" in _err(lib)
    assert bi(dA=ONE + 2) == E and b"dA_bf16 must be 4-byte aligned" in _err(lib)
    assert bi(dY=None) == E and b"null dY" in _err(lib)
    assert bi(W=None) == E and b"null W" in _err(lib)
    assert bw(A=None) == E and b"A_bf16" in _err(lib)
    assert bw(A=ONE + 2) == E and b"A_bf16 must be 4-byte aligned" in _err(lib)
    assert bw(dY=None) == E and b"null dY" in _err(lib)
    assert bw(dW=None) == E and b"null dW" in _err(lib)
    for call in (fw, bi, bw):                                                    # the shape checks of the fp32 forms
        name = {fw: b"forward_pooled_bf16", bi: b"backward_input_pooled_bf16", bw: b"backward_weight_pooled_bf16"}[call]
        assert call(pz_=3) == E and b"K = C pz" in _err(lib) and name in _err(lib)     # K = 8 is no multiple of 3
        assert call(M=2 * hw + 1) == E and b"M = n hw" in _err(lib)
        assert call(K=6, pz_=2) == E and b"multiple of 4" in _err(lib)
        assert call(hw_=0) == E and b"hw >= 1" in _err(lib)
        assert call(N=0) == E
    assert bw(perm=3) == E and b"perm_hw" in _err(lib)
    # the fp32 forms refuse the same shapes
    assert lib.aabr_roi_mlp_forward(ONE, _hip.MLP_POOLED, hw, 3, ONE, None, 0, 2 * hw, 3, C * pz, ONE, None) == E
    assert lib.aabr_roi_mlp_backward_input(ONE, None, ONE, 2 * hw + 1, 3, C * pz, _hip.MLP_POOLED, hw, pz, ONE, None) == E
    # an empty problem: success without a launch, where the fp32 form gives it (the weight gradient of M = 0 is a memset)
    assert fw(M=0, A=None, Y=None) == 0 and bi(M=0, dA=None, dY=None) == 0
    assert lib.aabr_roi_mlp_forward(None, _hip.MLP_POOLED, hw, pz, ONE, None, 0, 0, 3, C * pz, None, None) == 0
    assert lib.aabr_roi_mlp_backward_input(None, None, ONE, 0, 3, C * pz, _hip.MLP_POOLED, hw, pz, None, None) == 0


class _X(object):
    def __init__(self, V, C, dtype=torch.float32):
        self.features = torch.zeros((V, C), dtype=dtype)


def test_glue_dtype_checks_come_before_the_gpu_is_needed():
    import roi_glue
    boxes = [torch.zeros((3, 7))]
    args = ((5, 11, 4), (0.5, 0.25), 2, 8)
    for bad in (torch.float16, torch.float64, None, "bfloat16"):
        with pytest.raises(TypeError, match="pooled_dtype"):
            roi_glue.pool_rois([_X(4, 8), _X(3, 8)], boxes, *args, pooled_dtype=bad)
    for dt in (torch.float32, torch.bfloat16):                                    # the check passes for either storage
        with pytest.raises(RuntimeError, match="GPU|cuda|device"):
            roi_glue.pool_rois([_X(4, 8, dt), _X(3, 8, dt)], boxes, *args, pooled_dtype=torch.bfloat16)
    with pytest.raises(TypeError):                                               # the levels' own check is unchanged
        roi_glue.pool_rois([_X(4, 8, torch.float16)] * 2, boxes, *args, pooled_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bf16 is not part of this path"):
        roi_glue.dense_linear(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(3, 8), None, False)
    p16 = torch.zeros((2, 4, 2, 3, 2), dtype=torch.float16)
    w = torch.zeros((12, 4, 1, 1, 2))
    with pytest.raises(TypeError, match="pooled must be float32 or bfloat16"):
        roi_glue.box_head_mlp(p16, w, None, None, None, {}, torch.zeros(12, 72), None, torch.zeros(12, 12), None)
    with pytest.raises(TypeError, match="conv_w must be float32"):             # everything but `pooled` stays fp32
        roi_glue.box_head_mlp(p16.to(torch.bfloat16), w.to(torch.bfloat16), None, None, None, {}, torch.zeros(12, 72), None,
                              torch.zeros(12, 12), None)


def test_modules_carry_pooled_dtype_and_the_unfused_extractor_refuses_bf16():
    import roi_glue
    from maskrcnn_benchmark.modeling.poolers_3d import Pooler
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.roi_box_feature_extractors import make_roi_box_feature_extractor
    pooler = Pooler((2, 3, 2), (0.5, 0.25), 2, 10.0)
    assert pooler.pooled_dtype == torch.float32 and pooler.fused
    ext = make_roi_box_feature_extractor(roi_glue.box_head_cfg())
    assert ext.pooled_dtype == torch.float32 and ext.pooler.pooled_dtype == torch.float32
    ext.fused = False
    with pytest.raises(TypeError, match="float32"):
        ext.head(torch.zeros((2, 8, 2, 3, 2), dtype=torch.bfloat16))
    pooler.pooled_dtype = torch.float16
    with pytest.raises(TypeError, match="pooled_dtype"):
        pooler([_X(4, 8), _X(3, 8)], [])
