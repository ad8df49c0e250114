"""bf16 feature storage into the heads, without a GPU: the eight new C-ABI symbols (header, binding, library, the
argument checks that return before any HIP call), the ABI version and record sizes they leave alone, the explicit
`feature_dtype` keyword of rpn_glue.rpn_head / rpn_head_grouped, the pooler's dtype check, and FPN_Net.cast_outputs."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aabr_rpn_head_forward_bf16", "aabr_rpn_head_backward_bf16", "aabr_rpn_head_grouped_forward_bf16",
               "aabr_rpn_head_grouped_backward_bf16", "aabr_roi_pool_forward_bf16", "aabr_roi_pool_backward_bf16",
               "aabr_roi_align_rotated_3d_sparse_forward_bf16", "aabr_roi_align_rotated_3d_sparse_backward_bf16")
E = -1
ONE = 4096                                                                       # a non-null, aligned pointer nobody follows


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640 and _hip.ABI_VERSION == 640 and "#define AABR_ABI_VERSION 640" in hdr
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name
        # each mirrors the fp32 entry point of the same name; the two backward forms of the ROI kernels take the fp32
        # accumulation buffer as one more argument
        extra = 1 if name in ("aabr_roi_pool_backward_bf16", "aabr_roi_align_rotated_3d_sparse_backward_bf16") else 0
        assert len(_hip._SIGS[name][1]) == len(_hip._SIGS[name[:-len("_bf16")]][1]) + extra, name
    assert ctypes.sizeof(_hip.AabrRpnMap) == 40 and ctypes.sizeof(_hip.AabrRoiLevel) == 56
    for rec in ("AabrRpnMap", "AabrRoiLevel"):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (rec, rec), hdr, re.S).group(1)
        assert "bf16" in fields or "bf16" in hdr[:hdr.index("typedef struct %s {" % rec)][-400:], rec


def _table(rows, f=ONE, o=ONE, r=ONE, d=ONE):
    import _hip
    tab = (_hip.AabrRpnMap * len(rows))()
    for i, n in enumerate(rows):
        tab[i].features, tab[i].rows, tab[i].objectness, tab[i].box_regression, tab[i].d_features = f, n, o, r, d
    return tab


def test_rpn_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()
    fwd = lambda tab, n, C, A, w=ONE: lib.aabr_rpn_head_forward_bf16(tab, n, C, A, w, ONE, ONE, ONE, ONE, ONE, None, None)
    bwd = lambda tab, n, C, A, h=ONE, s=ONE: lib.aabr_rpn_head_backward_bf16(tab, n, C, A, ONE, ONE, ONE, h, ONE, ONE, ONE,
                                                                            ONE, ONE, ONE, s, None)
    gfwd = lambda tab, n, C, A, G: lib.aabr_rpn_head_grouped_forward_bf16(tab, n, C, A, G, ONE, ONE, ONE, ONE, ONE, ONE,
                                                                          None, None)
    gbwd = lambda tab, n, C, A, G: lib.aabr_rpn_head_grouped_backward_bf16(tab, n, C, A, G, ONE, ONE, ONE, ONE, ONE, ONE,
                                                                           ONE, ONE, ONE, ONE, ONE, None)
    assert fwd(_table([5]), 0, 32, 2) == E and b"n_maps" in lib.aabr_last_error()
    assert fwd(_table([5]), 1, 48, 2) == E and b"C must be" in lib.aabr_last_error()
    assert fwd(_table([5]), 1, 32, 5) == E and b"A must be" in lib.aabr_last_error()
    assert fwd(_table([5], f=None), 1, 32, 2) == E and b"null" in lib.aabr_last_error()
    assert fwd(_table([5]), 1, 32, 2, w=None) == E
    # two bf16 travel per lane: rows on a 2-byte boundary are refused
    assert fwd(_table([5], f=ONE + 2), 1, 32, 2) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert bwd(_table([5], d=ONE + 2), 1, 32, 2) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert bwd(_table([5], f=ONE + 2), 1, 32, 2) == E
    assert lib.aabr_rpn_head_forward(_table([5], f=ONE + 2), 1, 32, 2, ONE, ONE, ONE, ONE, ONE, ONE, None, None) == E
    assert fwd(_table([0, 0], f=None, o=None, r=None), 2, 32, 2) == 0            # every map empty: success, no launch
    assert bwd(_table([5], d=None), 1, 32, 2) == E and b"d_features" in lib.aabr_last_error()
    assert bwd(_table([5]), 1, 32, 2, h=None) == E and b"hidden" in lib.aabr_last_error()
    assert bwd(_table([5]), 1, 32, 2, s=None) == E and b"scratch" in lib.aabr_last_error()
    assert gfwd(_table([5]), 1, 32, 2, 1) == E and b"groups" in lib.aabr_last_error()
    assert gfwd(_table([5]), 1, 32, 4, 5) == E
    assert gbwd(_table([5]), 1, 32, 2, 9) == E and b"groups" in lib.aabr_last_error()
    assert gfwd(_table([5], f=ONE + 2), 1, 32, 2, 3) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert gfwd(_table([0], f=None, o=None, r=None), 1, 32, 2, 3) == 0


def test_roi_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()

    def levels(feats=ONE, V=4):
        tab = (_hip.AabrRoiLevel * 1)()
        tab[0].feats, tab[0].cellmap, tab[0].V, tab[0].nb = feats, ONE, V, 1
        tab[0].height = tab[0].width = tab[0].zsize = 2
        tab[0].spatial_scale = 1.0
        return tab
    pf = lambda tab, n_levels=1, rois=ONE: lib.aabr_roi_pool_forward_bf16(tab, n_levels, 8, 1, rois, ONE, 3, 2, 2, 2, 2, ONE,
                                                                         None)
    pb = lambda tab, acc=ONE, out=ONE, total=4, g=ONE: lib.aabr_roi_pool_backward_bf16(tab, 1, 8, 1, ONE, ONE, 3, 2, 2, 2, 2,
                                                                                      g, acc, out, total, None)
    assert pf(levels(), n_levels=0) == E and b"n_levels" in lib.aabr_last_error()
    assert pf(levels(feats=None)) == E
    assert pf(levels(), rois=None) == E and b"null" in lib.aabr_last_error()
    assert pf(levels(feats=ONE + 2)) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert pb(levels(), acc=None) == E and b"accum_f32" in lib.aabr_last_error()
    assert pb(levels(), out=None) == E
    assert pb(levels(), out=ONE + 2) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert pb(levels(), total=3) == E and b"row_offset" in lib.aabr_last_error()     # V = 4 rows do not fit
    assert pb(levels(V=0), acc=None, out=None, total=0) == 0                          # nothing to do: success, no launch
    sf = lambda f=ONE, out=ONE, C=8: lib.aabr_roi_align_rotated_3d_sparse_forward_bf16(f, C, ONE, 1, 2, 2, 2, ONE, 3, 1.0, 2,
                                                                                     2, 2, 2, out, None)
    sb = lambda acc=ONE, out=ONE, V=4, g=ONE: lib.aabr_roi_align_rotated_3d_sparse_backward_bf16(
        g, 8, ONE, 1, 2, 2, 2, ONE, 3, 1.0, 2, 2, 2, 2, V, acc, out, None)
    assert sf(f=None) == E and b"null" in lib.aabr_last_error()
    assert sf(out=None) == E
    assert sf(C=0) == E and b"geometry" in lib.aabr_last_error()
    assert sf(f=ONE + 2) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert sb(acc=None) == E and b"accum_f32" in lib.aabr_last_error()
    assert sb(out=None) == E
    assert sb(out=ONE + 2) == E and b"4-byte aligned" in lib.aabr_last_error()
    assert sb(V=-1) == E
    assert sb(acc=None, out=None, V=0) == 0


def _params(C, AG, dtype=torch.float32):
    return (torch.zeros(C, C, dtype=dtype), torch.zeros(C, dtype=dtype), torch.zeros(AG, C, dtype=dtype),
            torch.zeros(AG, dtype=dtype), torch.zeros(7 * AG, C, dtype=dtype), torch.zeros(7 * AG, dtype=dtype))


def test_rpn_glue_takes_bf16_maps_only_with_the_keyword():
    import rpn_glue
    b16, f32 = torch.zeros(3, 32, dtype=torch.bfloat16), torch.zeros(3, 32)
    # with the keyword the dtype checks pass on CPU tensors: the call gets as far as needing the GPU
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):
        rpn_glue.rpn_head([b16, b16], *_params(32, 2), feature_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):
        rpn_glue.rpn_head_grouped([b16], *_params(32, 6), 3, feature_dtype=torch.bfloat16)
    # without it: as before, and the message names the keyword
    with pytest.raises(TypeError, match="float32") as e:
        rpn_glue.rpn_head([b16], *_params(32, 2))
    assert "feature_dtype=torch.bfloat16" in str(e.value)
    with pytest.raises(TypeError, match="float32") as e:
        rpn_glue.rpn_head_grouped([b16], *_params(32, 6), 3)
    assert "feature_dtype=torch.bfloat16" in str(e.value)
    # fp32 maps under the keyword, a mix either way, bf16 parameters, another dtype
    with pytest.raises(TypeError, match="bfloat16"):
        rpn_glue.rpn_head([f32], *_params(32, 2), feature_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        rpn_glue.rpn_head([b16, f32], *_params(32, 2), feature_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        rpn_glue.rpn_head([f32, b16], *_params(32, 2))
    with pytest.raises(TypeError, match="float32"):
        rpn_glue.rpn_head([b16], *_params(32, 2, torch.bfloat16), feature_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="feature_dtype"):
        rpn_glue.rpn_head([f32.half()], *_params(32, 2), feature_dtype=torch.float16)
    # the shape checks are the fp32 path's
    with pytest.raises(ValueError, match="32 to 128"):
        rpn_glue.rpn_head([torch.zeros(3, 48, dtype=torch.bfloat16)], *_params(48, 2), feature_dtype=torch.bfloat16)


class _X(object):
    def __init__(self, V, C, dtype=torch.float32):
        self.features = torch.zeros((V, C), dtype=dtype)


def test_pooler_glue_takes_all_bf16_levels_and_refuses_a_mix():
    import roi_glue
    boxes = [torch.zeros((3, 7))]
    args = ((5, 11, 4), (0.5, 0.25), 2, 8)
    b16 = torch.bfloat16
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):                      # the dtype check passes
        roi_glue.pool_rois([_X(4, 8, b16), _X(3, 8, b16)], boxes, *args)
    for mix in ([_X(4, 8), _X(3, 8, b16)], [_X(4, 8, b16), _X(3, 8)], [_X(4, 8, torch.float16)] * 2,
                [_X(4, 8, torch.float64)] * 2):
        with pytest.raises(TypeError):
            roi_glue.pool_rois(mix, boxes, *args)
    # the dense layers behind the pooler keep refusing bf16: the pooled tensor stays fp32
    with pytest.raises(TypeError):
        roi_glue.dense_linear(torch.zeros(2, 8, dtype=b16), torch.zeros(3, 8), None, False)


def test_fpn_net_cast_outputs_defaults_to_true_and_refuses_the_compiled_graph():
    from test_cabi_and_host import default_fpn
    net = default_fpn(feature_dtype=torch.bfloat16)
    assert net.cast_outputs is True
    net.cast_outputs = False
    net.compiled_graph = True
    with pytest.raises(ValueError) as e:
        net(None)
    assert "compiled_graph" in str(e.value) and "cast_outputs" in str(e.value)
