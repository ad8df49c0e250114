"""Host-side checks of the batched input layer (BLInputLayer / BLOutputLayer, quantize_scenes_bl), no GPU:

* tests/bl_ref.py -- the numpy restatement the GPU tests hold the kernels to -- against hand-written tables for a 2 x 5
  batch, and its fp32 forward / backward passes BIT-EQUAL to the reference's own CPU kernels (InputLayer_ForwardPass /
  _BackwardPass of SCN/CPU/IOLayers.cpp, which cpu_BLInputLayer_* call too) run on the restatement's rule tables, through
  oracle/_ref/libref_kernels.so (skipped where that library has not been built);
* the argument refusals of the new C-ABI entry points and of the Python layers, all before any launch;
* header, binding and library agree on the new symbols, and the ABI version is still 640."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bl_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libref_kernels.so")
NEW_SYMBOLS = ("aabr_bl_input_layer_sites", "aabr_bl_points_prepare", "aabr_quantize_scenes_bl")

# the 2 x 5 batch: sample 0 holds (1,2,3) twice, one all -1 row and one row that is empty although y, z >= 0;
# sample 1 holds (4,5,6) four times -- the coordinate sample 0 has once -- and (1,2,3) once
COORDS = np.array([[[1, 2, 3], [-1, -1, -1], [4, 5, 6], [1, 2, 3], [-1, 7, 8]],
                   [[4, 5, 6], [1, 2, 3], [4, 5, 6], [4, 5, 6], [4, 5, 6]]], np.int64)
FEATS = np.array([[i + 1, 10 * (i + 1)] for i in range(10)], np.float32).reshape(2, 5, 2)
SITES = [[1, 2, 3, 0], [4, 5, 6, 0], [4, 5, 6, 1], [1, 2, 3, 1]]
POINT_SITE = [0, -1, 1, 0, -1, 2, 3, 2, 2, 2]
RULES = {3: [[2, 0, 3, 0, 0], [1, 2, 0, 0, 0], [4, 5, 7, 8, 9], [1, 6, 0, 0, 0]],
         1: [[1, 3], [1, 2], [1, 9], [1, 6]],          # the LAST point of a site
         2: [[1, 0], [1, 2], [1, 5], [1, 6]]}          # the FIRST
RULES[4] = RULES[0] = RULES[3]
OUT = {3: [[5, 50], [3, 30], [33, 330], [7, 70]], 4: [[2.5, 25], [3, 30], [8.25, 82.5], [7, 70]],
       1: [[4, 40], [3, 30], [10, 100], [7, 70]], 2: [[1, 10], [3, 30], [6, 60], [7, 70]]}
D_OUT = np.array([[v + 1, -(v + 1)] for v in range(4)], np.float32)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_restatement_rule_tables_by_hand(mode):
    rb = R.bl_rules(COORDS, mode)
    assert (rb["B"], rb["L"], rb["V"]) == (2, 5, 4)
    assert rb["site_coords"].tolist() == SITES
    assert rb["sample_off"].tolist() == [0, 2, 4]
    assert rb["point_site"].tolist() == POINT_SITE
    assert rb["rules"].tolist() == RULES[mode]
    assert rb["max_active"] == len(RULES[mode][0]) - 1


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_restatement_passes_by_hand(mode):
    rb = R.bl_rules(COORDS, mode)
    assert R.forward(rb, FEATS).tolist() == OUT[mode]
    want = np.zeros((10, 2), np.float32)
    for v, row in enumerate(RULES[mode]):
        for p in row[1:1 + row[0]]:
            want[p] = D_OUT[v] * (1.0 / row[0] if mode == 4 else 1.0)       # counts 1, 2, 4: exact in fp32
    assert R.same_bits(R.backward(rb, D_OUT), want.reshape(2, 5, 2))
    # BLOutputLayer: the listed points receive their site's row un-averaged, every other row is exactly zero
    site_rows = np.array(OUT[3], np.float32)
    got = R.output_layer(rb, site_rows).reshape(10, 2)
    listed = sorted(p for row in RULES[mode] for p in row[1:1 + row[0]])
    for p in range(10):
        assert got[p].tolist() == (site_rows[POINT_SITE[p]].tolist() if p in listed else [0.0, 0.0]), p
    # ... and its gradient sums the listed points' rows per site
    g = np.arange(20, dtype=np.float32).reshape(2, 5, 2)
    want_g = [[sum(g.reshape(10, 2)[p, c] for p in row[1:1 + row[0]]) for c in range(2)] for row in RULES[mode]]
    assert R.output_layer_grad(rb, g).tolist() == want_g


def test_restatement_empty_and_degenerate():
    for shape in ((0, 4, 3), (3, 0, 3)):
        rb = R.bl_rules(np.zeros(shape, np.int64), 3)
        assert rb["V"] == 0 and rb["sample_off"].tolist() == [0] * (shape[0] + 1)
        assert R.output_layer(rb, np.zeros((0, 2), np.float32)).shape == (shape[0], shape[1], 2)
    rb = R.bl_rules(np.full((2, 3, 3), -1, np.int64), 4)
    assert rb["V"] == 0 and rb["point_site"].tolist() == [-1] * 6
    assert R.forward(rb, np.ones((2, 3, 5), np.float32)).shape == (0, 5)


# ------------------------------------------------------------------ the reference's own CPU kernels
@pytest.fixture(scope="module")
def ref_kernels():
    if not os.path.exists(REF_LIB):
        pytest.skip("oracle/_ref/libref_kernels.so has not been built (the reference sources are not on this machine)")
    lib = C.CDLL(REF_LIB)
    f32p, i32p = (np.ctypeslib.ndpointer(dt, flags="C_CONTIGUOUS") for dt in (np.float32, np.int32))
    sig = [f32p, f32p, C.c_long, C.c_int, C.c_int, i32p, C.c_int]
    lib.ref_input_layer_fwd.argtypes = lib.ref_input_layer_bwd.argtypes = sig
    lib.ref_input_layer_fwd.restype = lib.ref_input_layer_bwd.restype = None
    return lib


def _random_batch(rng, B, L, box, C_, p_empty):
    coords = np.stack([rng.integers(0, s, (B, L)) for s in box], 2).astype(np.int64)
    coords[rng.random((B, L)) < p_empty, 0] = -1
    return coords, (rng.standard_normal((B, L, C_)) * 3).astype(np.float32)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("B,L,box,C_", [(3, 40, (3, 3, 2), 5), (2, 700, (12, 12, 6), 3)])
def test_restatement_bit_equal_to_reference_cpu_kernels(ref_kernels, mode, B, L, box, C_):
    rng = np.random.default_rng(1000 * mode + L)
    coords, feats = _random_batch(rng, B, L, box, C_, 0.15)
    rb = R.bl_rules(coords, mode)
    V, ma = rb["V"], rb["max_active"]
    assert V > 0 and (ma > 2 or mode in (1, 2))
    flat = np.ascontiguousarray(feats.reshape(B * L, C_))
    for average in sorted({mode == 4, False}):              # the layer's own pass, and the un-averaged OutputLayer pass
        out = np.zeros((V, C_), np.float32)
        ref_kernels.ref_input_layer_fwd(flat, out, V, ma, C_, rb["rules"], int(average))
        assert R.same_bits(R.forward(rb, feats, average), out), (mode, average)
        d_out = rng.standard_normal((V, C_)).astype(np.float32)
        d_in = np.zeros((B * L, C_), np.float32)
        ref_kernels.ref_input_layer_bwd(d_in, d_out, V, ma, C_, rb["rules"], int(average))
        assert R.same_bits(R.backward(rb, d_out, average), d_in.reshape(B, L, C_)), (mode, average)


# ------------------------------------------------------------------ refusals, before any launch
def test_cabi_refusals():
    import _hip
    lib = _hip.load()
    none10 = [None] * 10
    for B, L in ((-1, 4), (4, -1), (1 << 16, 1 << 15), (70000, 1)):
        assert lib.aabr_bl_input_layer_sites(None, B, L, None, 64, *none10) == -1, (B, L)
        assert b"B * L < 2^31" in lib.aabr_last_error()
        assert lib.aabr_bl_points_prepare(None, B, L, None, None, None, None, None, None) == -1, (B, L)
        assert b"B * L < 2^31" in lib.aabr_last_error()
    assert lib.aabr_bl_input_layer_sites(None, 2, 3, None, 8, *none10) == -1                      # cap < max(64, 2 n)
    assert b"cap" in lib.aabr_last_error()
    assert lib.aabr_bl_input_layer_sites(None, 2, 3, None, 64, *none10) == -1
    assert b"null pointer" in lib.aabr_last_error()
    assert lib.aabr_bl_points_prepare(None, 2, 3, None, None, None, None, None, None) == -1
    assert b"null" in lib.aabr_last_error()
    # the quantiser: sizes, then the host arrays, then the device pointers
    fs = _hip.i32x3((64, 64, 32))
    q = lib.aabr_quantize_scenes_bl
    assert q(None, None, None, -1, 0, 0, 20.0, fs, 4, None, None, None, None) == -1
    assert q(None, None, None, 1, 0, 0, 20.0, fs, 4, None, None, None, None) == -1
    assert b"null host array" in lib.aabr_last_error()
    xs = (C.c_void_p * 1)(4096)                    # a made-up scene address: every call below is refused before it is used
    assert q(xs, None, _hip.i64xn([5]), 1, 0, 0, 20.0, fs, 4, None, None, None, None) == -1
    assert b"more than L" in lib.aabr_last_error()
    assert q(xs, None, _hip.i64xn([4]), 1, 0, 2, 20.0, fs, 4, None, None, None, None) == -1      # extra planes, no array
    assert q(xs, None, _hip.i64xn([4]), 1, 0, 0, 0.0, fs, 4, None, None, None, None) == -1       # scale
    assert q((C.c_void_p * 1)(None), None, _hip.i64xn([4]), 1, 0, 0, 20.0, fs, 4, None, None, None, None) == -1
    assert b"null scene pointer" in lib.aabr_last_error()
    assert q(xs, None, _hip.i64xn([4]), 1, 0, 0, 20.0, fs, 4, None, None, None, None) == -1
    assert b"null pointer" in lib.aabr_last_error()
    assert q(xs, None, _hip.i64xn([0]), 1, 0, 0, 20.0, fs, 0, None, None, None, None) == 0         # L = 0: nothing to do


def test_python_layer_refusals():
    """TypeError / ValueError from the argument checks -- raised before the device is even asked for"""
    import sparseconvnet as scn
    ok_c, ok_f = torch.zeros((2, 4, 3), dtype=torch.int64), torch.zeros((2, 4, 5))
    for mode in (-1, 5, 7):
        with pytest.raises(ValueError, match="mode"):
            scn.BLInputLayer(3, [16, 16, 16], mode=mode)([ok_c, ok_f])
    layer = scn.BLInputLayer(3, [16, 16, 16], mode=4)
    for bad in (torch.zeros((8, 3), dtype=torch.int64), torch.zeros((2, 4, 4), dtype=torch.int64),
                torch.zeros((2, 4, 3, 1), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[B, L, 3\]"):
            layer([bad, ok_f])
    for bad in (torch.zeros((2, 4, 3)), torch.zeros((2, 4, 3), dtype=torch.bool)):
        with pytest.raises(TypeError, match="integer"):
            layer([bad, ok_f])
    for bad in (ok_f.double(), ok_f.bfloat16(), ok_f.half()):
        with pytest.raises(TypeError, match="float32"):
            layer([ok_c, bad])
    for bad in (torch.zeros((8, 5)), torch.zeros((2, 5, 5)), torch.zeros((3, 4, 5))):
        with pytest.raises(ValueError, match=r"\[B, L, C\]"):
            layer([ok_c, bad])
    with pytest.raises(ValueError, match="mode"):
        scn.SCN.BLInputLayer_updateOutput(scn.Metadata(3), layer.spatial_size, ok_c, ok_f, ok_f.new(), 9)


def test_surface_names():
    import sparseconvnet as scn
    for name in ("BLInputLayer", "BLOutputLayer", "BLInputLayerFunction", "BLOutputLayerFunction"):
        assert hasattr(scn, name), name
    for name in ("BLInputLayer_updateOutput", "BLInputLayer_updateGradInput", "BLOutputLayer_updateOutput",
                 "BLOutputLayer_updateGradInput"):
        assert hasattr(scn.SCN, name), name
    assert hasattr(scn.SCN.Metadata_3, "blLayer") and hasattr(scn.SCN.Metadata_3, "blLayerRuleBook")
    layer = scn.BLInputLayer(3, [16, 16, 16])
    assert layer.mode == 3 and layer.site_order == "first_seen" and layer.to("cuda:0") is layer
    assert scn.BLInputLayer.prepare is scn.InputLayer.prepare            # one prepare, not a copy
    assert scn.SCN.BL_KERNEL_MODE == {0: 3, 1: 2, 2: 1, 3: 3, 4: 4}
    import input_pipeline
    assert callable(input_pipeline.quantize_scenes_bl)


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    assert re.search(r"#define\s+AABR_ABI_VERSION\s+640\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(aabr_\w+)\s*\(", code))
    lib = C.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip._SIGS and hasattr(lib, name), name
        # the header cites what the symbol replaces
        doc = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert re.search(r"\.(py|h|cpp):\d+", doc), name
        # one ctypes argument per declared parameter
        params = code[code.index(name + "("):].split(")", 1)[0].split("(", 1)[1]
        assert len(_hip._SIGS[name][1]) == params.count(",") + 1, name
    assert _hip.ABI_VERSION == 640 and _hip.load().aabr_version() == 640
