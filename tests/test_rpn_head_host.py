"""The RPN head without a GPU: the new C-ABI symbols (header, binding, library, argument checks that return before any
HIP call), rpn_glue.rpn_head's refusals, the RPNHead / RPNModule modules against tests/golden/rpn_head_golden.npz (made
by importing the reference's own code: tests/golden/gen_rpn_head_golden.py) and against plain torch, and the fp64
definition (tests/rpn_head_ref.py) against torch autograd in float64, with the undecidable share of its test inputs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_head_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "rpn_head_golden.npz"))
NEW_SYMBOLS = ("aabr_rpn_head_tile_rows", "aabr_rpn_head_groups", "aabr_rpn_head_scratch_floats", "aabr_rpn_head_forward",
               "aabr_rpn_head_backward")


def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640 and _hip.ABI_VERSION == 640 and "#define AABR_ABI_VERSION 640" in hdr
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name
    fields = re.search(r"typedef struct AabrRpnMap \{(.*?)\} AabrRpnMap;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names == [n for n, _ in _hip.AabrRpnMap._fields_]
    assert ctypes.sizeof(_hip.AabrRpnMap) == 40


def test_dispatch_functions_are_monotone_and_in_their_documented_ranges():
    import _hip
    lib = _hip.load()
    tr, gr, sf = lib.aabr_rpn_head_tile_rows, lib.aabr_rpn_head_groups, lib.aabr_rpn_head_scratch_floats
    assert [tr(c) for c in (32, 64, 96, 128)] == [64] * 4
    assert [tr(c) for c in (0, 16, 48, 160, -32)] == [0] * 5
    assert gr(0) == 0 and gr(-3) == 0 and gr(1) == 1
    prev = 0
    for n in list(range(1, 600)) + [10 ** 6, 2 ** 31 - 2, 2 ** 40]:
        g = gr(n)
        assert prev <= g <= min(n, 256)                                        # monotone, never more groups than tiles
        prev = g
    assert gr(256) == 256 and gr(257) == 256
    for C in (32, 128):
        for A in (1, 4):
            per = C * C + 32 * C + C + 32
            assert sf(1, C, A) == per and sf(300, C, A) == 256 * per and sf(0, C, A) == 0
    assert sf(5, 48, 2) == 0 and sf(5, 32, 5) == 0 and sf(5, 32, 0) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()
    one = 4096                                                                   # a non-null pointer nobody follows
    E = -1

    def table(rows, f=one, o=one, r=one, d=one):
        tab = (_hip.AabrRpnMap * len(rows))()
        for i, n in enumerate(rows):
            tab[i].features, tab[i].rows, tab[i].objectness, tab[i].box_regression, tab[i].d_features = f, n, o, r, d
        return tab
    fwd = lambda tab, n, C, A, w=one, h=None: lib.aabr_rpn_head_forward(tab, n, C, A, w, one, one, one, one, one, h, None)
    bwd = lambda tab, n, C, A, w=one, h=one, g=one, s=one: lib.aabr_rpn_head_backward(tab, n, C, A, w, one, one, h, g, one,
                                                                                      one, one, one, one, s, None)
    assert fwd(table([5]), 0, 32, 2) == E and b"n_maps" in lib.aabr_last_error()
    assert fwd(table([5] * 9), 9, 32, 2) == E
    assert fwd(table([5]), 1, 48, 2) == E and b"C must be" in lib.aabr_last_error()
    assert fwd(table([5]), 1, 160, 2) == E
    assert fwd(table([5]), 1, 32, 5) == E and b"A must be" in lib.aabr_last_error()
    assert fwd(table([5]), 1, 32, 0) == E
    assert fwd(None, 1, 32, 2) == E
    assert fwd(table([-1]), 1, 32, 2) == E and b"negative" in lib.aabr_last_error()
    assert fwd(table([5], f=None), 1, 32, 2) == E and b"null" in lib.aabr_last_error()
    assert fwd(table([5], o=None), 1, 32, 2) == E
    assert fwd(table([5], r=None), 1, 32, 2) == E
    assert fwd(table([5]), 1, 32, 2, w=None) == E
    assert fwd(table([0, 0], f=None, o=None, r=None), 2, 32, 2) == 0             # every map empty: success, no launch
    assert bwd(table([5]), 1, 48, 2) == E
    assert bwd(table([5], d=None), 1, 32, 2) == E and b"d_features" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, h=None) == E and b"hidden" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, s=None) == E and b"scratch" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, g=None) == E
    assert bwd(table([5]), 1, 32, 2, w=None) == E
    assert bwd(table([5] * 9), 9, 32, 2) == E


def _params(C, A, dtype=torch.float32):
    return (torch.zeros(C, C, dtype=dtype), torch.zeros(C, dtype=dtype), torch.zeros(A, C, dtype=dtype),
            torch.zeros(A, dtype=dtype), torch.zeros(7 * A, C, dtype=dtype), torch.zeros(7 * A, dtype=dtype))


def test_glue_argument_checks_hold_before_it_needs_a_gpu():
    import rpn_glue
    with pytest.raises(TypeError, match="float32"):
        rpn_glue.rpn_head([torch.zeros(3, 32, dtype=torch.bfloat16)], *_params(32, 2))
    with pytest.raises(TypeError, match="float32"):
        rpn_glue.rpn_head([torch.zeros(3, 32)], *_params(32, 2, torch.float64))
    for C in (48, 160):
        with pytest.raises(ValueError, match="32 to 128"):
            rpn_glue.rpn_head([torch.zeros(3, C)], *_params(C, 2))
    with pytest.raises(ValueError, match="1 to 4"):
        rpn_glue.rpn_head([torch.zeros(3, 32)], *_params(32, 5))
    with pytest.raises(ValueError, match="maps"):
        rpn_glue.rpn_head([], *_params(32, 2))
    with pytest.raises(ValueError, match="maps"):
        rpn_glue.rpn_head([torch.zeros(1, 32)] * 9, *_params(32, 2))
    with pytest.raises(ValueError, match=r"features\[1\]"):                      # mismatched lists: a map of another width
        rpn_glue.rpn_head([torch.zeros(3, 32), torch.zeros(3, 64)], *_params(32, 2))
    p = list(_params(32, 2))
    p[4] = torch.zeros(7, 32)                                                    # reg_w for one anchor, cls_w for two
    with pytest.raises(ValueError, match="reg_w"):
        rpn_glue.rpn_head([torch.zeros(3, 32)], *p)
    p = list(_params(32, 2))
    p[1] = torch.zeros(31)
    with pytest.raises(ValueError, match="biases"):
        rpn_glue.rpn_head([torch.zeros(3, 32)], *p)
    with pytest.raises(ValueError, match="conv_w"):
        rpn_glue.rpn_head([torch.zeros(3, 32)], torch.zeros(32, 32, 3, 3), *_params(32, 2)[1:])


@pytest.mark.parametrize("key", ["h128", "h32"])
def test_rpn_head_parameters_are_the_reference_modules(key):
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    C, A = (int(v) for v in GOLDEN[key + "_C_A"])
    head = RPNHead(rpn_glue.rpn_cfg(C=C), C, A)
    want = {str(n): tuple(int(v) for v in s[:d]) for n, s, d in zip(GOLDEN[key + "_names"], GOLDEN[key + "_shapes"],
                                                                    GOLDEN[key + "_dims"])}
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want
    assert list(head.state_dict()) == [str(n) for n in GOLDEN[key + "_names"]]
    assert head.fused and head.seperate_rpn == 1 and head.num_anchors_per_location == A
    assert all(float(b.detach().abs().max()) == 0 for b in (head.conv.bias, head.cls_logits.bias, head.bbox_pred.bias))
    assert 0.005 < float(head.conv.weight.detach().std()) < 0.02                          # normal, std 0.01
    # a state dict in the reference's shapes loads
    sd = {n: torch.randn(*s) for n, s in want.items()}
    head.load_state_dict(sd, strict=True)
    assert torch.equal(head.bbox_pred.weight, sd["bbox_pred.weight"])


def test_unfused_head_is_plain_torch_bit_for_bit_in_every_input_form():
    import rpn_glue
    import sparseconvnet as scn
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    torch.manual_seed(3)
    C, A = 32, 2
    head = RPNHead(rpn_glue.rpn_cfg(C=C), C, A)
    head.fused = False
    with torch.no_grad():
        for p in head.parameters():
            p.normal_()
    rows = [torch.randn(37, C), torch.randn(1, C)]
    x4 = [r.t().unsqueeze(0).unsqueeze(3) for r in rows]                          # RPNModule.forward's reshape, :184-187
    logits, bbox = head(x4)
    for f, lg, bb in zip(x4, logits, bbox):                                       # rpn_sparse3d.py:115-124, typed out
        t = F.relu(F.conv2d(f, head.conv.weight, head.conv.bias))
        lo = F.conv2d(t, head.cls_logits.weight, head.cls_logits.bias).permute(0, 2, 1, 3)
        lo = lo.reshape(1, lo.shape[1], A, 1)
        rg = F.conv2d(t, head.bbox_pred.weight, head.bbox_pred.bias).permute(0, 2, 1, 3)
        rg = rg.reshape(1, rg.shape[1], A, 7)
        assert torch.equal(lg, lo) and torch.equal(bb, rg)
        assert tuple(lg.shape) == (1, f.shape[2], A, 1) and tuple(bb.shape) == (1, f.shape[2], A, 7)
    sp = [scn.SparseConvNetTensor(r, None, None) for r in rows]
    for form in (rows, sp):
        l2, b2 = head(form)
        assert all(torch.equal(a, b) for a, b in zip(l2 + b2, logits + bbox))
    flat_o, flat_r = head.forward_flat(rows)
    assert tuple(flat_o[0].shape) == (37 * A,) and tuple(flat_r[0].shape) == (37 * A, 7)
    l0, b0 = head([torch.zeros(0, C)])
    assert tuple(l0[0].shape) == (1, 0, A, 1) and tuple(b0[0].shape) == (1, 0, A, 7)


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_base_anchors_match_the_reference(key):
    from maskrcnn_benchmark.modeling.rpn.anchor_generator_sparse3d import AnchorGenerator, generate_anchors_3d
    sizes, yaws, ratios = GOLDEN[key + "_sizes"], GOLDEN[key + "_yaws"], GOLDEN[key + "_ratios"]
    use, want = GOLDEN[key + "_use_yaws"], GOLDEN[key + "_anchors"]
    for s, u, w in zip(sizes, use, want):
        got = generate_anchors_3d(s, yaws, ratios, int(u))
        assert got.dtype == torch.float32 and got.numpy().tobytes() == w.tobytes()
    if len(yaws) == len(ratios):
        gen = AnchorGenerator(20.0, sizes.tolist(), tuple(yaws.tolist()), ratios.tolist(), use.tolist(),
                              [[8, 8, 8]] * len(sizes))
        assert gen.num_anchors_per_location() == len(yaws)
        assert all(c.numpy().tobytes() == w.tobytes() for c, w in zip(gen.cell_anchors, want))


def test_rpn_module_builds_and_refuses_the_separated_configuration():
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead, RPNModule, build_rpn
    m = build_rpn(rpn_glue.rpn_cfg(C=32))
    assert isinstance(m, RPNModule) and isinstance(m.head, RPNHead)
    assert sorted(m.state_dict()) == sorted("head." + n for n in GOLDEN["h32_names"])
    assert m.head.num_anchors_per_location == 2 and len(m.anchor_generator.cell_anchors) == 2
    with pytest.raises(ValueError, match="SEPARATE_RPN"):
        build_rpn(rpn_glue.rpn_cfg(separate=("door",)))
    build_rpn(rpn_glue.rpn_cfg(separate=("door",), separate_rpn=False))          # one group: nothing separated
    cfg = rpn_glue.rpn_cfg()
    cfg.MODEL.RPN.RPN_HEAD = "SomethingElse"
    with pytest.raises(ValueError, match="RPN_HEAD"):
        build_rpn(cfg)
    with pytest.raises(ValueError, match="targets"):
        m.train()
        m.head.fused = False
        m(None, [torch.zeros(0, 32)], None)


@pytest.mark.parametrize("C,A", [(32, 1), (64, 4)])
def test_definition_agrees_with_torch_float64_autograd(C, A):
    p, f, g_obj, g_reg = R.make_case(C, A, (19, 0, 5), 11)
    f_all, go, gr = np.concatenate(f), np.concatenate(g_obj), np.concatenate(g_reg)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    tf = torch.tensor(f_all, dtype=torch.float64, requires_grad=True)
    t = torch.relu(tf @ tp["conv_w"].t() + tp["conv_b"])
    obj, reg = t @ tp["cls_w"].t() + tp["cls_b"], t @ tp["reg_w"].t() + tp["reg_b"]
    ((obj * torch.tensor(go, dtype=torch.float64)).sum() + (reg * torch.tensor(gr, dtype=torch.float64)).sum()).backward()
    fwd = R.forward(f_all, p)
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert rel(fwd["obj"].v, obj.detach().numpy()) < 1e-12 and rel(fwd["reg"].v, reg.detach().numpy()) < 1e-12
    bwd = R.backward(f_all, p, go, gr, fwd["t"].v, fwd)
    assert rel(bwd["d_f"].v, tf.grad.numpy()) < 1e-12
    for k in p:
        assert rel(bwd["d_" + k].v, tp[k].grad.numpy()) < 1e-12, k
    for v in list(fwd.values()) + list(bwd.values()):
        assert (v.s >= 0).all() and np.isfinite(v.s).all()


def test_undecidable_share_of_the_test_inputs_stays_under_the_cap():
    """for the reference alone: the seeds the GPU tests use leave far fewer than 1 % of the hidden units within their
    bound of zero"""
    T = 64
    cases = R.entry_cases(T) + R.hidden_cases(T) + [(32, 2, (258 * T + 5,), 5), (32, 2, (7,), 6)]
    for C, A, rows, seed in cases:
        p, f, _, _ = R.make_case(C, A, rows, seed)
        share = float(R.undecided(R.forward(np.concatenate(f), p)).mean())
        assert share < R.MAX_UNDECIDED, (C, A, rows, share)
