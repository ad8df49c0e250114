"""The separated-classifier RPN without a GPU: the RPNHead module with groups (the reference's parameter shapes, the
unfused forward against the reference's permute + reshape typed out here), rpn_glue.rpn_group_targets on host labels
against tests/sep_ref.py, the new C-ABI symbols (header, binding, library, argument checks that return before any HIP
call), the Python refusals, the SeperateClassifier's role flag, and the undecidable share of the inputs of
tests/test_gpu_sep_rpn_head.py."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rpn_head_grouped_ref as GR
import rpn_head_ref as R
import sep_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aabr_rpn_head_grouped_scratch_floats", "aabr_rpn_head_grouped_forward", "aabr_rpn_head_grouped_backward",
               "aabr_rpn_loss_grouped_scratch_words", "aabr_rpn_loss_grouped_forward", "aabr_rpn_loss_grouped_backward")


def _cfg(G, C=32, **kw):
    import rpn_glue
    names = ["c%d" % i for i in range(G - 1)]
    return rpn_glue.rpn_cfg(C=C, separate=names, separate_ids=[[i + 1] for i in range(G - 1)],
                            classes=["background"] + names + ["rest"], **kw)


# ------------------------------------------------------------------------------------------------ the head module
def test_parameter_shapes_and_state_dict_are_the_references():
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    C, A, G = 64, 4, 3
    head = RPNHead(_cfg(G, C), C, A)
    want = {"conv.weight": (C, C, 1, 1), "conv.bias": (C,), "cls_logits.weight": (A * G, C, 1, 1),
            "cls_logits.bias": (A * G,), "bbox_pred.weight": (7 * A * G, C, 1, 1), "bbox_pred.bias": (7 * A * G,)}
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want
    assert list(head.state_dict()) == list(want)
    assert head.fused and head.seperate_rpn == G and head.num_anchors_per_location == A
    sd = {n: torch.randn(*s) for n, s in want.items()}
    head.load_state_dict(sd, strict=True)
    assert torch.equal(head.cls_logits.weight, sd["cls_logits.weight"])


@pytest.mark.parametrize("A,G", [(2, 3), (4, 2), (1, 2)])
def test_unfused_head_is_the_references_permute_and_reshape_bit_for_bit(A, G):
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead
    torch.manual_seed(3)
    C = 32
    head = RPNHead(_cfg(G, C), C, A)
    head.fused = False
    with torch.no_grad():
        for p in head.parameters():
            p.normal_()
    rows = [torch.randn(37, C), torch.randn(1, C)]
    x4 = [r.t().unsqueeze(0).unsqueeze(3) for r in rows]
    logits, bbox = head(x4)
    flat_o, flat_r = head.forward_flat(rows)
    for f, lg, bb, fo, fr in zip(x4, logits, bbox, flat_o, flat_r):               # rpn_sparse3d.py:115-124, typed out
        t = F.relu(F.conv2d(f, head.conv.weight, head.conv.bias))
        lo = F.conv2d(t, head.cls_logits.weight, head.cls_logits.bias).permute(0, 2, 1, 3)
        lo = lo.reshape(1, lo.shape[1], A, G)
        rg = F.conv2d(t, head.bbox_pred.weight, head.bbox_pred.bias).permute(0, 2, 1, 3)
        rg = rg.reshape(1, rg.shape[1], A, 7 * G)
        assert torch.equal(lg, lo) and torch.equal(bb, rg)
        n = f.shape[2]
        assert tuple(fo.shape) == (G, n * A) and tuple(fr.shape) == (G, n * A, 7)
        for g in range(G):                                                        # group g: column g, the 7 g .. 7 g + 7 slice
            assert torch.equal(fo[g], lo[0, :, :, g].reshape(-1))
            assert torch.equal(fr[g], rg[0, :, :, 7 * g:7 * g + 7].reshape(-1, 7))
    l0, b0 = head([torch.zeros(0, C)])
    assert tuple(l0[0].shape) == (1, 0, A, G) and tuple(b0[0].shape) == (1, 0, A, 7 * G)
    o0, r0 = head.forward_flat([torch.zeros(0, C)])
    assert tuple(o0[0].shape) == (G, 0) and tuple(r0[0].shape) == (G, 0, 7)


def test_group_permutation_of_the_reference_file_is_its_own_inverse():
    rng = np.random.default_rng(0)
    for A, G in GR.GROUPS:
        for k in (1, 7):
            x = rng.standard_normal((5, k * A * G))
            y = GR.to_groups(x, A, G, k)
            assert y.shape == ((G, 5, A) if k == 1 else (G, 5, A, 7))
            assert np.array_equal(GR.from_groups(y, A, G, k), x)
        p = R.make_case(32, A * G, (3,), 1)[0]
        for g in range(G):
            pg = GR.group_params(p, A, G, g)
            assert all(np.array_equal(pg["cls_w"][a], p["cls_w"][a * G + g]) for a in range(A))
            assert all(np.array_equal(pg["reg_w"][a * 7 + k], p["reg_w"][a * 7 * G + 7 * g + k])
                       for a in range(A) for k in range(7))
            assert all(pg["reg_b"][a * 7 + k] == p["reg_b"][a * 7 * G + 7 * g + k] for a in range(A) for k in range(7))
        assert GR.dt_terms(A, G) == 32 * int(np.ceil(8 * A * G / 32)) + 2


# ------------------------------------------------------------------------------------------------ the targets
def test_group_targets_on_host_labels_equal_the_restatement():
    import rpn_glue
    gc = [[0, 2, 3, 6], [7, 1], [8, 4, 5]]                                        # seven classes, groups [[1], [5, 4]]
    labels = [torch.tensor([5, 4, 1, 5, 2, 4, 6, 2]), torch.tensor([2, 11, 6, 2, -1]), torch.zeros(0, dtype=torch.int64)]
    targets = [torch.arange(7.0 * len(l)).reshape(-1, 7) + 100 * b for b, l in enumerate(labels)]
    boxes, local, rows, counts = rpn_glue.rpn_group_targets(targets, labels, gc)
    assert len(boxes) == 3 and all(len(b) == 3 for b in boxes)
    for b, l in enumerate(labels):
        for g in range(3):
            r, loc = SR.filter_gt(l.numpy(), gc, g)
            assert rows[b][g].tolist() == r.tolist() and local[b][g].tolist() == loc.tolist()
            assert counts[b][g] == len(r) and torch.equal(boxes[b][g], targets[b][torch.as_tensor(r)])
            assert boxes[b][g].dtype == torch.float32 and tuple(boxes[b][g].shape) == (len(r), 7)
    assert counts == [[3, 1, 4], [3, 0, 0], [0, 0, 0]]                            # empty groups; 11 and -1 are dropped
    assert rows[0][2].tolist() == [1, 5, 0, 3] and local[0][2].tolist() == [1, 1, 2, 2]
    with pytest.raises(ValueError, match="labels"):
        rpn_glue.rpn_group_targets(targets, labels[:2], gc)
    with pytest.raises(ValueError, match="labels"):
        rpn_glue.rpn_group_targets(targets, [labels[0][:3]] + labels[1:], gc)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_library_agree_on_the_new_symbols():
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    lib = _hip.load()
    assert lib.aabr_version() == 640 and _hip.ABI_VERSION == 640 and "#define AABR_ABI_VERSION 640" in hdr
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert decl.count(",") + 1 == len(_hip._SIGS[name][1]), name


def test_scratch_sizes():
    import _hip
    lib = _hip.load()
    sf, sw = lib.aabr_rpn_head_grouped_scratch_floats, lib.aabr_rpn_loss_grouped_scratch_words
    for C in (32, 128):
        for A, G in GR.GROUPS:
            NP = 32 * -(-8 * A * G // 32)
            per = C * C + NP * C + C + NP
            assert sf(1, C, A, G) == per and sf(300, C, A, G) == 256 * per and sf(0, C, A, G) == 0
    assert sf(5, 48, 2, 2) == 0 and sf(5, 32, 2, 1) == 0 and sf(5, 32, 2, 9) == 0 and sf(5, 32, 3, 6) == 0
    assert sf(5, 32, 5, 2) == 0 and sf(5, 32, 0, 2) == 0
    assert sw(2, 3) == lib.aabr_rpn_loss_scratch_words(6) and sw(0, 3) == 0 and sw(2, 1) == 0


def test_grouped_entry_points_refuse_bad_arguments_before_any_launch():
    import _hip
    lib = _hip.load()
    one = 4096                                                                   # a non-null pointer nobody follows
    E = -1

    def table(rows, f=one, o=one, r=one, d=one):
        tab = (_hip.AabrRpnMap * len(rows))()
        for i, n in enumerate(rows):
            tab[i].features, tab[i].rows, tab[i].objectness, tab[i].box_regression, tab[i].d_features = f, n, o, r, d
        return tab
    fwd = lambda tab, n, C, A, G, w=one, h=None: lib.aabr_rpn_head_grouped_forward(tab, n, C, A, G, w, one, one, one, one,
                                                                                   one, h, None)
    bwd = lambda tab, n, C, A, G, w=one, h=one, g=one, s=one: lib.aabr_rpn_head_grouped_backward(
        tab, n, C, A, G, w, one, one, h, g, one, one, one, one, one, s, None)
    for call in (fwd, bwd):
        assert call(table([5]), 1, 32, 2, 1) == E and b"G" in lib.aabr_last_error()      # G = 1: the plain entry point
        assert call(table([5]), 1, 32, 2, 9) == E
        assert call(table([5]), 1, 32, 1, 17) == E                               # A G = 17
        assert call(table([5]), 1, 32, 3, 6) == E                                # A G = 18
        assert call(table([5]), 1, 32, 4, 5) == E
        assert call(table([5]), 1, 32, 5, 2) == E and b"A must be" in lib.aabr_last_error()
        assert call(table([5]), 1, 48, 2, 2) == E and b"C must be" in lib.aabr_last_error()
        assert call(table([5]), 0, 32, 2, 2) == E
        assert call(None, 1, 32, 2, 2) == E
        assert call(table([-1]), 1, 32, 2, 2) == E
        assert call(table([5], f=None), 1, 32, 2, 2) == E
        assert call(table([5]), 1, 32, 2, 2, w=None) == E
    assert fwd(table([5], o=None), 1, 32, 2, 2) == E
    assert fwd(table([5], r=None), 1, 32, 2, 2) == E
    assert fwd(table([0, 0], f=None, o=None, r=None), 2, 128, 2, 8) == 0         # every map empty: success, no launch
    assert bwd(table([5], d=None), 1, 32, 2, 2) == E and b"d_features" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, 2, h=None) == E and b"hidden" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, 2, s=None) == E and b"scratch" in lib.aabr_last_error()
    assert bwd(table([5]), 1, 32, 2, 2, g=None) == E

    # the grouped loss
    i32, i64 = _hip.i32xn, _hip.i64xn
    pp = _hip.ptrs([torch.zeros(1)])                                             # one non-null pointer per map (never read)

    def loss(n_maps=1, G=2, nb=1, seg=(0, 4), site=(0,), rows=(2,), B=16, pos=8, ptrs=pp, out=one):
        return lib.aabr_rpn_loss_grouped_forward(n_maps, ptrs, ptrs, ptrs, i64(rows), 0, 2, nb, G, i32(seg), i32(site), ptrs,
                                                 ptrs, 1, B, pos, 0.1, out, one, one, one, one, None)
    assert loss(G=1) == E and b"G" in lib.aabr_last_error()
    assert loss(G=17) == E
    assert loss(n_maps=0) == E
    assert loss(B=513) == E
    assert loss(pos=17) == E
    assert loss(ptrs=None) == E and b"null" in lib.aabr_last_error()
    assert loss(out=None) == E
    assert loss(rows=(1,)) == E and b"rows" in lib.aabr_last_error()             # 2 sites of the scene in a 1-row map
    assert loss(seg=(0, 3)) == E                                                 # not a multiple of A
    assert lib.aabr_rpn_loss_grouped_backward(1, pp, pp, i64((2,)), 0, 2, 1, 1, i32((0, 4)), i32((0,)), pp, 16, 0.1, one,
                                              one, one, one, pp, pp, None) == E
    assert lib.aabr_rpn_loss_grouped_backward(1, pp, pp, i64((2,)), 0, 2, 1, 2, i32((0, 4)), i32((0,)), None, 16, 0.1, one,
                                              one, one, one, pp, pp, None) == E


# ------------------------------------------------------------------------------------------------ Python refusals
def _params(C, AG, dtype=torch.float32):
    return (torch.zeros(C, C, dtype=dtype), torch.zeros(C, dtype=dtype), torch.zeros(AG, C, dtype=dtype),
            torch.zeros(AG, dtype=dtype), torch.zeros(7 * AG, C, dtype=dtype), torch.zeros(7 * AG, dtype=dtype))


def test_glue_argument_checks_hold_before_it_needs_a_gpu():
    import rpn_glue
    f = [torch.zeros(3, 32)]
    with pytest.raises(TypeError, match="float32"):
        rpn_glue.rpn_head_grouped([torch.zeros(3, 32, dtype=torch.bfloat16)], *_params(32, 6), 3)
    for C, AG, G in ((48, 6, 3), (32, 6, 1), (32, 18, 9), (32, 18, 6), (32, 10, 2), (32, 7, 3)):
        with pytest.raises(ValueError, match="A G <= 16"):
            rpn_glue.rpn_head_grouped([torch.zeros(3, C)], *_params(C, AG), G)
    with pytest.raises(ValueError, match="maps"):
        rpn_glue.rpn_head_grouped([], *_params(32, 6), 3)
    p = list(_params(32, 6))
    p[4] = torch.zeros(7 * 3, 32)
    with pytest.raises(ValueError, match="reg_w"):
        rpn_glue.rpn_head_grouped(f, *p, 3)
    p = list(_params(32, 6))
    p[3] = torch.zeros(5)
    with pytest.raises(ValueError, match="biases"):
        rpn_glue.rpn_head_grouped(f, *p, 3)
    with pytest.raises(ValueError, match=r"features\[1\]"):
        rpn_glue.rpn_head_grouped([torch.zeros(3, 32), torch.zeros(3, 64)], *_params(32, 6), 3)
    with pytest.raises(ValueError, match="per \\(scene, group\\)"):
        rpn_glue.rpn_loss_grouped([None], [None], [None], [None] * 5, [None], 2)


def test_modules_refuse_what_the_issue_lists():
    import rpn_glue
    from maskrcnn_benchmark.modeling.rpn.rpn_sparse3d import RPNHead, build_rpn
    for C, A, G in ((32, 4, 5), (48, 2, 2), (32, 2, 9), (32, 5, 2)):
        with pytest.raises(ValueError, match="A G <= 16") as e:
            RPNHead(_cfg(G, 32), C, A)
        assert "2 <= G <= 8" in str(e.value) and "1 <= A <= 4" in str(e.value) and "128" in str(e.value)
    RPNHead(_cfg(8, 128), 128, 2)                                                # the limit
    # groups without ids, or with another number of ids than names
    for cfg in (rpn_glue.rpn_cfg(separate=("door",)), rpn_glue.rpn_cfg(separate=("door",), separate_ids=[[2], [1]]),
                rpn_glue.rpn_cfg(separate=("door", "wall"), separate_ids=[[2]])):
        with pytest.raises(ValueError, match="SEPARATE_RPN") as e:
            build_rpn(cfg)
        assert "SEPARATE_CLASSES_ID" in str(e.value)
        with pytest.raises(ValueError, match="SEPARATE_CLASSES_ID"):
            RPNHead(cfg, 32, 2)
    assert not hasattr(rpn_glue.rpn_cfg().MODEL, "SEPARATE_CLASSES_ID")          # set only when given
    build_rpn(rpn_glue.rpn_cfg(separate=("door",), separate_rpn=False))          # one group: nothing separated
    m = build_rpn(rpn_glue.rpn_cfg(separate=("door",), separate_ids=[[2]]))
    sc = m.seperate_classifier
    assert sc.need_seperate and sc.flag == "RPN" and sc.grouped_classes == [[0, 1], [3, 2]] and m.head.seperate_rpn == 2
    assert tuple(m.head.cls_logits.weight.shape) == (4, 32, 1, 1)
    plain = build_rpn(rpn_glue.rpn_cfg())
    assert plain.seperate_classifier.need_seperate is False
    # targets must carry labels
    m.train()
    m.head.fused = False
    with pytest.raises(ValueError, match="labels"):
        m(None, [torch.zeros(0, 32)], [torch.zeros(2, 7)])
    with pytest.raises(ValueError, match="targets"):
        m(None, [torch.zeros(0, 32)], None)


def test_rpn_methods_work_on_the_rpn_instance_only():
    from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import DetectionList3D
    rpn = SeperateClassifier([[1], [5, 4]], 7, False, "RPN")
    roi = SeperateClassifier([[1], [5, 4]], 7, False, "ROI_LOSS")
    names = ("seperate_rpn_assin", "seperate_rpn_selector", "seperate_rpn_loss_evaluator", "seperate_targets",
             "seperate_targets_and_update_labels")
    for name in names:
        assert callable(getattr(rpn, name))
        with pytest.raises(NotImplementedError, match="later change"):
            getattr(roi, name)(None)
    targets = [DetectionList3D(torch.arange(56.0).reshape(8, 7), None, {"labels": torch.tensor([5, 4, 1, 5, 2, 4, 6, 2])})]
    boxes, local, rows, counts = rpn.seperate_rpn_assin(targets)
    assert counts == [[3, 1, 4]] and rows[0][2].tolist() == [1, 5, 0, 3] and rpn.targets_groups[3] == counts
    assert rpn.seperate_targets(rpn.targets_groups) is rpn.targets_groups         # a split is passed through
    per_group = rpn.seperate_targets_and_update_labels(targets)
    assert len(per_group) == 3 and len(per_group[0]) == 1
    assert per_group[2][0].get_field("labels").tolist() == [1, 1, 2, 2] and len(per_group[1][0]) == 1
    with pytest.raises(ValueError, match="labels"):
        rpn.seperate_targets([torch.zeros(2, 7)])
    with pytest.raises(TypeError):
        rpn.seperate_rpn_selector(len, None, None, None, None, False)
    with pytest.raises(TypeError):
        rpn.seperate_rpn_loss_evaluator(len, None, None, None, None)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_undecidable_share_of_the_head_cases_stays_under_the_cap():
    """for the reference alone: the seeds the GPU tests use leave far fewer than 1 % of the hidden units within their
    bound of zero (the worst case here: 4 of 24 832)"""
    T = 64
    cases = GR.entry_cases(T) + GR.hidden_cases(T) + GR.determinism_cases(T, 256) + [(64, 4, 3, (70, 0, 9), 9),
                                                                                     (32, 2, 3, (130, 0, 5), 12)]
    worst = 0.0
    for C, A, G, rows, seed in cases:
        p, f, _, _ = GR.make_case(C, A, G, rows, seed)
        und = R.undecided(R.forward(np.concatenate(f), p))
        share = float(und.mean())
        worst = max(worst, share)
        assert share < R.MAX_UNDECIDED, (C, A, G, rows, int(und.sum()), und.size)
    print("worst undecidable share: %.5f" % worst)
