"""The RPN loss on the device (rpn_glue.rpn_loss, csrc/rpn_loss.hip): the sample against the numpy restatement of the
selection rule (tests/rpn_loss_ref.py), the losses and gradients against torch autograd of the reference's composition
(modeling/rpn/loss_3d.py:238-249) on that sample, edge cases, determinism, no host sync, the bench's size, and the
reference-named list forms against tests/golden/rpn_loss_golden.npz."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_yardstick as Y
import rpn_loss_ref as R
import synth_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABEL_AUG = {"target_Y": 0.4, "anchor_Y": 0.0, "target_Z": 0.8, "anchor_Z": 0.0}   # config/defaults.py:161-162
YAWS = (0, -1.57, -0.785, 0.785)
SIZES = [[0.4, 1.5, 1.5], [1.5, 1.5, 1.0], [4, 4, 1.5], [0.2, 0.5, 3], [0.4, 1.5, 3], [0.6, 2.5, 3]]
STRIDES = [[2.0 ** s] * 3 for s in (5, 6, 7)] + [[2.0 ** s] * 3 for s in (4, 5, 6)]
BASE = [torch.tensor([[0.0, 0.0, 0.0] + list(s) + [y] for y in YAWS], dtype=torch.float32) for s in SIZES]
A = len(YAWS)
BETA = 1.0 / 9


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _scene(nb, npts, seed, vs, gts, order):
    """the default FPN_Net's six RPN maps of a synthetic batch in `order`, and rpn_label_matches(regression_targets=True)"""
    import rpn_glue
    from test_cabi_and_host import default_fpn
    torch.manual_seed(1)
    net = default_fpn().to(DEV)
    net.set_site_order(order)
    locs, feats = S.make_batch(nb, npts, seed, vs)
    with torch.no_grad():
        maps, _ = net([_t(locs), _t(feats)])
    labels = rpn_glue.rpn_label_matches(maps, BASE, STRIDES, float(vs), [_t(g) for g in gts], LABEL_AUG, 6,
                                        regression_targets=True)
    coords = [m.get_spatial_locations().numpy() for m in maps]
    counts = [[int((c[:, 3] == b).sum()) for b in range(nb)] for c in coords]
    return maps, labels, coords, counts


def _head(counts, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    obj = [(torch.randn(sum(c) * A, generator=g) * 2).to(DEV, dtype).requires_grad_() for c in counts]
    reg = [(torch.randn(sum(c) * A, 7, generator=g) * 0.3).to(DEV, dtype).requires_grad_() for c in counts]
    return obj, reg


def _reference(obj, reg, labels, counts, samples):
    """torch autograd (float64, CPU) of loss_3d.py:238-249 on the given sample over example-major concatenations;
    returns losses and per-map gradients"""
    n_maps, nb = len(obj), len(labels)
    ob = [o.detach().double().cpu().requires_grad_() for o in obj]
    rb = [r.detach().double().cpu().requires_grad_() for r in reg]
    O, Rg, T, pos, neg, s0, base = [], [], [], [], [], [0] * n_maps, 0
    for b in range(nb):
        for m in range(n_maps):
            c = counts[m][b]
            O.append(ob[m][s0[m] * A:(s0[m] + c) * A])
            Rg.append(rb[m][s0[m] * A:(s0[m] + c) * A])
            s0[m] += c
        T.append(labels[b][3].double().cpu())
        pos.append(torch.as_tensor(samples[b][0] + base))
        neg.append(torch.as_tensor(samples[b][1] + base))
        base += labels[b][0].numel()
    O, Rg, T = torch.cat(O), torch.cat(Rg), torch.cat(T)
    pos, neg = torch.cat(pos).long(), torch.cat(neg).long()
    sampled = torch.cat([pos, neg])
    y = torch.cat([torch.ones(len(pos)), torch.zeros(len(neg))]).double()
    d = torch.abs(Rg[pos] - T[pos])
    box = torch.where(d < BETA, 0.5 * d ** 2 / BETA, d - 0.5 * BETA).sum() / sampled.numel()
    objl = F.binary_cross_entropy_with_logits(O[sampled], y)
    (objl + box).backward()
    return objl.item(), box.item(), [o.grad.numpy() for o in ob], [r.grad.numpy() for r in rb]


def _grad_slack(obj, g_obj, g_reg, ns):
    """per-element bound on how far k_loss_backward's fp32 formulas (csrc/rpn_loss.hip) may move a gradient from its
    fp64 value, u = 2^-24, g = 1 / N_s (fl(1 / N_s): u):
    objectness (sigmoid(x) - y) g: expf <= 2 ulp (4u) -> 1 + e: + u -> 1 / (1 + e) (correctly rounded): 6u sigma;
    - y: + u |sigma - y|; * g: + 2u |sigma - y|  =>  u g (6 sigma + 3 |sigma - y|), where |sigma - y| g = |grad|;
    regression h(pred - target) g, h = diff / beta or sign(diff): fl(diff) u, beta = fl(1/9) u, the division u,
    g u, the product u  =>  5u |grad| (a branch taken the other way at |diff| within rounding of beta moves h by <= 2u).
    Zero where the exact gradient is zero (anchors outside the sample, diff == 0): those stores must be exactly 0."""
    u = 2.0 ** -24
    x = obj.detach().double().cpu().numpy()
    sig = 1.0 / (1.0 + np.exp(-x))
    so = np.where(g_obj != 0, u * (6 * sig / ns + 3 * np.abs(g_obj)), 0.0)
    return so, 5 * u * np.abs(g_reg)


def _check_sample(sel, labels, samples, B=256):
    base = 0
    for b, (p, n) in enumerate(samples):
        lab = labels[b][0].cpu().numpy()
        P, N = int((lab >= 0).sum()), int((lab == -1).sum())
        assert (len(p), len(n)) == R.counts(P, N)
        row = sel[b].cpu().numpy()
        np.testing.assert_array_equal(row[:len(p)], p + base)
        np.testing.assert_array_equal(row[len(p):len(p) + len(n)], n + base)
        assert (row[len(p) + len(n):] == -1).all()
        assert (lab[p] >= 0).all() and (lab[n] == -1).all()          # ignored (-2) anchors are never sampled
        base += lab.size


def _run(maps, obj, reg, labels, seed, **kw):
    import rpn_glue
    lo, lb, sel = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, seed=seed, return_samples=True, **kw)
    for t in obj + reg:
        t.grad = None
    (lo + lb).backward()
    return lo, lb, sel


def test_rpn_loss_vs_restatement_both_site_orders():
    """2 scenes through the default FPN_Net's six maps, first-seen and brick-major rows: the selected anchors bit-equal to
    the restatement, the same (map, x, y, z, a) set in both orders, counts min(P, 128) / min(N, 256 - num_pos), and the
    losses and gradients of torch autograd of the reference composition on that sample -- fp32 rtol 1e-5; bf16 inputs:
    losses rtol 1e-5 (fp32 arithmetic on the same bf16 values), every stored gradient the round-to-nearest-even bf16 of
    a value within the slack of the kernel's elementwise fp32 formulas (_grad_slack) of the fp64 autograd result"""
    gts = [S.make_gt_boxes(25, 8), np.zeros((0, 7), np.float32)]     # example 1 without ground truth: all negatives
    chosen = {}
    for order in ("first_seen", "brick"):
        maps, labels, coords, counts = _scene(2, 30000, 41, 20, gts, order)
        samples = R.sample_maps(coords, counts, A, [l[0].cpu().numpy() for l in labels], 1234)
        # (the low-quality pass of the matcher leaves few negatives in a scene with ground truth, matcher.py:126-128)
        assert len(samples[0][0]) == 128 and (len(samples[1][0]), len(samples[1][1])) == (0, 256)
        for dtype in (torch.float32, torch.bfloat16):
            obj, reg = _head(counts, dtype, 5)
            lo, lb, sel = _run(maps, obj, reg, labels, 1234)
            assert lo.dtype == lb.dtype == torch.float32 and lo.dim() == lb.dim() == 0
            _check_sample(sel, labels, samples)
            ro, rbx, go, gr = _reference(obj, reg, labels, counts, samples)
            np.testing.assert_allclose(lo.item(), ro, rtol=1e-5)
            np.testing.assert_allclose(lb.item(), rbx, rtol=1e-5)
            ns = sum(len(p) + len(n) for p, n in samples)
            for m in range(len(obj)):
                assert obj[m].grad.dtype == dtype and reg[m].grad.dtype == dtype
                if dtype == torch.float32:
                    np.testing.assert_allclose(obj[m].grad.float().cpu().numpy(), go[m], rtol=1e-5, atol=1e-9)
                    np.testing.assert_allclose(reg[m].grad.float().cpu().numpy(), gr[m], rtol=1e-5, atol=1e-9)
                    continue
                so, sr = _grad_slack(obj[m], go[m], gr[m], ns)
                Y.assert_bf16_rounded(obj[m].grad, go[m], so, "objectness gradient, map %d" % m)
                Y.assert_bf16_rounded(reg[m].grad, gr[m], sr, "regression gradient, map %d" % m)
        chosen[order] = [sorted(map(tuple, R.example_anchors(coords, counts, b, A)[np.concatenate(s)].tolist()))
                         for b, s in enumerate(samples)]
    assert chosen["first_seen"] == chosen["brick"]


def test_rpn_loss_edge_cases():
    """an example without ground truth (all negatives), fewer than 128 positives and fewer negatives than asked for
    (synthetic labels on the same anchors: 10 / 50), N_s == 0 (NaN losses, zero gradients), and 'SinDiff' refused"""
    import rpn_glue
    gts = [S.make_gt_boxes(25, 8), np.zeros((0, 7), np.float32)]
    maps, labels, coords, counts = _scene(2, 30000, 41, 20, gts, "brick")
    lab1 = labels[1][0].cpu().numpy()
    assert (lab1 == -1).all()
    lab0 = labels[0][0].cpu().numpy()
    # synthetic label vectors on the same anchors: 10 positives + 50 negatives in example 0 (fewer than 246 negatives)
    rng = np.random.default_rng(3)
    few = np.full(lab0.size, -2, np.int64)
    idx = rng.permutation(lab0.size)
    few[idx[:10]] = 0
    few[idx[10:60]] = -1
    cases = {"real": labels,
             "few": [(_t(few),) + tuple(labels[0][1:]), labels[1]],
             "empty": [(torch.full_like(l[0], -2),) + tuple(l[1:]) for l in labels]}
    obj, reg = _head(counts, torch.float32, 6)
    for name, labs in cases.items():
        samples = R.sample_maps(coords, counts, A, [l[0].cpu().numpy() for l in labs], 99)
        lo, lb, sel = _run(maps, obj, reg, labs, 99)
        _check_sample(sel, labs, samples)
        if name == "real":
            assert len(samples[1][0]) == 0 and len(samples[1][1]) == 256           # no ground truth: all negatives
            P0 = int((lab0 >= 0).sum())
            assert len(samples[0][0]) == min(P0, 128)
        if name == "few":
            assert (len(samples[0][0]), len(samples[0][1])) == (10, 50)
        if name == "empty":
            assert np.isnan(lo.item()) and np.isnan(lb.item())
            assert all((t.grad == 0).all().item() for t in obj + reg)
            continue
        ro, rbx, go, gr = _reference(obj, reg, labs, counts, samples)
        np.testing.assert_allclose([lo.item(), lb.item()], [ro, rbx], rtol=1e-5)
        for m in range(len(obj)):
            np.testing.assert_allclose(obj[m].grad.cpu().numpy(), go[m], rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(reg[m].grad.cpu().numpy(), gr[m], rtol=1e-5, atol=1e-9)
    for mode in ("SinDiff", "SinDiff_2"):
        with pytest.raises(ValueError):
            rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, yaw_loss_mode=mode)
    lo3, lb3 = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, yaw_loss_mode="Diff_3", seed=99)
    lo4, lb4 = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, seed=99)
    assert torch.equal(lo3, lo4) and torch.equal(lb3, lb4)


def test_rpn_loss_determinism_and_no_host_sync():
    """the same seed: bit-identical losses and gradients; another seed: another sample; seed=None follows
    torch.manual_seed; forward and backward under torch.cuda.set_sync_debug_mode('error')"""
    import rpn_glue
    gts = [S.make_gt_boxes(25, 8), S.make_gt_boxes(3, 9)]
    maps, labels, coords, counts = _scene(2, 30000, 41, 20, gts, "brick")
    obj, reg = _head(counts, torch.float32, 8)
    runs = []
    for seed in (7, 7, 8):
        lo, lb, sel = _run(maps, obj, reg, labels, seed)
        runs.append((lo.clone(), lb.clone(), sel.clone(), [t.grad.clone() for t in obj + reg]))
    a, b, c = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    assert not torch.equal(a[2], c[2])
    torch.manual_seed(11)
    s1 = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, return_samples=True)[2]
    torch.manual_seed(11)
    s2 = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE, return_samples=True)[2]
    assert torch.equal(s1, s2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lo, lb = rpn_glue.rpn_loss(maps, obj, reg, labels, BASE)
        (lo + 2 * lb).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rpn_loss_at_bench_size(dtype):
    """BASELINE configs[2] size: 4 scenes x S80k @ 2 cm, 40 ground-truth walls each, brick-major rows: the sample is the
    restatement's, every example with enough anchors draws 256 (here every scene's anchors are all matched by the
    low-quality pass: 128 positives, no negatives), the losses match the reference composition (rtol 1e-5)"""
    gts = [S.make_gt_boxes(40, 7000 + i) for i in range(4)]
    maps, labels, coords, counts = _scene(4, 80000, 9000, 50, gts, "brick")
    obj, reg = _head(counts, dtype, 9)
    samples = R.sample_maps(coords, counts, A, [l[0].cpu().numpy() for l in labels], 2024)
    lo, lb, sel = _run(maps, obj, reg, labels, 2024)
    _check_sample(sel, labels, samples)
    for b, (p, n) in enumerate(samples):
        lab = labels[b][0].cpu().numpy()
        kp = min(int((lab >= 0).sum()), 128)
        if int((lab == -1).sum()) >= 256 - kp:
            assert len(p) + len(n) == 256
    assert all(len(p) == 128 for p, _ in samples)
    ro, rbx, go, gr = _reference(obj, reg, labels, counts, samples)
    np.testing.assert_allclose([lo.item(), lb.item()], [ro, rbx], rtol=1e-5)
    rt = 1e-5 if dtype == torch.float32 else 1e-2
    for m in range(len(obj)):
        np.testing.assert_allclose(obj[m].grad.float().cpu().numpy(), go[m], rtol=rt, atol=1e-7)


def test_list_forms_vs_reference_fixture(golden_dir):
    """maskrcnn_benchmark.layers.smooth_l1_loss (mean, sum, 'Diff_3', gradient; fp32 and bf16 input) and
    BalancedPositiveNegativeSampler (counts of the reference sampler, masks = the restatement's sample, > 16 vectors in one
    call) against tests/golden/rpn_loss_golden.npz"""
    from maskrcnn_benchmark.layers import smooth_l1_loss
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    g = np.load(os.path.join(golden_dir, "rpn_loss_golden.npz"))
    x = _t(g["l1_input"]).requires_grad_()
    tg, an = _t(g["l1_target"]), torch.zeros(g["l1_input"].shape, device=DEV)
    mean = smooth_l1_loss(x, tg, an)
    mean.backward()
    np.testing.assert_allclose(mean.item(), g["l1_mean"], rtol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), g["l1_mean_grad"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(smooth_l1_loss(x, tg, an, size_average=False).item(), g["l1_sum"], rtol=1e-5)
    np.testing.assert_allclose(smooth_l1_loss(x, tg, an, size_average=False, yaw_loss_mode="Diff_3").item(),
                               g["l1_sum_diff3"], rtol=1e-5)
    xb = x.detach().bfloat16()
    want_b = R.smooth_l1(np.abs(xb.float().cpu().numpy().astype(np.float64) - g["l1_target"]), BETA).sum()
    np.testing.assert_allclose(smooth_l1_loss(xb, tg, an, size_average=False).item(), want_b, rtol=1e-5)
    with pytest.raises(ValueError):
        smooth_l1_loss(x, tg, an, yaw_loss_mode="SinDiff")
    vecs = np.split(g["count_vecs"], np.cumsum(g["count_vec_len"])[:-1])
    vecs = (vecs * 3)[:20]
    sampler = BalancedPositiveNegativeSampler(256, 0.5)
    sampler.seed = 5
    pos, neg = sampler([_t(v) for v in vecs])
    want = R.sample_list(vecs, 5)
    for i, (v, pm, nm, (p, n)) in enumerate(zip(vecs, pos, neg, want)):
        assert pm.dtype == nm.dtype == torch.uint8 and pm.shape == nm.shape == v.shape
        assert [int(pm.sum()), int(nm.sum())] == g["counts"][i % 8].tolist()
        np.testing.assert_array_equal(np.nonzero(pm.cpu().numpy())[0], np.sort(p))
        np.testing.assert_array_equal(np.nonzero(nm.cpu().numpy())[0], np.sort(n))
