"""The RPN loss without a GPU: the numpy restatement (tests/rpn_loss_ref.py) of the selection rule and the loss against the
reference's own smooth_l1_loss / sampler counts (tests/golden/rpn_loss_golden.npz, tests/golden/gen_rpn_loss_golden.py),
the uniformity of the rule, and the C ABI / Python surface of the feature."""
import os
import re

import numpy as np
import pytest

import rpn_loss_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_loss_matches_reference_composition(golden_dir):
    """loss_3d.py:238-249 with the reference's smooth_l1_loss and autograd (fixture) == the restatement, 1e-6 relative"""
    g = np.load(os.path.join(golden_dir, "rpn_loss_golden.npz"))
    pos = np.nonzero(g["pos_mask"])[0]
    neg = np.nonzero(g["neg_mask"])[0]
    assert (g["labels"][pos] == 1).all() and (g["labels"][neg] == 0).all() and len(pos) + len(neg) == 256
    bce, box, d_obj, d_reg = R.loss_and_grads(g["obj"], g["reg"], g["tgt"], pos, neg)
    np.testing.assert_allclose(bce, g["obj_loss"], rtol=1e-6)
    np.testing.assert_allclose(box, g["box_loss"], rtol=1e-6)
    np.testing.assert_allclose(d_obj, g["grad_obj"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(d_reg, g["grad_reg"], rtol=1e-6, atol=1e-12)
    assert (d_reg[np.setdiff1d(np.arange(len(d_reg)), pos)] == 0).all()
    # the list form: mean / sum, and 'Diff_3' is the same as 'Diff' (the weight is parsed, never applied)
    d = np.abs(g["l1_input"].astype(np.float64) - g["l1_target"])
    np.testing.assert_allclose(R.smooth_l1(d, 1.0 / 9).mean(), g["l1_mean"], rtol=1e-6)
    np.testing.assert_allclose(R.smooth_l1(d, 1.0 / 9).sum(), g["l1_sum"], rtol=1e-6)
    assert g["l1_sum_diff3"] == g["l1_sum"]


def test_restated_counts_match_reference_sampler(golden_dir):
    """num_pos = min(P, 128), num_neg = min(N, 256 - num_pos): the reference sampler's counts (fixture) exactly, for label
    vectors with many / few / no positives or negatives, through the list-form rule"""
    g = np.load(os.path.join(golden_dir, "rpn_loss_golden.npz"))
    vecs = np.split(g["count_vecs"], np.cumsum(g["count_vec_len"])[:-1])
    got = R.sample_list(vecs, seed=5)
    for v, (p, n), want in zip(vecs, got, g["counts"]):
        assert [len(p), len(n)] == want.tolist()
        assert (v[p] >= 1).all() and (v[n] == 0).all() and len(set(p.tolist())) == len(p)
        assert R.counts(int((v >= 1).sum()), int((v == 0).sum())) == tuple(want.tolist())
    assert {tuple(c) for c in g["counts"].tolist()} >= {(128, 128), (0, 250), (128, 0), (30, 20), (0, 0)}


def test_selection_rule_is_uniform():
    """400 seeds on a vector of 500 positives (and 500 negatives), 128 drawn per seed: every entry's selection count is
    Binomial(400, 128/500); all 500 stay within 5.5 standard deviations, and the mean is exact"""
    lab = np.concatenate([np.ones(500), np.zeros(500)])
    hits = np.zeros(1000, np.int64)
    for seed in range(400):
        p, n = R.sample_list([lab], seed)[0]
        assert len(p) == 128 and len(n) == 128
        hits[p] += 1
        hits[n] += 1
    q = 128 / 500.0
    mu, sd = 400 * q, np.sqrt(400 * q * (1 - q))
    assert hits[:500].sum() == hits[500:].sum() == 400 * 128
    assert np.abs(hits - mu).max() < 5.5 * sd, (hits.min(), hits.max(), mu, sd)
    # different examples of one call draw independently: example 1's sample differs from example 0's
    s = R.sample_list([lab, lab], 3)
    assert set(s[0][0].tolist()) != set(s[1][0].tolist())


def test_selection_is_independent_of_row_order():
    """the maps-form key and tie-break use (map, x, y, z, a) only: permuting an example's sites changes the label indices
    but not the selected anchors"""
    rng = np.random.default_rng(4)
    A = 4
    c0 = np.unique(rng.integers(0, 60, (900, 3)), axis=0)[:700]
    coords = [np.column_stack([c0, np.zeros(len(c0), np.int64)])]
    lab = rng.choice([0, -1, -2], len(c0) * A, p=[0.2, 0.7, 0.1]).astype(np.int64)
    perm = rng.permutation(len(c0))
    coords_p = [coords[0][perm]]
    lab_p = lab.reshape(-1, A)[perm].reshape(-1)
    for seed in (0, 1, 77):
        (p, n), = R.sample_maps(coords, [[len(c0)]], A, [lab], seed)
        (pp, nn), = R.sample_maps(coords_p, [[len(c0)]], A, [lab_p], seed)
        an = R.example_anchors(coords, [[len(c0)]], 0, A)
        anp = R.example_anchors(coords_p, [[len(c0)]], 0, A)
        assert len(p) == 128 and len(n) == 128
        assert an[p].tolist() == anp[pp].tolist() and an[n].tolist() == anp[nn].tolist()


def test_header_and_binding_declare_the_loss_entries():
    """the new entry points are declared in include/aabr_hip.h and bound in _hip._SIGS (the exports test then resolves them
    in the built library), with the ABI version bumped in both"""
    import _hip
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    for name in ("aabr_rpn_loss_scratch_words", "aabr_rpn_loss_forward", "aabr_rpn_loss_backward", "aabr_sample_list",
                 "aabr_smooth_l1_scratch_floats", "aabr_smooth_l1_forward", "aabr_smooth_l1_backward"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _hip._SIGS, name
    ver = int(re.search(r"#define AABR_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _hip.ABI_VERSION and ver >= 610


def test_python_surface():
    """rpn_glue.rpn_loss, the reference-named smooth_l1_loss / BalancedPositiveNegativeSampler, and SinDiff refused"""
    import rpn_glue
    from maskrcnn_benchmark.layers import smooth_l1_loss  # noqa: F401
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    assert callable(rpn_glue.rpn_loss)
    s = BalancedPositiveNegativeSampler(256, 0.5)
    assert s.batch_size_per_image == 256 and s.positive_fraction == 0.5 and s.seed is None
    assert rpn_glue.parse_yaw_loss_mode("Diff") == rpn_glue.parse_yaw_loss_mode("Diff_2.5") == "Diff"
    for bad in ("SinDiff", "SinDiff_1", "Abs"):
        with pytest.raises(ValueError):
            rpn_glue.parse_yaw_loss_mode(bad)
