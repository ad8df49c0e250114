"""CPU restatement of the box head's loss (FastRCNNLossComputation, maskrcnn_benchmark/modeling/roi_heads/box_head_3d/
loss.py:137-382, the non-separated path; csrc/roi_loss.hip) in numpy / fp64 -- TEST INFRASTRUCTURE ONLY.

Built from what is already pinned: the Matcher's rule on a GIVEN IoU matrix (so that a test can feed it the device's own
matrix and compare decisions exactly), oracle/box_oracle.encode_centroid_box (pinned by tests/golden/box_golden.npz), the
sampler's rule rpn_loss_ref.sample_list (pinned by the sampler's golden test) followed by an ascending sort (nonzero of a
mask, loss.py:279-281), and fp64 formulas for the two losses and their gradients."""
import sys

import numpy as np

import oracle_lib as O
import rpn_loss_ref as RL

sys.path.insert(0, O.ORACLE_DIR)
import box_oracle as BO  # noqa: E402

F = np.float32
BETA = 1.0 / 5                       # loss.py:374
BELOW_LOW_THRESHOLD, BETWEEN_THRESHOLDS = -1, -2


def match(iou, fg_iou, bg_iou):
    """Matcher.__call__ (matcher.py:58-106) with allow_low_quality_matches=False, yaw_diff=None on iou fp32 [G, n]:
    -> (matched_idx int64 [n], matched_val fp32 [n]); the first maximum at ties.  G == 0: all -1 / 0 (the caller's
    no-ground-truth branch, loss.py:200-206).  A NaN entry is the maximum of its column (np.argmax, like torch.max,
    returns the first NaN); both threshold comparisons are false for it, so the proposal stays matched to that box with
    matched_val NaN -- the rule k_roi_match states and follows."""
    iou = np.asarray(iou, F)
    g, n = iou.shape
    if g == 0:
        return np.full(n, -1, np.int64), np.zeros(n, F)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, F)
    idx = np.argmax(iou, axis=0).astype(np.int64)         # numpy: the first occurrence of the maximum
    val = iou[idx, np.arange(n)]
    out = idx.copy()
    out[val < F(bg_iou)] = BELOW_LOW_THRESHOLD
    out[(val >= F(bg_iou)) & (val < F(fg_iou))] = BETWEEN_THRESHOLDS
    return out, val


def labels_of(matched_idx, target_labels):
    """loss.py:213-222: the class of the match, 0 below the low threshold, -1 (ignored) between the thresholds"""
    mi = np.asarray(matched_idx, np.int64)
    tl = np.asarray(target_labels, np.int64)
    if tl.size == 0:
        return np.zeros(mi.shape, np.int64)
    lab = tl[np.maximum(mi, 0)].copy()
    lab[mi == BELOW_LOW_THRESHOLD] = 0
    lab[mi == BETWEEN_THRESHOLDS] = -1
    return lab


def regression_targets(matched_idx, targets, proposals, weights=(1.0,) * 7):
    """loss.py:225-227: encode(target[matched_idx.clamp(min=0)], proposal) for every proposal; zeros without ground truth"""
    p = np.asarray(proposals, F).reshape(-1, 7)
    t = np.asarray(targets, F).reshape(-1, 7)
    if t.shape[0] == 0 or p.shape[0] == 0:
        return np.zeros((p.shape[0], 7), F)
    return BO.encode_centroid_box(t[np.maximum(np.asarray(matched_idx), 0)], p, weights).astype(F)


def sample(labels_per_scene, seed, batch_size_per_image=500, positive_fraction=0.25):
    """per scene (rows ascending, num_pos, num_neg): the sampler's rule over the labels, then nonzero(pos | neg)"""
    out = []
    for p, n in RL.sample_list(labels_per_scene, seed, batch_size_per_image, positive_fraction):
        out.append((np.sort(np.concatenate([p, n]).astype(np.int64)), len(p), len(n)))
    return out


def targets_stage(ious, proposals, targets, target_labels, fg_iou, bg_iou, seed, batch_size_per_image=500,
                  positive_fraction=0.25, weights=(1.0,) * 7):
    """the whole of stage 1 from given IoU matrices: list over scenes of dicts"""
    res = []
    for iou, p, t, tl in zip(ious, proposals, targets, target_labels):
        mi, mv = match(np.asarray(iou, F).reshape(len(t), len(p)), fg_iou, bg_iou)
        res.append({"matched_idx": mi, "matched_val": mv, "labels": labels_of(mi, tl),
                    "regression_targets": regression_targets(mi, t, p, weights)})
    smp = sample([r["labels"] for r in res], seed, batch_size_per_image, positive_fraction)
    for r, (rows, kp, kn), p in zip(res, smp, proposals):
        lab = r["labels"]
        r.update(rows=rows, num_pos=kp, num_neg=kn, P=int((lab >= 1).sum()), N=int((lab == 0).sum()),
                 ignored=int(((lab < 0)).sum()))
    return res


def smooth_l1(d, beta=BETA):
    return np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)


def loss_and_grads(logits, regression, labels, reg_targets, class_specific, beta=BETA):
    """fp64: F.cross_entropy(logits, labels) (mean) and loss.py:343-377; rows whose label is outside [0, C) add nothing
    and get zero gradients (this project's rule; torch raises there).  Returns (cls, box, d logits, d regression, the
    per-row cross-entropy terms, the per-row box terms) for unit upstream gradients."""
    x = np.asarray(logits, np.float64)
    r = np.asarray(regression, np.float64)
    t = np.asarray(reg_targets, np.float64).reshape(-1, 7)
    lab = np.asarray(labels, np.int64)
    n, c = x.shape
    ok = (lab >= 0) & (lab < c)
    l_ = np.where(ok, lab, 0)
    m = x.max(1, keepdims=True) if n else x[:, :1]
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    prob = e / s
    rows = np.arange(n)
    ce = np.where(ok, (m[:, 0] + np.log(s[:, 0])) - x[rows, l_], 0.0)
    pos = ok & (lab > 0)
    cols = (7 * l_[:, None] if class_specific else np.zeros((n, 1), np.int64)) + np.arange(7)[None]
    diff = np.where(pos[:, None], r[rows[:, None], cols] - t, 0.0) if n else np.zeros((0, 7))
    bx = smooth_l1(np.abs(diff), beta).sum(1) * pos
    g_x = np.zeros_like(x)
    g_r = np.zeros_like(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        cls, box = ce.sum() / n if n else np.nan, bx.sum() / n if n else np.nan
    if n:
        onehot = np.zeros_like(x)
        onehot[rows, l_] = 1.0
        g_x = np.where(ok[:, None], (prob - onehot) / n, 0.0)
        h = np.where(np.abs(diff) < beta, diff / beta, np.sign(diff)) / n
        np.put_along_axis(g_r, cols, np.where(pos[:, None], h, 0.0), axis=1)
        # (rows that are not positive put zeros into columns 0..6 or 7 l..: zeros over zeros)
    return cls, box, g_x, g_r, ce, bx
