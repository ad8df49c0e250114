"""Generate tests/golden/rpn_loss_golden.npz by IMPORTING the reference's RPN-loss pieces and running them on seeded
inputs (build container only; needs /root/reference):

  * maskrcnn_benchmark/layers/smooth_l1_loss.py:34-52    smooth_l1_loss (yaw mode 'Diff'; it imports
    utils3d/geometric_torch.py, loaded from the reference tree)
  * maskrcnn_benchmark/modeling/balanced_positive_negative_sampler.py:19-68   the sampler's num_pos / num_neg (the
    counts are deterministic; its randperm subset is not, so only the counts are recorded)
  * the loss composition of RPNLossComputation.__call__ (modeling/rpn/loss_3d.py:238-249): box loss =
    smooth_l1_loss(box_regression[pos], regression_targets[pos], anchors, beta=1/9, size_average=False) / N_s,
    objectness loss = F.binary_cross_entropy_with_logits(objectness[sampled], labels[sampled]), and torch autograd of
    both on fixed sample masks.

The committed fixture is data only: inputs, masks, losses, gradients, label vectors and counts."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, REF)          # smooth_l1_loss.py: `from utils3d.geometric_torch import limit_period`
    sl1 = _load("ref_smooth_l1_loss", "maskrcnn_benchmark/layers/smooth_l1_loss.py")
    smp = _load("ref_sampler", "maskrcnn_benchmark/modeling/balanced_positive_negative_sampler.py")
    rng = np.random.default_rng(31)
    out = {}
    # ---------------------------------------------------------------- the loss composition on fixed masks
    n = 3000
    obj = (rng.standard_normal(n) * 3).astype(np.float32)
    reg = (rng.standard_normal((n, 7)) * 0.3).astype(np.float32)
    tgt = (rng.standard_normal((n, 7)) * 0.3).astype(np.float32)
    tgt[:50] = reg[:50] + (rng.standard_normal((50, 7)) * 0.02).astype(np.float32)   # both smooth-L1 branches
    labels = rng.choice([1.0, 0.0, -1.0], n, p=[0.1, 0.8, 0.1]).astype(np.float32)
    pos = np.nonzero(labels == 1)[0]
    neg = np.nonzero(labels == 0)[0]
    pos = rng.permutation(pos)[:128]
    neg = rng.permutation(neg)[:256 - len(pos)]
    pos_mask = np.zeros(n, np.uint8)
    neg_mask = np.zeros(n, np.uint8)
    pos_mask[pos] = 1
    neg_mask[neg] = 1
    o = torch.from_numpy(obj).double().requires_grad_()
    r = torch.from_numpy(reg).double().requires_grad_()
    t = torch.from_numpy(tgt).double()
    lab = torch.from_numpy(labels).double()
    sp = torch.nonzero(torch.from_numpy(pos_mask)).squeeze(1)
    sn = torch.nonzero(torch.from_numpy(neg_mask)).squeeze(1)
    sampled = torch.cat([sp, sn], 0)
    anchors = torch.zeros((n, 7), dtype=torch.float64)
    box = sl1.smooth_l1_loss(r[sp], t[sp], anchors[sp], beta=1.0 / 9, size_average=False,
                             yaw_loss_mode="Diff") / sampled.numel()
    objl = F.binary_cross_entropy_with_logits(o[sampled], lab[sampled])
    (objl + box).backward()
    out.update(obj=obj, reg=reg, tgt=tgt, labels=labels, pos_mask=pos_mask, neg_mask=neg_mask,
               obj_loss=np.float64(objl.item()), box_loss=np.float64(box.item()), grad_obj=o.grad.numpy(),
               grad_reg=r.grad.numpy())
    # the list form: smooth_l1_loss on [m, 7], mean and sum, and 'Diff_3' (weight parsed, not applied)
    m = 200
    a = (rng.standard_normal((m, 7)) * 0.2).astype(np.float32)
    b = (rng.standard_normal((m, 7)) * 0.2).astype(np.float32)
    ta = torch.from_numpy(a).double().requires_grad_()
    mean = sl1.smooth_l1_loss(ta, torch.from_numpy(b).double(), torch.zeros((m, 7), dtype=torch.float64))
    mean.backward()
    out.update(l1_input=a, l1_target=b, l1_mean=np.float64(mean.item()), l1_mean_grad=ta.grad.numpy(),
               l1_sum=np.float64(sl1.smooth_l1_loss(torch.from_numpy(a).double(), torch.from_numpy(b).double(),
                                                    torch.zeros((m, 7)), size_average=False).item()),
               l1_sum_diff3=np.float64(sl1.smooth_l1_loss(torch.from_numpy(a).double(), torch.from_numpy(b).double(),
                                                          torch.zeros((m, 7)), size_average=False,
                                                          yaw_loss_mode="Diff_3").item()))
    # ---------------------------------------------------------------- sampler counts (B = 256, f = 0.5)
    cases = [(5000, 600, 4000), (5000, 40, 4000), (300, 0, 250), (300, 250, 0), (100, 30, 20), (50, 0, 0),
             (2000, 128, 128), (2000, 129, 2)]
    sampler = smp.BalancedPositiveNegativeSampler(256, 0.5)
    vecs, counts = [], []
    for i, (nn, P, N) in enumerate(cases):
        v = np.full(nn, -1.0, np.float32)
        perm = rng.permutation(nn)
        v[perm[:P]] = 1.0
        v[perm[P:P + N]] = 0.0
        pm, nm = sampler([torch.from_numpy(v)])
        vecs.append(v)
        counts.append([int(pm[0].sum()), int(nm[0].sum())])
    out["count_vec_len"] = np.array([len(v) for v in vecs], np.int64)
    out["count_vecs"] = np.concatenate(vecs)
    out["counts"] = np.array(counts, np.int64)
    np.savez_compressed(os.path.join(HERE, "rpn_loss_golden.npz"), **out)
    print("wrote rpn_loss_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
