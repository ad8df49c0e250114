"""reference: maskrcnn_benchmark/modeling/balanced_positive_negative_sampler.py:5-68 on the library's list-form sampler
(include/aabr_hip.h aabr_sample_list): the same counts, num_pos = min(P, int(B * f)) and num_neg = min(N, B - num_pos), and
a uniform random subset of each class -- the one of the header's selection rule (a hash of (seed, example, index), the
smallest keys) instead of torch.randperm, with no nonzero / host read."""
import torch

import _hip
from _hip import check, ptr, stream


class BalancedPositiveNegativeSampler(object):
    """
    This class samples batches, ensuring that they contain a fixed proportion of positives
    """

    def __init__(self, batch_size_per_image, positive_fraction):
        """
        Arguments:
            batch_size_per_image (int): number of elements to be selected per image (<= 512)
            positive_fraction (float): percentace of positive elements per batch
        `seed` (attribute, extension): None draws one seed per call from torch's default CPU generator
        """
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.seed = None

    def __call__(self, matched_idxs):
        """
        Arguments:
            matched idxs: list of device tensors containing -1, 0 or positive values, one per image.
                -1 values are ignored, 0 are considered as negatives and > 0 (>= 1) as positives.

        Returns:
            pos_idx (list[tensor])
            neg_idx (list[tensor])

        Two lists of uint8 masks, one per image: the positives and the negatives selected.
        """
        from rpn_glue import draw_seed
        lib = _hip.load()
        nb = len(matched_idxs)
        if nb == 0:
            return [], []
        for m in matched_idxs:
            _hip.require_gpu(m)
        # the sampler's classes as int64 1 / 0 / -1 (a fractional label is neither `>= 1` nor `== 0`: ignored)
        lab = [torch.where(m >= 1, 1, torch.where(m == 0, 0, -1)).to(torch.int64).reshape(-1) for m in matched_idxs]
        pos = [torch.zeros_like(m, dtype=torch.uint8) for m in matched_idxs]
        neg = [torch.zeros_like(m, dtype=torch.uint8) for m in matched_idxs]
        dev = lab[0].device
        B = int(self.batch_size_per_image)
        sel = torch.empty((nb, B), dtype=torch.int64, device=dev)
        info = torch.empty((nb, 8), dtype=torch.int32, device=dev)
        scr = _hip.workspace("sampler", int(lib.aabr_rpn_loss_scratch_words(nb)) + 2, torch.int32, dev)
        so = (-scr.data_ptr() // 4) % 2
        seed = draw_seed() if self.seed is None else int(self.seed)
        check(lib.aabr_sample_list(nb, _hip.ptrs(lab), _hip.i64xn([l.numel() for l in lab]), seed & 0xffffffff, B,
                                   int(B * self.positive_fraction), ptr(sel), ptr(info), _hip.ptrs(pos), _hip.ptrs(neg),
                                   scr.data_ptr() + 4 * so, stream()))
        return pos, neg
