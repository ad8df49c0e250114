"""WarmupMultiStepLR (reference: maskrcnn_benchmark/solver/lr_scheduler.py:10-52): every group's base learning rate times
gamma ** (milestones at or before this iteration), and during the first `warmup_iters` iterations also times a warm-up
factor -- the constant `warmup_factor`, or ("linear") the line from `warmup_factor` at iteration 0 to 1 at
`warmup_iters`.  Host arithmetic in float64, in the order  base_lr * warm-up * gamma ** k;  the values land in
`optimizer.param_groups[i]["lr"]`, where solver_glue.FusedSGD reads them at its next step."""
import bisect

import torch


class WarmupMultiStepLR(torch.optim.lr_scheduler.LRScheduler):
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method="linear",
                 last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        if warmup_method not in ("constant", "linear"):
            raise ValueError("Only 'constant' or 'linear' warmup_method accepted, got {}".format(warmup_method))
        self.milestones = milestones
        self.gamma = gamma
        self.warmup_factor = warmup_factor
        self.warmup_iters = warmup_iters
        self.warmup_method = warmup_method
        super().__init__(optimizer, last_epoch)

    def _warmup(self):
        it = self.last_epoch
        if it >= self.warmup_iters:
            return 1
        if self.warmup_method == "constant":
            return self.warmup_factor
        alpha = it / self.warmup_iters
        return self.warmup_factor * (1 - alpha) + alpha

    def get_lr(self):
        w = self._warmup()
        decay = self.gamma ** bisect.bisect_right(self.milestones, self.last_epoch)
        return [base_lr * w * decay for base_lr in self.base_lrs]
