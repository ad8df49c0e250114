"""reference: maskrcnn_benchmark/solver/__init__.py -- the optimizer and its learning-rate schedule.  The optimizer is
solver_glue.FusedSGD (csrc/solver.hip: one launch per step), the schedule is host arithmetic."""
from .build import make_lr_scheduler, make_optimizer
from .lr_scheduler import WarmupMultiStepLR

__all__ = ["make_optimizer", "make_lr_scheduler", "WarmupMultiStepLR"]
