"""make_optimizer / make_lr_scheduler (reference: maskrcnn_benchmark/solver/build.py:7-35).  One parameter group per
trainable parameter: a parameter whose name contains "bias" trains at BASE_LR * BIAS_LR_FACTOR with WEIGHT_DECAY_BIAS,
every other one at BASE_LR with WEIGHT_DECAY; momentum SGD over them.  The optimizer returned is solver_glue.FusedSGD:
the same groups and state as torch.optim.SGD, one library launch per step (at most 8 distinct (lr, weight_decay) pairs;
this rule produces two)."""
from .lr_scheduler import WarmupMultiStepLR


def param_groups(cfg, named_parameters):
    """the rule alone, over (name, parameter) pairs: [{"params": [p], "lr": ..., "weight_decay": ...}]"""
    s = cfg.SOLVER
    groups = []
    for name, p in named_parameters:
        if not p.requires_grad:
            continue
        if "bias" in name:
            lr, wd = s.BASE_LR * s.BIAS_LR_FACTOR, s.WEIGHT_DECAY_BIAS
        else:
            lr, wd = s.BASE_LR, s.WEIGHT_DECAY
        groups.append({"params": [p], "lr": lr, "weight_decay": wd})
    return groups


def make_optimizer(cfg, model, flat=None):
    """flat: a dp.FlatParams that already holds the model's parameters (None: the optimizer builds one)"""
    from solver_glue import FusedSGD
    groups = param_groups(cfg, model.named_parameters())
    # the default lr is the last group's, as in the reference's call; every group carries its own anyway
    return FusedSGD(groups, groups[-1]["lr"], momentum=cfg.SOLVER.MOMENTUM, flat=flat)


def schedule_iters(cfg):
    """(milestones, warm-up iterations) in optimizer steps: epochs * examples / examples per step, truncated; the warm-up
    is capped at 500 steps"""
    steps = tuple(int(e * cfg.INPUT.Example_num / cfg.SOLVER.IMS_PER_BATCH) for e in cfg.SOLVER.LR_STEP_EPOCHS)
    warmup = min(int(cfg.SOLVER.WARMUP_EPOCHS * cfg.INPUT.Example_num / cfg.SOLVER.IMS_PER_BATCH), 500)
    return steps, warmup


def make_lr_scheduler(cfg, optimizer):
    steps, warmup = schedule_iters(cfg)
    return WarmupMultiStepLR(optimizer, steps, cfg.SOLVER.GAMMA, warmup_factor=cfg.SOLVER.WARMUP_FACTOR,
                             warmup_iters=warmup, warmup_method=cfg.SOLVER.WARMUP_METHOD)
