"""Generate tests/golden/solver_golden.npz by IMPORTING the reference's solver package and recording what it computes
(build container only; needs /root/reference):

  * maskrcnn_benchmark/solver/lr_scheduler.py:10-52   WarmupMultiStepLR: the learning rate of every group at every
    iteration
  * maskrcnn_benchmark/solver/build.py:7-35           make_optimizer's (lr, weight_decay) per parameter name and
    make_lr_scheduler's milestones / warm-up length out of the cfg keys

The package imports torch and bisect only and is loaded from where it lies.  The committed fixture is data only: the
cases (a JSON string: the inputs) and the recorded float64 learning rates / tables (the outputs)."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# name -> WarmupMultiStepLR arguments + iterations to record; two groups with the base rates of the reference's rule
SCHEDULES = {
    "linear": dict(milestones=[30, 45], gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=20, warmup_method="linear", iters=60),
    "constant": dict(milestones=[12, 25], gamma=0.1, warmup_factor=0.25, warmup_iters=7, warmup_method="constant", iters=32),
    "no_warmup": dict(milestones=[5, 9], gamma=0.5, warmup_factor=1.0 / 3, warmup_iters=0, warmup_method="linear", iters=14),
    "three_milestones": dict(milestones=[4, 8, 16], gamma=0.3, warmup_factor=0.1, warmup_iters=3, warmup_method="linear",
                             iters=20),
    "milestone_in_warmup": dict(milestones=[6, 40], gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=17,
                                warmup_method="linear", iters=48),
}
BASE_LRS = [0.001, 0.002, 0.0125]
# make_lr_scheduler: cfg keys -> (milestones, warm-up length); the second one runs into the cap of 500
CFGS = {
    "small": dict(Example_num=100, IMS_PER_BATCH=16, LR_STEP_EPOCHS=[3, 5], WARMUP_EPOCHS=0.5, GAMMA=0.1,
                  WARMUP_FACTOR=1.0 / 3, WARMUP_METHOD="linear", iters=40),
    "capped": dict(Example_num=20000, IMS_PER_BATCH=16, LR_STEP_EPOCHS=[30], WARMUP_EPOCHS=0.5, GAMMA=0.1,
                   WARMUP_FACTOR=1.0 / 3, WARMUP_METHOD="linear", iters=8),
    "odd": dict(Example_num=1201, IMS_PER_BATCH=7, LR_STEP_EPOCHS=[0.05, 0.11, 0.2], WARMUP_EPOCHS=0.03, GAMMA=0.2,
                WARMUP_FACTOR=0.5, WARMUP_METHOD="constant", iters=40),
}
NAMES = ["backbone.conv1.weight", "backbone.bn1.weight", "backbone.bn1.bias", "rpn.head.conv.weight",
         "rpn.head.conv.bias", "rpn.head.cls_logits.bias", "roi.fc6.weight", "roi.fc6.bias", "bias_free.scale",
         "unbiased.weight", "frozen.weight"]
FROZEN = ["frozen.weight"]
SOLVER = dict(BASE_LR=0.001, BIAS_LR_FACTOR=2, MOMENTUM=0.9, WEIGHT_DECAY=0.0005, WEIGHT_DECAY_BIAS=0)


def _load_solver():
    d = os.path.join(REF, "maskrcnn_benchmark", "solver")
    spec = importlib.util.spec_from_file_location("ref_solver", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_solver"] = mod
    spec.loader.exec_module(mod)
    return mod


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _optimizer():
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in BASE_LRS]
    return torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(ps, BASE_LRS)], BASE_LRS[-1], momentum=0.9)


def _record(opt, sched, iters):
    rows = []
    for _ in range(iters):
        rows.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()
    return np.array(rows, np.float64)


class _Named(object):
    def __init__(self, names, frozen):
        self.items = [(n, torch.nn.Parameter(torch.zeros(1), requires_grad=n not in frozen)) for n in names]

    def named_parameters(self):
        return iter(self.items)


def main():
    ref = _load_solver()
    out = {"cases": np.array(json.dumps(dict(schedules=SCHEDULES, base_lrs=BASE_LRS, cfgs=CFGS, names=NAMES, frozen=FROZEN,
                                             solver=SOLVER)))}
    for name, c in SCHEDULES.items():
        opt = _optimizer()
        sched = ref.WarmupMultiStepLR(opt, c["milestones"], c["gamma"], warmup_factor=c["warmup_factor"],
                                      warmup_iters=c["warmup_iters"], warmup_method=c["warmup_method"])
        out["sched_" + name] = _record(opt, sched, c["iters"])
    for name, c in CFGS.items():
        cfg = _ns(INPUT=_ns(Example_num=c["Example_num"]),
                  SOLVER=_ns(IMS_PER_BATCH=c["IMS_PER_BATCH"], LR_STEP_EPOCHS=c["LR_STEP_EPOCHS"],
                             WARMUP_EPOCHS=c["WARMUP_EPOCHS"], GAMMA=c["GAMMA"], WARMUP_FACTOR=c["WARMUP_FACTOR"],
                             WARMUP_METHOD=c["WARMUP_METHOD"]))
        opt = _optimizer()
        sched = ref.make_lr_scheduler(cfg, opt)
        out["cfg_%s_milestones" % name] = np.array(list(sched.milestones), np.int64)
        out["cfg_%s_warmup_iters" % name] = np.array(sched.warmup_iters, np.int64)
        out["cfg_%s_lrs" % name] = _record(opt, sched, c["iters"])
    model = _Named(NAMES, FROZEN)
    opt = ref.make_optimizer(_ns(SOLVER=_ns(**SOLVER)), model)
    by_param = {id(g["params"][0]): g for g in opt.param_groups}
    table = [[by_param[id(p)]["lr"], by_param[id(p)]["weight_decay"]] if id(p) in by_param else [np.nan, np.nan]
             for _, p in model.items]
    out["groups_table"] = np.array(table, np.float64)            # row i: (lr, weight_decay) of NAMES[i]; NaN = no group
    out["groups_momentum"] = np.array([g["momentum"] for g in opt.param_groups], np.float64)
    out["groups_default_lr"] = np.array(opt.defaults["lr"], np.float64)
    np.savez_compressed(os.path.join(HERE, "solver_golden.npz"), **out)
    print("wrote solver_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
