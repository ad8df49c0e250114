"""The solver without a GPU: the chunk cutter (csrc/solver_segs.h) against a brute-force enumeration of (segment, element)
and as a stand-alone program under the host sanitizers; the step entry's refusals before any launch; the yardsticks of the
GPU tests (tests/solver_ref.py and CPU torch.optim.SGD inside the first-order bounds of the float64 step); and the
schedule / parameter-group rule against results recorded from the reference (tests/golden/solver_golden.npz)."""
import ctypes as C
import json
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import solver_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW_SYMBOLS = ("aabr_sgd_chunk_elems", "aabr_sgd_chunk_table", "aabr_sgd_momentum_step")


def _sizes(chunk):
    """0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 3, in an order whose back-to-back packing starts segments at
    every phase of the flat offset, whatever the first offset"""
    return [0, 1, 5, 4, 1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 0, 5, 3, 4, 2 * chunk + 3, chunk + 1, chunk,
            chunk - 1, 0]


# ---- 1. chunk table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_chunk_table_against_enumeration(first):
    import solver_glue
    chunk = solver_glue.chunk_elems()
    assert chunk >= 4 and chunk % 4 == 0
    sizes = _sizes(chunk)
    off, o = [], first
    for s in sizes:
        off.append(o)
        o += s
    n = o
    group = [i % 8 for i in range(len(sizes))]
    # brute force: the owner of every flat element, by walking the segments
    owner = np.full(n, -1, np.int64)
    for i, (a, s) in enumerate(zip(off, sizes)):
        owner[a:a + s] = i
    assert {a % 4 for a, s in zip(off, sizes) if s} == {0, 1, 2, 3}, "every flat offset phase occurs"
    table = solver_glue.chunk_table(off, sizes, group, n).numpy()
    covered = np.zeros(n, np.int64)
    prev_end = 0
    for c_off, seg_first, c_n, sg in table.tolist():
        seg, grp = divmod(sg, 8)
        assert 1 <= c_n <= chunk and prev_end <= c_off and c_off + c_n <= n
        assert sizes[seg] > 0 and grp == group[seg] and seg_first == off[seg]
        assert (owner[c_off:c_off + c_n] == seg).all()
        # a chunk ends where its segment ends or on a multiple of 4 of the flat offset, and begins likewise
        assert c_off == off[seg] or c_off % 4 == 0
        assert c_off + c_n == off[seg] + sizes[seg] or (c_off + c_n) % 4 == 0
        covered[c_off:c_off + c_n] += 1
        prev_end = c_off + c_n
    assert (covered == (owner >= 0)).all(), "every element of every segment exactly once"
    assert len(table) >= sum(-(-s // chunk) for s in sizes)


def test_chunk_cutter_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "solver_segs_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "solver_segs_host_harness.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout


# ---- 2. entry points ------------------------------------------------------------------------------------------------
def test_solver_symbols_and_version():
    import _hip
    lib = _hip.load()
    hdr = open(os.path.join(REPO, "include", "aabr_hip.h")).read()
    assert lib.aabr_version() == 640 and _hip.ABI_VERSION == 640 and "#define AABR_ABI_VERSION 640" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _hip._SIGS and hasattr(lib, name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, code).group(1)
        nargs = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert nargs == len(_hip._SIGS[name][1]), name
    assert lib.aabr_sgd_chunk_elems() % 4 == 0


def test_step_refuses_misuse_before_any_launch():
    """no GPU here: had any of these calls reached a launch it would have failed differently (AABR_ELAUNCH)"""
    import _hip
    lib = _hip.load()
    E = -1
    one = 4096                                     # a non-null, 16-byte aligned pointer nobody follows
    lr, wd = _hip.f32xn([0.1] * 8), _hip.f32xn([0.0] * 8)
    host = (C.c_int64 * 8)(0, 0, 16, 0, 16, 16, 16, 8 + 1)          # two chunks: [0, 16) and [16, 32), segments 0 and 1
    good = dict(flat=one, mom=one, n=32, table=one, host=host, n_chunks=2, n_segs=2, gflat=one, gtab=None, bf16=0, lr=lr,
                wd=wd, groups=2, mu=0.9, gs=1.0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.aabr_sgd_momentum_step(a["flat"], a["mom"], a["n"], a["table"], a["host"], a["n_chunks"], a["n_segs"],
                                          a["gflat"], a["gtab"], a["bf16"], a["lr"], a["wd"], a["groups"], a["mu"],
                                          a["gs"], None)

    cases = {
        "both": dict(gtab=one), "neither": dict(gflat=None),
        "n_groups": dict(groups=0), "n_groups ": dict(groups=9),
        "null parameter": dict(flat=None), "null momentum": dict(mom=None), "null chunk": dict(table=None),
        "null host copy": dict(host=None), "null lr": dict(lr=None), "null lr ": dict(wd=None),
        "negative": dict(n=-1), "negative ": dict(n_chunks=-2), "negative  ": dict(n_segs=-1),
        "past n": dict(n=31), "n_segs": dict(n_segs=1), "aligned": dict(flat=one + 4),
    }
    for what, kw in cases.items():
        assert call(**kw) == E, what
        err = lib.aabr_last_error()
        assert b"aabr_sgd_momentum_step" in err and what.strip().encode() in err, (what, err)
    # nothing to do is not an error, and needs no device
    assert call(n_chunks=0, host=None, table=None) == 0
    # the table builder's refusals
    so, sn, sg = _hip.i64xn([0, 8]), _hip.i64xn([8, 8]), _hip.i32xn([0, 1])
    assert lib.aabr_sgd_chunk_table(so, sn, sg, 2, 16, None, 0) == 2
    assert lib.aabr_sgd_chunk_table(so, sn, sg, 2, 15, None, 0) == -1 and b"past n" in lib.aabr_last_error()
    assert lib.aabr_sgd_chunk_table(so, sn, _hip.i32xn([0, 8]), 2, 16, None, 0) == -1 and b"group" in lib.aabr_last_error()
    assert lib.aabr_sgd_chunk_table(_hip.i64xn([0, 7]), sn, sg, 2, 16, None, 0) == -1 and b"overlap" in lib.aabr_last_error()
    out = (C.c_int64 * 4)()
    assert lib.aabr_sgd_chunk_table(so, sn, sg, 2, 16, out, 1) == -1 and b"too small" in lib.aabr_last_error()


def test_fused_sgd_refuses_what_the_kernel_lacks():
    import solver_glue
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(10)]
    for kw in (dict(nesterov=True, momentum=0.9), dict(dampening=0.1, momentum=0.9), dict(maximize=True)):
        with pytest.raises(ValueError):
            solver_glue.FusedSGD(ps, 0.1, **kw)
    opt = solver_glue.FusedSGD([{"params": [p], "lr": 0.1 * (i + 1)} for i, p in enumerate(ps[:9])], 0.1, momentum=0.9)
    with pytest.raises(ValueError, match="at most 8"):
        opt._pairs()
    opt = solver_glue.FusedSGD([{"params": [p], "lr": 0.1 * (i + 1)} for i, p in enumerate(ps[:8])], 0.1, momentum=0.9)
    opt.param_groups[3]["nesterov"] = True
    with pytest.raises(ValueError, match="nesterov"):
        opt.step()
    # the parameters moved into one flat buffer, and the momentum views share one flat buffer of the same layout
    base = opt.flat.flat.data_ptr()
    assert [p.data_ptr() - base for p in ps[:8]] == [12 * i for i in range(8)]
    assert opt.momentum_flat.numel() == opt.flat.flat.numel() == 24


# ---- 3. the yardsticks ------------------------------------------------------------------------------------------------
HYPER = [(0.001, 5e-4, 0.9), (0.002, 0.0, 0.9), (0.01, 5e-4, 0.0), (0.1, 1e-2, 0.5)]     # (lr, weight decay, momentum)
SCALES = [1.0, 0.25, 1.0 / 3]


def _state(n, seed):
    rng = np.random.default_rng(seed)
    mk = lambda: (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 2, n)).astype(np.float32)
    return mk(), mk(), mk()


@pytest.mark.parametrize("n", [7, 1000, 40001])
@pytest.mark.parametrize("hyper", HYPER)
def test_restatement_and_cpu_torch_lie_inside_the_bounds(n, hyper):
    lr, wd, mu = hyper
    worst_p = worst_m = 0.0
    for si, gs in enumerate(SCALES):
        p, m, g = _state(n, 100 * si + n)
        p64, m64 = R.step_f64(p, m, g, lr, wd, mu, gs)
        Bp, Bm = R.bounds(p, m, g, lr, wd, mu, gs)
        got = {"restatement": R.step_f32(p, m, g, lr, wd, mu, gs)}
        g_scaled = g if gs == 1.0 else (g * np.float32(gs)).astype(np.float32)     # the all-reduce path's mul_ before the step
        for foreach in (False, True):
            tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
            opt = torch.optim.SGD([tp], lr, momentum=mu, weight_decay=wd, foreach=foreach)
            if mu:
                opt.state[tp]["momentum_buffer"] = torch.from_numpy(m.copy())
            tp.grad = torch.from_numpy(g_scaled.copy())
            opt.step()
            got["torch foreach=%s" % foreach] = (tp.detach().numpy(), opt.state[tp]["momentum_buffer"].numpy() if mu else m)
        for name, (pp, mm) in got.items():
            ep = np.abs(pp.astype(np.float64) - p64)
            assert (ep <= Bp).all(), (name, gs, float((ep / Bp).max()))
            worst_p = max(worst_p, float((ep / Bp).max()))
            if mu:
                em = np.abs(mm.astype(np.float64) - m64)
                assert (em <= Bm).all(), (name, gs, float((em / Bm).max()))
                worst_m = max(worst_m, float((em / Bm).max()))
    print("n=%d hyper=%s: worst error / bound  p %.4f  m %.4f" % (n, hyper, worst_p, worst_m))


def test_restatement_edge_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    p = np.array([inf, 1.0, 1.0, -inf, 2.0], np.float32)
    g = np.array([1.0, inf, nan, 1.0, 0.0], np.float32)
    m = np.zeros(5, np.float32)
    pp, mm = R.step_f32(p, m, g, 0.1, 0.0, 0.9)
    assert pp[0] == inf and pp[1] == -inf and np.isnan(pp[2]) and pp[3] == -inf and pp[4] == 2.0
    assert mm[1] == inf and np.isnan(mm[2])
    pp, _ = R.step_f32(p, m, g, 0.1, 5e-4, 0.9)          # with weight decay inf - 0.1 * inf is NaN: why wd == 0 skips the term
    assert np.isnan(pp[0])
    pp, mm = R.step_f32(p, m, g, 0.1, 0.0, 0.0)
    assert mm is m                                       # no buffer without momentum
    bits = R.to_bf16_bits(np.array([1.0, -2.5, 3.1415927, 1e-3], np.float32))
    assert (R.widen_bf16(bits) == torch.tensor([1.0, -2.5, 3.1415927, 1e-3]).bfloat16().float().numpy()).all()
    assert R.same_values(np.array([nan, 1.0, 0.0]), np.array([nan, 1.0, -0.0]))
    assert not R.same_values(np.array([nan, 1.0]), np.array([1.0, nan]))


# ---- 4. schedule and groups against the reference's recorded results ---------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "solver_golden.npz"))
    return z, json.loads(str(z["cases"]))


def _sgd(base_lrs):
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in base_lrs]
    return torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(ps, base_lrs)], base_lrs[-1], momentum=0.9)


def _record(opt, sched, iters):
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # no optimizer.step() between the scheduler's steps here
        for _ in range(iters):
            rows.append([g["lr"] for g in opt.param_groups])
            sched.step()
    return np.array(rows, np.float64)


def test_warmup_multistep_lr_equals_the_reference(golden):
    from maskrcnn_benchmark.solver import WarmupMultiStepLR
    z, cases = golden
    assert set(cases["schedules"]) == {"linear", "constant", "no_warmup", "three_milestones", "milestone_in_warmup"}
    for name, c in cases["schedules"].items():
        opt = _sgd(cases["base_lrs"])
        sched = WarmupMultiStepLR(opt, c["milestones"], c["gamma"], warmup_factor=c["warmup_factor"],
                                  warmup_iters=c["warmup_iters"], warmup_method=c["warmup_method"])
        got, want = _record(opt, sched, c["iters"]), z["sched_" + name]
        assert got.shape == want.shape and (got == want).all(), name     # float64 equality: the same operation order
    opt = _sgd([0.1])
    with pytest.raises(ValueError, match="increasing"):
        WarmupMultiStepLR(opt, [5, 3])
    with pytest.raises(ValueError, match="warmup_method"):
        WarmupMultiStepLR(opt, [3, 5], warmup_method="cosine")


def test_make_lr_scheduler_equals_the_reference(golden):
    import solver_glue
    from maskrcnn_benchmark.solver import make_lr_scheduler
    z, cases = golden
    for name, c in cases["cfgs"].items():
        cfg = solver_glue.solver_cfg(gamma=c["GAMMA"], lr_step_epochs=c["LR_STEP_EPOCHS"], warmup_factor=c["WARMUP_FACTOR"],
                                     warmup_epochs=c["WARMUP_EPOCHS"], warmup_method=c["WARMUP_METHOD"],
                                     ims_per_batch=c["IMS_PER_BATCH"], example_num=c["Example_num"])
        opt = _sgd(cases["base_lrs"])
        sched = make_lr_scheduler(cfg, opt)
        assert list(sched.milestones) == z["cfg_%s_milestones" % name].tolist(), name
        assert sched.warmup_iters == int(z["cfg_%s_warmup_iters" % name]), name
        got, want = _record(opt, sched, c["iters"]), z["cfg_%s_lrs" % name]
        assert got.shape == want.shape and (got == want).all(), name
    assert int(z["cfg_capped_warmup_iters"]) == 500        # the fixture does exercise the cap


def test_make_optimizer_groups_equal_the_reference(golden):
    import solver_glue
    from maskrcnn_benchmark.solver import make_lr_scheduler, make_optimizer
    z, cases = golden

    class Named(object):
        def __init__(self):
            self.items = [(n, torch.nn.Parameter(torch.zeros(3), requires_grad=n not in cases["frozen"]))
                          for n in cases["names"]]

        def named_parameters(self):
            return iter(self.items)

    s = cases["solver"]
    cfg = solver_glue.solver_cfg(base_lr=s["BASE_LR"], bias_lr_factor=s["BIAS_LR_FACTOR"], momentum=s["MOMENTUM"],
                                 weight_decay=s["WEIGHT_DECAY"], weight_decay_bias=s["WEIGHT_DECAY_BIAS"])
    model = Named()
    opt = make_optimizer(cfg, model)
    assert isinstance(opt, solver_glue.FusedSGD) and isinstance(opt, torch.optim.Optimizer)
    by_param = {id(g["params"][0]): g for g in opt.param_groups}
    assert all(len(g["params"]) == 1 for g in opt.param_groups)
    want = z["groups_table"]
    for (name, p), row in zip(model.items, want):
        if np.isnan(row[0]):
            assert id(p) not in by_param, name
        else:
            g = by_param[id(p)]
            assert (g["lr"], g["weight_decay"]) == (row[0], row[1]), name
    assert [g["momentum"] for g in opt.param_groups] == z["groups_momentum"].tolist()
    assert opt.defaults["lr"] == float(z["groups_default_lr"])
    lrs, wds, _ = opt._pairs()                              # two (lr, weight_decay) pairs: the kernel's groups
    assert sorted(zip(lrs, wds)) == sorted({(r[0], r[1]) for r in want if not np.isnan(r[0])})
    # a scheduler over it writes the groups' lr, which is where the next step reads them
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make_lr_scheduler(solver_glue.solver_cfg(example_num=160, ims_per_batch=16), opt)
    assert opt.param_groups[0]["lr"] == s["BASE_LR"] * (1.0 / 3)
    assert sched.warmup_iters == 5
