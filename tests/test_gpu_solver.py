"""The fused SGD step on the GPU (csrc/solver.hip through solver_glue.FusedSGD) against tests/solver_ref.py: exact
equality with the fp32 restatement over segment shapes, groups, gradient sources and non-finite values; CPU
torch.optim.SGD within twice the first-order bounds under a warm-up schedule; state dicts both ways; the dp.FlatParams
paths.  Every buffer the kernel touches lies inside a larger allocation whose guard elements are NaN before the call and
are checked untouched afterwards."""
import numpy as np
import pytest
import torch

import solver_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64            # guard elements on either side (keeps the 16-byte alignment of the view)


def _guarded(n, dtype=torch.float32, shift=0):
    """(allocation, view of n elements `shift` elements behind the front guard); the allocation is all NaN"""
    whole = torch.full((n + 2 * PAD + 4,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[PAD + shift:PAD + shift + n]


def _guards_intact(whole, n, shift=0):
    w = whole.float().cpu().numpy()
    return bool(np.isnan(w[:PAD + shift]).all() and np.isnan(w[PAD + shift + n:]).all())


class _Holder(object):
    """what FusedSGD reads of a dp.FlatParams: the flat parameter buffer"""

    def __init__(self, flat):
        self.flat = flat


class Rig(object):
    """segments of the given sizes packed back to back in a guarded flat buffer, one parameter group per parameter as
    the reference builds them, and the numpy state the restatement advances beside the device"""

    def __init__(self, sizes, lrs, wds, mu, seed=0):
        import solver_glue
        rng = np.random.default_rng(seed)
        self.sizes, self.n, self.mu = list(sizes), int(sum(sizes)), mu
        self.rng = rng
        self.p_np = rng.standard_normal(self.n).astype(np.float32)
        self.m_np = np.zeros(self.n, np.float32)
        self.p_all, self.p = _guarded(self.n)
        self.p.copy_(torch.from_numpy(self.p_np))
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.params = [torch.nn.Parameter(self.p[a:a + k]) for a, k in zip(self.off[:-1], self.sizes)]
        self.groups = [{"params": [q], "lr": lrs[i % len(lrs)], "weight_decay": wds[i % len(wds)]}
                       for i, q in enumerate(self.params)]
        self.opt = solver_glue.FusedSGD(self.groups, lrs[0], momentum=mu, flat=_Holder(self.p))
        self.m_all, m_view = _guarded(self.n)
        m_view.zero_()
        self.opt.momentum_flat = m_view          # before any step: the state's views are made from it

    def ref_step(self, grads, gs=1.0):
        """grads: one float32 array per segment, or None (skipped)"""
        for i, g in enumerate(grads):
            if g is None:
                continue
            a, b = self.off[i], self.off[i + 1]
            grp = self.opt.param_groups[i]
            self.p_np[a:b], m = R.step_f32(self.p_np[a:b], self.m_np[a:b], g, grp["lr"], grp["weight_decay"], self.mu, gs)
            self.m_np[a:b] = m

    def split(self, flat_np):
        return [flat_np[a:b] for a, b in zip(self.off[:-1], self.off[1:])]

    def check(self, what=""):
        torch.cuda.synchronize()
        p, m = self.p.cpu().numpy(), self.opt.momentum_flat.cpu().numpy()
        assert R.same_values(p, self.p_np), ("p differs from the restatement", what, int((p != self.p_np).sum()))
        assert R.same_values(m, self.m_np), ("m differs from the restatement", what, int((m != self.m_np).sum()))
        assert _guards_intact(self.p_all, self.n) and _guards_intact(self.m_all, self.n), ("guard overwritten", what)


def _chunk():
    import solver_glue
    return solver_glue.chunk_elems()


def _shape_sizes():
    c = _chunk()
    return [1, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4099, c - 1, c, c + 1, 2 * c + 3]


def _hyper(n_groups, wd):
    return [0.01 * (g + 1) for g in range(n_groups)], [wd * (1 + g % 2) for g in range(n_groups)]


# ---- 5. exactness by shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 0.25, 1.0 / 3])
@pytest.mark.parametrize("n_groups", [1, 2, 8])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("mu", [0.0, 0.9])
def test_exact_by_shape(mu, wd, n_groups, gs):
    lrs, wds = _hyper(n_groups, wd)
    rig = Rig(_shape_sizes(), lrs, wds, mu, seed=5)
    # gradients as the compiled backward leaves them: views of one buffer, the same addresses every step
    g_all, g = _guarded(rig.n)
    for q, a, k in zip(rig.params, rig.off[:-1], rig.sizes):
        q.grad = g[a:a + k]
    for step in range(5):
        g_np = rig.rng.standard_normal(rig.n).astype(np.float32)
        g.copy_(torch.from_numpy(g_np))
        rig.opt.step(grad_scale=gs)
        rig.ref_step(rig.split(g_np), gs)
        if step in (0, 4):
            rig.check("step %d" % step)
    assert _guards_intact(g_all, rig.n)
    # one library launch per step; the chunk table and the address table went up once
    assert rig.opt.launches == 5 and rig.opt.uploads == 2
    if mu:
        base = rig.opt.momentum_flat.data_ptr()
        assert [rig.opt.state[q]["momentum_buffer"].data_ptr() - base for q in rig.params] == (4 * rig.off[:-1]).tolist()
    else:
        assert all("momentum_buffer" not in rig.opt.state.get(q, {}) for q in rig.params)
        assert not rig.m_np.any()


def test_more_chunks_than_workgroups():
    """one segment of more than 2048 chunks (the grid's cap) beside small ones: every workgroup strides"""
    c = _chunk()
    rig = Rig([5, 2048 * c + 5 * c + 7, 3], [0.01, 0.02], [5e-4, 0.0], 0.9, seed=6)
    for step in range(2):
        g_np = rig.rng.standard_normal(rig.n).astype(np.float32)
        g_all, g = _guarded(rig.n)
        g.copy_(torch.from_numpy(g_np))
        rig.opt.step(flat_grad=g)
        rig.ref_step(rig.split(g_np))
    rig.check()
    assert rig.opt._table_host.shape[0] > 2048


# ---- 6. gradient sources -----------------------------------------------------------------------------------------------
def test_per_parameter_gradients_every_phase_fresh_addresses_and_none():
    sizes = [1, 3, 4, 5, 6, 7, 63, 65, 255, 257, 1023, 4099, _chunk() + 1, 2 * _chunk() + 3]
    rig = Rig(sizes, [0.01, 0.03], [5e-4, 0.0], 0.9, seed=7)
    absent = {2: (0, 1, 2), 9: (0, 1, 2, 3, 4), 11: (1, 3)}      # parameter -> steps without a gradient
    pairs, keep = set(), []
    for step in range(5):
        grads, allocs = [], []
        for i, (q, k) in enumerate(zip(rig.params, rig.sizes)):
            if step in absent.get(i, ()):
                q.grad = None
                grads.append(None)
                continue
            shift = (i + step) % 4                                # element offset of the gradient inside its allocation
            whole, view = _guarded(k, shift=shift)
            g_np = rig.rng.standard_normal(k).astype(np.float32)
            view.copy_(torch.from_numpy(g_np))
            q.grad = view
            grads.append(g_np)
            allocs.append((whole, k, shift))
            pairs.add((int(rig.off[i]) % 4, (view.data_ptr() // 4) % 4))
        before_p, before_m = rig.p.cpu().numpy().copy(), rig.opt.momentum_flat.cpu().numpy().copy()
        rig.opt.step()
        rig.ref_step(grads)
        rig.check("step %d" % step)
        p, m = rig.p.cpu().numpy(), rig.opt.momentum_flat.cpu().numpy()
        for i in absent:
            if step in absent[i]:                                 # bit for bit, not merely equal
                a, b = rig.off[i], rig.off[i + 1]
                assert (p[a:b].view(np.uint32) == before_p[a:b].view(np.uint32)).all()
                assert (m[a:b].view(np.uint32) == before_m[a:b].view(np.uint32)).all()
        assert all(_guards_intact(w, k, s) for w, k, s in allocs)
        keep.append(allocs)                                       # keep them alive: the next step's addresses are new
    assert len(pairs) == 16, "every (parameter phase, gradient phase) pair occurred"
    assert not rig.m_np[rig.off[9]:rig.off[10]].any() and "momentum_buffer" not in rig.opt.state.get(rig.params[9], {})
    # the address table followed: one upload per step beside the chunk table's, still one launch per step
    assert rig.opt.launches == 5 and rig.opt.uploads == 1 + 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shift", [0, 1])
def test_flat_gradient(dtype, shift):
    """one flat buffer of the parameters' layout, fp32 or bf16 (the all-reduce message read in place; the result is exact
    against the restatement fed the widened values); shift 1: a buffer whose address allows no 4-element loads"""
    rig = Rig(_shape_sizes(), [0.01, 0.02, 0.04], [5e-4, 0.0, 1e-3], 0.9, seed=8)
    for step in range(3):
        g_np = rig.rng.standard_normal(rig.n).astype(np.float32)
        if dtype == torch.bfloat16:
            g_np = R.widen_bf16(R.to_bf16_bits(g_np))
        g_all, g = _guarded(rig.n, dtype, shift)
        g.copy_(torch.from_numpy(g_np))
        assert (g.float().cpu().numpy() == g_np).all()
        rig.opt.step(flat_grad=g, grad_scale=0.5 if step == 1 else 1.0)
        rig.ref_step(rig.split(g_np), 0.5 if step == 1 else 1.0)
        rig.check("step %d" % step)
        assert _guards_intact(g_all, rig.n, shift)
    assert rig.opt.launches == 3 and rig.opt.uploads == 1
    with pytest.raises(ValueError):
        rig.opt.step(flat_grad=g[:-1])
    with pytest.raises(ValueError):
        rig.opt.step(flat_grad=g.double())


# ---- 7. non-finite values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_non_finite_values(wd):
    rig = Rig([5, 64, 257, 1030], [0.01, 0.02], [wd, wd], 0.9, seed=9)
    inf = np.float32(np.inf)
    rig.p_np[[0, 70, 300]] = [inf, -inf, inf]
    rig.p.copy_(torch.from_numpy(rig.p_np))
    for step in range(2):
        g_np = rig.rng.standard_normal(rig.n).astype(np.float32)
        g_np[[3, 71, 400]] = [inf, np.nan, -inf]
        g_all, g = _guarded(rig.n)
        g.copy_(torch.from_numpy(g_np))
        rig.opt.step(flat_grad=g)
        rig.ref_step(rig.split(g_np))
        rig.check("step %d" % step)
    p = rig.p.cpu().numpy()
    if wd == 0.0:
        assert p[0] == inf and p[70] == -inf and p[300] == inf        # an infinite p stays infinite, not NaN
        assert p[3] == -inf and p[400] == inf                         # an infinite gradient: an infinite step, twice
    assert np.isnan(p[71])
    assert np.isnan(rig.p_np).sum() < 12


# ---- 8. against torch under the warm-up schedule -----------------------------------------------------------------------
def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 129), torch.nn.ReLU(), torch.nn.Linear(129, 5)).to(DEV)


def test_against_cpu_torch_sgd_under_warmup_multistep():
    import solver_glue
    from maskrcnn_benchmark.solver import WarmupMultiStepLR, make_optimizer
    cfg = solver_glue.solver_cfg()
    model = _model(3)
    opt = make_optimizer(cfg, model)
    sched = WarmupMultiStepLR(opt, [3], 0.1, warmup_factor=1.0 / 3, warmup_iters=2, warmup_method="linear")
    # the reference's recipe on the CPU: one group per parameter, the "bias" rule, torch.optim.SGD
    cpu = [(k, torch.nn.Parameter(v.detach().cpu().clone())) for k, v in model.named_parameters()]
    groups = [{"params": [v], "lr": 0.001 * (2 if "bias" in k else 1), "weight_decay": 0 if "bias" in k else 0.0005}
              for k, v in cpu]
    ref = torch.optim.SGD(groups, groups[-1]["lr"], momentum=0.9)
    ref_sched = WarmupMultiStepLR(ref, [3], 0.1, warmup_factor=1.0 / 3, warmup_iters=2, warmup_method="linear")
    want_lr = [0.001 * (1.0 / 3), 0.001 * ((1.0 / 3) * (1 - 0.5) + 0.5), 0.001, 0.001 * 0.1, 0.001 * 0.1]
    mine = list(model.parameters())
    x = torch.randn(16, 37, device=DEV)
    for step in range(5):
        assert opt.param_groups[0]["lr"] == pytest.approx(want_lr[step], rel=1e-15)      # the weight of the first layer
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ref.param_groups]
        model.zero_grad(set_to_none=True)
        model(x + 0.1 * step).square().mean().backward()
        # re-synchronise: the CPU optimizer steps from the device's state and gradient
        before = []
        for q, (_, c) in zip(mine, cpu):
            c.data.copy_(q.data.cpu())
            c.grad = q.grad.cpu().clone()
            m = opt.state[q]["momentum_buffer"].cpu().clone() if step else None
            if m is not None:
                ref.state[c]["momentum_buffer"] = m
            before.append((c.detach().numpy().copy(), np.zeros(c.numel(), np.float32).reshape(c.shape) if m is None
                           else m.numpy().copy(), c.grad.numpy().copy()))
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        for q, (_, c), grp, (p0, m0, g0) in zip(mine, cpu, opt.param_groups, before):
            Bp, Bm = R.bounds(p0, m0, g0, grp["lr"], grp["weight_decay"], 0.9)
            dp_ = np.abs(q.detach().cpu().numpy().astype(np.float64) - c.detach().numpy())
            dm_ = np.abs(opt.state[q]["momentum_buffer"].cpu().numpy().astype(np.float64)
                         - ref.state[c]["momentum_buffer"].numpy())
            print("step %d %s: |p - torch| / B_p = %.3f   |m - torch| / B_m = %.3f"
                  % (step, tuple(q.shape), float((dp_ / np.maximum(Bp, 1e-300)).max()),
                     float((dm_ / np.maximum(Bm, 1e-300)).max())))
            assert (dp_ <= 2 * Bp).all() and (dm_ <= 2 * Bm).all(), (step, tuple(q.shape))
            assert np.abs(g0).max() > 0
        sched.step()
        ref_sched.step()


# ---- 9. state ----------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_torch_sgd():
    import solver_glue
    rig = Rig([5, 64, 257, 1030], [0.01, 0.02], [5e-4, 0.0], 0.9, seed=10)

    def one_step():
        g_np = rig.rng.standard_normal(rig.n).astype(np.float32)
        g_all, g = _guarded(rig.n)
        g.copy_(torch.from_numpy(g_np))
        rig.opt.step(flat_grad=g)
        rig.ref_step(rig.split(g_np))

    one_step()
    one_step()
    rig.check()
    # FusedSGD -> torch.optim.SGD
    sd = rig.opt.state_dict()
    cpu = [torch.nn.Parameter(q.detach().cpu().clone()) for q in rig.params]
    ref = torch.optim.SGD([{"params": [c]} for c in cpu], 0.5, momentum=0.1)
    ref.load_state_dict(sd)
    assert [g["lr"] for g in ref.param_groups] == [g["lr"] for g in rig.opt.param_groups]
    assert all(g["momentum"] == 0.9 for g in ref.param_groups)
    for c, a, b in zip(cpu, rig.off[:-1], rig.off[1:]):
        assert (ref.state[c]["momentum_buffer"].numpy() == rig.m_np[a:b]).all()
    for c in cpu:                         # torch steps from the loaded state
        c.grad = torch.ones_like(c)
    ref.step()
    # torch.optim.SGD -> FusedSGD: the buffers torch advanced come back into the flat buffer, the views are restored
    rig.opt.load_state_dict(ref.state_dict())
    base = rig.opt.momentum_flat.data_ptr()
    assert [rig.opt.state[q]["momentum_buffer"].data_ptr() - base for q in rig.params] == (4 * rig.off[:-1]).tolist()
    for c, a, b in zip(cpu, rig.off[:-1], rig.off[1:]):
        rig.m_np[a:b] = ref.state[c]["momentum_buffer"].numpy()
    rig.check("after load_state_dict")
    one_step()
    rig.check("the step after load_state_dict")
    # a state dict without buffers (a fresh torch optimizer's): the next step is a first step again
    rig.opt.load_state_dict(torch.optim.SGD([{"params": [c]} for c in cpu], 0.02, momentum=0.9).state_dict())
    rig.m_np[:] = 0
    one_step()
    rig.check("the step after loading an empty state")
    assert all(g["lr"] == 0.02 and g["weight_decay"] == 0 for g in rig.opt.param_groups)


def test_make_optimizer_end_to_end():
    import solver_glue
    from maskrcnn_benchmark.solver import make_lr_scheduler, make_optimizer
    cfg = solver_glue.solver_cfg(example_num=64, ims_per_batch=16, lr_step_epochs=(1,))
    model = _model(4)
    names = [k for k, _ in model.named_parameters()]
    opt = make_optimizer(cfg, model)
    sched = make_lr_scheduler(cfg, opt)
    assert sched.warmup_iters == 2 and tuple(sched.milestones) == (4,)
    p_np = [q.detach().cpu().numpy().copy() for q in model.parameters()]
    m_np = [np.zeros_like(v) for v in p_np]
    x = torch.randn(8, 37, device=DEV)
    for step in range(3):
        model.zero_grad(set_to_none=True)
        model(x).square().sum().backward()
        grads = [q.grad.cpu().numpy().copy() for q in model.parameters()]
        opt.step()
        for i, (k, grp) in enumerate(zip(names, opt.param_groups)):
            assert grp["weight_decay"] == (0 if "bias" in k else 0.0005)
            p_np[i], m_np[i] = R.step_f32(p_np[i], m_np[i], grads[i], grp["lr"], grp["weight_decay"], 0.9)
        sched.step()
        torch.cuda.synchronize()
        for q, want, m_want in zip(model.parameters(), p_np, m_np):
            assert R.same_values(q.detach().cpu().numpy(), want), step
            assert R.same_values(opt.state[q]["momentum_buffer"].cpu().numpy(), m_want), step
    assert opt.launches == 3


# ---- 10. dp paths ------------------------------------------------------------------------------------------------------
class _Done(object):
    """a finished collective, as dist.all_reduce(async_op=True) hands one back"""

    def wait(self):
        return True


def _dp_setup(seed, grad_dtype=None):
    import dp
    import solver_glue
    from maskrcnn_benchmark.solver import make_optimizer
    model = _model(seed)
    flat = dp.FlatParams([model], grad_dtype=grad_dtype)
    opt = make_optimizer(solver_glue.solver_cfg(), model, flat=flat)
    assert opt.flat is flat
    return model, flat, opt


def _backward(model):
    torch.manual_seed(11)
    x = torch.randn(8, 37, device=DEV)
    model.zero_grad(set_to_none=True)
    model(x).square().sum().backward()


def test_dp_paths_with_an_optimizer_equal_its_step():
    (ma, fa, oa), (mb, fb, ob), (mc, fc, oc) = _dp_setup(12), _dp_setup(12), _dp_setup(12)
    assert torch.equal(fa.flat, fb.flat) and torch.equal(fa.flat, fc.flat)
    for step in range(2):
        for m in (ma, mb, mc):
            _backward(m)
        oa.step()                                        # directly
        fb.sgd_step(123.0, 1, optimizer=ob)              # lr is ignored in favour of the optimizer's groups
        fc.pack_grads()
        fc._pending = _Done()
        assert fc.finish_update(123.0, 1, optimizer=oc) is True
        torch.cuda.synchronize()
        assert torch.equal(fa.flat, fb.flat) and torch.equal(oa.momentum_flat, ob.momentum_flat)
        assert torch.equal(fa.flat, fc.flat) and torch.equal(oa.momentum_flat, oc.momentum_flat)
    assert not torch.equal(oa.momentum_flat, torch.zeros_like(oa.momentum_flat))
    # several ranks' form: the summed bf16 message read in place, the mean's 1 / world size as the gradient scale
    (md, fd, od), (me, fe, oe) = _dp_setup(13, torch.bfloat16), _dp_setup(13)
    _backward(md)
    fd.pack_grads()
    fd.msg.copy_(fd.flat_grad)
    fd._pending = _Done()
    fd.finish_update(123.0, 4, optimizer=od)
    oe.step(flat_grad=fd.msg.float(), grad_scale=0.25)
    torch.cuda.synchronize()
    assert torch.equal(fd.flat, fe.flat) and torch.equal(od.momentum_flat, oe.momentum_flat)


def test_dp_paths_without_an_optimizer_are_unchanged():
    import dp
    lr = 1e-3
    ma, mb, mc, md = _model(14), _model(14), _model(14), _model(14)
    fa, fb = dp.FlatParams([ma]), dp.FlatParams([mb])
    for m in (ma, mb, mc, md):
        _backward(m)
    # the parent's two update lines, on copies of their own
    torch._foreach_add_([q.data for q in mc.parameters()], [q.grad for q in mc.parameters()], alpha=-lr)
    flat_d = torch.cat([q.data.reshape(-1) for q in md.parameters()])
    flat_d.add_(torch.cat([q.grad.reshape(-1) for q in md.parameters()]), alpha=-lr / 1)
    fa.sgd_step(lr, 1)
    fb.pack_grads()
    fb._pending = _Done()
    assert fb.finish_update(lr, 1) is True
    for q, w in zip(ma.parameters(), mc.parameters()):
        assert torch.equal(q.data, w.data)
    assert torch.equal(fb.flat, flat_d)
    assert fb.finish_update(lr, 1) is False              # nothing pending: no-op, as before
    # from_params: the same object over an explicit list
    me = _model(14)
    fd = dp.FlatParams.from_params(list(me.parameters()))
    assert torch.equal(fd.flat, dp.FlatParams([_model(14)]).flat) and len(fd.params) == 4
    assert all(q.data_ptr() >= fd.flat.data_ptr() for q in me.parameters())
