"""The deferred-join tail of the compiled FPN graph on the device (planExecutor `plan_tail`, csrc/plan.hip
AABR_PLAN_TAIL): the forward records no returned map depends on run on the library's tail stream beside the head and
the backward pass.  Same records, same operands: every number of a step is the bits of the one-stream list, whoever
joins the tail -- the backward list, the next forward, an accessor -- and an update right behind `backward()` does not
overtake it.  The `_fpn()` network of tests/test_gpu_fpn.py on 2 scenes x 20,000 points: the fine levels take the
three-launch BatchNorm and the wide and single-rule routes, the coarse ones the one-launch BatchNorm and the offset
split."""
import collections

import numpy as np
import pytest
import torch

import synth_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBOS = [(o, d) for o in ("first_seen", "brick") for d in (torch.float32, torch.bfloat16)]
IDS = ["%s-%s" % (o, "bf16" if d == torch.bfloat16 else "fp32") for o, d in COMBOS]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Rig(object):
    """one network, its start state and two inputs; `step` runs one training step under a tail mode"""

    def __init__(self, order, fdt):
        from test_cabi_and_host import default_fpn
        torch.manual_seed(8)
        self.net = default_fpn(feature_dtype=fdt).to(DEV)
        self.net.compiled_graph = True
        self.net.set_site_order(order)
        self.net.train(True)
        self.state = {k: v.clone() for k, v in self.net.state_dict().items()}
        locs, feats = S.make_batch(2, 20000, 43, 20)
        self.l, self.feats = _t(locs), _t(feats)
        locs2, feats2 = S.make_batch(2, 20000, 44, 20)
        self.l2, self.feats2 = _t(locs2), _t(feats2)
        self._ref = None

    def reset(self):
        self.net.join_unconsumed()
        self.net.load_state_dict(self.state)
        self.net.zero_grad()

    def running(self):
        return {k: v.clone() for k, v in self.net.state_dict().items() if "running" in k}

    def step(self, mode, backward=True, sync=True, after_backward=None, second=False):
        """-> dict of everything a step produces; `after_backward` runs right behind backward(), before any synchronize"""
        from sparseconvnet import planExecutor as pe
        pe.set_plan_tail(mode)
        self.reset()
        pe.debug_passes, pe.debug_kinds = [], []
        try:
            f = (self.feats2 if second else self.feats).clone().requires_grad_(True)
            rpn, roi = self.net([self.l2 if second else self.l, f])
            ps = pe.debug_passes[-1]
            in_flight = len(pe._tails)
            res = {"in_flight": in_flight, "ps": ps}
            if backward:
                w = [torch.linspace(0.5, 1.5, m.features.numel(), device=DEV).view_as(m.features) for m in rpn + roi]
                sum((m.features * wi).square().mean() for m, wi in zip(rpn + roi, w)).backward()
                res["in_flight_after_backward"] = len(pe._tails)
                if after_backward is not None:
                    after_backward()
            if sync:
                torch.cuda.synchronize()
            res["outs"] = [m.features.detach().clone() for m in rpn + roi]
            if backward:
                res["dx"] = f.grad.clone()
                res["grads"] = {n: p.grad.clone() for n, p in self.net.named_parameters() if p.grad is not None}
            res["kinds"] = [(d, sorted(collections.Counter(k).items())) for d, k in pe.debug_kinds]
            return res
        finally:
            pe.debug_passes, pe.debug_kinds = None, None

    def buffers(self, ps):
        """every buffer of the pass's arena that a record writes: a convolution whose add rides in its write-out writes
        the add's buffer, and its own slot stays as the allocator left it"""
        unwritten = {op.out for op in ps.t.fops if op.kind == "conv" and ps.fwd_route(op)[1] is not None}
        assert len(unwritten) < len(ps.t.fbufs) // 2
        return [ps.buffer(b).clone() for b in range(1, len(ps.t.fbufs)) if b not in unwritten]

    def ref(self):
        """the one-stream step (tail off), computed once per rig and left unchanged"""
        if self._ref is None:
            r = self.step(0)
            assert r["in_flight"] == 0
            r["bufs"], r["running"] = self.buffers(r["ps"]), self.running()
            r["bn"] = {m: v.clone() for m, v in r["ps"].bn_outputs().items()}
            r["dead_bn"] = [op.module for i, op in enumerate(r["ps"].t.fops) if op.kind == "bn" and i in r["ps"].t.dead]
            del r["ps"]
            self._ref = r
        return self._ref


_rigs = {}


@pytest.fixture(params=COMBOS, ids=IDS)
def rig(request):
    from sparseconvnet import planExecutor as pe
    r = _rigs.get(request.param)
    if r is None:
        r = _rigs[request.param] = _Rig(*request.param)
    keep = (pe.grad_segments, pe.on_grads_ready, pe.pipeline_records)
    try:
        yield r
    finally:
        pe.grad_segments, pe.on_grads_ready, pe.pipeline_records = keep
        pe.set_plan_tail(None)


def _same_step(ref, got, what):
    for x, y in zip(ref["outs"], got["outs"]):
        assert torch.equal(x, y), what
    assert torch.equal(ref["dx"], got["dx"]), what
    assert ref["grads"].keys() == got["grads"].keys()
    for n in ref["grads"]:
        assert torch.equal(ref["grads"][n], got["grads"][n]), (what, n)
    assert ref["kinds"] == got["kinds"], what


def test_unconsumed_set_is_what_pruning_would_drop(rig):
    """for this network the dataflow rule names exactly the stages `prune_unused_levels` would not run"""
    ref = rig.ref()
    net = rig.net
    n = len(net.m_downs) - 1
    keep = min(n, max(list(net.fpn_scales_from_top) + list(net.roi_scales_from_top)))
    assert 0 < keep < n
    want = {net.m_ups[k][0] for k in range(keep, n)}          # the BatchNorm of every top-down stage below the last map
    assert set(ref["dead_bn"]) == want


def test_tail_on_equals_tail_off_and_itself(rig):
    ref = rig.ref()
    for mode in (1, 2, 1):
        got = rig.step(mode)
        assert got["in_flight"] == 1 and got["in_flight_after_backward"] == 0     # forked by forward, joined by backward
        _same_step(ref, got, mode)
        for i, (x, y) in enumerate(zip(ref["bufs"], rig.buffers(got["ps"]))):
            assert torch.equal(x, y), (mode, i)
        run = rig.running()
        for k in ref["running"]:
            assert torch.equal(ref["running"][k], run[k]), (mode, k)


def test_forward_only_accessor_joins(rig):
    """`bn_outputs()` of the unconsumed stages read right behind the forward, no synchronize in between"""
    ref = rig.ref()
    got = rig.step(1, backward=False, sync=False)
    assert got["in_flight"] == 1
    bn = got["ps"].bn_outputs()
    vals = {m: bn[m].clone() for m in ref["dead_bn"]}
    from sparseconvnet import planExecutor as pe
    assert len(pe._tails) == 0
    torch.cuda.synchronize()
    assert ref["dead_bn"]
    for m in ref["dead_bn"]:
        assert torch.equal(vals[m], ref["bn"][m])


def test_dropped_pass_then_next_forward(rig):
    """a forward whose results are dropped without a backward, then at once a forward on another input: the second
    pass's numbers are those of the same two passes on one stream"""
    from sparseconvnet import planExecutor as pe

    def two(mode):
        pe.set_plan_tail(mode)
        rig.reset()
        f = rig.feats.clone().requires_grad_(True)
        out = rig.net([rig.l, f])
        n_tails = len(pe._tails)
        del out, f
        pe.debug_passes = []
        try:
            f2 = rig.feats2.clone().requires_grad_(True)
            rpn, roi = rig.net([rig.l2, f2])
            ps = pe.debug_passes[-1]
        finally:
            pe.debug_passes = None
        outs = [m.features.detach().clone() for m in rpn + roi]
        bufs = rig.buffers(ps)
        torch.cuda.synchronize()
        return n_tails, outs, bufs, rig.running()

    a, b = two(0), two(1)
    assert a[0] == 0 and b[0] == 1
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(x, y)
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_bucketed_hand_over(rig):
    """grad_segments = 4 with a recording hook: what each bucket hands over equals the one-piece gradients"""
    from sparseconvnet import planExecutor as pe
    ref = rig.ref()
    names = {id(p): n for n, p in rig.net.named_parameters()}
    seen, pieces = {}, []

    def hook(piece, total, flat, pairs):
        pieces.append((piece, total))
        for p, g in pairs:
            seen[names[id(p)]] = g.clone()

    pe.grad_segments, pe.on_grads_ready = 4, hook
    got = rig.step(1)
    pe.grad_segments, pe.on_grads_ready = 0, None
    assert got["in_flight"] == 1 and got["in_flight_after_backward"] == 0
    assert [p for p, _ in pieces] == sorted(p for p, _ in pieces) and pieces[-1] == (3, 4)
    graph = {names[id(p)] for p in got["ps"].t.params}        # (layers_in runs in front of the compiled graph)
    assert set(seen) == set(ref["grads"]) & graph and len(seen) > 100
    for n in seen:
        assert torch.equal(seen[n], ref["grads"][n]), n
    for x, y in zip(ref["outs"], got["outs"]):
        assert torch.equal(x, y)
    assert torch.equal(ref["dx"], got["dx"])
    run = rig.running()
    for k in ref["running"]:
        assert torch.equal(ref["running"][k], run[k]), k


def test_pipelined_hand_over_declines_the_tail(rig):
    from sparseconvnet import planExecutor as pe
    ref = rig.ref()
    pe.pipeline_records = 7
    got = rig.step(1)
    pe.pipeline_records = 0
    assert got["in_flight"] == 0
    _same_step(ref, got, "pipelined")
    run = rig.running()
    for k in ref["running"]:
        assert torch.equal(ref["running"][k], run[k]), k


def test_update_right_behind_backward_does_not_overtake_the_tail(rig):
    """an in-place update of EVERY parameter and BatchNorm buffer on the main stream right behind backward(), no
    synchronize in between: the backward list's join record must stand in front of it"""
    ref = rig.ref()
    kept = {}

    def update():
        kept.update(rig.running())                   # read on the main stream, in order behind the join
        with torch.no_grad():
            for p in rig.net.parameters():
                p.mul_(0.5)
            for n, b in rig.net.named_buffers():
                if "running" in n:
                    b.zero_()

    for mode in (1, 2):
        kept.clear()
        got = rig.step(mode, after_backward=update)
        assert got["in_flight"] == 1 and got["in_flight_after_backward"] == 0
        for k in ref["running"]:
            assert torch.equal(ref["running"][k], kept[k]), (mode, k)
        bn = got["ps"].bn_outputs()
        for m in ref["dead_bn"]:
            assert torch.equal(bn[m], ref["bn"][m]), mode
        _same_step(ref, got, mode)
