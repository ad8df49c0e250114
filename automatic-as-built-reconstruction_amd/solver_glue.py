"""The optimizer step on the device (csrc/solver.hip): `FusedSGD`, a `torch.optim.Optimizer` with torch.optim.SGD's
parameter groups and state, whose `step` is ONE library launch over all parameters -- momentum, weight decay and a
per-group learning rate included.  The parameters live in a `dp.FlatParams` buffer; the momentum buffers are views of one
flat buffer of the same layout; the per-group lr / weight decay travel in the kernel's arguments, so a scheduler that
writes `param_groups[i]["lr"]` costs no device write.

Per element, fp32, every operation rounded on its own (tests/solver_ref.py is the numpy restatement):
    g  = widen(grad);  g = g * grad_scale      only when grad_scale != 1
    d  = g + wd * p                            only when wd != 0
    m' = mu * m + d                            only when mu != 0   (no buffer otherwise)
    p' = p - lr * m'
Dampening is 0 and there is no Nesterov form: the reference's optimizer (maskrcnn_benchmark/solver/build.py:7-20)."""
import ctypes as C

import torch

import _hip
import dp

MAX_GROUPS = 8          # csrc/solver_segs.h kSgdMaxGroups: distinct (lr, weight_decay) pairs of one step
_WORDS = 4              # int64 words per chunk record


def chunk_elems():
    return int(_hip.load().aabr_sgd_chunk_elems())


def chunk_table(seg_off, seg_numel, seg_group, n):
    """host chunk table of the segments (flat offset, numel, group) of a flat buffer of n elements: an int64 tensor
    [chunks, 4] of (flat offset, segment's flat offset, elements, segment * 8 + group) records"""
    lib = _hip.load()
    k = len(seg_off)
    so, sn = _hip.i64xn(seg_off), _hip.i64xn(seg_numel)
    sg = _hip.i32xn(seg_group)
    count = lib.aabr_sgd_chunk_table(so, sn, sg, k, n, None, 0)
    if count < 0:
        raise _hip.AabrError("libaabr_hip: %s" % lib.aabr_last_error().decode())
    table = torch.empty((max(int(count), 1), _WORDS), dtype=torch.int64)
    got = lib.aabr_sgd_chunk_table(so, sn, sg, k, n, C.cast(table.data_ptr(), _hip._i64p), count)
    if got != count:
        raise _hip.AabrError("libaabr_hip: %s" % lib.aabr_last_error().decode())
    return table[:count]


class FusedSGD(torch.optim.Optimizer):
    """torch.optim.SGD (momentum, weight decay; dampening 0, nesterov False, maximize False) with one launch per step.

    params: parameters or parameter groups, as torch.optim.SGD takes them (one group per parameter is the reference's
    form).  flat: a `dp.FlatParams` that already holds these parameters; None builds one (`FlatParams.from_params`),
    which moves the parameters' storage into its flat buffer.  All parameters are fp32 on one device.

    `state[p]["momentum_buffer"]` are views of ONE flat momentum buffer (`momentum_flat`); `state_dict()` has
    torch.optim.SGD's form and either class loads the other's.  Every group carries the same momentum; at most 8 distinct
    (lr, weight_decay) pairs may be in use in one step.  Steps are issued on one stream."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, flat=None):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedSGD: lr, momentum and weight_decay must not be negative")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)
        self._check_groups()
        mine = [p for g in self.param_groups for p in g["params"]]
        if flat is None:
            flat = dp.FlatParams.from_params(mine)
        self.flat = flat
        buf = flat.flat
        if buf.dtype != torch.float32:
            raise ValueError("FusedSGD: the flat parameter buffer must be float32")
        n, base = buf.numel(), buf.data_ptr()
        segs = []
        for p in mine:
            o = (p.data_ptr() - base) // 4
            if p.dtype != torch.float32 or not p.data.is_contiguous() or (p.data_ptr() - base) % 4 or o < 0 \
                    or o + p.numel() > n or p.device != buf.device:
                raise ValueError("FusedSGD: every parameter must be a contiguous float32 view of flat.flat")
            segs.append((o, p.numel(), p))
        segs.sort(key=lambda t: t[0])
        self._seg_off = [t[0] for t in segs]
        self._seg_numel = [t[1] for t in segs]
        self._seg_params = [t[2] for t in segs]
        self._seg_of = {id(p): i for i, p in enumerate(self._seg_params)}
        # one flat momentum buffer of the parameters' layout; memory only, until a step with momentum touches it
        self.momentum_flat = torch.zeros(n, device=buf.device, dtype=torch.float32)
        self._gptr_dev = torch.zeros(max(len(segs), 1), device=buf.device, dtype=torch.int64)
        self._gptr_list = None
        self._sig = None
        self._table = self._table_host = None
        self._views_done = False
        self.launches = 0        # library launches issued (tools / tests)
        self.uploads = 0         # host-to-device copies issued: chunk table and gradient-address table

    # ---- hyper-parameters -------------------------------------------------------------------------------------------
    def _check_groups(self):
        mu = self.param_groups[0]["momentum"]
        for g in self.param_groups:
            if g.get("nesterov", False):
                raise ValueError("FusedSGD: nesterov=True is not supported (the kernel has no Nesterov form)")
            if g.get("dampening", 0) != 0:
                raise ValueError("FusedSGD: dampening != 0 is not supported (the kernel's dampening is 0)")
            if g.get("maximize", False):
                raise ValueError("FusedSGD: maximize=True is not supported")
            if g["momentum"] != mu:
                raise ValueError("FusedSGD: every parameter group must carry the same momentum")
        return float(mu)

    def _pairs(self):
        """the step's distinct (lr, weight_decay) pairs in first-seen order, as two lists, and the pair of every segment"""
        pairs, sig = {}, [0] * len(self._seg_params)
        for g in self.param_groups:
            key = (float(g["lr"]), float(g["weight_decay"]))
            k = pairs.get(key)
            if k is None:
                k = pairs[key] = len(pairs)
            for p in g["params"]:
                sig[self._seg_of[id(p)]] = k
        if len(pairs) > MAX_GROUPS:
            raise ValueError("FusedSGD: %d distinct (lr, weight_decay) pairs in use, the kernel takes at most %d"
                             % (len(pairs), MAX_GROUPS))
        return [k[0] for k in pairs], [k[1] for k in pairs], sig

    def _groups(self):
        """`_pairs` for a step: rebuilds and uploads the chunk table when a segment changed its pair (a scheduler that
        scales every lr keeps them)"""
        lrs, wds, sig = self._pairs()
        if sig != self._sig:
            host = chunk_table(self._seg_off, self._seg_numel, sig, self.flat.flat.numel())
            self._table_host = host                      # kept: the step entry checks its last record
            self._table = self._upload(host)
            self._sig = sig
        return lrs, wds

    def _upload(self, host, out=None):
        """stream-ordered host-to-device copy from FRESH pinned staging: the staging block is never written again, and
        the caching host allocator hands it out anew only after the copy has run"""
        staging = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
        staging.copy_(host)
        if out is None:
            out = torch.empty(host.shape, dtype=host.dtype, device=self.flat.flat.device)
        out.copy_(staging, non_blocking=True)
        self.uploads += 1
        return out

    # ---- state ------------------------------------------------------------------------------------------------------
    def _view(self, i):
        o, k, p = self._seg_off[i], self._seg_numel[i], self._seg_params[i]
        return self.momentum_flat[o:o + k].view_as(p.data)

    def _make_views(self, have_grad):
        done = True
        for i, p in enumerate(self._seg_params):
            st = self.state.get(p, None)
            if st and "momentum_buffer" in st:
                continue
            if have_grad is None or have_grad[i]:
                self.state[p]["momentum_buffer"] = self._view(i)
            else:
                done = False
        self._views_done = done

    def load_state_dict(self, state_dict):
        """torch's loader replaces the state tensors by copies: the loaded buffers are copied into the flat momentum
        buffer and the views restored, so the kernel and `state` keep speaking of the same memory.  A parameter without a
        loaded buffer starts from zeros, as in a first step."""
        super().load_state_dict(state_dict)
        self._check_groups()
        for i, p in enumerate(self._seg_params):
            st = self.state.get(p, None)
            view = self._view(i)
            loaded = st.get("momentum_buffer", None) if st else None
            if loaded is None:
                view.zero_()
                if st is not None:
                    st.pop("momentum_buffer", None)
            else:
                view.copy_(loaded)
                st["momentum_buffer"] = view
        self._views_done = False
        self._sig = None

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _grad_table(self):
        """device table of the parameters' gradient addresses (0 = no gradient); uploaded only when an address moved"""
        ptrs = [0 if p.grad is None else p.grad.data_ptr() for p in self._seg_params]
        if ptrs != self._gptr_list:
            for p, a in zip(self._seg_params, ptrs):
                if a:
                    g = p.grad       # (torch keeps a parameter's grad in the parameter's dtype: float32)
                    if g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.numel() != p.numel() \
                            or g.device != p.device:
                        raise ValueError("FusedSGD: a gradient must be a dense contiguous float32 tensor of its "
                                         "parameter's size")
            if ptrs:
                self._upload(torch.tensor(ptrs, dtype=torch.int64), out=self._gptr_dev)
            self._gptr_list = ptrs
        return ptrs

    @torch.no_grad()
    def step(self, closure=None, *, flat_grad=None, grad_scale=1.0):
        """One optimizer step = one library launch (plus one small host-to-device copy when the gradients' addresses
        moved since the last step).  flat_grad: a float32 or bfloat16 tensor of flat.flat.numel() elements in the flat
        layout (dp.FlatParams.flat_grad, or its bf16 all-reduce message read in place), or None = `p.grad` of every
        parameter where autograd left it; a parameter whose grad is None is skipped, buffer and all.  grad_scale
        multiplies every gradient first (1 / world size turns an all-reduced sum into the mean)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        mu = self._check_groups()
        lrs, wds = self._groups()
        buf = self.flat.flat
        _hip.require_gpu(buf)
        if flat_grad is not None:
            if flat_grad.dtype not in (torch.float32, torch.bfloat16) or flat_grad.numel() != buf.numel() \
                    or not flat_grad.is_contiguous() or flat_grad.device != buf.device:
                raise ValueError("FusedSGD: flat_grad must be a contiguous float32 or bfloat16 tensor of flat.numel() "
                                 "elements on the parameters' device")
            gflat, gtab, bf16, have = flat_grad.data_ptr(), None, int(flat_grad.dtype == torch.bfloat16), None
        else:
            ptrs = self._grad_table()
            gflat, gtab, bf16 = None, self._gptr_dev.data_ptr(), 0
            have = ptrs
        if mu != 0.0 and not self._views_done:
            self._make_views(have)
        n_chunks = self._table_host.shape[0]
        _hip.check(_hip.load().aabr_sgd_momentum_step(
            buf.data_ptr(), self.momentum_flat.data_ptr(), buf.numel(), self._table.data_ptr(),
            C.cast(self._table_host.data_ptr(), _hip._i64p), n_chunks, len(self._seg_params), gflat, gtab, bf16,
            _hip.f32xn(lrs), _hip.f32xn(wds), len(lrs), mu, float(grad_scale), _hip.stream()))
        if n_chunks:
            self.launches += 1
        return loss


def solver_cfg(base_lr=0.001, bias_lr_factor=2, momentum=0.9, weight_decay=0.0005, weight_decay_bias=0, gamma=0.1,
               lr_step_epochs=(30,), warmup_factor=1.0 / 3, warmup_epochs=0.5, warmup_method="linear", ims_per_batch=16,
               example_num=1000):
    """a plain attribute tree with the cfg keys the solver reads, named and defaulted as in the reference's
    config/defaults.py -- for smoke(), the timing tool and the tests, which have no yacs config"""
    from rpn_glue import _Cfg
    solver = _Cfg(BASE_LR=base_lr, BIAS_LR_FACTOR=bias_lr_factor, MOMENTUM=momentum, WEIGHT_DECAY=weight_decay,
                  WEIGHT_DECAY_BIAS=weight_decay_bias, GAMMA=gamma, LR_STEP_EPOCHS=tuple(lr_step_epochs),
                  WARMUP_FACTOR=warmup_factor, WARMUP_EPOCHS=warmup_epochs, WARMUP_METHOD=warmup_method,
                  IMS_PER_BATCH=ims_per_batch)
    return _Cfg(SOLVER=solver, INPUT=_Cfg(Example_num=example_num))
