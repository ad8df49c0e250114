"""Compiled execution of the static part of a SparseConvNet module graph (extension; the reference runs every
layer through its own Python module, autograd Function and pybind call: submanifoldConvolution.py:27-95,
convolution.py:29-90, deconvolution.py:16-87, batchNormalization.py:29-108, tables.py:27-41).

Between the input layer and the returned feature maps FPN_Net (fpn_net.py:168-203) is a fixed dataflow graph of
BatchNorm+LeakyReLU, submanifold / strided / transposed convolutions and residual adds over geometry that is
known before the first feature row is computed.  `run_fpn` turns every layer into one `AabrPlanOp` record of the
library's own entry point -- the launch `SCN.py` would have made, same kernel, same arguments, same order -- and
hands the list to `aabr_plan_run` in one call.  Activations live in one arena; the backward pass is a second list
generated in reverse (input gradients, weight gradients, BatchNorm backward, gradient sums for tensors with
several consumers in the order autograd would add them).  One autograd node stands for the whole graph;
parameters, running statistics and state_dict are the modules' own.

Two stages, so that a pass costs little Python:
  * `_Template` (once per network / input size / dtype / mode): walks the SAME module objects with symbolic
    tensors and records the structure -- which buffer feeds which launch, plane counts, rule-book keys, parameter
    and weight-pack addresses, the backward list and its gradient buffers;
  * a pass fills in what the scene decides: rows per scale, rule-book streams, arena addresses.

What it buys: the ~25 us of interpreter + autograd work per layer and direction leave the critical path.  What it
does not do: change any number -- `tests/test_gpu_fpn.py` holds it bit-equal to the module path.  Falls back
(returns None) when a module of the graph carries hooks or is of a type it does not know."""
import ctypes
import functools
import os
import threading
from collections import namedtuple

import torch
from torch.autograd import Function

import _hip
from _hip import stream, check
from . import SCN
from . import plan_records as R      # the AabrPlanOp record format: one field table and one writer per layout
from .plan_records import (K_CONV, K_WIDE, K_DW, K_BNF, K_BNB, K_ADD, K_CAST, K_WSPLIT, K_NARROW, K_SINGLE,  # noqa: F401
                           K_TAIL_JOIN, F_BF16, F_TO_BF16, F_SIDE, F_JOIN, F_TAIL)
from .sparseConvNetTensor import SparseConvNetTensor
from .sequential import Sequential
from .tables import AddTable, ConcatTable
from .identity import Identity
from .batchNormalization import BatchNormalization
from .submanifoldConvolution import SubmanifoldConvolution
from .convolution import Convolution
from .deconvolution import Deconvolution
from .fullConvolution import FullConvolution

_ALIGN = 256
BF16 = torch.bfloat16

stats = {"passes": 0, "fallbacks": 0, "templates": 0}
# weight gradients on the library's second stream (nothing later in a backward list reads them): they fill the CUs
# the tails and small launches of the input-gradient chain leave idle
dw_side_stream = os.environ.get("AABR_PLAN_DW_SIDE", "1") != "0"
# a residual / lateral add whose second operand comes straight from a wide-kernel convolution rides in that
# convolution's write-out (forward only; the backward list is unchanged)
fuse_adds = os.environ.get("AABR_PLAN_FUSE_ADDS", "1") != "0"
# ... the same in bf16 storage (round 6; forward adds, and the gradient sums of the backward list)
fuse_adds_bf16 = os.environ.get("AABR_PLAN_FUSE_ADDS_BF16", "1") != "0"
# a training-mode BatchNorm right behind a wide-kernel convolution takes its statistics' partial sums from that
# convolution's write-out (aabr_conv_forward_wide_stats -> aabr_bn_forward_parts): one pass over the matrix less
conv_bn_stats = os.environ.get("AABR_PLAN_CONV_BN_STATS", "1") != "0"
# ... and a BatchNorm backward right behind the wide-kernel input-gradient launch that produced its d_out takes its
# statistics from that launch's write-out (aabr_conv_forward_wide[_bf16]_bwd_stats -> aabr_bn_backward_parts[_bf16])
conv_bn_bwd_stats = os.environ.get("AABR_PLAN_CONV_BN_BWD_STATS", "1") != "0"
# ... the same two from the write-out of the 32 -> 32 kernel (csrc/conv_narrow.hip; bf16 storage).  Measured on the config-4
# step, same box, two runs each: narrow kernel off 10.22 / 10.18 ms, on 10.02 / 10.01, on with these statistics 10.13 / 10.13 --
# the wave-level reductions (16 x 8 fp64 values per 16-row group) cost the launch more than the BatchNorm's own HBM-bound
# statistics passes; off by default.
narrow_stats = os.environ.get("AABR_PLAN_NARROW_STATS", "0") != "0"
# The forward ops no returned map depends on (`unconsumed_ops`: for the bench network the top-down stages below the last
# consumed level, which the reference computes all the same) go to the END of a training pass's forward list, flagged
# AABR_PLAN_TAIL: the library runs them on its tail stream beside the head, the loss and the backward pass instead of
# in front of them, and the pass holds the ticket (`_Pass.join_tail`; who joins when: DESIGN.md "The deferred-join tail").
# Same records, same operands, same bits.  0 = today's list; 1 = a tail stream of its own; 2 = the tail shares one
# process-wide second stream with the weight gradients.  The environment variable is the library's PLAN_TAIL knob as
# well (one name, read by both sides); `set_plan_tail` switches both inside a process.
PLAN_TAIL_DEFAULT = 2                    # = kPlanTailDefault of csrc/plan.hip
plan_tail = int(os.environ.get("AABR_PLAN_TAIL", PLAN_TAIL_DEFAULT))


def set_plan_tail(v):
    """switch the tail (0 / 1 / 2) on both sides of the C ABI; None = the shipped default.  Joins what is in flight."""
    global plan_tail
    join_pending()
    plan_tail = PLAN_TAIL_DEFAULT if v is None else int(v)
    assert plan_tail in (0, 1, 2)
    _hip.set_knob("PLAN_TAIL", plan_tail)


def unconsumed_ops(fops, outs):
    """indices of the forward ops from which no returned buffer is reachable: walking the list backwards, an op is
    needed when a returned buffer or a needed op reads what it writes.  `fops`: the template's forward op records (`Add`,
    `Cast`, `Bn`, `Conv`: `.ins` / `.out`); `outs`: [(buffer, ..)] of the returned maps.  A rule over the dataflow, not
    over level numbers."""
    need = {b for b, _ in outs}
    dead = set()
    for i in range(len(fops) - 1, -1, -1):
        op = fops[i]
        if op.out in need:
            need.update(op.ins)
        else:
            dead.add(i)
    return frozenset(dead)


def tail_emission(fops, dead):
    """[(op, record flags)]: the consumed ops in their order, then the unconsumed ones in theirs, flagged for the tail.
    A stable partition, so two ops of the same class that stood next to each other still do: a convolution and the
    add that rides in its write-out (the add is the convolution's only reader, so both are in the same class), and a
    convolution and the BatchNorm that takes its statistics, unless the convolution is consumed and the BatchNorm is
    not -- the one pair that crosses (`_Template._cross_claims`)."""
    return [(op, 0) for i, op in enumerate(fops) if i not in dead] + \
           [(op, F_TAIL) for i, op in enumerate(fops) if i in dead]


# passes whose tail nobody has joined yet.  A STRONG reference: the arena, the geometry, the split scratch and the
# statistics buffers the tail reads and writes cannot go back to the allocator (which reuses blocks in main-stream
# order) before a join has been enqueued -- "the pass went away without a backward" cannot precede its join.
_tails = []
_tails_lock = threading.Lock()


def join_pending(device=None):
    """the current stream of `device` (None: of each pass's own device) waits for every tail still in flight there"""
    with _tails_lock:
        take = [p for p in _tails if device is None or p.dev == device]
    for p in take:
        p.join_tail()


# Data-parallel hook (extension; the reference wraps the model in DistributedDataParallel, whose bucketed all-reduce
# starts while backward is still running, tools/train_net_sparse3d.py:64-69): with `grad_segments` = S > 1 and
# `on_grads_ready` set, the compiled backward list is handed to the library in S pieces and after each piece the hook
# receives the gradients that are final by then -- `on_grads_ready(piece, S, flat, [(parameter, gradient view)])`,
# `flat` = the contiguous slice of the pass's gradient buffer that holds exactly those views -- so a collective on
# `flat` runs underneath the rest of the backward pass.  Same launches in the same order; a piece boundary only
# makes the caller's stream wait for the weight gradients issued so far on the library's second stream.
grad_segments = 0
on_grads_ready = None
# Pipelined hand-over (aabr_plan_submit / aabr_plan_drain; option): every `pipeline_records` records the part of the list
# that is final goes to the library's launcher thread, which issues its launches while this thread fills the next part --
# the two halves of a pass's host cost (filling records, issuing launches) overlap instead of adding up, and the device
# starts the pass one part in instead of after the whole list.  Same records in the same order, bit-equal results
# (tests/test_gpu_fpn.py).  Measured on the bench step (round 4, tools/tools_host_breakdown.py): the two passes' host time
# 2.50 -> 2.00 ms (the launcher needs 1.37 ms per step to issue ~450 launches either way, and the pass must be drained
# before torch's next launch), step time unchanged within noise in fp32 (device-bound) and bf16 (7.88 vs 7.90 ms: the
# device's chain of small launches is as long as the host's) -- so the default is 0 = one call per pass.
pipeline_records = int(os.environ.get("AABR_PLAN_PIPELINE", "0"))
# tests: a list here receives every _Pass that runs (its arena holds every activation of the pass --
# `_Pass.bn_outputs()`); None in production
debug_passes = None
# tests: a list here receives ("fwd" | "bwd", [record kinds]) of every launch list a pass builds; None in production
debug_kinds = None
debug_bwd_stats = None   # tests: a list that receives, per backward list, (kind, bwd_stats slot) of every record
# a pass that will not be differentiated packs its activations by liveness (AABR_PLAN_PACK_ARENA=0: one slot each, as
# the training pass needs them)
pack_inference_arena = os.environ.get("AABR_PLAN_PACK_ARENA", "1") != "0"


class Unsupported(Exception):
    pass


def _es(dt):
    return 2 if dt == BF16 else 4


def _dp(t):
    return t.data_ptr() if t is not None else 0


def _bf(dt):
    """the storage flag of a record over matrices of type `dt`"""
    return F_BF16 if dt == BF16 else 0


def _bytes(fbuf, V):
    """bytes the [rows(level), planes] matrix of a buffer (level, planes, dtype) takes in an arena, padding included"""
    lvl, planes, dt = fbuf
    return (V[lvl] * planes * _es(dt) + _ALIGN - 1) // _ALIGN * _ALIGN


def _view(arena, o, fbuf, V):
    """the [rows(level), planes] matrix of a buffer (level, planes, dtype) at byte offset `o` of `arena`"""
    lvl, planes, dt = fbuf
    return arena[o:o + V[lvl] * planes * _es(dt)].view(dt).view(V[lvl], planes)


def _slot_floats(p):
    """floats of parameter `p`'s slot in a pass's gradient buffer: padded, so that every slot starts 256-byte aligned"""
    return (p.numel() + 63) // 64 * 64


# buffer references inside a backward list: (space, index); spaces resolved to address lists per pass
F, G, E = 0, 1, 2      # forward arena (index 0 = the graph input) / gradient arena / external output gradients


# ---- The ops of a template: tuples with named fields, `kind` first; the loops over a list unpack a whole op in one
# statement, everything else goes by field name.  A forward op (`_Template.fops`) answers `.ins`, the buffers it reads,
# and `.out`, the buffer it writes: indices into `_Template.fbufs` (levels: into `_Template.levels`).
def _forward_op(name, fields, ins):
    reads = property(lambda op: tuple(getattr(op, f) for f in ins), doc="the buffers the op reads")
    return type(name, (namedtuple(name, fields),), {"__slots__": (), "ins": reads})


# "add": out = a + b, in this order (utils._sum_features), over [rows(lvl), planes] matrices; flags: F_BF16 in bf16 storage.
# The backward list holds `Add` and `Cast` too, with (space, index) references in their buffer fields.
Add = _forward_op("Add", "kind a b out lvl planes flags", ins=("a", "b"))
# "cast": flags F_TO_BF16 = fp32 -> bf16, 0 = bf16 -> fp32
Cast = _forward_op("Cast", "kind x out lvl planes flags", ins=("x",))
# "bn": BatchNorm + LeakyReLU.  flags: F_BF16; train: 1 = batch statistics, 0 = the running ones; stat: float offset of
# save_mean in the pass's statistics buffer, save_invstd follows at + planes; running_mean .. bias: addresses, 0 = none
Bn = _forward_op("Bn", "kind x out lvl planes flags train eps momentum leak stat running_mean running_var weight bias "
                 "module", ins=("x",))
# "conv": submanifold, strided or transposed.  lvl / lvl_out: level of x / of out; book: index into `_Template.books` and
# `_Pass.books`; side_fwd: the side of the book that gathers for the forward launch (0 = out, 1 = inn: Deconvolution);
# weight, pack_fwd, pack_t: addresses of the raw weight, its forward pack and its transposed pack (input gradient);
# side_din, din_flags: the input-gradient launch's side of the book and convolution flags; side_dw: the weight gradient's
Conv = _forward_op("Conv", "kind x out lvl lvl_out n_in n_out book side_fwd weight pack_fwd side_din din_flags side_dw "
                   "pack_t module", ins=("x",))

# ---- backward ops (`_Template._make_backward`): gx, gy, res and tmp are (space, index) references
# "bn": x, y: forward buffer indices of the BatchNorm's input and output; stat: as `Bn.stat`; weight, bias: addresses, 0 =
# not affine; d_weight_slot, d_bias_slot: byte offsets into the pass's parameter-gradient buffer, -1 = no gradient wanted;
# res: None, or the gradient that has arrived at x so far (the apply pass then writes gx = d_in + res)
BnBwd = namedtuple("BnBwd", "kind x gx y gy lvl planes flags leak stat weight d_weight_slot d_bias_slot bias res")
# "din": the input gradient of a convolution, a forward-form launch of its own that reads d_out and writes d_in -- so
# lvl_in / lvl_out and n_in / n_out are the forward op's lvl_out / lvl and n_out / n_in.  side, conv_flags: the forward
# op's side_din, din_flags; flags: F_BF16; res: as `BnBwd.res`, rides in a wide launch's write-out; tmp (with res): a spare
# buffer for d_in when the launch is not a wide one (then gx = res + tmp); one_rule: `_one_rule(module, True)`
Din = namedtuple("Din", "kind gy gx lvl_in lvl_out n_in n_out book side conv_flags weight pack_t flags res tmp one_rule")
# "dw": the weight gradient of a convolution.  x: forward buffer index of its input; lvl_out: the rows of gy; n_in, n_out,
# book: as the forward op's; side: its side_dw; slot: byte offset of the gradient in the parameter-gradient buffer
Dw = namedtuple("Dw", "kind x gy lvl_out n_in n_out book side slot flags")


class _Template(object):
    """the structure of the graph, independent of the scene"""

    def __init__(self, net, x_spatial, x_planes, dtype, plan):
        self.dtype = dtype
        self.levels, self.lvl = [], {}
        self.fbufs = []                      # (level, planes, dtype)
        self.books, self.bidx = [], {}       # rule books: (kind, dict key, builder args)
        self.fops = []
        self.params, self.pidx = [], {}
        self.stat_floats = 0
        self.bn_floats = 0
        self.max_planes = 1
        self.hidden = []                     # (level, planes) of every convolution output (hidden-state counter)
        self.macs = []                       # (book, weight) per convolution, in order
        self.bns = []
        self.packs = {id(w): (pf.data_ptr(), pt.data_ptr()) for w, (pf, pt) in zip(plan.weights, plan.packs)}
        self.lib = _hip.load()
        x = (self._new(self._level(x_spatial), x_planes, torch.float32), x_spatial)
        xs = self.cast(x, dtype)
        rpn, roi = _fpn_graph(net, self, xs)
        self.n_rpn = len(rpn)
        self.outs = [self.cast(t, torch.float32) for t in rpn] + [self.cast(t, torch.float32) for t in roi]
        self._bwd = {}
        self.fuse = self._fusable_adds() if fuse_adds else {}
        self.stat_claims = self._stat_claims()
        # the tail form of the list (a training pass with `plan_tail`): consumed records first, then the unconsumed ones
        self.dead = unconsumed_ops(self.fops, self.outs)
        self.emit_tail = tail_emission(self.fops, self.dead) if self.dead else None
        self.cross = self._cross_claims() if self.dead else {}
        stats["templates"] += 1

    def _next_on_stream(self, i):
        """the record behind forward op `i` on its stream in the one-stream list, the add that rides in op i's own
        write-out aside; None behind the last"""
        fz = self.fuse.get(id(self.fops[i]))
        return next((nop for nop in self.fops[i + 1:] if fz is None or nop is not fz[0]), None)

    def _stat_claims(self):
        """ids of the convolution ops whose write-out a training-mode BatchNorm may ask for its statistics (`_Pass._forward`):
        the next record on the convolution's stream -- its own fused add aside -- is that BatchNorm, reading what the
        launch writes"""
        out = set()
        for i, op in enumerate(self.fops):
            if op.kind != "conv":
                continue
            fz = self.fuse.get(id(op))
            wrote = (op.out,) if fz is None else (op.out, fz[0].out)
            nop = self._next_on_stream(i)
            if nop is not None and nop.kind == "bn" and nop.train and nop.planes == op.n_out and nop.x in wrote:
                out.add(id(op))
        return out

    def _cross_claims(self):
        """{id(BatchNorm op): id(convolution op)} of the statistics claims (`_stat_claims`) that cross from the caller's
        stream to the tail: a consumed convolution whose write-out forms the statistics of an UNCONSUMED BatchNorm (the
        first top-down stage below the last returned map normalises that map).  The convolution still forms them, into a
        buffer of the pair's own, and the BatchNorm record on the tail reads them there: the bits of the one-stream list."""
        idx = {id(op): i for i, op in enumerate(self.fops)}
        out = {}
        for i, op in enumerate(self.fops):
            if id(op) not in self.stat_claims or i in self.dead:
                continue
            nop = self._next_on_stream(i)        # the BatchNorm of the claim
            if idx[id(nop)] in self.dead:
                out[id(nop)] = id(op)
        return out

    def _fusable_adds(self):
        """{id(conv op): (add op, other operand)}: a convolution whose only reader is an add with an operand that
        exists before the convolution runs -- the add can ride in the convolution's write-out when the pass dispatches it
        to the wide kernel or the offset split (`aabr_conv_forward_wide_res`, `aabr_conv_forward_wide_bf16_res`, the
        split's second stage; a + b == b + a bit for bit, and in bf16 storage the write-out rounds the convolution's
        value before the sum exactly as the separate add would have read it)"""
        uses, prod = {}, {0: -1}
        for i, op in enumerate(self.fops):
            for b in op.ins:
                uses[b] = uses.get(b, 0) + 1
            prod[op.out] = i
        for b, _ in self.outs:
            uses[b] = uses.get(b, 0) + 1
        out = {}
        for op in self.fops:
            if op.kind != "add" or (op.flags and not fuse_adds_bf16):
                continue
            for conv_b, other in ((op.b, op.a), (op.a, op.b)):
                j = prod.get(conv_b, -1)
                if j >= 0 and self.fops[j].kind == "conv" and uses.get(conv_b) == 1 and prod.get(other, 1 << 30) < j \
                        and id(self.fops[j]) not in out:
                    out[id(self.fops[j])] = (op, other)
                    break
        return out

    # ---- bookkeeping -------------------------------------------------------------------------------------------
    def signature(self, plan):
        return (plan.arena.data_ptr(), tuple(p.data_ptr() for p in self.params),
                tuple(m.running_mean.data_ptr() for m in self.bns), tuple(m.running_var.data_ptr() for m in self.bns))

    def _level(self, sp):
        i = self.lvl.get(sp)
        if i is None:
            i = self.lvl[sp] = len(self.levels)
            self.levels.append(sp)
        return i

    def _new(self, lvl, planes, dt):
        self.fbufs.append((lvl, planes, dt))
        return len(self.fbufs) - 1

    def _param(self, p):
        """one gradient slot per parameter, STORED by its one dW / BatchNorm-backward launch: a parameter used by two
        operators of the graph (tied weights) would need a sum there, so such a network goes through the modules"""
        i = self.pidx.get(id(p))
        if i is not None:
            raise Unsupported("a parameter shared by two operators (tied weights)")
        i = self.pidx[id(p)] = len(self.params)
        self.params.append(p)
        return i

    def _book(self, kind, key, args):
        i = self.bidx.get((kind, key))
        if i is None:
            i = self.bidx[(kind, key)] = len(self.books)
            self.books.append((kind, key, args))
        return i

    # ---- symbolic forward: one handler per module type ----------------------------------------------------------
    def run(self, m, x):
        if isinstance(m, ConcatTable):
            return [self.run(c, x) for c in m._modules.values()]
        if isinstance(m, AddTable):
            return self.add(x)
        if isinstance(m, Sequential):
            for c in m._modules.values():
                x = self.run(c, x)
            return x
        if isinstance(m, Identity):
            return x
        if isinstance(m, BatchNormalization):
            return self.bn(m, x)
        if isinstance(m, SubmanifoldConvolution):
            return self.subm(m, x)
        if isinstance(m, Convolution):
            return self.conv(m, x)
        if isinstance(m, Deconvolution):
            return self.deconv(m, x)
        if isinstance(m, FullConvolution):       # creates a Metadata of its own: its level is not part of a static plan
            raise Unsupported("FullConvolution (it creates a new Metadata; run the network layer by layer)")
        raise Unsupported(type(m).__name__)

    def add(self, xs):
        """left-to-right sum (utils._sum_features)"""
        acc = xs[0]
        for t in xs[1:]:
            lvl, planes, dt = self.fbufs[acc[0]]
            assert self.fbufs[t[0]] == (lvl, planes, dt) and t[1] == acc[1]
            y = self._new(lvl, planes, dt)
            self.fops.append(Add("add", acc[0], t[0], y, lvl, planes, _bf(dt)))
            acc = (y, acc[1])
        return acc

    def cast(self, x, dtype):
        lvl, planes, dt = self.fbufs[x[0]]
        if dt == dtype:
            return x
        y = self._new(lvl, planes, dtype)
        self.fops.append(Cast("cast", x[0], y, lvl, planes, F_TO_BF16 if dtype == BF16 else 0))
        return (y, x[1])

    def bn(self, m, x):
        if not (m.training or m.track_running_stats):
            raise Unsupported("BatchNormalization on batch statistics in evaluation mode")
        lvl, planes, dt = self.fbufs[x[0]]
        assert planes == m.nPlanes, (planes, m.nPlanes)
        y = self._new(lvl, planes, dt)
        st = self.stat_floats
        self.stat_floats += 2 * planes
        w = m.weight if m.affine else None
        b = m.bias if m.affine else None
        if m.affine:
            self._param(w)
            self._param(b)
        self.bns.append(m)
        self.bn_floats = max(self.bn_floats, int(self.lib.aabr_bn_scratch_floats(planes)))
        self.max_planes = max(self.max_planes, planes)
        self.fops.append(Bn("bn", x[0], y, lvl, planes, _bf(dt), 1 if m.training else 0, float(m.eps), float(m.momentum),
                            float(m.leakiness), st, _dp(m.running_mean), _dp(m.running_var), _dp(w), _dp(b), m))
        return (y, x[1])

    def _conv_common(self, m, x, out_spatial, book, side_fwd, side_din, din_flags, side_dw):
        if hasattr(m, "bias") or getattr(m, "groups", 1) != 1:
            raise Unsupported("convolution with bias / groups")
        lvl, planes, dt = self.fbufs[x[0]]
        assert planes == m.nIn, (planes, m.nIn)
        w = m.weight
        if id(w) not in self.packs or not w.is_contiguous():
            raise Unsupported("weight packs missing (FPN_Net.prepack_weights)")
        lo = self._level(out_spatial)
        y = self._new(lo, m.nOut, dt)
        self._param(w)
        self.macs.append((book, w))
        self.hidden.append((lo, m.nOut))
        pf, pt = self.packs[id(w)]
        self.fops.append(Conv("conv", x[0], y, lvl, lo, m.nIn, m.nOut, book, side_fwd, w.data_ptr(), pf,
                              side_din, din_flags, side_dw, pt, m))
        return (y, out_spatial)

    def subm(self, m, x):
        fs = SCN._key(m.filter_size)
        book = self._book("s", x[1] + fs, (x[1], m.filter_size))
        return self._conv_common(m, x, x[1], book, 0, 0, 1 | 2, 0)

    def conv(self, m, x):
        fs, st = SCN._key(m.filter_size), SCN._key(m.filter_stride)
        osz = tuple((i - f) // s + 1 for i, f, s in zip(x[1], fs, st))
        assert all((o - 1) * s + f == i for o, s, f, i in zip(osz, st, fs, x[1])), (x[1], osz, fs, st)
        book = self._book("c", x[1] + fs + st, (x[1], osz, m.filter_size, m.filter_stride))
        return self._conv_common(m, x, osz, book, 0, 1, 1, 0)

    def deconv(self, m, x):
        fs, st = SCN._key(m.filter_size), SCN._key(m.filter_stride)
        osz = tuple((i - 1) * s + f for i, f, s in zip(x[1], fs, st))
        book = self._book("c", osz + fs + st, (osz, x[1], m.filter_size, m.filter_stride))
        return self._conv_common(m, x, osz, book, 1, 0, 1, 1)

    # ---- the backward list for one pattern of incoming gradients -------------------------------------------------
    def backward(self, pattern, need_dx):
        key = (pattern, need_dx, tuple(p.requires_grad for p in self.params))
        b = self._bwd.get(key)
        if b is None:
            b = self._bwd[key] = self._make_backward(pattern, need_dx)
        return b

    def _make_backward(self, pattern, need_dx):
        gbufs, ops = [], []
        poff, ptotal = {}, 0
        filled = [0]       # filled[i]: floats of the parameter-gradient buffer that are final once ops[:i] have run

        def put(op):
            ops.append(op)
            filled.append(ptotal)

        def gnew(lvl, planes, dt):
            gbufs.append((lvl, planes, dt))
            return (G, len(gbufs) - 1)

        def pslot(p):
            """byte offset of p's gradient slot; slots are laid out in the order their records appear"""
            nonlocal ptotal
            i = self.pidx[id(p)]
            if i not in poff:
                poff[i] = ptotal
                ptotal += _slot_floats(p)
            return poff[i] * 4

        acc = {}           # forward buffer -> the gradient accumulated so far (contributions in arrival order:
                           # autograd's order, the consumer created last delivers first; ((c0 + c1) + c2) ...)

        def arrive(b, ref, summed=False):
            """an existing gradient buffer contributes to forward buffer b (`summed`: the launch that wrote it has
            already added what had arrived so far)"""
            cur = acc.get(b)
            if cur is None or summed:
                acc[b] = ref
                return
            lvl, planes, dt = self.fbufs[b]
            s = gnew(lvl, planes, dt)
            put(Add("add", cur, ref, s, lvl, planes, _bf(dt)))
            acc[b] = s

        def riding(x, flg):
            """the gradient that has arrived at forward buffer x so far, when the launch that produces the next
            contribution can add it in its write-out (the backward side of `fuse_adds`); else None"""
            return acc.get(x) if (fuse_adds and (not flg or fuse_adds_bf16)) else None

        for k, ((b, _), has) in enumerate(zip(self.outs, pattern)):
            if has:
                arrive(b, (E, k))

        for op in reversed(self.fops):
            gy = acc.get(op.out)
            if gy is None:               # no incoming gradient depends on what this op wrote
                continue
            kind = op.kind
            if kind == "add":
                _, a_, b_, y, lvl, planes, flg = op
                arrive(a_, gy)           # same order as autograd's AddBackward: first operand, then second
                arrive(b_, gy)
            elif kind == "cast":
                _, x, y, lvl, planes, flg = op
                dtx = self.fbufs[x][2]
                gx = gnew(lvl, planes, dtx)
                put(Cast("cast", gy, gx, lvl, planes, F_TO_BF16 if dtx == BF16 else 0))
                arrive(x, gx)
            elif kind == "bn":
                _, x, y, lvl, planes, flg, train, eps, mom, leak, st, p_rm, p_rv, p_w, p_b, m = op
                gx = gnew(lvl, planes, self.fbufs[x][2])
                pw = pslot(m.weight) if m.affine and m.weight.requires_grad else -1
                pb = pslot(m.bias) if m.affine and m.bias.requires_grad else -1
                res = riding(x, flg)     # the sum with what has arrived so far rides in the apply pass
                put(BnBwd("bn", x, gx, y, gy, lvl, planes, flg, leak, st, p_w, pw, pb, p_b, res))
                arrive(x, gx, res is not None)
            else:
                _, x, y, lvl, lo, n_in, n_out, book, side_fwd, p_w, pf, side_din, din_flags, side_dw, pt, m = op
                dt = self.fbufs[x][2]
                flg = _bf(dt)
                if x != 0 or need_dx:
                    gx = gnew(lvl, n_in, dt)
                    res = riding(x, flg)
                    tmp = gnew(lvl, n_in, dt) if res is not None else None   # used when the launch is not a wide one
                    # the launch reads d_out (n_out planes) and writes d_in (n_in planes)
                    put(Din("din", gy, gx, lo, lvl, n_out, n_in, book, side_din, din_flags, p_w, pt, flg, res, tmp,
                            _one_rule(m, True)))
                    arrive(x, gx, res is not None)
                if m.weight.requires_grad:
                    put(Dw("dw", x, gy, lo, n_in, n_out, book, side_dw, pslot(m.weight), flg))
        # input-gradient records whose write-out a BatchNorm backward record may ask for its statistics: the next record,
        # weight gradients aside, is that BatchNorm, reading their d_in
        claimed = set()
        for i, op in enumerate(ops):
            if op.kind == "din":
                nxt = next((o for o in ops[i + 1:] if o.kind != "dw"), None)
                if nxt is not None and nxt.kind == "bn" and nxt.gy == op.gx and nxt.planes == op.n_out:
                    claimed.add(i)
        gx0 = acc.get(0) if need_dx else None
        return {"gbufs": gbufs, "ops": ops, "poff": poff, "ptotal": ptotal, "gx0": gx0, "filled": filled,
                "claimed": claimed}


def _one_rule(m, din):
    """0 when the rule book of this module's forward (`din` False) or input-gradient launch may give an output row several
    rules or none; 1 when it gives every output row exactly one, by construction: what entitles the caller to ask
    `SCN.single_route`; 2 for the input gradient of a Convolution with filter == stride (every fine row has one parent),
    which entitles it to `SCN.single_bwd_stats_route` ALONE: without statistics to deliver that launch stays where it was"""
    if isinstance(m, SubmanifoldConvolution):
        return int(m.filter_volume == 1)
    if isinstance(m, Deconvolution) and not din:
        return int(SCN._key(m.filter_size) == SCN._key(m.filter_stride))
    if isinstance(m, Convolution) and din:
        return 2 if SCN._key(m.filter_size) == SCN._key(m.filter_stride) else 0
    return 0


def _offsets(bufs, V, first=0):
    """arena offsets of [rows(level), planes] matrices; bufs[:first] are not in the arena"""
    offs, total = [0] * len(bufs), 0
    for i in range(first, len(bufs)):
        offs[i] = total
        total += _bytes(bufs[i], V)
    return offs, total


class _Pass(object):
    """one pass through the graph: the template bound to a scene"""

    def __init__(self, tpl, md, x):
        self.t, self.md, self.x = tpl, md, x
        self.dev = x.device
        self.lib = tpl.lib
        self.V = V = [md.grids[sp].V for sp in tpl.levels]
        assert V[tpl.fbufs[0][0]] == x.size(0)
        # rule books of the pass (built by FPN_Net._prebuild_geometry; looked up by their cache keys)
        bk = []
        for kind, key, args in tpl.books:
            tb = (md.submanifold if kind == "s" else md.rulebooks).get(key)
            if tb is None:
                tb = md.getSubmanifoldRuleBook(*args) if kind == "s" else md.getRuleBook(*args)
            bk.append((tb.out, tb.inn if tb.inn is not None else tb.out, tb))
        self.books = bk
        self.route = functools.lru_cache(maxsize=None)(SCN.conv_route)   # {launch shape: its ConvRoute} of the pass
        self.single = functools.lru_cache(maxsize=None)(SCN.single_route)
        self.single_bwd_stats = functools.lru_cache(maxsize=None)(SCN.single_bwd_stats_route)
        self._tmp = []
        self._tail_tmp = []                # the offset-split scratch of tail records: dropped after the join, not before
        self._ticket = 0                   # the tail of this pass's forward list (aabr_plan_run_tail), 0 = none / joined
        self._strm = None

    def join_tail(self):
        """the stream the pass ran on (and the current one) waits for the pass's tail; the ticket goes back.  From any
        thread, any number of times."""
        with _tails_lock:
            tk, self._ticket = self._ticket, 0
            if tk:
                _tails[:] = [p for p in _tails if p is not self]
        if not tk:
            return
        with torch.cuda.device(self.dev):
            cur = stream()
            check(self.lib.aabr_plan_tail_join(tk, self._strm))
            if cur != self._strm:
                check(self.lib.aabr_plan_tail_join(tk, cur))
            check(self.lib.aabr_plan_tail_release(tk))
        self._tail_tmp = []

    def fwd_route(self, op):
        """(route, fused add or None) of a forward convolution record: `SCN.single_route` first where the module's rule
        book has one rule per output row, then `SCN.conv_route`; the add behind the convolution rides in the write-out
        when the route takes a residual"""
        _, x, y, lvl, lo, n_in, n_out, book, side, p_w, pf, side_din, din_flags, side_dw, pt, m = op
        t, V = self.t, self.V
        fz = t.fuse.get(id(op))
        g, bfx = self.books[book][side], t.fbufs[x][2] == BF16
        r = None
        if _one_rule(m, False) == 1:
            r = self.single(n_in, n_out, V[lvl], V[lo], g.vol, bfx, conv_bn_stats and id(op) in t.stat_claims)
        if r is None and fz is not None:
            r = self.route(n_in, n_out, V[lvl], V[lo], g.vol, bfx, residual=True)
        if fz is not None and r.takes_residual:
            return r, fz
        if r is None or r.kind != "single":
            r = self.route(n_in, n_out, V[lvl], V[lo], g.vol, bfx)
        return r, None

    def conv_launch(self, route, buf, off, src, rows_in, n_in, dst, rows_out, n_out, gather, p_w, p_pack, flags, xf=0,
                    res=0):
        """the record of the launch SCN._conv_fwd makes for a prepacked weight along `route`; returns the new write
        offset and the BatchNorm partial sums its write-out can form for the record behind it (the narrow kernel's
        with AABR_PLAN_NARROW_STATS only), or 0"""
        assert route.takes_residual or not res
        if route.kind is None:
            return off, 0
        xf |= F_BF16 if route.bf16 else 0
        # the tile kernel: p3 the raw weight next to the pack
        kind, cflags, p3, wpack, tile_rows, parts, scratch = K_CONV, flags | 4, p_w, p_pack, 0, 0, 0
        if route.kind == "narrow":        # from the gather table, raw weights
            kind, cflags, wpack = K_NARROW, flags & 3, 0
        elif route.kind == "single":      # one rule per output row: from the offset pairs, residual in the write-out
            kind, cflags, p3 = K_SINGLE, flags & 3, res
        elif route.kind in ("wide", "split"):
            kind, cflags, p3, tile_rows = K_WIDE, flags & 3, res, route.tile_rows
            if route.kind == "split":     # coarse map: the wide kernel cut into parts over the filter offsets
                # its own scratch per record: the list is launched later in ONE call, so a shared grow-only workspace
                # could be reallocated under records already written (the allocator frees it in stream order once the
                # pass's next list is built)
                tmp = torch.empty(route.parts * rows_out * n_out, dtype=torch.float32, device=self.dev)
                (self._tail_tmp if xf & F_TAIL else self._tmp).append(tmp)
                kind, parts, scratch = K_WSPLIT, route.parts, tmp.data_ptr()
        R.CONV.pack_into(buf, off, kind, xf, n_in, n_out, gather.vol, cflags, tile_rows, parts, rows_in, rows_out,
                         src, dst, route.stream(gather).data_ptr(), p3, 0, wpack, scratch)
        return off + R.SIZE, route.stats_parts(rows_out) if (narrow_stats or route.kind != "narrow") else 0

    def _records(self, emit):
        """[(op, record flags, route, fused add)]: the records of a forward list, in the order of `emit`.  The one round
        of route decisions of a pass: a convolution gets its `fwd_route`; an add that rides in its convolution's
        write-out is not a record, the convolution writes the add's buffer (the add is the convolution's only reader and
        stands behind it in every emission order)."""
        out, skip = [], set()
        for op, xf in emit:
            if op.kind == "conv":
                r, fz = self.fwd_route(op)
                if fz is not None:
                    skip.add(id(fz[0]))
                out.append((op, xf, r, fz))
            elif id(op) not in skip:
                out.append((op, xf, None, None))
        return out

    def _live_offsets(self, records):
        """arena offsets for a pass nobody will differentiate (torch.no_grad): a buffer's bytes are handed on once its
        last reader has been recorded -- first fit over a free list, in record order (one stream) -- instead of every
        activation of the network living until the pass object dies.  Returns (offsets, total, total without reuse)."""
        t, V = self.t, self.V
        fbufs = t.fbufs
        # (buffers read, buffer written) per record
        steps = [(op.ins, op.out) if fz is None else ((op.x, fz[1]), fz[0].out) for op, _, _, fz in records]
        last = {}
        for i, (rd, _) in enumerate(steps):
            for b in rd:
                last[b] = i
        for b, _ in t.outs:
            last[b] = len(steps)
        size = lambda b: _bytes(fbufs[b], V)
        offs, free, top = [0] * len(fbufs), [], 0      # free: [offset, bytes], sorted by offset
        dying = {}
        for b, i in last.items():
            dying.setdefault(i, []).append(b)
        for i, (rd, wr) in enumerate(steps):
            need = size(wr)
            for f in free:                               # first fit
                if f[1] >= need:
                    offs[wr] = f[0]
                    f[0] += need
                    f[1] -= need
                    break
            else:
                offs[wr] = top
                top += need
            free = [f for f in free if f[1] > 0]
            if wr not in last:                           # written, never read, not an output: free at once
                dying.setdefault(i, []).append(wr)
            for b in dying.get(i, ()):                   # read for the last time by this record
                if b == 0:
                    continue                             # the graph input is not in the arena
                free.append([offs[b], size(b)])
            free.sort()
            merged = []
            for f in free:                               # coalesce neighbours
                if merged and merged[-1][0] + merged[-1][1] == f[0]:
                    merged[-1][1] += f[1]
                else:
                    merged.append(f)
            free = merged
        return offs, top, sum(size(b) for b in range(1, len(fbufs)))

    def forward(self, keep=True, tail=False):
        """`keep` False (no autograd): the arena is packed by liveness (`_live_offsets`); `tail`: a training pass, whose
        unconsumed records may go to the tail stream (`plan_tail`)"""
        try:
            return self._forward(keep, tail)
        except BaseException:
            self.lib.aabr_plan_drain()     # never leave parts of a failed pass in the launcher's queue
            raise

    def _forward(self, keep, tail=False):
        t, V = self.t, self.V
        self.join_tail()                   # (a pass object run twice)
        self._tmp = []
        # the tail: one slot per activation (nothing of the arena is handed on) and one call per list (the launcher
        # thread has nobody to hand a ticket to)
        use_tail = bool(tail and keep and plan_tail and t.emit_tail is not None and not pipeline_records)
        records = self._records(t.emit_tail if use_tail else [(op, 0) for op in t.fops])
        if keep:
            offs, total = _offsets(t.fbufs, V, 1)
        else:
            offs, total, flat = self._live_offsets(records)
            stats["arena_bytes_packed"], stats["arena_bytes_flat"] = total, flat
        self.arena = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        self.stat = torch.empty(max(t.stat_floats, 1), dtype=torch.float32, device=self.dev)
        base, sbase = self.arena.data_ptr(), self.stat.data_ptr()
        self.offs = offs
        A = self.A = [base + o for o in offs]
        A[0] = self.x.data_ptr()
        bnws = _hip.workspace("bn", t.bn_floats, torch.float32, self.dev).data_ptr() if t.bn_floats else 0
        # the tail's BatchNorm records run beside the backward list's, which use "bn" on this same stream key
        bnws_tail = _hip.workspace("bn_tail", t.bn_floats, torch.float32, self.dev).data_ptr() \
            if (use_tail and t.bn_floats) else 0
        SZ, off = R.SIZE, 0
        buf = bytearray(len(t.fops) * SZ)
        stats_patch, stats_at = R.CONV_STATS
        books = self.books
        # BatchNorm statistics from the producing convolution's write-out: a training-mode BatchNorm that is the NEXT
        # record on its stream after the k_conv_cs launch that wrote its input gets the per-tile partial sums from
        # that launch (record p6 -> BatchNorm p9) and skips its own statistics pass over the matrix
        last = {0: None, F_TAIL: None}     # per stream: (buffer index written, record offset, parts, planes)
        cstat = {}
        cross = t.cross if use_tail else {}
        cross_convs, xlast = set(cross.values()), {}
        part, start, strm = pipeline_records * SZ, 0, stream()
        for op, xf, r, fz in records:
            if part and off - start >= part:
                # records up to `safe` are final (a convolution record stays open while the BatchNorm behind it may
                # still claim its write-out for the statistics)
                safe = off
                for lw in last.values():
                    if lw is not None and lw[1] < safe:
                        safe = lw[1]
                start = self._submit(buf, start, safe, strm)
            kind = op.kind
            sk = xf & F_TAIL
            if kind == "conv":
                _, x, y, lvl, lo, n_in, n_out, book, side, p_w, pf, side_din, din_flags, side_dw, pt, m = op
                g, off0, res = books[book][side], off, 0
                if fz is not None:
                    add_op, other = fz           # out = conv + other, written where the add would have written
                    y, res = add_op.out, A[other]
                off, nparts = self.conv_launch(r, buf, off, A[x], V[lvl], n_in, A[y], V[lo], n_out, g, p_w, pf, 0,
                                               xf, res)
                last[sk] = (y, off0, nparts, n_out) if nparts else None
                if id(op) in cross_convs:
                    xlast[id(op)] = last[sk]
                continue
            elif kind == "bn":
                _, x, y, lvl, planes, flg, train, eps, mom, leak, st, p_rm, p_rv, p_w, p_b, m = op
                if V[lvl]:
                    parts, nparts, lw = 0, 0, last[sk]
                    wk = sk
                    if id(op) in cross:  # the convolution ran on the caller's stream: a buffer of this pair's own
                        lw, wk = xlast.get(cross[id(op)]), "_cross%d" % len(cstat)
                    if conv_bn_stats and train and lw is not None and lw[0] == x and lw[3] == planes:
                        nparts = lw[2]
                        ws = cstat.get(wk)
                        if ws is None:   # one buffer per stream: written by the convolution, read by the very next record
                            ws = cstat[wk] = _hip.workspace("conv_stats%s" % wk, (max(V) // 64 + 1) * 2 * t.max_planes,
                                                            torch.float64, self.dev).data_ptr()
                        parts = ws
                        stats_patch.pack_into(buf, lw[1] + stats_at, ws)      # the convolution record's `stats`
                    R.BN_FWD.pack_into(buf, off, K_BNF, flg | xf, planes, train, nparts, eps, mom, leak, V[lvl], A[x], A[y],
                                       sbase + st * 4, sbase + (st + planes) * 4, p_rm, p_rv, p_w, p_b,
                                       bnws_tail if sk else bnws, parts)
                    off += SZ
            elif kind == "add":
                _, a_, b_, y, lvl, planes, flg = op
                R.ADD.pack_into(buf, off, K_ADD, flg | xf, V[lvl] * planes, A[a_], A[b_], A[y])
                off += SZ
            else:
                _, x, y, lvl, planes, flg = op
                R.CAST.pack_into(buf, off, K_CAST, flg | xf, V[lvl] * planes, A[x], A[y])
                off += SZ
            last[sk] = None
        if debug_kinds is not None:
            debug_kinds.append(("fwd", R.kinds(buf, off)))
        if part:                                   # everything issued: the caller's next launches queue behind the pass
            self._submit_last(buf, start, off, strm)
        elif off and use_tail:
            ticket = ctypes.c_uint64(0)
            self._strm = strm
            check(self.lib.aabr_plan_run_tail(bytes(buf[:off]), off // SZ, strm, ctypes.byref(ticket)))
            if ticket.value:
                with _tails_lock:
                    self._ticket = ticket.value
                    _tails.append(self)
        elif off:
            check(self.lib.aabr_plan_run(bytes(buf[:off]), off // SZ, strm))
        return [_view(self.arena, offs[b], t.fbufs[b], V) for b, _ in t.outs]

    def _submit(self, buf, start, safe, strm):
        """hand records [start, safe) of `buf` (byte offsets), which are final, to the launcher thread, more to come;
        returns where the next part starts"""
        if safe <= start:
            return start
        check(self.lib.aabr_plan_submit(bytes(buf[start:safe]), (safe - start) // R.SIZE, strm, 1))
        return safe

    def _submit_last(self, buf, start, off, strm):
        """hand the last part [start, off) of a list to the launcher thread and wait until it has issued everything"""
        check(self.lib.aabr_plan_submit(bytes(buf[start:off]), (off - start) // R.SIZE, strm, 0))
        check(self.lib.aabr_plan_drain())

    def buffer(self, b):
        """forward buffer `b` of this pass as a tensor view into the arena (tests)"""
        self.join_tail()                   # an unconsumed stage's buffer is written on the tail stream
        return _view(self.arena, self.offs[b], self.t.fbufs[b], self.V)

    def bn_outputs(self):
        """{BatchNorm module: its output matrix of this pass} (tests: the compiled graph runs no module hooks)"""
        return {op.module: self.buffer(op.out) for op in self.t.fops if op.kind == "bn" and self.V[op.lvl]}

    def backward(self, gouts, need_dx):
        try:
            return self._backward(gouts, need_dx)
        except BaseException:
            self.lib.aabr_plan_drain()
            raise

    def _backward(self, gouts, need_dx):
        t, V, A = self.t, self.V, self.A
        self._tmp = []
        gouts = [g.contiguous() if g is not None else None for g in gouts]
        bw = t.backward(tuple(g is not None for g in gouts), need_dx)
        gbufs, bops = bw["gbufs"], bw["ops"]
        offs, total = _offsets(gbufs, V)
        garena = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        # pieces of the list for the data-parallel hook: cut after every len/S-th record; parameter gradients are laid
        # out in the order their records appear (pslot), so the ones a piece completes form one slice of `gparams`
        nseg = grad_segments if (grad_segments > 1 and on_grads_ready is not None) else 1
        # the data-parallel hook all-reduces slices of this buffer, 64-float padding between the slots included
        gparams = (torch.zeros if nseg > 1 else torch.empty)(max(bw["ptotal"], 1), dtype=torch.float32, device=self.dev)
        gbase, pbase, sbase = garena.data_ptr(), gparams.data_ptr(), self.stat.data_ptr()
        AD = (A, [gbase + o for o in offs], [_dp(g) for g in gouts])
        for (b, _), g in zip(t.outs, gouts):
            if g is not None:
                lvl, planes, dt = t.fbufs[b]
                assert g.dtype == dt and g.numel() == V[lvl] * planes
        books = self.books
        # weight-gradient scratch: the largest of the pass
        dws, dwmc = 0, []
        for op in bops:
            if op.kind == "dw":
                mc = books[op.book][op.side].max_chunks(op.n_in, op.n_out)
                dwmc.append(mc)
                dws = max(dws, mc * op.n_in * op.n_out)
        dwmc.reverse()
        dwws = _hip.workspace("dw", dws, torch.float32, self.dev).data_ptr() if dws else 0
        bnws = _hip.workspace("bn", t.bn_floats, torch.float32, self.dev).data_ptr() if t.bn_floats else 0
        SZ, off = R.SIZE, 0
        buf = bytearray((len(bops) * 2 + 1) * SZ)
        (flag_patch, flag_at), (bn_patch, bn_at) = R.CONV_BWD_STATS
        dw_side = F_SIDE if dw_side_stream else 0
        cut = [(len(bops) * (q + 1)) // nseg for q in range(nseg)] if nseg > 1 else []
        inv = sorted((o, i) for i, o in bw["poff"].items()) if nseg > 1 else []
        seg_no, next_inv = 0, 0

        def grad(i, o):
            """the gradient of parameter i: its slot at float offset `o` of the pass's gradient buffer"""
            return gparams[o:o + t.params[i].numel()].view_as(t.params[i])

        def hand_over(piece, upto):
            """the data-parallel hook receives, as piece `piece`, the parameters whose slots lie below float offset `upto`
            and have not been handed over yet: final, since every record that writes below `upto` has been issued"""
            nonlocal next_inv
            pairs = []
            while next_inv < len(inv) and inv[next_inv][0] < upto:
                o, i = inv[next_inv]
                pairs.append((t.params[i], grad(i, o)))
                next_inv += 1
            if pairs:
                lo = pairs[0][1].data_ptr() - pbase
                on_grads_ready(piece, nseg, gparams[lo // 4:upto], pairs)

        claimed = bw["claimed"]          # input-gradient records a BatchNorm backward record may ask for its statistics
        last_din, bstat = None, None     # the last wide input-gradient record of the main stream / statistics workspace
        part, start, strm = (pipeline_records * SZ if nseg == 1 else 0), 0, stream()
        for op_no, op in enumerate(bops):
            if part and off - start >= part:
                # (the last input-gradient record may still get the statistics)
                start = self._submit(buf, start, last_din[1] if last_din is not None else off, strm)
            if nseg > 1 and seg_no < nseg - 1 and op_no == cut[seg_no]:
                last_din = None          # its record has been handed over
                if off:
                    check(self.lib.aabr_plan_run(bytes(buf[:off]), off // SZ, stream()))
                    off = 0
                hand_over(seg_no, bw["filled"][op_no])
                seg_no += 1
            kind = op.kind
            if kind == "din":
                _, gy, gx, lo, lvl, n_in, n_out, book, side, flags, p_w, pt, flg, res, tmp, one_rule = op
                g = books[book][side]
                last_din, bf = None, flg == F_BF16
                r = None
                claim = conv_bn_bwd_stats and op_no in claimed   # a BatchNorm backward record may ask for its statistics
                if one_rule and claim:   # k_conv_single's backward-statistics form: one part per chunk of the pair list
                    r = self.single_bwd_stats(n_in, n_out, V[lo], V[lvl], g.vol, bf)
                    if r is not None:    # (holds from 32,768 rows on: V / 256 + vol <= V / 64 + 1)
                        assert r.parts <= max(V) // 64 + 1, "the conv_bwd_stats workspace does not hold this launch's parts"
                if r is None and one_rule == 1:
                    r = self.single(n_in, n_out, V[lo], V[lvl], g.vol, bf, claim)
                if r is None:
                    r = self.route(n_in, n_out, V[lo], V[lvl], g.vol, bf, residual=res is not None)
                if res is None or r.takes_residual:
                    off0 = off
                    off, nparts = self.conv_launch(r, buf, off, AD[gy[0]][gy[1]], V[lo], n_in, AD[gx[0]][gx[1]],
                                                   V[lvl], n_out, g, p_w, pt, flags, 0,
                                                   AD[res[0]][res[1]] if res is not None else 0)
                    if nparts:
                        last_din = (gx, off0, nparts, n_out)
                else:                    # not a wide launch: d_in into the spare buffer, then the sum
                    off, _ = self.conv_launch(self.route(n_in, n_out, V[lo], V[lvl], g.vol, bf), buf, off,
                                              AD[gy[0]][gy[1]], V[lo], n_in, AD[tmp[0]][tmp[1]], V[lvl], n_out, g, p_w,
                                              pt, flags)
                    R.ADD.pack_into(buf, off, K_ADD, flg, V[lvl] * n_out, AD[res[0]][res[1]], AD[tmp[0]][tmp[1]],
                                    AD[gx[0]][gx[1]])
                    off += SZ
            elif kind == "dw":
                _, x, gy, lo, n_in, n_out, book, side, pg, flg = op
                g = books[book][side]
                R.CONV_DW.pack_into(buf, off, K_DW, flg | dw_side, n_in, n_out, g.vol, V[lo], dwmc.pop(), A[x],
                                    AD[gy[0]][gy[1]], g.pairs().data_ptr(), pbase + pg, 0, dwws)
                off += SZ
            elif kind == "bn":
                _, x, gx, y, gy, lvl, planes, flg, leak, st, p_w, pw, pb, p_b, res = op
                if V[lvl]:
                    parts, nparts, ld = 0, 0, last_din
                    if (conv_bn_bwd_stats and ld is not None and ld[0] == gy and ld[3] == planes
                            and (flg == F_BF16 or (not flg and leak >= 0.0))):
                        # the BatchNorm's d_out was written by the wide-kernel input-gradient launch right before it (the
                        # weight-gradient record in between runs on the second stream): that launch's write-out forms the
                        # backward statistics (the record's bwd_stats = 1, leak, stats, then the BatchNorm's input and
                        # coefficients: save_invstd in fp32 storage, the BatchNorm's stored output in bf16)
                        nparts = ld[2]
                        if bstat is None:
                            bstat = _hip.workspace("conv_bwd_stats", (max(V) // 64 + 1) * 2 * t.max_planes,
                                                   torch.float64, self.dev).data_ptr()
                        parts = bstat
                        flag_patch.pack_into(buf, ld[1] + flag_at, 1, leak)
                        bn_patch.pack_into(buf, ld[1] + bn_at, bstat, A[x], sbase + st * 4,
                                           A[y] if flg == F_BF16 else sbase + (st + planes) * 4, p_w, p_b)
                    R.BN_BWD.pack_into(buf, off, K_BNB, flg, planes, nparts, leak, V[lvl], parts, A[x], AD[gx[0]][gx[1]],
                                       A[y], AD[gy[0]][gy[1]], sbase + st * 4, sbase + (st + planes) * 4, p_w,
                                       pbase + pw if pw >= 0 else 0, pbase + pb if pb >= 0 else 0, bnws, p_b,
                                       AD[res[0]][res[1]] if res is not None else 0)
                    off += SZ
                last_din = None
            elif kind == "add":
                _, a_, b_, s, lvl, planes, flg = op
                R.ADD.pack_into(buf, off, K_ADD, flg, V[lvl] * planes, AD[a_[0]][a_[1]], AD[b_[0]][b_[1]], AD[s[0]][s[1]])
                off += SZ
                last_din = None
            else:
                last_din = None
                _, gy, gx, lvl, planes, flg = op
                R.CAST.pack_into(buf, off, K_CAST, flg, V[lvl] * planes, AD[gy[0]][gy[1]], AD[gx[0]][gx[1]])
                off += SZ
        if debug_kinds is not None:      # (with grad_segments > 1: the last piece only)
            debug_kinds.append(("bwd", R.kinds(buf, off)))
        if debug_bwd_stats is not None:  # bwd_stats == 1 on a convolution record: its write-out delivers backward statistics
            debug_bwd_stats.append([(k, R.conv_bwd_stats(buf, i * SZ)) for i, k in enumerate(R.kinds(buf, off))])
        # The forward list's tail is joined HERE, by the last record of the (last piece of the) backward list: behind it
        # come the gradient hand-over and the caller's update, which rewrites the BatchNorm parameters and running
        # statistics the tail's records read and write.
        tk = self._ticket
        if tk and not part:
            R.TAIL_JOIN.pack_into(buf, off, K_TAIL_JOIN, 0, tk)
            off += SZ
        if part:
            self._submit_last(buf, start, off, strm)
        elif off:
            check(self.lib.aabr_plan_run(bytes(buf[:off]), off // SZ, stream()))
        if tk:                            # enqueued on this stream by the record; `join_tail` covers the other cases
            self.join_tail()              # (pipelined backward, another stream than the forward's) and returns the ticket
        if nseg > 1:                      # the last piece's gradients
            hand_over(nseg - 1, bw["ptotal"])
        pgrad = [None] * len(t.params)
        for i, o in bw["poff"].items():
            pgrad[i] = grad(i, o)
        dx = None
        gx0 = bw["gx0"]
        if gx0 is not None:
            if gx0[0] == G:
                dx = _view(garena, offs[gx0[1]], t.fbufs[0], V)
            else:   # the graph input reached an output untouched: its gradient is the incoming one
                dx = gouts[gx0[1]]
        return dx, pgrad


class _GraphFunction(Function):
    @staticmethod
    def forward(ctx, ps, x, *params):
        res = ps.forward(tail=True)
        ctx.ps = ps
        ctx.need_dx = x.requires_grad
        # The backward list reads the transposed weight packs of THIS forward and recomputes the BatchNorm activation
        # signs from the BatchNorm parameters: state held by reference.  An in-place parameter update between forward
        # and backward (torch would raise "modified by an inplace operation") must not pass silently.
        ctx.versions = [p._version for p in params]
        ctx.params = params
        return tuple(res)

    @staticmethod
    def backward(ctx, *gouts):
        ps, ctx.ps = ctx.ps, None
        for p, v in zip(ctx.params, ctx.versions):
            if p._version != v:
                raise RuntimeError("a parameter of the compiled FPN_Net graph was modified in place between forward and "
                                   "backward (version %d -> %d): its packed copy / the BatchNorm coefficients the backward "
                                   "list reads belong to the forward pass" % (v, p._version))
        ctx.params = None
        dx, pgrad = ps.backward(gouts, ctx.need_dx)
        return (None, dx) + tuple(pgrad)


def _fpn_graph(net, ps, x):
    """forward_fpn (fpn_net.py:168-203), symbolically, in the module path's order"""
    n = len(net.m_downs)
    downs = []
    for m in net.m_downs:
        x = ps.run(m, x)
        downs.append(x)
    x = ps.run(net.m_shortcuts[-1], x)
    ups = [x]
    for k in range(net._top_down_levels()):      # all n - 1 stages (the reference), or up to the last consumed map
        j = n - 1 - k - 1
        x = ps.run(net.m_ups[k], x)
        sc = ps.run(net.m_shortcuts[j], downs[j])
        x = ps.add([x, sc])
        ups.append(ps.run(net.m_mergeds[k], x))
    rpn3d = [ups[i] for i in net.fpn_scales_from_top]
    rpn2d = [ps.run(net.convs_pro2d[i], rpn3d[i]) for i in range(len(rpn3d))]
    maps = rpn3d + rpn2d
    rpn = [maps[i] for i in net.rpn_3d_2d_selector]
    roi = [ups[i] for i in net.roi_scales_from_top]
    for i in range(len(rpn3d)):
        assert tuple(int(v) for v in net.rpn_map_sizes[i]) == rpn3d[i][1], (rpn3d[i][1], net.rpn_map_sizes[i])
    return rpn, roi


def _template(net, x_spatial, x_planes, plan):
    """the cached template of this network state (rebuilt when a mode flag, a parameter address, the weight-pack
    arena or the set of hooks changes)"""
    mods = net.__dict__.get("_graph_modules")
    if mods is None:
        mods = net.__dict__["_graph_modules"] = list(net.modules())
    mode = 0
    for m in mods:                 # any hook anywhere in the graph: the modules themselves must run
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
            raise Unsupported("hooks")
        mode = mode * 2 + (1 if m.training else 0)
    cache = net.__dict__.setdefault("_graph_templates", {})
    key = (x_spatial, x_planes, net.feature_dtype, mode, bool(net.prune_unused_levels))
    tpl = cache.get(key)
    if tpl is not None and tpl.sig == tpl.signature(plan):
        return tpl
    tpl = _Template(net, x_spatial, x_planes, net.feature_dtype, plan)
    tpl.sig = tpl.signature(plan)
    if len(cache) > 8:
        cache.clear()
    cache[key] = tpl
    return tpl


def run_fpn(net, net1):
    """FPN_Net.forward after layers_in: (rpn_maps, roi_maps) as SparseConvNetTensors, or None when the graph
    holds something the executor does not handle (the caller then runs the modules)."""
    import sparseconvnet
    x = net1.features
    plan = net.__dict__.get("_pack_plan")
    if x.dim() != 2 or x.size(0) == 0 or x.dtype != torch.float32 or not x.is_contiguous() or plan is None or \
            plan.dtype != net.feature_dtype or plan._ptrs is None:
        return None
    try:
        tpl = _template(net, SCN._key(net1.spatial_size), x.size(1), plan)
    except Unsupported:
        stats["fallbacks"] += 1
        return None
    train = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in tpl.params))
    ps = _Pass(tpl, net1.metadata, x)
    if debug_passes is not None:
        debug_passes.append(ps)
    if SCN.count_macs:
        for book, w in tpl.macs:
            sparseconvnet.forward_pass_multiplyAdd_count += SCN._macs(ps.books[book][2], w)
    sparseconvnet.forward_pass_hidden_states += sum(ps.V[lvl] * planes for lvl, planes in tpl.hidden)
    if train:
        feats = _GraphFunction.apply(ps, x, *tpl.params)
    else:
        feats = ps.forward(keep=not pack_inference_arena)
    stats["passes"] += 1
    res = []
    for (b, sp), f in zip(tpl.outs, feats):
        t = SparseConvNetTensor()
        t.metadata = net1.metadata
        t.spatial_size = torch.LongTensor(list(sp))
        t.features = f
        res.append(t)
    return res[:tpl.n_rpn], res[tpl.n_rpn:]
