"""A/B of the wide kernel's step loop on the bench's own rule books (4 x S80k @ 2 cm): knob WIDE_XOFF 0 (a step never
straddles a filter offset) against 1 (a step takes blocks (b, b + 1) of the tile's list), interleaved, device time per call
with the host taken out -- the 3x3x3 submanifold books of L1 and L2 (64 -> 64) and the filter-2 / stride-2 books L0 -> L1
(32 -> 64) and L1 -> L2 (64 -> 64), each forward and flipped (the input gradient) where the route is the wide kernel.  Per
book: rules, 16-pair blocks and their fill, steps per tile before and after (from the compiled stream read back), TFLOP/s,
and whether the two outputs are the same bits.
usage: [rounds] [pmc]     pmc: only the L1 submanifold book, four calls per knob value (for a counter pass of its own)"""
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np
import torch

import bench
import synth_scenes as S
import _hip
from _hip import ptr, stream, check
from sparseconvnet import SCN

dev = torch.device("cuda:0")
lib = _hip.load()
rounds = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
pmc = "pmc" in sys.argv[1:]
PLANES = [32, 64, 64, 128]
l, _ = S.make_batch(4, 80000, 9000, 50)
md = SCN.Metadata_3("brick")
sizes = [(4096 >> k, 4096 >> k, 512 >> k) for k in range(4)]
md.inputLayer(torch.LongTensor(sizes[0]), torch.as_tensor(l).to(dev), 4, 4, dev)
three, two = torch.LongTensor([3, 3, 3]), torch.LongTensor([2, 2, 2])
down = [md.getRuleBook(torch.LongTensor(sizes[k]), torch.LongTensor(sizes[k + 1]), two, two) for k in range(2)]


def steps(words, V, vol, T):
    """(rules, blocks, steps per tile never straddling an offset, steps per tile over the block list)"""
    w = words.cpu().numpy()
    nt = (V + T - 1) // T
    pre = w[:nt * (vol + 1)].reshape(nt, vol + 1).astype(np.int64)
    nb = np.diff(pre, axis=1)
    ent = w[nt * (vol + 1):nt * (vol + 1) + nt * (T // 16) * vol * 16].reshape(nt, -1, 16)
    rules = sum(int((ent[t, :pre[t, -1]] >= 0).sum()) for t in range(nt))
    return rules, int(nb.sum()), float(((nb + 1) // 2).sum(1).mean()), float(((pre[:, -1] + 1) // 2).mean())


def run(name, ga, rows_in, n_in, n_out, transposed):
    vol, V = ga.vol, ga.rows
    torch.manual_seed(1)
    x = torch.randn((rows_in, n_in), device=dev)
    W = torch.randn((vol, n_out, n_in) if transposed else (vol, n_in, n_out), device=dev)
    wpack = torch.empty(lib.aabr_conv_wpack_floats(vol, n_in, n_out), device=dev)
    check(lib.aabr_conv_pack_weights(ptr(W), vol, n_in, n_out, 1 if transposed else 0, ptr(wpack), stream()))
    flags = 3 if transposed else 0
    route = SCN.conv_route(n_in, n_out, rows_in, V, vol, False, residual=False)
    if route.kind != "wide":
        print("%-18s %7d rows %3d->%-3d | route %s: not the wide kernel" % (name, V, n_in, n_out, route.kind), flush=True)
        return
    blocks, T = route.stream(ga), route.tile_rows
    SCN.flush_geom()
    out = {v: torch.full((V, n_out), float("nan"), device=dev) for v in (0, 1)}
    call = {v: (lambda v=v: check(lib.aabr_conv_forward_wide(ptr(x), n_in, rows_in, ptr(out[v]), n_out, V, ptr(blocks), T, vol,
                                                             None, flags, ptr(wpack), stream()))) for v in (0, 1)}
    if pmc:
        for v in (0, 1):
            _hip.set_knob("WIDE_XOFF", v)
            for _ in range(4):
                call[v]()
            torch.cuda.synchronize()
        _hip.set_knob("WIDE_XOFF", None)
        print("%s: 4 calls with WIDE_XOFF 0, then 4 with 1 (%s)" % (name, lib.aabr_conv_last_variant().decode()))
        return
    t = {0: [], 1: []}
    for _ in range(rounds):
        for v in (0, 1):
            _hip.set_knob("WIDE_XOFF", v)
            t[v].append(bench.device_time(torch, call[v]) * 1e6)
    _hip.set_knob("WIDE_XOFF", None)
    same = torch.equal(out[0], out[1]) and bool(torch.isfinite(out[0]).all())
    rules, nblk, s0, s1 = steps(blocks, V, vol, T)
    flop = 2.0 * rules * n_in * n_out
    med = {v: float(np.median(t[v])) for v in t}
    print("%-18s %7d rows %3d->%-3d T %3d | %-16s | %8d rules %7d blocks fill %.2f | steps/tile %5.1f -> %5.1f | "
          "off %6.1f us [%6.1f .. %6.1f] %5.1f TF | on %6.1f us [%6.1f .. %6.1f] %5.1f TF | %+5.1f %% %s"
          % (name, V, n_in, n_out, T, lib.aabr_conv_last_variant().decode(), rules, nblk, rules / (16.0 * nblk), s0, s1,
             med[0], min(t[0]), max(t[0]), flop / med[0] / 1e6, med[1], min(t[1]), max(t[1]), flop / med[1] / 1e6,
             100.0 * (med[1] / med[0] - 1.0), "same bits" if same else "(DIFFERS)"), flush=True)


if pmc:
    tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[1]), three)
    run("subm L1", tb.out, tb.V_in, 64, 64, False)
    sys.exit(0)
print("wide kernel, fp32 storage, brick order; WIDE_XOFF 0 / 1 interleaved, %d rounds, median [min .. max] of bench.device_time" % rounds)
for k in (1, 2):
    tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), three)
    run("subm L%d" % k, tb.out, tb.V_in, PLANES[k], PLANES[k], False)
    run("subm L%d flipped" % k, tb.out, tb.V_in, PLANES[k], PLANES[k], True)
for k in (0, 1):
    tb = down[k]
    run("down L%d->L%d" % (k, k + 1), tb.out, tb.V_in, PLANES[k], PLANES[k + 1], False)
    run("down L%d<-L%d flipped" % (k, k + 1), tb.inn, tb.V_out, PLANES[k + 1], PLANES[k], True)
