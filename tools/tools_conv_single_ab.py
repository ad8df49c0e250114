"""A/B of the two routes of a one-rule-per-row convolution launch on the bench's own rule books (4 x S80k @ 2 cm, levels
L0 .. L8): the route SCN.conv_route gives it today (k_conv_cs, its offset split or the 64-row-tile kernels) against
k_conv_single at both chunk lengths -- the up-sampling deconvolutions (filter 2 / stride 2, 128 -> 128), the 1x1x1 laterals
forward (planes -> 128) and their input gradients (128 -> planes), each with a residual in the write-out where the route
takes one.  Device time per call with the host taken out; outputs compared bit for bit where both routes run k_conv_cs'
arithmetic.  With `bwd_stats`: only the statistics-carrying books -- the input gradients of the down-sampling convolutions
(filter 2 / stride 2), whose write-out forms the backward statistics of the BatchNorm in front: k_conv_cs with backward
statistics (aabr_conv_forward_wide_bwd_stats) against k_conv_single with them (aabr_conv_forward_single_bwd_stats), outputs
compared bit for bit, column totals of the statistics to 1e-12.  usage: [first_seen|brick] [bwd_stats]"""
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import torch

import bench
import synth_scenes as S
import _hip
from _hip import ptr, stream, check
from sparseconvnet import SCN

dev = torch.device("cuda:0")
lib = _hip.load()
order = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "bwd_stats" else "brick"
PLANES = [32, 64, 64, 128, 128, 128, 256, 256, 256]
l, _ = S.make_batch(4, 80000, 9000, 50)
md = SCN.Metadata_3(order)
sizes = [(4096 >> k, 4096 >> k, 512 >> k) for k in range(9)]
md.inputLayer(torch.LongTensor(sizes[0]), torch.as_tensor(l).to(dev), 4, 4, dev)
one, two = torch.LongTensor([1, 1, 1]), torch.LongTensor([2, 2, 2])
books = [md.getRuleBook(torch.LongTensor(sizes[k]), torch.LongTensor(sizes[k + 1]), two, two) for k in range(8)]


def run(name, ga, rows_in, n_in, n_out, transposed):
    vol, V = ga.vol, ga.rows
    if V == 0:
        return
    torch.manual_seed(1)
    x = torch.randn((rows_in, n_in), device=dev)
    W = torch.randn((vol, n_out, n_in) if transposed else (vol, n_in, n_out), device=dev)
    res = torch.randn((V, n_out), device=dev)
    wpack = torch.empty(lib.aabr_conv_wpack_floats(vol, n_in, n_out), device=dev)
    check(lib.aabr_conv_pack_weights(ptr(W), vol, n_in, n_out, 1 if transposed else 0, ptr(wpack), stream()))
    flags = 3 if transposed else 0
    route = SCN.conv_route(n_in, n_out, rows_in, V, vol, False, residual=True)
    blocks = route.stream(ga)
    pairs = ga.pairs()
    SCN.flush_geom()
    out0 = torch.empty((V, n_out), device=dev)
    T, P = route.tile_rows, route.parts
    r0 = res if route.takes_residual else None
    if route.kind == "wide":
        old = lambda: check(lib.aabr_conv_forward_wide_res(ptr(x), n_in, rows_in, ptr(out0), n_out, V, ptr(blocks), T, vol,
                                                           None, flags, ptr(wpack), ptr(r0), stream()))
    elif route.kind == "split":
        scratch = torch.empty(P * V * n_out, device=dev)
        old = lambda: check(lib.aabr_conv_forward_wide_split(ptr(x), n_in, rows_in, ptr(out0), n_out, V, ptr(blocks), T, vol,
                                                             None, flags, ptr(wpack), ptr(r0), P, ptr(scratch), stream()))
    else:
        old = lambda: check(lib.aabr_conv_forward(ptr(x), n_in, rows_in, ptr(out0), n_out, V, ptr(blocks), vol, ptr(W), None,
                                                  flags | 4, ptr(wpack), stream()))
    old()
    v0 = lib.aabr_conv_last_variant().decode()
    t0 = bench.device_time(torch, old)
    flop = 2.0 * V * n_in * n_out
    line = "%-22s %7d rows %3d->%-3d | %-24s %7.1f us %5.1f TF |" % (name, V, n_in, n_out, v0, t0 * 1e6, flop / t0 / 1e12)
    why = lib.aabr_conv_single_refusal(n_in, n_out, rows_in, V, vol, 0, 0).decode()
    if why and "too few" not in why:
        print(line + " single: " + why, flush=True)
        return
    out1 = torch.empty((V, n_out), device=dev)
    new = lambda: check(lib.aabr_conv_forward_single(ptr(x), n_in, rows_in, ptr(out1), n_out, V, ptr(pairs), vol, None, flags,
                                                     ptr(wpack), ptr(r0), stream()))
    for chunk in (256, 1024):
        _hip.set_knob("SINGLE_CHUNK", chunk)
        out1.fill_(float("nan"))
        new()
        same = torch.equal(out0, out1) if route.kind in ("wide", "split") else \
            float((out0 - out1).abs().max()) <= 1e-5 * float(out0.abs().max())
        t1 = bench.device_time(torch, new)
        line += " single/%d %7.1f us %5.1f TF %s" % (chunk, t1 * 1e6, flop / t1 / 1e12, "" if same else "(DIFFERS)")
    _hip.set_knob("SINGLE_CHUNK", None)
    print(line, flush=True)


def run_bwd_stats(name, ga, rows_in, n_in, n_out):
    vol, V = ga.vol, ga.rows
    torch.manual_seed(1)
    x = torch.randn((rows_in, n_in), device=dev)
    W = torch.randn((vol, n_out, n_in), device=dev)
    bx, mean, invstd = torch.randn((V, n_out), device=dev), torch.randn(n_out, device=dev), torch.rand(n_out, device=dev) + 0.5
    bw, bb = torch.randn(n_out, device=dev), torch.randn(n_out, device=dev)
    wpack = torch.empty(lib.aabr_conv_wpack_floats(vol, n_in, n_out), device=dev)
    check(lib.aabr_conv_pack_weights(ptr(W), vol, n_in, n_out, 1, ptr(wpack), stream()))
    route = SCN.conv_route(n_in, n_out, rows_in, V, vol, False, residual=True)
    line = "%-22s %7d rows %3d->%-3d |" % (name, V, n_in, n_out)
    if route.kind != "wide" or not route.stats_parts(V):
        print(line + " no statistics in today's write-out (%s)" % route.kind, flush=True)
        return
    blocks, pairs, T = route.stream(ga), ga.pairs(), route.tile_rows
    SCN.flush_geom()
    out0, st0 = torch.empty((V, n_out), device=dev), torch.empty((route.stats_parts(V), 2, n_out), dtype=torch.float64, device=dev)
    bn = (ptr(bx), ptr(mean), ptr(invstd), ptr(bw), ptr(bb), 0.0)
    old = lambda: check(lib.aabr_conv_forward_wide_bwd_stats(ptr(x), n_in, rows_in, ptr(out0), n_out, V, ptr(blocks), T, vol,
                                                             None, 3, ptr(wpack), None, ptr(st0), *bn, stream()))
    old()
    v0 = lib.aabr_conv_last_variant().decode()
    t0 = bench.device_time(torch, old)
    flop = 2.0 * V * n_in * n_out
    line += " %-16s +stats %7.1f us %5.1f TF |" % (v0, t0 * 1e6, flop / t0 / 1e12)
    _hip.set_knob("SINGLE_ROWS", 0)
    _hip.set_knob("SINGLE_BWD_STATS", 1)
    for chunk in (256, 1024):
        _hip.set_knob("SINGLE_CHUNK", chunk)
        why = lib.aabr_conv_single_bwd_stats_refusal(n_in, n_out, rows_in, V, vol, 0).decode()
        if why:
            line += " single: " + why
            break
        P = lib.aabr_conv_single_bwd_stats_parts(V, vol, chunk)
        out1 = torch.full((V, n_out), float("nan"), device=dev)
        st1 = torch.full((P, 2, n_out), float("nan"), dtype=torch.float64, device=dev)
        new = lambda: check(lib.aabr_conv_forward_single_bwd_stats(ptr(x), n_in, rows_in, ptr(out1), n_out, V, ptr(pairs), vol,
                                                                   None, 3, ptr(wpack), None, ptr(st1), *bn, stream()))
        new()
        a, b = st0.sum(0), st1.sum(0)
        same = torch.equal(out0, out1) and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
        t1 = bench.device_time(torch, new)
        line += " single/%d +stats %7.1f us %5.1f TF %s" % (chunk, t1 * 1e6, flop / t1 / 1e12, "" if same else "(DIFFERS)")
    _hip.set_knob("SINGLE_CHUNK", None)
    _hip.set_knob("SINGLE_ROWS", None)
    _hip.set_knob("SINGLE_BWD_STATS", None)
    print(line, flush=True)


if "bwd_stats" in sys.argv[1:]:
    print("input gradients of the down-sampling convolutions with backward statistics in the write-out, fp32 storage, "
          "site order %s" % order)
    for k in range(8):
        run_bwd_stats("down d_in L%d<-L%d" % (k, k + 1), books[k].inn, books[k].V_out, PLANES[k + 1], PLANES[k])
    sys.exit(0)
print("one-rule-per-row launches, fp32 storage, site order %s; residual in the write-out where the route takes one" % order)
for k in range(8):
    tb = books[k]
    run("up      L%d<-L%d" % (k, k + 1), tb.inn, tb.V_out, 128, 128, False)
for k in range(9):
    tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), one)
    run("lateral L%d" % k, tb.out, tb.V_in, PLANES[k], 128, False)
    run("lateral L%d d_in" % k, tb.out, tb.V_out, 128, PLANES[k], True)
