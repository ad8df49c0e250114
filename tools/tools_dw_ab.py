"""A/B of the weight-gradient kernels on the bench's own rule books (4 x S80k @ 2 cm): the 64 x 64-block kernels
(k_conv_dw_pairs[_bf16], one workgroup per chunk and block) against the full-tile kernels (k_conv_dw_full_*, one workgroup
per equal range of the concatenated pair list, whole 128 x 128 blocks) at several workgroup counts; device time of the
whole aabr_conv_backward_weight call (kernel + reduce) with the host taken out.
usage: [f32|bf16] [first_seen|brick] [vec]
vec (fp32): the books the step sends through the 64 x 64-block kernel instead, each with the knob DW_VEC 0 (one dword load per
16-channel block) and 1 (one 16- / 8-byte load per lane, the default), interleaved; the 128 -> 128 books also through the
full-tile kernel at its default workgroup count, which is what the 250 k-rule threshold between the two chooses from."""
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
bf = len(sys.argv) > 1 and sys.argv[1] == "bf16"
order = sys.argv[2] if len(sys.argv) > 2 else "brick"
vec_mode = len(sys.argv) > 3 and sys.argv[3] == "vec"
l, _ = S.make_batch(4, 80000, 9000, 50)
md = SCN.Metadata_3(order)
sizes = [(4096 >> k, 4096 >> k, 512 >> k) for k in range(9)]
md.inputLayer(torch.LongTensor(sizes[0]), torch.as_tensor(l).to(dev), 4, 4, dev)
three, two = torch.LongTensor([3, 3, 3]), torch.LongTensor([2, 2, 2])
for k in range(7):
    md.getRuleBook(torch.LongTensor(sizes[k]), torch.LongTensor(sizes[k + 1]), two, two)
dt = torch.bfloat16 if bf else torch.float32
fn = lib.aabr_conv_backward_weight_bf16 if bf else lib.aabr_conv_backward_weight
WGS = [0, 128, 256, 384, 512, 768, 1024, 1536]


def run(name, ga, n_in, n_out, rows_in=None):
    vol, V = ga.vol, ga.rows
    torch.manual_seed(1)
    rows_in = V if rows_in is None else rows_in          # the gather's partner rows index the INPUT matrix
    assert int(ga.table.max()) < rows_in
    x = torch.randn((rows_in, n_in), device=dev).to(dt)
    g = torch.randn((V, n_out), device=dev).to(dt)
    pairs = ga.pairs()
    mc = ga.max_chunks(n_in, n_out)
    SCN.flush_geom()
    R = int(sum(ga.rule_counts()))
    mc = ga.max_chunks(n_in, n_out)     # (the exact chunk count now that the counts are on the host)
    scratch = torch.empty(int(lib.aabr_conv_dw_scratch_floats(mc, n_in, n_out)), device=dev)
    dW = torch.empty((vol, n_in, n_out), device=dev)
    call = lambda: check(fn(ptr(x), n_in, ptr(g), n_out, V, ptr(pairs), vol, mc, ptr(dW), None, ptr(scratch), stream()))
    _hip.set_knob("DW_FULL", 0)
    call()
    ref = dW.clone()
    t0 = bench.device_time(torch, call)
    _hip.set_knob("DW_FULL", None)
    out = ["%-18s %7d rows %8d rules %3d->%-3d chunks %5d | blocks %6.1f us %6.1f TF |" % (
        name, V, R, n_in, n_out, mc, t0 * 1e6, 2.0 * R * n_in * n_out / t0 / 1e12)]
    for w in WGS:
        _hip.set_knob("DW_FULL_WGS", w if w else None)
        _hip.set_knob("DW_FULL_MIN", 1 if not w else None)
        dW.fill_(float("nan"))
        call()
        v = lib.aabr_conv_last_variant().decode()
        if "full" not in v:
            out.append(" %s:-" % (w or "dflt"))
            continue
        err = float((dW - ref).abs().max() / ref.abs().max())
        t = bench.device_time(torch, call)
        out.append(" %s:%.1f" % (w or "dflt", t * 1e6) + ("" if err < 1e-4 else "(err %.1e)" % err))
    _hip.set_knob("DW_FULL_WGS", None)
    _hip.set_knob("DW_FULL_MIN", None)
    print("".join(out), flush=True)


def run_vec(name, ga, n_in, n_out, rows_in=None):
    """the 64 x 64-block kernel with DW_VEC 0 and 1, three interleaved rounds each (best of the three), bit-equality checked"""
    vol, V = ga.vol, ga.rows
    torch.manual_seed(1)
    rows_in = V if rows_in is None else rows_in
    x = torch.randn((rows_in, n_in), device=dev).to(dt)
    g = torch.randn((V, n_out), device=dev).to(dt)
    pairs = ga.pairs()
    mc = ga.max_chunks(n_in, n_out)
    SCN.flush_geom()
    R = int(sum(ga.rule_counts()))
    mc = ga.max_chunks(n_in, n_out)
    scratch = torch.empty(int(lib.aabr_conv_dw_scratch_floats(mc, n_in, n_out)), device=dev)
    dW = torch.empty((vol, n_in, n_out), device=dev)
    call = lambda: check(fn(ptr(x), n_in, ptr(g), n_out, V, ptr(pairs), vol, mc, ptr(dW), None, ptr(scratch), stream()))
    _hip.set_knob("DW_FULL", 0)
    t, res, var = {0: [], 1: []}, {}, {}
    for _ in range(3):
        for kv in (0, 1):
            _hip.set_knob("DW_VEC", kv)
            dW.fill_(float("nan"))
            call()
            var[kv] = lib.aabr_conv_last_variant().decode()
            res[kv] = dW.clone()
            t[kv].append(bench.device_time(torch, call))
    _hip.set_knob("DW_VEC", None)
    _hip.set_knob("DW_FULL", None)
    mask = lib.aabr_conv_dw_vec_operands(1 if bf else 0, ptr(x), n_in, ptr(g), n_out, V, vol, mc)
    tf = lambda s_: 2.0 * R * n_in * n_out / s_ / 1e12
    t0, t1 = min(t[0]), min(t[1])
    line = "%-22s %7d rows %8d rules %3d->%-3d %-28s | DW_VEC=0 %6.1f us %5.1f TF | DW_VEC=1 %6.1f us %5.1f TF | x%.2f | %s" % (
        name, V, R, n_in, n_out, var[1], t0 * 1e6, tf(t0), t1 * 1e6, tf(t1), t0 / t1,
        "bit-equal" if torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)) else "DIFFERENT")
    if n_in % 128 == 0 and n_out % 128 == 0:
        for w in (256, 512):                                  # the two workgroup counts the default rule chooses from
            _hip.set_knob("DW_FULL_WGS", w)
            call()
            if "full" in lib.aabr_conv_last_variant().decode():
                tfu = bench.device_time(torch, call)
                line += " | full-tile %d wgs %6.1f us %5.1f TF" % (w, tfu * 1e6, tf(tfu))
        _hip.set_knob("DW_FULL_WGS", None)
    print(line, flush=True)


if vec_mode:
    planes = [32, 64, 64, 128, 128, 128, 256, 256, 256]      # FPN_Net's planes per level
    print("weight gradient, %s storage, site order %s; k_conv_dw_pairs with the knob DW_VEC 0 / 1 (us per call: kernel + reduce)"
          % ("bf16" if bf else "fp32", order))
    for k in range(6):
        tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), three)
        run_vec("subm L%d" % k, tb.out, planes[k], planes[k])
    for k in (0, 1, 2, 3):
        tb = md.getRuleBook(torch.LongTensor(sizes[k]), torch.LongTensor(sizes[k + 1]), two, two)
        run_vec("down L%d->%d" % (k, k + 1), tb.out, planes[k], planes[k + 1], rows_in=tb.V_in)
        run_vec("up   L%d->%d" % (k + 1, k), tb.inn, planes[k + 1], planes[k], rows_in=tb.V_out)
    one = torch.LongTensor([1, 1, 1])
    for k in (1, 3):
        tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), one)
        run_vec("1x1x1 L%d" % k, tb.out, 128, 128)
    sys.exit(0)

print("weight gradient, %s storage, site order %s; full-tile kernel by number of workgroups (us per call)" % ("bf16" if bf else "fp32", order))
for k in (3, 2, 4, 1, 5, 0):
    tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), three)
    run("subm L%d 128->128" % k, tb.out, 128, 128)
tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[6]), three)
run("subm L6 256->256", tb.out, 256, 256)
tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[5]), three)
run("subm L5 256->256", tb.out, 256, 256)
one = torch.LongTensor([1, 1, 1])
for k in (3, 1):
    tb = md.getSubmanifoldRuleBook(torch.LongTensor(sizes[k]), one)
    run("1x1x1 L%d 128->128" % k, tb.out, 128, 128)
for k in (1, 3):
    tb = md.getRuleBook(torch.LongTensor(sizes[k]), torch.LongTensor(sizes[k + 1]), two, two)
    run("down L%d->%d 128->128" % (k, k + 1), tb.out, 128, 128, rows_in=tb.V_in)
    run("up   L%d->%d 128->128" % (k + 1, k), tb.inn, 128, 128, rows_in=tb.V_out)
