"""Dev tool: time the FullConvolution / TransposeConvolution path -- the level build (aabr_full_convolution_sites over hash
grids, aabr_brick_full_build in brick order), the rule tables over the grown level, and forward + backward of a 64 -> 64
layer in fp32 and bf16 storage -- from the input level of `--batch` synthetic wall scenes (synth_scenes.make_batch; about
200 k input sites at the defaults), for filter / stride 3/2 and 2/2, in both site orders.  Beside each line stands the same
measurement of what the code base had before: the SHRINKING level build with the same filter from the same sites
(aabr_convolution_sites / aabr_brick_build), its tables, and forward + backward of a Deconvolution 64 -> 64 from that
shrunk level back onto the prebuilt input level.  The two are not the same amount of work -- the grown level has several
times the rows of the input level, the Deconvolution writes the input level's rows -- so every line carries its rows,
candidates and rules, and ns per candidate / per rule.

Device events around `--iters` back-to-back calls after a warm-up, on preallocated buffers (no allocation and no host read
inside the timed region; the brick builds include the fills of their directory); the new and the old form alternate in
`--repeats` windows; median and min .. max over the windows.  The parent starts the child under its own `timeout`.  Writes
`--out` (profiles/full_conv_timing.txt)."""
import argparse
import importlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def child_time(args):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    importlib.import_module("automatic-as-built-reconstruction_amd")
    import torch
    import synth_scenes as S
    import _hip
    import sparseconvnet as scn
    from sparseconvnet import SCN
    from _hip import ptr, check, stream, i32x3
    lib = _hip.load()
    locs, _ = S.make_batch(args.batch, args.npts, 0, 20)
    L = lambda v: torch.LongTensor([int(i) for i in v])
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
    results = []

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    def pair(order, window, what, new, old):
        """new / old: (label, fn, rows, work items, name of the work items)"""
        for _, fn, _, _, _ in (new, old):
            fn()
        ts = {0: [], 1: []}
        for _ in range(args.repeats):
            for i, (_, fn, _, _, _) in enumerate((new, old)):
                ts[i].append(timed(fn))
        med = lambda v: [sorted(v)[len(v) // 2], min(v), max(v)]
        for i, (label, _, rows, items, unit) in enumerate((new, old)):
            results.append(dict(order=order, window=window, what=what, label=label, rows=rows, items=items, unit=unit,
                                ms=med(ts[i])))

    def hash_sites(fn, gi, fs, st, osz, E):
        cap = SCN.derived_cap(E)
        keys = torch.empty(2 * cap, dtype=torch.int64, device=DEV)
        scratch, out, meta = i32(E + 4 * ((max(E, 1) + 255) // 256) + 16), i32(max(E, 1), 4), i32(_hip.META_WORDS)
        return lambda: check(fn(ptr(gi.coords), gi.V, i32x3(fs), i32x3(st), i32x3(osz), ptr(keys), cap, ptr(scratch),
                                ptr(out), ptr(meta), stream()))

    def brick_level(fn, gi, fs, st, osz, ext, nb_bound, v_bound):
        bk = SCN._Brick(ext, gi.brick.dims[3], nb_bound, v_bound, DEV, i32(_hip.META_WORDS))
        scratch = i32(int(lib.aabr_brick_scratch_words(bk.nw, bk.nb_cap)) + 2)
        sp = scratch.data_ptr() + 4 * ((-scratch.data_ptr() // 4) % 2)
        return lambda: check(fn(ptr(gi.coords), gi.V, None, i32x3(fs), i32x3(st), i32x3(osz), bk.dims_c(), bk.dir_ptr(),
                                bk.bricks_ptr(), bk.nb_cap, bk.bcoord.data_ptr(), bk.coords_full.data_ptr(), bk.v_cap,
                                bk.meta.data_ptr(), sp, 0, stream()))

    def tables(fine, coarse, fs, st, clip):
        """a Convolution's two tables from level `fine` down to level `coarse`"""
        vol = fs[0] * fs[1] * fs[2]
        t_out, t_in = i32(vol, coarse.V), i32(vol, fine.V)
        c_out, c_in = i32(vol * ((coarse.V + 255) // 256)), i32(vol * ((fine.V + 255) // 256))
        if fine.brick is not None:
            return lambda: check(lib.aabr_brick_convolution_tables(
                ptr(fine.coords), fine.V, fine.brick.dims_c(), fine.brick.dir_ptr(), fine.brick.bricks_ptr(),
                ptr(coarse.coords), coarse.V, coarse.brick.dims_c(), coarse.brick.dir_ptr(), coarse.brick.bricks_ptr(),
                i32x3(fs), i32x3(st), i32x3(clip), ptr(t_out), ptr(t_in), ptr(c_out), ptr(c_in), stream()))
        return lambda: check(lib.aabr_convolution_tables2(
            ptr(fine.coords), fine.V, ptr(fine.keys), fine.cap, ptr(coarse.coords), coarse.V, ptr(coarse.keys), coarse.cap,
            i32x3(fs), i32x3(st), i32x3(clip), ptr(t_out), ptr(t_in), ptr(c_out), ptr(c_in), stream()))

    for order in ("first_seen", "brick"):
        for size, stride in ((3, 2), (2, 2)):
            fs, st = (size,) * 3, (stride,) * 3
            spatial = [s + (size - stride) for s in S.FULL_SCALE]          # an exact fit of the shrinking windows
            layer = scn.InputLayer(3, spatial, mode=4)
            layer.site_order = order
            x0 = layer([torch.as_tensor(locs).to(DEV), torch.zeros((len(locs), 1), device=DEV)])
            md, isz = x0.metadata, x0.spatial_size
            gi = md.grids[tuple(isz.tolist())]
            grown, shrunk = (isz - 1) * stride + size, (isz - size) // stride + 1
            new = scn.Metadata(3)
            tbf = md.getFullConvolutionRuleBook(isz, grown, L(fs), L(st), new)
            tbc = md.getRuleBook(isz, shrunk, L(fs), L(st))
            go, gc = new.grids[tuple(grown.tolist())], md.grids[tuple(shrunk.tolist())]
            vol, maxout = size ** 3, ((size + stride - 1) // stride) ** 3
            window = "%d/%d" % (size, stride)
            if order == "brick":
                b = gi.brick
                sites_new = brick_level(lib.aabr_brick_full_build, gi, fs, st, grown.tolist(),
                                        [(e - 1) * stride + size for e in b.ext], gi.V * vol, gi.V * vol)
                sites_old = brick_level(lib.aabr_brick_build, gi, fs, st, shrunk.tolist(),
                                        [min(o, (e - 1) // stride + 1) for o, e in zip(shrunk.tolist(), b.ext)],
                                        b.nb_cap * maxout, b.v_cap * maxout)
                names = ("aabr_brick_full_build", "aabr_brick_build")
            else:
                sites_new = hash_sites(lib.aabr_full_convolution_sites, gi, fs, st, grown.tolist(), gi.V * vol)
                sites_old = hash_sites(lib.aabr_convolution_sites, gi, fs, st, shrunk.tolist(), gi.V * maxout)
                names = ("aabr_full_convolution_sites", "aabr_convolution_sites")
            pair(order, window, "site build", (names[0], sites_new, go.V, gi.V * vol, "candidate"),
                 (names[1], sites_old, gc.V, gi.V * maxout, "candidate"))
            rules_f, rules_c = int(tbf.total_rules()), int(tbc.total_rules())
            pair(order, window, "tables", ("grown level <-> input level", tables(go, gi, fs, st, (SCN.kMaxSpatial,) * 3),
                                           go.V, rules_f, "rule"),
                 ("input level <-> shrunk level", tables(gi, gc, fs, st, shrunk.tolist()), gi.V, rules_c, "rule"))
            for dtype in (torch.float32, torch.bfloat16):
                torch.manual_seed(0)
                W = torch.randn((vol, 1, 64, 64), device=DEV) * 0.05
                nob = torch.empty(0, device=DEV)
                x, dy = (torch.randn((r, 64), device=DEV).to(dtype) for r in (gi.V, go.V))
                xc, dyf = (torch.randn((r, 64), device=DEV).to(dtype) for r in (gc.V, gi.V))
                y, dx, yd, dxd = (torch.empty(0, device=DEV, dtype=dtype) for _ in range(4))
                dW = torch.empty_like(W)
                geo_f, geo_d = (isz, grown, L(fs), L(st)), (shrunk, isz, L(fs), L(st))

                def full():
                    SCN.FullConvolution_updateOutput(*geo_f, md, new, x, y, W, nob)
                    SCN.FullConvolution_backward(*geo_f, md, new, x, dx, dy, W, dW, nob)

                def deconv():
                    SCN.Deconvolution_updateOutput(*geo_d, md, xc, yd, W, nob)
                    SCN.Deconvolution_backward(*geo_d, md, xc, dxd, dyf, W, dW, nob)
                pair(order, window, "fwd + bwd 64->64 " + str(dtype).split(".")[1],
                     ("FullConvolution", full, go.V, rules_f, "rule"), ("Deconvolution", deconv, gi.V, rules_c, "rule"))
                del x, dy, xc, dyf, y, dx, yd, dxd
            del md, new, x0, tbf, tbc, go, gc, gi
    print("RESULT " + json.dumps(results))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--npts", type=int, default=80000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--child", choices=("time",))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "full_conv_timing.txt"))
    args = ap.parse_args()
    if args.child == "time":
        return child_time(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "time"]
    for k in ("batch", "npts", "iters", "repeats"):
        cmd += ["--" + k, str(getattr(args, k))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stdout.write(r.stdout)
        raise SystemExit("the timing child ended with status %d" % r.returncode)
    res = json.loads(line[-1][7:])
    lines = ["FullConvolution path from the input level of %d synthetic scenes x %d points; device events around %d calls on "
             "preallocated buffers, median of %d windows (min .. max), the new and the old form alternating after a warm-up "
             "of each" % (args.batch, args.npts, args.iters, args.repeats),
             "each pair: the new entry point, then what the code base had before on the same input sites and filter -- the "
             "shrinking level build, its tables, a Deconvolution from the shrunk level back onto the input level; NOT the same "
             "amount of work: compare the per-item column",
             "rows: sites of the level built / rows the tables' fine side holds / rows the forward pass writes; items: "
             "candidate sites (input sites x filter volume, or x output-region size) or rules",
             "%-10s %-6s %-26s %-30s %9s %10s %9s  %s" % ("order", "window", "what", "form", "rows", "items", "ns/item",
                                                          "device us (min .. max)")]
    for r_ in res:
        m = r_["ms"]
        lines.append("%-10s %-6s %-26s %-30s %9d %10d %9.3f  %9.1f (%.1f .. %.1f)" % (
            r_["order"], r_["window"], r_["what"], r_["label"], r_["rows"], r_["items"],
            1e6 * m[0] / max(r_["items"], 1), 1e3 * m[0], 1e3 * m[1], 1e3 * m[2]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
