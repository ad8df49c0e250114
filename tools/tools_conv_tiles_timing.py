"""Dev tool: per-shape timing of the 64-row-tile convolution kernels (csrc/conv.hip) through the C ABI with prepacked
weights (flags 4): aabr_conv_forward and aabr_conv_forward_bf16 on the 80,000-point submanifold book of
tools_conv_bench.py and on a 700-row book (which reaches k_conv_blocks_mfma_small).  Per shape: the kernel instance the
library reports, then the median and min .. max over 5 windows of 20 calls (device events), after 3 warm-up calls.

To compare two builds run it once per library, each in a fresh process: `--lib PATH` loads that libaabr_hip.so instead
of the tree's.  profiles/conv_tiles_fold_timing.txt holds such a comparison."""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402

DEV = "cuda:0"
WINDOWS, CALLS, WARMUP = 5, 20, 3
LARGE = [(False, 9, 32), (False, 32, 32), (False, 32, 64), (False, 64, 64), (False, 128, 128), (False, 256, 256),
         (False, 128, 32), (True, 64, 64), (True, 128, 128), (True, 256, 256)]
SMALL = [(False, 128, 128), (False, 256, 256)]


def books():
    import sparseconvnet as scn
    import synth_scenes as S
    locs, feats = S.make_batch(1, 80000, 0, 20)
    x = scn.InputLayer(3, list(S.FULL_SCALE), mode=4)([torch.as_tensor(locs).to(DEV), torch.as_tensor(feats).to(DEV)])
    big = x.metadata.getSubmanifoldRuleBook(x.spatial_size, torch.LongTensor([3, 3, 3]))
    rng = np.random.default_rng(703)
    cells = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    coords = np.concatenate([cells[rng.choice(len(cells), 700, replace=False)], np.zeros((700, 1), np.int64)], 1)
    y = scn.InputLayer(3, [64, 64, 64], mode=4)([torch.as_tensor(coords).to(DEV), torch.zeros((700, 1), device=DEV)])
    small = y.metadata.getSubmanifoldRuleBook(y.spatial_size, torch.LongTensor([3, 3, 3]))
    return (big, x), (small, y)          # (the tensors keep the metadata alive)


def time_shape(lib, tb, bf, ci, co):
    V, vol = tb.V_out, tb.vol
    dt = torch.bfloat16 if bf else torch.float32
    g = torch.Generator(device=DEV).manual_seed(ci * 1000 + co)
    inp = torch.randn(V, ci, device=DEV, generator=g).to(dt)
    w = torch.randn(vol, ci, co, device=DEV, generator=g)
    out = torch.empty(V, co, device=DEV, dtype=dt)
    if bf:
        wp = torch.empty(int(lib.aabr_conv_wpack_bf16_elems(vol, ci, co)), dtype=dt, device=DEV)
        fn = lib.aabr_conv_forward_bf16
    else:
        wp = torch.empty(int(lib.aabr_conv_wpack_floats(vol, ci, co)), device=DEV)
        fn = lib.aabr_conv_forward
    blocks = tb.out.blocks()
    call = lambda flags: _hip.check(fn(_hip.ptr(inp), ci, V, _hip.ptr(out), co, V, _hip.ptr(blocks), vol, _hip.ptr(w), None,
                                       flags, _hip.ptr(wp), _hip.stream()))
    call(0)                                                   # packs the weights
    for _ in range(WARMUP):
        call(4)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(WINDOWS):
        a.record()
        for _ in range(CALLS):
            call(4)
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) / CALLS * 1e3)
    return lib.aabr_conv_last_variant().decode(), float(np.median(us)), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="load this libaabr_hip.so instead of the tree's")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    lib = _hip.load()
    (big, _x), (small, _y) = books()
    lines = []
    for tb, shapes in ((big, LARGE), (small, SMALL)):
        for bf, ci, co in shapes:
            variant, med, lo, hi = time_shape(lib, tb, bf, ci, co)
            lines.append("V %6d %s %3d->%3d  %-44s %9.1f us (%.1f .. %.1f)" % (tb.V_out, "bf16" if bf else "fp32", ci, co,
                                                                            variant, med, lo, hi))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
