"""Dev tool: one SHA-256 per launch over the raw output bytes of aabr_conv_forward / aabr_conv_forward_bf16 for every
64-row-tile kernel instance csrc/conv.hip compiles -- at the (book, planes, knobs) tests/test_gpu_conv_tiles.py::_config
finds for it -- and for the ragged-column configurations of tests/test_gpu_conv_exact.py (output planes that are no
multiple of 4, last column slab partly filled), each with flags 0 and 3, with and without bias.  The generic kernel is
reached through flags 8 << 8 on ordinary buffers (the bit only steers the decision; the > 2 GiB launch is left to
tests/test_gpu_conv_tiles.py).  Operands come from fixed numpy seeds; every line names the instance that ran.

Two libraries compute the same thing bit for bit when their lists are equal line for line: run this file once per
library, each in a fresh process (`--lib PATH` loads that libaabr_hip.so instead of the tree's).
profiles/conv_tiles_fold_digests.txt holds such a list.  Nothing in a test depends on this tool."""
import argparse
import hashlib
import importlib
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
import conv_tiles_rule as R  # noqa: E402

DEV = "cuda:0"
GENERIC = 8 << 8            # sets `exp` in the decision and none of the generic kernel's dbg & 1 / 2 / 4 branches
# (book, bf16, planes in, planes out, knobs): tests/test_gpu_conv_exact.py::RAGGED
RAGGED = [("large", False, 96, 198, {}), ("large", False, 96, 134, {}), ("large", False, 96, 70, {}),
          ("large", False, 9, 6, {}), ("large", False, 48, 198, {}), ("large", False, 96, 6, {}),
          ("large", True, 96, 160, {}), ("large", True, 64, 416, {}),
          ("small", False, 32, 134, {"CONV_WLDS": 2}), ("small", False, 96, 70, {"SMALL_WPB": 8}),
          ("small", False, 48, 198, {"CONV_WLDS": 0})]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def generic_config(TT, key):
    """the first (book, planes in, planes out, knobs) whose launch with flags 8 << 8 is the generic instance `key`"""
    for book, knobs, n_in, n_out in itertools.product(("small", "large", "one"), TT.KNOB_SETS, (32, 64, 16, 48, 96, 80),
                                                      (64, 256, 32)):
        V, vol = TT.BOOKS[book][0], TT.BOOKS[book][2] ** 3
        t = TT._decide(False, n_in, n_out, V, vol, GENERIC, TT._sizes(n_in, n_out, V, vol, False, False), knobs)
        if t[:7] == key:
            return book, n_in, n_out, knobs
    raise AssertionError("no configuration reaches " + R.name(key))


def launch(lib, TT, book, bf, n_in, n_out, knobs, flags, bias):
    ga, _ = TT._book(book)
    V, vol = ga.rows, ga.vol
    rng = np.random.default_rng(n_in * 1000 + n_out + vol + 7 * (flags & 3))
    x = rng.standard_normal((V, n_in)).astype(np.float32)
    # flags 3 (transposed, flipped): the weights are stored [vol][n_out][n_in]
    W = (rng.standard_normal((vol, n_out, n_in) if flags & 1 else (vol, n_in, n_out)) * 0.1).astype(np.float32)
    b = _t(rng.standard_normal(n_out).astype(np.float32)) if bias else None
    for name in R.KNOBS:
        _hip.set_knob(name, knobs.get(name))
    try:
        dt = torch.bfloat16 if bf else torch.float32
        xd, Wd = _t(x).to(dt), _t(W)
        out = torch.full((V, n_out), float("nan"), dtype=dt, device=DEV)
        if bf:
            wp = torch.empty(int(lib.aabr_conv_wpack_bf16_elems(vol, n_in, n_out)), dtype=dt, device=DEV)
            fn = lib.aabr_conv_forward_bf16
        else:
            wp = torch.empty(int(lib.aabr_conv_wpack_floats(vol, n_in, n_out)), device=DEV)
            fn = lib.aabr_conv_forward
        _hip.check(fn(_hip.ptr(xd), n_in, V, _hip.ptr(out), n_out, V, _hip.ptr(ga.blocks()), vol, _hip.ptr(Wd), _hip.ptr(b),
                      flags, _hip.ptr(wp), _hip.stream()))
        variant = lib.aabr_conv_last_variant().decode()
    finally:
        for name in R.KNOBS:
            _hip.set_knob(name, None)
    raw = out.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return variant, hashlib.sha256(raw).hexdigest()


def cases(TT):
    """(what, book, bf16, planes in, planes out, knobs, extra flag bits, instance expected at flags 0 or None)"""
    for key in R.compiled_instances():
        kind = R.KINDS[key[0]]
        book, n_in, n_out, knobs = generic_config(TT, key) if kind == "generic" else TT._config(key)
        yield ("instance", book, kind == "bf16", n_in, n_out, knobs, GENERIC if kind == "generic" else 0, R.name(key))
    for book, bf, n_in, n_out, knobs in RAGGED:
        yield ("ragged", book, bf, n_in, n_out, knobs, 0, None)
        if not bf:
            yield ("ragged", book, bf, n_in, n_out, knobs, GENERIC, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="load this libaabr_hip.so instead of the tree's")
    ap.add_argument("--out", default=None, help="also write the list to this file")
    args = ap.parse_args()
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    lib = _hip.load()
    import test_gpu_conv_tiles as TT
    lines = []
    for what, book, bf, n_in, n_out, knobs, extra, expect in cases(TT):
        for flags in (0, 3):
            for bias in (0, 1):
                variant, h = launch(lib, TT, book, bf, n_in, n_out, knobs, flags | extra, bias)
                assert expect is None or flags or variant == expect, (variant, expect)
                kn = ",".join("%s=%d" % kv for kv in sorted(knobs.items())) or "-"
                lines.append("%s %s %s %d->%d knobs %s flags %d%s bias %d %s %s" % (
                    what, book, "bf16" if bf else "fp32", n_in, n_out, kn, flags, "|8<<8" if extra else "", bias, variant, h))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
