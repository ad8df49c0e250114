"""Dev tool: one SHA-256 per case over the geometry `sparseconvnet.SCN.Metadata_3` builds -- the site list of every level
(`coords[:V]`), its `sample_off`, both gather tables and both count arrays of every rule book, the input layer's
point -> site array -- and over the sequence of builder calls that produced it: the `(kind, i32, i64)` fields of every
record handed to `SCN._geom`, pointers left out.  A builder the module calls directly instead (aabr_convolution_sites,
aabr_convolution_tables2, aabr_brick_convolution_tables: the entry points aabr_geom_run dispatches those kinds to) is
written into the sequence as the record it would have been, so the sequence does not depend on which of the two calling
conventions a path uses.

Geometry is integer and deterministic: two trees build the same thing when their lists are equal line for line.  Run this
file once from a checkout of each (it uses the package and the library of the tree it lies in), a fresh process each;
profiles/geometry_fold_digests.txt holds such a pair.  Every case runs in both site orders; the cases that build levels
or rule books run outside and inside `geom_plan`.  Nothing in a test depends on this tool."""
import argparse
import hashlib
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _hip  # noqa: E402
from sparseconvnet import SCN  # noqa: E402

DEV = torch.device("cuda", 0)
SP = (96, 72, 16)
ORDERS = ("first_seen", "brick")
records = []          # the builder calls of the running case: (kind, i32 x 10, i64 x 4)


def L(v):
    return torch.LongTensor([int(i) for i in v])


def _pad(v, n):
    v = [int(x) for x in v]
    return tuple(v + [0] * (n - len(v)))


def _record(kind, i32=(), i64=()):
    records.append((int(kind), _pad(i32, 10), _pad(i64, 4)))


def _packed(dims):
    d = list(dims)
    return d[0] | (d[1] << 16) | (d[2] << 32) | (d[3] << 48)


class _Lib(object):
    """the library with the three directly called builders written into `records` on their way through"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def aabr_convolution_sites(self, c, V, fs, st, osz, keys, cap, *rest):
        _record(SCN.G_SITES, list(fs) + list(st) + list(osz), (V, cap))
        return self._lib.aabr_convolution_sites(c, V, fs, st, osz, keys, cap, *rest)

    def aabr_convolution_tables2(self, ci, Vi, ki, capi, co, Vo, ko, capo, fs, st, osz, *rest):
        _record(SCN.G_TABLES, list(fs) + list(st) + list(osz), (Vi, capi, Vo, capo))
        return self._lib.aabr_convolution_tables2(ci, Vi, ki, capi, co, Vo, ko, capo, fs, st, osz, *rest)

    def aabr_brick_convolution_tables(self, ci, Vi, di, diri, bri, co, Vo, do, diro, bro, fs, st, osz, *rest):
        _record(SCN.G_BK_TABLES, list(fs) + list(st) + list(osz), (Vi, Vo, _packed(di), _packed(do)))
        return self._lib.aabr_brick_convolution_tables(ci, Vi, di, diri, bri, co, Vo, do, diro, bro, fs, st, osz, *rest)


def install_hooks():
    lib = _Lib(_hip.load())
    _hip.load = lambda: lib
    geom = SCN._geom

    def _geom(kind, i32=(), i64=(), ps=()):
        _record(kind, i32, i64)
        return geom(kind, i32, i64, ps)
    SCN._geom = _geom


def digest(mds):
    """the geometry of the Metadata objects `mds` and the builder calls recorded since the case began"""
    SCN.flush_geom()
    h = hashlib.sha256()

    def feed(name, t):
        h.update(name.encode())
        if t is None:
            h.update(b"none")
        elif torch.is_tensor(t):
            t = t.detach().cpu().contiguous()
            h.update(("%s%s" % (t.dtype, tuple(t.shape))).encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        else:
            h.update(repr(t).encode())

    for i, md in enumerate(mds):
        h.update(("md%d %s" % (i, md.site_order)).encode())
        for key in sorted(md.grids):
            g = md.grids[key]
            feed("grid%r V" % (key,), g.V)
            feed("coords", g.coords[:g.V])
            feed("sample_off", None if g.sample_off is None else [int(v) for v in g.sample_off])
        books = [("subm%r" % (k,), tb) for k, tb in sorted(md.submanifold.items())]
        books += [("book%r" % (k,), tb) for k, tb in sorted(md.rulebooks.items())]
        if md.fullConvolutionRuleBook is not None:
            books.append(("full", md.fullConvolutionRuleBook))
        for name, tb in books:
            feed(name, (tb.vol, tb.V_out, tb.V_in))
            for side, ga in (("out", tb.out), ("inn", tb.inn)):
                feed(side + " table", None if ga is None else ga.table)
                feed(side + " counts", None if ga is None else ga.counts)
        if md.input is not None:
            feed("input V", md.input["V"])
            feed("point_site", md.input["point_site"])
    for r in records:
        h.update(repr(r).encode())
    return h.hexdigest()


def scene(seed, n, size=SP, batch=2):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(0, s, n) for s in size] + [np.sort(rng.integers(0, batch, n))], 1).astype(np.int64)
    return torch.as_tensor(c).reshape(-1, 4).to(DEV)


def flat(order, coords, sp=SP):
    md = SCN.Metadata_3(order)
    md.inputLayer(L(sp), coords, 2, 3, DEV)
    return md


def half(sp, k=1):
    return tuple(max(s >> k, 1) for s in sp)


def out_size(sp, f, s):
    return tuple((a - f) // s + 1 for a in sp)


# ---- cases: each takes the site order and returns the Metadata objects to digest -------------------------------------
def c_subm(order):
    md = flat(order, scene(1, 4000))
    md.getSubmanifoldRuleBook(L(SP), L([3, 3, 3]))
    return [md]


def c_strided(f, s):
    def run(order):
        md = flat(order, scene(2, 4000))
        md.getRuleBook(L(SP), L(out_size(SP, f, s)), L([f] * 3), L([s] * 3))
        return [md]
    return run


def c_second_book(order):
    md = flat(order, scene(3, 4000))
    md.getRuleBook(L(SP), L(half(SP)), L([2, 2, 2]), L([2, 2, 2]))
    md.getRuleBook(L(SP), L(half(SP)), L([1, 1, 1]), L([2, 2, 2]))
    return [md]


def c_grids_chain(order):
    md = flat(order, scene(4, 5000))
    md.buildGridsFromInput(L(SP), [(L(half(SP, k)), L([1 << k] * 3)) for k in (1, 2, 3)])
    for k in (0, 1, 2):
        md.getRuleBook(L(half(SP, k)), L(half(SP, k + 1)), L([2, 2, 2]), L([2, 2, 2]))
    return [md]


def c_pyramid(defer):
    def run(order):
        md = flat(order, scene(5, 5000))
        if order != "brick":         # the hash grids' counterpart of the pyramid: level by level, built on demand
            for k in (0, 1, 2):
                md.getRuleBook(L(half(SP, k)), L(half(SP, k + 1)), L([2, 2, 2]), L([2, 2, 2]))
            return [md]
        specs = [(half(SP, k + 1), half(SP, k), (2, 2, 2), (2, 2, 2)) for k in (0, 1, 2)]
        s3 = half(SP, 3)
        specs.append(((s3[0], s3[1], 1), s3, (1, 1, s3[2]), (1, 1, s3[2])))
        md.buildBrickPyramid(specs, defer=defer)
        md.finishBrickPyramid()
        for osz, src, f, s in specs:
            md.getRuleBook(L(src), L(osz), L(f), L(s))
        return [md]
    return run


def c_pool(order):
    md = flat(order, scene(6, 4000))
    o = out_size(SP, 3, 2)
    md.getRuleBook(L(SP), L(o), L([3, 3, 3]), L([2, 2, 2]))
    SCN._unpool_book(L(SP), L(o), L([3, 3, 3]), L([2, 2, 2]), md)
    return [md]


def c_full(f, s, n=1500):
    def run(order):
        sp = (24, 18, 8)
        md = flat(order, scene(7, n, sp), sp)
        new = SCN.Metadata_3()
        osz = tuple((a - 1) * s + f for a in sp)
        md.getFullConvolutionRuleBook(L(sp), L(osz), L([f] * 3), L([s] * 3), new)
        if new.grids[osz].V:
            new.getSubmanifoldRuleBook(L(osz), L([3, 3, 3]))
        return [md, new]
    return run


def c_empty_scene(order):
    md = flat(order, scene(8, 0))
    md.getSubmanifoldRuleBook(L(SP), L([3, 3, 3]))
    md.getRuleBook(L(SP), L(half(SP)), L([2, 2, 2]), L([2, 2, 2]))
    return [md]


def c_bl_trailing_empty(order):
    rng = np.random.default_rng(9)
    c = np.stack([rng.integers(0, s, (3, 700)) for s in SP], 2).astype(np.int64)
    c[0, 500:] = -1
    c[2] = -1
    md = SCN.Metadata_3(order)
    md.blLayer(L(SP), torch.as_tensor(c).to(DEV), 3, DEV)
    md.getSubmanifoldRuleBook(L(SP), L([3, 3, 3]))
    md.getRuleBook(L(SP), L(half(SP)), L([2, 2, 2]), L([2, 2, 2]))
    return [md, SCN._batch_size(md)]


def c_scatter(variant, brick_scatter=True):
    def run(order):
        old = SCN.scatter_variant, SCN.SCATTER_MIN_POINTS, SCN.brick_scatter
        SCN.scatter_variant, SCN.SCATTER_MIN_POINTS, SCN.brick_scatter = variant, 1, brick_scatter
        try:
            md = flat(order, scene(10, 6000))
            md.getSubmanifoldRuleBook(L(SP), L([3, 3, 3]))
            md.getRuleBook(L(SP), L(half(SP)), L([2, 2, 2]), L([2, 2, 2]))
        finally:
            SCN.scatter_variant, SCN.SCATTER_MIN_POINTS, SCN.brick_scatter = old
        return [md]
    return run


# (name, case, also inside geom_plan)
CASES = [
    ("submanifold 3^3", c_subm, True),
    ("strided book on demand 2/2", c_strided(2, 2), True),
    ("strided book on demand 3/2", c_strided(3, 2), True),
    ("second book onto an existing level", c_second_book, True),
    ("buildGridsFromInput chain of three levels", c_grids_chain, True),
    ("buildBrickPyramid", c_pyramid(False), True),
    ("buildBrickPyramid defer", c_pyramid(True), True),
    ("pooling and UnPooling book 3/2", c_pool, True),
    ("FullConvolution 3/2", c_full(3, 2), True),
    ("FullConvolution 2/2", c_full(2, 2), True),
    ("FullConvolution 1/1", c_full(1, 1), True),
    ("FullConvolution from an empty level", c_full(3, 2, 0), True),
    ("empty scene", c_empty_scene, False),
    ("BL input with a trailing empty sample", c_bl_trailing_empty, False),
    ("AABR_SCATTER=0 AABR_BRICK_SCATTER=0", c_scatter(0, False), False),
    ("AABR_SCATTER=2 AABR_BRICK_SCATTER=0", c_scatter(2, False), False),
    ("AABR_SCATTER=2 AABR_BRICK_SCATTER=1", c_scatter(2, True), False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the list to this file")
    args = ap.parse_args()
    install_hooks()
    lines = []
    for name, case, planned in CASES:
        for order in ORDERS:
            for plan in ((False, True) if planned else (False,)):
                del records[:]
                if plan:
                    with SCN.geom_plan():
                        mds = case(order)
                else:
                    mds = case(order)
                extra = [m for m in mds if not isinstance(m, SCN.Metadata_3)]
                h = digest([m for m in mds if isinstance(m, SCN.Metadata_3)])
                lines.append("%s | %s | %s | %d builder calls%s | %s"
                             % (name, order, "geom_plan" if plan else "immediate", len(records),
                                "".join(" | %r" % (e,) for e in extra), h))
                print(lines[-1], flush=True)
    torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as fo_:
            fo_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
