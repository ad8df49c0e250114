"""The 64-row-tile launch rule of aabr_conv_forward / aabr_conv_forward_bf16, restated from the entry points as they
were before the decision moved into csrc/conv_tiles.h (the inline blocks and the kernel-name ternary of commit
a5b47ec), plus what the launch tables of csrc/conv.hip compile.  tests/test_conv_tiles_host.py holds the header to the
rule; tests/test_gpu_conv_tiles.py runs every listed instance."""
import os
import re

UNSET = -2147483647 - 1                                  # kKnobUnset
KNOBS = ("CONV_WLDS", "CONV_SMALL", "SMALL_WPB", "SMALL_MAX", "CONV_NBW", "CONV_WPB")   # TileKnobs order
KINDS = ("wlds", "small", "wpipe", "buf", "generic", "bf16")                           # TileKind order
G2 = 1 << 31


def cdiv(a, b):
    """C's truncating integer division"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def ceil_div(a, b):
    return cdiv(a + b - 1, b)


def launch(kind, nbw=0, wpb=0, nkc=0, kg=0, aligned=False, adj=False, grid=(0, 0), block=0, lds=0):
    """a TileLaunch as a tuple: kind index, template arguments, grid x / y, block threads, dynamic LDS bytes"""
    return (KINDS.index(kind), nbw, wpb, nkc, kg, int(aligned), int(adj), grid[0], grid[1], block, lds)


def name(t):
    """the kernel instance of a launch tuple, as aabr_conv_last_variant names it"""
    kind, nbw, wpb, nkc, kg, al, adj = t[:7]
    b = lambda v: "true" if v else "false"
    return {"wlds": "k_conv_blocks_mfma_wlds<%d,%d,%s>" % (nbw, nkc, b(al)),
            "small": "k_conv_blocks_mfma_small<%d>" % wpb,
            "wpipe": "k_conv_blocks_mfma_wpipe<%d,%d,true,%s>" % (nbw, wpb, b(adj)),
            "buf": "k_conv_blocks_mfma_buf<%d,%d,%s,%s>" % (nbw, wpb, b(adj), b(al)),
            "generic": "k_conv_blocks_mfma<%d,%d,%s>" % (nbw, wpb, b(al)),
            "bf16": "k_conv_blocks_mfma_bf16<%d,%d,%d,%s>" % (nbw, wpb, kg, b(adj))}[KINDS[kind]]


def fp32(n_in, n_out, V_out, vol, flags, in_bytes, wp_bytes, words_bytes, knobs):
    k_wlds, k_small, k_small_wpb, k_small_max, k_nbw, k_wpb = knobs
    nkc, nnb = ceil_div(n_in, 32), ceil_div(n_out, 16)
    aligned = n_in % 32 == 0
    lean_any = in_bytes < G2 and wp_bytes < G2 and words_bytes < G2 and not (flags >> 8)
    lean = aligned and lean_any
    if nkc <= 2 and in_bytes < G2 and words_bytes < G2 and not (flags >> 8):
        forced = -1 if k_wlds == UNSET else k_wlds
        ntiles = ceil_div(V_out, 64)
        nbw = nw = 0
        cand = 1
        while cand <= 4:
            skip = cand != forced if forced > 0 else (cand != 1 or nnb < 4)
            if not skip and not (cand > 1 and cand // 2 >= nnb):
                w_lds, tile_lds = vol * nkc * cand * 2048, 64 * cand * 16 * 4
                fit = min(cdiv(160 * 1024 - w_lds, tile_lds), 8)
                if fit >= 4:
                    nbw, nw = cand, fit
                    break
            cand <<= 1
        if nbw > 0 and forced != 0:
            slabs = ceil_div(nnb, nbw)
            w_lds, tile_lds = vol * nkc * nbw * 2048, 64 * nbw * 16 * 4
            wgx = ceil_div(ntiles, nw)
            cap = cdiv(256, slabs) if cdiv(256, slabs) > 0 else 1
            wgx = min(wgx, cap)
            while nw > 4 and wgx < cap and ceil_div(ntiles, nw - 1) <= cap:
                nw -= 1
                wgx = ceil_div(ntiles, nw)
            return launch("wlds", nbw=nbw, nkc=nkc, aligned=aligned, grid=(wgx, slabs), block=64 * nw,
                          lds=w_lds + nw * tile_lds)
    smax = 512 if k_small_max == UNSET else k_small_max
    if lean and nkc >= 2 and ceil_div(V_out, 64) * nnb < smax and k_small != 0:
        wpb = 16 if ceil_div(V_out, 64) * nnb < 1024 else 8
        if k_small_wpb in (8, 16):
            wpb = k_small_wpb
        return launch("small", wpb=wpb, grid=(ceil_div(V_out, 64), nnb), block=64 * wpb, lds=wpb * 64 * 16 * 4)
    nbw = 1 if nnb <= 1 else (2 if nnb == 2 else 4)
    while nbw > 1 and ceil_div(V_out, 64) * ceil_div(nnb, nbw) < 512:
        nbw >>= 1
    if nbw == 4 and ceil_div(V_out, 64) * ceil_div(nnb, 4) >= 8192:
        nbw = 2
    if k_nbw in (1, 2, 4) and k_nbw <= nbw:
        nbw = k_nbw
    wgs = ceil_div(V_out, 64) * ceil_div(nnb, nbw)
    best_wpb, best_cost = 2, -1
    for wpb in range(2, (3 if nbw == 4 else 4) + 1):
        lds = wpb * 64 * (nbw * 16) * 4
        per_cu = max(min(cdiv(160 * 1024, lds), cdiv(12 if nbw == 4 else 20, wpb)), 1)
        rounds = ceil_div(wgs, 256 * per_cu)
        if lds > 64 * 1024:
            continue
        cost = rounds * ceil_div(vol, wpb)
        if best_cost < 0 or cost <= best_cost:
            best_cost, best_wpb = cost, wpb
    if 2 <= k_wpb <= (3 if nbw == 4 else 4):
        best_wpb = k_wpb
    kw = dict(nbw=nbw, wpb=best_wpb, grid=(ceil_div(V_out, 64), ceil_div(nnb, nbw)), block=64 * best_wpb,
              lds=best_wpb * 64 * nbw * 16 * 4)
    if lean and nbw == 4 and wgs >= 8192:
        return launch("wpipe", adj=True, **kw)
    if lean and nbw == 4:
        return launch("wpipe", adj=False, **kw)
    if lean:
        return launch("buf", adj=True, aligned=True, **kw)
    if lean_any:
        return launch("buf", adj=True, aligned=False, **kw)
    return launch("generic", aligned=aligned, **kw)


def bf16(n_in, n_out, V_out, vol, flags, in_bytes, wp_bytes, words_bytes, knobs):
    """(plane counts multiples of 32 and buffers below 2 GiB: the entry point refuses anything else)"""
    k_nbw, k_wpb = knobs[4], knobs[5]
    nkc, nnb = ceil_div(n_in, 32), ceil_div(n_out, 16)
    nbw = 2 if nnb == 2 else 4
    if nbw == 4 and ceil_div(V_out, 64) * ceil_div(nnb, 4) < 512:
        nbw = 2
    if k_nbw in (2, 4) and k_nbw <= nbw:
        nbw = k_nbw
    kg = 4 if nkc >= 3 else nkc
    wgs = ceil_div(V_out, 64) * ceil_div(nnb, nbw)
    best_wpb, best_cost = 2, -1
    for wpb in range(2, (3 if nbw == 4 else 4) + 1):
        lds = wpb * 64 * (nbw * 16) * 4
        per_cu = max(min(cdiv(160 * 1024, lds), cdiv(16, wpb)), 1)
        cost = ceil_div(wgs, 256 * per_cu) * ceil_div(vol, wpb)
        if best_cost < 0 or cost <= best_cost:
            best_cost, best_wpb = cost, wpb
    if 2 <= k_wpb <= (3 if nbw == 4 else 4):
        best_wpb = k_wpb
    return launch("bf16", nbw=nbw, wpb=best_wpb, kg=kg, adj=True, grid=(ceil_div(V_out, 64), ceil_div(nnb, nbw)),
                  block=64 * best_wpb, lds=best_wpb * 64 * nbw * 16 * 4)


_ROW = {"WLDS": ("wlds", ("nbw", "nkc", "aligned")), "SMALL": ("small", ("wpb",)),
        "WPIPE": ("wpipe", ("wpb",)), "BUF": ("buf", ("nbw", "wpb", "aligned")),
        "GENERIC": ("generic", ("nbw", "wpb", "aligned")), "BF16": ("bf16", ("nbw", "wpb", "kg"))}
_FIXED = {"wpipe": dict(nbw=4), "buf": dict(adj=True), "bf16": dict(adj=True)}


def compiled_instances():
    """the rows of the launch tables in csrc/conv.hip (AABR_WLDS(1, 1, true), ...) as launch-tuple prefixes"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "automatic-as-built-reconstruction_amd",
                            "csrc", "conv.hip")).read()
    rows = []
    for m in re.finditer(r"^(?!#)(.*)$", src, re.M):
        for r in re.finditer(r"\bAABR_(WLDS|SMALL|WPIPE|BUF|GENERIC|BF16)\(([^()]*)\)", m.group(1)):
            kind, fields = _ROW[r.group(1)]
            args = [a.strip() for a in r.group(2).split(",")]
            vals = {f: (a == "true") if a in ("true", "false") else int(a) for f, a in zip(fields, args)}
            rows.append(launch(kind, **_FIXED.get(kind, {}), **vals)[:7])
    return rows
