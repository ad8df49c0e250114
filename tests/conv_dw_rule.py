"""The weight-gradient launch rule of aabr_conv_backward_weight / aabr_conv_backward_weight_bf16, restated from the entry
point as it was before the decision moved into csrc/conv_dw_tiles.h (conv_backward_weight_t with its AABR_LAUNCH_DW
ladder, dw_chunk, dw_tiling and dw_full_workgroups of csrc/conv.hip at commit a5f2696), plus what the instance tables of
csrc/conv_dw.hip compile.  tests/test_conv_dw_host.py holds the header to the rule; tests/test_gpu_conv_exact.py runs
every listed instance."""
import os
import re

UNSET = -2147483647 - 1                                  # kKnobUnset
KNOBS = ("DW_FULL", "DW_FULL_MIN", "DW_FULL_WGS")        # DwKnobs order
KINDS = ("pairs", "pairs_mfma", "full")                  # DwKind order
REDUCES = ("none", "chunks", "ranges")                   # DwReduce order


def ceil_div(a, b):
    return (a + b - 1) // b                               # (every operand of the rule's divisions is non-negative)


def launch(kind, bf, cb=0, nb=0, chunk=0, direct=False, grid=(0, 0), n_wg=0, reduce="none", tiles=0):
    """a DwLaunch as a tuple: kind index, storage, template arguments, pairs per chunk, direct, grid x / y, workgroups per
    128 x 128 block, the reduce that follows, destination (1: the scratch buffer), 64 x 64-block tiles"""
    return (KINDS.index(kind), int(bf), cb, nb, chunk, int(direct), grid[0], grid[1], n_wg, REDUCES.index(reduce),
            int(not direct), tiles)


def name(k):
    """the kernel instance of a launch tuple (or its first four fields), as aabr_conv_last_variant names it"""
    kind, bf, cb, nb = k[:4]
    return {"pairs": "k_conv_dw_pairs<%d,%d,%s>" % (cb, nb, "bf16" if bf else "float"),
            "pairs_mfma": "k_conv_dw_pairs_bf16<%d,%d>" % (cb, nb),
            "full": "k_conv_dw_full_%s" % ("bf16" if bf else "f32")}[KINDS[kind]]


def chunk_pairs(V, vol, n_in, n_out):
    return 256 if vol * V <= (1 << 21) and n_in * n_out <= 64 * 64 else 1024


def full_workgroups(ci, co, aligned16, max_chunks, vol, V_out, bf, knobs):
    k_full, k_min, k_wgs = knobs
    if ci % 128 or co % 128 or not aligned16 or k_full == 0:
        return 0
    tiles = (ci >> 7) * (co >> 7)
    slots = max_chunks - vol
    if k_wgs > 0:
        return k_wgs if k_wgs <= slots else 0
    if k_min > 0:
        n = slots if slots < 256 // tiles else 256 // tiles
        return n if n >= k_min else 0
    r_est = V_out if vol == 1 else vol * V_out // 3
    if r_est < (150000 if bf else 250000):
        return 0
    n = (512 if r_est >= 600000 else 256) // tiles
    if n > slots:
        n = 256 // tiles
    return n if 1 <= n <= slots else 0


def decide(bf, n_in, n_out, V_out, vol, max_chunks, aligned16, knobs):
    """V_out > 0 and max_chunks > 0 (the entry point answers anything else with two memsets)"""
    mfma16 = bf and n_in % 32 == 0 and n_out % 32 == 0 and aligned16
    ncb, nnb = ceil_div(n_in, 16), ceil_div(n_out, 16)
    cb = 4 if ncb >= 4 else (2 if ncb >= 2 else 1)
    nb = 4 if nnb >= 4 else (2 if nnb >= 2 else 1)
    tiles = ceil_div(ncb, cb) * ceil_div(nnb, nb)
    chunk = chunk_pairs(V_out, vol, n_in, n_out)
    direct = V_out <= chunk
    n_wg = 0 if direct else full_workgroups(n_in, n_out, aligned16, max_chunks, vol, V_out, bf, knobs)
    if n_wg:
        return launch("full", bf, chunk=chunk, grid=(n_wg, (n_in >> 7) * (n_out >> 7)), n_wg=n_wg, reduce="ranges",
                      tiles=tiles)
    kind = "pairs_mfma" if bf and cb > 1 and nb > 1 and mfma16 else "pairs"
    return launch(kind, bf, cb, nb, chunk, direct, (vol if direct else max_chunks, tiles),
                  reduce="none" if direct else "chunks", tiles=tiles)


def compiled_instances():
    """the rows of the instance tables in csrc/conv_dw.hip (AABR_DW_F32(1, 1), ...) as launch-tuple prefixes
    (kind, bf16, cb, nb)"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "automatic-as-built-reconstruction_amd",
                            "csrc", "conv_dw.hip")).read()
    rows = []
    for m in re.finditer(r"^(?!#)(.*)$", src, re.M):
        for r in re.finditer(r"\bAABR_DW_(F32|BF16|MFMA|FULL)\(([^()]*)\)", m.group(1)):
            a = [x.strip() for x in r.group(2).split(",")]
            if r.group(1) == "FULL":
                assert a in (["f32", "false"], ["bf16", "true"]), a
                rows.append((KINDS.index("full"), int(a[1] == "true"), 0, 0))
            else:
                kind = "pairs_mfma" if r.group(1) == "MFMA" else "pairs"
                rows.append((KINDS.index(kind), int(r.group(1) != "F32"), int(a[0]), int(a[1])))
    return rows
