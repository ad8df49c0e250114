"""The launch rule of the wide convolution kernel k_conv_cs, restated from csrc/conv_wide.hip as it was before the
decision moved into csrc/conv_wide_tiles.h (commit 683f854): the four dispatch queries (aabr_conv_wide_tile_rows, _bf16,
aabr_conv_wide_split, _bf16) and the four launch computations (wide_launch_f32, aabr_conv_forward_wide_split,
wide_launch_bf16, aabr_conv_forward_wide_split_bf16_res), one function each as the file had them, plus the instances its
macros compiled.  tests/test_conv_wide_host.py holds the header to the rule; tests/test_gpu_conv_wide.py runs every listed
release instance."""
from conv_tiles_rule import UNSET, G2, cdiv

KNOBS = ("WIDE_ROWS", "CONV_WIDE", "CONV_WIDE_BF16", "WIDE_SPLIT", "SPLIT_ROWS", "SPLIT_MIN_ITEMS", "SPLIT_TARGET",
         "WIDE_NBUF", "SPLIT_NBUF", "WIDE_NCB", "WIDE_PRIO")                            # WideKnobs order
NO_KNOBS = (UNSET,) * len(KNOBS)
K_WS, MAX_VOL, MAX_TILE_ROWS = 64, 63, 240


def _kn(knobs):
    return dict(zip(KNOBS, knobs))


def wide_words(V, vol, T):
    nt = cdiv(V + T - 1, T)
    return nt * (vol + 1) + nt * (T // 16) * vol * 16


# ---------------------------------------------------------------------------------------------- the dispatch queries
def tile_rows_f32(n_in, n_out, rows_in, V_out, vol, knobs=NO_KNOBS):
    kn = _kn(knobs)
    if n_in <= 0 or n_out <= 0 or (n_in & 31) or (n_out & 63) or vol <= 0 or vol > MAX_VOL:
        return 0
    if rows_in >= (1 << 23) or rows_in * n_in * 4 >= G2:
        return 0
    T = 112 if n_in <= 64 else 128
    slabs = n_out // 64
    if cdiv(V_out + T - 1, T) * slabs <= 512:
        for t in range(64, T, 16):
            if cdiv(V_out + t - 1, t) * slabs <= 512:
                T = t
                break
    v = kn["WIDE_ROWS"]
    if 16 <= v <= MAX_TILE_ROWS and (v & 15) == 0:
        T = v
    if wide_words(V_out, vol, T) * 4 >= G2:
        return 0
    if vol * n_in * n_out * 4 >= G2:
        return 0
    if n_in > 128 and (n_in & 127):
        return 0
    v = kn["CONV_WIDE"]
    if v == 0:
        return 0
    if v == 1:
        return T
    return T if cdiv(V_out + T - 1, T) * (n_out // 64) >= 320 else 0


def bf16_ncb(n_in, n_out, kn):
    if kn["WIDE_NCB"] == 1:
        return 1
    return 2 if (n_out & 127) == 0 and n_in <= 128 else 1


def tile_rows_bf16(n_in, n_out, rows_in, V_out, vol, knobs=NO_KNOBS):
    kn = _kn(knobs)
    if n_in <= 0 or n_out <= 0 or (n_in & 63) or (n_out & 63) or vol <= 0 or vol > MAX_VOL:
        return 0
    if rows_in >= (1 << 23) or rows_in * n_in * 2 >= G2:
        return 0
    if n_in > 256 and (n_in & 255):
        return 0
    ncb = bf16_ncb(n_in, n_out, kn)
    T = 64 if ncb == 2 else 96
    slabs = n_out // (64 * ncb)
    if cdiv(V_out + T - 1, T) * slabs <= 512:
        for t in range(64, T, 16):
            if cdiv(V_out + t - 1, t) * slabs <= 512:
                T = t
                break
    v = kn["WIDE_ROWS"]
    if 16 <= v <= MAX_TILE_ROWS and (v & 15) == 0:
        T = v
    if wide_words(V_out, vol, T) * 4 >= G2:
        return 0
    if vol * n_in * n_out * 2 >= G2:
        return 0
    v = kn["CONV_WIDE_BF16"]
    if v == 0:
        return 0
    if v == 1:
        return T
    return T if cdiv(V_out + T - 1, T) * (n_out // (64 * ncb)) >= 320 else 0


def _split_parts(kn, T, n_in, n_out, V_out, vol, elem):
    """the common end of the two split queries, as each of them spelled it out"""
    items = cdiv(V_out + T - 1, T) * (n_out // 64)
    min_items = 8 if kn["SPLIT_MIN_ITEMS"] == UNSET else kn["SPLIT_MIN_ITEMS"]
    if items < min_items:
        return 0
    target = 768 if kn["SPLIT_TARGET"] == UNSET else kn["SPLIT_TARGET"]
    P = cdiv(target + items - 1, items)
    P = min(P, vol)
    P = min(P, 32)
    v = kn["WIDE_SPLIT"]
    if 2 <= v <= 32:
        P = v if v < vol else vol
    if P < 2:
        return 0
    if wide_words(V_out, vol, T) * 4 >= G2 or vol * n_in * n_out * elem >= G2:
        return 0
    return (P << 16) | T


def split_f32(n_in, n_out, rows_in, V_out, vol, knobs=NO_KNOBS):
    kn = _kn(knobs)
    if n_in <= 0 or n_out <= 0 or (n_in & 31) or (n_out & 63) or vol <= 1 or vol > MAX_VOL or V_out <= 0:
        return 0
    if rows_in >= (1 << 23) or rows_in * n_in * 4 >= G2:
        return 0
    if n_in < 64 or (n_in > 128 and (n_in & 127)):
        return 0
    if kn["WIDE_SPLIT"] == 0:
        return 0
    if cdiv(V_out + 63, 64) * (n_out // 64) >= 320:
        return 0
    T = 96 if V_out >= 1024 else 64
    v = kn["SPLIT_ROWS"]
    if 64 <= v <= 128 and (v & 15) == 0:
        T = v
    return _split_parts(kn, T, n_in, n_out, V_out, vol, 4)


def split_bf16(n_in, n_out, rows_in, V_out, vol, knobs=NO_KNOBS):
    kn = _kn(knobs)
    if n_in <= 0 or n_out <= 0 or (n_in & 63) or (n_out & 63) or vol <= 1 or vol > MAX_VOL or V_out <= 0:
        return 0
    if rows_in >= (1 << 23) or rows_in * n_in * 2 >= G2:
        return 0
    if n_in > 256 and (n_in & 255):
        return 0
    if kn["WIDE_SPLIT"] == 0 or kn["CONV_WIDE_BF16"] == 0:
        return 0
    T = 64
    if cdiv(V_out + 63, 64) * (n_out // 64) >= 320:
        return 0
    v = kn["SPLIT_ROWS"]
    if 64 <= v <= 128 and (v & 15) == 0:
        T = v
    return _split_parts(kn, T, n_in, n_out, V_out, vol, 2)


# ------------------------------------------------------------------------------------------------------ the launches
# A launch is (message, kg, dbg, nbuf, bf16, ncb, split, grid_x, grid_y, lds_bytes, wflip, in_bytes, words_bytes, wp_bytes):
# message None and the rest as launched, message None and zeros for V_out == 0 (nothing is launched), or the text of the
# failed check and zeros.  Pointers are taken as valid and aligned.
EMPTY = (None,) + (0,) * 13


def _refuse(msg):
    return (msg,) + (0,) * 13


def _sizes(planes_mask, planes_msg, n_in, n_out, rows_in, V_out, tile_rows, vol, elem):
    """the checks all four launchers repeat, up to the byte sizes; (refusal or None, in_bytes, words_bytes)"""
    if not (n_in > 0 and n_out > 0 and (n_in & planes_mask) == 0 and (n_out & 63) == 0):
        return _refuse(planes_msg), 0, 0
    if not (vol > 0 and vol <= MAX_VOL and V_out >= 0 and rows_in >= 0):
        return _refuse("bad sizes"), 0, 0
    if not (tile_rows >= 16 and tile_rows <= MAX_TILE_ROWS and (tile_rows & 15) == 0):
        return _refuse("tile_rows: multiple of 16, <= 240"), 0, 0
    if V_out == 0:
        return EMPTY, 0, 0
    if not rows_in > 0:
        return _refuse("null pointer / empty input"), 0, 0
    if not rows_in < (1 << 23):
        return _refuse("too many input rows for the wide block format"), 0, 0
    in_bytes, words_bytes = rows_in * n_in * elem, wide_words(V_out, vol, tile_rows) * 4
    if not (in_bytes < G2 and words_bytes < G2):
        return _refuse("buffers must be < 2 GiB"), 0, 0
    return None, in_bytes, words_bytes


PARTS_MSG = "2 <= parts <= min(32, vol) and a 16-byte aligned scratch of parts x V_out x n_out floats"
DEV_ONLY_MSG = "the timing-experiment variants of k_conv_cs exist in a `make DEV=1` build only"


def launch_f32(n_in, n_out, rows_in, V_out, tile_rows, vol, flags, has_stats, knobs=NO_KNOBS, dev=False):
    kn = _kn(knobs)
    if has_stats and not tile_rows >= 64:
        return _refuse("statistics need tiles of >= 64 rows")
    r, in_bytes, words_bytes = _sizes(31, "plane counts: n_in % 32, n_out % 64", n_in, n_out, rows_in, V_out, tile_rows,
                                      vol, 4)
    if r is not None:
        return r
    dbg = flags >> 8
    nkc = n_in // 32
    wp_bytes = vol * nkc * (n_out // 16) * 2048
    if not wp_bytes < G2:
        return _refuse("packed weights must be < 2 GiB")
    if not (n_in <= 128 or (n_in & 127) == 0):
        return _refuse("n_in above 128 must be a multiple of 128")
    grid = (cdiv(V_out + tile_rows - 1, tile_rows), n_out // 64)
    flip = ((flags >> 1) & 1) | (0 if kn["WIDE_PRIO"] == 0 else 2)
    kg = 4 if nkc >= 4 else nkc
    nbuf = 1 if (kg == 4 or kg <= 2) else 2
    if kn["WIDE_NBUF"] in (1, 2):
        nbuf = kn["WIDE_NBUF"]
    D = 0
    if dev:
        if dbg & 7:
            if kg != 4:
                return _refuse("debug variants exist for n_in >= 128 only")
            nbuf = 2
            D = 4 if dbg & 4 else (dbg & 3)
    elif dbg & 7:
        return _refuse(DEV_ONLY_MSG)
    lds = ((tile_rows + 1) * K_WS + nbuf * 2 * 16 * kg * 32) * 4
    return (None, kg, D, nbuf, 0, 1, 0, grid[0], grid[1], lds, flip, in_bytes, words_bytes, wp_bytes)


def launch_split_f32(parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, knobs=NO_KNOBS):
    kn = _kn(knobs)
    if not (parts >= 2 and parts <= 32 and parts <= vol):
        return _refuse(PARTS_MSG)
    r, in_bytes, words_bytes = _sizes(31, "plane counts: n_in % 32, n_out % 64", n_in, n_out, rows_in, V_out, tile_rows,
                                      vol, 4)
    if r is not None:
        return r
    nkc = n_in // 32
    wp_bytes = vol * nkc * (n_out // 16) * 2048
    if not wp_bytes < G2:
        return _refuse("packed weights must be < 2 GiB")
    if not (n_in <= 128 or (n_in & 127) == 0):
        return _refuse("n_in above 128 must be a multiple of 128")
    grid = (cdiv(V_out + tile_rows - 1, tile_rows), (n_out // 64) * parts)
    flip = ((flags >> 1) & 1) | (0 if kn["WIDE_PRIO"] == 0 else 2) | (parts << 8)
    kg = 4 if nkc >= 4 else nkc
    nbuf = 2 if kn["SPLIT_NBUF"] == 2 else 1
    KG = 2 if kg == 2 else (3 if kg == 3 else 4)       # (kg == 1 fell through to the 128-channel instance: the latent fault)
    lds = ((tile_rows + 1) * K_WS + nbuf * 2 * 16 * KG * 32) * 4
    return (None, KG, 0, nbuf, 0, 1, 1, grid[0], grid[1], lds, flip, in_bytes, words_bytes, wp_bytes)


def launch_bf16(n_in, n_out, rows_in, V_out, tile_rows, vol, flags, has_stats, knobs=NO_KNOBS, dev=False):
    kn = _kn(knobs)
    if has_stats and not tile_rows >= 64:
        return _refuse("statistics need tiles of >= 64 rows")
    r, in_bytes, words_bytes = _sizes(63, "plane counts: n_in % 64, n_out % 64", n_in, n_out, rows_in, V_out, tile_rows,
                                      vol, 2)
    if r is not None:
        return r
    nkc = n_in // 64
    wp_bytes = vol * (n_in // 32) * (n_out // 16) * 1024
    if not wp_bytes < G2:
        return _refuse("packed weights must be < 2 GiB")
    if not (n_in <= 256 or (n_in & 255) == 0):
        return _refuse("n_in above 256 must be a multiple of 256")
    ncb = bf16_ncb(n_in, n_out, kn)
    grid = (cdiv(V_out + tile_rows - 1, tile_rows), n_out // (64 * ncb))
    flip = ((flags >> 1) & 1) | (2 if kn["WIDE_PRIO"] == 1 else 0)
    kg = 4 if nkc >= 4 else nkc
    nbuf = 1
    if kn["WIDE_NBUF"] in (1, 2):
        nbuf = kn["WIDE_NBUF"]
    if not (ncb == 1 or kg <= 2):
        return _refuse("128-column slabs need n_in <= 128")
    D = 0
    if dev and ((flags >> 8) & 4):
        if kg != 2:
            return _refuse("the bf16 phase-clock variant exists for n_in = 128 only")
        D, nbuf = 4, 1
    lds = ((tile_rows + 1) * K_WS * ncb + nbuf * 2 * 16 * kg * 32) * 4
    return (None, kg, D, nbuf, 1, ncb, 0, grid[0], grid[1], lds, flip, in_bytes, words_bytes, wp_bytes)


def launch_split_bf16(parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, knobs=NO_KNOBS):
    if not (parts >= 2 and parts <= 32 and parts <= vol):
        return _refuse(PARTS_MSG)
    r, in_bytes, words_bytes = _sizes(63, "plane counts: n_in % 64, n_out % 64", n_in, n_out, rows_in, V_out, tile_rows,
                                      vol, 2)
    if r is not None:
        return r
    nkc = n_in // 64
    wp_bytes = vol * (n_in // 32) * (n_out // 16) * 1024
    if not wp_bytes < G2:
        return _refuse("packed weights must be < 2 GiB")
    if not (n_in <= 256 or (n_in & 255) == 0):
        return _refuse("n_in above 256 must be a multiple of 256")
    grid = (cdiv(V_out + tile_rows - 1, tile_rows), (n_out // 64) * parts)
    flip = ((flags >> 1) & 1) | (parts << 8)
    kg = 4 if nkc >= 4 else nkc
    lds = ((tile_rows + 1) * K_WS + 2 * 16 * kg * 32) * 4
    return (None, kg, 0, 1, 1, 1, 1, grid[0], grid[1], lds, flip, in_bytes, words_bytes, wp_bytes)


def launch(storage, parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, has_stats, knobs=NO_KNOBS, dev=False):
    """parts == 0: the plain launch of that storage (0 fp32, 1 bf16); otherwise its split"""
    if parts == 0:
        return (launch_bf16 if storage else launch_f32)(n_in, n_out, rows_in, V_out, tile_rows, vol, flags, has_stats, knobs,
                                                        dev)
    return (launch_split_bf16 if storage else launch_split_f32)(parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags,
                                                                knobs)


# ---------------------------------------------------------------------------------------------------- the instances
def compiled_instances(dev=False):
    """(kg, dbg, nbuf, bf16, ncb) of every k_conv_cs the launchers' macros instantiated"""
    out = [(kg, 0, nb, 0, 1) for kg in (1, 2, 3, 4) for nb in (1, 2)]                       # AABR_WIDE_CS
    out += [(kg, 0, nb, 1, ncb) for kg in (1, 2) for ncb in (1, 2) for nb in (1, 2)]        # AABR_WIDE_BF_K
    out += [(kg, 0, nb, 1, 1) for kg in (3, 4) for nb in (1, 2)]                            # AABR_WIDE_BF_K1
    if dev:
        out += [(4, d, nb, 0, 1) for d in (1, 2, 3, 4) for nb in (1, 2)]                    # AABR_WIDE_CS(4, D)
        out += [(2, 4, 1, 1, ncb) for ncb in (1, 2)]                                        # AABR_WIDE_BF_D
    return out


def never_launched(dev=False):
    """compiled by the macro's unused arm: the fp32 debug variants always ran with two stage buffers"""
    return [(4, d, 1, 0, 1) for d in (1, 2, 3, 4)] if dev else []


def split_instances():
    """the instances a split launch runs too (AABR_SPLIT_CS, AABR_SPLIT_BF)"""
    return [(kg, 0, nb, 0, 1) for kg in (2, 3, 4) for nb in (1, 2)] + [(kg, 0, 1, 1, 1) for kg in (1, 2, 3, 4)]


def name(k, split=False):
    """the instance as aabr_conv_last_variant names it"""
    kg, dbg, nbuf, bf16, ncb = k[:5]
    return "k_conv_cs<%d,%d,%d%s%s%s>" % (kg, dbg, nbuf, ",bf16" if bf16 else "", ",x128" if ncb == 2 else "",
                                         ",split" if split else "")
