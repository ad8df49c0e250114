"""The launch-plan record format, Python side: which slot of an `AabrPlanOp` (include/aabr_hip.h: 176 bytes,
kind, flags, i32[6], f32[4], i64[4], p[12]) holds which operand, per record layout.  csrc/plan_records.h is the same
table on the C++ side; tests/test_plan_records_host.py writes records here, reads them there and compares both with
the slot numbers of the header's prose.  A new slot goes into both tables and into that prose.

Pure: `struct` only, so it loads without torch or a device.

A table lists (field name, array, index) for every slot its layout uses, in slot order; the layout's writer is a
precompiled `struct.Struct` over the whole record that takes kind, flags and then one value per table line, in that
order, and writes zeros into every slot the table does not name:

    BN_FWD.pack_into(buf, off, K_BNF, flags, planes, train, nparts, eps, momentum, leak, rows, A[x], A[y], ...)
"""
import struct

SIZE = 176
K_CONV, K_WIDE, K_DW, K_BNF, K_BNB, K_ADD, K_CAST, K_WSPLIT, K_NARROW, K_SINGLE = 1, 2, 3, 4, 5, 6, 7, 9, 10, 11
K_TAIL_JOIN = 12
F_BF16, F_TO_BF16, F_SIDE, F_JOIN, F_TAIL = 1, 2, 4, 8, 16

_ARRAYS = {"i32": (8, "i", 6), "f32": (32, "f", 4), "i64": (48, "q", 4), "p": (80, "Q", 12)}   # first byte, format, slots

# The five convolution kinds share one layout; CONV_LATER names the BatchNorm side of a backward-statistics write-out,
# which the writer leaves zero and the BatchNorm-backward record behind the convolution fills in (CONV_BWD_STATS).
CONV_FIELDS = (
    ("n_in", "i32", 0), ("n_out", "i32", 1), ("vol", "i32", 2), ("conv_flags", "i32", 3), ("tile_rows", "i32", 4),
    ("bwd_stats", "i32", 5),        # 1: the write-out forms the backward statistics of the BatchNorm whose d_out it is
    ("leak", "f32", 0), ("rows_in", "i64", 0), ("V_out", "i64", 1),
    ("in", "p", 0), ("out", "p", 1), ("gather", "p", 2),     # gather: block stream / pair list / (NARROW) gather table
    ("residual", "p", 3),           # WIDE, WSPLIT, SINGLE: added in the write-out, 0 = none
    ("bias", "p", 4), ("wpack", "p", 5),
    ("stats", "p", 6),              # partial sums of the forward or (bwd_stats) backward statistics, 0 = none
    ("bn_in", "p", 7), ("save_mean", "p", 8),
    ("save_invstd", "p", 9),        # fp32 storage
    ("bn_weight", "p", 10), ("bn_bias", "p", 11))            # fp32 storage only
CONV_LATER = ("leak", "bn_in", "save_mean", "save_invstd", "bn_weight", "bn_bias")
# a second name on a slot above: (name, array, index), and for which records it is the one that applies
CONV_OVERLAPS = (
    ("weight", "p", 3),             # CONV, NARROW: the raw weight (these kernels take no residual)
    ("parts", "i32", 5),            # WSPLIT: parts over the filter offsets (it delivers no backward statistics)
    ("scratch", "p", 6),            # WSPLIT: the parts' fp32 scratch (it delivers no statistics)
    ("bn_out", "p", 9))             # bf16 storage with bwd_stats: the BatchNorm's stored output (the sign)
CONV_DW_FIELDS = (
    ("n_in", "i32", 0), ("n_out", "i32", 1), ("vol", "i32", 2), ("V_out", "i64", 0), ("max_chunks", "i64", 1),
    ("in", "p", 0), ("d_out", "p", 1), ("pairs", "p", 2), ("dW", "p", 3), ("d_bias", "p", 4), ("scratch", "p", 5))
BN_FWD_FIELDS = (
    ("planes", "i32", 0), ("train", "i32", 1), ("nparts", "i32", 2), ("eps", "f32", 0), ("momentum", "f32", 1),
    ("leak", "f32", 2), ("rows", "i64", 0), ("in", "p", 0), ("out", "p", 1), ("save_mean", "p", 2),
    ("save_invstd", "p", 3), ("running_mean", "p", 4), ("running_var", "p", 5), ("weight", "p", 6), ("bias", "p", 7),
    ("scratch", "p", 8),
    ("parts", "p", 9))              # the statistics' partial sums from the producing convolution (nparts of them), 0 = none
BN_BWD_FIELDS = (
    ("planes", "i32", 0), ("nparts", "i32", 1), ("leak", "f32", 2), ("rows", "i64", 0),
    ("parts", "i64", 1),            # the ADDRESS of the partial sums from the producing launch (nparts of them), 0 = none
    ("in", "p", 0), ("d_in", "p", 1), ("out", "p", 2), ("d_out", "p", 3), ("save_mean", "p", 4), ("save_invstd", "p", 5),
    ("weight", "p", 6), ("d_weight", "p", 7), ("d_bias", "p", 8), ("scratch", "p", 9), ("bias", "p", 10),
    ("d_in_add", "p", 11))          # the gradient sum folded into the apply pass, 0 = none
ADD_FIELDS = (("n", "i64", 0), ("a", "p", 0), ("b", "p", 1), ("out", "p", 2))
CAST_FIELDS = (("n", "i64", 0), ("in", "p", 0), ("out", "p", 1))
TAIL_JOIN_FIELDS = (("ticket", "i64", 0),)


def offset(array, index):
    first, fmt, slots = _ARRAYS[array]
    assert 0 <= index < slots
    return first + index * struct.calcsize(fmt)


def _run(fields, at):
    """"<" + one format character per field, pad bytes in the gaps between them; the fields must stand in slot order"""
    fmt = "<"
    for _, array, index in fields:
        o = offset(array, index)
        assert o >= at, "fields out of slot order"
        fmt += "%dx" % (o - at) if o > at else ""
        fmt += _ARRAYS[array][1]
        at = o + struct.calcsize(_ARRAYS[array][1])
    return fmt, at


def _writer(fields, later=()):
    fmt, at = _run([f for f in fields if f[0] not in later], 8)
    s = struct.Struct("<ii" + fmt[1:] + ("%dx" % (SIZE - at) if at < SIZE else ""))
    assert s.size == SIZE
    return s


def _patch(fields, names):
    """((Struct, byte offset in the record), ..) that write the named fields into a record already written: one pair per
    run of adjacent slots, so that nothing between the runs is touched"""
    slot, runs = {f[0]: f for f in fields}, []
    for f in (slot[n] for n in names):
        if runs and offset(*f[1:]) == _run(runs[-1], offset(*runs[-1][0][1:]))[1]:
            runs[-1].append(f)
        else:
            runs.append([f])
    return tuple((struct.Struct(_run(r, offset(*r[0][1:]))[0]), offset(*r[0][1:])) for r in runs)


CONV = _writer(CONV_FIELDS, CONV_LATER)
CONV_DW = _writer(CONV_DW_FIELDS)
BN_FWD = _writer(BN_FWD_FIELDS)
BN_BWD = _writer(BN_BWD_FIELDS)
ADD = _writer(ADD_FIELDS)
CAST = _writer(CAST_FIELDS)
TAIL_JOIN = _writer(TAIL_JOIN_FIELDS)
# fields of a convolution record filled in after it has been written, by the BatchNorm record behind it:
# its forward statistics ...
CONV_STATS, = _patch(CONV_FIELDS, ("stats",))
# ... and the backward-statistics group: (bwd_stats = 1, leak), (stats, bn_in, save_mean, save_invstd | bn_out, bn_weight,
# bn_bias)
CONV_BWD_STATS = _patch(CONV_FIELDS, ("bwd_stats", "leak", "stats", "bn_in", "save_mean", "save_invstd", "bn_weight",
                                      "bn_bias"))

_CONV_LAYOUT = (CONV, CONV_FIELDS, CONV_OVERLAPS)
LAYOUT = {K_CONV: _CONV_LAYOUT, K_WIDE: _CONV_LAYOUT, K_WSPLIT: _CONV_LAYOUT, K_NARROW: _CONV_LAYOUT, K_SINGLE: _CONV_LAYOUT,
          K_DW: (CONV_DW, CONV_DW_FIELDS, ()), K_BNF: (BN_FWD, BN_FWD_FIELDS, ()), K_BNB: (BN_BWD, BN_BWD_FIELDS, ()),
          K_ADD: (ADD, ADD_FIELDS, ()), K_CAST: (CAST, CAST_FIELDS, ()),
          K_TAIL_JOIN: (TAIL_JOIN, TAIL_JOIN_FIELDS, ())}    # kind: (writer, table, overlaps)

_KIND = struct.Struct("<i")
_CONV_BWD_STATS_FLAG, = _patch(CONV_FIELDS, ("bwd_stats",))


def kinds(buf, end):
    """the kind of every record of buf[:end] (tests' debug hooks)"""
    return [_KIND.unpack_from(buf, o)[0] for o in range(0, end, SIZE)]


def conv_bwd_stats(buf, off):
    """a convolution record's `bwd_stats` (tests' debug hooks; 0 in every record of another layout)"""
    s, o = _CONV_BWD_STATS_FLAG
    return s.unpack_from(buf, off + o)[0]
