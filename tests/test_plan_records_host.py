"""The launch-plan record format without a GPU: sparseconvnet/plan_records.py (the writer's field tables) against
csrc/plan_records.h (the dispatcher's views, through tests/plan_records_host_harness.cpp) and against the slot numbers
of include/aabr_hip.h's prose, which stand below as literals.  Every kind and variant is written with a distinct
sentinel in every named field; the C++ side must read each name back, and the bytes must be those of the full record
packed positionally -- nothing moved."""
import importlib.util
import os
import re
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "automatic-as-built-reconstruction_amd")
RAW = struct.Struct("<ii6i4f4q12Q")      # AabrPlanOp as the header declares it: this file's own reference
ARRAYS = {"i32": 2, "f32": 8, "i64": 12, "p": 16}                 # first position of each array in RAW's tuple


def _load():
    """by file, not through the package: the module needs nothing but `struct`"""
    spec = importlib.util.spec_from_file_location("plan_records_alone", os.path.join(PKG, "sparseconvnet", "plan_records.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load()
BF16 = R.F_BF16

# ---- include/aabr_hip.h, "compiled launch plans": name -> slot per kind, typed in from the prose ---------------------------
_CONV_COMMON = {"in": ("p", 0), "rows_in": ("i64", 0), "out": ("p", 1), "V_out": ("i64", 1), "gather": ("p", 2),
                "vol": ("i32", 2), "bias": ("p", 4), "conv_flags": ("i32", 3),
                "n_in": ("i32", 0), "n_out": ("i32", 1)}           # (the narrow kernel's record carries them unread)
_BWD32 = {"bwd_stats": ("i32", 5), "stats": ("p", 6), "bn_in": ("p", 7), "save_mean": ("p", 8), "save_invstd": ("p", 9),
          "bn_weight": ("p", 10), "bn_bias": ("p", 11), "leak": ("f32", 0)}
_BWD16 = {"bwd_stats": ("i32", 5), "stats": ("p", 6), "bn_in": ("p", 7), "bn_out": ("p", 9), "save_mean": ("p", 8),
          "leak": ("f32", 0)}
HEADER = {
    1: dict(_CONV_COMMON, weight=("p", 3), wpack=("p", 5)),
    2: dict(_CONV_COMMON, tile_rows=("i32", 4), wpack=("p", 5), residual=("p", 3), **dict(_BWD32, **_BWD16)),
    9: dict(_CONV_COMMON, tile_rows=("i32", 4), wpack=("p", 5), residual=("p", 3), parts=("i32", 5), scratch=("p", 6)),
    10: dict(_CONV_COMMON, weight=("p", 3), **_BWD16),
    11: dict(_CONV_COMMON, wpack=("p", 5), residual=("p", 3), **_BWD32),
    3: {"in": ("p", 0), "n_in": ("i32", 0), "d_out": ("p", 1), "n_out": ("i32", 1), "V_out": ("i64", 0), "pairs": ("p", 2),
        "vol": ("i32", 2), "max_chunks": ("i64", 1), "dW": ("p", 3), "d_bias": ("p", 4), "scratch": ("p", 5)},
    4: {"in": ("p", 0), "out": ("p", 1), "rows": ("i64", 0), "planes": ("i32", 0), "save_mean": ("p", 2),
        "save_invstd": ("p", 3), "running_mean": ("p", 4), "running_var": ("p", 5), "weight": ("p", 6), "bias": ("p", 7),
        "eps": ("f32", 0), "momentum": ("f32", 1), "train": ("i32", 1), "leak": ("f32", 2), "scratch": ("p", 8),
        "parts": ("p", 9), "nparts": ("i32", 2)},
    5: {"in": ("p", 0), "d_in": ("p", 1), "out": ("p", 2), "d_out": ("p", 3), "rows": ("i64", 0), "planes": ("i32", 0),
        "save_mean": ("p", 4), "save_invstd": ("p", 5), "weight": ("p", 6), "bias": ("p", 10), "d_weight": ("p", 7),
        "d_bias": ("p", 8), "leak": ("f32", 2), "scratch": ("p", 9), "d_in_add": ("p", 11), "parts": ("i64", 1),
        "nparts": ("i32", 1)},
    6: {"a": ("p", 0), "b": ("p", 1), "out": ("p", 2), "n": ("i64", 0)},
    7: {"in": ("p", 0), "out": ("p", 1), "n": ("i64", 0)},
    12: {"ticket": ("i64", 0)},
}

# ---- the records: (id, kind, flags, names left zero, patch) -------------------------------------------------------------------
# Every name of the kind's HEADER entry gets its sentinel except those listed; `patch`: the convolution record's
# statistics fields arrive through the named patches after the writer, as in a pass.
_FWD = ("bwd_stats", "leak", "bn_in", "save_mean", "save_invstd", "bn_out", "bn_weight", "bn_bias")
_NO32, _NO16 = ("save_invstd", "bn_weight", "bn_bias"), ("bn_out",)
CASES = [
    ("conv", 1, 0, (), None), ("conv bf16", 1, BF16, (), None),
    ("wide plain", 2, 0, _FWD + ("residual", "stats"), None),
    ("wide residual", 2, BF16, _FWD + ("stats",), None),
    ("wide forward statistics", 2, 0, _FWD + ("residual",), "stats"),
    ("wide residual + forward statistics", 2, BF16, _FWD, "stats"),
    ("wide backward statistics fp32", 2, 0, _NO16 + ("residual",), "bwd"),
    ("wide residual + backward statistics fp32", 2, 0, _NO16, "bwd"),
    ("wide backward statistics bf16", 2, BF16, _NO32 + ("residual",), "bwd"),
    ("split", 9, 0, ("residual",), None), ("split residual", 9, BF16, (), None),
    ("narrow plain", 10, 0, _FWD + ("stats",), None),
    ("narrow forward statistics", 10, BF16, _FWD, "stats"),
    ("narrow backward statistics bf16", 10, BF16, (), "bwd"),
    ("single plain", 11, 0, _FWD + ("residual", "stats"), None),
    ("single residual", 11, 0, _FWD + ("stats",), None),
    ("single backward statistics", 11, 0, ("residual",), "bwd"),
    ("single residual + backward statistics", 11, 0, (), "bwd"),
    ("dw", 3, R.F_SIDE, (), None), ("dw bf16", 3, BF16 | R.F_SIDE, (), None),
    ("bn forward", 4, R.F_TAIL, ("parts", "nparts"), None), ("bn forward with partial sums", 4, BF16, (), None),
    ("bn backward", 5, 0, ("parts", "nparts", "d_in_add"), None),
    ("bn backward with partial sums", 5, BF16, ("d_in_add",), None),
    ("bn backward with d_in_add", 5, BF16, ("parts", "nparts"), None),
    ("bn backward with partial sums and d_in_add", 5, 0, (), None),
    ("add", 6, BF16 | R.F_JOIN, (), None), ("cast", 7, R.F_TO_BF16, (), None), ("tail join", 12, 0, (), None),
]


def _names(kind):
    _, fields, overlaps = R.LAYOUT[kind]
    return [f[0] for f in fields + overlaps]


def _sentinel(kind, name):
    """distinct per field of the kind's table; the number format follows the slot's array"""
    k = _names(kind).index(name)
    array = dict((f[0], f[1]) for f in R.LAYOUT[kind][1] + R.LAYOUT[kind][2])[name]
    return {"i32": 1000 + k, "i64": (1 << 40) + k, "p": (1 << 44) + 16 * k, "f32": 0.5 + k}[array]


def _values(kind, zero):
    return {n: _sentinel(kind, n) for n in HEADER[kind] if n not in zero}


def _write(kind, flags, zero, patch):
    """the record as a pass writes it: the layout's writer, then the named patches"""
    writer, fields, overlaps = R.LAYOUT[kind]
    val = _values(kind, zero)
    at = {}                                            # slot -> value: what the writer is handed for the table's name
    for n, array, index in fields + overlaps:
        if n in val:
            assert (array, index) not in at, "a record never carries two names of one slot"
            at[(array, index)] = val[n]
    later = R.CONV_LATER if fields is R.CONV_FIELDS else ()
    patched = {"stats": ("stats",), "bwd": ("bwd_stats", "stats")}.get(patch, ())
    buf = bytearray(R.SIZE * 3)                        # a record in the middle: a writer or patch that strays shows
    args = [0 if n in patched else at.get((a, i), 0) for n, a, i in fields if n not in later]
    writer.pack_into(buf, R.SIZE, kind, flags, *args)
    g = lambda *names: [at.get(next((a, i) for n, a, i in fields if n == m), 0) for m in names]
    if patch == "stats":
        s, o = R.CONV_STATS
        s.pack_into(buf, R.SIZE + o, *g("stats"))
    elif patch == "bwd":
        (s0, o0), (s1, o1) = R.CONV_BWD_STATS
        s0.pack_into(buf, R.SIZE + o0, *g("bwd_stats", "leak"))
        s1.pack_into(buf, R.SIZE + o1, *g("stats", "bn_in", "save_mean", "save_invstd", "bn_weight", "bn_bias"))
    assert not any(buf[:R.SIZE]) and not any(buf[2 * R.SIZE:])
    return bytes(buf[R.SIZE:2 * R.SIZE])


RECORDS = [_write(*c[1:]) for c in CASES]


def _compile(tmp, name, extra=()):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("no hipcc")
    exe = str(tmp / name)
    cmd = [cxx, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-o", exe,
           os.path.join(HERE, "plan_records_host_harness.cpp")]
    return exe, cmd, subprocess.run(cmd + list(extra), capture_output=True, text=True)


def _dump(exe, tmp):
    path = str(tmp / "records.bin")
    with open(path, "wb") as f:
        f.write(b"".join(RECORDS))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = []
    for line in r.stdout.split():
        name, value = line.split("=")
        if name == "kind":
            recs.append((int(value), []))
        else:
            recs[-1][1].append((name, int(value)))
    return recs


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan_records")
    exe, _, r = _compile(tmp, "plan_records_host")
    assert r.returncode == 0, r.stderr
    return _dump(exe, tmp)


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0] if isinstance(v, float) else v


def test_tables_name_every_slot_once_and_declare_their_overlaps():
    assert R.SIZE == RAW.size == 176 and sorted(R.LAYOUT) == sorted(HEADER)
    for kind, (writer, fields, overlaps) in R.LAYOUT.items():
        slots = [f[1:] for f in fields]
        assert writer.size == R.SIZE and len(set(slots)) == len(slots), kind        # two names on a slot: an overlap
        assert all(o[1:] in slots for o in overlaps) and len(set(_names(kind))) == len(fields + overlaps)
        assert set(HEADER[kind]) <= set(_names(kind)), kind
        assert all(0 <= R.offset(a, i) < R.SIZE for _, a, i in fields + overlaps)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_round_trip_python_writer_to_cpp_views(dumped, case):
    _, kind, flags, zero, patch = CASES[case]
    got_kind, got = dumped[case]
    _, fields, overlaps = R.LAYOUT[kind]
    val = _values(kind, zero)
    at = {(a, i): val[n] for n, a, i in fields + overlaps if n in val}
    assert got_kind == kind
    assert [n for n, _ in got] == _names(kind)                     # exactly the table's names: none missing on either side
    for (n, a, i), (_, v) in zip(fields + overlaps, got):
        assert v == _bits(at.get((a, i), 0)), (CASES[case][0], n)
    assert len(set(map(_bits, at.values()))) == len(at)            # distinct sentinels: a read of a wrong slot cannot pass


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bytes_are_those_of_the_positional_record(case):
    _, kind, flags, zero, patch = CASES[case]
    slots = [kind, flags] + [0] * 6 + [0.0] * 4 + [0] * 16
    named = set()
    for n, v in _values(kind, zero).items():
        array, index = HEADER[kind][n]
        slots[ARRAYS[array] + index] = v
        named.add(ARRAYS[array] + index)
    assert RECORDS[case] == RAW.pack(*slots)
    got = RAW.unpack(RECORDS[case])
    assert got[:2] == (kind, flags) and all(got[k] == 0 for k in range(2, len(got)) if k not in named)


def test_views_under_host_sanitizers(dumped, tmp_path):
    exe, cmd, r = _compile(tmp_path, "plan_records_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        subprocess.check_call(cmd)                     # the program itself must compile; only the runtime may be missing
        pytest.skip("host sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    assert _dump(exe, tmp_path) == dumped


def test_no_slot_arithmetic_outside_the_tables():
    """the writer holds no byte offset or record size of its own, the dispatcher reads no slot by number"""
    src = open(os.path.join(PKG, "sparseconvnet", "planExecutor.py")).read()
    assert not re.findall(r"\b176\b|\+ 128|\+ 32\b|5 \* 4|6 \* 8|o \+ 28|struct\.|_OP\b", src)
    hip = open(os.path.join(PKG, "csrc", "plan.hip")).read()
    geom = hip.index('extern "C" int aabr_geom_run(')
    hits = [m.start() for m in re.finditer(r"p\[[0-9]+\]|\.i32\[|\.i64\[|\.f32\[", hip)]
    assert hits and min(hits) > geom and max(hits) < hip.index("// ---- mailbox")
