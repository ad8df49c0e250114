"""SCN.conv_route, the one kernel-family decision of a forward-form convolution launch, against the decision the layer
code made before it existed (restated below from the library's C queries), over a grid of shapes, with and without
tuning knobs.  Host only: the queries need the library, not a GPU."""
import itertools

import pytest
import torch

import _hip
from sparseconvnet import SCN

PLANES = (9, 16, 32, 33, 64, 96, 128, 160, 256)
ROWS = (0, 1, 500, 5000, 40000, 300000, 399999, 400000, 2000000)     # bf16 narrow switches on at 400,000 output rows
VOLS = (1, 8, 27)


def reference(n_in, n_out, rows_in, rows_out, vol, bf16, prepacked, residual):
    """(kind, tile_rows, parts): narrow first (not with a residual in the write-out), then the wide kernel, then its
    offset split -- both in bf16 storage with a prepacked weight only -- else the 64-row-tile kernels"""
    lib = _hip.load()
    if rows_out == 0:
        return None, 0, 0
    if not residual and lib.aabr_conv_narrow_ok(n_in, n_out, rows_in, rows_out, vol, 1 if bf16 else 0):
        return "narrow", 0, 0
    if bf16 and not prepacked:
        return "tiles", 0, 0
    T = (lib.aabr_conv_wide_tile_rows_bf16 if bf16 else lib.aabr_conv_wide_tile_rows)(n_in, n_out, rows_in, rows_out,
                                                                                     vol)
    if T:
        return "wide", T, 0
    v = (lib.aabr_conv_wide_split_bf16 if bf16 else lib.aabr_conv_wide_split)(n_in, n_out, rows_in, rows_out, vol)
    if v:
        return "split", v & 0xffff, v >> 16
    return "tiles", 0, 0


def reference_parts(kind, T, bf16, rows_out):
    """the planner's statistics rule: a wide record with tiles of >= 64 rows, one part per tile; a bf16 narrow record,
    one part per workgroup"""
    if kind == "wide" and T >= 64:
        return -(-rows_out // T)
    if kind == "narrow" and bf16:
        return int(_hip.load().aabr_conv_narrow_parts(rows_out))
    return 0


def check_grid(planes=PLANES, rows=ROWS, vols=VOLS):
    kinds = {}
    for n_in, n_out, r, vol, bf16, prepacked, residual in itertools.product(planes, planes, rows, vols, (False, True),
                                                                            (False, True), (False, True)):
        for rows_in in (r, 2 * r + 7):
            want = reference(n_in, n_out, rows_in, r, vol, bf16, prepacked, residual)
            got = SCN.conv_route(n_in, n_out, rows_in, r, vol, bf16, prepacked=prepacked, residual=residual)
            assert (got.kind, got.tile_rows, got.parts, got.bf16) == want + (bf16,), \
                (n_in, n_out, rows_in, r, vol, bf16, prepacked, residual)
            assert got.takes_residual == (got.kind in ("wide", "split"))
            assert got.stats_parts(r) == reference_parts(got.kind, got.tile_rows, bf16, r)
            kinds[got.kind] = kinds.get(got.kind, 0) + 1
    return kinds


def test_conv_route_matches_the_layer_decision():
    kinds = check_grid()
    assert set(kinds) == {None, "narrow", "wide", "split", "tiles"}, kinds     # the grid reaches every family


def test_conv_route_defaults_are_the_prepacked_route_without_residual():
    for args in ((32, 32, 500000, 400000, 27, True), (64, 64, 300000, 300000, 27, True), (128, 128, 500, 500, 27, False)):
        assert SCN.conv_route(*args) == SCN.conv_route(*args, prepacked=True, residual=False)


def test_conv_route_narrow_from_400000_bf16_rows():
    assert SCN.conv_route(32, 32, 500000, 400000, 27, True).kind == "narrow"
    assert SCN.conv_route(32, 32, 500000, 399999, 27, True).kind != "narrow"
    assert SCN.conv_route(32, 32, 500000, 400000, 27, False).kind != "narrow"
    assert SCN.conv_route(32, 32, 500000, 400000, 27, True, residual=True).kind != "narrow"


@pytest.mark.parametrize("knob,value", [("CONV_WIDE", 0), ("CONV_NARROW", 1), ("WIDE_ROWS", 48),
                                        ("SPLIT_MIN_ITEMS", 1)])
def test_conv_route_follows_the_tuning_knobs(knob, value):
    """the route is asked afresh on every call: a knob set mid-process moves it the way the C queries move"""
    planes, rows = (32, 64, 128, 256), (0, 100, 500, 5000, 40000, 400000)
    before = {}
    for n_in, n_out, r in itertools.product(planes, planes, rows):
        before[(n_in, n_out, r)] = SCN.conv_route(n_in, n_out, r, r, 27, False)
    _hip.set_knob(knob, value)
    try:
        check_grid(planes, rows, (27,))
        after = {k: SCN.conv_route(k[0], k[1], k[2], k[2], 27, False) for k in before}
    finally:
        _hip.set_knob(knob)
    moved = [k for k in before if before[k] != after[k]]
    assert moved, "%s=%d moved no route" % (knob, value)
    if knob == "CONV_WIDE":
        assert not any(r.kind == "wide" for r in after.values())
    elif knob == "CONV_NARROW":
        assert all(after[k].kind == "narrow" for k in after if k[:2] == (32, 32) and k[2])
    elif knob == "WIDE_ROWS":
        wide = [r for r in after.values() if r.kind == "wide"]
        assert wide and all(r.tile_rows == 48 and r.stats_parts(400000) == 0 for r in wide)
    else:
        assert sum(r.kind == "split" for r in after.values()) > sum(r.kind == "split" for r in before.values())
    assert {k: SCN.conv_route(k[0], k[1], k[2], k[2], 27, False) for k in before} == before     # knob back to unset


class _Gather(object):
    """the three structures a forward-form launch can read, as SCN._Gather builds them; records what was built"""

    def __init__(self, rows, vol=27):
        self.rows, self.vol, self.table, self.built = rows, vol, "table", []

    def blocks(self):
        self.built.append("blocks")
        return "blocks"

    def blocks_wide(self, tile_rows):
        self.built.append(("wide", tile_rows))
        return ("wide", tile_rows)

    def pairs(self):
        self.built.append("pairs")
        return "pairs"


@pytest.mark.parametrize("n_in,n_out,rows,bf16", [(32, 32, 400000, True), (64, 64, 300000, False),
                                                  (128, 128, 2000, False), (16, 16, 5000, False)])
def test_conv_route_stream_is_what_compile_streams_builds(n_in, n_out, rows, bf16):
    route = SCN.conv_route(n_in, n_out, rows, rows, 27, bf16)
    want = {"narrow": "table", "wide": ("wide", route.tile_rows), "split": ("wide", route.tile_rows),
            "tiles": "blocks"}[route.kind]
    g = _Gather(rows)
    assert route.stream(g) == want
    g = _Gather(rows)
    SCN.compile_streams(g, rows, n_in, n_out, torch.bfloat16 if bf16 else torch.float32, weight_grad=True)
    assert g.built == ([] if route.kind == "narrow" else [want]) + ["pairs"]
