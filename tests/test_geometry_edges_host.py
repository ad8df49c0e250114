"""CPU twin of tests/test_gpu_geometry_edges.py: every case of tests/geometry_edges.py is what its name says -- it lies on
the stated side of the kernel constant it is sized from, which is the evidence that the device test reaches the path --
and the two references (the CPU oracle and `brute_rules`) agree on every small case before either judges the device."""
import os

import numpy as np
import pytest

import full_conv_ref as R
import geometry_edges as G
import oracle_lib as O


# ---------------------------------------------------------------------------------------------------- the constants
def test_constants_are_read_from_the_sources():
    assert set(G.K) == {"kScanThreads", "kScanItems", "kInlinePrefixBlocks", "kBsThreads", "kBsItems", "kMaxCoord"}
    assert all(isinstance(v, int) and v > 0 for v in G.K.values())
    assert G.MAX_COORD + 1 < 1 << 16                       # 16 bits per field of the key, biased by one
    from sparseconvnet import SCN
    assert G.max_samples() == SCN.MAX_SAMPLES and SCN.kMaxSpatial == G.MAX_COORD + 1
    # the one literal of this kind in geometry_edges.py: k_scan_blockprefix is launched with 1024 threads and steps by them
    src = open(os.path.join(G.CSRC, "geometry.hip")).read()
    assert "k_scan_blockprefix, dim3(1), dim3(%d)" % G.PREFIX_STEP in src and "base += %d" % G.PREFIX_STEP in src


# ---------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", sorted(G.A_STRIDED))
def test_a_strided_cases_sit_where_their_names_say(name):
    c = G.case("A strided " + name)
    V = len(c["coords"])
    E = V * c["maxout"]
    assert c["maxout"] == 8 and len(c["counts"]) == 2 and min(c["counts"]) > 0 and V == G.A_STRIDED[name]
    assert (np.diff(c["coords"][:, 3]) >= 0).all()
    if name == "last inline":
        assert E == G.INLINE_LIMIT and G.scan_blocks(E) == G.K["kInlinePrefixBlocks"]
    elif name == "first prefix":
        assert E == G.INLINE_LIMIT + c["maxout"] and G.scan_blocks(E) == G.K["kInlinePrefixBlocks"] + 1
    else:
        assert E > G.INLINE_LIMIT + G.INLINE_LIMIT // 5
    if name != "last inline":       # the prefix kernel's loop takes more than one trip, the last of them a partial one
        assert G.scan_blocks(E) > G.PREFIX_STEP and G.scan_blocks(E) % G.PREFIX_STEP != 0
    assert any(e % 2 for e in c["extent"]) and c["out_spatial"] == G.conv_out_spatial(c["extent"], (3, 3, 3), (2, 2, 2))
    rb, oc = O.convolution_rules(c["coords"], c["size"], c["stride"], c["out_spatial"])
    assert (np.diff(oc[:, 3]) >= 0).all() and set(oc[:, 3]) == {0, 1}, "first-seen output sites are not batch-contiguous"
    assert V < len(oc) < E                                  # several new sites per input site, and duplicates to drop
    # the scan block of the candidate that numbers each output site (its first input row's candidates lie in one block):
    # sites are numbered all along the scan, in the last block too, so every entry of prefix[] is read by somebody
    assert G.SCAN_TILE % c["maxout"] == 0
    blocks = np.unique(_first_rows(rb, len(oc), V) * c["maxout"] // G.SCAN_TILE)
    assert blocks[-1] == G.scan_blocks(E) - 1 and len(blocks) > 0.95 * G.scan_blocks(E)


def _first_rows(rb, V_out, V_in):
    """the smallest input row that reaches each output site; ascending along the list: that is first-seen order"""
    first = np.full(V_out, V_in, np.int64)
    for k in range(rb.vol):
        p = rb.pairs(k)
        np.minimum.at(first, p[:, 1], p[:, 0])
    assert (np.diff(first) >= 0).all() and first.max() < V_in
    return first


def test_a_full_case_sits_just_past_the_boundary():
    c = G.case("A full")
    V = len(c["coords"])
    E = V * c["maxout"]
    assert c["maxout"] == 27 and [n > 0 for n in c["counts"]] == [True, False, True]
    assert G.INLINE_LIMIT < E < G.INLINE_LIMIT + G.INLINE_LIMIT // 50
    assert G.K["kInlinePrefixBlocks"] < G.scan_blocks(E) and G.scan_blocks(E) % G.PREFIX_STEP != 0
    assert c["out_spatial"] == R.out_spatial(c["extent"], c["size"], c["stride"])
    out, rb = R.full_convolution_rules(c["coords"], c["size"], c["stride"])
    assert (np.diff(out[:, 3]) >= 0).all() and set(out[:, 3]) == {0, 2}, "first-seen output sites are not batch-contiguous"
    assert rb.total() == E and len(out) < E                                       # deduplication matters
    # candidate u * 27 + k numbers output site o when it is the smallest that reaches o: all along the scan, to its last block
    first = np.full(len(out), E, np.int64)
    for k in range(rb.vol):
        p = rb.pairs(k).astype(np.int64)
        np.minimum.at(first, p[:, 1], p[:, 0] * c["maxout"] + k)
    assert (np.diff(first) > 0).all()
    blocks = np.unique(first // G.SCAN_TILE)
    assert blocks[-1] == G.scan_blocks(E) - 1 and len(blocks) > 0.95 * G.scan_blocks(E)


# ---------------------------------------------------------------------------------------------------- B, C, D: two references
def _same_book(coords, size, stride, out_sp, kind):
    """brute_rules against the oracle: site list row for row, per-offset counts, pair sets"""
    vol = int(np.prod(size))
    if kind == "submanifold":
        rb, oc = O.submanifold_rules(coords, size), np.asarray(coords, np.int64)
    else:
        rb, oc = O.convolution_rules(coords, size, stride, out_sp)
    out, rules = G.brute_rules(coords, size, stride, out_sp, kind)
    np.testing.assert_array_equal(out, oc)
    per = G.rules_by_offset(rules, vol)
    assert rb.vol == vol
    np.testing.assert_array_equal(np.array([len(p) for p in per]), rb.counts)
    for k in range(vol):
        p = rb.pairs(k)
        np.testing.assert_array_equal(G.pair_keys(p[:, 0], p[:, 1]), per[k])
    return rb, oc


def test_b_filters_are_past_one_pass_of_64_offsets_and_the_references_agree():
    c = G.case("B")
    assert len(c["coords"]) == 4000 and len(c["counts"]) == 3 and min(c["counts"]) > 0
    for fs in G.B_SUBMANIFOLD.values():
        assert int(np.prod(fs)) > 64 and all(f % 2 for f in fs)
        rb, _ = _same_book(c["coords"], fs, None, None, "submanifold")
        assert (rb.counts > 0).all()                                              # every offset of both passes has rules
    assert sorted(int(np.prod(f)) for f in G.B_SUBMANIFOLD.values()) == [105, 125]
    for (fs, st), maxout in zip(G.B_STRIDED.values(), (8, 12)):
        assert int(np.prod(fs)) > 64 and G.max_outputs(fs, st) == maxout
        osz = G.conv_out_spatial(c["extent"], fs, st)
        rb, oc = _same_book(c["coords"], fs, st, osz, "strided")
        assert (rb.counts > 0).all() and set(oc[:, 3]) == {0, 1, 2}
    fs, st = G.B_STRIDED["5x5x5 / 3"]
    assert any((e - f) % s for e, f, s in zip(c["extent"], fs, st))               # extent not divisible by the stride


def test_c_sample_counts_and_the_references_agree():
    m = G.max_samples()
    names = G.c_case_names()
    assert len(names) == 6
    for name in names:
        c = G.case("C " + name)
        nb = int(name.split()[0])
        assert nb in (m + 1, m + 2, m + 9) and len(c["counts"]) == nb
        cnt = np.bincount(c["coords"][:, 3], minlength=nb)
        assert cnt.tolist() == c["counts"] and 2700 <= cnt.sum() <= 3300
        empty = [b for b in range(nb) if cnt[b] == 0]
        assert empty == ([1, nb // 2, nb - 1] if name.endswith("three empty") else [])
        assert (np.diff(c["coords"][:, 3]) >= 0).all()
        _, oc = _same_book(c["coords"], c["size"], c["stride"], c["out_spatial"], "strided")
        assert np.flatnonzero(np.bincount(oc[:, 3], minlength=nb) == 0).tolist() == empty
    # which side of the branch a dense case lies on: samples 0 .. MAX_SAMPLES keep their offsets, one more does not
    assert G.case("C %d samples" % (m + 1))["coords"][:, 3].max() == m
    assert G.case("C %d samples" % (m + 2))["coords"][:, 3].max() == m + 1


def test_d_sites_are_the_ends_of_the_key_range_and_the_references_agree():
    c = G.case("D")
    co = c["coords"]
    assert c["extent"] == (65535, 65535, 65535) and co.shape == (12, 4)
    assert co[:, :3].min() == 0 and co.max() == G.MAX_COORD == 65534
    assert np.bincount(co[:, 3])[[0, 1, G.MAX_COORD]].tolist() == [5, 5, 2]
    _, rules = G.brute_rules(co, (3, 3, 3))
    _same_book(co, (3, 3, 3), None, None, "submanifold")
    # 12 centre rules, and inside each of samples 0 and 1 four neighbour pairs -- (0,0,0)-(1,0,0) and three among the sites
    # at the far corner -- seen from both ends
    assert len(rules) == 12 + 2 * 4 * 2
    for fs, st in G.D_STRIDED.values():
        osz = G.conv_out_spatial(c["extent"], fs, st)
        assert osz == (32767, 32767, 32767)
        _same_book(co, fs, st, osz, "strided")
    # 2/2: a coordinate 65534 falls outside the 32767^3 output (OutputRegionCalculator's clamp leaves an empty region), so
    # only the cell at the origin of every sample remains; 3/2: the far corner survives as output cell 32766
    out, rules = G.brute_rules(co, (2, 2, 2), (2, 2, 2), (32767,) * 3, "strided")
    assert out.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, G.MAX_COORD]] and len(rules) == 5
    out, rules = G.brute_rules(co, (3, 3, 3), (2, 2, 2), (32767,) * 3, "strided")
    assert out[:, :3].max() == 32766 and len(out) == 2 + 2 + 2 and len(rules) == 12


# ---------------------------------------------------------------------------------------------------- E
def test_e_holds_more_bricks_than_one_round_of_the_look_back():
    c = G.case("E")
    assert len(c["coords"]) == G.E_SITES and len(c["counts"]) == 2
    assert G.BRICK_LOOKBACK == 64 * G.K["kBsThreads"] * G.K["kBsItems"]
    nbricks = G.occupied_bricks(c["coords"])
    assert nbricks > G.BRICK_LOOKBACK
    assert (nbricks + G.BRICK_CHUNK - 1) // G.BRICK_CHUNK > 65                     # chunks of k_brick_scan<1> with bricks in them
    # the 2/2 level below it: its bricks are the 8 x 8 x 8 blocks of the input level
    b8 = np.array(c["coords"])
    b8[:, :3] >>= 1
    assert G.occupied_bricks(b8) > G.BRICK_LOOKBACK // 2


def test_brute_rules_on_a_hand_made_scene():
    """three sites on a line, one in another sample: the books written out by hand"""
    co = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 3, 0], [0, 0, 1, 1]], np.int64)
    out, rules = G.brute_rules(co, (1, 1, 3))
    assert np.array_equal(out, co)
    assert rules == {(1, 0, 0), (1, 1, 1), (1, 2, 2), (1, 3, 3), (2, 1, 0), (0, 0, 1)}
    out, rules = G.brute_rules(co, (1, 1, 3), (1, 1, 2), (1, 1, 1), "strided")       # one output cell per sample: z 0 .. 2
    assert out.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1]]
    assert rules == {(0, 0, 0), (1, 1, 0), (1, 3, 1)}
    out, rules = G.brute_rules(co, (1, 1, 3), (1, 1, 2), (1, 1, 2), "strided")
    assert out.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]                # site z = 3: window of output 1 (z 2 .. 4)
    assert rules == {(0, 0, 0), (1, 1, 0), (1, 2, 1), (1, 3, 2)}
