"""The grid and rule-book builders (csrc/geometry.hip, csrc/geom.h, csrc/brick.hip) past everyday sizes, on a real MI355X,
against the CPU oracle, the FullConvolution restatement (tests/full_conv_ref.py) and `brute_rules`
(tests/geometry_edges.py, which also builds the cases; tests/test_geometry_edges_host.py shows that each case lies where
its name says):

  A  the scan of the hash builders at and past kInlinePrefixBlocks blocks (k_scan_blockprefix, the `prefix` branch of
     k_assign_sites<1> with several candidates per site and of k_assign_sites<2>);
  B  filter volumes above 64: the second pass of the brick table builders, the offset decoding of the hash ones;
  C  62, 63 and 70 samples: the per-sample offsets that ride with a level's site count, and k_sample_offsets past 64;
  D  rule books at coordinate 0, coordinate 65534 and sample 65534;
  E  a brick level of more than 65 536 occupied bricks (more than 64 chunks of k_brick_scan);
  F  k_table_to_rulebook at multiples of its 1024-row step.

Integer work: every comparison is exact."""
import numpy as np
import pytest
import torch

import full_conv_ref as R
import geometry_edges as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77


def _scn():
    import sparseconvnet as scn
    return scn


def _lt(v):
    return torch.LongTensor([int(x) for x in v])


def _input(coords, spatial, order):
    """an input-level tensor over distinct, sample-major sites: first-seen rows = the list's order"""
    layer = _scn().InputLayer(3, list(spatial), mode=3)
    layer.site_order = order
    c = torch.as_tensor(np.array(coords, np.int64).reshape(-1, 4))
    return layer([c.to(DEV), torch.zeros((len(c), 1), device=DEV)])


_REF = {}


def _ref(key, make):
    """a reference result, computed once and shared"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _oracle_strided(case_name, size, stride, out_sp):
    """(output sites, rules per offset as sorted keys) of the oracle's Convolution rule book over a case's sites"""
    def make():
        rb, oc = O.convolution_rules(G.case(case_name)["coords"], list(size), list(stride), list(out_sp))
        want = [G.pair_keys(rb.pairs(k)[:, 0], rb.pairs(k)[:, 1]) for k in range(rb.vol)]
        oc.setflags(write=False)
        return oc, want
    return _ref((case_name, tuple(size), tuple(stride)), make)


def _oracle_submanifold(case_name, size):
    return _ref((case_name, tuple(size)), lambda: O.submanifold_rules(G.case(case_name)["coords"], list(size)))


def _rows(dev_coords, ref_coords, order):
    """reference row of every device row: the identity in first-seen order (after checking it), found from the coordinates
    in brick order (after checking the brick-major rule of csrc/geom.h)"""
    dev_coords = np.asarray(dev_coords).reshape(-1, 4)
    if order == "first_seen":
        np.testing.assert_array_equal(dev_coords, ref_coords)
        return np.arange(len(ref_coords))
    r = R.match_rows(dev_coords, ref_coords)
    assert (np.diff(R.brick_major_key(dev_coords)) > 0).all(), "rows are not in brick-major order"
    return r


def _assert_book(tb, want, r_in, r_out):
    """both gather tables of a strided book hold exactly the rules `want` (per offset: sorted keys in_row << 32 | out_row
    in reference rows); r_in / r_out = reference row of every device row.  The counts are the device's own."""
    t_out = tb.out.table.cpu().numpy()              # [vol, V_out]: input row per output row
    t_in = tb.inn.table.cpu().numpy()               # [vol, V_in]: output row per input row
    assert t_out.shape == (len(want), len(r_out)) and t_in.shape == (len(want), len(r_in))
    assert list(tb.rule_counts()) == [len(w) for w in want]
    assert list(tb.inn.rule_counts()) == [len(w) for w in want]
    assert t_out.max() < len(r_in) and t_in.max() < len(r_out) and t_out.min() >= -1 and t_in.min() >= -1
    for k in range(len(want)):
        o = np.flatnonzero(t_out[k] >= 0)
        np.testing.assert_array_equal(G.pair_keys(r_in[t_out[k, o]], r_out[o]), want[k])
        u = np.flatnonzero(t_in[k] >= 0)
        np.testing.assert_array_equal(G.pair_keys(r_in[u], r_out[t_in[k, u]]), want[k])


def _strided_level(x, c_name, size, stride, out_sp, order, pyramid=False):
    """build the level and its book on x's metadata and hold them against the oracle; returns (grid, output sites)"""
    md = x.metadata
    coords = G.case(c_name)["coords"]
    oc, want = _oracle_strided(c_name, size, stride, out_sp)
    r_in = _rows(x.get_spatial_locations().numpy(), coords, order)
    if pyramid:
        md.buildGridsFromInput(x.spatial_size, [(tuple(out_sp), tuple(stride))])
    tb = md.getRuleBook(x.spatial_size, _lt(out_sp), _lt(size), _lt(stride))
    loc = md.getSpatialLocations(_lt(out_sp)).numpy()
    r_out = _rows(loc, oc, order)
    assert md.getNActive(_lt(out_sp)) == len(oc) and (np.diff(loc[:, 3]) >= 0).all()
    _assert_book(tb, want, r_in, r_out)
    return md.grids[tuple(out_sp)], oc


# ---------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name,order", [(n, "first_seen") for n in sorted(G.A_STRIDED)] + [("prefix", "brick")])
def test_a_strided_sites_and_tables_at_the_scan_boundary(name, order):
    c = G.case("A strided " + name)
    x = _input(c["coords"], c["extent"], order)
    assert x.metadata.site_order == order
    _strided_level(x, "A strided " + name, c["size"], c["stride"], c["out_spatial"], order)


def test_a_full_convolution_sites_and_tables_past_the_scan_boundary():
    c = G.case("A full")
    coords = c["coords"]
    def make():
        o, b = R.full_convolution_rules(coords, c["size"], c["stride"])
        return (o, b) + R.tables(b, len(coords), len(o))
    out, rb, t_out, t_in = _ref("A full", make)
    x = _input(coords, c["extent"], "first_seen")
    np.testing.assert_array_equal(x.get_spatial_locations().numpy().reshape(-1, 4), coords)
    new = _scn().Metadata(3)
    osz = c["out_spatial"]
    tb = x.metadata.getFullConvolutionRuleBook(x.spatial_size, _lt(osz), _lt(c["size"]), _lt(c["stride"]), new)
    got = new.getSpatialLocations(_lt(osz)).numpy().reshape(-1, 4)
    np.testing.assert_array_equal(got, out)                           # first-seen order is the contract: row for row
    assert new.getNActive(_lt(osz)) == len(out)
    assert (tb.V_out, tb.V_in, tb.vol) == (len(coords), len(out), 27)
    assert list(tb.rule_counts()) == [len(rb.pairs(k)) for k in range(27)] == [len(coords)] * 27
    assert list(tb.inn.rule_counts()) == [len(coords)] * 27
    np.testing.assert_array_equal(tb.out.table.cpu().numpy(), t_out)  # unique entries: the tables ARE the pair sets
    np.testing.assert_array_equal(tb.inn.table.cpu().numpy(), t_in)


# ---------------------------------------------------------------------------------------------------- B
def _table_of(rb, V):
    """oracle rule book -> gather table [vol, V] (input row per output row, -1)"""
    t = np.full((rb.vol, V), -1, np.int64)
    for k in range(rb.vol):
        p = rb.pairs(k)
        t[k, p[:, 1]] = p[:, 0]
    return t


def _assert_submanifold(x, c_name, fs, order):
    coords = G.case(c_name)["coords"]
    rb = _oracle_submanifold(c_name, fs)
    r = _rows(x.get_spatial_locations().numpy(), coords, order)
    tb = x.metadata.getSubmanifoldRuleBook(x.spatial_size, _lt(fs))
    assert list(tb.rule_counts()) == rb.counts.tolist()
    table = tb.out.table.cpu().numpy()
    assert table.shape == (rb.vol, len(coords))
    inv = np.empty_like(r)
    inv[r] = np.arange(len(r))
    want = _table_of(rb, len(coords))[:, r]                           # oracle partners of the device's rows ...
    want = np.where(want >= 0, inv[np.maximum(want, 0)], -1)          # ... in the device's numbering
    np.testing.assert_array_equal(table, want)
    return tb, rb


@pytest.mark.parametrize("order", G.ORDERS)
@pytest.mark.parametrize("name", sorted(G.B_SUBMANIFOLD))
def test_b_submanifold_filter_volume_above_64(name, order):
    fs = G.B_SUBMANIFOLD[name]
    c = G.case("B")
    x = _input(c["coords"], c["extent"], order)
    tb, rb = _assert_submanifold(x, "B", fs, order)
    if order == "first_seen":         # the reference-format book: pairs in ascending output row within an offset
        got = _scn().SCN.Metadata_3.tableToRuleBook(tb.out.table)
        assert len(got) == rb.vol
        for k in range(rb.vol):
            np.testing.assert_array_equal(got[k].cpu().numpy(), rb.pairs(k))


@pytest.mark.parametrize("order", G.ORDERS)
@pytest.mark.parametrize("name", sorted(G.B_STRIDED))
def test_b_strided_filter_volume_above_64(name, order):
    fs, st = G.B_STRIDED[name]
    c = G.case("B")
    x = _input(c["coords"], c["extent"], order)
    _strided_level(x, "B", fs, st, G.conv_out_spatial(c["extent"], fs, st), order)


# ---------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("order", G.ORDERS)
@pytest.mark.parametrize("name", G.c_case_names())
def test_c_many_samples_through_the_modules(name, order):
    import rpn_glue
    c = G.case("C " + name)
    coords, nb, m = c["coords"], len(c["counts"]), G.max_samples()
    x = _input(coords, c["extent"], order)
    md = x.metadata
    g, oc = _strided_level(x, "C " + name, c["size"], c["stride"], c["out_spatial"], order, pyramid=True)
    cnt = np.bincount(oc[:, 3], minlength=nb).tolist()
    # the offsets are kept when no sample index exceeds MAX_SAMPLES: 62 samples, or 63 of which the last is empty
    keeps = int(coords[:, 3].max()) <= m
    if not name.endswith("three empty"):
        assert keeps == (nb == m + 1)
    if keeps:
        assert isinstance(g.sample_off, list) and len(g.sample_off) == m + 2
        assert g.sample_off == np.searchsorted(oc[:, 3], np.arange(m + 2), "left").tolist()
        if nb <= m + 1:
            assert g.sample_counts(nb) == cnt
        else:                         # 63 samples, the last one empty: the list does not reach its end
            assert g.sample_counts(nb) is None and g.sample_counts(nb - 1) == cnt[:nb - 1]
    else:
        assert g.sample_off is None and g.sample_counts(nb) is None
    assert rpn_glue._site_counts([g], nb, DEV) == [cnt]
    g0 = md.grids[tuple(c["extent"])]
    assert rpn_glue._site_counts([g0, g], nb, DEV) == [np.bincount(coords[:, 3], minlength=nb).tolist(), cnt]


def test_c_sample_offsets_entry_point_past_64_samples():
    import _hip
    lib = _hip.load()
    c = G.case("C %d samples, three empty" % (G.max_samples() + 9))
    coords = c["coords"]
    batch, V = coords[:, 3], len(coords)
    assert len(c["counts"]) == 70 and (np.diff(batch) >= 0).all()
    sc = torch.as_tensor(coords.astype(np.int32)).to(DEV)
    meta = torch.zeros(_hip.META_WORDS, dtype=torch.int32, device=DEV)
    meta[0] = V
    for v_max in (V, V // 2):                                          # the site count is clamped to the caller's bound
        n = min(V, v_max)
        for ms in (1, 62, 63, 64, 65, 200):
            out = torch.full((ms + 2 + 67,), SENTINEL, dtype=torch.int32, device=DEV)
            _hip.check(lib.aabr_sample_offsets(_hip.ptr(sc), _hip.ptr(meta), v_max, ms, _hip.ptr(out), _hip.stream()))
            o = out.cpu().numpy()
            assert o[0] == n
            np.testing.assert_array_equal(o[1:ms + 2], np.searchsorted(batch[:n], np.arange(ms + 1), "left"))
            assert (o[ms + 2:] == SENTINEL).all(), "written past out[1 + max_samples]"


# ---------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("order", G.ORDERS)
def test_d_rule_books_at_the_ends_of_the_key_range(order):
    from sparseconvnet import SCN
    c = G.case("D")
    coords = c["coords"]
    declined = SCN.brick_stats["declined"]
    x = _input(coords, c["extent"], order)
    md = x.metadata
    # a dense brick directory over 65535^3 would not pay: the scene keeps its hash grids, loudly counted
    assert SCN.brick_stats["declined"] == declined + (order == "brick") and md.site_order == "first_seen"
    np.testing.assert_array_equal(x.get_spatial_locations().numpy(), coords)
    _, rules = G.brute_rules(coords, (3, 3, 3))
    want = G.rules_by_offset(rules, 27)
    tb = md.getSubmanifoldRuleBook(x.spatial_size, _lt((3, 3, 3)))
    table = tb.out.table.cpu().numpy()
    assert table.shape == (27, len(coords)) and list(tb.rule_counts()) == [len(w) for w in want]
    for k in range(27):
        o = np.flatnonzero(table[k] >= 0)
        np.testing.assert_array_equal(G.pair_keys(table[k, o], o), want[k])
        a, b = coords[table[k, o]], coords[o]
        assert (a[:, 3] == b[:, 3]).all(), "a rule links two samples"
        assert (np.abs(a[:, :3] - b[:, :3]) <= 1).all(), "a rule links sites that are no neighbours (0 and 65534 alias)"
    for fs, st in G.D_STRIDED.values():
        osz = G.conv_out_spatial(c["extent"], fs, st)
        md = _input(coords, c["extent"], "first_seen").metadata        # (both books reach one output size: one object each)
        out, rules = G.brute_rules(coords, fs, st, osz, "strided")
        tb = md.getRuleBook(_lt(c["extent"]), _lt(osz), _lt(fs), _lt(st))
        np.testing.assert_array_equal(md.getSpatialLocations(_lt(osz)).numpy(), out)
        assert md.getNActive(_lt(osz)) == len(out)
        ident = np.arange(len(coords)), np.arange(len(out))
        _assert_book(tb, G.rules_by_offset(rules, int(np.prod(fs))), *ident)


# ---------------------------------------------------------------------------------------------------- E
@pytest.fixture(params=["native", "renumbered"])
def scatter_form(request):
    """the two ways to a brick-ordered input level (tests/test_gpu_brick.py): the scatter straight into the brick grid, or
    the hash scatter followed by a renumbering of its first-seen sites"""
    from sparseconvnet import SCN
    old = SCN.brick_scatter
    SCN.brick_scatter = request.param == "native"
    yield request.param
    SCN.brick_scatter = old


def test_e_more_than_65536_occupied_bricks(scatter_form):
    c = G.case("E")
    x = _input(c["coords"], c["extent"], "brick")
    md = x.metadata
    g = md.grids[tuple(c["extent"])]
    assert md.site_order == "brick" and g.brick is not None and g.keys is None and g.V == len(c["coords"])
    assert g.brick.nb_cap > G.BRICK_LOOKBACK                           # more than 64 chunks in the scan over the bricks
    _assert_submanifold(x, "E", (3, 3, 3), "brick")                    # (checks the site list: brick-major, the same set)
    _strided_level(x, "E", c["size"], c["stride"], c["out_spatial"], "brick")


# ---------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("V", [1, 1023, 1024, 1025, 2048, 2049])
def test_f_table_to_rulebook_at_its_row_step(V):
    import _hip
    lib = _hip.load()
    table = np.full((3, V), -1, np.int32)
    table[0] = np.arange(V)[::-1] * 3 + 1                             # every row hits
    table[2, ::3] = np.arange(V)[::3] % 997                            # every third row hits; offset 1: no hit
    t = torch.as_tensor(table).to(DEV)
    rules = torch.full((3, V, 2), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((3 + 5,), SENTINEL, dtype=torch.int32, device=DEV)
    _hip.check(lib.aabr_table_to_rulebook(_hip.ptr(t), V, 3, _hip.ptr(rules), _hip.ptr(counts), _hip.stream()))
    r, n = rules.cpu().numpy(), counts.cpu().numpy()
    assert (n[3:] == SENTINEL).all()
    for k in range(3):
        rows = np.flatnonzero(table[k] >= 0)
        assert n[k] == len(rows) == (V, 0, (V + 2) // 3)[k]
        np.testing.assert_array_equal(r[k, :len(rows)], np.stack([table[k, rows], rows], 1))
        assert (r[k, len(rows):] == SENTINEL).all(), "pairs written past the count"
