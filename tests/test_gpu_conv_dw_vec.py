"""The gather form of the weight gradient's 64 x 64-block kernel (csrc/conv_dw.hip k_conv_dw_pairs<cb, nb, float>: an
operand whose tiles are all full and whose pointer is aligned is loaded with one 16- / 8-byte instruction per lane and the
accumulators hold a permutation of the channels; csrc/conv_dw_tiles.h dw_vec_operands) against the scalar form (knob
DW_VEC = 0) through the C ABI: dW and d_bias must be BIT-equal, since every element is the same sum in the same order.
Also: an fp64 sum with the bound of tests/test_gpu_conv_dw.py, identical bytes over two runs, guard words behind dW, d_bias
and the scratch buffer, the same kernel name either way, and the form the query reports.  Books of at most 1500 sites."""
import numpy as np
import pytest
import torch

import _hip
import test_conv_dw_vec_host as H       # _rule: the choice of the form restated
import test_gpu_conv_exact as X         # the rule books of the exact-arithmetic tests (cached for the session)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = 12345.6789
_cache = {}


class HandBook(object):
    """offsets with 0, 1, 15, 16, 17, 63, 64, 65, 130 and 300 rules over 300 output rows (rules written by hand): the ends of
    the 16-pair groups and 64-pair blocks of a wave's range; 130 rules in a 256-pair chunk leave its last wave without a pair,
    300 rules are a full chunk and a chunk of 44 (or, at 1024 pairs per chunk, two waves without a pair)"""
    COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 130, 300)

    def __init__(self):
        rng = np.random.default_rng(17)
        self.vol, self.V_out, self.rows_in = len(self.COUNTS), 300, 211
        t = np.full((self.vol, self.V_out), -1, np.int32)
        for k, c in enumerate(self.COUNTS):
            o = np.sort(rng.choice(self.V_out, c, replace=False))
            t[k, o] = rng.integers(0, self.rows_in, c)
        self.table = torch.as_tensor(t).to(DEV)
        self._w = None

    def pairs(self):
        if self._w is None:
            lib = _hip.load()
            V, vol = self.V_out, self.vol
            nb = (V + 255) // 256
            c = torch.zeros((vol, nb * 256), dtype=torch.int32, device=DEV)
            c[:, :V] = (self.table >= 0).to(torch.int32)
            counts = c.view(vol, nb, 256).sum(2, dtype=torch.int32).contiguous()
            w = torch.empty(max(lib.aabr_offset_pairs_words(V, vol), 1), dtype=torch.int32, device=DEV)
            _hip.check(lib.aabr_build_offset_pairs(_hip.ptr(self.table), _hip.ptr(counts), V, vol, _hip.ptr(w), _hip.stream()))
            self._w = w
        return self._w


def _book(name):
    if name not in _cache:
        if name == "hand":
            _cache[name] = HandBook()
        elif name == "s2down":
            _cache[name] = X.stride2_books()[0]
        elif name == "s2up":
            _cache[name] = X.stride2_books()[1]
        elif name.endswith("x1"):
            _cache[name] = X.sub_book(int(name[:-2]), fs=1)
        else:
            _cache[name] = X.sub_book(int(name))
    return _cache[name]


def _operands(bk, n_in, n_out):
    """rows, output gradients and the fp64 sums, once per (book, planes)"""
    k = ("op", id(bk), n_in, n_out)
    if k not in _cache:
        rng = np.random.default_rng(n_in * 131 + n_out + bk.V_out)
        x = rng.standard_normal((bk.rows_in, n_in)).astype(np.float32)
        g = rng.standard_normal((bk.V_out, n_out)).astype(np.float32)
        t = bk.table.cpu().numpy().reshape(bk.vol, bk.V_out)
        dW = np.zeros((bk.vol, n_in, n_out), np.float64)
        for kk in range(bk.vol):
            o = np.nonzero(t[kk] >= 0)[0]
            dW[kk] = x[t[kk, o]].astype(np.float64).T @ g[o].astype(np.float64)
        _cache[k] = (x, g, dW, g.astype(np.float64).sum(0), [int((t[kk] >= 0).sum()) for kk in range(bk.vol)])
    return _cache[k]


def _shifted(a, off):
    """the array on the device at `off` floats past a 16-byte boundary"""
    buf = torch.full((a.size + 8,), SENT, device=DEV)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def _run(bk, x, g, dw_off=0):
    lib = _hip.load()
    n_in, n_out, V, vol = x.shape[1], g.shape[1], bk.V_out, bk.vol
    cp = lib.aabr_conv_dw_chunk_pairs(V, vol, n_in, n_out)
    mc = (vol * V + cp - 1) // cp + vol
    ns, nw = int(lib.aabr_conv_dw_scratch_floats(mc, n_in, n_out)), vol * n_in * n_out
    scratch = torch.full((ns + GUARD,), SENT, device=DEV)
    wbuf = torch.full((dw_off + nw + GUARD,), SENT, device=DEV)
    bbuf = torch.full((n_out + GUARD,), SENT, device=DEV)
    dW = wbuf[dw_off:dw_off + nw]
    assert dW.data_ptr() % 16 == 4 * dw_off
    mask = lib.aabr_conv_dw_vec_operands(0, _hip.ptr(x), n_in, _hip.ptr(g), n_out, V, vol, mc)
    _hip.check(lib.aabr_conv_backward_weight(_hip.ptr(x), n_in, _hip.ptr(g), n_out, V, _hip.ptr(bk.pairs()), vol, mc,
                                             _hip.ptr(dW), _hip.ptr(bbuf), _hip.ptr(scratch), _hip.stream()))
    variant = lib.aabr_conv_last_variant().decode()
    torch.cuda.synchronize()
    for what, t in (("dW", wbuf[dw_off + nw:]), ("in front of dW", wbuf[:dw_off]), ("scratch", scratch[ns:]),
                    ("d_bias", bbuf[n_out:])):
        assert bool((t == SENT).all()), "guard words behind %s were written" % what
    return dW.clone().view(vol, n_in, n_out), bbuf[:n_out].clone(), variant, mask, cp


# (book, planes in, planes out, pairs per chunk, direct, floats off 16 bytes: input features, output gradients, dW)
CASES = [
    # plane pairs on the 700-site 3^3 book: one, two and four blocks of 16 per side, four tiles, and the three pairs that
    # mix a scalar operand with a vector one (9: one ragged block; 96, 48, 80: a ragged last tile)
    ("700", 16, 16, 256, False, 0, 0, 0), ("700", 32, 32, 256, False, 0, 0, 0), ("700", 32, 64, 256, False, 0, 0, 0),
    ("700", 64, 32, 256, False, 0, 0, 0), ("700", 64, 64, 256, False, 0, 0, 0), ("700", 64, 128, 1024, True, 0, 0, 0),
    ("700", 128, 128, 1024, True, 0, 0, 0), ("700", 9, 32, 256, False, 0, 0, 0), ("700", 96, 64, 1024, True, 0, 0, 0),
    ("700", 48, 80, 256, False, 0, 0, 0),
    # launch forms: direct at 129 sites, 256-pair chunks at 700 (above), 1024-pair chunks at 1500
    ("129", 64, 64, 256, True, 0, 0, 0), ("129", 32, 32, 256, True, 0, 0, 0), ("129", 128, 128, 1024, True, 0, 0, 0),
    ("1500", 64, 128, 1024, False, 0, 0, 0), ("1500", 128, 128, 1024, False, 0, 0, 0), ("1500", 96, 64, 1024, False, 0, 0, 0),
    ("1500", 64, 64, 256, False, 0, 0, 0),
    # filter volumes 1 and 8 (27 above)
    ("700x1", 64, 64, 256, False, 0, 0, 0), ("700x1", 128, 128, 1024, True, 0, 0, 0), ("s2down", 32, 64, 256, False, 0, 0, 0),
    ("s2up", 64, 32, 256, False, 0, 0, 0),
    # the ends of a wave's pair range
    ("hand", 64, 64, 256, False, 0, 0, 0), ("hand", 32, 32, 256, False, 0, 0, 0), ("hand", 64, 128, 1024, True, 0, 0, 0),
    ("hand", 9, 32, 256, False, 0, 0, 0),
    # pointers 4 and 8 bytes off: the operand falls back to dword loads (at two blocks an 8-byte load stays possible); dW 4
    # bytes off in the direct form: no 16-byte stores
    ("700", 64, 64, 256, False, 1, 0, 0), ("700", 64, 64, 256, False, 2, 0, 0), ("700", 64, 64, 256, False, 0, 1, 0),
    ("700", 64, 64, 256, False, 0, 2, 0), ("700", 64, 64, 256, False, 1, 2, 0), ("700", 32, 32, 256, False, 2, 2, 0),
    ("700", 32, 32, 256, False, 1, 1, 0), ("129", 64, 64, 256, True, 0, 0, 1), ("129", 128, 128, 1024, True, 2, 0, 3),
]


@pytest.mark.parametrize("book,n_in,n_out,chunk,direct,off_in,off_out,off_dw", CASES)
def test_vector_form_equals_scalar_form_bit_for_bit(book, n_in, n_out, chunk, direct, off_in, off_out, off_dw):
    bk = _book(book)
    x, g, dW_ref, db_ref, counts = _operands(bk, n_in, n_out)
    if book == "hand":
        assert tuple(counts) == HandBook.COUNTS
    xd, gd = _shifted(x, off_in), _shifted(g, off_out)
    _hip.set_knob("DW_FULL", 0)                     # (128 -> 128: four tiles of the 64 x 64-block kernel)
    try:
        dW, db, v, mask, cp = _run(bk, xd, gd, off_dw)
        dW2, db2, v2, mask2, _ = _run(bk, xd, gd, off_dw)
        _hip.set_knob("DW_VEC", 0)
        try:
            dW0, db0, v0, mask0, _ = _run(bk, xd, gd, off_dw)
        finally:
            _hip.set_knob("DW_VEC", None)
    finally:
        _hip.set_knob("DW_FULL", None)
    assert cp == chunk and (bk.V_out <= cp) == direct, (cp, bk.V_out)
    want = H._rule(0, n_in, n_out, xd.data_ptr(), gd.data_ptr(), H.UNSET)
    assert mask == mask2 == want and mask0 == 0, (mask, mask0, want)
    if off_in == 1:
        assert not mask & 1
    if off_out == 1:
        assert not mask & 2
    if (off_in, off_out) == (0, 0):
        assert mask == (1 if n_in % (16 * H._blocks(n_in)) == 0 and n_in >= 32 else 0) | \
            (2 if n_out % (16 * H._blocks(n_out)) == 0 and n_out >= 32 else 0)
    assert v == v2 == v0 == "k_conv_dw_pairs<%d,%d,float>" % (H._blocks(n_in), H._blocks(n_out)), (v, v0)
    assert torch.equal(dW.view(torch.int32), dW0.view(torch.int32)), "dW: vector and scalar forms differ"
    assert torch.equal(db.view(torch.int32), db0.view(torch.int32)), "d_bias differs"
    assert torch.equal(dW.view(torch.int32), dW2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))
    np.testing.assert_allclose(dW.cpu().numpy(), dW_ref, rtol=1e-4, atol=1e-5 * np.abs(dW_ref).max())
    np.testing.assert_allclose(db.cpu().numpy(), db_ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(db_ref).max()))
    for k, c in enumerate(counts):                  # offsets without a rule: exact zeros
        if c == 0:
            assert not dW[k].any()


def test_bf16_storage_and_the_full_tile_kernel_report_the_scalar_form():
    lib = _hip.load()
    bk = _book("1500")
    x = torch.zeros((bk.rows_in, 128), device=DEV)
    g = torch.zeros((bk.V_out, 128), device=DEV)
    mc = (bk.vol * bk.V_out + 1023) // 1024 + bk.vol
    q = lambda bf: lib.aabr_conv_dw_vec_operands(bf, _hip.ptr(x), 128, _hip.ptr(g), 128, bk.V_out, bk.vol, mc)
    assert q(0) == 3 and q(1) == 0
    _hip.set_knob("DW_FULL_MIN", 8)                 # the full-tile kernel takes this launch: no operand of the block kernel
    try:
        assert q(0) == 0
    finally:
        _hip.set_knob("DW_FULL_MIN", None)
    assert lib.aabr_conv_dw_vec_operands(0, _hip.ptr(x), 128, _hip.ptr(g), 128, 0, bk.vol, mc) == 0


def test_one_layer_through_the_module_path():
    """a 3^3 submanifold layer's backward (sparseconvnet module, autograd): the gradients with the knob off and on"""
    import sparseconvnet as scn
    bk = _book("700")
    torch.manual_seed(5)
    conv = scn.SubmanifoldConvolution(3, 64, 64, 3, True).to(DEV)
    f = torch.randn((bk.rows_in, 64), device=DEV)
    gy = torch.randn((bk.V_out, 64), device=DEV)

    def run(knob):
        _hip.set_knob("DW_VEC", knob)
        try:
            conv.zero_grad()
            leaf = f.clone().requires_grad_(True)
            xx = scn.SparseConvNetTensor()
            xx.metadata, xx.spatial_size, xx.features = bk.x.metadata, bk.x.spatial_size, leaf
            y = conv(xx)
            with torch.autograd.set_multithreading_enabled(False):
                y.features.backward(gy)
            torch.cuda.synchronize()
            return conv.weight.grad.clone(), conv.bias.grad.clone(), leaf.grad.clone()
        finally:
            _hip.set_knob("DW_VEC", None)

    a, b = run(None), run(0)
    for u, w in zip(a, b):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32))
    assert bool(a[0].abs().max() > 0)


@pytest.mark.parametrize("compiled", [False, True])
def test_network_gradients_do_not_depend_on_the_form(compiled):
    """FPN_Net forward and backward on two small scenes, module path and compiled graph: every parameter gradient and the
    input gradient with the knob off are the bits of the default"""
    import synth_scenes as S
    from test_gpu_fpn import _fpn
    torch.manual_seed(11)
    net = _fpn().to(DEV)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    locs, feats = S.make_batch(2, 6000, 47, 20)
    l = torch.as_tensor(locs).to(DEV)

    def run(knob):
        _hip.set_knob("DW_VEC", knob)
        try:
            net.load_state_dict(state)
            net.train(True)
            net.compiled_graph = compiled
            f = torch.as_tensor(feats).to(DEV).requires_grad_(True)
            net.zero_grad()
            rpn, roi = net([l, f])
            sum(m.features.float().square().mean() for m in rpn + roi).backward()
            torch.cuda.synchronize()
            return [f.grad.clone()] + [p.grad.clone() for _, p in sorted(net.named_parameters()) if p.grad is not None]
        finally:
            _hip.set_knob("DW_VEC", None)

    a, b = run(None), run(0)
    assert len(a) == len(b) > 10
    for u, w in zip(a, b):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32))
