"""The backward-statistics form of the single-rule convolution (csrc/conv_single.hip, k_conv_single<KG, true>): the C ABI
called directly (no row threshold), `aabr_conv_forward_single_bwd_stats` against `aabr_conv_forward_single` and
`aabr_conv_forward_wide_bwd_stats` on the same rule book, weight pack, bias, residual and BatchNorm.

Books of 1,500 and 2,777 output rows over a filter volume of 8, one rule per output row: an offset without pairs, one
of 37 pairs (no multiple of 32, less than a chunk), one of exactly a chunk, one of several chunks; the grid
(rows / chunk + 8 parts) has surplus chunks.  n_in and n_out 64 and 128 (two slabs), with and without bias and
residual, leakiness 0 and 0.25, chunks of 256 and 1024 pairs.  Per run:
  1. `out` bit-equal to both other launches;
  2. small-integer inputs and dyadic BatchNorm coefficients: every term and every sum is exact, so the parts added in part
     order equal the sum of k_conv_cs' per-tile parts and an int64 host sum, with zero tolerance;
  3. random inputs: every column total against the exactly rounded (math.fsum) sum of the same float terms, within
     n * 2^-53 * sum |term| for n rows: the bound for an fp64 summation of n terms in any order;
  4. two runs write identical bytes to every part, every part is written, surplus parts are zero.
Then the compiled FPN graph with the route on and off."""
import itertools
import math

import numpy as np
import pytest
import torch

import _hip
from test_gpu_conv_single import _p, _streams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOL = 8
# pairs per offset (they sum to the book's rows), partner rows
BOOKS = {1500: ((0, 37, 700, 256, 5, 170, 170, 162), 400),
         2777: ((1031, 0, 37, 256, 512, 1, 300, 640), 700)}
SETTINGS = list(itertools.product((0, 1), (0, 1), (0.0, 0.25), (256, 1024)))     # bias, residual, leakiness, chunk


@pytest.fixture
def knobs():
    yield
    for k in ("CONV_SINGLE", "SINGLE_ROWS", "SINGLE_CHUNK", "SINGLE_BWD_STATS"):
        _hip.set_knob(k)


def _book(V):
    """gather table [8][V]: output row o has its one rule at offset k(o), partner row i(o); offsets dealt to a random
    permutation of the rows"""
    counts, rows_in = BOOKS[V]
    assert sum(counts) == V and 0 in counts and any(c % 32 for c in counts)
    rng = np.random.default_rng(V)
    table = np.full((VOL, V), -1, np.int32)
    table[np.repeat(np.arange(VOL), counts), rng.permutation(V)] = rng.integers(0, rows_in, V)
    assert ((table >= 0).sum(0) == 1).all() and tuple((table >= 0).sum(1)) == counts
    t = torch.as_tensor(table).to(DEV)
    return (t,) + _streams(t) + (rows_in, counts)


@pytest.fixture(scope="module")
def books():
    return {V: _book(V) for V in BOOKS}


def _inputs(V, rows_in, n_in, n_out, exact, seed):
    """d_out of the coarse level, the layer's weight, bias, residual, and the BatchNorm in front of the convolution (its input
    x, saved statistics, affine coefficients); `exact`: small integers and dyadic coefficients, every product and sum
    below 2^24 and so exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        d = dict(x=ri(-3, 3, rows_in, n_in), W=ri(-2, 2, VOL, n_out, n_in), b=ri(-4, 4, n_out), r=ri(-8, 8, V, n_out),
                 bx=ri(-8, 8, V, n_out) / 4, mean=ri(-4, 4, n_out) / 4, invstd=2.0 ** ri(-1, 1, n_out),
                 bw=ri(-2, 2, n_out) / 2, bb=ri(-4, 4, n_out) / 4)
    else:
        rn = lambda *s: torch.randn(s, generator=g)
        d = dict(x=rn(rows_in, n_in), W=rn(VOL, n_out, n_in) / 8, b=rn(n_out), r=rn(V, n_out), bx=rn(V, n_out),
                 mean=rn(n_out) / 4, invstd=rn(n_out).abs() + 0.5, bw=rn(n_out), bb=rn(n_out) / 2)
    return {k: v.to(DEV) for k, v in d.items()}


def _launches(bk, V, n_in, n_out, bias, residual, leak, chunk, t, T=64):
    """the three launches; returns (out new, out plain, out wide, parts new [P][2][n_out] of a first and a second run, the wide
    kernel's per-tile parts)"""
    lib = _hip.load()
    table, pairs, blocks, rows_in, counts = bk
    _hip.set_knob("SINGLE_CHUNK", chunk)
    b, r = (t["b"] if bias else None), (t["r"] if residual else None)
    wpack = torch.empty(lib.aabr_conv_wpack_floats(VOL, n_in, n_out), dtype=torch.float32, device=DEV)
    _hip.check(lib.aabr_conv_pack_weights(_p(t["W"]), VOL, n_in, n_out, 1, _p(wpack), _hip.stream()))
    P = int(lib.aabr_conv_single_bwd_stats_parts(V, VOL, chunk))
    assert P == V // chunk + VOL
    bn = (_p(t["bx"]), _p(t["mean"]), _p(t["invstd"]), _p(t["bw"]), _p(t["bb"]), leak)
    outs, parts = [], []
    for fill in (float("nan"), -1.0):      # two runs over differently filled buffers: every part is written, the same bytes
        out = torch.full((V, n_out), 7.0, device=DEV)
        st = torch.full((P, 2, n_out), fill, dtype=torch.float64, device=DEV)
        _hip.check(lib.aabr_conv_forward_single_bwd_stats(_p(t["x"]), n_in, rows_in, _p(out), n_out, V, _p(pairs), VOL, _p(b),
                                                          3, _p(wpack), _p(r), _p(st), *bn, _hip.stream()))
        assert lib.aabr_conv_last_variant().decode() == "k_conv_single<%d,bwd_stats>" % (n_in // 32)
        outs.append(out)
        parts.append(st)
    plain = torch.full((V, n_out), -7.0, device=DEV)
    _hip.check(lib.aabr_conv_forward_single(_p(t["x"]), n_in, rows_in, _p(plain), n_out, V, _p(pairs), VOL, _p(b), 3, _p(wpack),
                                            _p(r), _hip.stream()))
    wide = torch.full((V, n_out), -9.0, device=DEV)
    wst = torch.full(((V + T - 1) // T, 2, n_out), float("nan"), dtype=torch.float64, device=DEV)
    _hip.check(lib.aabr_conv_forward_wide_bwd_stats(_p(t["x"]), n_in, rows_in, _p(wide), n_out, V, _p(blocks), T, VOL, _p(b), 3,
                                                    _p(wpack), _p(r), _p(wst), *bn, _hip.stream()))
    assert lib.aabr_conv_last_variant().decode().startswith("k_conv_cs<")
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    return outs[0], plain, wide, parts[0], parts[1], wst


def _check_parts(p0, p1, counts, chunk):
    """two runs: identical bytes in every part; the parts past the book's chunks are zero"""
    assert torch.equal(p0.view(torch.int64), p1.view(torch.int64))
    used = sum((c + chunk - 1) // chunk for c in counts)
    assert used < p0.size(0)
    assert not bool(p0[used:].view(torch.int64).any())          # (+0.0: all bits clear)
    assert bool(torch.isfinite(p0).all())


def _terms(t, v, leak):
    """the float terms of the write-out, on the host in numpy fp32 (no contraction): d and (x - mean) * d as fp64"""
    f = lambda a: a.cpu().numpy()
    x, mean = f(t["bx"]), f(t["mean"])
    bwc = f(t["invstd"]) * f(t["bw"])
    bbc = -mean * bwc + f(t["bb"])
    o = x * bwc + bbc
    vv = f(v)
    d = np.where(o > np.float32(0), vv, vv * np.float32(leak)).astype(np.float32)
    return d.astype(np.float64), (x - mean).astype(np.float64) * d.astype(np.float64)


@pytest.mark.parametrize("n_in,n_out", [(64, 64), (64, 128), (128, 64), (128, 128)])
@pytest.mark.parametrize("V", sorted(BOOKS))
def test_exact_sums_equal_the_wide_kernel_and_an_integer_host_sum(knobs, books, V, n_in, n_out):
    bk = books[V]
    for i, (bias, residual, leak, chunk) in enumerate(SETTINGS):
        t = _inputs(V, bk[3], n_in, n_out, True, 100 * V + i)
        new, plain, wide, p0, p1, wst = _launches(bk, V, n_in, n_out, bias, residual, leak, chunk, t)
        case = (bias, residual, leak, chunk)
        assert torch.equal(new, plain) and torch.equal(new, wide), case
        _check_parts(p0, p1, bk[4], chunk)
        got, want = p0.sum(0), wst.sum(0)      # (exact dyadic sums: any order gives the same doubles)
        assert torch.equal(got, want), (case, float((got - want).abs().max()))
        # int64 host sum of the same terms: d in quarters, x - mean in quarters
        d, xd = _terms(t, new, leak)
        d4 = np.rint(d * 4).astype(np.int64)
        xm4 = np.rint((t["bx"] - t["mean"]).cpu().numpy().astype(np.float64) * 4).astype(np.int64)
        assert (d4 == d * 4).all() and (xm4 * d4 == xd * 16).all()
        assert (got[0].cpu().numpy() * 4 == d4.sum(0)).all(), case
        assert (got[1].cpu().numpy() * 16 == (xm4 * d4).sum(0)).all(), case
        assert int(np.abs(d4).sum()) > 0 and (leak == 0.0) == bool(((d == 0) & (new.cpu().numpy() != 0)).any())


@pytest.mark.parametrize("n_in,n_out", [(64, 64), (64, 128), (128, 64), (128, 128)])
@pytest.mark.parametrize("V", sorted(BOOKS))
def test_random_inputs_within_the_fp64_summation_bound(knobs, books, V, n_in, n_out):
    bk = books[V]
    worst = 0.0
    for i, (bias, residual, leak, chunk) in enumerate(SETTINGS):
        t = _inputs(V, bk[3], n_in, n_out, False, 200 * V + i)
        new, plain, wide, p0, p1, wst = _launches(bk, V, n_in, n_out, bias, residual, leak, chunk, t)
        case = (bias, residual, leak, chunk)
        assert torch.equal(new, plain) and torch.equal(new, wide), case
        _check_parts(p0, p1, bk[4], chunk)
        got = p0.sum(0).cpu().numpy()
        for s, terms in enumerate(_terms(t, new, leak)):
            want = np.array([math.fsum(c) for c in terms.T])
            bound = V * 2.0 ** -53 * np.abs(terms).sum(0)
            err = np.abs(got[s] - want)
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))     # (a fully masked column: 0 <= 0)
            assert (err <= bound).all(), (case, s, float((err / bound).max()))
    print("largest error / bound: %.3g" % worst)


def test_compiled_fpn_graph_takes_the_route_and_keeps_its_results(knobs):
    """a small FPN through the compiled graph with SINGLE_ROWS = 0: the input-gradient records of the strided convolutions
    that owe a BatchNorm its backward statistics are k_conv_single records (kind AABR_PLAN_CONV_SINGLE, i32[5] == 1) where
    the run with CONV_SINGLE = 0 has wide ones; maps and input gradient bit-equal, parameter gradients within the bound
    tests/test_gpu_fpn.py holds its two paths to (the BatchNorm sums are added in another partition).  Both runs with
    CONV_WIDE = 1, as in test_gpu_conv_single.py: the route replaces k_conv_cs launches."""
    import synth_scenes as S
    from sparseconvnet import planExecutor
    from test_cabi_and_host import default_fpn
    torch.manual_seed(6)
    net = default_fpn().to(DEV)
    net.compiled_graph = True
    state = {k: v.clone() for k, v in net.state_dict().items()}
    locs, feats = S.make_batch(2, 20000, 41, 20)
    l = torch.as_tensor(locs).to(DEV)

    def run(on):
        _hip.set_knob("CONV_SINGLE", on)
        _hip.set_knob("SINGLE_ROWS", 0)
        _hip.set_knob("SINGLE_BWD_STATS", 1)
        _hip.set_knob("CONV_WIDE", 1)
        net.load_state_dict(state)
        net.train(True)
        net.zero_grad()
        f = torch.as_tensor(feats).to(DEV).requires_grad_(True)
        planExecutor.debug_bwd_stats = recs = []
        try:
            rpn, roi = net([l, f])
            w = [torch.linspace(0.5, 1.5, m.features.numel(), device=DEV).view_as(m.features) for m in rpn + roi]
            sum((m.features * wi).square().mean() for m, wi in zip(rpn + roi, w)).backward()
            torch.cuda.synchronize()
        finally:
            planExecutor.debug_bwd_stats = None
            _hip.set_knob("CONV_WIDE")
        return ([m.features.detach().clone() for m in rpn + roi], f.grad.clone(),
                {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, recs)

    on, off = run(1), run(0)
    K_WIDE, K_SINGLE = planExecutor.K_WIDE, planExecutor.K_SINGLE
    assert len(on[3]) == len(off[3]) == 1
    r_on, r_off = on[3][0], off[3][0]
    routed = [i for i, (k, s) in enumerate(r_on) if k == K_SINGLE and s == 1]
    # 64 -> 64, 64 -> 128 and two 128 -> 128 down-sampling convolutions have an input gradient the kernel serves
    assert len(routed) >= 3, r_on
    assert not any(k == K_SINGLE for k, _ in r_off)
    assert sum(1 for k, s in r_off if k == K_WIDE and s == 1) - sum(1 for k, s in r_on if k == K_WIDE and s == 1) == len(routed)
    for a, b in zip(on[0], off[0]):
        assert torch.equal(a, b)
    assert torch.equal(on[1], off[1])
    assert on[2].keys() == off[2].keys() and len(on[2]) > 100
    exact = 0
    for n in on[2]:
        ga, gb = on[2][n], off[2][n]
        if torch.equal(ga, gb):
            exact += 1
        else:
            assert float((ga - gb).abs().max()) <= 1e-6 * float(ga.abs().max()), n
    print("parameter gradients bit-equal: %d of %d" % (exact, len(on[2])))
