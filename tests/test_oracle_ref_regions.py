"""Pins the oracle's region geometry to the reference's OWN RectangularRegions.h, through what it returned on the
points below: tests/golden/ref_regions_golden.npz, written by tests/golden/gen_ref_golden.py from
oracle/_ref/libref_regions.so (the reference header compiled where it lies, recipe: oracle/Makefile).  The tests read
the stored vectors only."""
import os

import numpy as np
import pytest

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_regions_golden.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def region_points(seed=0, n=200):
    """the output-region query points of test_output_region_and_offsets"""
    return np.random.default_rng(seed).integers(0, 16, (n, 3)).astype(np.int64)


GEOMS = [((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((1, 1, 4), (1, 1, 1)), ((3, 3, 3), (1, 1, 1)),
         ((2, 3, 4), (2, 1, 3)), ((4, 4, 4), (2, 2, 2))]


OUT_SP = np.array([7, 6, 5], np.int64)
ITER_LB, ITER_UB = np.array([-1, 2, 5], np.int64), np.array([1, 3, 7], np.int64)


def geom_key(size, stride):
    return "geom/%s/%s/" % (size, stride)


@pytest.mark.parametrize("size,stride", GEOMS)
def test_output_region_and_offsets(ref, size, stride):
    key = geom_key(size, stride)
    size = np.array(size, np.int64)
    stride = np.array(stride, np.int64)
    L = O.lib()
    # per query point: the reference's output points (rows [start, start + n)) and, per output point j, its input
    # region's bounds and the query point's offset inside it
    n_ref, rp_all, lbub_all, off_all = ref[key + "n"], ref[key + "points"], ref[key + "lbub"], ref[key + "offset"]
    start = 0
    for i, p in enumerate(region_points()):
        lb, ub = np.zeros(3, np.int64), np.zeros(3, np.int64)
        L.oracle_output_region(p, size, stride, OUT_SP, lb, ub)
        op = np.zeros((64, 3), np.int64)
        n_or = L.oracle_region_points(lb, ub, op)
        assert n_or == n_ref[i]
        rp = rp_all[start:start + n_or]
        np.testing.assert_array_equal(op[:n_or], rp)
        for t, j in enumerate(rp):
            ilb, iub = np.zeros(3, np.int64), np.zeros(3, np.int64)
            L.oracle_input_region(np.ascontiguousarray(j), size, stride, ilb, iub)
            np.testing.assert_array_equal(np.concatenate([ilb, iub]), lbub_all[start + t])
            off_ref = int(off_all[start + t])
            assert L.oracle_region_offset(p, ilb, iub) == off_ref
            assert 0 <= off_ref < size.prod()
        start += n_or
    assert start == rp_all.shape[0]


def test_region_iteration_order_is_last_dim_fastest(ref):
    n = int(ref["iter/n"])
    rp, ro = ref["iter/points"], ref["iter/offsets"]
    assert n == 18 and rp.shape[0] == n
    assert (ro == np.arange(n)).all()  # offset() enumerates in iteration order
    op = np.zeros((32, 3), np.int64)
    assert O.lib().oracle_region_points(ITER_LB, ITER_UB, op) == n
    np.testing.assert_array_equal(op[:n], rp)
    # submanifold region = [p - size/2, p + size - 1 - size/2]
    slb, sub = np.zeros(3, np.int64), np.zeros(3, np.int64)
    O.lib().oracle_submanifold_region(np.array([0, 3, 6], np.int64), np.array([3, 2, 3], np.int64), slb, sub)
    np.testing.assert_array_equal(slb, ITER_LB)
    np.testing.assert_array_equal(sub, ITER_UB)
