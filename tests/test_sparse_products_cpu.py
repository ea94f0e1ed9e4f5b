"""The forward sparse product's reference, checked on the host: the plain-loop contract
(tests/sparse_product_cases.py) equals scipy's csr_matmat bit for bit on every case the GPU tests run
(where no row of B repeats a column), every ordinary sum lies within gamma(L+1) * sum |a b| of its fp64
value, and the case builders build what they claim (their own assertions run here)."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_product_cases as C
import spgemm_grad_ref as R

CASES = C.cpu_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_loops_equal_scipy_and_meet_the_bound(case):
    want = C.loops(case)
    assert want.indptr[-1] == want.indices.size == want.values.size > 0
    assert not (want.values == 0).any()
    if case.unique:
        C.assert_product_bits(want, C.spgemm_scipy(case.A, case.B), case.name)
    ok, checked = C.within_bound(want)
    assert ok and checked > 0


def test_builders_build_what_they_claim():
    """The self-checks of the builders (kinds of successor rows present, the 48 KiB boundary from the byte
    formula, m % 3 != 0) ran when CASES was built; here what they feed the kernel is looked at from C's
    side: the reuse rows really alternate between kept and empty results."""
    assert C.lds_switch() == (11912, 11913)
    assert len(C.width_ladder()) == 13 and C.LDS_COLS + 1 in C.width_ladder()
    case = C.reuse_lds()
    m = case.A.shape[0]
    assert m == 16384 + 700 and case.B.shape == (64, 96)
    cnt = np.diff(C.loops(case).indptr)
    first, after = cnt[:700], cnt[C.LDS_GRID:]
    assert first.min() >= 30                                    # wide rows
    assert after.max() == 1 and (after == 0).sum() >= 300       # narrow rows; empty, cancelling, empty B row
    # the all-cancel rows reach products (their pattern product is not empty) and keep nothing
    pat = lambda M: sp.csr_matrix((np.ones(M.nnz, np.float32), M.indices, M.indptr), shape=M.shape)
    reach = np.diff((pat(case.A) @ pat(case.B)).indptr)
    assert ((reach[C.LDS_GRID:] > 1) & (after == 0)).sum() >= 90
    for n in (16385, 20000):
        case = C.reuse_scratch(n)
        assert case.A.shape[0] == 301 and case.A.shape[0] % 3 != 0 and case.B.shape == (40, n)
        cnt = np.diff(C.loops(case).indptr)
        assert cnt[0::4].min() >= 60 and (cnt[1::4] == 1).all() and not cnt[2::4].any() and not cnt[3::4].any()
    assert C.reuse_scratch(16385, C.SCRATCH_SLOTS + 100).A.shape[0] == 2148


def test_special_values_keep_and_drop_what_scipy_does():
    """Each kind's row keeps exactly what SPECIAL_KINDS says, wherever it stands in the order."""
    for n in (40, 16500):
        case, order, col = C.special(n)
        want = C.loops(case)
        expect = {name: kept for name, _, kept in C.SPECIAL_KINDS}
        seen = set()
        for r, name in enumerate(order):
            row = slice(want.indptr[r], want.indptr[r + 1])
            if name == "ordinary":
                assert want.indptr[r + 1] > want.indptr[r]
                continue
            kept = expect[name]
            seen.add(name)
            if kept is None:
                assert want.indptr[r + 1] == want.indptr[r], name
                continue
            assert want.indices[row].tolist() == [col], name
            got = want.values[row][0]
            assert np.isnan(got) if np.isnan(kept) else got == np.float32(kept), (name, got)
        assert len(seen) == len(C.SPECIAL_KINDS)
        sub = np.float32(2.0 ** -146)
        assert 0 < sub < np.finfo(np.float32).tiny               # the kept sum is a subnormal


def test_repeated_columns_in_a_row_of_b_by_hand():
    """A 3 x 3 example with B rows that repeat a column: the products enter in A's order, then in the
    row's stored order.  B = [[c0:1, c2:10, c0:2], [c1:4, c1:-4], [c2:0.5]]."""
    B = C.csr([[(0, 1.0), (2, 10.0), (0, 2.0)], [(1, 4.0), (1, -4.0)], [(2, 0.5)]], 3)
    A = C.csr([[(0, 3.0), (2, 2.0)], [(1, 7.0)], [(2, 1.0), (0, 1.0), (2, 1.0)]], 3)
    got = C.spgemm_loops(A, B)
    # row 0: c0 = 3*1 + 3*2 = 9; c2 = 3*10 + 2*0.5 = 31.  row 1: c1 = 28 - 28 = 0, dropped.
    # row 2: c0 = 1 + 2 = 3; c2 = 0.5 + 10 + 0.5 = 11
    assert got.indptr.tolist() == [0, 2, 2, 4]
    assert got.indices.tolist() == [0, 2, 0, 2]
    assert got.values.tolist() == [9.0, 31.0, 3.0, 11.0]
    assert got.length.tolist() == [2, 2, 2, 3]
    assert got.exact.tolist() == [9.0, 31.0, 3.0, 11.0] and got.mag.tolist() == [9.0, 31.0, 3.0, 11.0]


def test_the_order_of_additions_is_the_contracts():
    """fp32 sums whose value depends on the order: (2^24 + 1) + 1 in A's order is 2^24 (each 1 is lost),
    1 + 1 + 2^24 is 2^24 + 2 -- the loops and scipy agree on both."""
    big, one = 2.0 ** 24, 1.0
    B = C.csr([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]], 1)
    A = C.csr([[(0, big), (1, one), (2, one)], [(1, one), (2, one), (0, big)]], 3)
    got = C.spgemm_loops(A, B)
    assert got.values.tolist() == [big, big + 2]
    C.assert_product_bits(got, C.spgemm_scipy(A, B), "order")
    assert R.within_bound(got.values, got.exact, got.mag, got.length).all()


@pytest.mark.parametrize("sorted_rows", [False, True])
def test_spmm_loops_equal_scipy_on_sorted_rows(sorted_rows):
    A, X = C.spmm_case(701, 5, sorted_rows)
    Y = C.spmm_loops(A, X)
    lens = np.diff(A.indptr)
    assert set(lens.tolist()) == {0, 1, 2, 3, 200}
    assert (Y[4] == np.float32(2.0 ** -146)).all() and not Y[5].any() and not np.signbit(Y[5]).any()
    if sorted_rows:
        with np.errstate(all="ignore"):
            want = np.asarray(A @ X, dtype=np.float32)
        np.testing.assert_array_equal(Y.view(np.uint32), want.view(np.uint32))
    else:
        ids = A.indices[A.indptr[0]:A.indptr[1]]
        assert ids[-1] == ids[0] and (np.diff(ids) < 0).any()      # a repeated column, unsorted
