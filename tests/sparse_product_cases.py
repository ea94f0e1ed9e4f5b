"""Shared by the sparse-product tests (CPU and GPU): the forward product's contract in plain loops, the
same product from scipy, the bitwise comparison, and deterministic operands for the places where the
Gustavson kernel (k_spgemm) can go wrong -- a workgroup that walks a second row on one accumulator
(LDS: more than 16384 rows; scratch: fewer slots than rows), the geometry of the output scan (32-column
bitmap words, 2048-column windows, the 48 KiB dynamic-LDS switch, the first scratch width), B rows
around the wave's 64 lanes, B rows that repeat a column, and values at the edges of `sum != 0`.

The contract (srg_spgemm.hip): C[i, j] = ((0 + A[i,k1] B[k1,j]) + A[i,k2] B[k2,j]) + ...
over row i of A in stored order and, inside a row of B, in stored order; every product rounded to fp32
before it is added; sums equal to 0 dropped; columns ascending.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import spgemm_grad_ref as R

LDS_COLS = 16384          # widest accumulator kept in LDS
LDS_GRID = 16384          # workgroups of the LDS launch: more rows than this and a workgroup walks two
SCRATCH_SLOTS = 2048      # accumulators srg_spgemm_scratch_bytes asks for at most
WINDOW_EDGES = (0, 31, 32, 63, 2047, 2048, 2049)   # bitmap-word and scan-window edges

Case = namedtuple("Case", "name A B unique")        # unique: no row of B repeats a column (scipy pins it)
Product = namedtuple("Product", "indptr indices values exact mag length")


def scratch_per(n):
    """Bytes of one scratch accumulator: n sums and their bitmap."""
    return 4 * n + 4 * ((n + 31) // 32)


def lds_bytes(n):
    """Dynamic LDS of the LDS launch at n columns."""
    return 4 * ((n + 3) & ~3) + 4 * ((n + 31) >> 5)


def csr(rows, n_cols):
    """scipy csr (fp32 values, int32 ids) from per-row lists of (column, value), kept in the given
    order: nothing is sorted and nothing is summed."""
    ip = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ip[1:])
    ix = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    v = np.array([x for r in rows for _, x in r], dtype=np.float32)
    return sp.csr_matrix((v, ix, ip), shape=(len(rows), n_cols))


def spgemm_loops(A, B):
    """The contract in plain loops.  Returns Product: (indptr, indices, values) of C and, per kept entry,
    the fp64 value of the same sum, sum |a b| in fp64 and the chain's number of products.  A row of B
    may repeat a column: its products enter the sum in stored order."""
    m, n = A.shape[0], B.shape[1]
    a_ip, a_ix, a_v = A.indptr.tolist(), A.indices.tolist(), A.data.astype(np.float32)
    b_ip, b_ix, b_v = B.indptr.tolist(), B.indices.tolist(), B.data.astype(np.float32)
    acc = np.zeros(n, np.float32)
    exact, mag, length = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    seen = np.zeros(n, bool)
    indptr = np.zeros(m + 1, np.int64)
    out_j, out_v, out_x, out_m, out_l = [], [], [], [], []
    with np.errstate(all="ignore"):
        for r in range(m):
            touched = []
            for e in range(a_ip[r], a_ip[r + 1]):           # A's entries in stored order
                k, a = a_ix[e], a_v[e]
                for q in range(b_ip[k], b_ip[k + 1]):       # B's row in stored order
                    j, b = b_ix[q], b_v[q]
                    if not seen[j]:
                        seen[j] = True
                        touched.append(j)
                    acc[j] = np.float32(acc[j] + np.float32(a * b))
                    p = float(a) * float(b)
                    exact[j] += p
                    mag[j] += abs(p)
                    length[j] += 1
            for j in sorted(touched):                       # columns ascending, zero sums dropped
                if acc[j] != 0:
                    out_j.append(j)
                    out_v.append(acc[j])
                    out_x.append(exact[j])
                    out_m.append(mag[j])
                    out_l.append(length[j])
                acc[j], exact[j], mag[j], length[j], seen[j] = 0.0, 0.0, 0.0, 0, False
            indptr[r + 1] = len(out_j)
    return Product(indptr, np.array(out_j, np.int64), np.array(out_v, np.float32), np.array(out_x, np.float64),
                   np.array(out_m, np.float64), np.array(out_l, np.int64))


def spgemm_scipy(A, B):
    """(indptr, indices, values) of scipy's fp32 A @ B as the forward emits it (R.forward_pattern)."""
    with np.errstate(all="ignore"):
        row, col, val = R.forward_pattern(A, B)
    ip = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=A.shape[0]), out=ip[1:])
    return ip, col, val


def assert_product_bits(got, want, what=""):
    """Structure exactly; fp32 values by their uint32 view, NaN by position (payloads are not pinned)."""
    gp, gi, gv = (np.asarray(a) for a in got[:3])
    wp, wi, wv = (np.asarray(a) for a in want[:3])
    np.testing.assert_array_equal(gp, wp, err_msg=f"{what}: indptr")
    np.testing.assert_array_equal(gi, wi, err_msg=f"{what}: indices")
    assert gv.dtype == np.float32 and wv.dtype == np.float32, f"{what}: values must be fp32"
    nan = np.isnan(wv)
    np.testing.assert_array_equal(np.isnan(gv), nan, err_msg=f"{what}: NaN positions")
    diff = np.ascontiguousarray(gv[~nan]).view(np.uint32) != np.ascontiguousarray(wv[~nan]).view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} fp32 values differ from the reference's bits"


def ordinary(prod):
    """The kept entries the rounding bound gamma(L+1) * sum |a b| speaks about: finite, and with sum |a b|
    at least 2^-102 -- below that a product may lose bits to underflow (absolute error up to 2^-150 each),
    which the relative bound does not cover; 2^-102 * 2^-24 is the smallest normal's ulp, far above it."""
    return np.isfinite(prod.values) & np.isfinite(prod.exact) & (prod.mag >= 2.0 ** -102)


def within_bound(prod):
    """|fp32 chain - fp64 value| <= gamma(L+1) * sum |a b| on the ordinary entries (and how many)."""
    keep = ordinary(prod)
    ok = R.within_bound(prod.values[keep], prod.exact[keep], prod.mag[keep], prod.length[keep])
    return bool(ok.all()), int(keep.sum())


def _vals(rng, size):
    return (rng.standard_normal(size) * 2).astype(np.float32).tolist()


def row_of(rng, cols):
    cols = [int(c) for c in cols]
    return list(zip(cols, _vals(rng, len(cols))))


# ---- accumulator reuse ---------------------------------------------------------------------------------

def _reuse_b(rng, n, n_wide, n_narrow, wide_mid):
    """B for the reuse cases.  Rows [0, n_wide): wide -- columns 0 and n - 1, every narrow column and
    wide_mid more; the last two wide rows are equal (a +v / -v pair of A entries cancels every sum).
    Then n_narrow rows of one middle column each, one empty row, and short random rows.
    Returns (rows, ids of: wide, narrow, empty, the equal pair, the rest)."""
    mid = rng.choice(np.arange(1, n - 1), size=n_narrow, replace=False)
    rows = []
    for _ in range(n_wide):
        more = rng.choice(np.arange(1, n - 1), size=wide_mid, replace=False)
        cols = sorted({0, n - 1} | set(mid.tolist()) | set(more.tolist()))
        rows.append(row_of(rng, cols))
    rows[n_wide - 1] = list(rows[n_wide - 2])
    wide = list(range(n_wide - 2))
    pair = (n_wide - 2, n_wide - 1)
    narrow = list(range(n_wide, n_wide + n_narrow))
    rows += [[(int(c), v)] for c, v in zip(mid, _vals(rng, n_narrow))]
    empty = len(rows)
    rows.append([])
    return rows, wide, narrow, empty, pair


@functools.lru_cache(maxsize=None)
def reuse_lds():
    """m = 16384 + 700 rows over n = 96 columns: workgroup r < 700 of the LDS launch walks row r (wide:
    columns 0 and 95 and most in between) and then row r + 16384 (narrow: one middle column the wide row
    also summed into, or empty, or all sums cancelling, or reaching only B's empty row)."""
    rng = np.random.default_rng(16384)
    m, k, n, first = LDS_GRID + 700, 64, 96, 700
    rows_b, wide, narrow, empty, pair = _reuse_b(rng, n, 10, 30, 40)
    rest = list(range(len(rows_b), k))
    rows_b += [row_of(rng, rng.choice(n, size=rng.integers(1, 7), replace=False)) for _ in rest]
    B = csr(rows_b, n)
    rows_a = []
    for r in range(first):                                          # wide: 1 to 3 entries, the first a wide row of B
        ks = [rng.choice(wide)] + rng.choice(k, size=rng.integers(0, 3)).tolist()
        rows_a.append(row_of(rng, ks))
    for r in range(first, LDS_GRID):                                # rows with a workgroup of their own
        rows_a.append(row_of(rng, rng.choice(k, size=rng.integers(0, 4))))
    kinds = {"empty": 0, "cancel": 0, "empty_b": 0, "narrow": 0}
    for r in range(LDS_GRID, m):                                    # the successors of the wide rows
        kind = ("narrow", "empty", "narrow", "cancel", "narrow", "empty_b", "narrow")[r % 7]
        kinds[kind] += 1
        if kind == "empty":
            rows_a.append([])
        elif kind == "cancel":
            v = _vals(rng, 1)[0]
            rows_a.append([(pair[0], v), (pair[1], -v)])
        elif kind == "empty_b":
            rows_a.append([(empty, 1.5)])
        else:
            rows_a.append(row_of(rng, [rng.choice(narrow)]))
    A = csr(rows_a, k)
    assert A.shape == (m, k) and m > LDS_GRID and np.diff(A.indptr).max() <= 3
    assert all(kinds.values()), kinds                               # every kind of successor exists
    lo = np.array([min(c for c, _ in rows_b[rows_a[r][0][0]]) for r in range(first)])
    hi = np.array([max(c for c, _ in rows_b[rows_a[r][0][0]]) for r in range(first)])
    assert (lo == 0).all() and (hi == n - 1).all()                  # the wide rows span the accumulator
    return Case("reuse_lds", A, B, True)


@functools.lru_cache(maxsize=None)
def reuse_scratch(n, m=301):
    """k = 40, rows in the cycle wide / narrow / empty / all-cancel (the narrow row's column is one the
    wide rows summed into): on one slot each follows the other, on three slots (m % 3 != 0, and 3 and 4
    are coprime) every workgroup still meets all four kinds."""
    rng = np.random.default_rng(n + m)
    k = 40
    rows_b, wide, narrow, empty, pair = _reuse_b(rng, n, 8, 6, 60)
    rows_b += [row_of(rng, rng.choice(n, size=rng.integers(1, 9), replace=False)) for _ in range(len(rows_b), k)]
    B = csr(rows_b, n)
    rows_a = []
    for r in range(m):
        kind = (r + r // SCRATCH_SLOTS) % 4      # row r + 2048 (the capped grid's second row) is the next kind
        if kind == 0:
            rows_a.append(row_of(rng, [rng.choice(wide)] + rng.choice(k, size=rng.integers(0, 3)).tolist()))
        elif kind == 1:
            rows_a.append(row_of(rng, [rng.choice(narrow)]))
        elif kind == 2:
            rows_a.append([] if r % 8 == 2 else [(empty, 2.5)])
        else:
            v = _vals(rng, 1)[0]
            rows_a.append([(pair[0], v), (pair[1], -v)])
    A = csr(rows_a, k)
    assert n > LDS_COLS
    assert m > SCRATCH_SLOTS or m % 3 != 0       # the one- and three-slot calls; past 2048 rows the cap reuses
    return Case(f"reuse_scratch_{n}_{m}", A, B, True)


# ---- widths ------------------------------------------------------------------------------------------------

def lds_switch():
    """(last n whose dynamic LDS fits 48 KiB, first n past it), from the kernel's byte formula."""
    first = next(n for n in range(1, LDS_COLS + 1) if lds_bytes(n) > 48 * 1024)
    assert lds_bytes(first - 1) <= 48 * 1024 < lds_bytes(first)
    return first - 1, first


def width_ladder():
    last, first = lds_switch()
    assert (last, first) == (11912, 11913) and (lds_bytes(last), lds_bytes(first)) == (49140, 49156)
    return (1, 31, 32, 33, 2047, 2048, 2049, 4097, last, first, LDS_COLS - 1, LDS_COLS, LDS_COLS + 1)


@functools.lru_cache(maxsize=None)
def width(n):
    """m = 70, k = 24.  B row 0 holds only column 0, row 1 only n - 1, row 2 both (empty scan windows in
    between), row 3 nothing; the others draw from the word / window edges inside [0, n) and a few random
    columns.  A's rows 0, 1, 2 reach only B's rows 0, 1, 2."""
    rng = np.random.default_rng(n)
    m, k = 70, 24
    edges = sorted({c for c in WINDOW_EDGES + (n - 1,) if 0 <= c < n})
    rows_b = [row_of(rng, [0]), row_of(rng, [n - 1]), row_of(rng, sorted({0, n - 1})), []]
    for _ in range(4, k):
        pick = [c for c in edges if rng.random() < 0.5]
        more = rng.choice(n, size=min(n, int(rng.integers(0, 5))), replace=False).tolist()
        rows_b.append(row_of(rng, sorted(set(pick) | set(more))))
    B = csr(rows_b, n)
    rows_a = [row_of(rng, [0]), row_of(rng, [1]), row_of(rng, [2])]
    rows_a += [row_of(rng, rng.choice(k, size=rng.integers(0, 4), replace=False)) for _ in range(3, m)]
    A = csr(rows_a, k)
    assert set(B.indices.tolist()) >= set(edges)
    return Case(f"width_{n}", A, B, True)


def widths():
    return [width(n) for n in width_ladder()]


# ---- row lengths -------------------------------------------------------------------------------------------

B_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 300)
A_LENGTHS = (0, 1, 2, 65)


@functools.lru_cache(maxsize=None)
def row_length(n):
    """B rows of B_LENGTHS entries (around the wave's 64 lanes per step) in shuffled stored order, then
    short rows up to k = 70; A rows of A_LENGTHS entries in turn (m = 41), the last one listing one row of
    B twice with another in between."""
    rng = np.random.default_rng(n + 7)
    k = 70
    rows_b = [row_of(rng, rng.choice(n, size=length, replace=False)) for length in B_LENGTHS]
    rows_b += [row_of(rng, rng.choice(n, size=rng.integers(0, 6), replace=False)) for _ in range(len(rows_b), k)]
    B = csr(rows_b, n)
    rows_a = []
    for r in range(40):
        length = A_LENGTHS[r % 4]
        ks = rng.choice(k, size=length, replace=False).tolist()
        if length in (1, 2):
            ks[0] = r // 4 % len(B_LENGTHS)                          # every length of B row gets reached
        rows_a.append(row_of(rng, ks))
    rows_a.append(row_of(rng, [5, 2, 5]))                             # the same k twice, not adjacent
    A = csr(rows_a, k)
    assert sorted(set(np.diff(A.indptr).tolist())) == [0, 1, 2, 3, 65]
    assert tuple(np.diff(B.indptr)[:len(B_LENGTHS)].tolist()) == B_LENGTHS
    return Case(f"row_lengths_{n}", A, B, True)


def row_lengths():
    return [row_length(512), row_length(16500)]


# ---- B rows that repeat a column ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def serial_b(n):
    """m = 90, k = 20.  B row 0 repeats a column twice and row 1 three times, never adjacent; row 2 has 70
    entries drawn with repeats (more than one wave's step); the rest are short draws with repeats."""
    rng = np.random.default_rng(n + 90)
    m, k = 90, 20
    c = rng.choice(n, size=6, replace=False).tolist()
    rows_b = [row_of(rng, [c[0], c[1], c[0], c[2]]), row_of(rng, [c[3], c[4], c[3], c[5], c[3]]),
              row_of(rng, rng.choice(min(n, 40), size=70) * (n // min(n, 40)))]
    rows_b += [row_of(rng, rng.choice(n, size=rng.integers(0, 8)) if rng.random() < 0.5 else
                    rng.choice(c, size=rng.integers(2, 6))) for _ in range(3, k)]
    B = csr(rows_b, n)
    rows_a = [row_of(rng, [0]), row_of(rng, [1]), row_of(rng, [2, 0, 1])]
    rows_a += [row_of(rng, rng.choice(k, size=rng.integers(0, 5))) for _ in range(3, m)]
    A = csr(rows_a, k)
    for r, times in ((0, 2), (1, 3)):
        ids = B.indices[B.indptr[r]:B.indptr[r + 1]]
        assert np.bincount(ids).max() == times and (ids[1:] != ids[:-1]).all()
    return Case(f"serial_b_{n}", A, B, False)


# ---- values at the edges of `sum != 0` ---------------------------------------------------------------------

INF = float("inf")
# name -> A's row over the special rows of B below (all on one column), what C keeps of it
SPECIAL_KINDS = (
    ("through_zero", [(0, 1.0), (0, -1.0), (1, 3.0)], 1.5),        # 1*2 + (-1)*2 + 3*0.5: 0 mid-way, kept
    ("cancel", [(0, 1.0), (0, -1.0)], None),                        # 1*2 + (-1)*2 = 0: dropped
    ("subnormal", [(2, 2.0 ** -75), (3, 2.0 ** -75)], 2.0 ** -146),  # 2^-145 - 2^-146: subnormal, kept
    ("underflow", [(4, 2.0 ** -100)], None),                        # 2^-200 rounds to 0: dropped
    ("nan", [(5, INF)], float("nan")),                              # inf * 0: kept
    ("inf", [(6, INF)], INF),                                       # inf * 1: kept
    ("minus_zero", [(5, -1.0)], None),                              # +0 + (-0) = +0: dropped
    ("zero_in_a", [(6, 0.0), (1, 2.0)], 1.0),                       # an explicit zero of A, then 2*0.5
    ("zeros_only", [(6, 0.0), (5, 4.0)], None),                     # explicit zeros of A and of B: dropped
)
SPECIAL_B = (2.0, 0.5, 2.0 ** -70, -(2.0 ** -71), 2.0 ** -100, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def special(n):
    """One row of A per kind of SPECIAL_KINDS plus ordinary rows that sum into the same column, in an
    order where every kind directly follows every kind (itself included) -- the order in which one scratch
    accumulator meets them."""
    rng = np.random.default_rng(n + 149)
    col = n // 2
    rows_b = [[(col, v)] for v in SPECIAL_B]
    k = len(rows_b) + 8
    for _ in range(len(rows_b), k):                                 # ordinary rows, all through `col`
        cols = {col, 0, n - 1} | set(rng.choice(n, size=5, replace=False).tolist())
        rows_b.append([(c, v if rng.random() > 0.2 else 0.0) for c, v in row_of(rng, sorted(cols))])
    B = csr(rows_b, n)
    kinds = [name for name, _, _ in SPECIAL_KINDS] + ["ordinary"]
    entries = {name: row for name, row, _ in SPECIAL_KINDS}
    order = [x for a in kinds for b in kinds for x in (a, b)]
    rows_a = [entries[name] if name != "ordinary" else
              row_of(rng, rng.choice(np.arange(len(SPECIAL_B), k), size=rng.integers(1, 4))) for name in order]
    A = csr(rows_a, k)
    pairs = set(zip(order[:-1], order[1:]))
    assert pairs == {(a, b) for a in kinds for b in kinds}          # each kind follows each kind
    assert (A.data == 0).any() and (B.data == 0).any()
    return Case(f"special_{n}", A, B, True), order, col


def special_values():
    return [special(40)[0], special(16500)[0]]


def cpu_cases():
    """Every builder's cases (the CPU test walks them all; the GPU tests pick by builder)."""
    return ([reuse_lds()] + [reuse_scratch(n) for n in (16385, 20000)] + [reuse_scratch(16385, SCRATCH_SLOTS + 100)]
            + widths() + row_lengths() + special_values() + [serial_b(30), serial_b(16500)])


_LOOPS = {}


def loops(case):
    """spgemm_loops of a case, computed once per process."""
    if case.name not in _LOOPS:
        _LOOPS[case.name] = spgemm_loops(case.A, case.B)
    return _LOOPS[case.name]


# ---- the scatter-order SpMM (srg_spmm_muladd_f32) ----------------------------------------------------------

def spmm_case(n_rows, d, sorted_rows):
    """(A csr n_rows x 300, X fp32 [300, d]).  Rows in the cycle 200 / 0 / 1 / 2 entries / subnormal sum /
    underflow; unsorted stored order with a repeated column, or (sorted_rows) ascending unique columns."""
    rng = np.random.default_rng(1000 * n_rows + d + (7 if sorted_rows else 0))
    n = 300
    X = (rng.standard_normal((n, d)) * 2).astype(np.float32)
    X[0, :], X[1, :], X[2, :] = 2.0 ** -70, -(2.0 ** -71), 2.0 ** -100
    rows = []
    for r in range(n_rows):
        kind = r % 6
        if kind == 4:
            rows.append([(0, 2.0 ** -75), (1, 2.0 ** -75), (2, 2.0 ** -100)])    # 2^-145 - 2^-146 + 0
            continue
        if kind == 5:
            rows.append([(2, 2.0 ** -100)])                                      # underflows: +0
            continue
        length = (200, 0, 1, 2)[kind]
        cols = rng.choice(np.arange(3, n), size=length, replace=False).tolist()
        if sorted_rows:
            cols.sort()
        elif length >= 2:
            cols[-1] = cols[0]                                                   # a repeated column
        rows.append(row_of(rng, cols))
    return csr(rows, n), X


def spmm_loops(A, X):
    """Y[r, :] = ((0 + v1 X[c1, :]) + v2 X[c2, :]) + ... in stored order, each product rounded to fp32."""
    Y = np.zeros((A.shape[0], X.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for r in range(A.shape[0]):
            s = np.zeros(X.shape[1], np.float32)
            for e in range(A.indptr[r], A.indptr[r + 1]):
                s = (s + (A.data[e] * X[A.indices[e]]).astype(np.float32)).astype(np.float32)
            Y[r] = s
    return Y
