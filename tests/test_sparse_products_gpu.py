"""The sparse-product kernels of srg_spgemm.hip where the other GPU tests do not reach: a workgroup of
k_spgemm that walks a second row on one accumulator (LDS: more than 16384 rows; scratch: fewer slots
than rows, by scratch_limit and by the library's own 2048-slot cap), the geometry of the output scan
(bitmap-word and window edges, the 48 KiB dynamic-LDS switch, the first scratch width), B rows around
the wave's 64 lanes, B rows that repeat a column (SRG_SPGEMM_SERIAL_B) with reuse, values at the edges of
`sum != 0` (subnormal sums, underflow, cancellation, NaN, inf, -0), the C entry srg_spgemm_f32 on raw
pointers, the adjoint's fill loop past 256 lanes on a reused accumulator, and srg_spmm_muladd_f32 on
strided operands.  Every comparison is bitwise against the plain-loop contract of
tests/sparse_product_cases.py (pinned to scipy in tests/test_sparse_products_cpu.py) and, where no row
of B repeats a column, against scipy's product itself; there are no tolerances in this file."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_product_cases as C
import spgemm_grad_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _device_csr(M):
    dev = _dev()
    return (torch.from_numpy(M.indptr.astype(np.int64)).to(dev), torch.from_numpy(M.indices.astype(np.int32)).to(dev),
            torch.from_numpy(M.data.astype(np.float32)).to(dev))


def _count_and_fill_agree(c_ip, c_ix, c_v, m, what):
    """What the count pass promised is what the fill pass wrote: row pointers from 0 to nnz without
    decreasing, columns strictly ascending inside a row, no stored zero."""
    assert c_ip.size == m + 1 and c_ip[0] == 0, what
    assert c_ip[-1] == c_ix.size == c_v.size, what
    assert (np.diff(c_ip) >= 0).all(), what
    if c_ix.size > 1:
        starts = np.zeros(c_ix.size, bool)
        starts[c_ip[:-1][np.diff(c_ip) > 0]] = True
        assert (starts[1:] | (np.diff(c_ix.astype(np.int64)) > 0)).all(), f"{what}: columns not ascending in a row"
    assert not (c_v == 0).any(), f"{what}: a stored zero"


def _spgemm(case, scratch_limit=None):
    from srgnn import sparse as S
    got = S.spgemm(*_device_csr(case.A), *_device_csr(case.B), case.B.shape[1], scratch_limit=scratch_limit)
    got = tuple(t.cpu().numpy() for t in got)
    _count_and_fill_agree(*got, case.A.shape[0], f"{case.name} (scratch_limit={scratch_limit})")
    return got


def _spspmm(case):
    """torch_sparse.spspmm on host COO tensors of the operands in stored order, back as a CSR triple."""
    import torch_sparse
    (m, k), n = case.A.shape, case.B.shape[1]
    ia, va = R.coo(case.A)
    ib, vb = R.coo(case.B)
    idx, val = torch_sparse.spspmm(torch.from_numpy(ia), torch.from_numpy(va), torch.from_numpy(ib),
                                   torch.from_numpy(vb), m, k, n)
    assert idx.device.type == "cpu" and val.dtype == torch.float32
    row = idx[0].numpy()
    assert (np.diff(row) >= 0).all()
    ip = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=m), out=ip[1:])
    got = (ip, idx[1].numpy(), val.numpy())
    _count_and_fill_agree(*got, m, f"{case.name} (spspmm)")
    return got


def _check(case, limits=(None,), shim=False):
    """Runs the case through srgnn.sparse.spgemm under every scratch limit (and through the torch_sparse
    shim), each call twice: every result has the reference's bits."""
    want = C.loops(case)
    runs = [(f"scratch_limit={lim}", lambda lim=lim: _spgemm(case, lim)) for lim in limits]
    if shim:
        runs.append(("spspmm", lambda: _spspmm(case)))
    for how, run in runs:
        first, again = run(), run()
        C.assert_product_bits(first, want, f"{case.name} {how} vs the loops")
        C.assert_product_bits(again, first, f"{case.name} {how}, the second call")
    if case.unique:
        C.assert_product_bits(want, C.spgemm_scipy(case.A, case.B), f"{case.name}: the loops vs scipy")


def _limits(n):
    """Default scratch, and for a scratch width also exactly one accumulator."""
    return (None, C.scratch_per(n)) if n > C.LDS_COLS else (None,)


# ---- accumulator reuse -------------------------------------------------------------------------------------

def test_lds_accumulator_serves_a_second_row():
    """m = 16384 + 700 > the LDS launch's 16384 workgroups: the first 700 walk a wide row and then a row
    that is narrow, empty, all-cancelling or reaches only an empty row of B."""
    case = C.reuse_lds()
    assert case.A.shape[0] > C.LDS_GRID and case.B.shape[1] <= C.LDS_COLS
    _check(case)


@pytest.mark.parametrize("n", [16385, 20000])
def test_scratch_accumulator_serves_many_rows(n):
    """One slot (one workgroup walks all 301 rows), three slots, and the default (a slot per row): the same
    bits, the reference's."""
    case = C.reuse_scratch(n)
    per = C.scratch_per(n)
    assert per == 4 * n + 4 * -(-n // 32)
    _check(case, limits=(per, 3 * per, None))


def test_the_2048_slot_cap_makes_the_reuse():
    """m = 2048 + 100 at the first scratch width with the default scratch: srg_spgemm_scratch_bytes asks
    for 2048 accumulators, so 100 workgroups walk a second row (of the next kind)."""
    from srgnn import _lib
    n, L = 16385, _lib.lib()
    per = C.scratch_per(n)
    need = ctypes.c_int64(-1)
    for m in (0, 1, 2048, 2049):
        assert L.srg_spgemm_scratch_bytes(m, n, ctypes.byref(need)) == _lib.SRG_OK
        assert need.value == min(max(m, 1), 2048) * per
    for width in (0, 1, 16384):
        need.value = -1
        assert L.srg_spgemm_scratch_bytes(3000, width, ctypes.byref(need)) == _lib.SRG_OK
        assert need.value == 0
    case = C.reuse_scratch(n, C.SCRATCH_SLOTS + 100)
    assert case.A.shape[0] == 2148 and case.B.shape[1] == n
    free, _ = torch.cuda.mem_get_info(_dev())
    assert free // 4 >= 2048 * per                      # else the default budget, not the cap, sets the grid
    _check(case)


# ---- widths, row lengths, repeated columns, special values -------------------------------------------------

@pytest.mark.parametrize("n", C.width_ladder())
def test_widths_at_the_scan_and_launch_edges(n):
    _check(C.width(n), limits=_limits(n), shim=True)


@pytest.mark.parametrize("n", [512, 16500])
def test_row_lengths_around_the_wave(n):
    _check(C.row_length(n), limits=_limits(n))


@pytest.mark.parametrize("n", [30, 16500])
def test_b_rows_that_repeat_a_column(n):
    """SRG_SPGEMM_SERIAL_B (one lane walks B's row in stored order), at n = 16500 also with all 90 rows
    on one accumulator; the shim detects the repeats by itself."""
    from srgnn import sparse as S
    case = C.serial_b(n)
    assert not S._rows_have_unique_cols(*_device_csr(case.B)[:2], case.B.shape[0])
    _check(case, limits=_limits(n), shim=True)


@pytest.mark.parametrize("n", [40, 16500])
def test_special_values(n):
    """Kept: a sum that passed through 0, a subnormal sum, NaN, inf.  Dropped: an exact cancellation, an
    underflowed product, +0 + (-0), explicit zeros.  At n = 16500 with one slot every kind follows every
    kind on one accumulator."""
    case, order, col = C.special(n)
    _check(case, limits=_limits(n), shim=True)
    got = _spgemm(case, C.scratch_per(n) if n > C.LDS_COLS else None)
    r = order.index("subnormal")
    v = got[2][got[0][r]:got[0][r + 1]]
    assert v.size == 1 and v.view(np.uint32)[0] == np.float32(2.0 ** -146).view(np.uint32)   # not flushed


# ---- the C entry on raw pointers ---------------------------------------------------------------------------

SENT_I64, SENT_I32, SENT_F32 = -7777, -5555, -1234.5


@pytest.mark.parametrize("n", [512, 16500])
def test_c_entry_on_raw_pointers_and_its_argument_checks(n):
    """srg_spgemm_f32 through ctypes on device pointers (one LDS and one scratch case): phase 0 writes
    cnt[0:m] and nothing else, phase 1 writes exactly C's nnz entries with the Python path's bits, any
    scratch of at least one accumulator gives the same bits, and a bad argument returns SRG_ERR_INVALID
    with a message and writes nothing."""
    from srgnn import _lib
    L = _lib.lib()
    dev = _dev()
    case = C.row_length(n)
    m = case.A.shape[0]
    want = _spgemm(case)
    C.assert_product_bits(want, C.loops(case), case.name)
    nnz = int(want[0][-1])
    a, b = _device_csr(case.A), _device_csr(case.B)
    per = C.scratch_per(n)
    need = ctypes.c_int64(-1)
    assert L.srg_spgemm_scratch_bytes(m, n, ctypes.byref(need)) == _lib.SRG_OK
    assert need.value == (m * per if n > C.LDS_COLS else 0)
    pad, guard = 8, 16
    cnt_buf = torch.full((m + 2 * pad,), SENT_I64, dtype=torch.int64, device=dev)
    ci_buf = torch.full((nnz + 2 * guard,), SENT_I32, dtype=torch.int32, device=dev)
    cv_buf = torch.full((nnz + 2 * guard,), SENT_F32, dtype=torch.float32, device=dev)
    cnt, ci, cv = cnt_buf[pad:pad + m], ci_buf[guard:guard + nnz], cv_buf[guard:guard + nnz]
    c_ip = torch.from_numpy(want[0]).to(dev)

    def call(phase, scratch, scratch_bytes, **over):
        args = dict(a_ptr=a[0].data_ptr(), a_idx=a[1].data_ptr(), a_val=a[2].data_ptr(), m=m, b_ptr=b[0].data_ptr(),
                    b_idx=b[1].data_ptr(), b_val=b[2].data_ptr(), n_cols=n, c_cnt=cnt.data_ptr(),
                    c_ptr=c_ip.data_ptr() if phase else None, c_idx=ci.data_ptr(), c_val=cv.data_ptr())
        args.update(over)
        torch.cuda.synchronize()
        rc = L.srg_spgemm_f32(phase, args["a_ptr"], args["a_idx"], args["a_val"], args["m"], args["b_ptr"],
                              args["b_idx"], args["b_val"], args["n_cols"], args["c_cnt"], args["c_ptr"],
                              args["c_idx"], args["c_val"], scratch, scratch_bytes, 0, None)
        torch.cuda.synchronize()
        return rc

    def untouched(buf, sentinel, lo=0, hi=0):
        """Everything outside buf[lo:hi] still holds the sentinel."""
        x = buf.cpu().numpy()
        return bool((x[:lo] == sentinel).all() and (x[hi:] == sentinel).all())

    def all_sentinel():
        return untouched(cnt_buf, SENT_I64) and untouched(ci_buf, SENT_I32) and untouched(cv_buf, SENT_F32)

    def reset():
        cnt_buf.fill_(SENT_I64)
        ci_buf.fill_(SENT_I32)
        cv_buf.fill_(SENT_F32)

    def scratch_of(nbytes):
        return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)    # the library zeroes what it uses

    sizes = [0] if n <= C.LDS_COLS else [need.value, per, (m + 5) * per + 7]
    for nbytes in sizes:
        scratch = scratch_of(nbytes) if nbytes else None
        sp = scratch.data_ptr() if nbytes else None
        reset()
        assert call(0, sp, nbytes) == _lib.SRG_OK, _lib.last_error()
        assert untouched(cnt_buf, SENT_I64, pad, pad + m), "phase 0 wrote outside cnt[0:m]"
        np.testing.assert_array_equal(cnt.cpu().numpy(), np.diff(want[0]))
        assert untouched(ci_buf, SENT_I32) and untouched(cv_buf, SENT_F32), "phase 0 wrote into C"
        cnt_buf.fill_(SENT_I64)
        assert call(1, sp, nbytes) == _lib.SRG_OK, _lib.last_error()
        assert untouched(ci_buf, SENT_I32, guard, guard + nnz) and untouched(cv_buf, SENT_F32, guard, guard + nnz), \
            "phase 1 wrote outside [0, nnz)"
        assert untouched(cnt_buf, SENT_I64), "phase 1 wrote cnt"
        C.assert_product_bits((want[0], ci.cpu().numpy(), cv.cpu().numpy()), want, f"{case.name}, scratch of {nbytes} B")

    # refusals: SRG_ERR_INVALID, a message, nothing written
    reset()
    scratch = scratch_of(max(need.value, 1))
    sp, nb = (scratch.data_ptr(), need.value) if need.value else (None, 0)
    refused = [("shape", dict(m=-1)), ("shape", dict(n_cols=2 ** 31)), ("null", dict(a_ptr=None))]
    for phase in (0, 1):
        for word, over in refused:
            assert call(phase, sp, nb, **over) == _lib.SRG_ERR_INVALID, (phase, over)
            assert word in _lib.last_error(), (over, _lib.last_error())
    assert call(1, sp, nb, c_ptr=None) == _lib.SRG_ERR_INVALID
    assert "null" in _lib.last_error()
    if n > C.LDS_COLS:
        for small in ((scratch.data_ptr(), per - 1), (None, need.value)):
            for phase in (0, 1):
                assert call(phase, *small) == _lib.SRG_ERR_INVALID, small
                assert "scratch" in _lib.last_error()
    assert all_sentinel(), "a refused call wrote to its outputs"
    assert L.srg_spgemm_f32(0, None, None, None, 0, None, None, None, n, None, None, None, None, None, 0, 0,
                            None) == _lib.SRG_OK
    assert L.srg_spgemm_f32(1, None, None, None, 0, None, None, None, n, None, None, None, None, None, 0, 0,
                            None) == _lib.SRG_OK


# ---- the adjoint: the two holes left -----------------------------------------------------------------------

def _grad_a(A, B, rng):
    """dL/dA through srgnn.sparse.spgemm_grad (P = A, D = G on C's pattern, R = B) and scipy's sampled
    product of the same operands."""
    from srgnn import sparse as S
    (m, _), n = A.shape, B.shape[1]
    crow, ccol, cval = R.forward_pattern(A, B)
    G = R.g_csr(crow, ccol, rng.standard_normal(cval.size).astype(np.float32), (m, n))
    p_ip, p_ix, _ = _device_csr(A)
    got = S.spgemm_grad(p_ip, p_ix, *_device_csr(G), *_device_csr(B), n)
    return got.cpu().numpy(), R.scipy_grads(A, B, G)[0], G


def test_adjoint_fill_loop_past_256_lanes_on_a_reused_accumulator():
    """m = 2100 > the adjoint's 2048 workgroups at an LDS width, every row of D = dL/dC with 257 to 600
    entries: the 256-lane loops that expand D's row into the accumulator and reset it take two or three
    steps, and 52 workgroups do it for a second row."""
    rng = np.random.default_rng(2100)
    m, k, n = 2100, 12, 2000
    B = C.csr([C.row_of(rng, np.sort(rng.choice(n, size=rng.integers(260, 301), replace=False))) for _ in range(k)], n)
    A = C.csr([C.row_of(rng, np.sort(rng.choice(k, size=rng.integers(1, 3), replace=False))) for _ in range(m)], k)
    got, want, G = _grad_a(A, B, rng)
    lens = np.diff(G.indptr)
    assert m > C.SCRATCH_SLOTS and n <= C.LDS_COLS and lens.min() >= 257 and 512 < lens.max() <= 600
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_adjoint_scratch_grid_set_by_the_2048_cap():
    """m = 2100 at the first scratch width with a scratch of more than m accumulators: the library's cap
    of 2048 workgroups, not the scratch, sets the grid."""
    from srgnn import _lib
    rng = np.random.default_rng(2101)
    m, k, n = 2100, 30, 16385
    need = ctypes.c_int64(-1)
    assert _lib.lib().srg_spgemm_scratch_bytes(m, n, ctypes.byref(need)) == _lib.SRG_OK
    free, _ = torch.cuda.mem_get_info(_dev())
    assert min(need.value, free // 4) // (4 * n) >= m           # the slots spgemm_grad's default scratch holds
    B = C.csr([C.row_of(rng, np.sort(rng.choice(n, size=rng.integers(0, 40), replace=False))) for _ in range(k)], n)
    A = C.csr([C.row_of(rng, np.sort(rng.choice(k, size=rng.integers(0, 4), replace=False))) for _ in range(m)], k)
    got, want, _ = _grad_a(A, B, rng)
    assert got.size == A.nnz > m
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- srg_spmm_muladd_f32 on strided operands ---------------------------------------------------------------

@pytest.mark.parametrize("sorted_rows", [False, True], ids=["stored_order", "sorted"])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 701])
def test_spmm_muladd_on_column_windows(n_rows, d, sorted_rows):
    """X is a column window of a wider panel (ldx = d + 5), out a window of a sentinel-filled panel
    (ldy = d + 3, two more rows below): the window has the loop reference's bits (scipy's on sorted
    rows), the sentinel columns and the rows past n_rows stay as they were."""
    from srgnn import sparse as S
    dev = _dev()
    A, X = C.spmm_case(n_rows, d, sorted_rows)
    want = C.spmm_loops(A, X)
    if sorted_rows:
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(want.view(np.uint32), np.asarray(A @ X, dtype=np.float32).view(np.uint32))
    x_panel = torch.from_numpy(np.random.default_rng(d).standard_normal((X.shape[0], d + 5)).astype(np.float32)).to(dev)
    x_panel[:, 2:2 + d] = torch.from_numpy(X).to(dev)
    out_panel = torch.full((n_rows + 2, d + 3), SENT_F32, dtype=torch.float32, device=dev)
    xw, ow = x_panel[:, 2:2 + d], out_panel[:n_rows, 1:1 + d]
    assert xw.stride(0) == d + 5 and ow.stride(0) == d + 3 and xw.stride(1) == 1 and ow.stride(1) == 1
    for _ in range(2):
        ret = S.spmm_scatter(*_device_csr(A), xw, out=ow)
        assert ret.data_ptr() == ow.data_ptr()
        got = out_panel.cpu().numpy()
        np.testing.assert_array_equal(got[:n_rows, 1:1 + d].view(np.uint32), want.view(np.uint32))
        assert (got[:, 0] == SENT_F32).all() and (got[:, 1 + d:] == SENT_F32).all() and (got[n_rows:] == SENT_F32).all()
    if n_rows >= 5:
        assert (got[4, 1:1 + d] == np.float32(2.0 ** -146)).all()      # the subnormal sum is kept, not flushed
    if n_rows >= 6:
        assert not got[5, 1:1 + d].any() and not np.signbit(got[5, 1:1 + d]).any()
