"""The device-built wavelet basis: srg_dense_sparsify_f64 (threshold + compact), srg_csr_append_rows_f32
(the hstack), srg_csr_row_normalize_l1_f32 (sklearn's L1) and srgnn.wavelet.wavelet_basis_device /
spectral_features_device over them, against the numpy restatement (tests/wavelet_sparsify_ref.py, pinned to
the reference's lines in tests/test_wavelet_sparsify_cpu.py), scipy / sklearn themselves, the golden wav_*
bases and the host-assembled wavelet_basis.  Every comparison is bitwise."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import wavelet_sparsify_ref as WS

pytestmark = pytest.mark.gpu

GUARD = 64                     # untouched words expected behind every output array
WIDTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000]
ROWS = [0, 1, 5, 257]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _window(block, ldr, offset):
    """`block` [n, w] as a column window of a device panel with row stride ldr whose base is `offset`
    doubles past a 16-byte boundary; the rest of the panel holds 7.0 (a survivor, were it read)."""
    n, w = block.shape
    buf = torch.full((offset + n * ldr + 2,), 7.0, dtype=torch.float64, device="cuda")
    panel = buf[offset:offset + n * ldr].view(n, ldr)
    panel[:, :w] = torch.from_numpy(block).cuda()
    R = panel[:, :w]
    assert n == 0 or R.data_ptr() % 16 == (8 * offset) % 16
    return R


def _sparsify(R, tol, col0):
    """Both phases through the C entry, the outputs with guard words behind them."""
    from srgnn import _lib
    n, w = R.shape
    dev, st = R.device, _lib.stream(R.device)
    cnt = torch.full((n + GUARD,), -5, dtype=torch.int64, device=dev)
    _lib.call(dev, "srg_dense_sparsify_f64", 0, R.data_ptr(), R.stride(0) if n else w, n, w, tol, col0,
              cnt.data_ptr(), None, None, None, st)
    assert bool((cnt[n:] == -5).all())
    cnt = cnt[:n]
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=ptr[1:])
    nnz = int(ptr[-1])
    idx = torch.full((nnz + GUARD,), -7, dtype=torch.int32, device=dev)
    val = torch.full((nnz + GUARD,), -7.0, dtype=torch.float32, device=dev)
    _lib.call(dev, "srg_dense_sparsify_f64", 1, R.data_ptr(), R.stride(0) if n else w, n, w, tol, col0,
              None, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), st)
    assert bool((idx[nnz:] == -7).all()) and bool((val[nnz:] == -7.0).all())
    return cnt.cpu().numpy(), idx[:nnz].cpu().numpy(), val[:nnz].cpu().numpy()


@pytest.mark.parametrize("w", WIDTHS)
def test_sparsify_entry_equals_restatement(w):
    """Every width x row count x row stride (the block itself, a window of a panel 3 columns wider) x base
    alignment (16 bytes, 8 bytes) x col0 x tolerance, with NaN, +-Inf, -0, 1e-50 and 1e-40 planted, a row
    without survivors, a row where every column survives and a row whose last column alone survives.
    w + 3 is odd for even w, so both strides reach both load paths; the two paths give the same bits."""
    for n in ROWS:
        block = WS.planted_block(n, w, seed=1000 * n + w)
        for tol in WS.TOLERANCES:
            for col0 in (0, 1000):
                want_cnt, _, want_idx, want_val = WS.sparsify_block(block, tol, col0)
                got = {}
                for ldr in (w, w + 3):
                    for offset in (0, 1):
                        cnt, idx, val = _sparsify(_window(block, ldr, offset), tol, col0)
                        where = f"n={n} w={w} ldr={ldr} offset={offset} tol={tol} col0={col0}"
                        np.testing.assert_array_equal(cnt, want_cnt, err_msg=where)
                        np.testing.assert_array_equal(idx, want_idx, err_msg=where)
                        np.testing.assert_array_equal(_u32(val), _u32(want_val), err_msg=where)
                        got[ldr, offset] = (idx, _u32(val))
                for k in got:
                    assert np.array_equal(got[k][0], got[w, 0][0]) and np.array_equal(got[k][1], got[w, 0][1])
        if n >= 5:                                 # the structured rows are what they claim to be
            cnt = WS.sparsify_block(block, 1e-4, 0)[0]
            assert cnt[0] == 0 and cnt[1] == w and cnt[2] == 1


def test_sparsify_invalid_arguments_write_nothing():
    from srgnn import _lib
    R = torch.ones((4, 8), dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), -5, dtype=torch.int64, device="cuda")
    ptr = torch.arange(0, 40, 8, dtype=torch.int64, device="cuda")
    idx = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    val = torch.full((32,), -7.0, dtype=torch.float32, device="cuda")
    st = _lib.stream(R.device)
    for phase, ldr, w, col0, word in ((0, 7, 8, 0, "ldr"), (1, 7, 8, 0, "ldr"), (0, 8, 8, 2 ** 31 - 8, "int32"),
                                      (1, 8, 8, 2 ** 31 - 8, "int32"), (2, 8, 8, 0, "phase"), (0, 8, 8, -1, "col0")):
        with pytest.raises(_lib.SrgError, match=word):
            _lib.call(R.device, "srg_dense_sparsify_f64", phase, R.data_ptr(), ldr, 4, w, 1e-4, col0, cnt.data_ptr(),
                      ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), st)
        assert _lib.lib().srg_last_error_code() == _lib.SRG_ERR_INVALID and word in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((cnt == -5).all()) and bool((idx == -7).all()) and bool((val == -7.0).all())
    # the largest column id that fits is accepted
    _lib.call(R.device, "srg_dense_sparsify_f64", 0, R.data_ptr(), 8, 4, 8, 1e-4, 2 ** 31 - 9, cnt.data_ptr(), None,
              None, None, st)
    assert cnt.tolist() == [8, 8, 8, 8]
    _lib.lib().srg_clear_error()


def _random_rows(rng, counts, n_cols):
    """A CSR with counts[r] entries in row r, column ids ascending."""
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, k, replace=False)) for k in counts] + [np.zeros(0, np.int64)])
    data = (rng.random(indices.size) * 3 - 1).astype(np.float32)
    return sp.csr_matrix((data, indices.astype(np.int32), indptr), shape=(len(counts), n_cols))


def test_append_rows_is_the_hstack():
    """Three block-local CSRs over 9 rows appended in order: row 0 empty in every block, row 4 empty in the
    middle block only, row 6 with 200 entries in the last block alone (a whole-wave row; the others are
    packed four to a wave) == sp.hstack(blocks).tocsr(); afterwards the cursor stands at indptr[1:]."""
    from srgnn import _lib
    rng = np.random.default_rng(5)
    counts = [[0, 3, 1, 17, 2, 64, 0, 5, 1], [0, 1, 65, 2, 0, 4, 0, 16, 0], [0, 2, 0, 33, 7, 1, 200, 0, 1]]
    blocks = [_random_rows(rng, c, 300) for c in counts]
    want = sp.hstack(blocks).tocsr()
    n = 9
    indptr = torch.from_numpy(want.indptr.astype(np.int64)).cuda()
    cursor = indptr[:-1].clone()
    indices = torch.full((want.nnz + GUARD,), -7, dtype=torch.int32, device="cuda")
    values = torch.full((want.nnz + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    for b, m in enumerate(blocks):
        ptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
        idx = torch.from_numpy((m.indices + 300 * b).astype(np.int32)).cuda()
        val = torch.from_numpy(m.data).cuda()
        _lib.call("cuda", "srg_csr_append_rows_f32", ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), n,
                  cursor.data_ptr(), indices.data_ptr(), values.data_ptr(), _lib.stream(torch.device("cuda")))
    np.testing.assert_array_equal(indices[:want.nnz].cpu().numpy(), want.indices)
    np.testing.assert_array_equal(_u32(values[:want.nnz].cpu().numpy()), _u32(want.data))
    assert torch.equal(cursor, indptr[1:])
    assert bool((indices[want.nnz:] == -7).all()) and bool((values[want.nnz:] == -7.0).all())


def test_row_normalize_l1_equals_sklearn():
    """The 400 x 300 matrix of test_wavelet_cpu.py's L1 test (mixed signs, fp32) plus a row of explicit
    zeros (left as it is), an empty row and a row of 5,000 entries (the whole-wave path)."""
    from sklearn.preprocessing import normalize
    from srgnn import _lib
    rng = np.random.default_rng(3)
    M = sp.random(400, 300, density=0.2, format="csr", dtype=np.float32, random_state=4)
    M.data = (rng.random(M.nnz).astype(np.float32) * 3 - 1).astype(np.float32)
    extra = [(np.arange(10), np.zeros(10, np.float32)), (np.arange(0), np.zeros(0, np.float32)),
             (np.arange(5000), (rng.random(5000) * 3 - 1).astype(np.float32))]
    indptr = np.concatenate([M.indptr, M.indptr[-1] + np.cumsum([c.size for c, _ in extra])]).astype(np.int64)
    indices = np.concatenate([M.indices] + [c for c, _ in extra]).astype(np.int32)
    data = np.concatenate([M.data] + [v for _, v in extra]).astype(np.float32)
    full = sp.csr_matrix((data, indices, indptr), shape=(403, 5000))
    want = normalize(full, norm="l1", axis=1)
    assert want.nnz == full.nnz and np.array_equal(want.indptr, indptr)
    ip = torch.from_numpy(indptr).cuda()
    v = torch.cat([torch.from_numpy(data).cuda(), torch.full((GUARD,), -7.0, device="cuda")])
    _lib.call("cuda", "srg_csr_row_normalize_l1_f32", ip.data_ptr(), v.data_ptr(), 403, _lib.stream(torch.device("cuda")))
    got = v[:data.size].cpu().numpy()
    np.testing.assert_array_equal(_u32(got), _u32(want.data))
    assert not got[indptr[400]:indptr[401]].any() and bool((v[data.size:] == -7.0).all())
    np.testing.assert_array_equal(_u32(got), _u32(WS.l1_normalize(indptr, data)))


def test_row_normalize_l1_nan_sum_makes_the_row_nan():
    from srgnn import _lib
    indptr = np.array([0, 3, 5, 5 + 70], dtype=np.int64)
    data = np.r_[[1.0, np.nan, -2.0], [0.5, -0.5], np.r_[np.ones(69), np.inf]].astype(np.float32)
    v = torch.from_numpy(data).cuda()
    _lib.call("cuda", "srg_csr_row_normalize_l1_f32", torch.from_numpy(indptr).cuda().data_ptr(), v.data_ptr(), 3,
              _lib.stream(torch.device("cuda")))
    np.testing.assert_array_equal(_u32(v.cpu().numpy()), _u32(WS.l1_normalize(indptr, data)))
    assert np.isnan(v[:3].cpu().numpy()).all()


def _golden(name):
    import golden_cases as G
    z = np.load(f"{G.GOLDEN}/{name}.npz", allow_pickle=False)
    n = z["adj_indptr"].size - 1
    return z, sp.csr_matrix((z["adj_data"], z["adj_indices"], z["adj_indptr"]), shape=(n, n))


def _same_csr(got, want):
    got, want = sp.csr_matrix(got), sp.csr_matrix(want)
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(_u32(got.data), _u32(want.data))


@pytest.mark.parametrize("batch", [1000, 37])
@pytest.mark.parametrize("name", ["wav_rand", "wav_cora"])
def test_device_basis_equals_reference_spectral_model(name, batch):
    from srgnn.wavelet import wavelet_basis_device
    z, adj = _golden(name)
    phi, phi_inv, lmax = wavelet_basis_device(adj, float(z["scale"]), int(z["order"]), float(z["tolerance"]),
                                              lmax=float(z["lmax"]), batch=batch, device="cuda")
    assert lmax == float(z["lmax"])
    for s, m in enumerate((phi, phi_inv)):
        got = m.to_scipy()
        np.testing.assert_array_equal(got.indptr, z[f"phi{s}_indptr"])
        np.testing.assert_array_equal(got.indices, z[f"phi{s}_indices"])
        np.testing.assert_array_equal(_u32(got.data), _u32(z[f"phi{s}_data"]))


def _graphs():
    """graphs() of tests/test_wavelet_gpu.py: the 60-node graph and the 3,000-node RMAT graph."""
    from srgnn import synth
    rng = np.random.default_rng(0)
    m = np.triu(rng.random((60, 60)) < 0.1, 1)
    a = sp.csr_matrix((m + m.T).astype(float))
    n = 3000
    u, v = synth.rmat_undirected_t(n, 15000, seed=8)
    ip, ix = synth.symmetric_csr_t(n, u, v)
    b = sp.csr_matrix((np.ones(ix.numel()), ix.numpy(), ip.numpy()), shape=(n, n))
    return {"small": a, "rmat3000": b}


def test_device_basis_equals_host_assembled_small():
    from srgnn.wavelet import wavelet_basis, wavelet_basis_device
    a = _graphs()["small"]
    want = wavelet_basis(a, scale=0.5, order=3, tolerance=1e-4, batch=25, device="cuda")
    got = wavelet_basis_device(a, scale=0.5, order=3, tolerance=1e-4, batch=25, device="cuda")
    assert got[2] == want[2]
    _same_csr(got[0].to_scipy(), want[0])
    _same_csr(got[1].to_scipy(), want[1])


@pytest.fixture(scope="module")
def rmat_features():
    """spectral_features and spectral_features_device once, on the RMAT graph with d = 24 and batch 700."""
    from srgnn.wavelet import spectral_features, spectral_features_device
    a = _graphs()["rmat3000"]
    X = np.random.default_rng(5).random((a.shape[0], 24)).astype(np.float32)
    kw = dict(scale=0.5, order=3, tolerance=1e-4, batch=700, device="cuda")
    return spectral_features(a, X, **kw), spectral_features_device(a, X, **kw)


def test_device_basis_equals_host_assembled_rmat(rmat_features):
    (_, phi, phi_inv, lmax), (_, dphi, dphi_inv, dlmax) = rmat_features
    assert lmax == dlmax
    _same_csr(dphi.to_scipy(), phi)
    _same_csr(dphi_inv.to_scipy(), phi_inv)


def test_spectral_features_device_equals_host_path(rmat_features):
    (out, *_), (dout, *_) = rmat_features
    assert dout.is_cuda and dout.dtype == torch.float32 and dout.shape == (3000, 48)
    assert torch.equal(dout.cpu(), out)


def test_return_types_and_run_to_run_identity():
    from srgnn.wavelet import DeviceBasis, wavelet_basis_device
    a = _graphs()["small"]
    runs = [wavelet_basis_device(a, batch=25, device="cuda") for _ in range(2)]
    for m in runs[0][:2]:
        assert isinstance(m, DeviceBasis) and m.n == 60
        assert m.indptr.is_cuda and m.indices.is_cuda and m.values.is_cuda
        assert m.indptr.dtype == torch.int64 and m.indptr.shape == (61,)
        assert m.indices.dtype == torch.int32 and m.values.dtype == torch.float32
        assert m.indices.numel() == m.values.numel() == int(m.indptr[-1])
    assert isinstance(runs[0][2], float)
    for m0, m1 in zip(runs[0][:2], runs[1][:2]):
        assert torch.equal(m0.indptr, m1.indptr) and torch.equal(m0.indices, m1.indices)
        assert torch.equal(m0.values.view(torch.int32), m1.values.view(torch.int32))
