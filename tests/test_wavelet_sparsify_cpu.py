"""The yardstick of the device-built wavelet basis (tests/wavelet_sparsify_ref.py), checked without a
device: it equals the golden wav_* bases (the reference's own SpectralModel.preprocess) when fed the
oracle's cheby_op on identity blocks of any batch size, and it equals the reference's own lines
(sub[sub < tol] = 0, csr_matrix(astype(float32)), hstack, sklearn's L1 normalisation) on blocks with the
special values planted.  The kernels are checked against it in tests/test_wavelet_sparsify_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import wavelet_sparsify_ref as WS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wavelet_golden(name):
    import golden_cases as G
    z = np.load(f"{G.GOLDEN}/{name}.npz", allow_pickle=False)
    n = z["adj_indptr"].size - 1
    adj = sp.csr_matrix((z["adj_data"], z["adj_indices"], z["adj_indptr"]), shape=(n, n))
    return z, adj, n


@pytest.mark.parametrize("batch", [1000, 37])
@pytest.mark.parametrize("name", ["wav_rand", "wav_cora"])
def test_restatement_equals_golden_bases(oracle_mod, name, batch):
    """Cora at batch 1000: two full blocks and a ragged one of 708 columns; batch 37: the result does not
    depend on the batch size."""
    z, adj, n = _wavelet_golden(name)
    lmax, scale, order, tol = float(z["lmax"]), float(z["scale"]), int(z["order"]), float(z["tolerance"])
    L = oracle_mod.laplacian(adj.indptr, adj.indices, adj.data, n)
    coeffs = np.stack([oracle_mod.cheby_coeffs(t, lmax, order) for t in (-scale, scale)])
    dense = [[], []]
    for c0 in range(0, n, batch):
        w = min(batch, n - c0)
        S = np.zeros((n, w))
        S[np.arange(c0, c0 + w), np.arange(w)] = 1
        R = oracle_mod.cheby_op(L, coeffs, S, lmax)
        for s in range(2):
            dense[s].append((c0, R[s]))
    for s in range(2):
        indptr, idx, val = WS.basis(dense[s], tol, n)
        np.testing.assert_array_equal(indptr, z[f"phi{s}_indptr"])
        np.testing.assert_array_equal(idx, z[f"phi{s}_indices"])
        np.testing.assert_array_equal(val.view(np.uint32), z[f"phi{s}_data"].view(np.uint32))


def _reference_lines(dense_blocks, tol, l1):
    """base_model.py:251-257, 287-290 on dense blocks; l1: the in-place L1 routine applied to the hstack."""
    blocks = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for _, R in dense_blocks:
            sub = R.copy()
            sub[sub < tol] = 0
            blocks.append(sp.csr_matrix(sub.astype(np.float32)))
    phi = sp.hstack(blocks).tocsr()
    return l1(phi)


def _sklearn_normalize(phi):
    from sklearn.preprocessing import normalize
    return normalize(phi, norm="l1", axis=1)


def _sklearn_inner(phi):
    """What sklearn.preprocessing.normalize(norm='l1') runs on a CSR matrix after its input check, which
    refuses NaN and Inf: the only way to put non-finite values through sklearn's own arithmetic."""
    from sklearn.utils.sparsefuncs_fast import inplace_csr_row_normalize_l1
    phi = sp.csr_matrix(phi, copy=True)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        inplace_csr_row_normalize_l1(phi)
    return phi


FINITE = tuple(v for v in WS.SPECIALS if np.isfinite(v))


@pytest.mark.parametrize("specials,l1", [(FINITE, _sklearn_normalize), (WS.SPECIALS, _sklearn_inner)],
                         ids=["finite-normalize", "nonfinite-inner"])
@pytest.mark.parametrize("tol", WS.TOLERANCES, ids=[str(t) for t in WS.TOLERANCES])
def test_restatement_equals_reference_lines(tol, specials, l1):
    """7 x 10 random values with NaN, +-Inf, -0.0, 1e-50, 1e-40 and an all-zero row planted, in blocks of
    4 + 4 + 2 columns.  sklearn.preprocessing.normalize itself takes the block without NaN / Inf (its
    input check raises on them); the full set goes through the routine normalize calls."""
    n, w = 7, 10
    R = WS.planted_block(n, w, seed=11, specials=specials)
    planted = R[3:]                                # rows 0..2 are the structured ones
    for v in specials:
        hit = np.isnan(planted) if np.isnan(v) else (planted == v) & (np.signbit(planted) == np.signbit(v))
        assert hit.any(), f"{v} not planted"
    dense = [(0, R[:, 0:4]), (4, R[:, 4:8]), (8, R[:, 8:10])]
    want = _reference_lines(dense, tol, l1)
    indptr, idx, val = WS.basis(dense, tol, n)
    np.testing.assert_array_equal(indptr, want.indptr)
    np.testing.assert_array_equal(idx, want.indices)
    np.testing.assert_array_equal(val.view(np.uint32), want.data.astype(np.float32).view(np.uint32))
    assert want.dtype == np.float32


def test_planted_block_has_the_structured_rows():
    R = WS.planted_block(5, 65, seed=3)
    for tol in (1e-4, 0.0, -1.0):
        cnt = WS.sparsify_block(R, tol, 0)[0]
        assert cnt[0] == 0 and cnt[1] == 65 and cnt[2] == 1
    assert WS.sparsify_block(R, 1e-4, 1000)[2][WS.sparsify_block(R, 1e-4, 1000)[1][2]] == 1064


def test_entries_are_declared_exported_and_bound():
    from srgnn import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "srgnn_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, nargs in {"srg_dense_sparsify_f64": 12, "srg_csr_append_rows_f32": 8,
                        "srg_csr_row_normalize_l1_f32": 4}.items():
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), f"include/srgnn_hip.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        fn = getattr(_lib.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int


def test_invalid_arguments_fail_before_any_launch():
    """The argument checks need no device: a bad phase, ldr < w, a negative col0 and column ids past int32
    return SRG_ERR_INVALID with srg_last_error set; empty problems are no-ops."""
    from srgnn import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    for args, word in (((2, p, 8, 4, 8, 1e-4, 0), "phase"), ((0, p, 7, 4, 8, 1e-4, 0), "ldr"),
                       ((0, p, 8, 4, 8, 1e-4, -1), "col0"), ((1, p, 8, 4, 8, 1e-4, 2 ** 31 - 8), "int32")):
        assert L.srg_dense_sparsify_f64(*args, p, p, p, p, None) == _lib.SRG_ERR_INVALID
        assert L.srg_last_error_code() == _lib.SRG_ERR_INVALID and word in _lib.last_error()
    assert L.srg_dense_sparsify_f64(0, None, 8, 0, 8, 1e-4, 0, None, None, None, None, None) == _lib.SRG_OK
    assert L.srg_dense_sparsify_f64(1, None, 8, 4, 0, 1e-4, 0, None, None, None, None, None) == _lib.SRG_OK
    assert L.srg_csr_append_rows_f32(None, None, None, 0, None, None, None, None) == _lib.SRG_OK
    assert L.srg_csr_row_normalize_l1_f32(None, None, 0, None) == _lib.SRG_OK
    assert L.srg_csr_append_rows_f32(None, None, None, -1, None, None, None, None) == _lib.SRG_ERR_INVALID
    assert L.srg_csr_row_normalize_l1_f32(None, None, -1, None) == _lib.SRG_ERR_INVALID
    L.srg_clear_error()
