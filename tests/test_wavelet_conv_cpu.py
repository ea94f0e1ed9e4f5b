"""The fused graph-wavelet filter without a device: the host restatement (tests/wavelet_conv_ref.py) that
pins the kernels bit for bit is itself (a) bit for bit the composition of the existing restatements and
scipy in the re-associated order, (b) within the derived rounding bound of the fp64
value and (c) of the reference's association on the committed wavelet fixtures; its corner cases are
stated once; and the two C entries are declared, exported, bound, and reject every invalid argument
before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_grad_ref as R
import wavelet_conv_ref as W
from sddmm_ref import assert_bits, csr_rows, sddmm_ref
from sparse_product_cases import spmm_loops
from srgnn import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srgnn_hip.h")


def _basis(rng, n, density):
    """A coalesced random basis: column-sorted rows, unique (row, column), values in [0.5, 1.5)."""
    M = sp.random(n, n, density=density, format="csr", random_state=rng, dtype=np.float32)
    M.data = (rng.random(M.nnz) + 0.5).astype(np.float32) * rng.choice([-1, 1], M.nnz).astype(np.float32)
    M.sort_indices()
    return M


def _triple(M):
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float32)


def _case(n, density, d, seed):
    rng = np.random.default_rng(seed)
    phi, phi_inv = _basis(rng, n, density), _basis(rng, n, density)
    theta = rng.uniform(0.9, 1.1, n).astype(np.float32)
    Z = rng.standard_normal((n, d)).astype(np.float32)
    G = rng.standard_normal((n, d)).astype(np.float32)
    return phi, phi_inv, theta, Z, G


def _diag(theta):
    n = theta.size
    return sp.csr_matrix((theta, np.arange(n, dtype=np.int32), np.arange(n + 1)), shape=(n, n))


# ---- (a) lineage ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,density,d", [(120, 0.1, 16), (90, 0.2, 7), (64, 0.3, 1)])
def test_restatement_is_the_composition_of_the_existing_restatements_reassociated(n, density, d):
    """spmm(*spspmm(phi, diag theta), n, n, spmm(phi^-1, n, n, Z)) and its autograd from the pieces that
    pin the shims: scipy's fp32 product for spspmm (spgemm_grad_ref.forward_pattern), the scatter
    contract (sparse_product_cases.spmm_loops) for spmm and its matrix gradient, sddmm_ref for spmm's
    value gradient and scipy's sampled product (spgemm_grad_ref.scipy_grads) for spspmm's B side."""
    phi, phi_inv, theta, Z, G = _case(n, density, d, 7 * n + d)
    Y, P = W.forward_ref(_triple(phi), _triple(phi_inv), theta, Z)
    gP, gZ, gtheta = W.backward_ref(_triple(phi), _triple(phi_inv), theta, P, G)
    D = _diag(theta)
    r1, c1, w1 = R.forward_pattern(phi, D)
    assert w1.size == phi.nnz                               # no rescaled value is an exact zero
    C1 = R.g_csr(r1, c1, w1, (n, n))
    P2 = spmm_loops(phi_inv, Z)
    assert_bits(P, P2, "P")
    assert_bits(Y, spmm_loops(C1, P2), "Y")
    C1t, _ = R.transpose_stable(C1)
    gP2 = spmm_loops(C1t, G)
    assert_bits(gP, gP2, "gP")
    assert_bits(gZ, spmm_loops(R.transpose_stable(phi_inv)[0], gP2), "gZ")
    g_val = sddmm_ref(r1, c1, G, P2)
    _, g_diag = R.scipy_grads(phi, D, R.g_csr(r1, c1, g_val, (n, n)))
    assert_bits(gtheta, g_diag, "gtheta")


# ---- (b), (c) the bounds -----------------------------------------------------------------------------------

def _magnitudes(phi, phi_inv, theta, Z, G):
    """(exact Y, S, exact gZ, Sz, exact gtheta, St) in fp64 from the dense operands."""
    n = theta.size
    A, B = W.dense64(phi, n), W.dense64(phi_inv, n)
    T, Z, G = theta.astype(np.float64), Z.astype(np.float64), G.astype(np.float64)
    P, aP = B @ Z, np.abs(B) @ np.abs(Z)
    Y, S = (A * T) @ P, (np.abs(A) * np.abs(T)) @ aP
    gZ, Sz = B.T @ ((A * T).T @ G), np.abs(B).T @ ((np.abs(A) * np.abs(T)).T @ np.abs(G))
    gt, St = (A * (G @ P.T)).sum(axis=0), (np.abs(A) * (np.abs(G) @ aP.T)).sum(axis=0)
    return Y, S, gZ, Sz, gt, St


def _ratio(got, exact, bound):
    diff = np.abs(got.astype(np.float64) - exact)
    return float(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0)).max())


def _col_longest(triple, n):
    return int(np.bincount(triple[1], minlength=n).max())


@pytest.mark.parametrize("n,density,d", [(200, 0.1, 16), (150, 0.3, 7), (300, 0.05, 33)])
def test_restatement_is_within_the_derived_bound_of_the_fp64_value(n, density, d):
    """With La, Lb the longest rows of phi and phi^-1 and Ma, Mb their longest columns, every term of
      Y      carries at most La + Lb + 1 factors (1 + delta): Lb in P's chain (its product and Lb - 1
             inexact additions; the addition to +0 is exact), the rescale, the product, La - 1 additions;
      gZ     Ma + Mb + 1: the rescale, gP's product and Ma - 1 additions, gZ's product and Mb - 1;
      gtheta Ma + Lb + d: P's Lb, the column chain's d, the product by phi, Ma - 1 additions;
    so |computed - exact| <= gamma_m * sum |terms|.  Inputs of order 1 do not underflow; the fp64
    value's own error is about 2^-29 of the bound."""
    phi, phi_inv, theta, Z, G = _case(n, density, d, n + d)
    p, q = _triple(phi), _triple(phi_inv)
    Y, P = W.forward_ref(p, q, theta, Z)
    _, gZ, gt = W.backward_ref(p, q, theta, P, G)
    eY, S, eZ, Sz, et, St = _magnitudes(p, q, theta, Z, G)
    La, Lb, Ma, Mb = W.longest_row(p[0]), W.longest_row(q[0]), _col_longest(p, n), _col_longest(q, n)
    for what, r in (("Y", _ratio(Y, eY, W.gamma(La + Lb + 1) * S)), ("gZ", _ratio(gZ, eZ, W.gamma(Ma + Mb + 1) * Sz)),
                    ("gtheta", _ratio(gt, et, W.gamma(Ma + Lb + d) * St))):
        print(f"n={n} d={d} {what}: max |chain - exact| / bound = {r:.4f}")
        assert r <= 1.0, what


@pytest.mark.parametrize("name", ["wav_rand", "wav_cora"])
def test_restatement_is_within_the_derived_bound_of_the_reference_association(name):
    """The reference computes spmm(spspmm(spspmm(phi, diag theta), phi^-1), Z): scipy's fp32 products of the
    fixture's bases (the arithmetic the shims are pinned to).  Its terms carry at most La + Lc + 1 factors
    (the rescale; the second product's multiply and La - 1 additions; spmm's multiply and Lc - 1
    additions, Lc the longest row of the product), so
      |restatement - reference| <= (gamma_{La+Lb+1} + gamma_{La+Lc+1}) * S."""
    z = np.load(os.path.join(REPO, "tests", "golden", f"{name}.npz"), allow_pickle=False)
    p, q = [(z[f"phi{i}_indptr"].astype(np.int64), z[f"phi{i}_indices"].astype(np.int32),
             z[f"phi{i}_data"].astype(np.float32)) for i in (0, 1)]
    n, d = p[0].size - 1, 16
    rng = np.random.default_rng(n)
    theta = rng.uniform(0.9, 1.1, n).astype(np.float32)
    Z = rng.standard_normal((n, d)).astype(np.float32)
    Y, _ = W.forward_ref(p, q, theta, Z)
    phi, phi_inv = (sp.csr_matrix((t[2], t[1], t[0]), shape=(n, n)) for t in (p, q))
    C1 = R.g_csr(*R.forward_pattern(phi, _diag(theta)), (n, n))
    C2 = R.g_csr(*R.forward_pattern(C1, phi_inv), (n, n))
    ref = np.asarray(C2 @ Z, dtype=np.float32)
    _, S, *_ = _magnitudes(p, q, theta, Z, Z)
    La, Lb, Lc = W.longest_row(p[0]), W.longest_row(q[0]), W.longest_row(C2.indptr)
    r = _ratio(Y, ref.astype(np.float64), (W.gamma(La + Lb + 1) + W.gamma(La + Lc + 1)) * S)
    print(f"{name}: n={n} La={La} Lb={Lb} Lc={Lc} nnz(product)={C2.nnz}: max |fused - reference| / bound = {r:.4f}")
    assert r <= 1.0


# ---- corner cases, stated once -----------------------------------------------------------------------------

def test_corner_cases():
    f32 = np.float32
    # 4 x 4: row 1 of phi is empty; row 2 holds column 3 twice (duplicates, unsorted: 3, 0, 3)
    phi = (np.array([0, 2, 2, 5, 6], np.int64), np.array([0, 1, 3, 0, 3, 2], np.int32),
           np.array([1.0, 2.0, 0.5, -1.0, 0.25, 2.0 ** -100], f32))
    phi_inv = (np.array([0, 1, 2, 3, 4], np.int64), np.array([0, 1, 2, 3], np.int32), np.array([1.0, 1.0, 1.0, 1.0], f32))
    theta = np.array([-1.5, 0.0, 2.0 ** -40, 3.0], f32)      # a negative, a zero, one that makes a subnormal
    Z = np.array([[1.0, 2.0], [3.0, 4.0], [1.0, 1.0], [5.0, -6.0]], f32)
    Y, P = W.forward_ref(phi, phi_inv, theta, Z)
    assert_bits(P, Z)
    assert_bits(Y[0], np.array([-1.5, -3.0], f32))          # 1 * -1.5 * Z[0] + 2 * 0 * Z[1]
    assert not Y[1].any() and not np.signbit(Y[1]).any()    # the empty row: +0
    # duplicates each taken, in stored order: ((0 + 1.5 * 5) + 1.5 * 1) + 0.75 * 5, second column likewise
    assert_bits(Y[2], np.array([f32(f32(7.5 + 1.5) + 3.75), f32(f32(-9.0 + 3.0) - 4.5)], f32))
    assert Y[3, 0] == f32(2.0 ** -140) and Y[3, 0] != 0     # fl(2^-100 * 2^-40) is subnormal and kept
    G = np.ones((4, 2), f32)
    gP, gZ, gt = W.backward_ref(phi, phi_inv, theta, P, G)
    # theta[1] = 0: the composition's spspmm drops the entry and loses this gradient; the formula keeps it
    assert gt[1] == f32(2.0 * (3.0 + 4.0))
    assert gt[0] == f32(f32(1.0 * 3.0) + f32(-1.0 * 3.0)) and gt[3] == f32(f32(0.5 * -1.0) + f32(0.25 * -1.0))
    assert_bits(gP[0], np.array([0.0, 0.0], f32))           # (1 * -1.5) * 1 + (-1 * -1.5) * 1 = +0
    assert_bits(gZ, gP)
    # the C entries' restatements on an empty problem and on d == 0
    assert W.spmm_scaled_ref(np.array([0], np.int64), [], [], None, 0, np.zeros((3, 2), f32)).shape == (0, 2)
    out = W.sddmm_rowsum_ref(phi[0], phi[1], phi[2], np.zeros((4, 0), f32), np.zeros((4, 0), f32))
    assert out.shape == (4,) and not out.view(np.uint32).any()


# ---- the C entries, without a device ------------------------------------------------------------------------

ENTRIES = {"srg_spmm_scaled_f32": 12, "srg_sddmm_rowsum_f32": 11}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entries_are_declared_exported_and_bound(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), "include/srgnn_hip.h does not declare it"
    assert name in _lib.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert any(line.split()[-1] == name and " T " in line for line in out.splitlines())
    fn = getattr(_lib.lib(), name)
    assert len(fn.argtypes) == ENTRIES[name] and fn.restype is ctypes.c_int


def _scaled_args(**kw):
    """A well-formed call on fake non-null pointers (never dereferenced: every case fails, or returns,
    before the device is touched)."""
    p = ctypes.c_void_p(4096)
    a = dict(indptr=p, indices=p, values=p, scale=p, scale_axis=0, n_rows=4, X=p, ldx=8, Y=p, ldy=8, d=8, stream=None)
    a.update(kw)
    return [a[k] for k in ("indptr", "indices", "values", "scale", "scale_axis", "n_rows", "X", "ldx", "Y", "ldy",
                           "d", "stream")]


def _rowsum_args(**kw):
    p = ctypes.c_void_p(4096)
    a = dict(indptr=p, indices=p, values=p, n_rows=4, G=p, ldg=8, P=p, ldp=8, d=8, out=p, stream=None)
    a.update(kw)
    return [a[k] for k in ("indptr", "indices", "values", "n_rows", "G", "ldg", "P", "ldp", "d", "out", "stream")]


def _rejected(fn, args):
    L = _lib.lib()
    L.srg_clear_error()
    assert fn(*args) == _lib.SRG_ERR_INVALID
    assert L.srg_last_error_code() == _lib.SRG_ERR_INVALID and _lib.last_error()
    L.srg_clear_error()
    assert L.srg_last_error_code() == 0


@pytest.mark.parametrize("bad", [dict(n_rows=-1), dict(d=-1), dict(ldx=7), dict(ldy=7), dict(ldx=-8), dict(scale_axis=2),
                                 dict(scale_axis=-1), dict(scale=None, scale_axis=2), dict(indptr=None), dict(Y=None)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_spmm_scaled_rejects_invalid_arguments_before_any_device_call(bad):
    _rejected(_lib.lib().srg_spmm_scaled_f32, _scaled_args(**bad))


@pytest.mark.parametrize("bad", [dict(n_rows=-1), dict(d=-1), dict(ldg=7), dict(ldp=7), dict(ldg=-8), dict(indptr=None),
                                 dict(out=None), dict(P=None), dict(out=None, d=0)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_rowsum_rejects_invalid_arguments_before_any_device_call(bad):
    _rejected(_lib.lib().srg_sddmm_rowsum_f32, _rowsum_args(**bad))


def test_empty_problems_return_ok_without_a_device():
    L = _lib.lib()
    assert L.srg_spmm_scaled_f32(*_scaled_args(n_rows=0)) == _lib.SRG_OK
    assert L.srg_spmm_scaled_f32(*_scaled_args(d=0)) == _lib.SRG_OK
    assert L.srg_spmm_scaled_f32(None, None, None, None, 1, 0, None, 0, None, 0, 0, None) == _lib.SRG_OK
    assert L.srg_sddmm_rowsum_f32(*_rowsum_args(n_rows=0)) == _lib.SRG_OK
    assert L.srg_sddmm_rowsum_f32(None, None, None, 0, None, 0, None, 0, 0, None, None) == _lib.SRG_OK
    assert L.srg_last_error_code() == 0
