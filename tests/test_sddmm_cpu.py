"""The sampled dense-dense product without a device: the host restatement (tests/sddmm_ref.py) that pins
srg_sddmm_f32 bit for bit is itself within the derived rounding bound of the exact dot product and
within the existing shim test's tolerance of torch's CPU autograd; the C entry is declared, exported
and bound, and rejects every invalid argument before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sddmm_ref import exact_and_scale, sddmm_ref
from srgnn import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srgnn_hip.h")
DIMS = [1, 3, 16, 17, 64, 130]
M, N, NNZ = 700, 500, 7000
U = 2.0 ** -24


def _case(d):
    rng = np.random.default_rng(1000 + d)
    rows = np.sort(rng.integers(0, M, NNZ))
    cols = rng.integers(0, N, NNZ)
    G = rng.standard_normal((M, d)).astype(np.float32)
    X = rng.standard_normal((N, d)).astype(np.float32)
    return rows, cols, G, X


@pytest.mark.parametrize("d", DIMS)
def test_restatement_is_within_the_rounding_bound_of_the_exact_dot_product(d):
    """|chain - exact| <= gamma_d * sum_j |G[r,j] X[c,j]| with gamma_d = d u / (1 - d u), u = 2^-24:
    d rounded products and d - 1 inexact additions (the first, to +0, is exact), so every term
    carries at most d factors (1 + delta), |delta| <= u.  Standard-normal inputs do not underflow.
    (The fp64 dot product's own error, about d * 2^-53 relative to the scale, is 2^-29 of the bound.)"""
    rows, cols, G, X = _case(d)
    got = sddmm_ref(rows, cols, G, X).astype(np.float64)
    exact, scale = exact_and_scale(rows, cols, G, X)
    gamma = d * U / (1.0 - d * U)
    ratio = np.abs(got - exact) / (gamma * scale)
    print(f"d={d}: max |chain - exact| / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("d", DIMS)
def test_restatement_is_within_the_shim_tolerance_of_torch_cpu_autograd(d):
    """torch's CPU autograd of the index_select / mul / index_add composition (the value gradient's
    sum over columns in torch's own vectorised order), at tests/test_shims_gpu.py's tolerance."""
    rows, cols, G, X = _case(d)
    idx = torch.from_numpy(np.stack([rows, cols]))
    v = torch.from_numpy(np.random.default_rng(d).standard_normal(NNZ).astype(np.float32)).requires_grad_(True)
    Xt = torch.from_numpy(X)
    torch.zeros(M, d).index_add(0, idx[0], Xt.index_select(0, idx[1]) * v.unsqueeze(-1)).backward(torch.from_numpy(G))
    want = v.grad
    got = torch.from_numpy(sddmm_ref(rows, cols, G, X))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_restatement_special_values_and_zero_width():
    """The chain's IEEE corner cases, stated once on the host: (-0)*x added to +0 is +0, Inf*0 is NaN,
    subnormal products are kept, and d == 0 leaves +0."""
    G = np.array([[-0.0, 0.0], [np.inf, 1.0], [2.0 ** -100, 0.0], [1.0, 1.0]], dtype=np.float32)
    X = np.array([[3.0, 0.0], [0.0, 1.0], [2.0 ** -40, 0.0], [-1.0, 1.0]], dtype=np.float32)
    out = sddmm_ref([0, 1, 2, 3], [0, 1, 2, 3], G, X)
    assert out[0] == 0 and not np.signbit(out[0])
    assert np.isnan(out[1])
    assert out[2] == np.float32(2.0 ** -140) and out[2] != 0          # a subnormal, not flushed
    assert out[3] == 0 and not np.signbit(out[3])                     # (-1 + 1) rounds to +0
    z = sddmm_ref([0, 1], [1, 0], G[:, :0], X[:, :0])
    assert z.shape == (2,) and not z.any() and not np.signbit(z).any()


# ---- the C entry, without a device -------------------------------------------------------------------

def test_entry_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"^int\s+srg_sddmm_f32\s*\(", text, flags=re.M), "include/srgnn_hip.h does not declare it"
    assert "srg_sddmm_f32" in _lib.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert any(line.split()[-1] == "srg_sddmm_f32" and " T " in line for line in out.splitlines())
    fn = _lib.lib().srg_sddmm_f32
    assert len(fn.argtypes) == 12 and fn.restype is ctypes.c_int


def _args(**kw):
    """A well-formed call on fake non-null pointers (never dereferenced: every case fails, or
    returns, before the device is touched)."""
    p = ctypes.c_void_p(4096)
    a = dict(indptr=p, indices=p, n_rows=4, nnz=8, G=p, ldg=8, X=p, ldx=8, d=8, perm=None, out=p, stream=None)
    a.update(kw)
    return [a[k] for k in ("indptr", "indices", "n_rows", "nnz", "G", "ldg", "X", "ldx", "d", "perm", "out",
                           "stream")]


@pytest.mark.parametrize("bad", [dict(n_rows=-1), dict(nnz=-1), dict(d=-1), dict(ldg=7), dict(ldx=7),
                                 dict(ldg=-8), dict(indptr=None), dict(out=None), dict(G=None), dict(X=None)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_invalid_arguments_fail_before_any_device_call(bad):
    L = _lib.lib()
    L.srg_clear_error()
    assert L.srg_sddmm_f32(*_args(**bad)) == _lib.SRG_ERR_INVALID
    assert L.srg_last_error_code() == _lib.SRG_ERR_INVALID
    assert _lib.last_error()
    L.srg_clear_error()
    assert L.srg_last_error_code() == 0


def test_empty_problems_return_ok_without_a_device():
    L = _lib.lib()
    assert L.srg_sddmm_f32(*_args(n_rows=0, nnz=0)) == _lib.SRG_OK
    assert L.srg_sddmm_f32(*_args(nnz=0)) == _lib.SRG_OK
    assert L.srg_sddmm_f32(*_args(n_rows=0)) == _lib.SRG_OK
    assert L.srg_sddmm_f32(None, None, 0, 0, None, 0, None, 0, 0, None, None, None) == _lib.SRG_OK
    assert L.srg_sddmm_f32(None, None, 4, 0, None, 8, None, 8, 8, None, None, None) == _lib.SRG_OK
    assert L.srg_last_error_code() == 0
