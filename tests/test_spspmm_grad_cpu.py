"""The contract of spspmm's adjoint on the host: the plain-loop restatement of its chains
(tests/spgemm_grad_ref.py) equals scipy's sampled products bit for bit on column-sorted operands and
meets the rounding bound; and without a HIP device the differentiable call raises RuntimeError like
every other entry point of the shim."""
import numpy as np
import pytest
import torch

import spgemm_grad_ref as R


@pytest.mark.parametrize("m,k,n", [(70, 50, 90), (33, 65, 130), (40, 30, 2000)])
def test_chain_restatement_equals_scipy_and_meets_the_bound(m, k, n):
    rng = np.random.default_rng(m * 1000 + n)
    A, B = R.rand_csr(rng, m, k, 0.2), R.rand_csr(rng, k, n, 0.15)
    crow, ccol, _ = R.forward_pattern(A, B)
    assert crow.size
    G = R.g_csr(crow, ccol, rng.standard_normal(crow.size), (m, n))
    (ga, xa, ma, la), (gb, xb, mb, lb) = R.loops_grads(A, B, G)
    sa, sb = R.scipy_grads(A, B, G)
    np.testing.assert_array_equal(ga.view(np.uint32), sa.view(np.uint32))
    np.testing.assert_array_equal(gb.view(np.uint32), sb.view(np.uint32))
    assert R.within_bound(ga, xa, ma, la).all() and R.within_bound(gb, xb, mb, lb).all()
    # the fp64 chain values are the dense adjoints
    Gd, Ad, Bd = (np.asarray(M.todense(), np.float64) for M in (G, A, B))
    ia, _ = R.coo(A)
    ib, _ = R.coo(B)
    np.testing.assert_allclose(xa, (Gd @ Bd.T)[ia[0], ia[1]], rtol=0, atol=1e-12 * max(1.0, ma.max()))
    np.testing.assert_allclose(xb, (Ad.T @ Gd)[ib[0], ib[1]], rtol=0, atol=1e-12 * max(1.0, mb.max()))


def test_duplicates_each_get_the_full_value():
    """Two stored copies of one (row, col) of A, and of B: each copy's gradient is the whole chain."""
    import scipy.sparse as sp
    A = sp.csr_matrix((np.array([1, 2, 3], np.float32), np.array([0, 0, 1], np.int32), np.array([0, 3])), shape=(1, 2))
    B = sp.csr_matrix((np.array([5, 7, 11, 13], np.float32), np.array([0, 0, 1, 1], np.int32), np.array([0, 2, 4])),
                      shape=(2, 2))
    G = sp.csr_matrix((np.array([0.5, 0.25], np.float32), np.array([0, 1], np.int32), np.array([0, 2])), shape=(1, 2))
    (ga, *_), (gb, *_) = R.loops_grads(A, B, G)
    assert ga.tolist() == [6.0, 6.0, 6.0]            # .5*5 + .5*7 ; the same ; .25*11 + .25*13
    assert gb.tolist() == [1.5, 1.5, 0.75, 0.75]     # (1 + 2) * .5 twice ; 3 * .25 twice


def test_grad_without_a_device_raises_runtime_error(monkeypatch):
    """No HIP device (as torch reports it): a RuntimeError that is not the NotImplementedError the
    shim raised while it had no adjoint."""
    import torch_sparse
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    i = torch.tensor([[0], [0]])
    v = torch.tensor([2.0], requires_grad=True)
    with pytest.raises(RuntimeError) as info:
        torch_sparse.spspmm(i, v, i, torch.tensor([3.0]), 1, 1, 1)
    assert not isinstance(info.value, NotImplementedError)
