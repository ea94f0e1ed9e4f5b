"""torch_sparse.spspmm's backward on the GPU (srg_spgemm_grad_f32): both operands' gradients bit for
bit against scipy's sampled products of the same fp32 operands (tests/spgemm_grad_ref.py), in the
caller's entry order, for the LDS and the scratch accumulator, dropped zero sums, duplicates and
shuffled input; the wavelet layer's two chained products on the committed fixture; one training
step of the reference's sparse-then-dense wavelet network; and the C entry on raw device pointers.
torch_sparse itself is absent, so parity with it stays unpinned, as for the forward."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spgemm_grad_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(index, value, requires_grad=False):
    return torch.from_numpy(np.ascontiguousarray(index)), \
        torch.from_numpy(np.ascontiguousarray(value)).requires_grad_(requires_grad)


def _backward(A, B, rng, need=(True, True), g=None):
    """spspmm on host COO tensors of the csr operands in stored order, then value.backward(G).
    Returns (C's row ids, C's column ids, G, valueA.grad, valueB.grad) as numpy (None where not asked)."""
    import torch_sparse
    (m, k), n = A.shape, B.shape[1]
    ia, va = _t(*R.coo(A), need[0])
    ib, vb = _t(*R.coo(B), need[1])
    idx, val = torch_sparse.spspmm(ia, va, ib, vb, m, k, n)
    assert val.requires_grad and not idx.requires_grad and val.device.type == "cpu"
    G = rng.standard_normal(val.numel()).astype(np.float32) if g is None else g
    val.backward(torch.from_numpy(G))
    for v in (va, vb):
        assert v.grad is None or (v.grad.device.type == "cpu" and v.grad.shape == v.shape)
    grads = [None if v.grad is None else v.grad.numpy() for v in (va, vb)]
    return idx[0].numpy(), idx[1].numpy(), G, grads[0], grads[1]


def _assert_bits(got, want):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# (m, k, n, density of A, of B): the LDS accumulator; pattern rows longer than a wave (65) and than
# the workgroup's 256 lanes (300 entries); the smallest case; the last LDS width and the first scratch
# width; the scratch accumulator on the A side (n columns) and on the B side (D has m columns)
CASES = [(70, 50, 90, 0.2, 0.15), (33, 65, 130, 1.0, 0.1), (5, 300, 40, 1.0, 0.1), (1, 1, 1, 1.0, 1.0),
         (500, 400, 16384, 0.02, 0.02), (64, 30, 16385, 0.3, 0.01), (64, 30, 20000, 0.3, 0.01),
         (20000, 30, 64, 0.01, 0.3)]


@pytest.mark.parametrize("m,k,n,da,db", CASES)
def test_both_gradients_equal_scipy_sampled_products(m, k, n, da, db):
    rng = np.random.default_rng(m * 7 + n)
    A, B = R.rand_csr(rng, m, k, da), R.rand_csr(rng, k, n, db)
    if m == 1:
        A.data[:], B.data[:] = 1.5, -2.0
    crow, ccol, G, ga, gb = _backward(A, B, rng)
    want = R.forward_pattern(A, B)
    np.testing.assert_array_equal(crow, want[0])
    np.testing.assert_array_equal(ccol, want[1])
    sa, sb = R.scipy_grads(A, B, R.g_csr(crow, ccol, G, (m, n)))
    _assert_bits(ga, sa)
    _assert_bits(gb, sb)


@pytest.mark.parametrize("side", [0, 1])
def test_only_the_side_that_requires_grad_is_computed(side, monkeypatch):
    """One operand requires grad: the other gets none, and the B side's transposes are built only
    when B's gradient is asked for."""
    import srgnn.sparse as S
    calls = []
    real = S.csr_transpose
    monkeypatch.setattr(S, "csr_transpose", lambda *a: (calls.append(1), real(*a))[1])
    rng = np.random.default_rng(11 + side)
    A, B = R.rand_csr(rng, 40, 30, 0.2), R.rand_csr(rng, 30, 50, 0.2)
    crow, ccol, G, ga, gb = _backward(A, B, rng, need=(side == 0, side == 1))
    want = R.scipy_grads(A, B, R.g_csr(crow, ccol, G, (40, 50)))
    got = (ga, gb)
    assert got[1 - side] is None
    _assert_bits(got[side], want[side])
    assert len(calls) == (0 if side == 0 else 3)


def test_dropped_zero_sums_are_plus_zero_of_the_gradient():
    """Row 0 of A is [1, -1, 1] against two equal rows of B and a third: the equal rows cancel
    exactly, C lacks those entries, and both gradients still equal the sampled scipy products."""
    rng = np.random.default_rng(5)
    m, k, n = 20, 12, 40
    A, B = R.rand_csr(rng, m, k, 0.3).toarray(), R.rand_csr(rng, k, n, 0.3).toarray()
    B[1, :] = B[0, :]
    A[0, :] = 0
    A[0, 0], A[0, 1], A[0, 5] = 1.0, -1.0, 1.0
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)                 # sorted columns, no stored zeros
    crow, ccol, G, ga, gb = _backward(A, B, rng)
    pat = lambda M: sp.csr_matrix((np.ones(M.nnz, np.float32), M.indices, M.indptr), shape=M.shape)
    assert crow.size < (pat(A) @ pat(B)).nnz                  # some sums cancelled and were dropped
    assert (crow == 0).sum() < B[0].nnz + B[5].nnz
    sa, sb = R.scipy_grads(A, B, R.g_csr(crow, ccol, G, (m, n)))
    _assert_bits(ga, sa)
    _assert_bits(gb, sb)


def _with_duplicates(rng, M, extra):
    """COO of M plus `extra` repeated (row, col) pairs with values of their own."""
    idx, val = R.coo(M)
    pick = rng.integers(0, val.size, extra)
    return np.hstack([idx, idx[:, pick]]), np.hstack([val, rng.standard_normal(extra).astype(np.float32)])


def _csr_in_order(idx, val, shape, order):
    ip = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(idx[0], minlength=shape[0]), out=ip[1:])
    return sp.csr_matrix((val[order], idx[1][order].astype(np.int32), ip), shape=shape)


def test_coalesced_shuffled_input_with_duplicates_keeps_the_callers_order():
    """coalesced=True: COO input in shuffled order with duplicate entries in A and in B.  Gradients
    arrive in the caller's entry order, each duplicate carries the full value, bitwise scipy's
    sampled products of the operands sorted by (row, col) (duplicates in stored order)."""
    import torch_sparse
    rng = np.random.default_rng(21)
    m, k, n = 45, 35, 60
    ia, va = _with_duplicates(rng, R.rand_csr(rng, m, k, 0.2), 40)
    ib, vb = _with_duplicates(rng, R.rand_csr(rng, k, n, 0.2), 50)
    pa, pb = rng.permutation(va.size), rng.permutation(vb.size)
    ia, va, ib, vb = ia[:, pa], va[pa], ib[:, pb], vb[pb]
    tia, tva = _t(ia, va, True)
    tib, tvb = _t(ib, vb, True)
    idx, val = torch_sparse.spspmm(tia, tva, tib, tvb, m, k, n, coalesced=True)
    G = rng.standard_normal(val.numel()).astype(np.float32)
    val.backward(torch.from_numpy(G))
    oa = np.lexsort((np.arange(va.size), ia[1], ia[0]))          # stable by (row, col)
    ob = np.lexsort((np.arange(vb.size), ib[1], ib[0]))
    A, B = _csr_in_order(ia, va, (m, k), oa), _csr_in_order(ib, vb, (k, n), ob)
    sa, sb = R.scipy_grads(A, B, R.g_csr(idx[0].numpy(), idx[1].numpy(), G, (m, n)))
    wa, wb = np.empty_like(sa), np.empty_like(sb)
    wa[oa], wb[ob] = sa, sb
    _assert_bits(tva.grad.numpy(), wa)
    _assert_bits(tvb.grad.numpy(), wb)
    # two stored copies of one (row, col) have one gradient
    key = ia[0] * k + ia[1]
    first, dup = {}, []
    for e, x in enumerate(key.tolist()):
        if x in first:
            dup.append((first[x], e))
        first.setdefault(x, e)
    got = tva.grad.numpy()
    assert dup and all(got[e0] == got[e1] for e0, e1 in dup)


def test_rows_in_stored_order_when_not_coalesced():
    """coalesced=False with the columns shuffled inside every row (and duplicates): the chains run in
    stored order -- bitwise the plain-loop restatement, and within the rounding bound of fp64."""
    import torch_sparse
    rng = np.random.default_rng(22)
    m, k, n = 40, 30, 70
    ia, va = _with_duplicates(rng, R.rand_csr(rng, m, k, 0.25), 30)
    ib, vb = _with_duplicates(rng, R.rand_csr(rng, k, n, 0.25), 30)
    oa = np.lexsort((rng.random(va.size), ia[0]))                # by row, shuffled within the row
    ob = np.lexsort((rng.random(vb.size), ib[0]))
    ia, va, ib, vb = ia[:, oa], va[oa], ib[:, ob], vb[ob]
    tia, tva = _t(ia, va, True)
    tib, tvb = _t(ib, vb, True)
    idx, val = torch_sparse.spspmm(tia, tva, tib, tvb, m, k, n)
    G = rng.standard_normal(val.numel()).astype(np.float32)
    val.backward(torch.from_numpy(G))
    A = _csr_in_order(ia, va, (m, k), np.arange(va.size))
    B = _csr_in_order(ib, vb, (k, n), np.arange(vb.size))
    (ga, xa, ma, la), (gb, xb, mb, lb) = R.loops_grads(A, B, R.g_csr(idx[0].numpy(), idx[1].numpy(), G, (m, n)))
    _assert_bits(tva.grad.numpy(), ga)
    _assert_bits(tvb.grad.numpy(), gb)
    assert R.within_bound(tva.grad.numpy(), xa, ma, la).all() and R.within_bound(tvb.grad.numpy(), xb, mb, lb).all()


def test_the_same_call_twice_gives_the_same_bits():
    rng = np.random.default_rng(3)
    A, B = R.rand_csr(rng, 300, 200, 0.1), R.rand_csr(rng, 200, 17000, 0.01)
    g = None
    runs = []
    for _ in range(2):
        _, _, g, ga, gb = _backward(A, B, rng, g=g)
        runs.append((ga, gb))
    _assert_bits(runs[0][0], runs[1][0])
    _assert_bits(runs[0][1], runs[1][1])


def test_edge_cases():
    """An empty A; an empty row of A and a row of B with no entries; device-resident inputs (host
    ones are every other test's); no_grad and no requires_grad run today's product; double
    backward raises."""
    import torch_sparse
    from srgnn import sparse as S
    rng = np.random.default_rng(9)
    m, k, n = 12, 9, 15
    B = R.rand_csr(rng, k, n, 0.4)
    ib, vb = _t(*R.coo(B), True)
    ea, eva = torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, requires_grad=True)
    idx, val = torch_sparse.spspmm(ea, eva, ib, vb, m, k, n)
    assert idx.shape == (2, 0) and val.numel() == 0
    val.sum().backward()
    assert eva.grad.shape == (0,) and vb.grad.shape == vb.shape and not vb.grad.any()
    assert not np.signbit(vb.grad.numpy()).any()
    # empty rows
    A, B = R.rand_csr(rng, m, k, 0.4).toarray(), B.toarray()
    A[3, :] = 0
    B[4, :] = 0
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    assert A.indptr[3] == A.indptr[4] and B.indptr[4] == B.indptr[5] and (A.indices == 4).any()
    crow, ccol, G, ga, gb = _backward(A, B, rng)
    sa, sb = R.scipy_grads(A, B, R.g_csr(crow, ccol, G, (m, n)))
    _assert_bits(ga, sa)
    _assert_bits(gb, sb)
    assert not ga[A.indices == 4].any()                       # an empty row of R: +0
    # device-resident inputs: gradients on the device, the same bits
    ia, va = R.coo(A)
    ib, vb = R.coo(B)
    dva = torch.from_numpy(va).cuda().requires_grad_(True)
    dvb = torch.from_numpy(vb).cuda().requires_grad_(True)
    idx, val = torch_sparse.spspmm(torch.from_numpy(ia).cuda(), dva, torch.from_numpy(ib).cuda(), dvb, m, k, n)
    assert idx.is_cuda and val.is_cuda
    val.backward(torch.from_numpy(G).cuda())
    assert dva.grad.is_cuda and dvb.grad.is_cuda
    _assert_bits(dva.grad.cpu().numpy(), sa)
    _assert_bits(dvb.grad.cpu().numpy(), sb)
    # no graph asked for: the values are srgnn.sparse.spgemm's, bit for bit
    a = S.csr_from_coo(torch.from_numpy(ia[0]).cuda(), torch.from_numpy(ia[1]).cuda(), torch.from_numpy(va).cuda(), m)
    b = S.csr_from_coo(torch.from_numpy(ib[0]).cuda(), torch.from_numpy(ib[1]).cuda(), torch.from_numpy(vb).cuda(), k)
    c_ip, c_ix, c_v = S.spgemm(*a, *b, n)
    tia, tib = torch.from_numpy(ia), torch.from_numpy(ib)
    with torch.no_grad():
        i1, v1 = torch_sparse.spspmm(tia, torch.from_numpy(va).requires_grad_(True), tib, torch.from_numpy(vb), m, k, n)
    i2, v2 = torch_sparse.spspmm(tia, torch.from_numpy(va), tib, torch.from_numpy(vb), m, k, n)
    i3, v3 = torch_sparse.spspmm(tia, torch.from_numpy(va).requires_grad_(True), tib, torch.from_numpy(vb), m, k, n)
    for i, v in ((i1, v1), (i2, v2), (i3, v3)):
        np.testing.assert_array_equal(i[1].numpy(), c_ix.cpu().numpy())
        _assert_bits(v.detach().numpy(), c_v.cpu().numpy())
    assert not v1.requires_grad and not v2.requires_grad and v3.requires_grad
    # double backward is not supported
    tva = torch.from_numpy(va).requires_grad_(True)
    _, val = torch_sparse.spspmm(tia, tva, tib, torch.from_numpy(vb), m, k, n)
    (g1,) = torch.autograd.grad(val, tva, torch.from_numpy(G), create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


# ---- the wavelet layer on the committed fixture ----------------------------------------------------

def _wav_rand():
    z = np.load(os.path.join(REPO, "tests", "golden", "wav_rand.npz"), allow_pickle=False)
    n = z["phi0_indptr"].size - 1
    phis = [sp.csr_matrix((z[f"phi{i}_data"], z[f"phi{i}_indices"], z[f"phi{i}_indptr"]), shape=(n, n)) for i in (0, 1)]
    return n, phis, z["x"]


def _diag(theta):
    n = theta.size
    return sp.csr_matrix((theta, np.arange(n, dtype=np.int32), np.arange(n + 1)), shape=(n, n))


def test_layer_chain_on_the_fixture_theta_grad_equals_scipy():
    """C1 = spspmm(phi0, diag theta), C2 = spspmm(C1, phi1), C2.backward(G2): theta.grad is bit for
    bit sample_diag(phi0^T @ G1) with G1 = sample_C1(G2 @ phi1^T) from scipy; a gross-error guard
    against the fp64 dense value (the plain-loop restatement of these chains sits at 1.2e-7
    relative on this fixture: 3.7e-7 against 3.1)."""
    import torch_sparse
    n, (phi0, phi1), _ = _wav_rand()
    assert (n, phi0.nnz, phi1.nnz) == (130, 3630, 2628)
    rng = np.random.default_rng(130)
    theta = rng.uniform(0.9, 1.1, n).astype(np.float32)
    i0, v0 = _t(*R.coo(phi0))
    i1, v1 = _t(*R.coo(phi1))
    di = torch.arange(n).repeat(2, 1)
    th = torch.from_numpy(theta).view(n, 1).requires_grad_(True)
    c1i, c1v = torch_sparse.spspmm(i0, v0, di, th.view(-1), n, n, n)
    c2i, c2v = torch_sparse.spspmm(c1i, c1v, i1, v1, n, n, n)
    assert (c1v.numel(), c2v.numel()) == (3630, 15810)
    G2 = rng.standard_normal(c2v.numel()).astype(np.float32)
    c2v.backward(torch.from_numpy(G2))
    # scipy: the forward's patterns and values, then the two sampled products
    D = _diag(theta)
    r1, q1, w1 = R.forward_pattern(phi0, D)
    np.testing.assert_array_equal(c1i.numpy(), np.vstack([r1, q1]))
    _assert_bits(c1v.detach().numpy(), w1)
    C1 = R.g_csr(r1, q1, w1, (n, n))
    r2, q2, _ = R.forward_pattern(C1, phi1)
    np.testing.assert_array_equal(c2i.numpy(), np.vstack([r2, q2]))
    assert max(np.diff(phi1.indptr).max(), np.diff(phi0.tocsc().indptr).max()) <= 57
    G1, _ = R.scipy_grads(C1, phi1, R.g_csr(r2, q2, G2, (n, n)))
    _, want = R.scipy_grads(phi0, D, R.g_csr(r1, q1, G1, (n, n)))
    got = th.grad.numpy().reshape(-1)
    assert th.grad.shape == (n, 1)
    _assert_bits(got, want)
    G2d = np.asarray(R.g_csr(r2, q2, G2, (n, n)).todense(), np.float64)
    P0, P1 = (np.asarray(p.todense(), np.float64) for p in (phi0, phi1))
    G1d = (G2d @ P1.T) * (P0 != 0)
    dense = (P0 * G1d).sum(axis=0)
    assert np.abs(got - dense).max() <= 1e-4 * np.abs(dense).max()


def _network(spspmm, spmm, mm, phi, phi_inv, feat, params, n):
    """The call sequence of the reference's wavelet network (wavelet/src: GraphWaveletNeuralNetwork =
    SparseGraphWaveletLayer, then DenseGraphWaveletLayer, then log_softmax), restated: each layer
    rescales phi by its diagonal filter with one spspmm, multiplies by phi^-1 with a second, and
    applies the product to the filtered features with spmm; the sparse layer filters COO features
    with spmm and ends in relu and dropout (rate 0 here, so that fp64 autograd sees the same
    network), the dense layer filters with mm."""
    w1, t1, w2, t2 = params
    di = torch.arange(n).repeat(2, 1)
    ri, rv = spspmm(phi[0], phi[1], di, t1.view(-1), n, n, n)
    pi, pv = spspmm(ri, rv, phi_inv[0], phi_inv[1], n, n, n)
    filtered = spmm(feat[0], feat[1], n, w1.shape[0], w1)
    h = torch.nn.functional.dropout(torch.nn.functional.relu(spmm(pi, pv, n, n, filtered)), training=True, p=0.0)
    ri, rv = spspmm(phi[0], phi[1], di, t2.view(-1), n, n, n)
    pi, pv = spspmm(ri, rv, phi_inv[0], phi_inv[1], n, n, n)
    return torch.nn.functional.log_softmax(spmm(pi, pv, n, n, mm(h, w2)), dim=1)


def _dense_ops(dtype):
    """spspmm / spmm on dense matrices carried as (None, matrix): the same network in plain torch."""
    def to_dense(i, v, rows, cols):
        return v if i is None else torch.zeros(rows, cols, dtype=dtype).index_put((i[0], i[1]), v.to(dtype), accumulate=True)

    def spspmm(ia, va, ib, vb, m, k, n):
        return None, to_dense(ia, va, m, k) @ to_dense(ib, vb, k, n)

    def spmm(i, v, m, n, mat):
        return to_dense(i, v, m, n) @ mat
    return spspmm, spmm


def test_one_training_step_of_the_wavelet_network():
    """Three Adam steps of the sparse-then-dense wavelet network on wav_rand through the shim: at
    step 1 every parameter (both diagonal filters included) has a finite, nonzero gradient that
    agrees with fp64 dense CPU autograd of the same network under the gross-error guard
    (max |g - g64| <= 1e-4 max |g64|); the loss is finite at every step."""
    import torch_sparse
    n, (phi0, phi1), x = _wav_rand()
    filters, classes = 16, 4
    gen = torch.Generator().manual_seed(7)
    labels = torch.randint(0, classes, (n,), generator=gen)
    xavier = lambda i, o: torch.empty(i, o).uniform_(-(6.0 / (i + o)) ** 0.5, (6.0 / (i + o)) ** 0.5, generator=gen)
    w1, w2 = xavier(x.shape[1], filters), xavier(filters, classes)
    t1 = torch.empty(n, 1).uniform_(0.9, 1.1, generator=gen)
    t2 = torch.empty(n, 1).uniform_(0.9, 1.1, generator=gen)
    fr, fc = x.nonzero()
    feat = (torch.from_numpy(np.vstack([fr, fc])), torch.from_numpy(x[fr, fc]))
    phi, phi_inv = _t(*R.coo(phi0)), _t(*R.coo(phi1))

    p64 = [p.double().requires_grad_(True) for p in (w1, t1, w2, t2)]
    s64, m64 = _dense_ops(torch.float64)
    loss64 = torch.nn.functional.nll_loss(_network(s64, m64, torch.mm, phi, phi_inv, feat, p64, n), labels)
    loss64.backward()

    params = [p.clone().requires_grad_(True) for p in (w1, t1, w2, t2)]
    opt = torch.optim.Adam(params, lr=0.01)
    for step in range(3):
        opt.zero_grad()
        pred = _network(torch_sparse.spspmm, torch_sparse.spmm, torch.mm, phi, phi_inv, feat, params, n)
        loss = torch.nn.functional.nll_loss(pred, labels)
        assert torch.isfinite(loss), (step, loss)
        loss.backward()
        if step == 0:
            assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item())
            for name, p, q in zip(("W1", "theta1", "W2", "theta2"), params, p64):
                g, g64 = p.grad.double(), q.grad
                assert g.shape == p.shape and bool(torch.isfinite(g).all()) and bool((g != 0).any()), name
                assert float((g - g64).abs().max()) <= 1e-4 * float(g64.abs().max()), name
        opt.step()


# ---- the C entry -------------------------------------------------------------------------------------

def test_c_entry_on_raw_pointers_and_its_argument_checks():
    """srg_spgemm_grad_f32 through ctypes on device pointers, one LDS and one scratch case: bitwise
    the Python path's gradient of A; a null pointer, a negative shape and a scratch smaller than
    one accumulator return SRG_ERR_INVALID with a message and launch nothing."""
    import torch_sparse
    from srgnn import _lib
    from srgnn import sparse as S
    L = _lib.lib()
    for m, k, n in ((50, 40, 300), (50, 40, 16500)):
        rng = np.random.default_rng(n)
        A, B = R.rand_csr(rng, m, k, 0.2), R.rand_csr(rng, k, n, 0.02)
        crow, ccol, G, ga, _ = _backward(A, B, rng, need=(True, False))
        dev = torch.device("cuda", torch.cuda.current_device())
        p_ip = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
        p_ix = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
        Gc = R.g_csr(crow, ccol, G, (m, n))
        d_ip, d_ix, d_v = (torch.from_numpy(a).to(dev) for a in (Gc.indptr.astype(np.int64), Gc.indices.astype(np.int32), Gc.data))
        r_ip, r_ix, r_v = (torch.from_numpy(a).to(dev) for a in (B.indptr.astype(np.int64), B.indices.astype(np.int32), B.data))
        out = torch.full((A.nnz,), float("nan"), device=dev)
        need = ctypes.c_int64(-1)
        assert L.srg_spgemm_scratch_bytes(m, n, ctypes.byref(need)) == _lib.SRG_OK
        assert (need.value > 0) == (n > 16384)
        scratch = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        args = [p_ip.data_ptr(), p_ix.data_ptr(), m, d_ip.data_ptr(), d_ix.data_ptr(), d_v.data_ptr(), r_ip.data_ptr(),
                r_ix.data_ptr(), r_v.data_ptr(), n, out.data_ptr(), scratch.data_ptr() if need.value else None,
                need.value, None]
        torch.cuda.synchronize()
        assert L.srg_spgemm_grad_f32(*args) == _lib.SRG_OK, _lib.last_error()
        torch.cuda.synchronize()
        _assert_bits(out.cpu().numpy(), ga)
        # one accumulator of scratch is enough (one workgroup walks every row)
        if need.value:
            out.fill_(float("nan"))
            torch.cuda.synchronize()
            assert L.srg_spgemm_grad_f32(*args[:12], 4 * n, None) == _lib.SRG_OK, _lib.last_error()
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), ga)
            for small in ((scratch.data_ptr(), 4 * n - 1), (None, need.value)):
                assert L.srg_spgemm_grad_f32(*args[:11], small[0], small[1], None) == _lib.SRG_ERR_INVALID
                assert "scratch" in _lib.last_error()
        assert L.srg_spgemm_grad_f32(None, *args[1:]) == _lib.SRG_ERR_INVALID
        assert "null" in _lib.last_error()
        for bad in ((2, -1), (9, -5)):
            a = list(args)
            a[bad[0]] = bad[1]
            assert L.srg_spgemm_grad_f32(*a) == _lib.SRG_ERR_INVALID
            assert "shape" in _lib.last_error()
        assert L.srg_spgemm_grad_f32(None, None, 0, None, None, None, None, None, None, 5, None, None, 0, None) == _lib.SRG_OK
    # the Python entry (the scratch case): the same bits, also with one accumulator of scratch; it
    # validates what the kernel trusts
    _assert_bits(S.spgemm_grad(p_ip, p_ix, d_ip, d_ix, d_v, r_ip, r_ix, r_v, n).cpu().numpy(), ga)
    _assert_bits(S.spgemm_grad(p_ip, p_ix, d_ip, d_ix, d_v, r_ip, r_ix, r_v, n, scratch_limit=4 * n).cpu().numpy(), ga)
    twice = d_ix.clone()
    row = int((d_ip[1:] - d_ip[:-1]).argmax())
    assert int(d_ip[row + 1] - d_ip[row]) >= 2
    twice[int(d_ip[row]) + 1] = twice[int(d_ip[row])]
    with pytest.raises(ValueError):
        S.spgemm_grad(p_ip, p_ix, d_ip, twice, d_v, r_ip, r_ix, r_v, n)              # a row of D repeats a column
    with pytest.raises(ValueError):
        S.spgemm_grad(p_ip, p_ix, d_ip, d_ix, d_v, r_ip[:-1], r_ix, r_v, n)          # P's ids past R's rows / bad R
    with pytest.raises(ValueError):
        S.spgemm_grad(p_ip, p_ix, d_ip, d_ix, d_v, r_ip, r_ix, r_v, n - 16000)       # column ids >= n_cols
    with pytest.raises(ValueError):
        S.spgemm_grad(p_ip, p_ix, d_ip[:-1], d_ix, d_v, r_ip, r_ix, r_v, n)          # D's rows != P's
