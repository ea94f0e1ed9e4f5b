"""srg_sddmm_f32 on the GPU: every result bit for bit the host restatement (tests/sddmm_ref.py) -- one
sequential chain per entry, columns ascending, products rounded before they are added -- through
srgnn.sparse.sddmm (tile tails, the aligned and the unaligned path, rows across tiles, tiles across
rows, column windows, perm, special values), through torch_sparse.spmm's backward (the caller's
entry order, duplicates, expanded and transposed gradients, only the asked side computed, peak
memory), under another stream, on raw device pointers, and on the wavelet layer chain of the
committed fixture."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sddmm_ref import assert_bits, csr_rows, sddmm_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 257]
SINGLES = [1, 63, 64, 65, 127, 128, 129]
PATTERNS = ["random", "one_long_row", "one_by_one", "deep_search"] + [f"single_{k}" for k in SINGLES]


@functools.lru_cache(maxsize=None)
def _pattern(name):
    """(indptr int64, indices int32, rows of X) of a named CSR pattern."""
    rng = np.random.default_rng(len(name) * 131 + sum(map(ord, name)))
    if name == "random":                    # 64-entry tiles straddle many rows (about 10 entries a row)
        A = sp.random(700, 500, density=0.02, format="csr", random_state=rng, dtype=np.float32)
        return A.indptr.astype(np.int64), A.indices.astype(np.int32), 500
    if name == "one_long_row":              # 9 rows, only row 3 holds entries: 300, over five tiles
        ip = np.array([0, 0, 0, 0, 300, 300, 300, 300, 300, 300], dtype=np.int64)
        return ip, rng.integers(0, 40, 300).astype(np.int32), 40
    if name == "one_by_one":
        return np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), 1
    if name == "deep_search":               # 20000 rows, 50 entries: the row search's depth
        rows = np.sort(rng.choice(20000, 50, replace=False))
        ip = np.zeros(20001, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=20000), out=ip[1:])
        return ip, rng.integers(0, 300, 50).astype(np.int32), 300
    k = int(name.split("_")[1])             # k rows of one entry: 64 different rows per tile, and the tile tails
    return np.arange(k + 1, dtype=np.int64), rng.integers(0, 90, k).astype(np.int32), 90


def _panels(rng, m, n, d):
    return rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("d", DIMS)
def test_every_entry_is_the_restated_chain(d, name):
    from srgnn.sparse import sddmm
    ip, ix, n = _pattern(name)
    G, X = _panels(np.random.default_rng(d), ip.size - 1, n, d)
    tip, tix, tG, tX = _dev(ip, ix, G, X)
    got = sddmm(tip, tix, tG, tX)
    assert got.shape == (ix.size,) and got.dtype == torch.float32 and got.is_cuda
    assert_bits(got.cpu().numpy(), sddmm_ref(csr_rows(ip), ix, G, X), f"{name} d={d}")


@pytest.mark.parametrize("name", ["random", "single_65"])
def test_zero_width_panels_give_plus_zero(name):
    from srgnn.sparse import sddmm
    ip, ix, n = _pattern(name)
    tip, tix = _dev(ip, ix)
    out = torch.full((ix.size,), 7.0, device="cuda")
    got = sddmm(tip, tix, torch.empty(ip.size - 1, 0, device="cuda"), torch.empty(n, 0, device="cuda"), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert not got.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("aligned", [False, True], ids=["4-byte aligned", "16-byte aligned"])
@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("d", [4, 16, 33])
def test_column_windows_perm_and_a_canary_around_out(d, with_perm, aligned):
    """G and X are column windows of wider panels: row stride d + 3 and first column 1 (4-byte but not
    16-byte aligned: the unaligned path), or first column 4 and a row stride that is a multiple of 4
    (the aligned path on a window; d = 33 leaves it one column for its tail).  out is a slice of a
    larger buffer whose other cells keep their canary."""
    from srgnn.sparse import sddmm
    first, extra = (4, 8 + (-d) % 4) if aligned else (1, 3)
    ip, ix, n = _pattern("random")
    m, nnz = ip.size - 1, ix.size
    rng = np.random.default_rng(1000 * d + first)
    Gw, Xw = _panels(rng, m, n, d + extra)
    tip, tix, tGw, tXw = _dev(ip, ix, Gw, Xw)
    tG, tX = tGw[:, first:first + d], tXw[:, first:first + d]
    assert tG.stride(0) == d + extra and tG.data_ptr() % 16 == (4 * first) % 16
    want = sddmm_ref(csr_rows(ip), ix, Gw[:, first:first + d], Xw[:, first:first + d])
    perm = rng.permutation(nnz)
    if with_perm:
        scattered = np.empty_like(want)
        scattered[perm] = want
        want = scattered
    buf = torch.full((nnz + 23,), -12345.0, device="cuda")
    out = buf[11:11 + nnz]
    got = sddmm(tip, tix, tG, tX, perm=_dev(perm.astype(np.int64))[0] if with_perm else None, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert_bits(host[11:11 + nnz], want)
    assert (host[:11] == -12345.0).all() and (host[11 + nnz:] == -12345.0).all()


def test_non_unit_column_stride_is_made_contiguous():
    from srgnn.sparse import sddmm
    ip, ix, n = _pattern("random")
    G, X = _panels(np.random.default_rng(5), ip.size - 1, n, 12)
    tip, tix, tGt, tXt = _dev(ip, ix, G.T, X.T)
    got = sddmm(tip, tix, tGt.t(), tXt.t())
    assert_bits(got.cpu().numpy(), sddmm_ref(csr_rows(ip), ix, G, X))


@pytest.mark.parametrize("d", [16, 17], ids=["aligned path", "unaligned path"])
def test_special_values_follow_ieee_through_the_chain(d):
    """NaN, +-Inf, -0 and subnormals in both panels: NaN where the restatement has NaN, every other
    result bitwise; (-0)*x from +0 is +0, Inf*0 is NaN, subnormal products are not flushed."""
    from srgnn.sparse import sddmm
    ip, ix, n = _pattern("random")
    m = ip.size - 1
    rng = np.random.default_rng(77 + d)
    G, X = _panels(rng, m, n, d)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, 2.0 ** -100, -2.0 ** -120],
                        dtype=np.float32)
    for P in (G, X):
        hit = rng.random(P.shape) < 0.01
        P[hit] = rng.choice(specials, int(hit.sum()))
    # five stated entries, appended as rows m .. m+4 of the pattern, each meeting its own row of X
    G4, X4 = np.zeros((5, d), np.float32), np.zeros((5, d), np.float32)
    G4[0, 0], X4[0, 0] = -0.0, 3.0                          # +0 + (-0 * 3) = +0
    G4[1, 0], X4[1, 0] = np.inf, 0.0                        # Inf * 0 = NaN
    G4[2, 0], X4[2, 0] = 2.0 ** -100, 2.0 ** -40            # a subnormal product, kept
    G4[3, :2], X4[3, :2] = [1.0, 1.0], [-1.0, 1.0]          # -1 + 1 = +0
    G4[4, -2:], X4[4, -2:] = [1e-40, -3e-42], [0.5, 0.25]   # subnormal products, a subnormal sum
    G, X = np.vstack([G, G4]), np.vstack([X, X4])
    ip = np.concatenate([ip, ip[-1] + np.arange(1, 6)])
    ix = np.concatenate([ix, n + np.arange(5)]).astype(np.int32)
    want = sddmm_ref(csr_rows(ip), ix, G, X)
    assert np.isnan(want).any() and np.isinf(want).any() and 0 < np.isnan(want).sum() < want.size // 2
    tail = want[-5:]
    assert tail[0] == 0 and not np.signbit(tail[0]) and np.isnan(tail[1])
    assert tail[2] == np.float32(2.0 ** -140) and tail[3] == 0 and not np.signbit(tail[3])
    assert 0 < tail[4] < np.finfo(np.float32).tiny
    tip, tix, tG, tX = _dev(ip, ix, G, X)
    assert_bits(sddmm(tip, tix, tG, tX).cpu().numpy(), want)


# ---- through torch_sparse.spmm with host tensors -------------------------------------------------------

def _coo_case(rng, m, n, nnz, d, shuffled):
    """Host COO (with duplicates when shuffled), values, X, G as numpy."""
    rows = rng.integers(0, m, nnz)
    cols = rng.integers(0, n, nnz)
    if not shuffled:
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
    val = rng.standard_normal(nnz).astype(np.float32)
    X, G = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    return rows, cols, val, X, G


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled with duplicates"])
@pytest.mark.parametrize("d", [1, 16, 17, 64, 130])
def test_spmm_value_gradient_is_the_restated_chain_in_the_callers_order(d, shuffled):
    import torch_sparse
    m, n, nnz = (40, 30, 3000) if shuffled else (700, 500, 7000)
    rows, cols, val, X, G = _coo_case(np.random.default_rng(d + 50 * shuffled), m, n, nnz, d, shuffled)
    if shuffled:
        assert np.unique(rows * n + cols).size < nnz and (np.diff(rows) < 0).any()
    idx = torch.from_numpy(np.stack([rows, cols]))
    v = torch.from_numpy(val).requires_grad_(True)
    Xt = torch.from_numpy(X).requires_grad_(True)
    torch_sparse.spmm(idx, v, m, n, Xt).backward(torch.from_numpy(G))
    assert v.grad.device.type == "cpu" and v.grad.shape == v.shape
    assert_bits(v.grad.numpy(), sddmm_ref(rows, cols, G, X), "value gradient")
    # the matrix gradient keeps its bits: the index_add composition's CPU autograd
    vr, Xr = torch.from_numpy(val).requires_grad_(True), torch.from_numpy(X).requires_grad_(True)
    torch.zeros(m, d).index_add(0, idx[0], Xr.index_select(0, idx[1]) * vr.unsqueeze(-1)).backward(torch.from_numpy(G))
    assert_bits(Xt.grad.numpy(), Xr.grad.numpy(), "matrix gradient")
    torch.testing.assert_close(v.grad, vr.grad, rtol=1e-5, atol=1e-5 * float(vr.grad.abs().max()))


def test_expanded_and_transposed_gradients():
    """.sum().backward() hands the backward an expanded gradient (every stride 0); backward through a
    transpose hands it a transposed view."""
    import torch_sparse
    m, n, nnz, d = 60, 50, 900, 19
    rows, cols, val, X, G = _coo_case(np.random.default_rng(19), m, n, nnz, d, True)
    idx, Xt = torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(X)
    v = torch.from_numpy(val).requires_grad_(True)
    torch_sparse.spmm(idx, v, m, n, Xt).sum().backward()
    assert_bits(v.grad.numpy(), sddmm_ref(rows, cols, np.ones((m, d), np.float32), X), "expanded")
    v = torch.from_numpy(val).requires_grad_(True)
    torch_sparse.spmm(idx, v, m, n, Xt).t().backward(torch.from_numpy(np.ascontiguousarray(G.T)))
    assert_bits(v.grad.numpy(), sddmm_ref(rows, cols, G, X), "transposed")


@pytest.mark.parametrize("side", ["value", "matrix"])
def test_only_the_side_that_requires_grad_is_computed(side, monkeypatch):
    import srgnn.sparse as S
    import torch_sparse
    calls = {"spmm_scatter": 0, "sddmm": 0}
    for name in calls:
        def counted(*a, _f=getattr(S, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(S, name, counted)
    m, n, nnz, d = 60, 50, 900, 8
    rows, cols, val, X, G = _coo_case(np.random.default_rng(8), m, n, nnz, d, True)
    v = torch.from_numpy(val).requires_grad_(side == "value")
    Xt = torch.from_numpy(X).requires_grad_(side == "matrix")
    out = torch_sparse.spmm(torch.from_numpy(np.stack([rows, cols])), v, m, n, Xt)
    assert calls == {"spmm_scatter": 1, "sddmm": 0}
    out.backward(torch.from_numpy(G))
    if side == "value":
        assert calls == {"spmm_scatter": 1, "sddmm": 1} and Xt.grad is None
        assert_bits(v.grad.numpy(), sddmm_ref(rows, cols, G, X))
    else:
        assert calls == {"spmm_scatter": 2, "sddmm": 0} and v.grad is None and Xt.grad is not None


def test_backward_peak_memory_stays_far_below_one_nnz_by_d_buffer():
    """Device tensors, 2000 x 2000, nnz = 200 000, d = 64, only `value` requiring grad.  T = nnz*d*4 =
    51.2 MB is one of the index_select / mul temporaries of the composition this replaces (it holds
    two to three of them); the kernel's path allocates the nnz*4-byte result."""
    import torch_sparse
    m = n = 2000
    nnz, d = 200_000, 64
    gen = torch.Generator(device="cuda").manual_seed(3)
    idx = torch.randint(0, m, (2, nnz), device="cuda", generator=gen)
    v = torch.randn(nnz, device="cuda", generator=gen).requires_grad_(True)
    X = torch.randn(n, d, device="cuda", generator=gen)
    G = torch.randn(m, d, device="cuda", generator=gen)
    out = torch_sparse.spmm(idx, v, m, n, X)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    T = nnz * d * 4
    print(f"backward peak above the forward's state: {peak} bytes = {peak / T:.4f} T")
    assert peak < T / 2
    assert_bits(v.grad.cpu().numpy(), sddmm_ref(idx[0].cpu().numpy(), idx[1].cpu().numpy(), G.cpu().numpy(),
                                                X.cpu().numpy()))


# ---- determinism, streams, the C entry ---------------------------------------------------------------

def test_same_bits_twice_and_under_another_stream():
    from srgnn.sparse import sddmm
    ip, ix, n = _pattern("random")
    G, X = _panels(np.random.default_rng(4), ip.size - 1, n, 70)
    tip, tix, tG, tX = _dev(ip, ix, G, X)
    a = sddmm(tip, tix, tG, tX)
    b = sddmm(tip, tix, tG, tX)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = sddmm(tip, tix, tG, tX)
    side.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert_bits(a.cpu().numpy(), sddmm_ref(csr_rows(ip), ix, G, X))


@pytest.mark.parametrize("path", ["aligned", "unaligned"])
@pytest.mark.parametrize("with_perm", [False, True])
def test_c_entry_on_raw_device_pointers(path, with_perm):
    from srgnn import _lib
    L = _lib.lib()
    ip, ix, n = _pattern("random")
    m, nnz, d = ip.size - 1, ix.size, 22        # aligned: 20 columns in 16-byte pieces and a tail of 2
    first, ld = (0, 24) if path == "aligned" else (1, 23)
    rng = np.random.default_rng(ld)
    Gw, Xw = _panels(rng, m, n, ld)
    perm = rng.permutation(nnz).astype(np.int64)
    tip, tix, tG, tX, tperm = _dev(ip, ix, Gw, Xw, perm)
    out = torch.full((nnz,), -1.0, device="cuda")
    gp, xp = tG.data_ptr() + 4 * first, tX.data_ptr() + 4 * first
    assert (gp % 16 == 0) == (path == "aligned")
    torch.cuda.synchronize()
    rc = L.srg_sddmm_f32(tip.data_ptr(), tix.data_ptr(), m, nnz, gp, ld, xp, ld, d,
                         tperm.data_ptr() if with_perm else None, out.data_ptr(), None)
    assert rc == _lib.SRG_OK, _lib.last_error()
    torch.cuda.synchronize()
    want = sddmm_ref(csr_rows(ip), ix, Gw[:, first:first + d], Xw[:, first:first + d])
    if with_perm:
        scattered = np.empty_like(want)
        scattered[perm] = want
        want = scattered
    assert_bits(out.cpu().numpy(), want)


# ---- the wavelet layer chain on the committed fixture --------------------------------------------------

def test_layer_chain_on_the_fixture_product_value_grad_is_the_restated_chain():
    """theta -> spspmm(phi0, diag theta) -> spspmm(., phi1) = (pi, pv); spmm(pi, pv, n, n, filtered)
    .backward(G): pv.grad is bit for bit the restatement, and the gradient reaches theta."""
    import torch_sparse
    z = np.load(os.path.join(REPO, "tests", "golden", "wav_rand.npz"), allow_pickle=False)
    n = z["phi0_indptr"].size - 1
    phi = [(np.stack([csr_rows(z[f"phi{i}_indptr"]), z[f"phi{i}_indices"].astype(np.int64)]),
            z[f"phi{i}_data"].astype(np.float32)) for i in (0, 1)]
    assert (n, phi[0][1].size, phi[1][1].size) == (130, 3630, 2628)
    rng = np.random.default_rng(130)
    theta = torch.from_numpy(rng.uniform(0.9, 1.1, n).astype(np.float32)).requires_grad_(True)
    di = torch.arange(n).repeat(2, 1)
    c1i, c1v = torch_sparse.spspmm(torch.from_numpy(phi[0][0]), torch.from_numpy(phi[0][1]), di, theta, n, n, n)
    pi, pv = torch_sparse.spspmm(c1i, c1v, torch.from_numpy(phi[1][0]), torch.from_numpy(phi[1][1]), n, n, n)
    assert pv.numel() == 15810
    pv.retain_grad()
    filtered, G = _panels(rng, n, n, 16)
    torch_sparse.spmm(pi, pv, n, n, torch.from_numpy(filtered)).backward(torch.from_numpy(G))
    assert_bits(pv.grad.numpy(), sddmm_ref(pi[0].numpy(), pi[1].numpy(), G, filtered))
    assert theta.grad is not None and bool(torch.isfinite(theta.grad).all()) and bool(theta.grad.abs().max() > 0)
