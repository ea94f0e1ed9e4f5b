"""srgnn.wavelet_conv on the GPU: srg_spmm_scaled_f32 and srg_sddmm_rowsum_f32 bit for bit the host
restatement (tests/wavelet_conv_ref.py) over every lane-group width, the cooperative load's size and its
neighbours, both scale axes, column windows inside canaries and IEEE special values; wavelet_conv's Y, gZ
and gtheta bit for bit the existing shims' re-associated composition and within the derived bound
 of the shims' chain in the reference's call order; host and device inputs, only the
asked side computed, determinism on a side stream, three Adam steps of the wavelet network against fp64
dense autograd, the backward's peak memory, and both C entries on raw device pointers."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import wavelet_conv_ref as W
from sddmm_ref import assert_bits, csr_rows

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every lane-group size (1, 2, 4, ..., 64), its neighbours, and the 64-column loop
DIMS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 64, 65, 130]
# the cooperative load's 16 entries and its neighbours, a wave's 64, and a row longer than a wave
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 257]
N_COLS = 300


def _csr_of_lengths(lengths, n_cols, rng):
    """A CSR with the given row lengths, unsorted column ids, a repeated id in every row of 2 or more."""
    ip = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=ip[1:])
    ix = rng.integers(0, n_cols, int(ip[-1])).astype(np.int32)
    for r, n in enumerate(lengths):
        if n >= 2:
            ix[ip[r] + n - 1] = ix[ip[r]]
    v = (rng.standard_normal(ix.size) * 2).astype(np.float32)
    return ip, ix, v


@functools.lru_cache(maxsize=None)
def _ladder_csr():
    """65 rows cycling through LENGTHS: 65 = 1 mod 2, 4, ..., 64, so at every lane-group width the row
    count is no multiple of the rows per wave and the last wave has one live group; 4 rows per
    workgroup at d > 32 makes 17 workgroups."""
    return _csr_of_lengths([LENGTHS[r % len(LENGTHS)] for r in range(65)], N_COLS, np.random.default_rng(65))


@functools.lru_cache(maxsize=None)
def _rowsum_csr(name):
    rng = np.random.default_rng(len(name))
    if name == "lengths":                   # 300 entries: one row across five 64-entry tiles
        return _csr_of_lengths([0, 1, 63, 64, 65, 300, 0, 2], N_COLS, rng)
    return _csr_of_lengths(rng.integers(0, 4, 20000).tolist(), N_COLS, rng)      # 20,000 short rows: the grid


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _scale(mode, n_rows, n_cols, rng):
    if mode == "none":
        return None, 0
    axis = 1 if mode == "row" else 0
    return rng.uniform(0.5, 1.5, n_rows if axis else n_cols).astype(np.float32), axis


# ---- srg_spmm_scaled_f32 ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "col", "row"])
@pytest.mark.parametrize("d", DIMS)
def test_spmm_scaled_is_the_restated_chain(d, mode):
    from srgnn.sparse import spmm_scatter
    from srgnn.wavelet_conv import spmm_scaled
    ip, ix, v = _ladder_csr()
    rng = np.random.default_rng(100 + d)
    X = rng.standard_normal((N_COLS, d)).astype(np.float32)
    scale, axis = _scale(mode, ip.size - 1, N_COLS, rng)
    tip, tix, tv, tX, ts = _dev(ip, ix, v, X, scale)
    got = spmm_scaled(tip, tix, tv, tX, scale=ts, scale_axis=axis)
    assert got.shape == (ip.size - 1, d) and got.dtype == torch.float32 and got.is_cuda
    assert_bits(got.cpu().numpy(), W.spmm_scaled_ref(ip, ix, v, scale, axis, X), f"d={d} {mode}")
    if mode == "none":                      # the bits of the kernel it stands in for, on the device
        assert torch.equal(got.view(torch.int32), spmm_scatter(tip, tix, tv, tX).view(torch.int32))


@pytest.mark.parametrize("mode", ["none", "col", "row"])
def test_spmm_scaled_one_by_one_operator(mode):
    from srgnn.wavelet_conv import spmm_scaled
    ip, ix, v = np.array([0, 1], np.int64), np.array([0], np.int32), np.array([1.5], np.float32)
    X = np.array([[-2.25]], np.float32)
    scale, axis = _scale(mode, 1, 1, np.random.default_rng(1))
    tip, tix, tv, tX, ts = _dev(ip, ix, v, X, scale)
    got = spmm_scaled(tip, tix, tv, tX, scale=ts, scale_axis=axis)
    assert_bits(got.cpu().numpy(), W.spmm_scaled_ref(ip, ix, v, scale, axis, X))


@pytest.mark.parametrize("aligned", [False, True], ids=["4-byte aligned", "16-byte aligned"])
@pytest.mark.parametrize("d", [4, 16, 33])
def test_spmm_scaled_column_windows_and_a_canary_around_y(d, aligned):
    """X and Y are column windows of wider panels (first column 1 and an odd row stride, or first
    column 4 and a row stride that is a multiple of 4); Y's other cells keep their canary."""
    from srgnn.wavelet_conv import spmm_scaled
    first, extra = (4, 8 + (-d) % 4) if aligned else (1, 3)
    ip, ix, v = _ladder_csr()
    m = ip.size - 1
    rng = np.random.default_rng(1000 * d + first)
    Xw = rng.standard_normal((N_COLS, d + extra)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, N_COLS).astype(np.float32)
    tip, tix, tv, tXw, ts = _dev(ip, ix, v, Xw, scale)
    Yw = torch.full((m, d + extra), -12345.0, device="cuda")
    tX, tY = tXw[:, first:first + d], Yw[:, first:first + d]
    assert tX.stride(0) == d + extra and tX.data_ptr() % 16 == (4 * first) % 16
    got = spmm_scaled(tip, tix, tv, tX, scale=ts, scale_axis=0, out=tY)
    assert got.data_ptr() == tY.data_ptr()
    host = Yw.cpu().numpy()
    assert_bits(host[:, first:first + d], W.spmm_scaled_ref(ip, ix, v, scale, 0, Xw[:, first:first + d]))
    assert (host[:, :first] == -12345.0).all() and (host[:, first + d:] == -12345.0).all()


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, 2.0 ** -100, -2.0 ** -120], dtype=np.float32)


def _sprinkle(rng, *arrays):
    for a in arrays:
        hit = rng.random(a.shape) < 0.01
        a[hit] = rng.choice(SPECIALS, int(hit.sum()))


@pytest.mark.parametrize("mode", ["col", "row"])
@pytest.mark.parametrize("d", [7, 16])
def test_spmm_scaled_special_values_follow_ieee(d, mode):
    """NaN, +-Inf, -0, subnormals and scale = 0 in values, scale and panel: NaN where the restatement has
    NaN, every other result bitwise (a subnormal rescaled value is not flushed, 0 * Inf is NaN)."""
    from srgnn.wavelet_conv import spmm_scaled
    ip, ix, v = _ladder_csr()
    v = v.copy()
    rng = np.random.default_rng(7 + d)
    X = rng.standard_normal((N_COLS, d)).astype(np.float32)
    scale, axis = _scale(mode, ip.size - 1, N_COLS, rng)
    _sprinkle(rng, v, X, scale)
    scale[::7] = 0.0
    v[5], scale[ix[5] if axis == 0 else csr_rows(ip)[5]] = 2.0 ** -100, 2.0 ** -40    # a subnormal rescaled value
    want = W.spmm_scaled_ref(ip, ix, v, scale, axis, X)
    assert np.isnan(want).any() and not np.isnan(want).all()
    tip, tix, tv, tX, ts = _dev(ip, ix, v, X, scale)
    assert_bits(spmm_scaled(tip, tix, tv, tX, scale=ts, scale_axis=axis).cpu().numpy(), want)


# ---- srg_sddmm_rowsum_f32 -----------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("d", DIMS)
def test_rowsum_is_the_restated_chain(d, aligned):
    """Rows of 0, 1, 63, 64, 65 and 300 entries; G and P whole panels (16-byte aligned) or column windows
    from column 1 (4-byte aligned); out inside a canary buffer."""
    from srgnn.wavelet_conv import sddmm_rowsum
    ip, ix, v = _rowsum_csr("lengths")
    m = ip.size - 1
    rng = np.random.default_rng(200 + d)
    first, extra = (0, 0) if aligned else (1, 3)
    Gw = rng.standard_normal((N_COLS, d + extra)).astype(np.float32)
    Pw = rng.standard_normal((m, d + extra)).astype(np.float32)
    tip, tix, tv, tGw, tPw = _dev(ip, ix, v, Gw, Pw)
    buf = torch.full((m + 23,), -12345.0, device="cuda")
    got = sddmm_rowsum(tip, tix, tv, tGw[:, first:first + d], tPw[:, first:first + d], out=buf[11:11 + m])
    host = buf.cpu().numpy()
    assert got.data_ptr() == buf[11:].data_ptr()
    assert_bits(host[11:11 + m], W.sddmm_rowsum_ref(ip, ix, v, Gw[:, first:first + d], Pw[:, first:first + d]))
    assert (host[:11] == -12345.0).all() and (host[11 + m:] == -12345.0).all()
    assert host[11] == 0 and not np.signbit(host[11])                      # the empty row: +0


@pytest.mark.parametrize("d", [7, 16])
def test_rowsum_over_twenty_thousand_short_rows(d):
    from srgnn.wavelet_conv import sddmm_rowsum
    ip, ix, v = _rowsum_csr("short")
    rng = np.random.default_rng(300 + d)
    G = rng.standard_normal((N_COLS, d)).astype(np.float32)
    P = rng.standard_normal((ip.size - 1, d)).astype(np.float32)
    got = sddmm_rowsum(*_dev(ip, ix, v, G, P))
    assert_bits(got.cpu().numpy(), W.sddmm_rowsum_ref(ip, ix, v, G, P))


def test_rowsum_zero_width_gives_plus_zero():
    from srgnn.wavelet_conv import sddmm_rowsum
    ip, ix, v = _rowsum_csr("lengths")
    m = ip.size - 1
    tip, tix, tv = _dev(ip, ix, v)
    out = torch.full((m,), 7.0, device="cuda")
    sddmm_rowsum(tip, tix, tv, torch.empty(N_COLS, 0, device="cuda"), torch.empty(m, 0, device="cuda"), out=out)
    assert not out.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("d", [7, 33])
def test_rowsum_special_values_follow_ieee(d):
    from srgnn.wavelet_conv import sddmm_rowsum
    ip, ix, v = _rowsum_csr("lengths")
    v = v.copy()
    rng = np.random.default_rng(17 + d)
    G = rng.standard_normal((N_COLS, d)).astype(np.float32)
    P = rng.standard_normal((ip.size - 1, d)).astype(np.float32)
    _sprinkle(rng, v, G)
    P[2, 0] = 0.0
    P[4, d - 1] = 1e-40
    want = W.sddmm_rowsum_ref(ip, ix, v, G, P)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert_bits(sddmm_rowsum(*_dev(ip, ix, v, G, P)).cpu().numpy(), want)


# ---- wavelet_conv end to end ----------------------------------------------------------------------------

def _fixture(name):
    z = np.load(os.path.join(REPO, "tests", "golden", f"{name}.npz"), allow_pickle=False)
    return [(z[f"phi{i}_indptr"].astype(np.int64), z[f"phi{i}_indices"].astype(np.int32),
             z[f"phi{i}_data"].astype(np.float32)) for i in (0, 1)]


def _random_basis(n, density, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        M = sp.random(n, n, density=density, format="csr", random_state=rng, dtype=np.float32)
        M.data = (rng.random(M.nnz) + 0.5).astype(np.float32)
        M.sort_indices()
        out.append((M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data))
    return out


@functools.lru_cache(maxsize=None)
def _basis(name):
    """(phi csr, phi^-1 csr), both coalesced: column-sorted rows, unique (row, column)."""
    return _random_basis(2000, 0.01, 2000) if name == "rand2000" else _fixture(name)


def _coo(csr):
    ip, ix, v = csr
    return torch.from_numpy(np.stack([csr_rows(ip), ix.astype(np.int64)])), torch.from_numpy(v.copy())


def _operands(name, d, seed):
    phi, phi_inv = _basis(name)
    n = phi[0].size - 1
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.9, 1.1, n).astype(np.float32)
    Z = rng.standard_normal((n, d)).astype(np.float32)
    G = rng.standard_normal((n, d)).astype(np.float32)
    return phi, phi_inv, n, theta, Z, G


def _fused(phi, phi_inv, n, theta, Z, G, device="cpu", need=(True, True)):
    from srgnn.wavelet_conv import WaveletOperator, wavelet_conv
    (pi, pv), (qi, qv) = _coo(phi), _coo(phi_inv)
    op = WaveletOperator(pi.to(device), pv.to(device), qi.to(device), qv.to(device), n)
    th = torch.from_numpy(theta).to(device).view(n, 1).requires_grad_(need[0])
    z = torch.from_numpy(Z).to(device).requires_grad_(need[1])
    y = wavelet_conv(op, th, z)
    y.backward(torch.from_numpy(G).to(device))
    return y, th, z


@pytest.mark.parametrize("name,d", [("wav_rand", 16), ("wav_rand", 7), ("wav_cora", 16), ("rand2000", 7)])
def test_wavelet_conv_is_the_restatement_and_the_shims_reassociated_composition(name, d):
    """Y, gZ and gtheta are bit for bit the restatement and bit for bit
    spmm(*spspmm(phi, diag theta), n, n, spmm(phi^-1, n, n, Z)) with its autograd (coalesced phi, theta
    in [0.9, 1.1]: no rescaled value is an exact zero)."""
    import torch_sparse
    phi, phi_inv, n, theta, Z, G = _operands(name, d, 11 + d)
    y, th, z = _fused(phi, phi_inv, n, theta, Z, G)
    assert y.device.type == "cpu" and th.grad.shape == (n, 1) and z.grad.shape == (n, d)
    wy, wP = W.forward_ref(phi, phi_inv, theta, Z)
    _, wgz, wgt = W.backward_ref(phi, phi_inv, theta, wP, G)
    assert_bits(y.detach().numpy(), wy, "Y")
    assert_bits(z.grad.numpy(), wgz, "gZ")
    assert_bits(th.grad.numpy().reshape(-1), wgt, "gtheta")
    (pi, pv), (qi, qv) = _coo(phi), _coo(phi_inv)
    th2 = torch.from_numpy(theta).requires_grad_(True)
    z2 = torch.from_numpy(Z).requires_grad_(True)
    ri, rv = torch_sparse.spspmm(pi, pv, torch.arange(n).repeat(2, 1), th2, n, n, n)
    y2 = torch_sparse.spmm(ri, rv, n, n, torch_sparse.spmm(qi, qv, n, n, z2))
    y2.backward(torch.from_numpy(G))
    assert_bits(y.detach().numpy(), y2.detach().numpy(), "Y against the shims")
    assert_bits(z.grad.numpy(), z2.grad.numpy(), "gZ against the shims")
    assert_bits(th.grad.numpy().reshape(-1), th2.grad.numpy(), "gtheta against the shims")


def test_wavelet_conv_is_within_the_derived_bound_of_the_reference_call_order():
    """The shims' chain in the reference's order, spmm(spspmm(spspmm(phi, diag theta), phi^-1), Z), on
    wav_rand (La, Lb, Lc the longest rows of phi, phi^-1 and of the product, Ma, Mb, Mc
    their longest columns):
      |Y - Y_ref|           <= (gamma_{La+Lb+1} + gamma_{La+Lc+1}) S
      |gZ - gZ_ref|         <= (gamma_{Ma+Mb+1} + gamma_{La+Mc+1}) Sz
      |gtheta - gtheta_ref| <= 2 gamma_{Ma+Lb+d} St
    with S, Sz, St the sums of the absolute values of the terms, in fp64."""
    import torch_sparse
    d = 16
    phi, phi_inv, n, theta, Z, G = _operands("wav_rand", d, 5)
    y, th, z = _fused(phi, phi_inv, n, theta, Z, G)
    (pi, pv), (qi, qv) = _coo(phi), _coo(phi_inv)
    th2 = torch.from_numpy(theta).requires_grad_(True)
    z2 = torch.from_numpy(Z).requires_grad_(True)
    ri, rv = torch_sparse.spspmm(pi, pv, torch.arange(n).repeat(2, 1), th2, n, n, n)
    ci, cv = torch_sparse.spspmm(ri, rv, qi, qv, n, n, n)
    y2 = torch_sparse.spmm(ci, cv, n, n, z2)
    y2.backward(torch.from_numpy(G))
    A, B = np.abs(W.dense64(phi, n)), np.abs(W.dense64(phi_inv, n))
    T, aZ, aG = np.abs(theta.astype(np.float64)), np.abs(Z.astype(np.float64)), np.abs(G.astype(np.float64))
    La, Lb = W.longest_row(phi[0]), W.longest_row(phi_inv[0])
    Ma, Mb = int(np.bincount(phi[1], minlength=n).max()), int(np.bincount(phi_inv[1], minlength=n).max())
    Lc, Mc = int(np.bincount(ci[0].numpy(), minlength=n).max()), int(np.bincount(ci[1].numpy(), minlength=n).max())
    S = (A * T) @ (B @ aZ)
    Sz = B.T @ ((A * T).T @ aG)
    St = (A * (aG @ (B @ aZ).T)).sum(axis=0)
    g = W.gamma
    for what, got, ref, bound in (
            ("Y", y.detach(), y2.detach(), (g(La + Lb + 1) + g(La + Lc + 1)) * S),
            ("gZ", z.grad, z2.grad, (g(Ma + Mb + 1) + g(La + Mc + 1)) * Sz),
            ("gtheta", th.grad.reshape(-1), th2.grad, 2 * g(Ma + Lb + d) * St)):
        diff = np.abs(got.numpy().astype(np.float64) - ref.numpy().astype(np.float64))
        ratio = float((diff / bound).max())
        print(f"{what}: max |fused - reference order| / bound = {ratio:.4f}")
        assert ratio <= 1.0, what


def test_device_inputs_give_the_host_inputs_bits_on_the_device():
    ops = _operands("wav_rand", 7, 3)
    y, th, z = _fused(*ops)
    yd, thd, zd = _fused(*ops, device="cuda")
    assert yd.is_cuda and thd.grad.is_cuda and zd.grad.is_cuda
    for a, b in ((y, yd), (th.grad, thd.grad), (z.grad, zd.grad)):
        assert_bits(a.detach().numpy(), b.detach().cpu().numpy())


@pytest.mark.parametrize("side", ["theta", "Z"])
def test_only_the_side_that_requires_grad_is_computed(side, monkeypatch):
    import srgnn.wavelet_conv as WC
    calls = {"spmm_scaled": 0, "sddmm_rowsum": 0}
    for name in calls:
        def counted(*a, _f=getattr(WC, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(WC, name, counted)
    y, th, z = _fused(*_operands("wav_rand", 7, 4), need=(side == "theta", side == "Z"))
    if side == "theta":
        assert calls == {"spmm_scaled": 2, "sddmm_rowsum": 1} and z.grad is None and th.grad is not None
    else:
        assert calls == {"spmm_scaled": 4, "sddmm_rowsum": 0} and th.grad is None and z.grad is not None


def test_same_bits_twice_and_under_another_stream():
    ops = _operands("wav_rand", 16, 6)
    a = _fused(*ops, device="cuda")
    b = _fused(*ops, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _fused(*ops, device="cuda")
    side.synchronize()
    for other in (b, c):
        for x, y in zip((a[0], a[1].grad, a[2].grad), (other[0], other[1].grad, other[2].grad)):
            assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))


def test_input_checks():
    from srgnn.wavelet_conv import WaveletOperator, wavelet_conv
    phi, phi_inv, n, theta, Z, _ = _operands("wav_rand", 4, 9)
    (pi, pv), (qi, qv) = _coo(phi), _coo(phi_inv)
    op = WaveletOperator(pi, pv, qi, qv, n)
    with pytest.raises(TypeError):
        wavelet_conv(op, torch.from_numpy(theta).double(), torch.from_numpy(Z))
    with pytest.raises(TypeError):
        wavelet_conv(op, torch.from_numpy(theta), torch.from_numpy(Z).double())
    with pytest.raises(ValueError):
        WaveletOperator(pi, pv.clone().requires_grad_(True), qi, qv, n)
    bad = pi.clone()
    bad[1, 3] = n
    with pytest.raises(ValueError):
        WaveletOperator(bad, pv, qi, qv, n)
    with pytest.raises(ValueError):
        wavelet_conv(op, torch.from_numpy(theta[:-1].copy()), torch.from_numpy(Z))


# ---- training ---------------------------------------------------------------------------------------------

def test_three_adam_steps_of_the_wavelet_network_on_wavelet_conv():
    """The sparse-then-dense wavelet network on wav_rand with both layers on wavelet_conv, against fp64
    dense CPU autograd of the same network: the structure and the tolerance of
    tests/test_spspmm_grad_gpu.py's training test (max |g - g64| <= 1e-4 max |g64| at step 1, the loss
    finite at every step)."""
    import torch_sparse
    from srgnn.wavelet_conv import WaveletOperator, wavelet_conv
    z = np.load(os.path.join(REPO, "tests", "golden", "wav_rand.npz"), allow_pickle=False)
    phi, phi_inv = _basis("wav_rand")
    n, x = phi[0].size - 1, z["x"]
    filters, classes = 16, 4
    gen = torch.Generator().manual_seed(7)
    labels = torch.randint(0, classes, (n,), generator=gen)
    xavier = lambda i, o: torch.empty(i, o).uniform_(-(6.0 / (i + o)) ** 0.5, (6.0 / (i + o)) ** 0.5, generator=gen)
    w1, w2 = xavier(x.shape[1], filters), xavier(filters, classes)
    t1 = torch.empty(n, 1).uniform_(0.9, 1.1, generator=gen)
    t2 = torch.empty(n, 1).uniform_(0.9, 1.1, generator=gen)
    fr, fc = x.nonzero()
    feat = (torch.from_numpy(np.vstack([fr, fc])), torch.from_numpy(x[fr, fc]))

    P0 = torch.from_numpy(W.dense64(phi, n))
    P1 = torch.from_numpy(W.dense64(phi_inv, n))
    X64 = torch.from_numpy(x.astype(np.float64))

    def net64(a, ta, b, tb):
        h = torch.relu((P0 * ta.view(1, -1)) @ P1 @ (X64 @ a))
        return torch.nn.functional.log_softmax((P0 * tb.view(1, -1)) @ P1 @ (h @ b), dim=1)
    p64 = [p.double().requires_grad_(True) for p in (w1, t1, w2, t2)]
    loss64 = torch.nn.functional.nll_loss(net64(*p64), labels)
    loss64.backward()

    op = WaveletOperator(*_coo(phi), *_coo(phi_inv), n)

    def net(a, ta, b, tb):
        filtered = torch_sparse.spmm(feat[0], feat[1], n, a.shape[0], a)
        h = torch.nn.functional.dropout(torch.relu(wavelet_conv(op, ta, filtered)), training=True, p=0.0)
        return torch.nn.functional.log_softmax(wavelet_conv(op, tb, torch.mm(h, b)), dim=1)
    params = [p.clone().requires_grad_(True) for p in (w1, t1, w2, t2)]
    opt = torch.optim.Adam(params, lr=0.01)
    for step in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(net(*params), labels)
        assert torch.isfinite(loss), (step, loss)
        loss.backward()
        if step == 0:
            assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item())
            for name, p, q in zip(("W1", "theta1", "W2", "theta2"), params, p64):
                g, g64 = p.grad.double(), q.grad
                assert g.shape == p.shape and bool(torch.isfinite(g).all()) and bool((g != 0).any()), name
                assert float((g - g64).abs().max()) <= 1e-4 * float(g64.abs().max()), name
        opt.step()


# ---- memory -------------------------------------------------------------------------------------------------

def test_forward_and_backward_hold_panels_only():
    """n = 4096, 2 % bases, d = 16, device tensors: the peak above the operands (the operator, theta, Z and
    G) is at most Y, P, gP, gZ, one spare panel and gtheta -- 5 n d 4 + n 4 bytes plus the allocator's
    512-byte rounding per tensor -- so nothing of size nnz (335,544 entries per basis) is held."""
    from srgnn.wavelet_conv import WaveletOperator, wavelet_conv
    n, d = 4096, 16
    phi, phi_inv = _random_basis(n, 0.02, 4096)
    op = WaveletOperator(*(t.cuda() for t in _coo(phi)), *(t.cuda() for t in _coo(phi_inv)), n)
    gen = torch.Generator(device="cuda").manual_seed(3)
    theta = (torch.rand(n, device="cuda", generator=gen) * 0.2 + 0.9).requires_grad_(True)
    Z = torch.randn(n, d, device="cuda", generator=gen).requires_grad_(True)
    G = torch.randn(n, d, device="cuda", generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = wavelet_conv(op, theta, Z)
    y.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = 5 * n * d * 4 + n * 4 + 6 * 512
    print(f"peak above the operands: {peak} bytes, limit {limit}, one basis' values {4 * phi[2].size}")
    assert peak <= limit
    assert theta.grad.shape == (n,) and Z.grad.shape == (n, d)


# ---- the C entries on raw pointers ----------------------------------------------------------------------------

def test_c_entries_on_raw_device_pointers():
    from srgnn import _lib
    L = _lib.lib()
    ip, ix, v = _ladder_csr()
    m, d, ld = ip.size - 1, 22, 23
    rng = np.random.default_rng(23)
    Xw = rng.standard_normal((N_COLS, ld)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, N_COLS).astype(np.float32)
    tip, tix, tv, tXw, ts = _dev(ip, ix, v, Xw, scale)
    Y = torch.full((m, ld), -1.0, device="cuda")
    torch.cuda.synchronize()
    rc = L.srg_spmm_scaled_f32(tip.data_ptr(), tix.data_ptr(), tv.data_ptr(), ts.data_ptr(), 0, m,
                               tXw.data_ptr() + 4, ld, Y.data_ptr() + 4, ld, d, None)
    assert rc == _lib.SRG_OK, _lib.last_error()
    torch.cuda.synchronize()
    host = Y.cpu().numpy()
    assert_bits(host[:, 1:1 + d], W.spmm_scaled_ref(ip, ix, v, scale, 0, Xw[:, 1:1 + d]))
    assert (host[:, 0] == -1.0).all()

    ip, ix, v = _rowsum_csr("lengths")
    m = ip.size - 1
    Pw = rng.standard_normal((m, ld)).astype(np.float32)
    tip, tix, tv, tPw = _dev(ip, ix, v, Pw)
    out = torch.full((m,), -1.0, device="cuda")
    torch.cuda.synchronize()
    rc = L.srg_sddmm_rowsum_f32(tip.data_ptr(), tix.data_ptr(), tv.data_ptr(), m, tXw.data_ptr() + 4, ld,
                                tPw.data_ptr() + 4, ld, d, out.data_ptr(), None)
    assert rc == _lib.SRG_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert_bits(out.cpu().numpy(), W.sddmm_rowsum_ref(ip, ix, v, Xw[:, 1:1 + d], Pw[:, 1:1 + d]))
