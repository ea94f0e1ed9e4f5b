"""srgnn.gat on the GPU: the fused aggregation within the first-order bound of the fp64 restatement
(tests/gat_ref.py), bit for bit where the bits are pinned, deterministic across runs, load paths and head
counts, indifferent to what other rows hold, safe on bad ids, across the launch chunk, inside GATConv and GAT,
and without a per-edge [nnz, H, C] temporary."""
import numpy as np
import pytest
import torch

import gat_ref as R
from srgnn import _lib
from srgnn import gat as GT

pytestmark = pytest.mark.gpu

CASES = [(k, sl, H, C) for k in R.GRAPHS for sl in (False, True) for (H, C) in R.SHAPES]
_graphs, _refs = {}, {}


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32)


def host(x):
    return x.detach().cpu().numpy()


def device_graph(kind, sl):
    """The GATGraph of a base graph on the device, built once from the edge list."""
    if (kind, sl) not in _graphs:
        dst, src = R.base_edges(kind)
        g = GT.GATGraph.from_edge_index(np.stack([src, dst]), R.N, add_self_loops=sl, device=dev())
        ip, ix = R.graph(kind, sl)
        assert np.array_equal(host(g.indptr), ip) and np.array_equal(host(g.indices), ix)
        _graphs[(kind, sl)] = g
    return _graphs[(kind, sl)]


def reference(kind, sl, H, C):
    key = (kind, sl, H, C)
    if key not in _refs:
        ip, ix = R.graph(kind, sl)
        Hf, a_src, a_dst, G = R.inputs(R.N, H, C, R.case_seed(kind, sl, H, C))
        _refs[key] = (ip, ix, (Hf, a_src, a_dst, G), R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G))
    return _refs[key]


def run(g, Hf, a_src, a_dst, G, slope=0.2):
    """Everything the three entries return, as host arrays, through the autograd function."""
    x, s, d = (v.clone().requires_grad_(True) for v in (Hf, a_src, a_dst))
    out = GT.gat_attend(g, x, s, d, slope)
    out.backward(G)
    _, M, Z = GT.attend_forward(g, Hf, a_src, a_dst, slope)
    return dict(out=host(out), M=host(M), Z=host(Z), dHf=host(x.grad), da_src=host(s.grad), da_dst=host(d.grad))


@pytest.mark.parametrize("kind,sl,H,C", CASES)
def test_within_the_bound(kind, sl, H, C):
    ip, ix, (Hf, a_src, a_dst, G), ref = reference(kind, sl, H, C)
    assert ref["band"] == 0
    got = run(device_graph(kind, sl), t(Hf), t(a_src), t(a_dst), t(G))
    R.check(f"device {kind} loops={sl} H={H} C={C}", ref, got)
    if not sl:                      # the isolated nodes have empty rows: +0 with the sign bit clear, Z = 0,
        iso = list(R.ISOLATED)      # and nothing from them reaches a gradient
        assert not bits(got["out"][iso]).any() and not bits(got["Z"][iso]).any() and not bits(got["M"][iso]).any()
        assert not bits(got["da_dst"][iso]).any() and not bits(got["da_src"][iso]).any()
        assert not bits(got["dHf"][iso]).any()


# ---- pinned bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", ((1, 47), (4, 64), (2, 65)))
def test_one_entry_per_row_returns_hf(H, C):
    n = 300
    g = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), n, add_self_loops=True, device=dev())
    Hf, a_src, a_dst, _ = R.inputs(n, H, C, 40 + C)
    Hf[5, 0] = -0.0
    out, M, Z = GT.attend_forward(g, t(Hf), t(a_src), t(a_dst))
    assert np.array_equal(bits(out), bits(R.single_entry_ref(np.arange(n), Hf)))
    assert (host(Z) == 1.0).all()


@pytest.mark.parametrize("kind,sl", (("asym", False), ("sym", True)))
@pytest.mark.parametrize("H,C", ((1, 47), (3, 7), (4, 64), (1, 260)))
def test_zero_attention_is_the_sequential_mean(kind, sl, H, C):
    """Pins the chain's order: the sequential fp32 sum of the row's source rows in stored order, over len."""
    ip, ix = R.graph(kind, sl)
    Hf = R.inputs(R.N, H, C, 50 + C)[0]
    zero = torch.zeros((R.N, H), device=dev())
    out, M, Z = GT.attend_forward(device_graph(kind, sl), t(Hf), zero, zero)
    assert np.array_equal(bits(out), bits(R.zero_att_ref(ip, ix, Hf)))
    assert np.array_equal(host(Z), np.repeat(np.diff(ip).astype(np.float32)[:, None], H, axis=1))


def test_zero_score_takes_the_slope_on_the_device():
    """s = 0 exactly on every entry: the derivative is `slope` (torch's leaky_relu), here against the fp64
    restatement's values with its bound (the band is the whole graph, and it is the convention under test)."""
    ip, ix = R.graph("asym", True)
    H, C = 2, 5
    Hf, _, _, G = R.inputs(R.N, H, C, 9)
    zero = np.zeros((R.N, H), dtype=np.float32)
    ref = R.evaluate(ip, ix, Hf, zero, zero, 0.2, G)
    got = run(device_graph("asym", True), t(Hf), t(zero), t(zero), t(G))
    R.check("zero scores", ref, {k: got[k] for k in ("da_src", "da_dst")})
    wrong = R.evaluate(ip, ix, Hf, zero, zero, 0.2, G, mistake="derivative_one")
    assert R.worst_ratio(got["da_src"], wrong["da_src"], wrong["E_da_src"]) >= 50


# ---- determinism ------------------------------------------------------------------------------------
def test_run_to_run_identical():
    ip, ix, (Hf, a_src, a_dst, G), _ = reference("sym", True, 8, 16)
    g = device_graph("sym", True)
    args = (t(Hf), t(a_src), t(a_dst), t(G))
    first = run(g, *args)
    for _ in range(2):
        again = run(g, *args)
        for k in first:
            assert np.array_equal(bits(again[k]), bits(first[k])), k


@pytest.mark.parametrize("H,C", ((4, 64), (8, 16), (1, 260)))
def test_strided_windows_take_the_4_byte_path(H, C):
    """Contiguous panels of a width that is a multiple of 4 take 16-byte loads; the same columns as a window
    at an odd offset of a wider panel cannot.  The same bits."""
    ip, ix, (Hf, a_src, a_dst, G), _ = reference("sym", True, 4, 64) if (H, C) == (4, 64) else \
        (*R.graph("sym", True), R.inputs(R.N, H, C, 60 + C), None)
    g = device_graph("sym", True)
    W = H * C
    wide_h = torch.zeros((R.N, W + 3), device=dev())
    wide_h[:, 1:W + 1] = t(Hf)
    wide_g = torch.zeros((R.N, W + 7), device=dev())
    wide_g[:, 3:W + 3] = t(G)
    a = run(g, t(Hf), t(a_src), t(a_dst), t(G))
    b = run(g, wide_h[:, 1:W + 1], t(a_src), t(a_dst), wide_g[:, 3:W + 3])
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("kind,sl", (("asym", False), ("sym", True)))
def test_heads_are_independent(kind, sl):
    """Head h of an H-head call has the bits of a one-head call on that head's columns, forward and backward."""
    H, C = 3, 7
    ip, ix, (Hf, a_src, a_dst, G), _ = reference(kind, sl, H, C)
    g = device_graph(kind, sl)
    full = run(g, t(Hf), t(a_src), t(a_dst), t(G))
    for h in range(H):
        cols = slice(h * C, (h + 1) * C)
        one = run(g, t(Hf)[:, cols], t(a_src[:, h:h + 1]), t(a_dst[:, h:h + 1]), t(G)[:, cols])
        for k in ("out", "dHf"):
            assert np.array_equal(bits(one[k]), bits(full[k][:, cols])), (k, h)
        for k in ("M", "Z", "da_src", "da_dst"):
            assert np.array_equal(bits(one[k]), bits(full[k][:, h:h + 1])), (k, h)
    # and with 16-byte loads on both sides
    H, C = 4, 64
    ip, ix, (Hf, a_src, a_dst, G), _ = reference(kind, sl, H, C)
    full = run(g, t(Hf), t(a_src), t(a_dst), t(G))
    cols = slice(2 * C, 3 * C)
    one = run(g, t(Hf[:, cols]), t(a_src[:, 2:3]), t(a_dst[:, 2:3]), t(G[:, cols]))
    for k in ("out", "dHf"):
        assert np.array_equal(bits(one[k]), bits(full[k][:, cols])), k
    for k in ("M", "Z", "da_src", "da_dst"):
        assert np.array_equal(bits(one[k]), bits(full[k][:, 2:3])), k


# ---- rows do not reach each other -------------------------------------------------------------------
@pytest.mark.parametrize("bad", (np.nan, np.inf))
def test_a_non_finite_row_reaches_its_targets_only(bad):
    kind, sl, H, C = "asym", True, 3, 7
    ip, ix, (Hf, a_src, a_dst, G), _ = reference(kind, sl, H, C)
    g = device_graph(kind, sl)
    node = 30
    rows = R.entry_rows(ip)
    targets = np.unique(rows[ix == node])
    assert 0 < targets.size < R.N - 1
    others = np.setdiff1d(np.arange(R.N), targets)
    clean, _, _ = GT.attend_forward(g, t(Hf), t(a_src), t(a_dst))
    dirty_h = Hf.copy()
    dirty_h[node] = bad
    out, _, _ = GT.attend_forward(g, t(dirty_h), t(a_src), t(a_dst))
    assert np.array_equal(bits(out[t(others)]), bits(clean[t(others)]))
    # by class against the restatement: alpha > 0 on every entry here, so a target of the node is NaN or Inf
    # exactly where fp64 says so
    import hop_attention_ref as HR
    with np.errstate(invalid="ignore", over="ignore"):
        want = R.evaluate(ip, ix, dirty_h, a_src, a_dst)["out"]
    assert np.array_equal(HR.classes(host(out)[targets]), HR.classes(want[targets]))
    assert (HR.classes(want[targets]) != HR.FINITE).any()
    # a NaN in G outside the node's targets does not reach the node's dHf
    sources_of_node = np.unique(rows[ix == node])          # the rows of G that dHf[node] reads
    far = np.setdiff1d(np.arange(R.N), sources_of_node)
    dirty_g = G.copy()
    dirty_g[far[:5]] = np.nan
    a = GT.attend_backward(g, t(Hf), t(a_src), t(a_dst), clean, *GT.attend_forward(g, t(Hf), t(a_src), t(a_dst))[1:],
                           t(G), need=(True, False, False))[0]
    b = GT.attend_backward(g, t(Hf), t(a_src), t(a_dst), clean, *GT.attend_forward(g, t(Hf), t(a_src), t(a_dst))[1:],
                           t(dirty_g), need=(True, False, False))[0]
    assert np.array_equal(bits(a[node]), bits(b[node])) and np.isfinite(host(a[node])).all()


def test_saturated_scores_give_exact_zeros():
    """Scores scaled until l_e - m < -104 for some entries of a row: their alpha is exactly 0, nothing is NaN,
    and the results stay within the bound plus expf's subnormal range, len * 2^-150 * |x| per element."""
    kind, sl, H, C = "sym", True, 3, 7
    ip, ix = R.graph(kind, sl)
    Hf, a_src, a_dst, G = R.inputs(R.N, H, C, 77, scale=60.0)
    ref = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G)
    assert ref["band"] == 0
    rows = R.entry_rows(ip)
    s = ref["s"]
    l = np.where(s > 0, s, 0.2 * s)
    gap = l - ref["M"][rows]
    assert (gap < -104).any() and (gap > -80).any()
    g = device_graph(kind, sl)
    got = run(g, t(Hf), t(a_src), t(a_dst), t(G))
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    ln = np.diff(ip).astype(np.float64)[:, None]
    absx = np.abs(Hf.astype(np.float64))
    allow = dict(ref)
    # p in expf's subnormal range is off by up to 2^-150 absolutely instead of 2 eps relatively
    allow["E_out"] = ref["E_out"] + ln * R.TINY * absx.max()
    allow["E_Z"] = ref["E_Z"] + ln * R.TINY
    R.check("saturated forward", allow, {k: got[k] for k in R.FORWARD})
    # alpha is exactly 0 where the gap is past the subnormals: dHf of a source whose every edge is saturated
    tp, tx, perm = R.transpose_of(ip, ix, R.N)
    dead = np.ones((R.N, H), bool)
    np.logical_and.at(dead, ix, gap < -104)
    dead &= (np.diff(tp) > 0)[:, None]
    assert dead.any()
    dh = got["dHf"].reshape(R.N, H, C)
    assert not bits(dh[dead]).any()


# ---- ids --------------------------------------------------------------------------------------------
def test_out_of_range_ids_are_skipped():
    """-1 and n given straight to the C entries: skipped, never read.  The results are those of the graph
    without the bad entries, bit for bit (a skipped entry moves no other term of a row sum: see the order)."""
    kind, sl, H, C = "asym", True, 3, 7
    ip, ix, (Hf, a_src, a_dst, G), _ = reference(kind, sl, H, C)
    n, nnz = R.N, ix.size
    bad = ix.copy()
    hit = np.zeros(nnz, bool)
    hit[[ip[R.STAR] + 3, ip[R.STAR] + 70, ip[20], ip[50 + 1] - 1]] = True
    bad[hit] = [-1, n, n, -1]
    d = dev()
    f = lambda a: t(a)
    tip, tix, x, s_, d_, g_ = f(ip), f(bad), f(Hf), f(a_src), f(a_dst), f(G)
    W = H * C
    out, M, Z = (torch.full(sh, 9.0, device=d) for sh in ((n, W), (n, H), (n, H)))
    st = _lib.stream(d)
    _lib.call(d, "srg_gat_attend_f32", tip.data_ptr(), tix.data_ptr(), nnz, n, n, s_.data_ptr(), d_.data_ptr(), 0.2,
              x.data_ptr(), W, H, C, out.data_ptr(), W, M.data_ptr(), Z.data_ptr(), st)
    D, dS, da_dst = (torch.full(sh, 9.0, device=d) for sh in ((n, H), (nnz, H), (n, H)))
    _lib.call(d, "srg_gat_edge_grad_f32", tip.data_ptr(), tix.data_ptr(), nnz, n, n, s_.data_ptr(), d_.data_ptr(), 0.2,
              x.data_ptr(), W, H, C, out.data_ptr(), W, M.data_ptr(), Z.data_ptr(), g_.data_ptr(), W, D.data_ptr(),
              dS.data_ptr(), da_dst.data_ptr(), st)
    # the reference: the same rows with the bad entries taken out, through the restatement
    keep = ~hit
    ip2 = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ip2, R.entry_rows(ip)[keep] + 1, 1)
    ip2 = np.cumsum(ip2)
    ref = R.evaluate(ip2, ix[keep], Hf, a_src, a_dst, 0.2, G)
    R.check("bad ids forward", ref, dict(out=host(out), M=host(M), Z=host(Z)))
    R.check("bad ids da_dst", ref, dict(da_dst=host(da_dst)))
    assert not bits(dS[t(np.flatnonzero(hit))]).any()                  # +0 for a skipped entry
    assert R.worst_ratio(host(dS)[keep], ref["ds"], ref["E_ds"]) <= 1.0
    # the adjoint: bad targets in At, and a perm entry out of range
    tp, tx, perm = R.transpose_of(ip, ix, n)
    bad_t = tx.copy()
    hit_t = np.zeros(nnz, bool)
    hit_t[[tp[30], tp[60] + 1, nnz - 1]] = True
    bad_t[hit_t] = [n, -1, n]
    bad_perm = perm.copy()
    bad_perm[hit_t] = [-1, nnz, nnz + 5]
    M2, Z2 = t(ref["M"].astype(np.float32)), t(ref["Z"].astype(np.float32))
    clean_ds = t(np.zeros((nnz, H), dtype=np.float32))
    clean_ds[t(np.flatnonzero(keep))] = t(ref["ds"].astype(np.float32))
    dHf, da_src = torch.full((n, W), 9.0, device=d), torch.full((n, H), 9.0, device=d)
    ttp, ttx, tperm = f(tp), f(bad_t), f(bad_perm)                     # kept alive across the call
    _lib.call(d, "srg_gat_attend_adjoint_f32", ttp.data_ptr(), ttx.data_ptr(), tperm.data_ptr(), nnz, n, n,
              s_.data_ptr(), d_.data_ptr(), 0.2, H, C, M2.data_ptr(), Z2.data_ptr(), g_.data_ptr(), W,
              clean_ds.data_ptr(), dHf.data_ptr(), W, da_src.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.isfinite(host(dHf)).all() and np.isfinite(host(da_src)).all()
    # dHf[j] sums alpha_t G[i_t] over the entries of At that were not hit, with alpha from the (M2, Z2) handed
    # in: restated directly in fp64 with the first-order bound of a len_t-term chain of products
    sel = np.ones(nnz, bool)
    sel[perm[hit_t]] = False
    rows = R.entry_rows(ip)
    sc = a_src.astype(np.float64)[ix[sel]] + a_dst.astype(np.float64)[rows[sel]]
    lk = np.where(sc > 0, sc, 0.2 * sc)
    al = np.exp(lk - M2.cpu().numpy().astype(np.float64)[rows[sel]]) / Z2.cpu().numpy().astype(np.float64)[rows[sel]]
    Gd = G.astype(np.float64).reshape(n, H, C)
    want = np.zeros((n, H, C))
    np.add.at(want, ix[sel], al[:, :, None] * Gd[rows[sel]])
    mag = np.zeros((n, H, C))
    np.add.at(mag, ix[sel], np.abs(al[:, :, None] * Gd[rows[sel]]))
    lt = np.diff(tp).astype(np.float64)[:, None, None]
    # alpha: two adds, the slope product, the subtraction, expf, the divide: (|s| + |l| + |l - M| + 3) eps relative
    r_al = (np.abs(sc) + np.abs(lk) + np.abs(lk - M2.cpu().numpy().astype(np.float64)[rows[sel]]) + 3) * R.EPS
    e_al = np.zeros((n, H, C))
    np.add.at(e_al, ix[sel], (r_al * al)[:, :, None] * np.abs(Gd[rows[sel]]))
    assert R.worst_ratio(host(dHf).reshape(n, H, C), want, e_al + lt * R.EPS * mag) <= 1.0
    # da_src[j]: the row sum of the dS handed in over the entries whose perm is in range
    ds64 = host(clean_ds).astype(np.float64)
    want_s, mag_s = np.zeros((n, H)), np.zeros((n, H))
    np.add.at(want_s, ix[sel], ds64[sel])
    np.add.at(mag_s, ix[sel], np.abs(ds64[sel]))
    assert R.worst_ratio(host(da_src), want_s, lt[:, :, 0] * R.EPS * mag_s) <= 1.0


def test_a_forged_target_with_an_empty_row_adds_nothing():
    """indices_t is not trusted: an entry of At that names a target whose row of A is empty (Z = 0) is left out
    of dHf like an id out of range -- the same bits -- instead of dividing by zero."""
    kind, sl, H, C = "asym", False, 3, 7
    ip, ix, (Hf, a_src, a_dst, G), _ = reference(kind, sl, H, C)
    n, nnz, W = R.N, ix.size, H * C
    g = device_graph(kind, sl)
    x, s_, d_, g_ = t(Hf), t(a_src), t(a_dst), t(G)
    _, M, Z = GT.attend_forward(g, x, s_, d_)
    assert not bits(Z[R.ISOLATED[0]]).any()
    tp, tx, perm = R.transpose_of(ip, ix, n)
    hit = [int(tp[30]), int(tp[R.STAR]) + 2, nnz - 1]
    results = []
    for forged in (R.ISOLATED[0], -1):
        bad = tx.copy()
        bad[hit] = forged
        ttp, ttx = t(tp), t(bad)                                       # kept alive across the call
        dHf = torch.full((n, W), 9.0, device=dev())
        _lib.call(dev(), "srg_gat_attend_adjoint_f32", ttp.data_ptr(), ttx.data_ptr(), None, nnz, n, n, s_.data_ptr(),
                  d_.data_ptr(), 0.2, H, C, M.data_ptr(), Z.data_ptr(), g_.data_ptr(), W, None, dHf.data_ptr(), W, None,
                  _lib.stream(dev()))
        torch.cuda.synchronize()
        results.append(host(dHf))
    assert np.isfinite(results[0]).all()
    assert np.array_equal(bits(results[0]), bits(results[1]))


def test_rows_past_one_launch():
    """n_rows just past SRG_GAT_LAUNCH_ROWS at H = C = 1, rows of one or two entries: every kernel of the three
    entries goes out in two launches.  Checked exactly where the arithmetic is exact: zero scores, Hf of small
    integers, so out is a mean of one or two integers and every gradient a short sum of dyadic numbers."""
    n = _lib.SRG_GAT_LAUNCH_ROWS + 5
    d = dev()
    i = torch.arange(n, device=d)
    two = (i % 3 == 0)
    src = torch.cat([i, ((i * 7 + 3) % n)[two]])
    dst = torch.cat([i, i[two]])
    g = GT.GATGraph.from_edge_index(torch.stack([src, dst]), n, add_self_loops=False, device=d)
    assert g.nnz > _lib.SRG_GAT_LAUNCH_ROWS
    Hf = ((i % 13).float() - 6.0)[:, None].requires_grad_(True)
    a_s = torch.zeros((n, 1), device=d, requires_grad=True)
    a_d = torch.zeros((n, 1), device=d, requires_grad=True)
    out = GT.gat_attend(g, Hf, a_s, a_d)
    G = ((i % 5).float() - 2.0)[:, None]
    out.backward(G)
    rows = torch.repeat_interleave(i, g.indptr[1:] - g.indptr[:-1])
    ix = g.indices.long()
    ln = (g.indptr[1:] - g.indptr[:-1]).float()[:, None]
    x = Hf.detach()
    want = torch.zeros((n, 1), device=d).index_add(0, rows, x[ix]) / ln
    assert torch.equal(out.detach(), want)
    alpha = (1.0 / ln)[rows]
    assert torch.equal(Hf.grad, torch.zeros((n, 1), device=d).index_add(0, ix, alpha * G[rows]))
    ds = alpha * (G[rows] * x[ix] - (G * want)[rows]) * 0.2
    # halves and integers times 0.2 in fp32: the sums of at most a few such terms; compare within 4 ulp of the
    # largest term instead of exactly (0.2 is not dyadic)
    tol = 4 * R.EPS * 40.0
    assert float((a_d.grad - torch.zeros((n, 1), device=d).index_add(0, rows, ds)).abs().max()) <= tol
    assert float((a_s.grad - torch.zeros((n, 1), device=d).index_add(0, ix, ds)).abs().max()) <= tol
    tail = slice(_lib.SRG_GAT_LAUNCH_ROWS - 2, n)
    assert float(out.detach()[tail].abs().sum()) > 0 and float(Hf.grad[tail].abs().sum()) > 0


def test_empty_operands():
    d = dev()
    g0 = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), 0, add_self_loops=False, device=d)
    z = torch.zeros((0, 6), device=d, requires_grad=True)
    a = torch.zeros((0, 2), device=d, requires_grad=True)
    out = GT.gat_attend(g0, z, a, a)
    out.sum().backward()
    assert tuple(out.shape) == (0, 6) and tuple(z.grad.shape) == (0, 6)
    g5 = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), 5, add_self_loops=False, device=d)
    x = torch.ones((5, 6), device=d, requires_grad=True)
    s = torch.ones((5, 2), device=d, requires_grad=True)
    t_ = torch.ones((5, 2), device=d, requires_grad=True)
    out = GT.gat_attend(g5, x, s, t_)
    out.backward(torch.ones_like(out))
    for v in (out, x.grad, s.grad, t_.grad):
        assert not bits(v).any()


# ---- the layer and the model ------------------------------------------------------------------------
# GATConv with gat_attend replaced by the torch composition in fp64 on the layer's own fp32 Hf, a_src and a_dst;
# everything else -- lin, the scores, the bias -- is the same fp32 torch code on the same device
ComposedConv = R.composed_conv(torch.float64)


def layer_inputs(feat, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R.N, feat)).astype(np.float32)


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("sl", (True, False))
def test_gatconv_against_the_fp64_composition(concat, sl):
    """One layer: both modules hand bit-identical Hf, a_src, a_dst to the aggregation (the same torch kernels on
    the same inputs), so the logits differ by E_out, the rounding of the composition's cast to fp32 and of the
    two bias adds; with the mean over heads, by the mean of E_out and its H adds and divide."""
    H, C, feat = 4, 8, 19
    g = device_graph("sym", sl)
    torch.manual_seed(11)
    ours = GT.GATConv(feat, C, heads=H, concat=concat, add_self_loops=sl).to(dev())
    theirs = ComposedConv(feat, C, heads=H, concat=concat, add_self_loops=sl).to(dev())
    with torch.no_grad():
        ours.bias.uniform_(-0.5, 0.5)
    theirs.load_state_dict(ours.state_dict())                     # round trip of the state dict
    for (k, p), (k2, q) in zip(ours.state_dict().items(), theirs.state_dict().items()):
        assert k == k2 and torch.equal(p, q)
    x = t(layer_inputs(feat, 12))
    y, y2 = ours(x, g), theirs(x, g)
    # the bound, from the fp32 operands the layer really used
    Hf = ours.lin(x).detach()
    Hv = Hf.view(-1, H, C)
    a_src = torch.einsum("nhc,hc->nh", Hv, ours.att_src[0]).detach()
    a_dst = torch.einsum("nhc,hc->nh", Hv, ours.att_dst[0]).detach()
    ip, ix = R.graph("sym", sl)
    Cot = layer_inputs(H * C if concat else C, 13)
    Gagg = Cot if concat else np.repeat(Cot[:, None, :] / np.float32(H), H, axis=1).reshape(R.N, H * C)
    ref = R.evaluate(ip, ix, host(Hf), host(a_src), host(a_dst), ours.negative_slope, Gagg)
    assert ref["band"] == 0
    E = ref["E_out"] + R.EPS * np.abs(ref["out"])                 # the composition's cast to fp32
    val = ref["out"]
    if not concat:                                               # H-term sum and a divide on either side
        E = E.reshape(R.N, H, C).sum(axis=1) / H + 2 * (H + 1) * R.EPS * np.abs(val.reshape(R.N, H, C)).sum(axis=1) / H
        val = val.reshape(R.N, H, C).mean(axis=1)
    b = host(ours.bias).astype(np.float64)
    E = E + 2 * R.EPS * (np.abs(val) + np.abs(b))                # the bias add, once on either side
    err = np.abs(host(y).astype(np.float64) - host(y2).astype(np.float64))
    print(f"gat layer logits concat={concat} loops={sl}: {float((err / E).max()):.4f} of the bound")
    assert (err <= E).all()

    # parameter gradients.  dL/d(aggregation output) is Gagg on both sides up to the mean's rounding; the
    # aggregation's own gradients differ by the bounds of evaluate (the composition's fp64 gradients are cast to
    # fp32: 1 eps); the dense backward that follows is the same fp32 torch code on both sides, an n-term (lin,
    # att) or C-term (scores) sum of products each, applied to inputs that differ by those bounds.
    (y * t(Cot)).sum().backward()
    (y2 * t(Cot)).sum().backward()
    n = R.N
    absH = np.abs(host(Hf).astype(np.float64)).reshape(n, H, C)
    att_s, att_d = (host(p).astype(np.float64)[0] for p in (ours.att_src, ours.att_dst))
    e_s = ref["E_da_src"] + R.EPS * np.abs(ref["da_src"])
    e_d = ref["E_da_dst"] + R.EPS * np.abs(ref["da_dst"])
    # att gradients: sum_n da[n,h] Hf[n,h,c], n terms, twice (either side's own rounding)
    for name, e_a, da in (("att_src", e_s, ref["da_src"]), ("att_dst", e_d, ref["da_dst"])):
        bound = np.einsum("nh,nhc->hc", e_a, absH) + 2 * n * R.EPS * np.einsum("nh,nhc->hc", np.abs(da), absH)
        err = np.abs(host(getattr(ours, name).grad).astype(np.float64) - host(getattr(theirs, name).grad).astype(np.float64))[0]
        print(f"gat layer {name}.grad: {float((err / bound).max()):.4f} of the bound")
        assert (err <= bound).all(), name
    # dHf in total: the aggregation's part, and the scores' parts da_src[n,h] att_src[h,c] + da_dst[n,h] att_dst[h,c]
    # (a product each and two adds, either side)
    dH = ref["dHf"].reshape(n, H, C)
    parts = np.abs(dH) + np.abs(ref["da_src"])[:, :, None] * np.abs(att_s) + np.abs(ref["da_dst"])[:, :, None] * np.abs(att_d)
    e_H = ref["E_dHf"].reshape(n, H, C) + R.EPS * np.abs(dH) + e_s[:, :, None] * np.abs(att_s) + \
        e_d[:, :, None] * np.abs(att_d) + 2 * 3 * R.EPS * parts
    absx = np.abs(host(x).astype(np.float64))
    bound = np.einsum("nw,nf->wf", e_H.reshape(n, H * C), absx) + \
        2 * n * R.EPS * np.einsum("nw,nf->wf", parts.reshape(n, H * C), absx)
    err = np.abs(host(ours.lin.weight.grad).astype(np.float64) - host(theirs.lin.weight.grad).astype(np.float64))
    print(f"gat layer lin.weight.grad: {float((err / bound).max()):.4f} of the bound")
    assert (err <= bound).all()
    # bias: a column sum of the same cotangent on both sides, n terms each (the mean passes Cot / H on, exact)
    colsum = np.abs(Cot.astype(np.float64)).sum(axis=0)
    err = np.abs(host(ours.bias.grad).astype(np.float64) - host(theirs.bias.grad).astype(np.float64))
    assert (err <= 2 * n * R.EPS * colsum).all()


def test_gat_model_against_the_fp64_composition():
    """The two-layer GAT against the same model with gat_attend replaced by the fp64 composition in both
    layers: logits and all eight parameter gradients within the bound composed in gat_ref.two_layer_bound (the
    first layer's bound pushed through ReLU, the second layer's dense steps, evaluate's E_x / E_asrc / E_adst /
    E_G inputs, log_softmax and back); no ReLU input and no score in its kink band.  The state dict round-trips
    into the composed model and into a second fused model, which returns the same bits."""
    n = R.MODEL_N
    dst, src = R.model_edges()
    ip, ix = R.csr_of(dst, src, n, True)
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n, device=dev())
    torch.manual_seed(R.MODEL_SEED)
    ours = GT.GAT(19, 8, 5, 2, 0.0, 4).to(dev())
    with torch.no_grad():
        for conv in ours.convs:
            conv.bias.uniform_(-0.5, 0.5)
    theirs = GT.GAT(19, 8, 5, 2, 0.0, 4).to(dev())
    for conv in theirs.convs:
        conv.__class__ = ComposedConv
    assert sorted(ours.state_dict()) == sorted(
        f"convs.{i}.{k}" for i in (0, 1) for k in ("att_src", "att_dst", "bias", "lin.weight"))
    theirs.load_state_dict(ours.state_dict())
    x = t(np.random.default_rng(22).standard_normal((n, 19)).astype(np.float32))
    Cot = np.random.default_rng(23).standard_normal((n, 5)).astype(np.float32)
    y, y2 = ours(x, g), theirs(x, g)
    assert tuple(y.shape) == (n, 5)
    (y * t(Cot)).sum().backward()
    (y2 * t(Cot)).sum().backward()
    L1, L2 = R.model_layers(ours, x, lambda conv, Hf, a_s, a_d: GT.gat_attend(g, Hf, a_s, a_d, conv.negative_slope))
    bound = R.two_layer_bound(ip, ix, host(x), L1, L2, Cot)
    R.check_model("device", bound, y, y2, list(ours.named_parameters()), list(theirs.named_parameters()))
    other = GT.GAT(19, 8, 5, 2, 0.0, 4).to(dev())
    other.load_state_dict(ours.state_dict())
    assert np.array_equal(bits(other(x, g)), bits(y))


# ---- memory -----------------------------------------------------------------------------------------
def test_no_per_edge_message_tensor():
    """n = 2,048, 64 entries per row, H = 4, C = 64: the peak of forward + backward beyond the operands, out
    and the returned gradients stays below a quarter of nnz * H * C * 4 bytes (the composition's smallest
    per-edge temporary, 134 MB here)."""
    n, deg, H, C = 2048, 64, 4, 64
    d = dev()
    rng = np.random.default_rng(31)
    src = rng.integers(0, n, n * deg)
    dst = np.repeat(np.arange(n), deg)
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n, add_self_loops=False, device=d)
    nnz = g.nnz
    Hf = torch.randn((n, H * C), device=d, requires_grad=True)
    a_s = torch.randn((n, H), device=d, requires_grad=True)
    a_d = torch.randn((n, H), device=d, requires_grad=True)
    G = torch.randn((n, H * C), device=d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(d)
    base = torch.cuda.memory_allocated(d)
    out = GT.gat_attend(g, Hf, a_s, a_d)
    out.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(d) - base
    kept = 4 * (2 * n * H * C + 2 * n * H)                      # out, dHf, da_src, da_dst
    extra = peak - kept
    print(f"gat peak beyond operands and results: {extra} bytes; nnz*H*4 = {nnz * H * 4}, nnz*H*C*4 = {nnz * H * C * 4}")
    assert extra < nnz * H * C * 4 // 4
    assert Hf.grad is not None and a_s.grad is not None and a_d.grad is not None
