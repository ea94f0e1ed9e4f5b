"""srgnn.gat's rows= on the GPU: the batch path against the project's own full path, bit for
bit -- out, M, Z are the full call's rows; under the cotangent that is zero outside the batch the full backward's
dHf and da_src are the batch's, its da_dst the batch's rows and zero elsewhere, its dS the compact dS at the batch
rows' entries -- then within gat_ref's bound of the fp64 formula, deterministic, indifferent to the load path and
to what rows outside the batch hold, safe on bad ids, positions and prefix sums, inside GATConv and GAT, and
without a temporary of the full path's size."""
import numpy as np
import pytest
import torch

import gat_ref as R
import gat_rows_ref as RR
from srgnn import _lib
from srgnn import gat as GT

pytestmark = pytest.mark.gpu

SENT = 9.0
_graphs, _inputs, _full = {}, {}, {}


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


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.size} elements differ, first at {tuple(bad[0])}")


def device_graph(kind, sl):
    if (kind, sl) not in _graphs:
        dst, src = R.base_edges(kind)
        _graphs[(kind, sl)] = GT.GATGraph.from_edge_index(np.stack([src, dst]), R.N, add_self_loops=sl, device=dev())
    return _graphs[(kind, sl)]


def inputs(kind, sl, H, C):
    """(Hf, a_src, a_dst, G) of a case as device tensors, built once and never changed."""
    key = (kind, sl, H, C)
    if key not in _inputs:
        _inputs[key] = tuple(t(a) for a in R.inputs(R.N, H, C, R.case_seed(kind, sl, H, C)))
    return _inputs[key]


def edge_grad_full(g, x, s_, d_, out, M, Z, G):
    """(dS [nnz, H], da_dst) of srg_gat_edge_grad_f32 on raw pointers."""
    n, nnz, H, W = g.n, g.nnz, s_.shape[1], x.shape[1]
    D, dS, da = (torch.full(sh, SENT, device=dev()) for sh in ((n, H), (nnz, H), (n, H)))
    _lib.call(dev(), "srg_gat_edge_grad_f32", g.indptr.data_ptr(), g.indices.data_ptr(), nnz, n, n, s_.data_ptr(),
              d_.data_ptr(), 0.2, x.data_ptr(), W, H, W // H, out.data_ptr(), W, M.data_ptr(), Z.data_ptr(), G.data_ptr(),
              W, D.data_ptr(), dS.data_ptr(), da.data_ptr(), _lib.stream(dev()))
    return dS, da


def full_forward(kind, sl, H, C):
    key = (kind, sl, H, C)
    if key not in _full:
        x, s_, d_, _ = inputs(kind, sl, H, C)
        _full[key] = GT.attend_forward(device_graph(kind, sl), x, s_, d_)
    return _full[key]


def ptr(x):
    return x.data_ptr() if x is not None and x.numel() else None


class Raw:
    """The three rows entries on raw pointers, every output a window of a sentinel buffer (one row, or entry,
    of SENT before and after).  Operands default to the consistent ones of (g, ids); any may be replaced."""

    def __init__(self, g, ids, x, s_, d_, G, **over):
        self.g, self.n, self.nnz = g, g.n, g.nnz
        self.H, self.W = s_.shape[1], x.shape[1]
        self.C = self.W // self.H
        self.x, self.s_, self.d_, self.G = x, s_, d_, G
        ids_np = np.asarray(ids, dtype=np.int64)
        self.B = ids_np.size
        ok = (ids_np >= 0) & (ids_np < g.n)
        ip = host(g.indptr)
        lens = np.where(ok, ip[np.where(ok, ids_np, 0) + 1] - ip[np.where(ok, ids_np, 0)], 0)
        pos = np.full(g.n, -1, dtype=np.int32)
        pos[ids_np[ok]] = np.flatnonzero(ok).astype(np.int32)
        self.eptr_np = np.r_[0, np.cumsum(lens)].astype(np.int64)
        self.rows, self.pos, self.eptr = t(ids_np), t(pos), t(self.eptr_np)
        self.nnzB = int(self.eptr_np[-1])
        self.ip, self.ix = g.indptr, g.indices
        self.ip_t, self.ix_t, self.perm = g.indptr_t, g.indices_t, g.perm
        for k, v in over.items():
            assert hasattr(self, k), k
            setattr(self, k, v)
        self.bufs = {}

    def guarded(self, name, rows, cols):
        buf = torch.full((rows + 2, cols), SENT, device=dev())
        self.bufs[name] = (buf, rows)
        return buf[1:rows + 1]

    def run(self):
        B, H, C, W, n, nnz, st = self.B, self.H, self.C, self.W, self.n, self.nnz, _lib.stream(dev())
        out, M, Z = self.guarded("out", B, W), self.guarded("M", B, H), self.guarded("Z", B, H)
        _lib.call(dev(), "srg_gat_attend_rows_f32", self.ip.data_ptr(), ptr(self.ix), nnz, n, n, ptr(self.rows), B,
                  self.s_.data_ptr(), self.d_.data_ptr(), 0.2, self.x.data_ptr(), W, H, C, ptr(out), W, ptr(M), ptr(Z), st)
        D, dS, da_dst = self.guarded("D", B, H), self.guarded("dS", self.nnzB, H), self.guarded("da_dst", B, H)
        _lib.call(dev(), "srg_gat_edge_grad_rows_f32", self.ip.data_ptr(), ptr(self.ix), nnz, n, n, ptr(self.rows), B,
                  self.eptr.data_ptr(), self.nnzB, self.s_.data_ptr(), self.d_.data_ptr(), 0.2, self.x.data_ptr(), W, H, C,
                  ptr(out), W, ptr(M), ptr(Z), ptr(self.G), W, ptr(D), ptr(dS), ptr(da_dst), st)
        return self.adjoint(M, Z, dS, dict(out=out, M=M, Z=Z, dS=dS, da_dst=da_dst))

    def adjoint(self, M, Z, dS, res=None):
        B, H, C, W, n, nnz, st = self.B, self.H, self.C, self.W, self.n, self.nnz, _lib.stream(dev())
        dHf, da_src = self.guarded("dHf", n, W), self.guarded("da_src", n, H)
        _lib.call(dev(), "srg_gat_attend_rows_adjoint_f32", self.ip_t.data_ptr(), ptr(self.ix_t), ptr(self.perm), nnz, n, n,
                  self.pos.data_ptr(), B, self.ip.data_ptr(), self.eptr.data_ptr(), self.nnzB, self.s_.data_ptr(),
                  self.d_.data_ptr(), 0.2, H, C, ptr(M), ptr(Z), ptr(self.G), W, ptr(dS), dHf.data_ptr(), W,
                  da_src.data_ptr(), st)
        torch.cuda.synchronize()
        res = dict(res or {}, dHf=dHf, da_src=da_src)
        for name, (buf, rows) in self.bufs.items():
            edge = torch.cat([buf[0], buf[rows + 1]])
            assert bool((edge == SENT).all()), f"{name}: a sentinel was overwritten"
        return {k: host(v).copy() for k, v in res.items()}


# ---- bitwise parity with the full path --------------------------------------------------------------
@pytest.mark.parametrize("H,C", RR.SHAPES)
@pytest.mark.parametrize("kind,sl", RR.GRAPHS)
def test_bitwise_parity_with_the_full_path(kind, sl, H, C):
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    out_f, M_f, Z_f = full_forward(kind, sl, H, C)
    ip = host(g.indptr)
    for name in RR.BATCHES:
        rows = RR.batch(name, kind, sl)
        idx = t(rows)
        B = rows.size
        out, M, Z = GT.attend_forward(g, x, s_, d_, rows=idx)
        assert tuple(out.shape) == (B, H * C) and tuple(M.shape) == (B, H) and tuple(Z.shape) == (B, H)
        same(out, out_f[idx], f"{name}: out")
        same(M, M_f[idx], f"{name}: M")
        same(Z, Z_f[idx], f"{name}: Z")
        Gb = G[idx].contiguous()
        Gpad = torch.zeros_like(G).index_copy_(0, idx, Gb)
        dHf_f, das_f, dad_f = GT.attend_backward(g, x, s_, d_, out_f, M_f, Z_f, Gpad)
        dHf, das, dad = GT.attend_backward(g, x, s_, d_, out, M, Z, Gb, rows=idx)
        assert tuple(dHf.shape) == (R.N, H * C) and tuple(das.shape) == (R.N, H) and tuple(dad.shape) == (R.N, H)
        same(dHf, dHf_f, f"{name}: dHf")
        same(das, das_f, f"{name}: da_src")
        same(dad[idx], dad_f[idx], f"{name}: da_dst at the batch")
        outside = np.setdiff1d(np.arange(R.N), rows)
        assert not host(dad_f)[outside].any() and not bits(dad)[outside].any(), f"{name}: da_dst outside the batch"
        # the compact dS against the full dS at the batch rows' entries, on raw pointers
        dS_f, _ = edge_grad_full(g, x, s_, d_, out_f, M_f, Z_f, Gpad)
        raw = Raw(g, rows, x, s_, d_, Gb).run() if B else None
        if B:
            same(raw["dS"], dS_f[t(RR.entries_of(ip, rows))], f"{name}: dS")
            for k, v in (("out", out), ("M", M), ("Z", Z), ("dHf", dHf), ("da_src", das), ("da_dst", dad[idx])):
                same(raw[k], v, f"{name}: {k} on raw pointers")
        if name == "isolated" and not sl:                     # +0, M = Z = 0, and no gradient anywhere
            for v in (out, M, Z, dHf, das, dad):
                assert not bits(v).any(), name
        if name == "all":                                     # the identity batch is the full call
            dHf_u, das_u, dad_u = GT.attend_backward(g, x, s_, d_, out_f, M_f, Z_f, G)
            same(dHf, dHf_u, "all: dHf against the unpadded full call")
            same(das, das_u, "all: da_src against the unpadded full call")
            same(dad, dad_u, "all: da_dst against the unpadded full call")
        if name == "empty":
            for v in (dHf, das, dad):
                assert not bits(v).any(), name


def run_rows(g, Hf, a_src, a_dst, G, rows, slope=0.2):
    """Everything the batch path returns, as host arrays, through the autograd function."""
    x, s, d = (v.clone().requires_grad_(True) for v in (Hf, a_src, a_dst))
    out = GT.gat_attend(g, x, s, d, slope, rows=rows)
    out.backward(G)
    return dict(out=host(out), dHf=host(x.grad), da_src=host(s.grad), da_dst=host(d.grad))


@pytest.mark.parametrize("H,C", RR.SHAPES)
def test_within_the_bound_of_the_fp64_formula(H, C):
    """gat_ref.evaluate with the padded G, indexed: the bound the full path is held to."""
    kind, sl = "sym", False
    ip, ix = R.graph(kind, sl)
    Hf, a_src, a_dst, G = R.inputs(R.N, H, C, R.case_seed(kind, sl, H, C))
    rows = RR.batch("mixed37", kind, sl)
    Gb = G[rows]
    full = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, RR.pad(Gb, rows, R.N))
    assert full["band"] == 0
    ref = RR.index_ref(full, rows, ip)
    g = device_graph(kind, sl)
    got = run_rows(g, t(Hf), t(a_src), t(a_dst), t(Gb), t(rows))
    got["da_dst"] = got["da_dst"][rows]
    _, M, Z = GT.attend_forward(g, t(Hf), t(a_src), t(a_dst), rows=t(rows))
    got.update(M=host(M), Z=host(Z))
    R.check(f"device rows H={H} C={C}", ref, got)
    # and the rows reference of the helper, which never sees the rows outside the batch
    R.check(f"device rows H={H} C={C}, restricted graph", RR.evaluate_rows(ip, ix, Hf, a_src, a_dst, rows, 0.2, Gb), got)


def test_run_to_run_identical():
    kind, sl, H, C = "sym", True, 4, 64
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    idx = t(RR.batch("mixed37", kind, sl))
    first = run_rows(g, x, s_, d_, G[idx], idx)
    for _ in range(2):
        again = run_rows(g, x, s_, d_, G[idx], idx)
        for k in first:
            same(again[k], first[k], k)


@pytest.mark.parametrize("H,C", ((4, 64), (3, 8)))
def test_strided_windows_take_the_4_byte_path(H, C):
    """Contiguous panels of a width that is a multiple of 4 take 16-byte loads; the same columns as a window at
    an odd offset of a wider panel cannot.  The same bits."""
    kind, sl = "sym", True
    g = device_graph(kind, sl)
    Hf, a_src, a_dst, G = (t(a) for a in R.inputs(R.N, H, C, 60 + C))
    idx = t(RR.batch("mixed37", kind, sl))
    W, B = H * C, idx.numel()
    wide_h = torch.zeros((R.N, W + 3), device=dev())
    wide_h[:, 1:W + 1] = Hf
    wide_g = torch.zeros((B, W + 7), device=dev())
    wide_g[:, 3:W + 3] = G[idx]
    a = run_rows(g, Hf, a_src, a_dst, G[idx].contiguous(), idx)
    b = run_rows(g, wide_h[:, 1:W + 1], a_src, a_dst, wide_g[:, 3:W + 3], idx)
    for k in a:
        same(a[k], b[k], k)


# ---- skipped, not multiplied ------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", ((3, 7), (4, 64)))
def test_rows_outside_the_batch_are_skipped_not_multiplied(H, C):
    """a_dst of a target outside the batch set to NaN, of another to Inf: both are targets of sources that also
    reach the batch, and no result of the rows call moves.  (The padded full call would turn NaN there.)"""
    kind, sl = "sym", False
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    rows = RR.batch("mixed37", kind, sl)
    ip, ix = R.graph(kind, sl)
    # two targets outside the batch that share a source with the star row
    member = np.zeros(R.N, bool)
    member[rows] = True
    star_sources = set(ix[ip[R.STAR]:ip[R.STAR + 1]].tolist())
    er = R.entry_rows(ip)
    cand = [int(r) for r in np.unique(er[np.isin(ix, list(star_sources))]) if not member[r]]
    assert len(cand) >= 2
    dirty = d_.clone()
    dirty[cand[0]] = float("nan")
    dirty[cand[1]] = float("inf")
    idx = t(rows)
    clean = run_rows(g, x, s_, d_, G[idx], idx)
    got = run_rows(g, x, s_, dirty, G[idx], idx)
    for k in clean:
        assert np.isfinite(got[k]).all(), k
        same(got[k], clean[k], k)
    _, M, Z = GT.attend_forward(g, x, s_, dirty, rows=idx)
    _, M0, Z0 = GT.attend_forward(g, x, s_, d_, rows=idx)
    same(M, M0, "M")
    same(Z, Z0, "Z")


# ---- ids, positions and prefix sums are never addresses before they are checked ---------------------
def case_for_raw():
    kind, sl, H, C = "asym", False, 3, 7
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    return kind, sl, g, x, s_, d_, G


def test_bad_row_ids_give_zero_rows():
    """rows holding -1 and n: out = +0, M = Z = 0 there, nothing of theirs in dS or any gradient; every other
    row and result as in the call without them."""
    kind, sl, g, x, s_, d_, G = case_for_raw()
    good = np.array([R.STAR, 20, 30, R.ISOLATED[0], 77], dtype=np.int64)
    bad = np.array([R.STAR, -1, 20, 30, R.N, R.ISOLATED[0], 77], dtype=np.int64)
    at = np.array([0, 2, 3, 5, 6])
    Gb = G[:bad.size].contiguous()
    a = Raw(g, bad, x, s_, d_, Gb).run()
    b = Raw(g, good, x, s_, d_, Gb[t(at)].contiguous()).run()
    for k in ("out", "M", "Z", "da_dst"):
        same(a[k][at], b[k], k)
        assert not bits(a[k][[1, 4]]).any(), k
    for k in ("dS", "dHf", "da_src"):
        same(a[k], b[k], k)


def test_bad_positions_are_no_members():
    """pos holding B, -2 and, for a target outside the batch, the position of the batch's empty row: the three
    targets stay outside.  (A forged position of a row with entries is computed with that row's statistics: the
    header says so.)"""
    kind, sl, g, x, s_, d_, G = case_for_raw()
    rows = RR.batch("mixed37", kind, sl)
    ip, ix = R.graph(kind, sl)
    Gb = G[t(rows)].contiguous()
    clean = Raw(g, rows, x, s_, d_, Gb)
    want = clean.run()
    member = np.zeros(R.N, bool)
    member[rows] = True
    targets = [int(r) for r in np.flatnonzero((np.diff(ip) > 0) & ~member)][:3]
    pos = host(clean.pos).copy()
    empty_slot = int(np.flatnonzero(rows == R.ISOLATED[0])[0])
    assert clean.eptr_np[empty_slot + 1] == clean.eptr_np[empty_slot]
    pos[targets] = [rows.size, -2, empty_slot]
    got = Raw(g, rows, x, s_, d_, Gb, pos=t(pos)).run()
    for k in want:
        same(got[k], want[k], k)


def test_bad_transpose_ids_and_perm_are_skipped():
    """indices_t holding -1 and n at two member entries, perm holding -1 and nnz at two others.  dHf is the chain
    of the transpose without the two entries (built here); da_src the clean call's with +0 in dS at the four
    entries' places: a skipped entry leaves its position out and moves no other term."""
    kind, sl, g, x, s_, d_, G = case_for_raw()
    rows = RR.batch("mixed37", kind, sl)
    ip, ix = R.graph(kind, sl)
    tp, tx, perm = R.transpose_of(ip, ix, R.N)
    Gb = G[t(rows)].contiguous()
    clean = Raw(g, rows, x, s_, d_, Gb)
    want = clean.run()
    hits = np.flatnonzero(tx == R.STAR)[[1, 50, 120, 200]]       # members: entries of At whose target is the star
    bad_t, bad_p = tx.copy(), perm.copy()
    bad_t[hits[:2]] = [-1, R.N]
    bad_p[hits[2:]] = [-1, ix.size]
    M, Z, dS = t(want["M"]), t(want["Z"]), t(want["dS"])
    got = Raw(g, rows, x, s_, d_, Gb, ix_t=t(bad_t), perm=t(bad_p)).adjoint(M, Z, dS)
    # da_src: the clean operands with +0 at the four places
    eptr, star_slot = clean.eptr_np, int(np.flatnonzero(rows == R.STAR)[0])
    places = eptr[star_slot] + (perm[hits] - ip[R.STAR])
    zeroed = dS.clone()
    zeroed[t(places)] = 0.0
    ref_s = Raw(g, rows, x, s_, d_, Gb).adjoint(M, Z, zeroed)
    same(got["da_src"], ref_s["da_src"], "da_src")
    assert not np.array_equal(bits(ref_s["da_src"]), bits(want["da_src"]))
    # dHf: the transpose with the two entries taken out
    keep = np.ones(tx.size, bool)
    keep[hits[:2]] = False
    tp2 = np.zeros(R.N + 1, dtype=np.int64)
    np.add.at(tp2, R.entry_rows(tp)[keep] + 1, 1)
    ref_h = Raw(g, rows, x, s_, d_, Gb, ip_t=t(np.cumsum(tp2)), ix_t=t(tx[keep]), perm=t(perm[keep])).adjoint(M, Z, dS)
    same(got["dHf"], ref_h["dHf"], "dHf")
    assert not np.array_equal(bits(ref_h["dHf"]), bits(want["dHf"]))


def test_a_prefix_sum_past_nnzB_is_clamped():
    """eptr's tail exceeds nnzB: no compact position at or past nnzB is written or read.  dS below nnzB is the
    clean call's, the sentinel behind it stays, da_dst of the cut row is the sum of what is left, da_src the clean
    call's with +0 behind the cut."""
    kind, sl, g, x, s_, d_, G = case_for_raw()
    rows = RR.batch("mixed37", kind, sl)
    rows = np.r_[rows[rows != R.STAR], R.STAR]                    # the star row last: it is the one cut
    Gb = G[t(rows)].contiguous()
    clean = Raw(g, rows, x, s_, d_, Gb)
    want = clean.run()
    cut = int(clean.eptr_np[-2]) + 100                            # 100 of the star's 320 entries stay
    assert clean.eptr_np[-2] < cut < clean.nnzB
    got = Raw(g, rows, x, s_, d_, Gb, nnzB=cut).run()
    for k in ("out", "M", "Z", "dHf"):
        same(got[k], want[k], k)
    same(got["dS"], want["dS"][:cut], "dS below the cut")
    same(got["da_dst"][:-1], want["da_dst"][:-1], "da_dst of the whole rows")
    left = want["dS"][clean.eptr_np[-2]:cut].astype(np.float64)
    err = np.abs(got["da_dst"][-1] - left.sum(axis=0))
    assert (err <= left.shape[0] * R.EPS * np.abs(left).sum(axis=0)).all()
    zeroed = t(want["dS"])
    zeroed[cut:] = 0.0
    ref = Raw(g, rows, x, s_, d_, Gb).adjoint(t(want["M"]), t(want["Z"]), zeroed)
    same(got["da_src"], ref["da_src"], "da_src")


def test_empty_operands():
    d = dev()
    g5 = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), 5, add_self_loops=False, device=d)
    x = torch.ones((5, 6), device=d, requires_grad=True)
    s = torch.ones((5, 2), device=d, requires_grad=True)
    t_ = torch.ones((5, 2), device=d, requires_grad=True)
    out = GT.gat_attend(g5, x, s, t_, rows=[4, 1])
    out.backward(torch.ones_like(out))
    assert tuple(out.shape) == (2, 6)
    for v in (out, x.grad, s.grad, t_.grad):
        assert not bits(v).any()
    g = device_graph("sym", True)
    Hf, a_src, a_dst, _ = (v.clone().requires_grad_(True) for v in inputs("sym", True, 3, 7))
    out = GT.gat_attend(g, Hf, a_src, a_dst, rows=[])
    out.sum().backward()
    assert tuple(out.shape) == (0, 21)
    for v in (Hf.grad, a_src.grad, a_dst.grad):
        assert tuple(v.shape)[0] == R.N and not bits(v).any()


# ---- the Python side --------------------------------------------------------------------------------
def test_a_repeated_id_is_computed_once_and_its_cotangents_add():
    kind, sl, H, C = "sym", True, 3, 7
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    rows = np.array([R.STAR, 20, R.STAR, -1, 20, 5, R.STAR], dtype=np.int64)
    wrapped = np.where(rows < 0, rows + R.N, rows)
    uniq, inverse = np.unique(wrapped, return_inverse=True)
    Gb = G[:rows.size].contiguous()
    got = run_rows(g, x, s_, d_, Gb, rows.tolist())
    Gsum = torch.zeros((uniq.size, H * C), device=dev()).index_add_(0, t(inverse), Gb)
    want = run_rows(g, x, s_, d_, Gsum, t(uniq))
    same(got["out"], want["out"][inverse], "out")
    # index_add_ above and torch's indexing backward both sum the repeats' cotangents, of at most three terms
    # each: the same fp32 sum whatever the order only up to rounding, so G is made of small integers
    Gi = torch.round(Gb * 4)
    got = run_rows(g, x, s_, d_, Gi, rows.tolist())
    want = run_rows(g, x, s_, d_, torch.zeros_like(Gsum).index_add_(0, t(inverse), Gi), t(uniq))
    for k in want:
        same(got[k], want[k] if k != "out" else want[k][inverse], k)


def test_host_rows_lists_ranges_and_need_flags():
    kind, sl, H, C = "sym", True, 3, 7
    g = device_graph(kind, sl)
    x, s_, d_, G = inputs(kind, sl, H, C)
    want = run_rows(g, x, s_, d_, G[10:50:3], t(np.arange(10, 50, 3)))
    for rows in (range(10, 50, 3), list(range(10, 50, 3)), torch.arange(10, 50, 3), np.arange(10, 50, 3) - R.N):
        got = run_rows(g, x, s_, d_, G[10:50:3], rows)
        for k in want:
            same(got[k], want[k], k)
    with pytest.raises(IndexError):
        GT.gat_attend(g, x, s_, d_, rows=[R.N])
    # only the gradients autograd asks for
    idx = t(np.arange(10, 50, 3))
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        ops = [v.clone().requires_grad_(f) for v, f in zip((x, s_, d_), need)]
        GT.gat_attend(g, *ops, rows=idx).backward(G[10:50:3])
        for v, f, k in zip(ops, need, ("dHf", "da_src", "da_dst")):
            if f:
                same(v.grad, want[k], (k, need))
            else:
                assert v.grad is None


# ---- the layer and the model ------------------------------------------------------------------------
def layer_inputs(n, feat, seed):
    return t(np.random.default_rng(seed).standard_normal((n, feat)).astype(np.float32))


def bias_bound(G64, B):
    """A B-term fp32 column sum in any order against the fp64 sum: B eps sum |G| per column."""
    return B * R.EPS * np.abs(G64).sum(axis=0)


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("sl", (True, False))
def test_gatconv_rows_against_the_same_layer_indexed(concat, sl):
    """GATConv(x, g, rows=idx) against forward(x, g)[idx] with the loss read at idx: the output and the
    gradients of lin.weight, att_src and att_dst bit for bit (the bit-equal dHf, da_src, da_dst go through the
    same dense ops on the same shapes); the bias gradient, a torch sum over B rows on one side and n on the other,
    against the fp64 sum."""
    H, C, feat = 4, 8, 19
    g = device_graph("sym", sl)
    torch.manual_seed(11)
    conv = GT.GATConv(feat, C, heads=H, concat=concat, add_self_loops=sl).to(dev())
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    x = layer_inputs(R.N, feat, 12)
    rows = RR.batch("mixed37", "sym", sl)
    idx = t(rows)
    Cot = layer_inputs(rows.size, H * C if concat else C, 13)
    y_full = conv(x, g)[idx]
    (y_full * Cot).sum().backward()
    want = {k: p.grad.clone() for k, p in conv.named_parameters()}
    conv.zero_grad(set_to_none=True)
    y = conv(x, g, rows=idx)
    assert tuple(y.shape) == (rows.size, H * C if concat else C)
    (y * Cot).sum().backward()
    same(y, y_full, "the layer's output")
    for k in ("lin.weight", "att_src", "att_dst"):
        same(dict(conv.named_parameters())[k].grad, want[k], k)
    exact = host(Cot).astype(np.float64)
    bound = bias_bound(exact, rows.size)
    for name, got in (("rows", conv.bias.grad), ("full", want["bias"])):
        err = np.abs(host(got).astype(np.float64) - exact.sum(axis=0))
        print(f"gat rows layer bias.grad ({name}) concat={concat} loops={sl}: {float((err / bound).max()):.4f} of the bound")
        assert (err <= bound).all(), name
    # rows as a list with a repeat: the same rows again
    again = conv(x, g, rows=[int(rows[0]), int(rows[1]), int(rows[0])])
    same(again, y[t(np.array([0, 1, 0]))], "a repeated id in the layer")


def test_gat_model_rows_against_the_same_model_indexed():
    """The two-layer GAT on gat_ref's 64-node model graph: model(x, g, rows=idx) against model(x, g)[idx], the
    loss read at idx.  The last layer's output before log_softmax is compared bit for bit as well, so that a
    difference in torch's log_softmax between [B, k] and [n, k] would be told apart from one of the layer."""
    n = R.MODEL_N
    dst, src = R.model_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n, device=dev())
    torch.manual_seed(R.MODEL_SEED)
    model = GT.GAT(19, 8, 5, 2, 0.0, 4).to(dev())
    with torch.no_grad():
        for conv in model.convs:
            conv.bias.uniform_(-0.5, 0.5)
    x = layer_inputs(n, 19, 22)
    rows = np.random.default_rng(24).permutation(n)[:23].astype(np.int64)
    idx = t(rows)
    Cot = layer_inputs(rows.size, 5, 23)
    seen = []
    hook = model.convs[-1].register_forward_hook(lambda m, a, out: seen.append(out.detach().clone()))
    y_full = model(x, g)[idx]
    (y_full * Cot).sum().backward()
    want = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    y = model(x, g, rows=idx)
    hook.remove()
    assert tuple(y.shape) == (rows.size, 5)
    (y * Cot).sum().backward()
    same(seen[1], seen[0][idx], "the last layer's output before log_softmax")
    same(y, y_full, "the log-probabilities")
    for k, p in model.named_parameters():
        if k == "convs.1.bias":
            continue
        same(p.grad, want[k], k)
    # the last bias: dz = Cot - softmax * sum(Cot), summed over B rows here and over n rows there
    sm = np.exp(host(y).astype(np.float64))
    c64 = host(Cot).astype(np.float64)
    dz = c64 - sm * c64.sum(axis=1, keepdims=True)
    # dz itself carries fp32 rounding on both sides: 4 eps (|Cot| + |sm sum Cot|) covers exp, the sum, the product
    # and the subtraction per element
    slack = 4 * R.EPS * (np.abs(c64) + sm * np.abs(c64).sum(axis=1, keepdims=True)).sum(axis=0)
    for name, got in (("rows", model.convs[1].bias.grad), ("full", want["convs.1.bias"])):
        err = np.abs(host(got).astype(np.float64) - dz.sum(axis=0))
        assert (err <= bias_bound(dz, rows.size) + slack).all(), name


# ---- memory -----------------------------------------------------------------------------------------
def test_no_temporary_of_the_full_paths_size():
    """An R-MAT of n = 20,000 and about 400,000 entries, H = 8, C = 4, B = 64: the [nnz, H] gradient of the
    scores dominates the full path.  The peak of the rows path's forward + backward beyond the operands and the
    returned gradients stays below 4 nnz H bytes, the full path's dS alone; the batch's own temporaries are less
    than a quarter of that, so the cap cannot hide a full-size one."""
    from srgnn import synth
    n, H, C, B = 20000, 8, 4, 64
    d = dev()
    u, v = synth.rmat_undirected_t(n, 200000, seed=synth.RMAT_SEED, device=d)
    g = GT.GATGraph.from_edge_index(torch.stack([torch.cat([u, v]), torch.cat([v, u])]), n, add_self_loops=True, device=d)
    nnz = g.nnz
    assert 300000 <= nnz <= 500000, nnz
    rows = torch.from_numpy(np.random.default_rng(5).choice(n, B, replace=False)).to(d)
    ip = g.indptr
    nnzB = int((ip[rows + 1] - ip[rows]).sum())
    assert 4 * (nnzB * H + 3 * B * H + B * H * C) < 4 * nnz * H // 4, (nnzB, nnz)
    Hf = torch.randn((n, H * C), device=d, requires_grad=True)
    a_s = torch.randn((n, H), device=d, requires_grad=True)
    a_d = torch.randn((n, H), device=d, requires_grad=True)
    G = torch.randn((B, H * C), device=d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(d)
    base = torch.cuda.memory_allocated(d)
    out = GT.gat_attend(g, Hf, a_s, a_d, rows=rows)
    out.backward(G)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(d) - base
    kept = 4 * (B * H * C + n * H * C + 2 * n * H)              # out, dHf, da_src, da_dst
    extra = peak - kept
    print(f"gat rows peak beyond operands and results: {extra} bytes; full dS = nnz*H*4 = {nnz * H * 4}; "
          f"nnzB = {nnzB}")
    assert extra < 4 * nnz * H
    assert Hf.grad is not None and a_s.grad is not None and a_d.grad is not None
