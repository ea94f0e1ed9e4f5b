"""srgnn.cluster on the device: srg_csr_induced_f32 and induced_subgraph against scipy's A[S][:, S] / A[S] and the
numpy restatement (tests/cluster_ref.py) on a 300-node operator with unsorted rows, duplicates and row lengths on
every edge of the kernel's layout; forged ids; sentinel-guarded outputs; chunked launches; run-to-run identity;
and a ClusterLoader end to end, through GraphConvolution2 and the two-layer GAT, against the same layers on
operators built from scipy's slice."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cluster_ref as CR

pytestmark = pytest.mark.gpu

PAD = 64
SENT_I32, SENT_I64, SENT_F32 = -77, -7777, np.float32(-7.5)
CAPS = (1, 3, 8)


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def fixture():
    """The host arrays, the scipy matrix, the named node sets and the device operator, built once."""
    from srgnn.csr import DeviceCSR
    ip, ix, v = CR.graph()
    A_sp = sp.csr_matrix((v, ix, ip), shape=(CR.N, CR.N))
    A = DeviceCSR.from_tensors(ip, ix, v, n_cols=CR.N, device=dev())
    return ip, ix, v, A_sp, CR.node_sets(ip, ix), A


def guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * PAD,), sentinel, dtype=dtype, device=dev())
    return buf, buf[PAD:PAD + n]


def raw(ip_d, ix_d, v_d, n_rows, n_cols, nodes, relabel, with_val=True, with_eid=True):
    """Both phases of srg_csr_induced_f32 on over-allocated, sentinel-filled buffers; returns host arrays
    (ptr, idx, val or None, eid or None) after checking that nothing outside [0, B) / [0, nnzB) was written."""
    from srgnn import _lib
    d = dev()
    nodes = np.asarray(nodes, dtype=np.int64)
    B = nodes.size
    ids = t(nodes)
    pos = t(CR.pos_of(nodes, n_cols)) if relabel else None
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None   # noqa: E731
    head = (ip_d.data_ptr(), p(ix_d), p(v_d) if with_val else None, n_rows, n_cols, p(ids), B, p(pos))
    cnt_buf, cnt = guarded(B, torch.int64, SENT_I64)
    _lib.call(d, "srg_csr_induced_f32", 0, *head, cnt.data_ptr(), None, None, None, None, _lib.stream(d))
    cnt_h = cnt_buf.cpu().numpy()
    assert (cnt_h[:PAD] == SENT_I64).all() and (cnt_h[PAD + B:] == SENT_I64).all(), "phase 0 wrote outside cnt[0, B)"
    cnt_h = cnt_h[PAD:PAD + B]
    assert (cnt_h >= 0).all()
    ptr = np.concatenate([[0], np.cumsum(cnt_h)]).astype(np.int64)
    nnzB = int(ptr[-1])
    idx_buf, _ = guarded(nnzB, torch.int32, SENT_I32)
    val_buf, _ = guarded(nnzB, torch.float32, float(SENT_F32))
    eid_buf, _ = guarded(nnzB, torch.int64, SENT_I64)
    ptr_d = t(ptr)
    # pointers from the buffers' bases: an empty view has none, and a batch without a kept entry still runs phase 1
    _lib.call(d, "srg_csr_induced_f32", 1, *head, None, ptr_d.data_ptr(), idx_buf.data_ptr() + 4 * PAD,
              val_buf.data_ptr() + 4 * PAD if with_val else None, eid_buf.data_ptr() + 8 * PAD if with_eid else None,
              _lib.stream(d))
    torch.cuda.synchronize()
    out = []
    for buf, sent, used in ((idx_buf, SENT_I32, True), (val_buf, SENT_F32, with_val), (eid_buf, SENT_I64, with_eid)):
        h = buf.cpu().numpy()
        assert (h[:PAD] == sent).all() and (h[PAD + nnzB:] == sent).all(), "phase 1 wrote outside [0, nnzB)"
        if not used:
            assert (h == sent).all(), "an output that was not asked for was written"
        out.append(h[PAD:PAD + nnzB].copy() if used else None)
    return (ptr, *out)


def same(got, want, what):
    g_ptr, g_idx, g_val, g_eid = got
    w_ptr, w_idx, w_val, w_eid = want
    assert np.array_equal(g_ptr, w_ptr), f"{what}: indptr"
    assert np.array_equal(g_idx, w_idx), f"{what}: indices"
    if g_val is not None:
        assert np.array_equal(g_val.view(np.int32), w_val.view(np.int32)), f"{what}: values"
    if g_eid is not None:
        assert np.array_equal(g_eid, w_eid), f"{what}: entry ids"


SETS = CR.SETS


def test_the_fixtures_hold_what_they_say():
    ip, ix, v, A_sp, sets, A = fixture()
    CR.check_fixtures(ip, ix, v, sets)
    assert torch.equal(A.indices.cpu(), torch.from_numpy(ix)) and torch.equal(A.indptr.cpu(), torch.from_numpy(ip))
    assert (np.diff(ix[ip[40]:ip[41]]) < 0).any()                 # stored unsorted on the device too


@pytest.mark.parametrize("relabel", (True, False))
@pytest.mark.parametrize("name", SETS)
def test_entry_equals_scipy_and_the_restatement(name, relabel):
    ip, ix, v, A_sp, sets, A = fixture()
    S = sets[name]
    want = CR.induced(ip, ix, v, CR.N, S, relabel)
    sc = CR.scipy_slice(A_sp, S, relabel)
    assert np.array_equal(want[0], sc[0]) and np.array_equal(want[1], sc[1])
    assert np.array_equal(want[2].view(np.int32), sc[2].astype(np.float32).view(np.int32))
    got = raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, relabel)
    same(got, want, f"{name}, relabel={relabel}")
    ptr, idx, val, eid = got
    assert np.array_equal(val.view(np.int32), v[eid].view(np.int32))
    assert np.array_equal(CR.pos_of(S, CR.N)[ix[eid]] if relabel else ix[eid], idx)
    # without values and without entry ids: the same structure, the other outputs untouched
    same(raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, relabel, with_val=False, with_eid=False), want,
         f"{name}, relabel={relabel}, structure only")
    same(raw(A.indptr, A.indices, None, CR.N, CR.N, S, relabel, with_val=False), want,
         f"{name}, relabel={relabel}, an operator without values")


@pytest.mark.parametrize("relabel,with_eid", ((True, False), (True, True), (False, True)))
@pytest.mark.parametrize("name", SETS)
def test_induced_subgraph_returns_the_slice(name, relabel, with_eid):
    from srgnn import cluster as CL
    ip, ix, v, A_sp, sets, A = fixture()
    S = sets[name]
    w_ptr, w_idx, w_val = CR.scipy_slice(A_sp, S, relabel)
    for nodes in (S, t(S), S.tolist()) if name == "shuffled37" else (S,):
        res = CL.induced_subgraph(A, nodes, relabel=relabel, eid=with_eid)
        sub, ids = res[0], res[1]
        assert sub.n_rows == S.size and sub.n_cols == (S.size if relabel else CR.N) and sub.device == A.device
        assert sub.indptr.dtype == torch.int64 and sub.indices.dtype == torch.int32 and sub.values.dtype == torch.float32
        assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), S)
        assert np.array_equal(sub.indptr.cpu().numpy(), w_ptr) and np.array_equal(sub.indices.cpu().numpy(), w_idx)
        assert np.array_equal(sub.values.cpu().numpy().view(np.int32), w_val.astype(np.float32).view(np.int32))
        if with_eid:
            assert np.array_equal(res[2].cpu().numpy(), CR.induced(ip, ix, v, CR.N, S, relabel)[3])
            assert torch.equal(A.values[res[2]].view(torch.int32), sub.values.view(torch.int32))
    # negative ids wrap as torch indexing does
    if name == "shuffled37":
        sub, ids = CL.induced_subgraph(A, S - CR.N, relabel=relabel)
        assert np.array_equal(ids.cpu().numpy(), S) and np.array_equal(sub.indices.cpu().numpy(), w_idx)


def test_forged_ids_are_dropped_or_copied_and_never_addresses():
    from srgnn.csr import DeviceCSR
    ip, ix, v, A_sp, sets, _ = fixture()
    bad = ix.copy()
    forged = np.array([-1, -5, CR.N, 2 ** 31 - 1, -2 ** 31, CR.N + 7], dtype=np.int32)
    where = np.arange(3, bad.size, 5)
    bad[where] = forged[np.arange(where.size) % forged.size]
    A = DeviceCSR.from_tensors(ip, bad, v, n_cols=CR.N, device=dev(), validate=False)
    for name in ("all", "reversed", "shuffled37", "one"):
        S = sets[name]
        want = CR.induced(ip, bad, v, CR.N, S, True)
        assert ((bad[want[3]] >= 0) & (bad[want[3]] < CR.N)).all() and want[0][-1] < np.diff(ip)[S].sum()
        same(raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, True), want, f"forged, {name}, relabel")
        want = CR.induced(ip, bad, v, CR.N, S, False)
        assert np.array_equal(want[1], bad[want[3]]) and want[0][-1] == np.diff(ip)[S].sum()
        assert np.isin(forged, want[1]).all() or name == "one"
        same(raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, False), want, f"forged, {name}, verbatim")
    # forged node ids: empty rows, both modes (the Python layer raises for them before any launch)
    nodes = np.array([40, -2, CR.N, 2 ** 40, -2 ** 62, 41, 2 ** 31], dtype=np.int64)
    for relabel in (True, False):
        want = CR.induced(ip, bad, v, CR.N, nodes, relabel)
        assert np.diff(want[0])[[1, 2, 3, 4, 6]].sum() == 0 and (want[0][-1] > 0 or relabel)
        same(raw(A.indptr, A.indices, A.values, CR.N, CR.N, nodes, relabel), want, f"forged nodes, relabel={relabel}")


@pytest.mark.parametrize("relabel", (True, False))
@pytest.mark.parametrize("name", ("all", "reversed"))
def test_across_chunks(name, relabel):
    """19 blocks of 16 rows: under a bound of 1, 3 and 8 blocks both phases go out in several launches, each later
    one with its block_base: the unbounded run's bits, with at least twice its chunk launches."""
    from srgnn import _lib
    ip, ix, v, A_sp, sets, A = fixture()
    S = sets[name]
    L = _lib.lib()
    prev = L.srg_debug_launch_cap(0)
    try:
        with _lib.launch_cap(0) as base:
            want = raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, relabel)
        same(want, CR.induced(ip, ix, v, CR.N, S, relabel), "the unbounded run against the restatement")
        assert base.launches == 2, base.launches                   # count, fill
        for cap in CAPS:
            with _lib.launch_cap(cap) as m:
                got = raw(A.indptr, A.indices, A.values, CR.N, CR.N, S, relabel)
            assert L.srg_debug_launch_cap(0) == 0
            assert m.launches >= 2 * base.launches, (cap, m.launches, base.launches)
            assert m.launches == 2 * -(-19 // cap)
            same(got, want, f"{name} under a bound of {cap} blocks ({m.launches} launches)")
    finally:
        L.srg_debug_launch_cap(prev)


def test_two_runs_give_identical_bytes():
    from srgnn import cluster as CL
    ip, ix, v, A_sp, sets, A = fixture()
    for name in ("shuffled37", "reversed"):
        runs = [CL.induced_subgraph(A, sets[name], eid=True) for _ in range(2)]
        (s0, _, e0), (s1, _, e1) = runs
        assert torch.equal(s0.indptr, s1.indptr) and torch.equal(s0.indices, s1.indices) and torch.equal(e0, e1)
        assert torch.equal(s0.values.view(torch.int32), s1.values.view(torch.int32))


# ---- end to end -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def epoch():
    """An R-MAT operator Â of 2,000 nodes, its features, and one shuffled epoch of a ClusterLoader over 8 parts in
    batches of 3, each batch with scipy's slice of the same node list."""
    from srgnn import cluster as CL
    from srgnn import synth
    from srgnn.csr import DeviceCSR
    from srgnn.normalize import sym_norm_binary
    n, d = 2000, 24
    u, v = synth.rmat_undirected_t(n, 9000, seed=synth.RMAT_SEED, device=dev())
    ip, ix = synth.symmetric_csr_t(n, u, v)
    ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
    A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev())
    A_sp = sp.csr_matrix((vals.cpu().numpy(), ix.cpu().numpy(), ip.cpu().numpy()), shape=(n, n))
    x = synth.uniform_features_t(n, d, device=dev())
    rng = np.random.default_rng(12)
    part = rng.integers(0, 8, n)                                   # scattered parts: unsorted node lists
    cd = CL.ClusterData(A, 8, part)
    loader = CL.ClusterLoader(cd, 3, shuffle=True, generator=torch.Generator().manual_seed(5))
    batches = list(loader)
    slices = []
    for b in batches:
        S = b.nodes.cpu().numpy()
        slices.append(A_sp[S][:, S])
    return n, d, A, A_sp, x, part, loader, batches, slices


def test_loader_batches_are_scipy_slices_and_partition_the_nodes():
    n, d, A, A_sp, x, part, loader, batches, slices = epoch()
    assert len(loader) == 3 and [len(b.parts) for b in batches] == [3, 3, 2]
    assert sorted(sum((b.parts for b in batches), [])) == list(range(8))
    nodes = np.concatenate([b.nodes.cpu().numpy() for b in batches])
    assert np.array_equal(np.sort(nodes), np.arange(n))            # every node in exactly one batch
    for b, M in zip(batches, slices):
        S = b.nodes.cpu().numpy()
        assert np.array_equal(S, np.concatenate([np.flatnonzero(part == p) for p in b.parts]))
        assert not np.array_equal(S, np.sort(S)) and b.nodes.device == A.device
        assert b.csr.n_rows == S.size == b.csr.n_cols and M.nnz > 0
        assert np.array_equal(b.csr.indptr.cpu().numpy(), M.indptr)
        assert np.array_equal(b.csr.indices.cpu().numpy(), M.indices)
        assert np.array_equal(b.csr.values.cpu().numpy().view(np.int32), M.data.astype(np.float32).view(np.int32))
        assert torch.equal(A.values[b.eid].view(torch.int32), b.csr.values.view(torch.int32))
        assert torch.equal(b.nodes[b.csr.indices.long()], A.indices[b.eid].long())


def _train_step(model, forward, params_of):
    model.zero_grad(set_to_none=True)
    out = forward()
    G = torch.linspace(-1.0, 1.0, out.numel(), device=out.device).reshape(out.shape)
    (out * G).sum().backward()
    return [out.detach().cpu().numpy()] + [p.grad.detach().cpu().numpy() for p in params_of(model)]


def test_graph_convolution_trains_on_a_batch_as_on_scipys_slice():
    from srgnn.graph_conv import GraphConvolution2, GraphConvOperator
    from srgnn.spmm import gather_rows
    n, d, A, A_sp, x, part, loader, batches, slices = epoch()
    torch.manual_seed(3)
    model = GraphConvolution2(d, 16, 5, dropout=0.0).to(dev())
    used = lambda m: [p for k, p in m.named_parameters() if k.split(".")[0] in ("fc1_node_edge", "fc2_node")]   # noqa: E731
    for b, M in zip(batches, slices):
        xb = gather_rows(x, b.nodes)
        assert torch.equal(xb, x[b.nodes])
        got_op, want_op = b.graph_conv_operator(), GraphConvOperator.from_scipy(M, device=dev())
        assert got_op.transpose_kind == want_op.transpose_kind
        res = []
        for op in (got_op, want_op):
            model.adj = op
            res.append(_train_step(model, lambda: model(xb), used))
        assert len(res[0]) == 5 and np.abs(res[0][1]).sum() > 0
        for g, w in zip(*res):
            assert np.array_equal(g.view(np.int32), w.view(np.int32))


def test_gat_trains_on_a_batch_as_on_scipys_slice():
    from srgnn.gat import GAT, GATGraph
    n, d, A, A_sp, x, part, loader, batches, slices = epoch()
    torch.manual_seed(4)
    model = GAT(d, 8, 5, 2, 0.0, 2).to(dev())
    for b, M in zip(batches, slices):
        xb = x[b.nodes].contiguous()
        got_g, want_g = b.gat_graph(), GATGraph.from_scipy(M, device=dev())
        for k in ("indptr", "indices", "indptr_t", "indices_t", "perm"):
            assert torch.equal(getattr(got_g, k), getattr(want_g, k)), k
        res = [_train_step(model, lambda: model(xb, g), lambda m: list(m.parameters())) for g in (got_g, want_g)]
        assert np.abs(res[0][1]).sum() > 0
        for g, w in zip(*res):
            assert np.array_equal(g.view(np.int32), w.view(np.int32))
