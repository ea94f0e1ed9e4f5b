"""srgnn.neighbor on the device: srg_csr_sample_f32, sample_neighbors, sample_block and NeighborLoader against the
host restatement (tests/neighbor_ref.py) on a 400-node operator with unsorted rows, duplicates and row lengths on
every edge of the kernel's layout, of the copy / sample switch at every fanout and of 4^h; forged node ids and a
ptr that disagrees with the counts; sentinel-guarded outputs; run-to-run identity; and a two-layer loader over an
R-MAT graph, block by block."""
import functools

import numpy as np
import pytest
import torch

import neighbor_ref as NR

pytestmark = pytest.mark.gpu

PAD = 64
SENT_I32, SENT_I64, SENT_F32 = -77, -7777, np.float32(-7.5)


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def fixture():
    """The host arrays, the named node sets and the device operator, built once."""
    from srgnn.csr import DeviceCSR
    ip, ix, v = NR.graph()
    A = DeviceCSR.from_tensors(ip, ix, v, n_cols=NR.N, device=dev())
    return ip, ix, v, NR.node_sets(ip), A


@functools.lru_cache(maxsize=None)
def want_of(name, fanout, seed):
    """The restatement's (ptr, idx, val, eid) of a named node set: computed once, shared, never written to."""
    ip, ix, v, sets, _ = fixture()
    return NR.sample(ip, ix, v, sets[name], fanout, seed)


def counts(ip, nodes, fanout):
    lens = np.diff(ip)
    return np.array([NR.count_of(int(lens[r]), fanout) if 0 <= r < lens.size else 0 for r in np.asarray(nodes).tolist()],
                    dtype=np.int64)


def raw(A, nodes, fanout, seed, with_val=True, with_eid=True, ptr=None, values=True):
    """srg_csr_sample_f32 on over-allocated, sentinel-filled buffers; returns host arrays (ptr, idx, val or None,
    eid or None), unwritten slots still holding their sentinel, after checking that nothing outside [0, ptr[B])
    was written.  ptr None: the prefix sum of the closed-form counts."""
    from srgnn import _lib
    d = dev()
    nodes = np.asarray(nodes, dtype=np.int64)
    B = nodes.size
    if ptr is None:
        ptr = np.concatenate([[0], np.cumsum(counts(A.indptr.cpu().numpy(), nodes, fanout))]).astype(np.int64)
    nnzB = int(ptr[-1])
    ids, ptr_d = t(nodes), t(ptr)
    bufs = [torch.full((nnzB + 2 * PAD,), s, dtype=dt, device=d)
            for s, dt in ((SENT_I32, torch.int32), (float(SENT_F32), torch.float32), (SENT_I64, torch.int64))]
    p = lambda x: x.data_ptr() if x is not None and x.numel() else None   # noqa: E731
    _lib.call(d, "srg_csr_sample_f32", A.indptr.data_ptr(), p(A.indices), p(A.values) if values else None, A.n_rows,
              p(ids), B, fanout, seed, ptr_d.data_ptr(), bufs[0].data_ptr() + 4 * PAD,
              bufs[1].data_ptr() + 4 * PAD if with_val else None, bufs[2].data_ptr() + 8 * PAD if with_eid else None,
              _lib.stream(d))
    torch.cuda.synchronize()
    out = []
    for buf, sent, used in zip(bufs, (SENT_I32, SENT_F32, SENT_I64), (True, with_val, with_eid)):
        h = buf.cpu().numpy()
        assert (h[:PAD] == sent).all() and (h[PAD + nnzB:] == sent).all(), "wrote outside [0, ptr[B])"
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


def test_the_fixtures_hold_what_they_say():
    ip, ix, v, sets, A = fixture()
    NR.check_fixtures(ip, ix, v, sets)
    assert torch.equal(A.indices.cpu(), torch.from_numpy(ix)) and torch.equal(A.indptr.cpu(), torch.from_numpy(ip))


@pytest.mark.parametrize("fanout", NR.FANOUTS)
@pytest.mark.parametrize("name", NR.SETS)
def test_entry_equals_the_restatement(name, fanout):
    ip, ix, v, sets, A = fixture()
    S = sets[name]
    for seed in NR.SEEDS:
        want = want_of(name, fanout, seed)
        got = raw(A, S, fanout, seed)
        same(got, want, f"{name}, fanout={fanout}, seed={seed}")
        assert np.array_equal(got[2].view(np.int32), v[got[3]].view(np.int32)) and np.array_equal(got[1], ix[got[3]])
    # without values and without entry ids: the same structure, the other outputs untouched
    seed = NR.SEEDS[1]
    want = want_of(name, fanout, seed)
    same(raw(A, S, fanout, seed, with_val=False, with_eid=False), want, f"{name}, fanout={fanout}, structure only")
    same(raw(A, S, fanout, seed, with_val=False, values=False), want, f"{name}, fanout={fanout}, no values")
    same(raw(A, S, fanout, seed, with_eid=False), want, f"{name}, fanout={fanout}, no entry ids")


@pytest.mark.parametrize("fanout", (2, 25, 64, -1))
def test_forged_node_ids_are_empty_rows_and_never_addresses(fanout):
    ip, ix, v, sets, A = fixture()
    lens = np.diff(ip)
    r1, r2 = (int(np.flatnonzero(lens == k)[0]) for k in (129, 11))
    nodes = np.array([r1, -1, NR.N, 2 ** 62, -2 ** 63, r2, 2 ** 31], dtype=np.int64)
    want = NR.sample(ip, ix, v, nodes, fanout, 9)
    assert np.diff(want[0])[[1, 2, 3, 4, 6]].sum() == 0 and want[0][-1] == sum(NR.count_of(k, fanout) for k in (129, 11))
    same(raw(A, nodes, fanout, 9), want, f"forged nodes, fanout={fanout}")


@pytest.mark.parametrize("fanout", (10, -1))
@pytest.mark.parametrize("delta", (1, -1))
def test_a_row_whose_ptr_disagrees_with_its_count_is_not_written(fanout, delta):
    """One row's slot is one entry too long or too short, the rows after it shifted: every other row is written
    at its shifted place, the forged row's slots keep their sentinels, and so do the guards."""
    ip, ix, v, sets, A = fixture()
    lens = np.diff(ip)
    for length in (3, 25, 1025):                          # a group's copy, a group's copy / a sampled row, a wave's row
        S = sets["all"]
        bad = int(np.flatnonzero(lens[S] == length)[0])
        want = want_of("all", fanout, 4)
        ptr = want[0].copy()
        ptr[bad + 1:] += delta
        g_ptr, g_idx, g_val, g_eid = raw(A, S, fanout, 4, ptr=ptr)
        for b in range(S.size):
            lo, hi = int(ptr[b]), int(ptr[b + 1])
            if b == bad:
                assert (g_idx[lo:hi] == SENT_I32).all() and (g_val[lo:hi] == SENT_F32).all() and (g_eid[lo:hi] == SENT_I64).all()
            else:
                w = slice(int(want[0][b]), int(want[0][b + 1]))
                assert np.array_equal(g_idx[lo:hi], want[1][w]) and np.array_equal(g_eid[lo:hi], want[3][w])
                assert np.array_equal(g_val[lo:hi].view(np.int32), want[2][w].view(np.int32))


@pytest.mark.parametrize("fanout", (10, 64, -1))
def test_sample_neighbors_returns_the_sampled_slice(fanout):
    from srgnn import neighbor as NB
    ip, ix, v, sets, A = fixture()
    for name in NR.SETS:
        S = sets[name]
        want = want_of(name, fanout, NR.SEEDS[1])
        for nodes in (S, t(S), S.tolist(), S - NR.N) if name == "shuffled37" else (S,):
            sub, ids, eid = NB.sample_neighbors(A, nodes, fanout, NR.SEEDS[1], eid=True)
            assert sub.n_rows == S.size and sub.n_cols == NR.N and sub.device == A.device
            assert sub.indptr.dtype == torch.int64 and sub.indices.dtype == torch.int32 and sub.values.dtype == torch.float32
            assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), S)
            same((sub.indptr.cpu().numpy(), sub.indices.cpu().numpy(), sub.values.cpu().numpy(), eid.cpu().numpy()),
                 want, f"{name}, fanout={fanout}")
            sub2, _ = NB.sample_neighbors(A, nodes, fanout, NR.SEEDS[1])
            assert torch.equal(sub2.indices, sub.indices) and torch.equal(sub2.indptr, sub.indptr)
    # a seed outside [0, 2^64) is taken mod 2^64
    a = NB.sample_neighbors(A, sets["long_rows"], 10, -1)[0]
    b = NB.sample_neighbors(A, sets["long_rows"], 10, 2 ** 64 - 1)[0]
    assert torch.equal(a.indices, b.indices)


def test_two_runs_give_identical_bytes():
    from srgnn import neighbor as NB
    ip, ix, v, sets, A = fixture()
    for name in ("shuffled37", "reversed"):
        runs = [NB.sample_neighbors(A, sets[name], 10, 77, eid=True) for _ in range(2)]
        (s0, _, e0), (s1, _, e1) = runs
        assert torch.equal(s0.indptr, s1.indptr) and torch.equal(s0.indices, s1.indices) and torch.equal(e0, e1)
        assert torch.equal(s0.values.view(torch.int32), s1.values.view(torch.int32))


# ---- blocks and the loader --------------------------------------------------------------------------
def check_block(blk, want, A, what):
    ptr, cols, val, n_id, eid = want
    assert blk.n_dst == ptr.size - 1 and np.array_equal(blk.n_id.cpu().numpy(), n_id), f"{what}: n_id"
    assert blk.n_id.dtype == torch.int64 and blk.csr.indices.dtype == torch.int32
    assert blk.csr.n_rows == blk.n_dst and blk.csr.n_cols == n_id.size, f"{what}: shape"
    assert np.array_equal(blk.csr.indptr.cpu().numpy(), ptr) and np.array_equal(blk.csr.indices.cpu().numpy(), cols), what
    assert np.array_equal(blk.csr.values.cpu().numpy().view(np.int32), val.view(np.int32)), f"{what}: values"
    assert np.array_equal(blk.eid.cpu().numpy(), eid), f"{what}: entry ids"
    assert torch.equal(blk.n_id[blk.csr.indices.long()], A.indices[blk.eid].long())
    sq = blk.square_csr()
    assert sq.n_rows == sq.n_cols == n_id.size and sq.indptr.numel() == n_id.size + 1
    assert torch.equal(sq.indptr[:ptr.size], blk.csr.indptr) and bool((sq.indptr[ptr.size:] == int(ptr[-1])).all())


@pytest.mark.parametrize("fanout", (2, 10, -1))
def test_sample_block_puts_the_targets_first_and_the_frontier_ascending(fanout):
    from srgnn import neighbor as NB
    ip, ix, v, sets, A = fixture()
    for name in NR.SETS:
        S = sets[name]
        blk = NB.sample_block(A, S, fanout, 21)
        check_block(blk, NR.block(ip, ix, v, NR.N, S, fanout, 21), A, f"{name}, fanout={fanout}")
        assert torch.equal(blk.n_id[:S.size].cpu(), torch.from_numpy(S))


def test_sample_block_rejects_a_forged_column_before_it_indexes_with_it():
    from srgnn import neighbor as NB
    from srgnn.csr import DeviceCSR
    ip, ix, v, sets, _ = fixture()
    for forged in (-1, NR.N, 2 ** 31 - 1, -2 ** 31):
        bad = ix.copy()
        r = int(np.flatnonzero(np.diff(ip) == 3)[0])
        bad[ip[r] + 1] = forged
        A = DeviceCSR.from_tensors(ip, bad, v, n_cols=NR.N, device=dev(), validate=False)
        with pytest.raises(ValueError, match="outside"):
            NB.sample_block(A, [r, (r + 1) % NR.N], 10, 0)
        sub, _ = NB.sample_neighbors(A, [r], 10, 0)            # the row slice copies it verbatim
        assert sub.indices.cpu().tolist() == bad[ip[r]:ip[r + 1]].tolist()


@functools.lru_cache(maxsize=None)
def rmat():
    """An R-MAT operator Â of 2,000 nodes on the device and on the host."""
    from srgnn import synth
    from srgnn.csr import DeviceCSR
    from srgnn.normalize import sym_norm_binary
    n = 2000
    u, v = synth.rmat_undirected_t(n, 9000, seed=synth.RMAT_SEED, device=dev())
    ip, ix = synth.symmetric_csr_t(n, u, v)
    ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
    A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev())
    return n, A, ip.cpu().numpy(), ix.cpu().numpy(), vals.cpu().numpy()


def test_a_two_layer_loader_yields_the_restatements_blocks():
    from srgnn import neighbor as NB
    n, A, ip, ix, vals = rmat()
    assert np.diff(ip).max() > 10, "some row must be cut"
    idx = torch.from_numpy(np.random.default_rng(3).permutation(n)[:170])
    loader = NB.NeighborLoader(A, idx, [10, 5], 50, shuffle=True, generator=torch.Generator().manual_seed(5), seed=99)
    assert len(loader) == 4
    g = torch.Generator().manual_seed(5)
    orders = [idx[torch.randperm(170, generator=g)] for _ in range(2)]      # a new permutation per epoch
    for epoch, order in enumerate(orders):
        batches = list(loader)
        assert [b.batch_size for b in batches] == [50, 50, 50, 20]
        for i, b in enumerate(batches):
            seeds = order[50 * i:50 * i + 50].numpy()
            w_n_id, w_blocks = NR.loader_batch(ip, ix, vals, n, seeds, [10, 5], 99, epoch, i)
            assert len(b.blocks) == 2 and np.array_equal(b.n_id.cpu().numpy(), w_n_id)
            assert np.array_equal(b.n_id[:b.batch_size].cpu().numpy(), seeds)
            for l, (blk, want) in enumerate(zip(b.blocks, w_blocks)):
                check_block(blk, want, A, f"epoch {epoch}, batch {i}, block {l}")
            # targets first: a block's sources are the next block's targets, the outermost's are the batch's n_id
            assert torch.equal(b.blocks[0].n_id, b.n_id) and b.blocks[1].n_dst == b.batch_size
            assert torch.equal(b.blocks[0].n_id[:b.blocks[0].n_dst], b.blocks[1].n_id)
            assert b.blocks[0].csr.n_rows == b.blocks[1].csr.n_cols
            # the outer layer was cut to 5 and the inner to 10
            assert int((b.blocks[0].csr.indptr[1:] - b.blocks[0].csr.indptr[:-1]).max()) == 5
            assert int((b.blocks[1].csr.indptr[1:] - b.blocks[1].csr.indptr[:-1]).max()) <= 10

