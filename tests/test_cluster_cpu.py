"""srgnn.cluster without a device: the numpy restatement (tests/cluster_ref.py) against scipy's own slicing,
induced_subgraph's argument checks, the C entry's checks that return before a launch, ClusterData's partition
arrays and ClusterLoader's epochs."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cluster_ref as CR
from srgnn import _lib
from srgnn import cluster as CL
from srgnn.csr import DeviceCSR


def host_csr(indptr, indices, values, n_cols=None):
    """A DeviceCSR over host tensors: enough for everything that returns before a launch."""
    ip, ix, v = torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(values)
    return DeviceCSR(ip, ix, v, ip.numel() - 1, ip.numel() - 1 if n_cols is None else n_cols, None, None, None, None)


# ---- the restatement against scipy ------------------------------------------------------------------
def test_the_gpu_tests_fixtures_hold_what_they_say():
    ip, ix, v = CR.graph()
    CR.check_fixtures(ip, ix, v, CR.node_sets(ip, ix))



@pytest.mark.parametrize("relabel", (True, False))
def test_restatement_equals_scipy_bit_for_bit(relabel):
    ip, ix, v = CR.graph()
    assert (np.diff(ix[ip[40]:ip[41]]) < 0).any(), "the rows are meant to be unsorted"
    assert any(np.unique(ix[ip[r]:ip[r + 1]]).size < ip[r + 1] - ip[r] for r in range(CR.N)), "and to hold duplicates"
    A = sp.csr_matrix((v, ix, ip), shape=(CR.N, CR.N))
    sets = CR.node_sets(ip, ix)
    assert not np.array_equal(sets["shuffled37"], np.sort(sets["shuffled37"]))
    for name, S in sets.items():
        ptr, idx, val, eid = CR.induced(ip, ix, v, CR.N, S, relabel)
        w_ptr, w_idx, w_val = CR.scipy_slice(A, S, relabel)
        assert np.array_equal(ptr, w_ptr) and np.array_equal(idx, w_idx), name
        assert np.array_equal(val.view(np.int32), w_val.astype(np.float32).view(np.int32)), name
        assert np.array_equal(val.view(np.int32), v[eid].view(np.int32))
        if relabel:
            assert np.array_equal(CR.pos_of(S, CR.N)[ix[eid]], idx), name
        else:
            assert np.array_equal(ix[eid], idx), name


def test_restatement_on_a_rectangular_slice_and_forged_ids():
    rng = np.random.default_rng(2)
    n, m = 20, 35
    lens = rng.integers(0, 9, n)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ix = rng.integers(0, m, int(ip[-1])).astype(np.int32)
    v = rng.standard_normal(ix.size).astype(np.float32)
    S = rng.permutation(n)[:11]
    ptr, idx, val, _ = CR.induced(ip, ix, v, m, S, relabel=False)
    w = CR.scipy_slice(sp.csr_matrix((v, ix, ip), shape=(n, m)), S, relabel=False)
    assert np.array_equal(ptr, w[0]) and np.array_equal(idx, w[1]) and np.array_equal(val, w[2])
    # forged ids: dropped under relabel, copied verbatim without; a forged node is an empty row
    bad = ix.copy()
    bad[::5] = np.array([-1, -5, n, 2 ** 31 - 1], dtype=np.int32)[np.arange(bad[::5].size) % 4]
    nodes = np.array([3, -2, n, 7], dtype=np.int64)
    ptr, idx, _, eid = CR.induced(ip, bad, v, n, nodes, relabel=True)
    assert ((idx >= 0) & (idx < nodes.size)).all() and ptr[2] == ptr[1] and ptr[3] == ptr[2]
    assert ((bad[eid] >= 0) & (bad[eid] < n)).all()
    ptr, idx, _, eid = CR.induced(ip, bad, v, n, nodes, relabel=False)
    assert np.array_equal(idx, bad[eid]) and ptr[-1] == lens[3] + lens[7]


# ---- induced_subgraph's checks ----------------------------------------------------------------------
def test_induced_subgraph_checks_its_arguments_before_the_device():
    ip, ix, v = CR.graph()
    A, n = host_csr(ip, ix, v), CR.N
    with pytest.raises(IndexError):
        CL.induced_subgraph(A, [0, n])
    with pytest.raises(IndexError):
        CL.induced_subgraph(A, torch.tensor([-n - 1]))
    with pytest.raises(TypeError, match="integer"):
        CL.induced_subgraph(A, torch.tensor([0.0, 1.0]))
    with pytest.raises(TypeError, match="integer"):
        CL.induced_subgraph(A, torch.tensor([True, False]))
    with pytest.raises(ValueError, match="1-D"):
        CL.induced_subgraph(A, torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="repeats"):
        CL.induced_subgraph(A, [4, 9, 4])
    with pytest.raises(ValueError, match="repeats"):
        CL.induced_subgraph(A, [4, 4 - n], relabel=False)
    with pytest.raises(TypeError, match="DeviceCSR"):
        CL.induced_subgraph(sp.csr_matrix((v, ix, ip), shape=(n, n)), [0])
    wide = host_csr(ip, ix, v, n_cols=n + 5)
    with pytest.raises(ValueError, match="square"):
        CL.induced_subgraph(wide, [0, 1])
    # good ids of every accepted kind reach the device check: no fall-back to the host
    for nodes in ([0, 3], range(0, 10, 2), torch.tensor([1, -1]), np.array([2, 5]), torch.tensor([4], dtype=torch.int32), []):
        with pytest.raises(RuntimeError, match="HIP device"):
            CL.induced_subgraph(A, nodes)
    with pytest.raises(RuntimeError, match="HIP device"):
        CL.induced_subgraph(wide, [0, 1], relabel=False, eid=True)


def test_entry_is_bound_and_rejects_bad_sizes_before_a_launch():
    L = _lib.lib()
    E = _lib.SRG_ERR_INVALID
    assert "srg_csr_induced_f32" in _lib.EXPORTED_SYMBOLS

    def call(phase=0, n_rows=4, n_cols=4, B=2, cnt=None, nodes=None):
        return L.srg_csr_induced_f32(phase, None, None, None, n_rows, n_cols, nodes, B, None, cnt, None, None, None,
                                     None, None)

    assert call(phase=2) == E and "phase 2" in _lib.last_error()
    assert call(phase=-1) == E
    assert call(n_cols=2 ** 31) == E and "n_cols" in _lib.last_error()
    assert call(n_cols=2 ** 40) == E
    assert call(B=2 ** 31) == E and "B=" in _lib.last_error()
    assert call(n_rows=-1) == E and call(n_cols=-1) == E and call(B=-1) == E
    assert "negative" in _lib.last_error()
    assert call() == E and "null" in _lib.last_error()
    assert call(phase=1, nodes=ctypes.c_void_p(16)) == E and "null" in _lib.last_error()   # nothing to fill
    assert call(B=0) == _lib.SRG_OK and call(phase=1, B=0) == _lib.SRG_OK                   # launches nothing
    assert L.srg_last_error_code() == _lib.SRG_OK


# ---- ClusterData ------------------------------------------------------------------------------------
def test_cluster_data_builds_partptr_and_perm():
    ip, ix, v = CR.graph()
    A, n = host_csr(ip, ix, v), CR.N
    rng = np.random.default_rng(3)
    P = 9
    part = rng.integers(0, P, n)
    part[part == 4] = 5          # part 4 is empty
    part[part == 0] = 1          # and so is the first
    cd = CL.ClusterData(A, P, part)
    assert cd.partptr.dtype == torch.int64 and cd.perm.dtype == torch.int64 and len(cd) == P
    assert cd.partptr.tolist() == np.concatenate([[0], np.cumsum(np.bincount(part, minlength=P))]).tolist()
    assert cd.perm.tolist() == np.argsort(part, kind="stable").tolist()
    bounds = cd.partptr.tolist()
    assert bounds[0] == 0 and bounds[1] == 0 and bounds[5] == bounds[4] and bounds[-1] == n
    for p in range(P):
        mine = cd.perm[bounds[p]:bounds[p + 1]].numpy()
        assert (part[mine] == p).all() and (np.diff(mine) > 0).all()      # stable: increasing ids inside a part
    assert cd.nodes_of([5, 1]).tolist() == np.concatenate([np.flatnonzero(part == 5), np.flatnonzero(part == 1)]).tolist()
    assert cd.nodes_of([]).numel() == 0 and cd.nodes_of([4, 0]).numel() == 0
    # the same from a tensor and a list
    assert torch.equal(CL.ClusterData(A, P, torch.from_numpy(part).to(torch.int32)).perm, cd.perm)
    assert torch.equal(CL.ClusterData(A, P, part.tolist()).partptr, cd.partptr)


def test_cluster_data_rejects_a_bad_part():
    ip, ix, v = CR.graph()
    A, n = host_csr(ip, ix, v), CR.N
    with pytest.raises(ValueError, match="assignment"):
        CL.ClusterData(A, 4, np.zeros(n - 1, dtype=np.int64))
    with pytest.raises(ValueError, match="assignment"):
        CL.ClusterData(A, 4, np.zeros((n, 1), dtype=np.int64))
    bad = np.zeros(n, dtype=np.int64)
    bad[7] = 4
    with pytest.raises(ValueError, match="outside"):
        CL.ClusterData(A, 4, bad)
    bad[7] = -1
    with pytest.raises(ValueError, match="outside"):
        CL.ClusterData(A, 4, bad)
    with pytest.raises(TypeError, match="integer"):
        CL.ClusterData(A, 4, np.zeros(n))
    with pytest.raises(TypeError, match="integer"):
        CL.ClusterData(A, 4, np.zeros(n, dtype=bool))
    with pytest.raises(ValueError, match="num_parts"):
        CL.ClusterData(A, 0)
    with pytest.raises(ValueError, match="square"):
        CL.ClusterData(host_csr(ip, ix, v, n_cols=n + 1), 4)
    with pytest.raises(TypeError):
        CL.ClusterData(np.zeros((3, 3)), 2)


@pytest.mark.parametrize("P", (1, 7, 128, 301))
def test_default_partition_is_contiguous_blocks_covering_every_node_once(P):
    ip, ix, v = CR.graph()
    A, n = host_csr(ip, ix, v), CR.N
    cd = CL.ClusterData(A, P)
    assert cd.perm.tolist() == list(range(n))                     # contiguous blocks in row order
    assert (np.diff(cd.part.numpy()) >= 0).all() and cd.partptr[-1] == n and cd.part.numel() == n
    w = np.diff(ip) + 1                                           # the weight that is balanced: rows + entries
    load = np.array([w[cd.partptr[p]:cd.partptr[p + 1]].sum() for p in range(P)])
    assert load.sum() == w.sum() and load.max() <= w.sum() / P + w.max()


# ---- ClusterLoader ----------------------------------------------------------------------------------
def test_loader_epochs_visit_every_part_once():
    ip, ix, v = CR.graph()
    A = host_csr(ip, ix, v)
    cd = CL.ClusterData(A, 10)
    for bs, want_len in ((3, 4), (5, 2), (10, 1), (16, 1), (1, 10)):
        plain = CL.ClusterLoader(cd, bs, shuffle=False)
        assert len(plain) == want_len
        batches = plain.part_batches()
        assert len(batches) == want_len and sum(batches, []) == list(range(10))
        assert all(len(b) == bs for b in batches[:-1]) and len(batches[-1]) == 10 - bs * (want_len - 1)
        g = torch.Generator().manual_seed(11)
        shuffled = CL.ClusterLoader(cd, bs, shuffle=True, generator=g)
        e1, e2 = shuffled.part_batches(), shuffled.part_batches()
        for e in (e1, e2):
            assert len(e) == want_len and sorted(sum(e, [])) == list(range(10))
            assert len(e[-1]) == 10 - bs * (want_len - 1)
        assert sum(e1, []) != sum(e2, [])                             # a new permutation per epoch
        again = CL.ClusterLoader(cd, bs, shuffle=True, generator=torch.Generator().manual_seed(11))
        assert again.part_batches() == e1 and again.part_batches() == e2
        assert sum(e1, []) == torch.randperm(10, generator=torch.Generator().manual_seed(11)).tolist()
    # a batch's node list is its parts' nodes, part after part; building the batch needs the device
    loader = CL.ClusterLoader(cd, 3, shuffle=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        next(iter(loader))
    with pytest.raises(ValueError, match="batch_size"):
        CL.ClusterLoader(cd, 0)
    with pytest.raises(TypeError):
        CL.ClusterLoader(A, 2)
