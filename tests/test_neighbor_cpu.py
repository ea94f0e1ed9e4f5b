"""srgnn.neighbor without a device: the restatement (tests/neighbor_ref.py) against scipy's row slice where
nothing is cut, the sampled rows' shape, the walk's bound, the shared helper as the host compiles it
(tests/sample_perm_main.cpp) against the restatement, the uniformity of the restatement's draws, the Python
functions' argument checks up to the device check, and the C entry's checks that return before a launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_augment_ref as ER
import neighbor_ref as NR
from srgnn import _lib
from srgnn import neighbor as NB
from srgnn.csr import DeviceCSR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def host_csr(indptr, indices, values, n_cols=None):
    """A DeviceCSR over host tensors: enough for everything that returns before a launch."""
    ip, ix, v = torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(values)
    return DeviceCSR(ip, ix, v, ip.numel() - 1, ip.numel() - 1 if n_cols is None else n_cols, None, None, None, None)


# ---- the restatement ----------------------------------------------------------------------------------
def test_the_gpu_tests_fixtures_hold_what_they_say():
    ip, ix, v = NR.graph()
    NR.check_fixtures(ip, ix, v, NR.node_sets(ip))
    assert len(set(NR.SEEDS)) == 3 and 0 in NR.SEEDS and 2 ** 64 - 1 in NR.SEEDS


@pytest.mark.parametrize("fanout", (-1, -7, 64))
def test_without_a_cut_the_restatement_is_scipys_row_slice(fanout):
    ip, ix, v = NR.graph()
    if fanout > 0:                                   # every row at most fanout long: drop the long rows' entries
        lens = np.minimum(np.diff(ip), fanout)
        keep = np.concatenate([np.arange(ip[r], ip[r] + lens[r]) for r in range(NR.N)])
        ip, ix, v = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), ix[keep], v[keep]
        assert np.diff(ip).max() == fanout
    A = sp.csr_matrix((v, ix, ip), shape=(NR.N, NR.N))
    for name, S in NR.node_sets(NR.graph()[0]).items():
        ptr, idx, val, eid = NR.sample(ip, ix, v, S, fanout, 5)
        M = A[S]
        assert np.array_equal(ptr, M.indptr) and np.array_equal(idx, M.indices), name
        assert np.array_equal(val.view(np.int32), M.data.astype(np.float32).view(np.int32)), name
        assert np.array_equal(eid, np.concatenate([np.arange(ip[r], ip[r + 1]) for r in S] + [np.zeros(0, np.int64)]))


@pytest.mark.parametrize("fanout", [f for f in NR.FANOUTS if f > 0])
def test_sampled_rows_hold_fanout_distinct_ascending_positions_of_their_row(fanout):
    ip, ix, v = NR.graph()
    lens = np.diff(ip)
    S = NR.node_sets(ip)["shuffled37"]
    for seed in NR.SEEDS:
        ptr, idx, val, eid = NR.sample(ip, ix, v, S, fanout, seed)
        assert np.array_equal(np.diff(ptr), np.where(lens[S] <= fanout, lens[S], fanout))
        assert np.array_equal(idx, ix[eid]) and np.array_equal(val.view(np.int32), v[eid].view(np.int32))
        for b, r in enumerate(S.tolist()):
            e = eid[ptr[b]:ptr[b + 1]]
            assert (np.diff(e) > 0).all() and (e.size == 0 or (ip[r] <= e[0] and e[-1] < ip[r + 1]))
            if lens[r] <= fanout:
                assert np.array_equal(e, np.arange(ip[r], ip[r + 1]))
    # a node's sample does not depend on the batch it is in, and does depend on the seed and on the node
    r = int(np.flatnonzero(lens == 1025)[0])
    alone = NR.sample(ip, ix, v, [r], fanout, 3)[3]
    ptr, _, _, eid = NR.sample(ip, ix, v, S, fanout, 3)
    b = S.tolist().index(r)
    assert np.array_equal(alone, eid[ptr[b]:ptr[b + 1]])
    assert not np.array_equal(alone, NR.sample(ip, ix, v, [r], fanout, 4)[3])
    assert NR.positions(3, r, 1025, fanout) != NR.positions(3, r + 1, 1025, fanout)


def test_forged_nodes_are_empty_rows():
    ip, ix, v = NR.graph()
    r = int(np.flatnonzero(np.diff(ip) == 129)[0])
    ptr, idx, _, _ = NR.sample(ip, ix, v, [-1, r, NR.N, 2 ** 62, -2 ** 63], 10, 1)
    assert ptr.tolist() == [0, 0, 10, 10, 10, 10] and idx.size == 10


def test_the_draw_is_the_edge_augmentation_samplers_bijection():
    """Row 0 of srg_sample_distinct_i64 over n nodes with a query node past every draw (no shift) is the walk
    over m = n - 1 under node 0's key; and the two restatements here agree."""
    for m, k, seed in ((37, 10, 5), (1025, 64, 2 ** 64 - 1), (4, 3, 0), (155868, 25, 77)):
        want = ER.sample_distinct([m], [0, k], m + 1, seed).tolist()
        assert NR.draws_int(seed, 0, m, k) == want
        assert NR.draws_many([seed], [0], m, k)[0].tolist() == want
    assert NR.draws_many([1, 2, 3], [9], 65, 64).tolist() == [NR.draws_int(s, 9, 65, 64) for s in (1, 2, 3)]
    assert NR.draws_many([8], [0, 2 ** 40], 17, 16).tolist() == [NR.draws_int(8, u, 17, 16) for u in (0, 2 ** 40)]


PERM_M = (2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 1024, 1025, 155868)


def test_the_shared_helper_on_the_host_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "sample_perm_main")
    # the header holds device code as well: compiled as HIP, for a named target (no search for a GPU)
    build = subprocess.run([HIPCC, "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                            "-I", os.path.join(REPO, "scalable-roubust-gnn_amd", "csrc"), "-o", exe,
                            os.path.join(HERE, "sample_perm_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    cases = []
    for i, m in enumerate(PERM_M):
        for seed, v in ((0, 0), (2 ** 64 - 1, 7), (0x1234567 * (i + 1) + 11, 2 ** 40 + i), (5, 2 ** 63 - 1)):
            for k in sorted({1, min(m - 1, 10), min(m - 1, 64), min(m, 64)}):
                cases.append((seed, v, m, k))
    cases.append((9, 3, 155868, 2000))
    text = "".join(f"{s} {v} {m} {k}\n" for s, v, m, k in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) and "failed" not in run.stdout
    for (s, v, m, k), ln in zip(cases, lines):
        got = [int(x) for x in ln.split()]
        assert got == NR.draws_int(s, v, m, k), (s, v, m, k)
        assert len(set(got)) == k and max(got) < m


# ---- uniformity of the restatement ------------------------------------------------------------------
def _within_six_sigma(draws, m, k):
    S = draws.shape[0]
    assert draws.shape == (S, k) and (np.sort(draws, axis=1)[:, 1:] != np.sort(draws, axis=1)[:, :-1]).all()
    counts = np.bincount(draws.reshape(-1).astype(np.int64), minlength=m)
    p = k / m
    band = 6.0 * np.sqrt(S * p * (1.0 - p))
    worst = np.abs(counts - S * p).max()
    assert counts.size == m and worst <= band, (m, k, S, worst, band)


@pytest.mark.parametrize("m,k,S", ((37, 10, 4096), (5, 1, 4096), (17, 16, 4096), (65, 64, 2048), (257, 10, 8192),
                                   (1025, 25, 8192), (3, 2, 4096), (2, 1, 4096)))
def test_every_position_is_included_equally_often_over_seeds(m, k, S):
    seeds = [(s * 0x1234567 + 11) & NR.M64 for s in range(S)]
    _within_six_sigma(NR.draws_many(seeds, [7], m, k), m, k)


def test_every_position_is_included_equally_often_over_small_seeds_and_over_nodes():
    _within_six_sigma(NR.draws_many(np.arange(4096), [7], 37, 10), 37, 10)
    _within_six_sigma(NR.draws_many([5], np.arange(4096), 37, 10), 37, 10)


# ---- block, frontier and the loader's seeds ---------------------------------------------------------
def test_block_puts_targets_first_and_the_frontier_ascending():
    ip, ix, v = NR.graph()
    S = NR.node_sets(ip)["shuffled37"]
    ptr, cols, val, n_id, eid = NR.block(ip, ix, v, NR.N, S, 10, 21)
    assert np.array_equal(n_id[:S.size], S) and (np.diff(n_id[S.size:]) > 0).all()
    assert np.unique(n_id).size == n_id.size and not np.isin(n_id[S.size:], S).any()
    assert np.array_equal(n_id[cols], ix[eid]) and cols.max() < n_id.size
    assert set(n_id[S.size:].tolist()) == set(ix[eid].tolist()) - set(S.tolist())


def test_loader_seeds_differ_between_layers_batches_and_epochs():
    seen = {NR.layer_seed(s, e, b, l) for s in (0, 2 ** 64 - 1) for e in range(4) for b in range(50) for l in range(6)}
    assert len(seen) == 2 * 4 * 50 * 6
    assert NR.layer_seed(2 ** 64 - 1, 0, 0, 0) == (NR.EPOCH_MUL + NR.BATCH_MUL + NR.LAYER_MUL - 1) % 2 ** 64
    for args in ((0, 0, 0, 0), (77, 3, 12, 1), (2 ** 64 - 1, 9, 0, 2), (-5, 1, 1, 1)):
        assert NB.layer_seed(*args) == NR.layer_seed(*args)
    assert NR.EPOCH_MUL % 2 == NR.BATCH_MUL % 2 == NR.LAYER_MUL % 2 == 1


def test_loader_epochs_visit_every_seed_node_once():
    ip, ix, v = NR.graph()
    A = host_csr(ip, ix, v)
    idx = torch.arange(0, NR.N, 3)
    for bs, want_len in ((50, 3), (134, 1), (1, 134), (67, 2)):
        plain = NB.NeighborLoader(A, idx, [10, 5], bs, shuffle=False)
        assert len(plain) == want_len and torch.equal(torch.cat(plain.seed_batches()), idx)
        g = torch.Generator().manual_seed(11)
        shuffled = NB.NeighborLoader(A, idx, [10, 5], bs, shuffle=True, generator=g)
        e1, e2 = torch.cat(shuffled.seed_batches()), torch.cat(shuffled.seed_batches())
        assert torch.equal(e1.sort().values, idx) and torch.equal(e2.sort().values, idx) and not torch.equal(e1, e2)
        assert torch.equal(e1, idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(11))])
        assert [b.numel() for b in shuffled.seed_batches()][:-1] == [bs] * (want_len - 1)
    assert len(NB.NeighborLoader(A, None, [3], 128)) == 4
    with pytest.raises(RuntimeError, match="HIP device"):
        next(iter(NB.NeighborLoader(A, idx, [10, 5], 50, shuffle=False)))
    with pytest.raises(ValueError, match="batch_size"):
        NB.NeighborLoader(A, idx, [10], 0)
    with pytest.raises(ValueError, match="fanout"):
        NB.NeighborLoader(A, idx, [10, 0], 5)
    with pytest.raises(ValueError, match="fanout"):
        NB.NeighborLoader(A, idx, [65], 5)
    with pytest.raises(ValueError, match="sizes"):
        NB.NeighborLoader(A, idx, [], 5)
    with pytest.raises(ValueError, match="repeats"):
        NB.NeighborLoader(A, [1, 2, 1], [4], 5)
    with pytest.raises(IndexError):
        NB.NeighborLoader(A, [NR.N], [4], 5)
    with pytest.raises(ValueError, match="square"):
        NB.NeighborLoader(host_csr(ip, ix, v, n_cols=NR.N + 1), idx, [4], 5)
    with pytest.raises(TypeError):
        NB.NeighborLoader(sp.csr_matrix((v, ix, ip), shape=(NR.N, NR.N)), idx, [4], 5)


# ---- the Python functions' checks -------------------------------------------------------------------
@pytest.mark.parametrize("fn", (NB.sample_neighbors, NB.sample_block))
def test_sampling_checks_its_arguments_before_the_device(fn):
    ip, ix, v = NR.graph()
    A, n = host_csr(ip, ix, v), NR.N
    with pytest.raises(IndexError):
        fn(A, [0, n], 10, 0)
    with pytest.raises(IndexError):
        fn(A, torch.tensor([-n - 1]), 10, 0)
    with pytest.raises(TypeError, match="integer"):
        fn(A, torch.tensor([0.0, 1.0]), 10, 0)
    with pytest.raises(TypeError, match="integer"):
        fn(A, torch.tensor([True, False]), 10, 0)
    with pytest.raises(ValueError, match="1-D"):
        fn(A, torch.zeros((2, 2), dtype=torch.int64), 10, 0)
    with pytest.raises(ValueError, match="repeats"):
        fn(A, [4, 9, 4], 10, 0)
    with pytest.raises(ValueError, match="repeats"):
        fn(A, [4, 4 - n], -1, 0)
    with pytest.raises(TypeError, match="DeviceCSR"):
        fn(sp.csr_matrix((v, ix, ip), shape=(n, n)), [0], 10, 0)
    for bad in (0, 65, 1000):
        with pytest.raises(ValueError, match="fanout"):
            fn(A, [0, 1], bad, 0)
    for bad in (2.0, True, None, "3"):
        with pytest.raises(TypeError, match="fanout"):
            fn(A, [0, 1], bad, 0)
    for bad in (1.5, None, False):
        with pytest.raises(TypeError, match="seed"):
            fn(A, [0, 1], 10, bad)
    # good arguments of every accepted kind reach the device check: no fall-back to the host
    for nodes in ([0, 3], range(0, 10, 2), torch.tensor([1, -1]), np.array([2, 5]), torch.tensor([4], dtype=torch.int32), []):
        for fanout, seed in ((1, 0), (64, 2 ** 64 - 1), (-1, -3), (10, 2 ** 70)):
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(A, nodes, fanout, seed)


def test_rectangular_operators_go_to_sample_neighbors_only():
    ip, ix, v = NR.graph()
    wide = host_csr(ip, ix, v, n_cols=NR.N + 5)
    with pytest.raises(ValueError, match="square"):
        NB.sample_block(wide, [0, 1], 10, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        NB.sample_neighbors(wide, [0, 1], 10, 0, eid=True)


# ---- the C entry ------------------------------------------------------------------------------------
def test_entry_is_declared_bound_and_rejects_bad_arguments_before_a_launch():
    L = _lib.lib()
    E = _lib.SRG_ERR_INVALID
    assert "srg_csr_sample_f32" in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(REPO, "include", "srgnn_hip.h")).read()
    assert re.search(r"\bint srg_csr_sample_f32\(const int64_t\* indptr, const int32_t\* indices, const float\* values", header)
    assert re.search(r"#define SRG_SAMPLE_MAX_FANOUT 64\b", header) and NB.MAX_FANOUT == NR.MAX_FANOUT == 64
    assert L.srg_csr_sample_f32.argtypes[6] is ctypes.c_int32 and L.srg_csr_sample_f32.argtypes[7] is ctypes.c_uint64
    some = ctypes.c_void_p(16)

    def call(n_rows=4, B=2, fanout=10, nodes=None, ptr=None, out_idx=None, out_val=None, values=None, indptr=None,
             indices=None):
        return L.srg_csr_sample_f32(indptr, indices, values, n_rows, nodes, B, fanout, 7, ptr, out_idx, out_val, None, None)

    assert call(fanout=0) == E and "fanout=0" in _lib.last_error()
    assert call(fanout=65) == E and "fanout=65" in _lib.last_error()
    assert call(fanout=2 ** 31 - 1) == E
    assert call(fanout=0, B=0) == E                                  # a bad fanout even where nothing would launch
    assert call(n_rows=-1) == E and call(B=-1) == E and "negative" in _lib.last_error()
    assert call(B=2 ** 31) == E and "B=" in _lib.last_error()
    assert call() == E and "null" in _lib.last_error()
    assert call(nodes=some, ptr=some) == E and "null" in _lib.last_error()          # nothing to write to
    assert call(nodes=some, ptr=some, out_idx=some) == E and "indptr" in _lib.last_error()
    assert call(nodes=some, ptr=some, out_idx=some, indptr=some, indices=some, out_val=some) == E
    assert "out_val without values" in _lib.last_error()
    for fanout in (1, 64, -1, -2 ** 31):
        assert call(B=0, fanout=fanout) == _lib.SRG_OK                # launches nothing
    assert L.srg_last_error_code() == _lib.SRG_OK
