"""Edge augmentation on the device: srg_knn_select_f32 and srg_sample_distinct_i64 against the host
restatement (tests/edge_augment_ref.py) bit for bit -- ids and distance bits with array_equal -- and
srgnn.augment.edge_augment against the reference's recorded edge lists (tests/golden/edge_augment.npz)."""
import os
import random

import numpy as np
import pytest
import torch

import edge_augment_ref as R
from srgnn import _lib
from srgnn import augment as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_augment.npz")
CASES = ("synth600_L3", "synth600_L1", "cora_0_0.7_L2")
M_SWEEP = (1, 2, 63, 64, 65, 100, 257)
GRID_ROWS = _lib.SRG_KNN_LAUNCH_ROWS      # rows of one launch; test_edge_augment_cpu.py holds it to the header


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def device_select(X, query, cand_ptr, cand, out_ptr):
    """X: a device tensor (any layout the wrapper takes); the rest numpy.  (ids, distance bits)."""
    sel, dist = A.knn_select(X, t(query), t(cand_ptr), t(cand), t(out_ptr), return_dist=True)
    torch.cuda.synchronize()
    return sel.cpu().numpy(), dist.cpu().numpy().view(np.uint32)


def ragged_problem(rng, n, d, rows, with_empty=True):
    """Rows cycling through the M sweep (and M = 0) and through k in {1, 3, M, 0}; distinct candidates."""
    Ms = list(M_SWEEP) + ([0] if with_empty else [])
    X = rng.standard_normal((n, d)).astype(np.float32)
    query = rng.integers(0, n, rows).astype(np.int64)
    lens, ks, cand = [], [], []
    for r in range(rows):
        M = Ms[(r + rows) % len(Ms)]
        k = (1, 3, M, 0)[(r // len(Ms) + r) % (4 if with_empty else 3)]
        lens.append(M)
        ks.append(min(k, M))
        cand.append(rng.choice(n, M, replace=False))
    cand = np.concatenate(cand).astype(np.int64) if cand else np.zeros(0, np.int64)
    return X, query, ptr_of(lens), cand, ptr_of(ks)


@pytest.mark.parametrize("rows", (1, 5, 300))
@pytest.mark.parametrize("d", (1, 3, 4, 7, 63, 64, 65, 263))
def test_shape_sweep(d, rows):
    rng = np.random.default_rng(1000 * d + rows)
    X, query, cand_ptr, cand, out_ptr = ragged_problem(rng, 400, d, rows)
    want_sel, want_bits = R.select(X, query, cand_ptr, cand, out_ptr)
    sel, bits = device_select(t(X), query, cand_ptr, cand, out_ptr)
    assert np.array_equal(sel, want_sel)
    assert np.array_equal(bits, want_bits)


@pytest.mark.parametrize("d", (1, 7, 64, 263))
def test_every_m_with_every_k(d):
    """One row per (M, k) of the sweep, k in {1, 3, M}."""
    rng = np.random.default_rng(77 + d)
    n = 400
    X = rng.standard_normal((n, d)).astype(np.float32)
    lens = [M for M in M_SWEEP for _ in range(3)]
    ks = [min(k, M) for M in M_SWEEP for k in (1, 3, M)]
    query = rng.integers(0, n, len(lens)).astype(np.int64)
    cand = np.concatenate([rng.choice(n, M, replace=False) for M in lens]).astype(np.int64)
    want = R.select(X, query, ptr_of(lens), cand, ptr_of(ks))
    got = device_select(t(X), query, ptr_of(lens), cand, ptr_of(ks))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_no_rows_and_rows_without_work():
    X = torch.zeros((10, 5), device=dev())
    e = np.zeros(0, np.int64)
    sel, bits = device_select(X, e, np.zeros(1, np.int64), e, np.zeros(1, np.int64))
    assert sel.size == 0 and bits.size == 0
    # rows with candidates and k = 0, rows without candidates
    sel, bits = device_select(X, np.array([1, 2, 3]), ptr_of([4, 0, 2]), np.arange(6), ptr_of([0, 0, 0]))
    assert sel.size == 0
    # d == 0: every distance +0, so the first k positions
    X0 = torch.zeros((10, 0), device=dev())
    sel, bits = device_select(X0, np.array([4]), ptr_of([5]), np.array([9, 3, 4, 0, 7]), ptr_of([3]))
    assert sel.tolist() == [9, 3, 4] and bits.tolist() == [0, 0, 0]


def test_candidate_cap():
    cap = _lib.SRG_KNN_MAX_CAND
    rng = np.random.default_rng(5)
    n = cap + 50
    X = rng.standard_normal((n, 1)).astype(np.float32)
    query = np.array([7, 8], dtype=np.int64)
    cand = np.concatenate([rng.choice(n, cap, replace=False), rng.choice(n, 3, replace=False)]).astype(np.int64)
    cand_ptr, out_ptr = ptr_of([cap, 3]), ptr_of([cap, 1])      # k = M at the cap: the whole row, sorted
    want = R.select(X, query, cand_ptr, cand, out_ptr)
    got = device_select(t(X), query, cand_ptr, cand, out_ptr)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    over = np.concatenate([cand[:cap], [1]]).astype(np.int64)
    with pytest.raises(_lib.SrgError, match="SRG_KNN_MAX_CAND"):
        A.knn_select(t(X), t(query[:1]), t(ptr_of([cap + 1])), t(over), t(ptr_of([1])))


def test_rows_past_one_launch():
    """More rows than one launch holds (the launches are chunked): d = 1, M = 2, k = 1."""
    rows = GRID_ROWS + 3
    rng = np.random.default_rng(9)
    n = 1000
    X = rng.standard_normal((n, 1)).astype(np.float32)
    query = rng.integers(0, n, rows).astype(np.int64)
    cand = rng.integers(0, n, 2 * rows).astype(np.int64)
    ptr = np.arange(rows + 1, dtype=np.int64)
    d0 = R.distance(X[query], X[cand[0::2]])
    d1 = R.distance(X[query], X[cand[1::2]])
    first = d0.view(np.uint32) <= d1.view(np.uint32)            # no NaN here: bits order the distances
    want_sel = np.where(first, cand[0::2], cand[1::2])
    want_bits = np.where(first, d0, d1).view(np.uint32)
    sel, bits = device_select(t(X), query, 2 * ptr, cand, ptr)
    assert np.array_equal(sel, want_sel) and np.array_equal(bits, want_bits)


@pytest.mark.parametrize("d", (4, 64, 65, 263))
def test_same_bits_in_every_layout(d):
    rng = np.random.default_rng(31 + d)
    X, query, cand_ptr, cand, out_ptr = ragged_problem(rng, 300, d, 40, with_empty=False)
    want = R.select(X, query, cand_ptr, cand, out_ptr)
    wide = torch.zeros((300, d + 12), device=dev())
    assert wide.data_ptr() % 16 == 0
    layouts = {"contiguous": t(X)}
    for name, c0 in (("window on 16 bytes", 4), ("window 4 bytes off", 5)):
        wide_k = wide.clone()
        wide_k[:, c0:c0 + d] = t(X)
        layouts[name] = wide_k[:, c0:c0 + d]
        assert layouts[name].stride(0) == d + 12 and layouts[name].data_ptr() % 16 == (c0 * 4) % 16
    # a padded panel whose row stride is a multiple of 4 elements: the 16-byte path with ldx > d
    pad = torch.zeros((300, (d + 7) // 4 * 4 + 4), device=dev())
    pad[:, :d] = t(X)
    layouts["ldx multiple of 4"] = pad[:, :d]
    for name, Xd in layouts.items():
        got = device_select(Xd, query, cand_ptr, cand, out_ptr)
        assert np.array_equal(got[0], want[0]), name
        assert np.array_equal(got[1], want[1]), name


def test_ties_come_out_in_position_order():
    rng = np.random.default_rng(12)
    n, d = 60, 19
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[10] = X[11] = X[12] = X[30]           # duplicated feature rows among the candidates
    X[20] = X[21] = X[5]                    # copies of query row 5: distance +0
    X[40:50] = X[40]                        # a whole row of equal distances
    query = np.array([5, 5, 3], dtype=np.int64)
    lists = [[12, 33, 21, 10, 5, 30, 20, 11], [11, 12, 10, 30], list(range(49, 39, -1))]
    ks = [8, 4, 4]
    cand = np.concatenate(lists).astype(np.int64)
    cand_ptr, out_ptr = ptr_of([len(l) for l in lists]), ptr_of(ks)
    want = R.select(X, query, cand_ptr, cand, out_ptr)
    sel, bits = device_select(t(X), query, cand_ptr, cand, out_ptr)
    assert np.array_equal(sel, want[0]) and np.array_equal(bits, want[1])
    assert sel[:3].tolist() == [21, 5, 20] and bits[:3].tolist() == [0, 0, 0]
    rest = sel[3:8].tolist()
    assert [c for c in rest if c != 33] == [12, 10, 30, 11]                      # equal distances: list order
    assert sel[8:12].tolist() == [11, 12, 10, 30]
    assert sel[12:16].tolist() == [49, 48, 47, 46] and len(set(bits[12:16].tolist())) == 1


@pytest.mark.parametrize("d", (3, 70))
def test_special_values(d):
    f = np.float32
    n = 16
    X = np.zeros((n, d), dtype=f)
    X[1, 0] = np.nan
    X[2, 0] = np.inf                        # against a finite query: +Inf
    X[3, 0] = -np.inf
    X[4, d - 1] = np.nan
    X[5, 0] = 1.0
    X[6, 0] = f(1e-20)                      # the square is subnormal (1e-40), the distance 1e-20
    X[7, d - 1] = f(3e-23)                  # the square (9e-46) is the smallest subnormals' neighbourhood
    X[8, 0] = f(1e-39)                      # a subnormal difference: its square underflows to +0
    X[9, 0] = np.inf                        # query 9 against candidate 2: Inf - Inf = NaN
    X[10, 0] = f(3e38)                      # the square overflows: +Inf
    X[11, 0] = -0.0
    query = np.array([0, 9, 1], dtype=np.int64)
    lists = [[1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 0], [2, 3, 5, 9, 1], [5, 0, 1]]
    cand = np.concatenate(lists).astype(np.int64)
    cand_ptr = ptr_of([len(l) for l in lists])
    want = R.select(X, query, cand_ptr, cand, cand_ptr)
    sel, bits = device_select(t(X), query, cand_ptr, cand, cand_ptr)
    assert np.array_equal(sel, want[0]) and np.array_equal(bits, want[1])
    # row 0, spelled out: +0 three times in list order (the underflowed square, -0 and the query itself), the two
    # subnormal squares, 1, +Inf three times in list order, then the NaNs in list order
    assert sel[:11].tolist() == [8, 11, 0, 7, 6, 5, 2, 3, 10, 1, 4]
    dist = bits[:11].view(np.float32)
    assert bits[:3].tolist() == [0, 0, 0] and dist[3] == np.sqrt(f(3e-23) * f(3e-23)) and dist[3] > 0
    assert dist[4] == np.sqrt(f(1e-20) * f(1e-20)) and dist[5] == 1.0
    assert bits[6:9].tolist() == [0x7F800000] * 3 and bits[9:11].tolist() == [0x7FC00000] * 2
    # row 1 (query +Inf): Inf - Inf is NaN, Inf - (-Inf) is +Inf; row 2 (a NaN query row): everything NaN, list order
    assert sel[11:16].tolist() == [3, 5, 2, 9, 1]
    assert bits[11:16].tolist() == [0x7F800000, 0x7F800000, 0x7FC00000, 0x7FC00000, 0x7FC00000]
    assert sel[16:19].tolist() == [5, 0, 1] and bits[16:19].tolist() == [0x7FC00000] * 3


@pytest.mark.parametrize("d", (1, 23, 263))
def test_out_of_range_candidates_are_never_read(d):
    """X is rows [8, 8 + n) of a larger allocation whose outside rows hold the query row itself: a kernel that
    read them would rank them first (distance +0) -- without leaving the allocation: every id used here lies in
    [-8, 0) or [n, n + 8).  Ids far outside (n + 2^32) are covered by test_edge_augment_cpu.py's restatement test
    and by the wrapper's IndexError, never by a launch."""
    rng = np.random.default_rng(d)
    n = 50
    big = rng.standard_normal((n + 16, d)).astype(np.float32)
    q = 17
    big[:8] = big[8 + q]
    big[8 + n:] = big[8 + q]
    big_d = t(big)
    Xw = big_d[8:8 + n]
    outside = list(range(-8, 0)) + list(range(n, n + 8))
    lists = [[-3, 4, n, 9, -8, n + 7, 30], outside, [5] + outside[::3] + [6]]
    query = np.array([q, q, q], dtype=np.int64)
    cand = np.concatenate(lists).astype(np.int64)
    cand_ptr = ptr_of([len(l) for l in lists])
    want = R.select(big[8:8 + n], query, cand_ptr, cand, cand_ptr)
    sel, bits = device_select(Xw, query, cand_ptr, cand, cand_ptr)
    assert np.array_equal(sel, want[0]) and np.array_equal(bits, want[1])
    assert sorted(sel[:3].tolist()) == [4, 9, 30]                                # the valid ones first
    assert sel[3:7].tolist() == [-3, n, -8, n + 7]                                # the others in list order
    assert bits[3:7].tolist() == [0x7FC00000] * 4
    assert sel[7:7 + 16].tolist() == outside
    assert sorted(sel[23:25].tolist()) == [5, 6] and sel[25:].tolist() == outside[::3]


def test_c_entry_rejects_bad_pointer_arrays():
    X = torch.zeros((10, 4), device=dev())
    ok = dict(query=np.array([1, 2]), cand_ptr=ptr_of([3, 3]), cand=np.arange(6), out_ptr=ptr_of([1, 3]))
    device_select(X, **ok)
    bad = [(dict(query=np.array([1, 10])), "query id"), (dict(query=np.array([-1, 2])), "query id"),
           (dict(out_ptr=ptr_of([1, 4])), "k > M"), (dict(out_ptr=np.array([0, 2, 1])), "out_ptr"),
           (dict(cand_ptr=np.array([0, 4, 3]), out_ptr=ptr_of([1, 0])), "cand_ptr")]
    for change, msg in bad:
        args = {**ok, **{k: np.asarray(v, dtype=np.int64) for k, v in change.items()}}
        with pytest.raises(_lib.SrgError, match=msg):
            device_select(X, **args)


# ---- the sampler ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 3, 64, 65, 1000, 2 ** 20 + 1))
def test_sampler_equals_the_restatement(n):
    query = np.array([0, n - 1, n // 2, 1 % n, 0], dtype=np.int64)
    cand_ptr = ptr_of([n - 1, n - 1, min(n - 1, 100), 0, min(n - 1, 7)])
    for seed in (0, 5, 2 ** 64 - 1):
        got = A.sample_distinct(t(query), t(cand_ptr), n, seed).cpu().numpy()
        assert np.array_equal(got, R.sample_distinct(query, cand_ptr, n, seed)), seed
    full = got[:n - 1]
    assert np.array_equal(np.sort(full), np.arange(1, n))                         # every id but node 0, once


def test_sampler_rejects_bad_rows():
    with pytest.raises(_lib.SrgError, match="n - 1"):
        A.sample_distinct(t(np.array([0, 1])), t(ptr_of([3, 10])), 10, 0)
    with pytest.raises(_lib.SrgError, match="query id"):
        A.sample_distinct(t(np.array([10])), t(ptr_of([3])), 10, 0)
    assert A.sample_distinct(t(np.zeros(0, np.int64)), t(np.zeros(1, np.int64)), 10, 0).numel() == 0


# ---- end to end ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case(golden, name):
    g = {k.split("__", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "__")}
    for k in ("row", "col", "nodes", "cand", "edge_index"):
        g[k] = g[k].astype(np.int64)
    for k in ("n", "L", "seed"):
        g[k] = int(g[k])
    return g


@pytest.mark.parametrize("name", CASES)
def test_edge_augment_equals_the_reference(golden, name):
    g = case(golden, name)
    nodes, ptr, ids = A._rows_by_node_id(g["nodes"], g["cand_ptr"], g["cand"])
    row, col, F = torch.from_numpy(g["row"]), torch.from_numpy(g["col"]), torch.from_numpy(g["features"])
    want = torch.from_numpy(g["edge_index"])
    # host inputs, candidate ids in the fixture's narrow dtype: the result returns on the host
    out = A.edge_augment(row, col, g["n"], F, degree_level=g["L"],
                         candidates=(torch.from_numpy(ptr), torch.from_numpy(ids.astype(np.int16))))
    assert out.device.type == "cpu" and out.dtype == torch.int64 and torch.equal(out, want)
    # device inputs, the features a strided column window of a wider panel
    wide = torch.zeros((g["n"], F.shape[1] + 9), device=dev())
    wide[:, 5:5 + F.shape[1]] = F.to(dev())
    out, chosen = A.edge_augment(row.to(dev()), col.to(dev()), g["n"], wide[:, 5:5 + F.shape[1]], degree_level=g["L"],
                                 candidates=(t(ptr), t(ids)), return_selected=True)
    assert out.device == dev() and torch.equal(out.cpu(), want)
    assert np.array_equal(chosen.nodes.cpu().numpy(), nodes)
    want_sel, want_bits = R.select(g["features"], nodes, ptr, ids, chosen.out_ptr.cpu().numpy())
    assert np.array_equal(chosen.sel.cpu().numpy(), want_sel)
    assert np.array_equal(chosen.dist.cpu().numpy().view(np.uint32), want_bits)


@pytest.mark.parametrize("name", CASES[:2])
def test_reference_spelling_replays_the_reference_draw(golden, name):
    g = case(golden, name)

    class Edge:
        row, col = torch.from_numpy(g["row"]), torch.from_numpy(g["col"])

    class Dataset:
        edge, x = Edge, g["features"]

    random.seed(g["seed"])
    out = A.edge_augument(Dataset, torch.from_numpy(g["features"]), g["L"])
    assert random.random() == float(g["random_after"])
    assert torch.equal(out, torch.from_numpy(g["edge_index"]))


def test_edge_augment_with_the_device_draw(golden):
    g = case(golden, "synth600_L3")
    n, L = g["n"], g["L"]
    row, col, F = t(g["row"]), t(g["col"]), t(g["features"])
    out, chosen = A.edge_augment(row, col, n, F, degree_level=L, seed=99, return_selected=True)
    again = A.edge_augment(row, col, n, F, degree_level=L, seed=99)
    other = A.edge_augment(row, col, n, F, degree_level=L, seed=100)
    assert torch.equal(out, again) and not torch.equal(out, other)
    e = out.cpu().numpy()
    key = e[0] * n + e[1]
    assert np.all(np.diff(key) > 0)                                               # sorted by (row, col), unique
    assert np.array_equal(np.sort(e[1] * n + e[0]), key)                          # symmetric
    have = set(key.tolist())
    assert set((g["row"] * n + g["col"]).tolist()) <= have and set((g["col"] * n + g["row"]).tolist()) <= have
    # the drawn lists and the selection agree with the restatement
    nodes, cand_ptr, out_ptr = R.low_degree_rows(g["row"], g["col"], n, L)
    assert np.array_equal(chosen.nodes.cpu().numpy(), nodes)
    assert np.array_equal(chosen.cand_ptr.cpu().numpy(), cand_ptr) and np.array_equal(chosen.out_ptr.cpu().numpy(), out_ptr)
    cand = R.sample_distinct(nodes, cand_ptr, n, 99)
    assert np.array_equal(chosen.cand.cpu().numpy(), cand)
    want_sel, want_bits = R.select(g["features"], nodes, cand_ptr, cand, out_ptr)
    assert np.array_equal(chosen.sel.cpu().numpy(), want_sel)
    assert np.array_equal(chosen.dist.cpu().numpy().view(np.uint32), want_bits)
    assert np.array_equal(e, R.assemble(g["row"], g["col"], nodes, out_ptr, want_sel))


def test_wrapper_rejects_bad_candidates_and_sizes(golden):
    g = case(golden, "synth600_L1")
    n, L = g["n"], g["L"]
    nodes, ptr, ids = A._rows_by_node_id(g["nodes"], g["cand_ptr"], g["cand"])
    row, col, F = t(g["row"]), t(g["col"]), t(g["features"])
    for bad_id in (-1, n, n + 2 ** 32, 5 - 2 ** 32):      # the last two: valid ids once cut to 32 bits
        bad = ids.copy()
        bad[5] = bad_id
        with pytest.raises(IndexError, match="candidate ids"):
            A.edge_augment(row, col, n, F, degree_level=L, candidates=(t(ptr), t(bad)))
    own = ids.copy()
    own[ptr[3]] = nodes[3]
    with pytest.raises(ValueError, match="its own node"):
        A.edge_augment(row, col, n, F, degree_level=L, candidates=(t(ptr), t(own)))
    with pytest.raises(ValueError, match="per_edge x"):
        A.edge_augment(row, col, n, F, degree_level=L, candidates=(t(ptr[:-1]), t(ids[:ptr[-2]])))
    with pytest.raises(ValueError, match="per_edge x"):
        A.edge_augment(row, col, n, F, degree_level=L, candidates=(t(ptr), t(ids[:-1])))
    with pytest.raises(IndexError, match="edge ids"):
        A.edge_augment(t(np.array([0, n])), t(np.array([1, 2])), n, F)
    with pytest.raises(ValueError, match="distinct candidates"):                  # 100 x 7 > n - 1
        A.edge_augment(row, col, n, F, degree_level=7)
    small = torch.zeros((50, 3), device=dev())
    with pytest.raises(ValueError, match="distinct candidates"):                  # 100 > 49
        A.edge_augment(t(np.array([0])), t(np.array([1])), 50, small)
    bigF = torch.zeros((5000, 2), device=dev())
    with pytest.raises(ValueError, match="SRG_KNN_MAX_CAND"):                     # 100 x 41 > 4096
        A.edge_augment(t(np.array([0])), t(np.array([1])), 5000, bigF, degree_level=41)
    # nothing to repair: the symmetrised, sorted, unique input
    out = A.edge_augment(t(np.array([0, 1, 1])), t(np.array([1, 0, 2])), 3, small[:3], degree_level=1)
    assert out.cpu().tolist() == [[0, 1, 1, 2], [1, 0, 2, 1]]
    assert A.edge_augment(row, col, n, F, degree_level=0).shape[0] == 2
