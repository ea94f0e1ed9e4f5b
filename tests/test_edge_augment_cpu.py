"""Edge augmentation without a device: the host restatement against the reference's recorded runs, the
replay of the reference's draw, the sampler's arithmetic and the argument checks of srgnn.augment."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import edge_augment_ref as R
from srgnn import _lib
from srgnn import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_augment.npz")
CASES = ("synth600_L3", "synth600_L1", "cora_0_0.7_L2")
SIZES = (2, 3, 64, 65, 1000, 2 ** 20 + 1)


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


def test_fixture_holds_every_case(golden):
    assert {k.split("__", 1)[0] for k in golden.files} == set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_edge_index(golden, name):
    g = case(golden, name)
    got = R.edge_augment(g["row"], g["col"], g["n"], g["features"], g["L"], g["nodes"], g["cand_ptr"], g["cand"])
    assert got.dtype == np.int64 and np.array_equal(got, g["edge_index"])
    # the fixture is what the issue describes: low-degree nodes of several degrees, a self loop, a duplicate
    deg = R.degrees(g["row"], g["col"], g["n"])
    assert np.array_equal(np.sort(g["nodes"]), np.nonzero(deg < g["L"])[0])
    if name.startswith("synth600"):
        assert (g["row"] == g["col"]).sum() == 1 and g["features"].shape == (600, 23)
        pairs = g["row"] * g["n"] + g["col"]
        assert np.unique(pairs).size == pairs.size - 1
        assert {0, 1, 2} <= set(deg.tolist())


@pytest.mark.parametrize("name", CASES)
def test_reference_replay_draws_the_recorded_candidates(golden, name):
    g = case(golden, name)
    random.seed(g["seed"])
    nodes, ptr, ids = A.reference_candidates(g["row"], g["col"], g["n"], g["L"])
    after = random.random()
    assert np.array_equal(nodes, g["nodes"]) and np.array_equal(ptr, g["cand_ptr"]) and np.array_equal(ids, g["cand"])
    assert after == float(g["random_after"])
    # rows reordered by node id keep each list's order
    n2, p2, i2 = A._rows_by_node_id(nodes, ptr, ids)
    assert np.array_equal(n2, np.sort(nodes))
    for i in (0, len(n2) // 2, len(n2) - 1):
        j = int(np.nonzero(nodes == n2[i])[0][0])
        assert np.array_equal(i2[p2[i]:p2[i + 1]], ids[ptr[j]:ptr[j + 1]])


def test_reference_replay_rejects_a_draw_larger_than_the_pool():
    with pytest.raises(ValueError):
        A.reference_candidates(np.zeros(0, np.int64), np.zeros(0, np.int64), 50, 1)   # 100 > 49


@pytest.mark.parametrize("n", SIZES)
def test_sampler_full_draw_is_a_permutation(n):
    query = np.array([0, n - 1, n // 2, 1 % n], dtype=np.int64)
    ptr = np.arange(5, dtype=np.int64) * (n - 1)
    a = R.sample_distinct(query, ptr, n, seed=5).reshape(4, n - 1)
    for r in range(4):
        want = np.delete(np.arange(n, dtype=np.int64), query[r])
        assert np.array_equal(np.sort(a[r]), want)
    b = R.sample_distinct(query, ptr, n, seed=6).reshape(4, n - 1)
    if n > 3:
        assert not np.array_equal(a, b)
        assert not np.array_equal(a[0] - 1, a[1])   # rows 0 (shifted past node 0) and 1 (past n-1) differ too
    # a shorter draw is a prefix: entry t depends on (seed, r, t) only
    short = R.sample_distinct(query, np.arange(5, dtype=np.int64) * min(n - 1, 7), n, seed=5)
    assert np.array_equal(short.reshape(4, -1), a[:, :min(n - 1, 7)])


def test_sampler_rejects_more_than_n_minus_one():
    with pytest.raises(ValueError):
        R.sample_distinct(np.array([0]), np.array([0, 10]), 10, seed=1)


def test_sampler_counts_are_uniform():
    n, rows, M = 1000, 4096, 100
    query = np.full(rows, n - 1, dtype=np.int64)         # every row excludes the same node: ids 0 .. n-2
    ids = R.sample_distinct(query, np.arange(rows + 1, dtype=np.int64) * M, n, seed=20261020)
    counts = np.bincount(ids, minlength=n)
    lam = rows * M / (n - 1)
    assert counts[n - 1] == 0
    assert np.abs(counts[:n - 1] - lam).max() <= 6 * np.sqrt(lam), (counts[:n - 1].min(), counts[:n - 1].max(), lam)


def test_distance_order_is_the_stated_one():
    """The vectorised restatement against a scalar transcription of the header's wording."""
    rng = np.random.default_rng(3)
    f32 = np.float32
    for d in (0, 1, 3, 4, 5, 23, 64, 65, 263, 300):
        xq = rng.standard_normal(d).astype(f32)
        xc = rng.standard_normal(d).astype(f32)
        G = R.group_lanes(d)
        p = [f32(0)] * G
        for piece in range((d + 3) // 4):
            for j in range(4 * piece, min(4 * piece + 4, d)):
                t = f32(xq[j] - xc[j])
                p[piece % G] = f32(p[piece % G] + f32(t * t))
        h = G // 2
        while h >= 1:
            for g in range(h):
                p[g] = f32(p[g] + p[g + h])
            h //= 2
        want = np.sqrt(p[0])
        got = R.distance(xq[None, :], xc[None, :])[0]
        assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), d
    assert R.group_lanes(263) == 64 and R.group_lanes(23) == 8 and R.group_lanes(4) == 1 and R.group_lanes(0) == 1


def test_selection_orders_ties_nan_and_outside_ids():
    X = np.zeros((6, 2), dtype=np.float32)
    X[1] = (3, 4)            # distance 5 from row 0
    X[2] = (3, 4)            # the same distance: position decides
    X[3] = (np.inf, 0)       # +Inf
    X[4] = (np.nan, 0)       # NaN: after +Inf
    X[5] = (0, 0)            # a copy of the query row: +0
    ids, bits = R.select_row(X, 0, [4, 9, 3, 2, -1, 1, 5], 7)
    assert ids.tolist() == [5, 2, 1, 3, 4, 9, -1]
    assert bits.tolist() == [0, 0x40A00000, 0x40A00000, 0x7F800000, 0x7FC00000, 0x7FC00000, 0x7FC00000]
    # an id whose low 32 bits are a valid id (a copy of the query row at that) is outside all the same
    far = [1, 5 + 2 ** 32, -(2 ** 32) + 5, 5]
    ids, bits = R.select_row(X, 0, far, 4)
    assert ids.tolist() == [5, 1, 5 + 2 ** 32, -(2 ** 32) + 5]
    assert bits.tolist() == [0, 0x40A00000, 0x7FC00000, 0x7FC00000]


def test_binding_lists_the_new_entries_and_cap():
    assert {"srg_knn_select_f32", "srg_sample_distinct_i64"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib.SRG_KNN_MAX_CAND >= 4096
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srgnn_hip.h")).read()
    assert f"#define SRG_KNN_MAX_CAND {_lib.SRG_KNN_MAX_CAND}\n" in text
    assert f"#define SRG_KNN_MAX_D {_lib.SRG_KNN_MAX_D}\n" in text
    assert f"#define SRG_KNN_LAUNCH_ROWS {_lib.SRG_KNN_LAUNCH_ROWS}\n" in text


def test_c_entries_reject_bad_arguments_before_the_device():
    L = _lib.lib()
    p = ctypes.c_void_p(64)
    assert L.srg_knn_select_f32(None, 8, 10, 16, None, None, None, None, 3, None, None, None) == _lib.SRG_ERR_INVALID
    assert "ldx=8 < d=16" in _lib.last_error()
    assert L.srg_knn_select_f32(None, 8, 10, -1, None, None, None, None, 3, None, None, None) == _lib.SRG_ERR_INVALID
    assert L.srg_knn_select_f32(None, 1 << 20, 10, _lib.SRG_KNN_MAX_D + 1, None, None, None, None, 3, None, None,
                                None) == _lib.SRG_ERR_INVALID
    assert L.srg_knn_select_f32(None, 8, 10, 8, None, None, None, None, -1, None, None, None) == _lib.SRG_ERR_INVALID
    assert L.srg_knn_select_f32(p, 8, 10, 8, None, p, p, p, 3, p, None, None) == _lib.SRG_ERR_INVALID
    assert "null" in _lib.last_error()
    assert L.srg_sample_distinct_i64(None, None, -2, 10, 0, None, None) == _lib.SRG_ERR_INVALID
    assert L.srg_sample_distinct_i64(None, p, 2, 10, 0, p, None) == _lib.SRG_ERR_INVALID
    # empty problems need no device
    assert L.srg_knn_select_f32(None, 8, 10, 8, None, None, None, None, 0, None, None, None) == _lib.SRG_OK
    assert L.srg_sample_distinct_i64(None, None, 0, 10, 0, None, None) == _lib.SRG_OK
    assert L.srg_last_error_code() == _lib.SRG_OK


def test_wrapper_argument_errors_need_no_device():
    row = torch.tensor([0, 1, 2])
    col = torch.tensor([1, 2, 3])
    F = torch.zeros(500, 4)
    with pytest.raises(ValueError, match="edge_row has 3 entries"):
        A.edge_augment(row, col[:2], 500, F)
    with pytest.raises(TypeError, match="integer"):
        A.edge_augment(row.float(), col, 500, F)
    with pytest.raises(TypeError, match="float32"):
        A.edge_augment(row, col, 500, F.double())
    with pytest.raises(ValueError, match="features must be"):
        A.edge_augment(row, col, 499, F)
    with pytest.raises(ValueError, match="features must be"):
        A.edge_augment(row, col, 500, F[:, 0])
    with pytest.raises(ValueError, match="degree_level"):
        A.edge_augment(row, col, 500, F, degree_level=-1)
    with pytest.raises(ValueError, match="per_edge"):
        A.edge_augment(row, col, 500, F, per_edge=0)
    with pytest.raises(ValueError, match="candidates must be"):
        A.edge_augment(row, col, 500, F, candidates="random")
    with pytest.raises(ValueError, match="candidates must be"):
        A.edge_augment(row, col, 500, F, candidates=(torch.zeros(1, dtype=torch.int64),))
    with pytest.raises(TypeError, match="candidates ids"):
        A.edge_augment(row, col, 500, F, candidates=(torch.zeros(1, dtype=torch.int64), torch.zeros(3)))
    with pytest.raises(ValueError, match="columns"):
        A.edge_augment(row, col, 2, torch.zeros(2, _lib.SRG_KNN_MAX_D + 1))


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        A.edge_augment(torch.tensor([0]), torch.tensor([1]), 500, torch.zeros(500, 4))
