"""The ladder operator (tests/ladder_cases.py) on the CPU: its generator's invariants, the condition
that its data shows the order of a row's chain in the result bits, and the numpy epilogue references
the GPU tests compare against (held to the oracle's own cheby_op).  No GPU."""
import numpy as np
import pytest

import ladder_cases as LC

DETECT = 0.95      # the share of mutated rows whose bits must change
D_DETECT = 32      # one fp32 hub slice


def test_lengths_cover_the_ladder_and_the_edges():
    lens = LC.lengths()
    assert lens.shape == (LC.N,) and LC.N == 4096
    have = set(int(x) for x in lens)
    assert all(k in have for k in range(LC.LADDER_MAX + 1)), "a ladder length is missing"
    edge = LC.edge_lengths()
    assert len(edge) == 72 and max(edge) == 3081 and all(e in have for e in edge)
    # every length the ladder and the edge rows name has a row of its own beside the filler's
    counts = np.bincount(lens, minlength=3082)
    filler = np.bincount(np.arange(LC.N - (LC.LADDER_MAX + 1) - len(edge)) % LC.FILLER_CYCLE, minlength=3082)
    want = filler.copy()
    for k in list(range(LC.LADDER_MAX + 1)) + edge:
        want[k] += 1
    assert np.array_equal(counts, want)
    # the rows are shuffled: long and short rows are neighbours (a packed wave's rows differ in length)
    assert np.abs(np.diff(lens)).max() > 1000 and not np.array_equal(lens, np.sort(lens))


def test_structure_sorted_unique_in_range():
    indptr, indices = LC.structure()
    lens = LC.lengths()
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    assert indptr[0] == 0 and np.array_equal(np.diff(indptr), lens) and indptr[-1] == indices.size
    assert 700_000 < indices.size < 850_000
    assert indices.min() >= 0 and indices.max() < LC.N
    inner = np.ones(indices.size, dtype=bool)
    inner[indptr[:-1][lens > 0]] = False            # a row's first entry has no predecessor in the row
    assert np.all(np.diff(indices.astype(np.int64))[inner[1:]] > 0), "ids not strictly increasing within a row"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_values_and_outputs_bounded(oracle_mod, dtype):
    ip, ix, v = LC.operator(dtype)
    assert v.dtype == np.dtype(dtype) and np.all((np.abs(v) >= 0.5) & (np.abs(v) < 1.5))
    assert (v > 0).any() and (v < 0).any()
    for d in (4, 64):
        X = LC.x_panel(dtype, d)
        assert X.dtype == np.dtype(dtype) and X.shape == (LC.N, d) and X.min() >= 1.0 and X.max() < 2.25
        Y = oracle_mod.spmm(ip, ix, v, X) if dtype == "float32" else oracle_mod.spmm64(ip, ix, v, X)
        assert np.isfinite(Y).all()
        # the walk keeps every column's partial sums O(1): the end values too
        assert np.abs(Y).max() < 32.0, np.abs(Y).max()
        assert np.array_equal(Y[LC.lengths() == 0], np.zeros((int((LC.lengths() == 0).sum()), d), Y.dtype))


def _changed_share(oracle_mod, dtype, name):
    ip, ix, v = LC.operator(dtype)
    X = LC.x_panel(dtype, D_DETECT)
    mul = oracle_mod.spmm if dtype == "float32" else oracle_mod.spmm64
    u = np.uint32 if dtype == "float32" else np.uint64
    base = mul(ip, ix, v, X)
    first = LC.mutations(LC.lengths(), commuting_head=dtype == "float64")[name]
    mix, mv, rows = LC.swap_links(ip, ix, v, first)
    got = mul(ip, mix, mv, X)
    diff = (got.view(u) != base.view(u)).any(axis=1)
    assert not diff[np.setdiff1d(np.arange(LC.N), rows)].any(), "a row the mutation left alone changed"
    return int(diff[rows].sum()), int(rows.size)


@pytest.mark.parametrize("name", ["first", "middle", "last", "window256", "window512"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_data_shows_a_swapped_pair_of_links(oracle_mod, dtype, name):
    """A condition on the data, not a measurement: a transposed pair of links anywhere in the rows
    changes the bits of at least 95 % of the rows it is applied to (d = 32).  Measured, rows changed of
    rows applied to: fp32 first 3993 / 4002 (99.8 %), middle 3954 / 4002 (98.8 %), last 3992 / 4002
    (99.8 %), window256 869 / 880 (98.8 %), window512 620 / 624 (99.4 %); fp64 (the walk centred at 3 and
    first = links (1, 2): ladder_cases.WALK_CENTRE, ladder_cases.mutations) first 3815 / 3955 (96.5 %),
    middle 3858 / 3908 (98.7 %), last 3955 / 3955 (100 %), window256 854 / 880 (97.0 %), window512
    611 / 624 (97.9 %)."""
    changed, applied = _changed_share(oracle_mod, dtype, name)
    print(f"{dtype} {name}: {changed} of {applied} rows changed ({100.0 * changed / applied:.2f} %)")
    assert applied >= {"first": 3900, "middle": 3900, "last": 3900, "window256": 880, "window512": 620}[name]
    assert changed >= DETECT * applied, (changed, applied)


def test_fp64_first_two_links_commute(oracle_mod):
    """Why the fp64 first-links case swaps (1, 2): swapping links 0 and 1 of the fp64 chain (from +0,
    product and sum rounded separately) gives the same bits in every row -- it is the same chain."""
    ip, ix, v = LC.operator("float64")
    X = LC.x_panel("float64", D_DETECT)
    mix, mv, rows = LC.swap_links(ip, ix, v, np.where(LC.lengths() >= 2, 0, -1))
    assert rows.size > 3900
    assert np.array_equal(oracle_mod.spmm64(ip, mix, mv, X).view(np.uint64),
                          oracle_mod.spmm64(ip, ix, v, X).view(np.uint64))


def test_mutation_positions():
    lens = np.array([0, 1, 2, 3, 4, 5, 256, 257, 512, 513, 1000])
    m32, m64 = LC.mutations(lens, False), LC.mutations(lens, True)
    assert m32["first"].tolist() == [-1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert m64["first"].tolist() == [-1, -1, -1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert m32["middle"].tolist() == [-1, -1, 0, 0, 1, 1, 127, 127, 255, 255, 499]
    assert m64["middle"].tolist() == [-1, -1, -1, -1, 1, 1, 127, 127, 255, 255, 499]
    assert m32["last"].tolist() == [-1, -1, 0, 1, 2, 3, 254, 255, 510, 511, 998]
    assert m64["last"].tolist() == [-1, -1, -1, 1, 2, 3, 254, 255, 510, 511, 998]
    assert m32["window256"].tolist() == [-1] * 7 + [255] * 4 == m64["window256"].tolist()
    assert m32["window512"].tolist() == [-1] * 9 + [511] * 2
    ip = np.array([0, 3, 5])
    ix, v, rows = LC.swap_links(ip, np.arange(5, dtype=np.int32), np.arange(5.0), np.array([1, 0]))
    assert ix.tolist() == [0, 2, 1, 4, 3] and v.tolist() == [0.0, 2.0, 1.0, 4.0, 3.0] and rows.tolist() == [0, 1]


def test_schedules_are_what_they_say():
    lens = LC.lengths()
    n_empty = int((lens == 0).sum())
    for thr in ((-1, -1), (0, -1), (0, 0)):
        order, n_hub, n_heavy = LC.sched_desc(lens, *thr)
        assert sorted(order.tolist()) == list(range(LC.N)) and np.all(np.diff(lens[order]) <= 0)
        assert (n_hub, n_heavy) == {(-1, -1): (0, 0), (0, -1): (0, LC.N - n_empty), (0, 0): (LC.N - n_empty, 0)}[thr]
    order, n_hub, n_heavy = LC.sched_asc(lens, 96, 700)
    assert sorted(order.tolist()) == list(range(LC.N)) and lens[order[0]] == 1 and lens[order[:96]].max() <= 3
    assert np.all(lens[order[-n_empty:]] == 0) and np.all(np.diff(lens[order[:-n_empty]]) >= 0)
    order, _, _ = LC.sched_asc(lens, 96, 700, empty_first=True)
    assert np.all(lens[order[:n_empty]] == 0) and lens[order[n_empty]] == 1
    for seed in (1, 2):
        order, n_hub, n_heavy = LC.sched_rand(lens, seed, 48, 900, leave_out=100)
        assert order.size == LC.N - 100 and np.unique(order).size == order.size
        assert lens[order[:48]].min() >= 1 and lens[order[:48]].max() > 20 * lens[order[:48]].min()
        hv, lt = lens[order[48:948]], lens[order[948:]]
        assert hv.min() == 0 and hv.max() > 1000 and lt.min() == 0 and lt.max() > 1000
        # very different lengths side by side in one packed wave (8 rows at d = 64)
        assert max(lt[i:i + 8].max() - lt[i:i + 8].min() for i in range(0, lt.size - 8, 8)) > 2000
    order, n_hub, _ = LC.sched_rand(lens, 3, 400, 0, empty_hubs=True)
    assert (lens[order[:n_hub]] == 0).any()
    for n_slices in (1, 2):
        launches = LC.w512_sweep(lens, n_slices)
        assert len(launches) == -(-(LC.N - n_empty) // (256 // n_slices))
        seen = np.concatenate([o[:h] for o, h, _ in launches])
        assert np.array_equal(np.sort(seen), np.flatnonzero(lens > 0))      # every non-empty row a hub row once
        for o, h, hv in launches:
            assert h * n_slices <= 256 and hv == 0 and sorted(o.tolist()) == list(range(LC.N)) and lens[o[:h]].min() > 0


def _small_laplacian(oracle_mod, n=300, seed=5):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    keep = u != v
    key = np.unique(u[keep] * n + v[keep])
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, key // n + 1, 1)
    return oracle_mod.laplacian(np.cumsum(ptr), (key % n).astype(np.int32), rng.uniform(0.5, 2.0, key.size), n)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_numpy_epilogue_equals_the_oracle_filter(oracle_mod, order):
    """oracle.spmm64 plus ladder_cases.cheby_ref, plain (INIT, STEP, ...) and lean (INIT_T, STEP_FIRST,
    ..., STEP | NO_T), equal oracle.cheby_op bit for bit."""
    n, d = 300, 7
    L = _small_laplacian(oracle_mod, n)
    lmax = 2.0 * float(np.max(L[2]))
    coeffs = np.stack([oracle_mod.cheby_coeffs(t, lmax, order) for t in (0.5, 2.0, 7.0)])
    S = np.random.default_rng(order).standard_normal((n, d))
    want = oracle_mod.cheby_op(L, coeffs, S, lmax)
    plain = LC.cheby_filter_ref(oracle_mod.spmm64, L, coeffs, S, lmax, lean=False)
    lean = LC.cheby_filter_ref(oracle_mod.spmm64, L, coeffs, S, lmax, lean=True)
    assert np.array_equal(plain.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(lean.view(np.uint64), plain.view(np.uint64))


def test_numpy_epilogues_round_every_operation():
    """The references work in the arrays' precision: fp32 in, every intermediate fp32 (compared with
    the same expression evaluated in fp64 and rounded once, which differs), and the aggregation step
    is a separately rounded product and sum."""
    rng = np.random.default_rng(0)
    acc, tc, to = (rng.standard_normal((50, 9)).astype(np.float32) for _ in range(3))
    R0 = rng.standard_normal((3, 50, 9)).astype(np.float32)
    a1, a2 = np.float32(1.37), np.float32(0.81)
    c0, c1 = rng.standard_normal(3).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    tn, R = LC.cheby_ref(LC.INIT, acc, tc, None, R0, a1, a2, c0, c1)
    assert tn.dtype == np.float32 and R.dtype == np.float32
    t1 = ((acc - (a2 * tc).astype(np.float32)).astype(np.float32) / a1).astype(np.float32)
    assert np.array_equal(tn, t1)
    once = ((acc.astype(np.float64) - np.float64(a2) * tc) / np.float64(a1)).astype(np.float32)
    assert not np.array_equal(tn, once)
    assert np.array_equal(R[1], (np.float32(0.5) * c0[1]) * tc + c1[1] * tn)
    tn2, R2 = LC.cheby_ref(LC.STEP | LC.NO_T, acc, tc, to, R0, a1, a2, None, c1)
    assert tn2 is None and np.array_equal(R2[2], R0[2] + c1[2] * (acc - to))
    tn3, R3 = LC.cheby_ref(LC.INIT_T, acc, tc, None, R0, a1, a2, None, None)
    assert np.array_equal(tn3, tn) and np.array_equal(R3, R0)
    cp = np.concatenate([c0, c1])
    tn4, R4 = LC.cheby_ref(LC.STEP_FIRST, acc, tc, to, R0, a1, a2, cp, c0)
    assert np.array_equal(tn4, acc - to)
    assert np.array_equal(R4[0], ((np.float32(0.5) * c0[0]) * to + c1[0] * tc) + c0[0] * tn4)
    y, prev = acc, tc
    w = np.float32(0.37)
    assert np.array_equal(LC.agg_ref(prev, 0.37, y), prev + (w * y))
    assert np.array_equal(LC.agg_ref(prev, 0.37, y, init=True), np.float32(0) + (w * y))
    assert LC.agg_ref(prev, 0.37, y).dtype == np.float32
