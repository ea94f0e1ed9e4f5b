"""The ladder operator (tests/ladder_cases.py) on the CPU: its generator's invariants, the condition
that its data shows the order of a row's chain in the result bits, the numpy epilogue references the
GPU tests compare against (held to the oracle's own cheby_op), and the conditions the special-value
panels' references must meet for tests/test_ladder_special_gpu.py to mean something.  No GPU."""
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


# ------------------------------------------------------------------------------------------------
# the special-value panels: conditions the reference alone must meet, so that a host with
# flush-to-zero set, or a changed ladder, cannot hollow the GPU tests out
# ------------------------------------------------------------------------------------------------
SPECIAL_D = [4, 32, 100, 256]
TINY = float(np.finfo(np.float32).tiny)


def _special_product(oracle_mod, kind, dtype, d):
    ip, ix, _ = LC.operator(dtype)
    v, X = LC.special(kind, dtype, d)
    with np.errstate(all="ignore"):
        y = oracle_mod.spmm(ip, ix, v, X) if dtype == "float32" else oracle_mod.spmm64(ip, ix, v, X)
    return v, X, y


def _subnormal(a):
    return (a != 0) & (np.abs(a) < TINY)


def test_special_builders_are_what_they_say():
    d = 20
    _, _, v = LC.operator("float32")
    base = LC.x_panel("float32", d)
    for kind in LC.KINDS:
        a, b = LC.special(kind, "float32", d), LC.special(kind, "float32", d)
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b)), kind
        assert a[0].dtype == a[1].dtype == np.float32 and a[0].shape == v.shape and a[1].shape == (LC.N, d)
        if kind not in LC.SUB_SCALES:
            assert np.array_equal(a[0], v), kind
    X = LC.special("poison", "float32", d)[1]
    assert np.all(X.view(np.uint32)[[0, LC.N - 1]] == 0x7FC00000) and np.array_equal(X[1:-1], base[1:-1])
    X64 = LC.special("poison", "float64", d)[1]
    assert np.all(X64.view(np.uint64)[[0, LC.N - 1]] == 0x7FF8000000000000) and np.isfinite(X64[1:-1]).all()
    X = LC.special("inf", "float32", d)[1]
    k = (31 * np.arange(LC.N)[:, None] + 7 * np.arange(d)[None, :]) % 257
    assert np.all(X[k == 0] == np.inf) and np.all(X[k == 1] == -np.inf) and np.array_equal(X[k > 1], base[k > 1])
    assert (k == 0).sum() > 300 and (k == 1).sum() > 300
    X = LC.special("overflow", "float32", d)[1]
    assert np.isfinite(X).all() and np.array_equal(X.astype(np.float64), base.astype(np.float64) * 2.0 ** 126)
    for kind, (sv, sx) in LC.SUB_SCALES.items():
        vs, Xs = LC.special(kind, "float32", d)
        assert np.array_equal(vs.astype(np.float64), v.astype(np.float64) * 2.0 ** sv), kind     # exact: normal
        want = (LC._x64()[:, :d] * 2.0 ** sx).astype(np.float32)                               # rounded once
        assert np.array_equal(Xs, want) and (Xs > 0).all(), kind
    y0 = LC.y0_special(d).view(np.uint32)
    assert y0.shape == (LC.N, d) and y0[0, 0] == 0x80000000 and y0[3, 4] == 0x807FFFFF and y0[5, 5] == 0x7FC01234
    assert sorted(set(y0.ravel().tolist())) == sorted(LC.Y0_WORDS)
    assert 0x7FC0DEAD not in LC.Y0_WORDS                # the GPU tests' unwritten-cell sentinel


def test_special_diff_rules():
    lens = np.array([3, 0, 5])
    s = 0x7FC0DEAD
    bits = lambda *w: np.array(w, dtype=np.uint32).view(np.float32).reshape(3, -1)      # noqa: E731
    want = bits(0x3F800000, 0x7FC00000, 0x80000000, s, 0x7FC01234, 0x00000001)
    assert LC.special_diff(want.copy(), want, lens, s) is None
    # an expected NaN takes any NaN but the sentinel; payload and sign are free
    assert LC.special_diff(bits(0x3F800000, 0xFFC00000, 0x80000000, s, 0x7FC00000, 0x00000001), want, lens, s) is None
    assert "row 0 (length 3)" in LC.special_diff(bits(0x3F800000, s, 0x80000000, s, 0x7FC01234, 1), want, lens, s)
    assert "row 0" in LC.special_diff(bits(0x3F800000, 0x7F800000, 0x80000000, s, 0x7FC01234, 1), want, lens, s)
    # -0 is not +0, a flushed subnormal is seen, an overwritten sentinel is seen
    assert "row 1 (length 0), buffer column 0" in LC.special_diff(bits(0x3F800000, 0x7FC00000, 0, s, 0x7FC01234, 1), want, lens, s)
    assert "row 2 (length 5), buffer column 1" in LC.special_diff(bits(0x3F800000, 0x7FC00000, 0x80000000, s, 0x7FC01234, 0), want, lens, s)
    assert "row 1" in LC.special_diff(bits(0x3F800000, 0x7FC00000, 0x80000000, 0x7FC00000, 0x7FC01234, 1), want, lens, s)
    # rows marked exact keep their payloads
    moved = bits(0x3F800000, 0x7FC00000, 0x80000000, s, 0x7FC00000, 1)
    assert LC.special_diff(moved, want, lens, s, exact=[True, True, False]) is None
    assert "row 2" in LC.special_diff(moved, want, lens, s, exact=[False, False, True])
    w64 = np.array([[0x7FF8000000000000, 0x3FF0000000000000]], dtype=np.uint64).view(np.float64)
    g64 = np.array([[0xFFF8000000000000, 0x3FF0000000000000]], dtype=np.uint64).view(np.float64)
    assert LC.special_diff(g64, w64, np.array([1]), 0x7FF8DEADBEEF0BAD) is None


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_poison_reaches_only_the_rows_that_reference_it(oracle_mod, dtype):
    """Rows that reference neither poisoned column are bitwise the unpoisoned reference, all other rows
    NaN in every column; most rows -- of every role's lengths -- are clean, so a lane without an entry
    that gathers X[0] into the chain shows.  Measured: 3,769 of 4,096 rows clean, 2,986 of the 3,024 rows
    with at most 64 entries, 17 of the 54 rows longer than 1,064 (fp32 and fp64: the structure's)."""
    lens = LC.lengths()
    clean = LC.poison_free_rows()
    u = LC.uint_of(dtype)
    print(f"{dtype}: clean {clean.sum()} of {LC.N}; <= 64 entries {clean[lens <= 64].sum()} of {(lens <= 64).sum()}; "
          f"> 1064 entries {clean[lens > 1064].sum()} of {(lens > 1064).sum()}")
    assert clean.sum() >= 0.90 * LC.N
    assert clean[lens <= 64].sum() >= 0.95 * (lens <= 64).sum()
    assert clean[lens > 1064].sum() >= 10
    assert clean[lens == 0].all()
    for d in SPECIAL_D if dtype == "float32" else [16]:
        ip, ix, v = LC.operator(dtype)
        mul = oracle_mod.spmm if dtype == "float32" else oracle_mod.spmm64
        base = mul(ip, ix, v, LC.x_panel(dtype, d))
        _, _, y = _special_product(oracle_mod, "poison", dtype, d)
        assert np.array_equal(y[clean].view(u), base[clean].view(u)), d
        assert np.isnan(y[~clean]).all(), d


@pytest.mark.parametrize("d", SPECIAL_D)
def test_subnormal_panels_stay_subnormal(oracle_mod, d):
    """Measured over d = 4, 32, 100, 256: sub_deep 99.94 - 99.96 % of the elements of non-empty rows nonzero
    subnormals; sub_edge 85 - 89 % subnormal and 11 - 15 % normal; sub_x every X element subnormal and
    98.7 - 99.2 % of the results subnormal.  A host that flushes subnormals gives 0 % everywhere."""
    ne = LC.lengths() > 0
    _, X, y = _special_product(oracle_mod, "sub_deep", "float32", d)
    share = _subnormal(y[ne]).mean()
    print(f"d={d} sub_deep: subnormal {100 * share:.2f} %")
    assert np.isfinite(y).all() and share >= 0.99 and not y[~ne].any()
    _, X, y = _special_product(oracle_mod, "sub_edge", "float32", d)
    sub, normal = _subnormal(y[ne]).mean(), (np.abs(y[ne]) >= TINY).mean()
    print(f"d={d} sub_edge: subnormal {100 * sub:.2f} %, normal {100 * normal:.2f} %")
    assert np.isfinite(y).all() and sub >= 0.05 and normal >= 0.05
    v, X, y = _special_product(oracle_mod, "sub_x", "float32", d)
    share = _subnormal(y[ne]).mean()
    print(f"d={d} sub_x: subnormal {100 * share:.2f} %")
    assert _subnormal(X).all() and (np.abs(v) >= TINY).all() and np.isfinite(y).all() and share >= 0.95


@pytest.mark.parametrize("d", SPECIAL_D)
def test_inf_and_overflow_panels_mix_their_classes(oracle_mod, d):
    """Measured: inf about 60 / 20 / 20 % finite / infinite / NaN results; overflow 6.8 - 10.3 % infinite
    results from a finite X and no NaN (a partial sum that crossed FLT_MAX stays infinite with its sign:
    which elements are infinite depends on the chain's order)."""
    _, X, y = _special_product(oracle_mod, "inf", "float32", d)
    fin, inf, nan = np.isfinite(y).mean(), np.isinf(y).mean(), np.isnan(y).mean()
    print(f"d={d} inf: finite {100 * fin:.1f} %, infinite {100 * inf:.1f} %, NaN {100 * nan:.1f} %")
    assert min(fin, inf, nan) >= 0.10
    _, X, y = _special_product(oracle_mod, "overflow", "float32", d)
    inf = np.isinf(y).mean()
    print(f"d={d} overflow: infinite {100 * inf:.2f} %")
    assert np.isfinite(X).all() and 0.03 <= inf <= 0.30 and not np.isnan(y).any()


@pytest.mark.parametrize("d", SPECIAL_D)
def test_accumulate_from_special_words(oracle_mod, d):
    """ACCUMULATE from y0_special: the 47 empty rows come back bit for bit (payloads and -0 included),
    every NaN the start holds is a NaN in the result, and -- sub_deep on that start -- the chains that
    start from a subnormal, a zero of either sign or an infinity stay what IEEE makes of them."""
    ip, ix, v = LC.operator("float32")
    lens = LC.lengths()
    y0 = LC.y0_special(d)
    empty = lens == 0
    assert empty.sum() == 47
    for kind in (None, "sub_deep"):
        vals, X = (v, LC.x_panel("float32", d)) if kind is None else LC.special(kind, "float32", d)
        y = oracle_mod.spmm(ip, ix, vals, X, out=y0.copy(), accumulate=True)
        assert np.array_equal(y[empty].view(np.uint32), y0[empty].view(np.uint32)), kind
        assert np.isnan(y[np.isnan(y0)]).all() and np.array_equal(np.isinf(y), np.isinf(y0)), kind
    # the last y is sub_deep's: from +-0 or the smallest subnormal the result is a nonzero subnormal (as
    # 99.9 % of sub_deep's own results are); from the largest negative subnormal a negative sum ends normal
    tiny0 = (np.abs(y0) <= np.float32(2.0 ** -149)) & ~empty[:, None]
    share = _subnormal(y[tiny0]).mean()
    edge = (y0.view(np.uint32) == 0x807FFFFF) & ~empty[:, None]
    sub, normal = _subnormal(y[edge]).mean(), (np.abs(y[edge]) >= TINY).mean()
    print(f"d={d} sub_deep from y0_special: {100 * share:.2f} % of the chains from +-0 / 2^-149 end subnormal; "
          f"from -(2^-126 - 2^-149): {100 * sub:.1f} % subnormal, {100 * normal:.1f} % normal")
    assert share >= 0.99 and sub >= 0.25 and normal >= 0.25


@pytest.mark.parametrize("d", [32, 64, 100])
def test_aggregation_weight_keeps_the_products_subnormal(oracle_mod, d):
    """The aggregation epilogue's product w * acc on sub_deep: acc is a multiple of 2^-149 of magnitude up
    to a few thousand units, so 0.37 acc rounds to zero only for |acc| of one unit: at least 99 % of the
    products of non-empty rows are nonzero subnormals, and the sums with y0_special's tiny words are too."""
    ne = LC.lengths() > 0
    _, _, y = _special_product(oracle_mod, "sub_deep", "float32", d)
    p = LC.agg_ref(None, 0.37, y, init=True)
    share = _subnormal(p[ne]).mean()
    print(f"d={d}: {100 * share:.2f} % of 0.37 acc nonzero subnormals")
    assert share >= 0.99
