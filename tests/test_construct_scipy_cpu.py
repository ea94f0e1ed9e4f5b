"""construct_adj on weighted graphs against scipy's own arithmetic (CPU).

Â is promised to be the reference's fp64 scipy arithmetic bit for bit.  With binary or dyadic
weights every summation order gives the same bits, so these tests use weights that show the order:
  * oracle.row_sum_numpy (a[0] + numpy's pairwise sum of a[1:]) is pinned to csr.sum(1) of the
    installed scipy on one row of every length -- the test that notices a scipy or numpy whose
    order changes;
  * the data is shown to distinguish that order from a left-to-right sum and from five near misses;
  * the oracle's sym_norm / ppr_norm and the host logic of srgnn.construct equal the cw_* fixtures,
    which hold the reference's own Â (tests/golden/make_golden_construct.py): non-dyadic weights,
    and zero / negative degrees, where sp.diags drops an entry by its zero factor even when the
    other factor is NaN.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import construct_cases as CC
from srgnn import construct as C
from test_construct_cpu import mirror_np, segsum_np

KINDS = ("decades", "signed")


def scipy_row_sums(ptr, v):
    """csr.sum(1) of a matrix whose row s holds segment s (columns 0 .. len-1)."""
    lens = np.diff(ptr)
    cols = np.concatenate([np.arange(k) for k in lens]) if lens.size else np.zeros(0)
    a = sp.csr_matrix((v, cols.astype(np.int32), ptr.astype(np.int32)), shape=(lens.size, max(int(lens.max()), 1)))
    return np.asarray(a.sum(1)).ravel()


@pytest.fixture(scope="module")
def sums(oracle_mod):
    """Per value kind: ptr, values, scipy's row sums and the restatement's, computed once."""
    out = {}
    for i, kind in enumerate(KINDS):
        ptr, v = CC.ladder(kind, seed=40 + i, extra=(1000, 4097))
        out[kind] = (ptr, v, scipy_row_sums(ptr, v), oracle_mod.row_sum_numpy(ptr, v))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_row_sum_numpy_equals_installed_scipy(sums, kind):
    ptr, v, want, got = sums[kind]
    assert want.dtype == np.float64
    bad = np.flatnonzero(CC.bits(got) != CC.bits(want))
    assert bad.size == 0, f"segment lengths {np.diff(ptr)[bad][:20].tolist()} differ from scipy {sp.__name__}"


def test_row_sum_numpy_on_a_hub_row(oracle_mod):
    """155,868 entries (the longest row of the products-shaped graph): eleven levels of halving."""
    rng = np.random.default_rng(44)
    v = rng.standard_normal(155868) * 10.0 ** rng.integers(-3, 4, 155868)
    ptr = np.array([0, v.size], dtype=np.int64)
    assert np.array_equal(CC.bits(oracle_mod.row_sum_numpy(ptr, v)), CC.bits(scipy_row_sums(ptr, v)))


@pytest.mark.parametrize("kind", KINDS)
def test_row_sum_host_is_the_same_sum(sums, kind):
    """srgnn.construct's default for CPU tensors (np.add.reduceat, as scipy's _minor_reduce)."""
    ptr, v, want, _ = sums[kind]
    got = C.row_sum_host(torch.from_numpy(ptr), torch.from_numpy(v)).numpy()
    assert np.array_equal(CC.bits(got), CC.bits(want))


def leaves(m, block=128, align=8):
    """Leaf boundaries of the pairwise recursion over m elements."""
    if m <= block:
        return [m]
    n2 = m // 2
    n2 -= n2 % align
    return leaves(n2, block, align) + leaves(m - n2, block, align)


# mutant: (keywords of oracle.row_sum_numpy, the segment lengths whose expression tree it changes)
MUTANTS = {
    "block_64": (dict(block=64), lambda L: leaves(L - 1, block=64) != leaves(L - 1)),
    "block_256": (dict(block=256), lambda L: leaves(L - 1, block=256) != leaves(L - 1)),
    "halving_not_rounded_to_8": (dict(align=1), lambda L: leaves(L - 1, align=1) != leaves(L - 1)),
    "first_element_inside": (dict(head_outside=False), lambda L: L >= 3),
    "no_eight_accumulators": (dict(unroll=False), lambda L: L - 1 >= 8),
}


@pytest.mark.parametrize("kind", KINDS)
def test_left_to_right_sum_differs(oracle_mod, sums, kind):
    """A left-to-right sum from +0 (the order this project used for the degrees) must differ from
    scipy's on at least 3/4 of the segments with >= 16 entries, or the data could not tell the two
    apart.  Measured: 86 % (decades), 84 % (signed)."""
    ptr, v, want, _ = sums[kind]
    seq = oracle_mod.segment_sum(ptr, v)
    long_ = np.diff(ptr) >= 16
    share = float((CC.bits(seq) != CC.bits(want))[long_].mean())
    print(f"left-to-right differs on {share:.3f} of {int(long_.sum())} segments")
    assert share >= 0.75


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_of_the_restatement_differ(oracle_mod, sums, kind, mutant):
    """Each near miss of numpy's order must differ from scipy on at least half of the segments
    whose expression tree it changes, and on no other (the same tree gives the same bits).
    Measured shares, decades / signed: block_64 0.69 / 0.69, block_256 0.77 / 0.76,
    halving_not_rounded_to_8 0.62 / 0.65, first_element_inside 0.68 / 0.73,
    no_eight_accumulators 0.78 / 0.77; no difference outside."""
    ptr, v, want, _ = sums[kind]
    kw, applies = MUTANTS[mutant]
    got = oracle_mod.row_sum_numpy(ptr, v, **kw)
    differs = CC.bits(got) != CC.bits(want)
    on = np.array([bool(applies(int(L))) for L in np.diff(ptr)])
    assert on.sum() >= 20
    share = float(differs[on].mean())
    print(f"{mutant}: differs on {share:.3f} of {int(on.sum())} segments it changes, {int(differs[~on].sum())} others")
    assert share >= 0.5
    assert not differs[~on].any()


@pytest.fixture(scope="module")
def fixtures():
    return {name: CC.load(name) for name in CC.CW}


def test_fixtures_are_small_and_say_their_versions(fixtures):
    for name, z in fixtures.items():
        assert z["adj_indptr"].size - 1 <= 1300 and z["adj_data"].size <= 12000
        assert str(z["scipy_version"]) and str(z["numpy_version"])
    z = fixtures["cw_degenerate"]
    assert np.isnan(z["sym_r05_data"]).any() and (z["adj_data"] == 0).any()
    lens = np.diff(fixtures["cw_ladder"]["adj_indptr"]) + 1      # rows of A + I (no stored diagonal)
    assert {8, 9, 128, 129, 130, 137, 138, 257, 258, 1025, 1033} <= set(lens.tolist())


@pytest.mark.parametrize("name,variant,kind,r", CC.variants())
def test_oracle_equals_reference(oracle_mod, fixtures, name, variant, kind, r):
    z = fixtures[name]
    args = (z["adj_indptr"], z["adj_indices"], z["adj_data"], z["adj_indptr"].size - 1, r)
    got = oracle_mod.sym_norm(*args) if kind == "sym" else oracle_mod.ppr_norm(*args, 0.15)
    CC.assert_csr_bits(got, CC.want_of(z, variant), f"{name} {variant}")


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name,variant,kind,r", CC.variants())
def test_host_logic_equals_reference(fixtures, name, variant, kind, r, fast):
    """srgnn.construct on CPU tensors: the general path and the fast one (cw_ladder takes the
    in-place A + I merge, cw_sym also the mirror transpose, cw_degenerate falls back)."""
    z = fixtures[name]
    args = (z["adj_indptr"], z["adj_indices"], z["adj_data"], z["adj_indptr"].size - 1, r)
    kw = dict(device="cpu", segsum=segsum_np, mirror=mirror_np, fast=fast)
    got = C.sym_norm(*args, **kw) if kind == "sym" else C.ppr_norm(*args, 0.15, **kw)
    CC.assert_csr_bits([t.numpy() for t in got], CC.want_of(z, variant), f"{name} {variant} fast={fast}")


def test_fast_paths_are_the_ones_the_fixtures_name(fixtures):
    """cw_ladder and cw_sym are canonical (in-place merge); cw_sym mirrors, cw_ladder does not."""
    for name, merges, mirrors in (("cw_ladder", True, False), ("cw_sym", True, True), ("cw_degenerate", False, None)):
        a = CC.adj_of(fixtures[name])
        n = a.shape[0]
        ip = torch.from_numpy(a.indptr.astype(np.int64))
        ix = torch.from_numpy(a.indices.astype(np.int64))
        rows = torch.repeat_interleave(torch.arange(n), ip[1:] - ip[:-1])
        api = C._canonical_plus_identity(ip, ix, torch.from_numpy(a.data.astype(np.float64)), rows, n)
        assert (api is not None) == merges, name
        if api is not None:
            m = mirror_np(api[0], api[1].to(torch.int32), api[3])
            assert bool((m >= 0).all()) == mirrors, name


def test_hops_of_the_reference(oracle_mod, fixtures):
    """The stored hop panels are those of the stored Â (fp32 cast, the reference's fma chain)."""
    z = fixtures["cw_sym"]
    ip, ix, v = CC.want_of(z, "sym_r05")
    hops = oracle_mod.propagate(ip, ix, v.astype(np.float32), z["x"], 3)
    for k in (1, 2, 3):
        assert np.array_equal(CC.bits(hops[k]), CC.bits(z[f"hop{k}"])), f"hop {k}"
