"""Shared by the weighted construct_adj tests (CPU and GPU): the cw_* fixtures written by
tests/golden/make_golden_construct.py, the segment ladder, and the bitwise comparison."""
import os

import numpy as np

import golden_cases as G

CW = ("cw_ladder", "cw_sym", "cw_degenerate")
# one segment of every length 0..300 and around numpy's pairwise-sum boundaries: the first split
# (a[1:] longer than 128), halves that are / are not multiples of 8, the second level of splits
LADDER = tuple(range(301)) + (511, 512, 513, 1023, 1024, 1025, 1032, 1033)


def ladder(kind, seed, extra=(), shuffle=False, empty_ends=False, dtype=np.float64):
    """(ptr int64, values) with one segment per length of LADDER + extra.
    kind "decades": normal * 10^[-3, 3]; "signed": +-U[0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    lens = np.array(LADDER + tuple(extra), dtype=np.int64)
    if shuffle:
        rng.shuffle(lens)
    if empty_ends:
        lens = np.r_[0, 0, lens, 0]
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    m = int(ptr[-1])
    if kind == "decades":
        v = rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)
    else:
        v = (rng.random(m) + 0.5) * rng.choice([-1.0, 1.0], m)
    return ptr, v.astype(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def variants():
    """(fixture, variant, kind, r) of every stored Â."""
    m = G.manifest()
    out = []
    for name in CW:
        for v in m[name]["variants"]:
            kind, tag = v.split("_r")
            out.append((name, v, kind, {"03": 0.3, "05": 0.5}[tag]))
    return out


def load(name):
    return np.load(os.path.join(G.GOLDEN, name + ".npz"), allow_pickle=False)


def adj_of(z):
    import scipy.sparse as sp
    n = z["adj_indptr"].size - 1
    return sp.csr_matrix((z["adj_data"], z["adj_indices"], z["adj_indptr"].astype(np.int32)), shape=(n, n))


def assert_csr_bits(got, want, what=""):
    """Structure exactly; values by bits, NaN by position (NaN payloads are not pinned)."""
    gp, gi, gv = (np.asarray(a) for a in got)
    wp, wi, wv = (np.asarray(a) for a in want)
    np.testing.assert_array_equal(gp, wp, err_msg=f"{what}: indptr")
    np.testing.assert_array_equal(gi, wi, err_msg=f"{what}: indices")
    assert gv.dtype == np.float64 and wv.dtype == np.float64
    nan = np.isnan(wv)
    np.testing.assert_array_equal(np.isnan(gv), nan, err_msg=f"{what}: NaN positions")
    diff = bits(gv[~nan]) != bits(wv[~nan])
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} fp64 values differ from the reference's bits"


def want_of(z, variant):
    return z[f"{variant}_indptr"], z[f"{variant}_indices"], z[f"{variant}_data"]
