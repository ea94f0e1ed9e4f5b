"""Host restatement of the sampled dense-dense product (srg_sddmm_f32, torch_sparse.spmm's value
gradient): for every entry (r, c),

    out = ((((+0 + G[r,0]*X[c,0]) + G[r,1]*X[c,1]) + ...) + G[r,d-1]*X[c,d-1]),

columns ascending, every product rounded to fp32 before it is added.  numpy's float32 multiply and add
are IEEE operations on the arrays' elements (no fused multiply-add, subnormals kept), so the loop
over the columns, vectorised over the entries, is the chain itself.
"""
import numpy as np


def sddmm_ref(rows, cols, G, X):
    """out[e] for entries (rows[e], cols[e]); G: [., d] fp32, X: [., d] fp32 (any strides)."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert G.dtype == np.float32 and X.dtype == np.float32 and G.shape[1] == X.shape[1]
    acc = np.zeros(rows.size, dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(G.shape[1]):
            acc = (acc + (G[rows, j] * X[cols, j]).astype(np.float32)).astype(np.float32)
    return acc


def csr_rows(indptr):
    """The row of every entry of a CSR."""
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def exact_and_scale(rows, cols, G, X):
    """(the fp64 dot product, sum_j |G[r,j] X[c,j]|) per entry: the bound's two sides."""
    g = G[np.asarray(rows)].astype(np.float64)
    x = X[np.asarray(cols)].astype(np.float64)
    return (g * x).sum(axis=1), np.abs(g * x).sum(axis=1)


def assert_bits(got, want, what=""):
    """Bitwise equality of two fp32 arrays; NaN positions must agree (payloads may differ)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    a, b = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} entries differ bitwise, first at {bad[:5]}: "
                           f"{got[~nan][bad[:5]]} vs {want[~nan][bad[:5]]}")
