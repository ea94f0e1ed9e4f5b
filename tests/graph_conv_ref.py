"""Host restatement of srgnn.graph_conv's two row-restricted entries, built on oracle.spmm (one sequential
fp32 fma chain per element from +0 in stored order), plus the fixture reader and the rounding bound that
the tests of the full products hold against the reference's own torch.mm.

  srg_gconv_rows_f32          Y[b, :]  = chain over row rows[b] of A, every entry
  srg_gconv_rows_adjoint_f32  dX[c, :] = chain over row c of At, the entries whose column is in the batch

Both cut a sub-operator out of the CSR arrays with numpy boolean masks and hand it to oracle.spmm: entries
keep their stored order, nothing is re-sorted, and the adjoint's columns are renumbered through pos so that
they index G's rows.  A skipped entry is absent from the sub-operator; it is not an entry with a zero.
"""
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_conv.npz")
CASES = ("gc_sym05", "gc_sym03", "gc_dir05")
KINDS = {"gc_sym05": "same", "gc_sym03": "mirrored", "gc_dir05": "sorted"}
WIDTHS = (7, 47)

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def case(name):
    """(indptr int64, indices int32, values fp32) of a fixture operator."""
    g = golden()
    return g[f"{name}__indptr"], g[f"{name}__indices"], g[f"{name}__values"]


def panels(d):
    """The fixture's inputs Z and G for width d: int8 multiples of 1 / panel_scale, exact in fp32."""
    g = golden()
    s = np.float32(int(g["panel_scale"]))
    return g[f"Zq{d}"].astype(np.float32) / s, g[f"Gq{d}"].astype(np.float32) / s


def entry_rows(indptr):
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def transpose_stable(indptr, indices, values, n_cols):
    """The transpose as a stable sort of the entries by column (srgnn.sparse.csr_transpose's order)."""
    perm = np.argsort(indices, kind="stable")
    ptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(ptr, indices.astype(np.int64) + 1, 1)
    return np.cumsum(ptr), entry_rows(indptr)[perm].astype(np.int32), values[perm]


def rows_forward_ref(indptr, indices, values, rows, X):
    """Y[b] = the chain of row rows[b]; a row id outside [0, n_rows) gives +0."""
    n = indptr.size - 1
    rows = np.asarray(rows, dtype=np.int64)
    ok = (rows >= 0) & (rows < n)
    safe = np.where(ok, rows, 0)
    lens = np.where(ok, indptr[safe + 1] - indptr[safe], 0)
    sub_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # entry e of the sub-operator = entry indptr[rows[b]] + (e - sub_ptr[b]) of A
    b_of = np.repeat(np.arange(rows.size), lens)
    src = indptr[safe][b_of] + (np.arange(int(sub_ptr[-1])) - sub_ptr[b_of])
    return O.spmm(sub_ptr, indices[src], values[src], X)


def rows_adjoint_ref(indptr_t, indices_t, values_t, pos, G):
    """dX[c] = the chain over row c's entries whose column is a member (pos >= 0), in stored order, reading
    G[pos[column]]; the other entries are masked out of the CSR arrays."""
    n = indptr_t.size - 1
    pos = np.asarray(pos, dtype=np.int64)
    B = G.shape[0]
    ix = indices_t.astype(np.int64)
    inside = (ix >= 0) & (ix < pos.size)
    p = np.where(inside, pos[np.where(inside, ix, 0)], -1)
    member = (p >= 0) & (p < B)
    rows = entry_rows(indptr_t)[member]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, rows + 1, 1)
    Gp = G if B else np.zeros((1, G.shape[1]), dtype=np.float32)     # an empty batch: no entry reads it
    return O.spmm(np.cumsum(ptr), p[member].astype(np.int32), values_t[member], Gp)


def pos_of(rows, n):
    pos = np.full(n, -1, dtype=np.int32)
    pos[np.asarray(rows, dtype=np.int64)] = np.arange(len(rows), dtype=np.int32)
    return pos


def chain_bound(indptr, indices, values, X, extra=0):
    """2 gamma_len sum_e |v_e| |x_e| per element, gamma_len = len u / (1 - len u), u = 2^-24, len = the row's
    length: any two fp32 evaluations of the row's sum -- fma chain or separately rounded products, in any
    order -- each lie within gamma_len sum |v||x| of the exact sum (Higham, Accuracy and Stability, §3.1:
    len products or fmas and len - 1 additions give at most len roundings per term), so they differ by at
    most twice that.  extra: further roundings every term passes before the chain (len + extra in place of
    len).  Computed in fp64."""
    n = indptr.size - 1
    lens = np.diff(indptr).astype(np.float64) + extra
    u = 2.0 ** -24
    gamma = lens * u / (1.0 - lens * u)
    absum = np.zeros((n, X.shape[1]))
    np.add.at(absum, entry_rows(indptr), np.abs(values.astype(np.float64))[:, None]
              * np.abs(X.astype(np.float64))[indices.astype(np.int64)])
    return 2.0 * gamma[:, None] * absum


def star_graph(n=400, seed=5):
    """A symmetric 400-node operator: row 7 holds 320 entries, nodes 3 and 11 are isolated (no entry at
    all, not even a diagonal), the rest a thin random graph; values are arbitrary fp32, so the transpose is
    "mirrored"."""
    rng = np.random.default_rng(seed)
    live = np.setdiff1d(np.arange(n), [3, 11])
    e = 700
    r, c = rng.choice(live, e), rng.choice(live, e)
    star = rng.choice(np.setdiff1d(live, [7]), 319, replace=False)
    r, c = np.r_[r, np.full(star.size, 7), 7], np.r_[c, star, 7]
    r, c = np.r_[r, c], np.r_[c, r]
    key = np.unique(r.astype(np.int64) * n + c)
    r, c = key // n, key % n
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, r + 1, 1)
    ptr = np.cumsum(ptr)
    v = rng.standard_normal(key.size).astype(np.float32)
    assert ptr[8] - ptr[7] >= 300 and ptr[4] == ptr[3] and ptr[12] == ptr[11]
    return ptr, c.astype(np.int32), v
