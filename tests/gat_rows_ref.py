"""The row-restricted GAT aggregation (srgnn.gat's rows=) restated on top of tests/gat_ref.py:
the batches the tests use, the padded cotangent that ties the batch path to the full one, and the fp64 rows
reference with its bound (evaluate_rows).  The expected values of tests/test_gat_rows_{cpu,gpu}.py and
tests/test_launch_chunks_gat_rows_gpu.py.

The batch path has the full path for a reference: with G_full zero except G_full[rows] = G, the full backward's
dHf and da_src are the batch's, da_dst[rows] is the batch's and zero elsewhere, and ds at the batch rows' entries
is the batch's compact ds.  evaluate_rows states the same thing without the full path: the formula of
gat_ref.evaluate on the graph whose rows outside the batch are emptied."""
import numpy as np

import gat_ref as R

SHAPES = ((1, 47), (3, 7), (4, 64), (2, 65))                 # 4-byte loads, a tile spanning heads, 16-byte, past a tile
GRAPHS = (("asym", False), ("sym", False), ("sym", True))
BATCHES = ("star", "isolated", "mixed37", "past_blocks129", "all", "empty")


def star_neighbour(kind, sl):
    """A source of the star row that is not the star itself."""
    ip, ix = R.graph(kind, sl)
    row = ix[ip[R.STAR]:ip[R.STAR + 1]]
    return int(row[row != R.STAR][0])


def batch(name, kind, sl):
    """The row ids (int64, unique) of a named batch on a base graph."""
    if name == "star":
        return np.array([R.STAR], dtype=np.int64)
    if name == "isolated":
        return np.array([R.ISOLATED[0]], dtype=np.int64)
    if name == "all":
        return np.arange(R.N, dtype=np.int64)
    if name == "empty":
        return np.zeros(0, dtype=np.int64)
    rng = np.random.default_rng(41 + len(name))
    if name == "mixed37":                                     # the star, an isolated node, a neighbour of the star
        fixed = np.array([R.STAR, R.ISOLATED[0], star_neighbour(kind, sl)], dtype=np.int64)
        rest = rng.choice(np.setdiff1d(np.arange(R.N), fixed), 37 - fixed.size, replace=False)
        return rng.permutation(np.r_[fixed, rest]).astype(np.int64)
    if name == "past_blocks129":                              # one row past 32 blocks of 4 row waves
        return rng.choice(R.N, 129, replace=False).astype(np.int64)
    raise KeyError(name)


def pad(G, rows, n):
    """G_full [n, .]: zero except G_full[rows] = G."""
    full = np.zeros((n,) + G.shape[1:], dtype=G.dtype)
    full[rows] = G
    return full


def eptr_of(ip, rows):
    """The prefix sum of the batch rows' lengths, int64 [B + 1]."""
    ip = np.asarray(ip, dtype=np.int64)
    return np.r_[0, np.cumsum(ip[rows + 1] - ip[rows])].astype(np.int64)


def entries_of(ip, rows):
    """The entries of A that the compact dS holds, in its order."""
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(ip[r], ip[r + 1], dtype=np.int64) for r in rows])


def pos_of(rows, n):
    pos = np.full(n, -1, dtype=np.int32)
    pos[rows] = np.arange(rows.size, dtype=np.int32)
    return pos


def restricted(ip, ix, rows):
    """(indptr, indices, kept) of the graph with every row outside the batch emptied."""
    member = np.zeros(ip.size - 1, bool)
    member[rows] = True
    kept = member[R.entry_rows(ip)]
    ptr = np.zeros(ip.size, dtype=np.int64)
    np.add.at(ptr, R.entry_rows(ip)[kept] + 1, 1)
    return np.cumsum(ptr), ix[kept], kept


COMPACT = ("out", "M", "Z", "da_dst")


def index_ref(ref, rows, ip):
    """evaluate's result (full graph or restricted, padded G) as the rows call returns it: out, M, Z and da_dst
    indexed by the batch, ds at the batch rows' entries, dHf and da_src whole; the bounds alike."""
    res = dict(band=ref["band"])
    for k in COMPACT:
        if k in ref:
            res[k], res["E_" + k] = ref[k][rows], ref["E_" + k][rows]
    for k in ("dHf", "da_src"):
        if k in ref:
            res[k], res["E_" + k] = ref[k], ref["E_" + k]
    return res


def evaluate_rows(ip, ix, Hf, a_src, a_dst, rows, slope=0.2, G=None):
    """The fp64 rows reference with its bound: gat_ref.evaluate on the restricted graph, G [B, .] padded; out, M,
    Z, da_dst [B, .], ds [nnzB, H] in the compact order, dHf and da_src [n, .]."""
    n = ip.size - 1
    ip2, ix2, kept = restricted(ip, ix, rows)
    full = R.evaluate(ip2, ix2, Hf, a_src, a_dst, slope, None if G is None else pad(G, rows, n))
    res = index_ref(full, rows, ip2)
    if G is not None:
        e = entries_of(ip2, rows)
        res["ds"], res["E_ds"] = full["ds"][e], full["E_ds"][e]
    return res
