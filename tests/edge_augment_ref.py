"""Host restatement (numpy only) of edge augmentation: the distance in srg_knn_select_f32's fixed summation
order, the (distance, position) selection with NaN last and out-of-range ids after that, the integer
arithmetic of srg_sample_distinct_i64, and the assembly of the output edge list.  include/srgnn_hip.h
states all of it; nothing here is read from the library."""
import numpy as np

QUIET_NAN = np.uint32(0x7FC00000)
KEY_NAN = np.uint32(0x7F800001)
KEY_OUTSIDE = np.uint32(0x7F800002)


def group_lanes(d):
    """G: the smallest power of two >= ceil(d / 4), at most 64 (1 for d <= 4)."""
    pieces = (d + 3) // 4
    G = 1
    while G < pieces and G < 64:
        G *= 2
    return G


def distance(xq, xc):
    """dist[p] = ||xq[p] - xc[p]||_2 for fp32 [P, d] pairs of rows (xq may be one row), in the fixed order:
    piece j // 4 of 4 columns goes to partial sum (j // 4) % G, each partial sum one chain from +0 over its
    pieces in ascending order, then the halving tree p[g] += p[g + h], h = G/2 .. 1; correctly rounded
    sqrt.  Every operation is an fp32 numpy operation (round to nearest even, subnormals kept)."""
    xc = np.ascontiguousarray(xc, dtype=np.float32)
    xq = np.broadcast_to(np.asarray(xq, dtype=np.float32), xc.shape)
    P, d = xc.shape
    with np.errstate(all="ignore"):
        t = xq - xc
        s = t * t
        G = group_lanes(d)
        pieces = (d + 3) // 4
        steps = (pieces + G - 1) // G if d else 0
        # columns past d add +0: the sums are never -0 (squares are >= +0 or NaN), so x + (+0) = x
        pad = np.zeros((P, steps * G * 4), dtype=np.float32)
        pad[:, :d] = s
        pad = pad.reshape(P, steps, G, 4)
        p = np.zeros((P, G), dtype=np.float32)
        for c in range(steps):
            for e in range(4):
                p = p + pad[:, c, :, e]
        while G > 1:
            h = G // 2
            p = p[:, :h] + p[:, h:G]
            G = h
        return np.sqrt(p[:, 0])


def keys_of(dist, inside):
    """The uint32 ordering key: a distance's bits (non-negative floats order as their bits), every NaN
    after +Inf, ids outside [0, n) after every NaN."""
    key = dist.astype(np.float32).view(np.uint32).copy()
    key[np.isnan(dist)] = KEY_NAN
    key[~inside] = KEY_OUTSIDE
    return key


def select_row(X, q, cand, k):
    """The k nearest of `cand` (ids, list order) to row q of X: (ids, distance bits as uint32), nearest
    first, ties by position, NaN after +Inf, ids outside [0, n) last (never read)."""
    n = X.shape[0]
    cand = np.asarray(cand, dtype=np.int64)
    inside = (cand >= 0) & (cand < n)
    safe = np.where(inside, cand, q)
    dist = distance(X[q], X[safe]) if cand.size else np.zeros(0, dtype=np.float32)
    key = keys_of(dist, inside)
    order = np.argsort(key, kind="stable")[:k]
    bits = np.where(key[order] <= np.uint32(0x7F800000), key[order], QUIET_NAN).astype(np.uint32)
    return cand[order], bits


def select(X, query, cand_ptr, cand, out_ptr):
    """srg_knn_select_f32 on the host: (sel int64, distance bits uint32), both [out_ptr[-1]]."""
    sel = np.zeros(int(out_ptr[-1]), dtype=np.int64)
    bits = np.zeros(int(out_ptr[-1]), dtype=np.uint32)
    for r in range(len(query)):
        k = int(out_ptr[r + 1] - out_ptr[r])
        ids, b = select_row(X, int(query[r]), cand[cand_ptr[r]:cand_ptr[r + 1]], k)
        sel[out_ptr[r]:out_ptr[r + 1]] = ids
        bits[out_ptr[r]:out_ptr[r + 1]] = b
    return sel, bits


# ---- the sampler ---------------------------------------------------------------------------------------
_U = np.uint64


def _mix(z):
    z = z ^ (z >> _U(30))
    z = z * _U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> _U(27))
    z = z * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def sample_distinct(query, cand_ptr, n, seed):
    """srg_sample_distinct_i64 on the host, uint64 arithmetic that wraps: a four-round Feistel network over
    2h bits (4^h >= n - 1, h >= 1) keyed per row, cycle-walked from t until it lands below n - 1, then
    shifted past the query node."""
    query = np.asarray(query, dtype=np.int64)
    cand_ptr = np.asarray(cand_ptr, dtype=np.int64)
    lens = np.diff(cand_ptr)
    if lens.size and lens.max() > n - 1:
        raise ValueError("a row asks for more than n - 1 distinct candidates")
    m = _U(max(n - 1, 0))
    h = 1
    while (1 << (2 * h)) < n - 1:
        h += 1
    hh, mask = _U(h), _U((1 << h) - 1)
    rows = np.repeat(np.arange(len(query), dtype=np.int64), lens)
    t = (np.arange(int(cand_ptr[-1]), dtype=np.int64) - cand_ptr[:-1][rows]).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = _mix(_U(seed & 0xFFFFFFFFFFFFFFFF) + _U(0x9E3779B97F4A7C15) * (rows.astype(np.uint64) + _U(1)))
        rk = [key ^ (_U(0xD6E8FEB86659FD93) * _U(i + 1)) for i in range(4)]
        x = t.copy()
        todo = np.ones(x.size, dtype=bool)
        while todo.any():
            idx = np.nonzero(todo)[0]
            L, R = x[idx] >> hh, x[idx] & mask
            for i in range(4):
                L, R = R, L ^ (_mix(rk[i][idx] ^ R) & mask)
            x[idx] = (L << hh) | R
            todo[idx] = x[idx] >= m
    x = x.astype(np.int64)
    return x + (x >= query[rows])


# ---- the whole function --------------------------------------------------------------------------------
def degrees(row, col, n):
    return np.bincount(np.concatenate([row, col]).astype(np.int64), minlength=n).astype(np.int64)


def low_degree_rows(row, col, n, L, per_edge=100):
    """(nodes ascending, cand_ptr, out_ptr) of the nodes with degree < L."""
    deg = degrees(row, col, n)
    nodes = np.nonzero(deg < L)[0].astype(np.int64)
    need = L - deg[nodes]
    out_ptr = np.concatenate([[0], np.cumsum(need)]).astype(np.int64)
    return nodes, out_ptr * per_edge, out_ptr


def assemble(row, col, nodes, out_ptr, sel):
    """Old and new pairs, all flipped as well, sorted by (row, col), duplicates removed: int64 [2, E]."""
    new_row = np.repeat(nodes, np.diff(out_ptr))
    r = np.concatenate([row, new_row, col, sel]).astype(np.int64)
    c = np.concatenate([col, sel, row, new_row]).astype(np.int64)
    return np.unique(np.stack([r, c]), axis=1)


def edge_augment(row, col, n, X, L, nodes, cand_ptr, cand, per_edge=100):
    """The reference's edge_index from candidate lists given per low-degree node (rows in the order of
    `nodes`, any order): selection by (distance, position), then the assembly."""
    deg = degrees(row, col, n)
    out_ptr = np.concatenate([[0], np.cumsum(L - deg[nodes])]).astype(np.int64)
    sel, _ = select(X, nodes, cand_ptr, cand, out_ptr)
    return assemble(row, col, nodes, out_ptr, sel)
