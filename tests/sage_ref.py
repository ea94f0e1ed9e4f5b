"""GraphSAGE's mean layer on the host: the oracle's hop followed by an fp32 division (what srgnn.sage.sage_mean
must return bit for bit), and SAGEConv / the two-layer SAGE in fp64 over dense mean matrices together with the
first-order rounding bound of their fp32 evaluation (DESIGN.md 5.13 derives it).

The bound is a running error analysis: every quantity is a pair (val, err) of fp64 arrays, val the fp64 value
and err a bound on |fp32 value - val| to first order in u = 2^-24, pushed through each step:

  mean        m = (sum_j x_j) / cnt: a chain of len additions (the products by 1.0 are exact) and one division,
              at most len + 1 roundings per term: err = M err_x + (len + 1) u M |x|   (M the dense mean matrix)
  product     a b over an inner dimension K, in any summation order (Higham, Accuracy and Stability, 3.1):
              err = |a| err_b + err_a |b| + err_a err_b + (K + 2) u |a| |b|   (the + 2: the result's own rounding
              and a bias or a second product added to it)
  ReLU        1-Lipschitz: err unchanged.  Its mask in the backward pass is the one step that is not continuous:
              where |z| <= err_z the two evaluations may disagree on it, and the bound there is |g| + err_g
  log-softmax out_i = z_i - lse(z): |d lse| <= max_j err_j, plus the roundings of C exponentials (2 ulp each), C - 1
              additions, a logarithm and two subtractions on operands of magnitude |z_i - max|, |lse - max| and 1
  its backward g_z = Cot - p * sum(Cot): p = exp(out) moves by at most p (err_out + 3 u), the row sum of Cot is a
              C-term sum
"""
import numpy as np

from oracle import oracle as O

U = 2.0 ** -24


def mean_forward(ptr, idx, X, rows=None):
    """fp32 [B, d]: the oracle's chain fma(1, x, acc) from +0 in stored order, then acc / max(len, 1) correctly
    rounded (numpy's fp32 division), for every row or for `rows`."""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int32)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        lens = ptr[rows + 1] - ptr[rows]
        src = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows.tolist()] + [np.zeros(0, np.int64)]).astype(np.int64)
        ptr, idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[src]
    acc = O.spmm(ptr, idx, np.ones(idx.size, dtype=np.float32), X)
    return acc / np.maximum(np.diff(ptr), 1).astype(np.float32)[:, None]


def mean_backward(ptr, idx, n_cols, G, rows=None):
    """fp32 [n_cols, d]: G / cnt correctly rounded, then the chain over the transpose's rows, the transpose being
    the stable sort of the entries by column; with `rows` G belongs to those rows and the other rows' entries are
    left out of the chains."""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    n = ptr.size - 1
    cnt = np.maximum(np.diff(ptr), 1).astype(np.float32)
    row_of = np.repeat(np.arange(n), np.diff(ptr))
    if rows is None:
        Gs, keep, g_row = G / cnt[:, None], np.ones(idx.size, dtype=bool), row_of
    else:
        rows = np.asarray(rows, dtype=np.int64)
        pos = np.full(n, -1, dtype=np.int64)
        pos[rows] = np.arange(rows.size)
        Gs, keep, g_row = G / cnt[rows][:, None], pos[row_of] >= 0, pos[row_of]
    perm = np.argsort(idx, kind="stable")
    perm = perm[keep[perm]]
    t_ptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(t_ptr, idx[perm] + 1, 1)
    Gp = Gs if Gs.shape[0] else np.zeros((1, G.shape[1]), dtype=np.float32)
    return O.spmm(np.cumsum(t_ptr), g_row[perm].astype(np.int32), np.ones(perm.size, dtype=np.float32), Gp)


def dense_mean(ptr, idx, n_cols):
    """(M fp64 [n_rows, n_cols] with M[i, j] = multiplicity of j in row i / max(len_i, 1), len, len_t)."""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    n = ptr.size - 1
    M = np.zeros((n, n_cols))
    np.add.at(M, (np.repeat(np.arange(n), np.diff(ptr)), idx), 1.0)
    lens = np.diff(ptr).astype(np.float64)
    return M / np.maximum(lens, 1.0)[:, None], lens, np.bincount(idx, minlength=n_cols).astype(np.float64)


class V:
    """A value and the bound on its fp32 evaluation's distance from it."""

    def __init__(self, val, err=None):
        self.val = np.asarray(val, dtype=np.float64)
        self.err = np.zeros_like(self.val) if err is None else np.asarray(err, dtype=np.float64)

    @property
    def T(self):
        return V(self.val.T, self.err.T)

    def __getitem__(self, k):
        return V(self.val[k], self.err[k])


def mm(a, b):
    K = a.val.shape[1]
    A, B = np.abs(a.val), np.abs(b.val)
    return V(a.val @ b.val, A @ b.err + a.err @ B + a.err @ b.err + (K + 2) * U * (A @ B))


def add(*terms):
    val = sum(t.val for t in terms)
    return V(val, sum(t.err for t in terms) + len(terms) * U * sum(np.abs(t.val) for t in terms))


def mean(M, lens, x):
    return V(M @ x.val, M @ x.err + (lens[:, None] + 1) * U * (M @ np.abs(x.val)))


def mean_t(M, lens_t, g):
    return V(M.T @ g.val, M.T @ g.err + (lens_t[:, None] + 1) * U * (M.T @ np.abs(g.val)))


def col_sum(g):
    n = g.val.shape[0]
    return V(g.val.sum(0), g.err.sum(0) + (n + 1) * U * np.abs(g.val).sum(0))


def conv(p, M, lens, x, x_dst):
    """SAGEConv: (z, m) with z = m Wl^T + b + x_dst Wr^T."""
    m = mean(M, lens, x)
    z = add(mm(m, V(p["lin_l.weight"]).T), V(np.broadcast_to(p["lin_l.bias"], (M.shape[0], p["lin_l.bias"].size))),
            mm(x_dst, V(p["lin_r.weight"]).T))
    return z, m


def conv_backward(p, M, lens_t, g_z, m, x_dst, n_src):
    """The parameter gradients of one SAGEConv and the gradient of its sources."""
    grads = {"lin_l.weight": mm(g_z.T, m), "lin_l.bias": col_sum(g_z), "lin_r.weight": mm(g_z.T, x_dst)}
    g_src = mean_t(M, lens_t, mm(g_z, V(p["lin_l.weight"])))
    g_root = mm(g_z, V(p["lin_r.weight"]))
    pad = V(np.zeros((n_src, g_root.val.shape[1])))
    pad.val[:g_root.val.shape[0]], pad.err[:g_root.val.shape[0]] = g_root.val, g_root.err
    return grads, add(g_src, pad)


def one_layer(p, M, lens, lens_t, x, cot):
    """SAGEConv under loss = sum(out * cot): {name: V} for out and the three parameter gradients."""
    x = V(x)
    x_dst = x[:M.shape[0]]
    z, m = conv(p, M, lens, x, x_dst)
    grads, _ = conv_backward(p, M, lens_t, V(cot), m, x_dst, M.shape[1])
    return {"out": z, **grads}


def two_layer(p1, p2, mats, x, cot):
    """The two-layer SAGE (dropout 0) under loss = sum(log_softmax * cot); mats = [(M, lens, lens_t)] per layer.
    {name: V} for out and the six parameter gradients, named convs.<i>.<parameter>."""
    (M1, l1, t1), (M2, l2, t2) = mats
    x, cot = V(x), np.asarray(cot, dtype=np.float64)
    x1 = x[:M1.shape[0]]
    z1, m1 = conv(p1, M1, l1, x, x1)
    h = V(np.maximum(z1.val, 0.0), z1.err)
    h2 = h[:M2.shape[0]]
    z2, m2 = conv(p2, M2, l2, h, h2)
    C = z2.val.shape[1]
    zmax = z2.val.max(1, keepdims=True)
    lse = zmax + np.log(np.exp(z2.val - zmax).sum(1, keepdims=True))
    out = V(z2.val - lse, z2.err + z2.err.max(1, keepdims=True)
            + (C + 8) * U * (1.0 + np.abs(z2.val - zmax) + np.abs(lse - zmax)))
    prob = np.exp(out.val)
    s = cot.sum(1, keepdims=True)
    g_z2 = V(cot - prob * s, prob * (out.err + 3 * U) * np.abs(s) + (C + 1) * U * prob * np.abs(cot).sum(1, keepdims=True)
             + 2 * U * (np.abs(cot) + prob * np.abs(s)))
    grads2, g_h = conv_backward(p2, M2, t2, g_z2, m2, h2, M2.shape[1])
    sure = np.abs(z1.val) > z1.err
    mask = z1.val > 0
    g_z1 = V(g_h.val * mask, np.where(sure, g_h.err * mask, np.abs(g_h.val) + g_h.err))
    grads1, _ = conv_backward(p1, M1, t1, g_z1, m1, x1, M1.shape[1])
    res = {"out": out}
    res.update({f"convs.0.{k}": g for k, g in grads1.items()})
    res.update({f"convs.1.{k}": g for k, g in grads2.items()})
    return res


def worst_ratio(got, want):
    """max |got - want.val| / want.err over the elements (0 where both vanish)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want.val)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / want.err)
    return float(r.max()) if r.size else 0.0
