"""Link classification on the host: what srgnn.link's EdgeBatch, srg_pair_gather_add_f32, srg_pair_segment_sum_f32
and pair_linear compute, restated with numpy loops, and the first-order rounding bounds of DESIGN.md 5.14 against an
fp64 evaluation of the reference's formula

    out = linear(cat(z[q[:, 0]], z[q[:, 1]], dim=-1))

(the edge head of SSRG/models/base_scalable/simple_models.py; the relabelling is link_cls_mini_batch_train's,
SSRG/tasks/utils.py, restated with searchsorted).  Nothing here imports the package under test."""
import numpy as np

U32 = 2.0 ** -24            # the unit roundoff of fp32


# ---- the relabelling --------------------------------------------------------------------------------
def relabel(edges, n):
    """(n_id, local) of int pairs [E, 2] over n nodes: the sorted distinct endpoints (the reference's
    torch.unique(...) as train_idx) and each endpoint's position among them (its node_idx_map_dict lookups).
    Negative ids wrap as torch indexing does."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = np.where(e < 0, e + n, e)
    n_id = np.unique(e.reshape(-1))
    local = np.searchsorted(n_id, e).astype(np.int64).reshape(-1, 2)
    return n_id.astype(np.int64), local


def incidence(local, U):
    """(inc_ptr [U + 1], inc_slot [2E]): slot 2 e + side is endpoint `side` of pair e; the slots of node v are
    inc_slot[inc_ptr[v] : inc_ptr[v + 1]], ascending.  Plain loops."""
    flat = np.asarray(local, dtype=np.int64).reshape(-1)
    lists = [[] for _ in range(U)]
    for slot, v in enumerate(flat.tolist()):
        lists[v].append(slot)
    inc_ptr = np.zeros(U + 1, dtype=np.int64)
    for v in range(U):
        inc_ptr[v + 1] = inc_ptr[v] + len(lists[v])
    inc_slot = np.array([s for l in lists for s in l], dtype=np.int64)
    return inc_ptr, inc_slot


# ---- the two entries --------------------------------------------------------------------------------
def gather_add(P, q, b, U=None):
    """out[e, c] = (P[q[e, 0], c] + P[q[e, 1], C + c]) + b[c] in fp32, one element at a time; a position outside
    [0, U) reads as a row of +0."""
    P = np.asarray(P, dtype=np.float32)
    U = P.shape[0] if U is None else U
    C = P.shape[1] // 2
    q = np.asarray(q, dtype=np.int64).reshape(-1, 2)
    zero = np.zeros(C, dtype=np.float32)
    out = np.empty((q.shape[0], C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for e, (a, c) in enumerate(q.tolist()):
            p0 = P[a, :C] if 0 <= a < U else zero
            p1 = P[c, C:] if 0 <= c < U else zero
            r = p0 + p1
            out[e] = r + b if b is not None else r
    return out


def segment_sum(g, inc_ptr, inc_slot, U):
    """S[v, side C + c]: one fp32 chain from +0 over node v's slots of that side in stored order, a slot outside
    [0, 2E) skipped: the plain loop."""
    g = np.asarray(g, dtype=np.float32)
    E, C = g.shape
    S = np.zeros((U, 2 * C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for v in range(U):
            for j in range(max(int(inc_ptr[v]), 0), min(int(inc_ptr[v + 1]), 2 * E)):
                slot = int(inc_slot[j])
                if not 0 <= slot < 2 * E:
                    continue
                e, side = slot >> 1, slot & 1
                S[v, side * C:(side + 1) * C] = S[v, side * C:(side + 1) * C] + g[e]
    return S


def same_bits(got, want):
    """array_equal on the bits, with every NaN equal to every NaN (the sign of zero is checked)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn]))


# ---- the reference's formula in fp64 and the bounds -------------------------------------------------
def reference64(z, q, W, b, g=None):
    """The reference's head in fp64 on fp32 inputs: out [E, C] and its term sum |b| + sum_k |W||x|; with g
    (d out) also (dz, T_z, dW, T_W, db, T_b): the exact gradients and their term sums sum |g||W|, sum |g||x|,
    sum |g|."""
    z, W = np.asarray(z, dtype=np.float64), np.asarray(W, dtype=np.float64)
    q = np.asarray(q, dtype=np.int64).reshape(-1, 2)
    x = np.concatenate([z[q[:, 0]], z[q[:, 1]]], axis=1)             # [E, 2h]
    bb = np.zeros(W.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
    out = x @ W.T + bb
    T_out = np.abs(x) @ np.abs(W).T + np.abs(bb)
    if g is None:
        return out, T_out
    g = np.asarray(g, dtype=np.float64)
    h = z.shape[1]
    dx, T_x = g @ W, np.abs(g) @ np.abs(W)                           # [E, 2h]
    dz, T_z = np.zeros_like(z), np.zeros_like(z)
    for side in (0, 1):
        np.add.at(dz, q[:, side], dx[:, side * h:(side + 1) * h])
        np.add.at(T_z, q[:, side], T_x[:, side * h:(side + 1) * h])
    return out, T_out, dz, T_z, g.T @ x, np.abs(g).T @ np.abs(x), g.sum(0), np.abs(g).sum(0)


def slot_counts(q, U):
    """m [U]: the number of slots (both sides) of every node."""
    return np.bincount(np.asarray(q, dtype=np.int64).reshape(-1), minlength=U)


def forward_bound(T_out, h):
    """|out - exact| <= (h + 3) u (|b| + sum_k |W||x|): h roundings through a side's product, one for the add
    of the two sides, one for the bias, one spare."""
    return (h + 3) * U32 * T_out


def backward_bounds(T_z, T_W, T_b, m, C, E):
    """(dz, dW, db) bounds: a term of dz passes its segment's chain (at most m - 1 adds), a product of C terms
    and the add of the two sides: (m + C + 2) u sum |g||W| per node; a term of dW its segment's chain and a
    product over the U nodes that have a slot: (max m + U + 2) u sum |g||x|; db is E terms."""
    m = np.asarray(m, dtype=np.float64)
    mmax = float(m.max()) if m.size else 0.0
    return ((m[:, None] + C + 2) * U32 * T_z, (mmax + np.count_nonzero(m) + 2) * U32 * T_W, max(E, 1) * U32 * T_b)
