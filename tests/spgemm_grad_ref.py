"""Host references for the adjoint of the sparse product (srg_spgemm_grad_f32, torch_sparse.spspmm's
backward): the chains restated in plain loops in fp32, the same values from scipy's products, the fp64
value of every chain and its rounding bound.

For C = A @ B (A: m x k, B: k x n) and G = dL/dC on C's pattern:
  gA[(i,k)] = ((0 + G[i,j1] B[k,j1]) + G[i,j2] B[k,j2]) + ...   over row k of B in stored order;
  gB[(k,j)] = ((0 + A[i1,k] G[i1,j]) + A[i2,k] G[i2,j]) + ...   over column k of A, rows ascending,
              duplicates in stored order (row k of A^T under a stable sort);
every product rounded before it is added, G = +0 outside C's pattern.  Both are one shape,
out[e] = chain over row col(e) of R of dense_row(e)[idx_R] * val_R, which chain_loops() evaluates.
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24."""
    return n * U / (1.0 - n * U)


def chain_loops(p_ip, p_ix, d_ip, d_ix, d_v, r_ip, r_ix, r_v, n_cols):
    """out[e] for every entry e = (r, c) of the pattern P, the chain over row c of R in stored order.
    Returns (fp32 chain, fp64 value of the same sum, sum |product| in fp64, chain length)."""
    nnz = p_ix.size
    out = np.zeros(nnz, np.float32)
    exact = np.zeros(nnz, np.float64)
    mag = np.zeros(nnz, np.float64)
    length = np.zeros(nnz, np.int64)
    dense = np.zeros(n_cols, np.float32)
    for r in range(p_ip.size - 1):
        cols = d_ix[d_ip[r]:d_ip[r + 1]]
        dense[cols] = d_v[d_ip[r]:d_ip[r + 1]]
        for e in range(p_ip[r], p_ip[r + 1]):
            c = p_ix[e]
            s = np.float32(0.0)
            x = 0.0
            a = 0.0
            for q in range(r_ip[c], r_ip[c + 1]):
                g, b = dense[r_ix[q]], r_v[q]
                s = np.float32(s + np.float32(g * b))
                x += float(g) * float(b)
                a += abs(float(g) * float(b))
            out[e], exact[e], mag[e], length[e] = s, x, a, r_ip[c + 1] - r_ip[c]
        dense[cols] = 0.0
    return out, exact, mag, length


def transpose_stable(M):
    """(M^T as csr with every row's entries in the operand's stored order, perm): entry e of the
    transpose is entry perm[e] of M."""
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    perm = np.argsort(M.indices, kind="stable")
    ip = np.zeros(M.shape[1] + 1, np.int64)
    np.cumsum(np.bincount(M.indices, minlength=M.shape[1]), out=ip[1:])
    T = sp.csr_matrix((M.data[perm], rows[perm].astype(np.int32), ip), shape=(M.shape[1], M.shape[0]))
    return T, perm


def forward_pattern(A, B):
    """C = A @ B as the forward emits it: scipy's fp32 product, columns sorted, zero sums dropped."""
    C = (A @ B).tocsr()
    C.sort_indices()
    C = C.tocoo()
    keep = C.data != 0
    return C.row[keep].astype(np.int64), C.col[keep].astype(np.int64), C.data[keep]


def g_csr(crow, ccol, g, shape):
    ip = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(crow, minlength=shape[0]), out=ip[1:])
    return sp.csr_matrix((np.asarray(g, np.float32), ccol.astype(np.int32), ip), shape=shape)


def loops_grads(A, B, G):
    """(gA, gB) by chain_loops plus each side's (exact, mag, length); A, B, G csr (G on C's pattern)."""
    m, n = G.shape
    a = chain_loops(A.indptr, A.indices, G.indptr, G.indices, G.data, B.indptr, B.indices, B.data, n)
    Bt, bperm = transpose_stable(B)
    Gt, _ = transpose_stable(G)
    At, _ = transpose_stable(A)
    bt = chain_loops(Bt.indptr, Bt.indices, Gt.indptr, Gt.indices, Gt.data, At.indptr, At.indices, At.data, m)
    b = []
    for t in bt:
        x = np.empty_like(t)
        x[bperm] = t
        b.append(x)
    return a, tuple(b)


def _sample(P, pattern):
    rows = np.repeat(np.arange(pattern.shape[0]), np.diff(pattern.indptr))
    return np.asarray(P.todense(), dtype=np.float32)[rows, pattern.indices]


def scipy_grads(A, B, G):
    """(gA, gB) as scipy's fp32 products sampled at the operands' patterns: (G @ B^T) at A's,
    (A^T @ G) at B's -- csr_matmat's chains, which are the contract's when B's rows are
    column-sorted."""
    gA = _sample(G @ B.T.tocsr(), A)
    gB = _sample(A.T.tocsr() @ G, B)
    return gA, gB


def within_bound(got, exact, mag, length):
    """|computed - exact| <= gamma_{L+1} * sum |g b| for a chain of L products."""
    return np.abs(got.astype(np.float64) - exact) <= gamma(length + 1) * mag


def rand_csr(rng, m, n, density):
    """Random fp32 csr with sorted columns and a few explicit zeros."""
    M = sp.random(m, n, density=density, format="csr", random_state=rng, dtype=np.float32)
    M.data = (rng.standard_normal(M.nnz) * 2).astype(np.float32)
    M.data[rng.random(M.nnz) < 0.05] = 0.0
    M.sort_indices()
    return M


def coo(M):
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return np.vstack([rows, M.indices]).astype(np.int64), M.data.astype(np.float32)
