"""Host restatement of the fused graph-wavelet filter (srgnn.wavelet_conv) and of its two C entries, in
plain numpy fp32 loops.  "chain" = a sequential sum from +0 in the stated order, every product rounded
to fp32 before it is added (numpy's float32 multiply and add are IEEE operations on the elements: no
fused multiply-add, subnormals kept).

  srg_spmm_scaled_f32   Y[r, j] = chain over row r in stored order of fl(fl(v_e scale[s_e]) X[ix[e], j])
  srg_sddmm_rowsum_f32  out[k]  = chain over row k in stored order of fl(v_e s_e),
                        s_e     = chain over j ascending of fl(G[ix[e], j] P[k, j])     (sddmm_ref)
  forward    P = phi^-1 Z (no scale);  Y = phi P scaled by theta per column
  backward   gP = phi^T G scaled by theta per row;  gZ = phi^-T gP;  gtheta = rowsum(phi^T, G, P)
with phi^T, phi^-T the stable transposes (rows ascending, duplicates in stored order).

The loops run over the position inside a row, vectorised over the rows that are that long: every
output element still sees its row's entries one at a time, in stored order.
"""
import numpy as np

from sddmm_ref import csr_rows, sddmm_ref

U = 2.0 ** -24


def gamma(m):
    """gamma_m = m u / (1 - m u), u = 2^-24."""
    return m * U / (1.0 - m * U)


def spmm_scaled_ref(indptr, indices, values, scale, scale_axis, X):
    """The restatement of srg_spmm_scaled_f32; scale None skips the rescale (srg_spmm_muladd_f32)."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    values = np.asarray(values, np.float32)
    assert X.dtype == np.float32 and scale_axis in (0, 1)
    n_rows = indptr.size - 1
    lens = np.diff(indptr)
    Y = np.zeros((n_rows, X.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        w = values
        if scale is not None:
            assert scale.dtype == np.float32
            s = scale[csr_rows(indptr)] if scale_axis == 1 else scale[indices]
            w = (values * s).astype(np.float32)
        for p in range(int(lens.max()) if n_rows else 0):
            rows = np.flatnonzero(lens > p)
            e = indptr[rows] + p
            Y[rows] = (Y[rows] + (w[e, None] * X[indices[e]]).astype(np.float32)).astype(np.float32)
    return Y


def sddmm_rowsum_ref(indptr, indices, values, G, P):
    """The restatement of srg_sddmm_rowsum_f32 (d == 0: every s_e is +0 and every row's sum is +0)."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    values = np.asarray(values, np.float32)
    n_rows = indptr.size - 1
    out = np.zeros(n_rows, np.float32)
    if G.shape[1] == 0:
        return out
    lens = np.diff(indptr)
    with np.errstate(all="ignore"):
        s = sddmm_ref(indices, csr_rows(indptr), G, P)      # G's row by the entry's id, P's by its row
        t = (values * s).astype(np.float32)
        for p in range(int(lens.max()) if n_rows else 0):
            rows = np.flatnonzero(lens > p)
            out[rows] = (out[rows] + t[indptr[rows] + p]).astype(np.float32)
    return out


def transpose_stable(indptr, indices, values, n_cols):
    """(indptr, indices, values) of the transpose, every row's entries with the operand's rows
    ascending and equal (row, column) pairs in stored order: srgnn.sparse.csr_transpose."""
    indices = np.asarray(indices, np.int64)
    rows = csr_rows(indptr)
    perm = np.argsort(indices, kind="stable")
    ip = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n_cols), out=ip[1:])
    return ip, rows[perm].astype(np.int32), np.asarray(values, np.float32)[perm]


def forward_ref(phi, phi_inv, theta, Z):
    """(Y, P) for csr triples phi, phi_inv = (indptr, indices, values)."""
    P = spmm_scaled_ref(*phi_inv, None, 0, Z)
    return spmm_scaled_ref(*phi, theta, 0, P), P


def backward_ref(phi, phi_inv, theta, P, G):
    """(gP, gZ, gtheta) for G = dL/dY."""
    n = theta.size
    phi_t = transpose_stable(*phi, n)
    gP = spmm_scaled_ref(*phi_t, theta, 1, G)
    gZ = spmm_scaled_ref(*transpose_stable(*phi_inv, n), None, 0, gP)
    return gP, gZ, sddmm_rowsum_ref(*phi_t, G, P)


def dense64(csr, n):
    ip, ix, v = csr
    M = np.zeros((ip.size - 1, n), np.float64)
    np.add.at(M, (csr_rows(ip), np.asarray(ix, np.int64)), np.asarray(v, np.float64))
    return M


def longest_row(indptr):
    return int(np.diff(indptr).max()) if len(indptr) > 1 else 0
