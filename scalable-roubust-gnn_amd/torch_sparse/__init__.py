"""torch_sparse's functional API, backed by libsrgnn_hip (gfx950).

The wavelet model of the reference imports `from torch_sparse import spspmm, spmm`
(SSRG/models/base_scalable/base_model.py:13, simple_models.py:3) and its operators import
`coalesce` (SSRG/operators/utils.py:10).  torch_sparse is not installed in this image and the
reference pins no version; these are the published torch_sparse 0.6.x semantics, run on the GPU
(the package directory on sys.path makes `import torch_sparse` resolve here):

  spspmm(indexA, valueA, indexB, valueB, m, k, n, coalesced=False) -> (index [2, nnz], value)
      SparseTensor(A) @ SparseTensor(B) (spspmm_sum): per output row, the products of A's entries
      in stored order with B's rows, each rounded then added from 0; zero sums dropped; entries
      sorted by (row, col).  With coalesced=False the inputs are taken as sorted by row (torch_sparse
      builds its row pointers from them as given); coalesced=True sorts both inputs by (row, col)
      first and KEEPS duplicate entries (0.6.x builds SparseTensor(..., is_sorted=not coalesced),
      which sorts without summing, whatever its docstring says: a1*b and a2*b are rounded and added
      separately).  Parity unpinned: torch_sparse is absent and the reference never passes it.
      -> srgnn.sparse.spgemm (srg_spgemm_f32).
      Differentiable (once) in valueA and valueB, as the wavelet layers need (wavelet/src/gwnn_layer.py:
      spspmm(phi, diag(theta)) then spspmm(., phi^-1) with theta a Parameter).  For G = dL/dvalue:
        gA[(i,k)] = ((0 + G[i,j1] B[k,j1]) + G[i,j2] B[k,j2]) + ...   over row k of B in stored order,
        gB[(k,j)] = ((0 + A[i1,k] G[i1,j]) + A[i2,k] G[i2,j]) + ...   over column k of A, rows
                    ascending, duplicates in stored order,
      products rounded before they are added, G = +0 at the exact-zero sums the forward dropped,
      every duplicate entry getting the full value; with column-sorted rows that is scipy's
      (G @ B.T) sampled at A's pattern and (A.T @ G) at B's.  Gradients arrive in the caller's entry
      order on the caller's device; only the sides that require grad are computed.
      -> srgnn.sparse.spgemm_grad (srg_spgemm_grad_f32).
  spmm(index, value, m, n, matrix) -> [m, ...] dense
      index_select, mul, scatter_add: each output row is the sum of its entries' rounded products in
      index order from 0 -> srgnn.sparse.spmm_scatter (srg_spmm_muladd_f32); differentiable (once) in
      `matrix` (the adjoint scatter runs through the same kernel) and in `value`:
        g_value[(r,c)] = ((0 + G[r,0] matrix[c,0]) + G[r,1] matrix[c,1]) + ...   columns ascending,
      products rounded before they are added, every duplicate entry getting the full value, in the
      caller's entry order -> srgnn.sparse.sddmm (srg_sddmm_f32).  torch_sparse's own value gradient
      is torch's vectorised sum, whose order depends on the host's SIMD width; this chain is pinned
      by its host restatement and lies within d * 2^-24 / (1 - d * 2^-24) * sum |G[r,j] matrix[c,j]|
      of the exact dot product.  Only the sides that require grad are computed.
  coalesce(index, value, m, n, op="add") -> (index, value)
      sorted by row * n + col, each run of equal keys summed in order (srgnn.directed).

Inputs may live on the host (as in the reference): they are moved to the current HIP device, and
the results come back to the inputs' device.  No CPU fallback: without a HIP device these raise.
Computation is fp32 (the reference passes torch.FloatTensor values).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

__version__ = "0.6.x-srgnn-hip"

__all__ = ["spspmm", "spmm", "coalesce", "transpose"]


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("torch_sparse (srgnn HIP build) needs a HIP device")
    return torch.device("cuda", torch.cuda.current_device())


def _on(t: torch.Tensor, dev):
    return t.to(dev) if t.device != dev else t


def _spspmm_csr(iA, vA, iB, vB, m, k, n, coalesced):
    """The product of two device COO operands: (A's CSR + its sort's permutation, B's likewise,
    C's CSR, C's COO index)."""
    from srgnn.sparse import csr_from_coo, spgemm
    # coalesced=True: both inputs sorted by (row, col), duplicates kept in their stored order
    # (torch_sparse 0.6.x: SparseTensor(row, col, value, is_sorted=not coalesced) sorts, never sums)
    a = csr_from_coo(iA[0], iA[1], vA, m, sort_cols=coalesced, return_perm=True)
    b = csr_from_coo(iB[0], iB[1], vB, k, sort_cols=coalesced, return_perm=True)
    if a[1].numel() and int(a[1].max()) >= k:
        raise ValueError(f"indexA has a column >= k = {k}")
    c = spgemm(*a[:3], *b[:3], n)
    rows = torch.repeat_interleave(torch.arange(m, device=vA.device), c[0][1:] - c[0][:-1])
    return a, b, c, torch.stack([rows, c[1].to(torch.int64)], dim=0)


class _SpSpMM(torch.autograd.Function):
    """spspmm with the adjoint of srgnn.sparse.spgemm_grad; gradients in the caller's entry order."""

    @staticmethod
    def forward(ctx, indexA, valueA, indexB, valueB, m, k, n, coalesced):
        a, b, c, index = _spspmm_csr(indexA, valueA.detach(), indexB, valueB.detach(), m, k, n, coalesced)
        ctx.save_for_backward(*a, *b, c[0], c[1])
        ctx.shape = (m, k, n)
        ctx.mark_non_differentiable(index)
        return index, c[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, _grad_index, grad):
        from srgnn.sparse import csr_transpose, spgemm_grad
        a_ip, a_ix, a_v, a_perm, b_ip, b_ix, b_v, b_perm, c_ip, c_ix = ctx.saved_tensors
        m, k, n = ctx.shape
        g = grad.contiguous()
        g_a = g_b = None
        if ctx.needs_input_grad[1]:
            # gA[(i,k)] = sum over row k of B of G[i,j] * B[k,j]; back from the row sort to the caller's order
            g_a = torch.empty_like(a_v)
            g_a[a_perm] = spgemm_grad(a_ip, a_ix, c_ip, c_ix, g, b_ip, b_ix, b_v, n, check=False)
        if ctx.needs_input_grad[3]:
            # gB[(k,j)] = sum over column k of A of A[i,k] * G[i,j]: the same kernel on the transposes
            bt_ip, bt_ix, _, bt_perm = csr_transpose(b_ip, b_ix, b_v, n)
            gt_ip, gt_ix, gt_v, _ = csr_transpose(c_ip, c_ix, g, n)
            at_ip, at_ix, at_v, _ = csr_transpose(a_ip, a_ix, a_v, k)
            g_csr = torch.empty_like(b_v)
            g_csr[bt_perm] = spgemm_grad(bt_ip, bt_ix, gt_ip, gt_ix, gt_v, at_ip, at_ix, at_v, m, check=False)
            g_b = torch.empty_like(b_v)
            g_b[b_perm] = g_csr
        return None, g_a, None, g_b, None, None, None, None


def spspmm(indexA, valueA, indexB, valueB, m, k, n, coalesced=False):
    """Matrix product of two sparse tensors in COO form (torch_sparse 0.6.x `spspmm`); differentiable
    (once) in valueA and valueB."""
    home = valueA.device
    dev = _device()
    iA, vA, iB, vB = (_on(t, dev) for t in (indexA, valueA, indexB, valueB))
    for v in (vA, vB):
        if v.dtype != torch.float32:
            raise TypeError(f"spspmm computes in float32, got {v.dtype}")
    m, k, n, coalesced = int(m), int(k), int(n), bool(coalesced)
    if torch.is_grad_enabled() and (vA.requires_grad or vB.requires_grad):
        index, value = _SpSpMM.apply(iA, vA, iB, vB, m, k, n, coalesced)
    else:
        _, _, c, index = _spspmm_csr(iA, vA, iB, vB, m, k, n, coalesced)
        value = c[2]
    return index.to(home), value.to(home)


class _SpMM(torch.autograd.Function):
    """spmm with the value gradient of srgnn.sparse.sddmm, in the caller's entry order."""

    @staticmethod
    def forward(ctx, row, col, value, m, matrix):
        from srgnn.sparse import csr_from_coo, spmm_scatter
        ip, ix, v, perm = csr_from_coo(row, col, value.detach(), m, return_perm=True)
        ctx.save_for_backward(row, col, value, matrix, ip, ix, perm)
        ctx.m = m
        return spmm_scatter(ip, ix, v, matrix.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        from srgnn.sparse import csr_from_coo, sddmm, spmm_scatter
        row, col, value, matrix, ip, ix, perm = ctx.saved_tensors
        g_val = g_mat = None
        if ctx.needs_input_grad[4]:
            # adjoint of the scatter: grad_matrix[c] = sum over entries with column c of v * grad[r]
            ip_t, ix_t, v = csr_from_coo(col, row, value.detach(), matrix.shape[0])
            g_mat = spmm_scatter(ip_t, ix_t, v, grad.contiguous())
        if ctx.needs_input_grad[2]:
            # g_val[(r,c)] = the chain over the columns of grad[r, j] * matrix[c, j]; CSR entry e is the
            # caller's entry perm[e] (the forward checked the pattern)
            g_val = sddmm(ip, ix, grad, matrix, perm=perm, check=False)
        return None, None, g_val, None, g_mat


def spmm(index, value, m, n, matrix):
    """Matrix product of a sparse matrix (COO `index`, `value`, shape m x n) with a dense matrix
    (torch_sparse 0.6.x `spmm`)."""
    if matrix.size(-2) != n:         # torch_sparse's first check (a 1-D matrix raises IndexError here)
        raise AssertionError(f"matrix has {matrix.size(-2)} rows, the sparse matrix {n} columns")
    home = matrix.device
    dev = _device()
    mat = _on(matrix, dev)
    if mat.dim() != 2:
        raise NotImplementedError("spmm: batched dense operands are not supported by this build")
    if mat.dtype != torch.float32 or value.dtype != torch.float32:
        raise TypeError("spmm computes in float32")
    idx, val = _on(index, dev), _on(value, dev)
    return _SpMM.apply(idx[0], idx[-1], val, int(m), mat.contiguous()).to(home)


def coalesce(index, value, m, n, op="add"):
    """Row-major sorted COO with duplicate entries summed in order (torch_sparse 0.6.x `coalesce`)."""
    from srgnn.directed import _coalesce, segment_sum
    if op not in ("add", "sum"):
        raise NotImplementedError(f"coalesce op={op!r}: only 'add' is supported")
    home = index.device
    dev = _device()
    idx = _on(index, dev).to(torch.int64)
    if value is None:
        r, c, _ = _coalesce(idx[0], idx[1], [], int(n), segment_sum)
        return torch.stack([r, c]).to(home), None
    val = _on(value, dev)
    cols = [val] if val.dim() == 1 else [val[:, j].contiguous() for j in range(val.shape[1])]
    r, c, out = _coalesce(idx[0], idx[1], cols, int(n), segment_sum)
    v = out[0] if val.dim() == 1 else torch.stack(out, dim=1)
    return torch.stack([r, c]).to(home), v.to(home)


def transpose(index, value, m, n, coalesced=True):
    """The transposed COO matrix (torch_sparse 0.6.x `transpose`)."""
    row, col = index[0], index[1]
    index = torch.stack([col, row], dim=0)
    if coalesced:
        return coalesce(index, value, n, m)
    return index, value
