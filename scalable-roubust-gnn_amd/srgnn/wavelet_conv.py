"""The graph-wavelet filter Y = phi diag(theta) phi^-1 Z on the device without its n x n product.

The reference's wavelet layers (SSRG simple_models.py:296-386, wavelet/src/gwnn_layer.py) form
phi diag(theta) phi^-1 with two spspmm calls per forward and multiply it into an [n, d] panel with spmm;
that product is close to dense whatever the sparsity of phi.  wavelet_conv evaluates the same operator
re-associated, Y = phi (theta (.) (phi^-1 Z)), over the bases' own entries:

  forward   P  = phi^-1 Z                           srg_spmm_scaled_f32, no scale
            Y  = (phi diag theta) P                 srg_spmm_scaled_f32, scale by column
  backward  gP = (phi diag theta)^T G               srg_spmm_scaled_f32 on phi^T, scale by row
            gZ = phi^-T gP                          srg_spmm_scaled_f32 on phi^-T, no scale
            gtheta[k] = sum_i phi[i,k] <G[i], P[k]> srg_sddmm_rowsum_f32 on phi^T

All fp32; every output element is one sequential chain from +0 in the stored order of the CSR row it
runs over, every product rounded before it is added, the rescaled value fl(phi[i,k] theta[k]) rounded
first (what spspmm(phi, diag theta) produces).  phi^T and phi^-T are srgnn.sparse.csr_transpose's stable
transposes.  With phi sorted by (row, column) and unique, and no rescaled value an exact zero, Y, gZ and
gtheta are bit for bit torch_sparse.spmm(*spspmm(phi, diag theta), n, n, spmm(phi^-1, n, n, Z)) and its
autograd; against the reference's association (the product formed first) they differ in rounding only,
within the bound of DESIGN.md §5.7.4.  The path is opt-in: torch_sparse.spspmm / spmm are unchanged.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .sparse import _panel, csr_from_coo, csr_transpose

__all__ = ["WaveletOperator", "wavelet_conv", "spmm_scaled", "sddmm_rowsum"]


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("srgnn.wavelet_conv needs a HIP device")
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def spmm_scaled(ip, ix, v, X: torch.Tensor, scale: torch.Tensor | None = None, scale_axis: int = 0,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """Y[r, j] = chain over row r of the device CSR (ip, ix, v), in stored order from +0, of
    fl(fl(v_e * scale[s_e]) * X[ix[e], j]) with s_e = ix[e] (scale_axis 0) or r (scale_axis 1); without
    `scale` the bits of srgnn.sparse.spmm_scatter (srg_spmm_scaled_f32).  The CSR is trusted: its ids
    index X's rows (WaveletOperator checks that once).  X and out may be column windows."""
    dev = ip.device
    n_rows = ip.numel() - 1
    X, ldx = _panel(X, "X", dev)
    d = X.shape[1]
    if v.dtype != torch.float32 or ix.dtype != torch.int32 or ip.dtype != torch.int64:
        raise TypeError("spmm_scaled takes an int64 / int32 / float32 CSR")
    if scale is not None:
        if scale.dtype != torch.float32 or scale.device != dev or scale.dim() != 1 or not scale.is_contiguous():
            raise ValueError("scale must be a contiguous 1-D float32 tensor on the CSR's device")
        if scale_axis == 1 and scale.numel() != n_rows:
            raise ValueError(f"a row scale has {scale.numel()} entries, the CSR {n_rows} rows")
        if scale_axis == 0 and scale.numel() != X.shape[0]:
            raise ValueError(f"a column scale has {scale.numel()} entries, X {X.shape[0]} rows")
    if out is None:
        out = torch.empty((n_rows, d), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or out.dim() != 2 or tuple(out.shape) != (n_rows, d)
          or (d > 1 and out.stride(1) != 1) or (n_rows > 1 and out.stride(0) < d)):
        raise ValueError(f"out must be a float32 [{n_rows}, {d}] tensor with unit column stride on {dev}")
    ldy = out.stride(0) if n_rows > 1 else d
    _lib.call(dev, "srg_spmm_scaled_f32", ip.data_ptr(), _ptr(ix), _ptr(v), _ptr(scale), int(scale_axis), n_rows,
              _ptr(X), ldx, _ptr(out), ldy, d, _lib.stream(dev))
    return out


def sddmm_rowsum(ip, ix, v, G: torch.Tensor, P: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[k] = chain over row k of the device CSR, in stored order from +0, of fl(v_e * s_e) with
    s_e = chain over j ascending of fl(G[ix[e], j] * P[k, j]) (srg_sddmm_rowsum_f32).  Empty rows and
    d == 0 give +0.  The CSR is trusted: its ids index G's rows."""
    dev = ip.device
    n_rows = ip.numel() - 1
    G, ldg = _panel(G, "G", dev)
    P, ldp = _panel(P, "P", dev)
    if G.shape[1] != P.shape[1]:
        raise ValueError(f"G has {G.shape[1]} columns, P {P.shape[1]}")
    if P.shape[0] != n_rows:
        raise ValueError(f"the CSR has {n_rows} rows, P {P.shape[0]}")
    if v.dtype != torch.float32 or ix.dtype != torch.int32 or ip.dtype != torch.int64:
        raise TypeError("sddmm_rowsum takes an int64 / int32 / float32 CSR")
    if out is None:
        out = torch.empty(n_rows, dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.numel() != n_rows
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 [{n_rows}] tensor on {dev}")
    _lib.call(dev, "srg_sddmm_rowsum_f32", ip.data_ptr(), _ptr(ix), _ptr(v), n_rows, _ptr(G), ldg, _ptr(P), ldp,
              G.shape[1], _ptr(out), _lib.stream(dev))
    return out


class WaveletOperator:
    """The device CSRs of one wavelet basis: phi, phi^T, phi^-1 and phi^-T, each with its values.  Built
    once per basis from the reference's own COO layout ([2, nnz] long indices, float values; host or
    device), entries kept in their stored order within a row (a stable sort by row).  check=True reads
    the indices back once and rejects ids outside [0, n), so a bad id never becomes an address."""

    def __init__(self, phi_indices, phi_values, phi_inverse_indices, phi_inverse_values, n: int, check: bool = True):
        dev = _device()
        self.n = int(n)
        self.device = dev
        csrs = []
        for name, idx, val in (("phi", phi_indices, phi_values), ("phi_inverse", phi_inverse_indices,
                                                                  phi_inverse_values)):
            if val.requires_grad:
                raise ValueError(f"{name}'s values require grad: the basis is not a parameter of wavelet_conv")
            if val.dtype != torch.float32:
                raise TypeError(f"wavelet_conv computes in fp32, {name}'s values are {val.dtype}")
            if idx.dim() != 2 or idx.shape[0] != 2 or val.dim() != 1 or idx.shape[1] != val.numel():
                raise ValueError(f"{name} must be COO: indices [2, nnz] and values [nnz]")
            if idx.dtype not in (torch.int64, torch.int32):
                raise TypeError(f"{name}'s indices must be integers, got {idx.dtype}")
            if check and idx.numel():
                host = idx.detach().cpu()
                if int(host.min()) < 0 or int(host.max()) >= self.n:
                    raise ValueError(f"{name} has an index outside [0, {self.n})")
            idx, val = idx.detach().to(dev), val.detach().to(dev)
            ip, ix, v = csr_from_coo(idx[0], idx[1], val, self.n)
            csrs.append((ip, ix, v))
            csrs.append(csr_transpose(ip, ix, v, self.n)[:3])
        self.phi, self.phi_t, self.phi_inv, self.phi_inv_t = csrs

    @property
    def nnz(self):
        return self.phi[1].numel(), self.phi_inv[1].numel()


class _WaveletConv(torch.autograd.Function):

    @staticmethod
    def forward(ctx, op, theta, Z):
        th = theta.detach().reshape(-1).contiguous()
        P = spmm_scaled(*op.phi_inv, Z.detach())
        Y = spmm_scaled(*op.phi, P, scale=th, scale_axis=0)
        ctx.op = op
        ctx.theta_shape = theta.shape
        ctx.save_for_backward(th, P)
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        op = ctx.op
        th, P = ctx.saved_tensors
        g_theta = g_z = None
        if ctx.needs_input_grad[2]:
            gP = spmm_scaled(*op.phi_t, grad, scale=th, scale_axis=1)
            g_z = spmm_scaled(*op.phi_inv_t, gP)
        if ctx.needs_input_grad[1]:
            g_theta = sddmm_rowsum(*op.phi_t, grad, P).reshape(ctx.theta_shape)
        return None, g_theta, g_z


def wavelet_conv(op: WaveletOperator, theta: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """phi diag(theta) phi^-1 Z as phi (theta (.) (phi^-1 Z)): [n, d] fp32, differentiable (once) in
    `theta` ([n] or [n, 1], the reference's diagonal_weight_filter) and in `Z` ([n, d]); only the sides
    that require grad are computed, and the backward keeps P = phi^-1 Z, nothing of size nnz.  Inputs on
    the host are moved to the operator's device and the result comes back to Z's device."""
    if not isinstance(op, WaveletOperator):
        raise TypeError("wavelet_conv takes a WaveletOperator")
    for name, t in (("theta", theta), ("Z", Z)):
        if t.dtype != torch.float32:
            raise TypeError(f"wavelet_conv computes in fp32, {name} is {t.dtype}")
    if Z.dim() != 2 or Z.shape[0] != op.n:
        raise ValueError(f"Z must be [{op.n}, d], got {tuple(Z.shape)}")
    if tuple(theta.shape) not in ((op.n,), (op.n, 1)):
        raise ValueError(f"theta must be [{op.n}] or [{op.n}, 1], got {tuple(theta.shape)}")
    home = Z.device
    th = theta.to(op.device) if theta.device != op.device else theta
    z = Z.to(op.device) if Z.device != op.device else Z
    return _WaveletConv.apply(op, th, z).to(home)
