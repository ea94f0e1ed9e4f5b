"""Graph attention on the device: a fused GAT layer, forward and backward.

The reference's runner trains a GAT baseline (model.py: GATConv with 8 heads and hidden 256).  Its aggregation
is a sparse product whose values are computed per edge and per head -- a leaky-ReLU score, then a softmax
over each target's incoming edges -- and differentiated through in every step.  Written with torch
primitives it materialises [nnz, H] scores and an [nnz, H, C] message tensor; here it is three entries of
libsrgnn_hip that keep nothing per edge but an [nnz, H] gradient of the scores in the backward:

  out, M, Z      = srg_gat_attend_f32            the softmax statistics and the weighted gather, over A
  ds, da_dst     = srg_gat_edge_grad_f32         the gradient of the scores, over A
  dHf, da_src    = srg_gat_attend_adjoint_f32    the adjoint gather and the source sums, over At and perm

and, for the last layer, whose output the loss reads at a batch of rows only (rows=), the
same three for those rows: srg_gat_attend_rows_f32, srg_gat_edge_grad_rows_f32 and
srg_gat_attend_rows_adjoint_f32 keep out, M, Z, D and the gradient of the scores for the batch alone and give,
on finite operands, the bits of the full path with a cotangent that is zero outside the batch.

GATGraph holds the structure (A over targets, its transpose and the permutation between them), built once;
gat_attend is the differentiable aggregation (attend_forward and attend_backward are the same calls without
autograd, supported for callers who keep M and Z themselves); GATConv and GAT are the layer and the model with PyG's
parameter names and shapes.  The arithmetic restates PyG's published formula (PyG itself is absent: parity
against its bits is unpinned); the softmax's `+ 1e-16` in the denominator is absorbed by z >= 1 in fp32 and
left out.  There is no torch fallback: every aggregation is a kernel of libsrgnn_hip.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .sparse import _panel, csr_from_coo, csr_transpose

__all__ = ["GATGraph", "gat_attend", "attend_forward", "attend_backward", "GATConv", "GAT"]


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class GATGraph:
    """The structure a GAT layer aggregates over, built once:

      indptr, indices        A, a CSR over targets: row i holds the sources of i's incoming edges in stored
                             order (a row of PyG's adj_t); int64 / int32
      indptr_t, indices_t    At, csr_transpose's stable sort by source: row j holds the targets of j's edges
      perm                   entry t of At is entry perm[t] of A

    add_self_loops=True does what PyG's GATConv does to its input: existing diagonal entries are removed, one
    is added per node and every row is sorted by source.  Without it the entries keep the order they came in.
    Duplicate edges are kept (each takes part in the softmax); values are ignored: GAT has no edge weights."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, n: int, has_self_loops: bool):
        if indptr.dtype != torch.int64 or indptr.dim() != 1 or indptr.numel() != n + 1:
            raise ValueError(f"indptr must be a 1-D int64 tensor of {n + 1} entries")
        if indices.dtype != torch.int32 or indices.dim() != 1 or indices.device != indptr.device:
            raise ValueError("indices must be a 1-D int32 tensor on indptr's device")
        self.n = int(n)
        self.indptr, self.indices = indptr.contiguous(), indices.contiguous()
        self.has_self_loops = bool(has_self_loops)
        dummy = torch.zeros(indices.numel(), dtype=torch.int8, device=indices.device)
        t_ip, t_ix, _, perm = csr_transpose(self.indptr, self.indices, dummy, self.n)
        self.indptr_t, self.indices_t, self.perm = t_ip, t_ix, perm.contiguous()

    @property
    def device(self):
        return self.indptr.device

    @property
    def nnz(self) -> int:
        return self.indices.numel()

    @classmethod
    def _build(cls, dst, src, n, add_self_loops, device):
        n = int(n)
        dst, src = dst.reshape(-1).to(torch.int64), src.reshape(-1).to(torch.int64)
        if device is not None:
            dst, src = dst.to(device), src.to(device)
        if n < 0 or n > 2 ** 31 - 65:
            raise ValueError(f"n={n} out of range [0, 2^31-64)")
        if dst.numel() and (int(min(dst.min(), src.min())) < 0 or int(max(dst.max(), src.max())) >= n):
            raise ValueError(f"a node id is out of range [0, {n})")
        if add_self_loops:
            keep = dst != src
            loops = torch.arange(n, dtype=torch.int64, device=dst.device)
            dst, src = torch.cat([dst[keep], loops]), torch.cat([src[keep], loops])
        dummy = torch.zeros(dst.numel(), dtype=torch.int8, device=dst.device)
        ip, ix, _ = csr_from_coo(dst, src, dummy, n, sort_cols=bool(add_self_loops))
        return cls(ip, ix, n, add_self_loops)

    @classmethod
    def from_edge_index(cls, edge_index, n: int, add_self_loops: bool = True, device=None) -> "GATGraph":
        """From PyG's edge_index [2, E]: row 0 the sources, row 1 the targets."""
        ei = torch.as_tensor(edge_index)
        if ei.dim() != 2 or ei.shape[0] != 2 or ei.is_floating_point():
            raise ValueError(f"edge_index must be an integer [2, E] tensor, got {tuple(ei.shape)} {ei.dtype}")
        return cls._build(ei[1], ei[0], n, add_self_loops, device)

    @classmethod
    def from_scipy(cls, adj_t, add_self_loops: bool = True, device=None) -> "GATGraph":
        """From a square scipy sparse matrix over targets (row i: the sources of i's incoming edges)."""
        import numpy as np
        import scipy.sparse as sp
        if not sp.issparse(adj_t):
            raise TypeError(f"from_scipy takes a scipy sparse matrix, got {type(adj_t).__name__}")
        if adj_t.shape[0] != adj_t.shape[1]:
            raise ValueError(f"from_scipy takes a square matrix, got {adj_t.shape}")
        csr = adj_t if sp.isspmatrix_csr(adj_t) else adj_t.tocsr()
        n = csr.shape[0]
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(csr.indptr))
        return cls._build(torch.from_numpy(rows), torch.from_numpy(csr.indices.astype(np.int64)), n, add_self_loops,
                          device)

    @classmethod
    def from_torch_sparse(cls, t, add_self_loops: bool = True, device=None) -> "GATGraph":
        """From a square torch sparse COO tensor over targets, coalesced (duplicates merged by torch)."""
        if not isinstance(t, torch.Tensor) or t.layout != torch.sparse_coo:
            raise TypeError("from_torch_sparse takes a torch sparse COO tensor")
        if t.dim() != 2 or t.dense_dim() != 0 or t.shape[0] != t.shape[1]:
            raise ValueError(f"from_torch_sparse takes a square 2-D sparse matrix, got shape {tuple(t.shape)}")
        idx = t.detach().coalesce().indices()
        if device is None and t.is_cuda:
            device = t.device
        return cls._build(idx[0], idx[1], t.shape[0], add_self_loops, device)

    @classmethod
    def from_device_csr(cls, A, add_self_loops: bool = True) -> "GATGraph":
        """From a square srgnn DeviceCSR over targets; its values are ignored."""
        from .csr import DeviceCSR
        if not isinstance(A, DeviceCSR):
            raise TypeError("from_device_csr takes a DeviceCSR")
        if A.n_rows != A.n_cols:
            raise ValueError(f"from_device_csr takes a square operator, got {A.n_rows}x{A.n_cols}")
        ip = A.indptr.to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(A.n_rows, device=ip.device), ip[1:] - ip[:-1])
        return cls._build(rows, A.indices, A.n_rows, add_self_loops, None)

    def to(self, device) -> "GATGraph":
        dev = torch.device(device)
        if dev == self.device or (dev.type == self.device.type and dev.index is None):
            return self
        g = object.__new__(GATGraph)
        g.n, g.has_self_loops = self.n, self.has_self_loops
        for k in ("indptr", "indices", "indptr_t", "indices_t", "perm"):
            setattr(g, k, getattr(self, k).to(dev))
        return g

    def __repr__(self):
        return f"GATGraph(n={self.n}, nnz={self.nnz}, self_loops={self.has_self_loops}, device={self.device})"


# ---- the three entries ------------------------------------------------------------------------------
class _Batch:
    """A batch of target rows as the rows entries take it: ids int64 [B] (unique), pos int32 [n] with
    pos[ids[b]] = b and -1 elsewhere, and, built when the backward first asks, eptr int64 [B + 1], the prefix
    sum of the batch rows' lengths, with nnzB = eptr[B]."""

    def __init__(self, graph, ids, pos):
        self.graph, self.ids, self.pos = graph, ids, pos
        self.B = ids.numel()
        self._eptr = None

    def eptr(self):
        if self._eptr is None:
            ip = self.graph.indptr
            e = torch.zeros(self.B + 1, dtype=torch.int64, device=ip.device)
            if self.B:
                torch.cumsum(ip[self.ids + 1] - ip[self.ids], 0, out=e[1:])
            self._eptr = (e, int(e[-1]))
        return self._eptr


def _batch_of(graph, rows):
    """(batch, inverse) for `rows` as gat_attend takes them (graph_conv.batch_rows): inverse is None for unique
    ids, else the batch holds torch.unique(rows) and rows = unique[inverse]."""
    from .graph_conv import batch_rows
    if isinstance(rows, _Batch):
        if rows.graph is not graph:
            raise ValueError("the batch was made for another graph")
        return rows, None
    ids, pos, unique = batch_rows(rows, graph.n, graph.device)
    if unique:
        return _Batch(graph, ids, pos), None
    uniq, inverse = torch.unique(ids, return_inverse=True)
    ids, pos, _ = batch_rows(uniq, graph.n, graph.device)
    return _Batch(graph, ids, pos), inverse


def _check(graph, Hf, a_src, a_dst, slope, rows=None):
    """(H, C) after gat_attend's argument checks; with rows, (H, C, batch, inverse): the ids are checked on
    whatever device the graph lives, before the device itself is."""
    if not isinstance(graph, GATGraph):
        raise TypeError("gat_attend takes a GATGraph")
    for name, t in (("Hf", Hf), ("a_src", a_src), ("a_dst", a_dst)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"gat_attend computes in fp32, {name} is {t.dtype}")
        if t.dim() != 2 or t.shape[0] != graph.n:
            raise ValueError(f"{name} must be [{graph.n}, .], got {tuple(t.shape)}")
    H = a_src.shape[1]
    if tuple(a_dst.shape) != tuple(a_src.shape):
        raise ValueError(f"a_src {tuple(a_src.shape)} and a_dst {tuple(a_dst.shape)} differ in shape")
    if H < 1 or H > _lib.SRG_GAT_MAX_HEADS:
        raise ValueError(f"H={H} heads, the fused layer takes 1 to {_lib.SRG_GAT_MAX_HEADS}")
    W = Hf.shape[1]
    if W < H or W % H:
        raise ValueError(f"Hf has {W} columns, not a positive multiple of H={H}")
    if W > _lib.SRG_GAT_MAX_WIDTH:
        raise ValueError(f"H*C={W} exceeds {_lib.SRG_GAT_MAX_WIDTH}")
    if not math.isfinite(float(slope)):
        raise ValueError(f"negative_slope={slope} is not finite")
    batch = _batch_of(graph, rows) if rows is not None else None
    if not graph.device.type == "cuda":
        raise RuntimeError("gat_attend runs on a HIP device: build the GATGraph there (device=) or move it with to()")
    for name, t in (("Hf", Hf), ("a_src", a_src), ("a_dst", a_dst)):
        if t.device != graph.device:
            raise ValueError(f"{name} is on {t.device}, the graph on {graph.device}")
    return (H, W // H) if batch is None else (H, W // H, *batch)


def _unique_batch(batch, inverse, who):
    if inverse is not None:
        raise ValueError(f"{who} takes unique row ids; gat_attend computes a repeated id once")
    return batch


def attend_forward(graph: GATGraph, Hf, a_src, a_dst, negative_slope: float = 0.2, rows=None):
    """(out [n, H*C], M [n, H], Z [n, H]) of srg_gat_attend_f32; no autograd.  With rows (unique ids, as
    gat_attend takes them): (out [B, H*C], M [B, H], Z [B, H]) of srg_gat_attend_rows_f32, row b for rows[b]."""
    if rows is not None:
        H, C, batch, inverse = _check(graph, Hf, a_src, a_dst, negative_slope, rows)
        return _attend_rows_forward(graph, Hf, a_src, a_dst, negative_slope, H, C,
                                    _unique_batch(batch, inverse, "attend_forward"))
    H, C = _check(graph, Hf, a_src, a_dst, negative_slope)
    dev, n = graph.device, graph.n
    Hf, ldh = _panel(Hf.detach(), "Hf", dev)
    a_src, a_dst = a_src.detach().contiguous(), a_dst.detach().contiguous()
    out = torch.empty((n, H * C), dtype=torch.float32, device=dev)
    M = torch.empty((n, H), dtype=torch.float32, device=dev)
    Z = torch.empty((n, H), dtype=torch.float32, device=dev)
    _lib.call(dev, "srg_gat_attend_f32", _ptr(graph.indptr), _ptr(graph.indices), graph.nnz, n, n, _ptr(a_src),
              _ptr(a_dst), float(negative_slope), _ptr(Hf), ldh, H, C, _ptr(out), H * C, _ptr(M), _ptr(Z),
              _lib.stream(dev))
    return out, M, Z


def _attend_rows_forward(graph, Hf, a_src, a_dst, slope, H, C, batch):
    dev, n, B = graph.device, graph.n, batch.B
    Hf, ldh = _panel(Hf.detach(), "Hf", dev)
    a_src, a_dst = a_src.detach().contiguous(), a_dst.detach().contiguous()
    out = torch.empty((B, H * C), dtype=torch.float32, device=dev)
    M = torch.empty((B, H), dtype=torch.float32, device=dev)
    Z = torch.empty((B, H), dtype=torch.float32, device=dev)
    _lib.call(dev, "srg_gat_attend_rows_f32", _ptr(graph.indptr), _ptr(graph.indices), graph.nnz, n, n,
              _ptr(batch.ids), B, _ptr(a_src), _ptr(a_dst), float(slope), _ptr(Hf), ldh, H, C, _ptr(out), H * C,
              _ptr(M), _ptr(Z), _lib.stream(dev))
    return out, M, Z


def _attend_rows_backward(graph, Hf, a_src, a_dst, out, M, Z, G, slope, need, H, C, batch):
    dev, n, nnz, W, B = graph.device, graph.n, graph.nnz, H * C, batch.B
    need_h, need_s, need_d = (bool(x) for x in need)
    Hf, ldh = _panel(Hf.detach(), "Hf", dev)
    G, ldg = _panel(G.detach(), "G", dev)
    out, ldo = _panel(out.detach(), "out", dev)
    if tuple(G.shape) != (B, W) or tuple(out.shape) != (B, W):
        raise ValueError(f"G and out must be [{B}, {W}], got {tuple(G.shape)} and {tuple(out.shape)}")
    a_src, a_dst, M, Z = (t.detach().contiguous() for t in (a_src, a_dst, M, Z))
    if tuple(M.shape) != (B, H) or tuple(Z.shape) != (B, H):
        raise ValueError(f"M and Z must be [{B}, {H}]")
    slope, s = float(slope), _lib.stream(dev)
    dS = da_dst = da_src = dHf = None
    eptr, nnzB = (None, 0)
    if need_s or need_d:
        eptr, nnzB = batch.eptr()
        D = torch.empty((B, H), dtype=torch.float32, device=dev)
        dS = torch.empty((nnzB, H), dtype=torch.float32, device=dev)
        compact = torch.empty((B, H), dtype=torch.float32, device=dev)
        _lib.call(dev, "srg_gat_edge_grad_rows_f32", _ptr(graph.indptr), _ptr(graph.indices), nnz, n, n,
                  _ptr(batch.ids), B, eptr.data_ptr(), nnzB, _ptr(a_src), _ptr(a_dst), slope, _ptr(Hf), ldh, H, C,
                  _ptr(out), ldo, _ptr(M), _ptr(Z), _ptr(G), ldg, _ptr(D), _ptr(dS), _ptr(compact), s)
        del D
        if need_d:   # the ids are unique: index_copy_ is deterministic
            da_dst = torch.zeros((n, H), dtype=torch.float32, device=dev).index_copy_(0, batch.ids, compact)
        del compact
    if need_h or need_s:
        if need_h:
            dHf = torch.empty((n, W), dtype=torch.float32, device=dev)
        if need_s:
            da_src = torch.empty((n, H), dtype=torch.float32, device=dev)
        _lib.call(dev, "srg_gat_attend_rows_adjoint_f32", _ptr(graph.indptr_t), _ptr(graph.indices_t),
                  _ptr(graph.perm), nnz, n, n, batch.pos.data_ptr() if n else None, B, graph.indptr.data_ptr(),
                  eptr.data_ptr() if need_s else None, nnzB, _ptr(a_src), _ptr(a_dst), slope, H, C, _ptr(M), _ptr(Z),
                  _ptr(G), ldg, _ptr(dS) if need_s else None, _ptr(dHf), W, _ptr(da_src), s)
    return dHf, da_src, da_dst


def attend_backward(graph: GATGraph, Hf, a_src, a_dst, out, M, Z, G, negative_slope: float = 0.2,
                    need=(True, True, True), rows=None):
    """(dHf, da_src, da_dst) from what attend_forward returned and G = dL/dout; an entry of `need` that is
    False gives None and skips the work only it needs (srg_gat_edge_grad_f32 when neither score gradient is
    asked for).  With rows (the ids attend_forward was given): out, M, Z and G are the batch's [B, .] panels;
    dHf and da_src are [n, .], and da_dst [n, H] holds the batch's rows and +0 elsewhere."""
    if rows is not None:
        H, C, batch, inverse = _check(graph, Hf, a_src, a_dst, negative_slope, rows)
        return _attend_rows_backward(graph, Hf, a_src, a_dst, out, M, Z, G, negative_slope, need, H, C,
                                     _unique_batch(batch, inverse, "attend_backward"))
    H, C = _check(graph, Hf, a_src, a_dst, negative_slope)
    dev, n, nnz, W = graph.device, graph.n, graph.nnz, H * C
    need_h, need_s, need_d = (bool(x) for x in need)
    Hf, ldh = _panel(Hf.detach(), "Hf", dev)
    G, ldg = _panel(G.detach(), "G", dev)
    out, ldo = _panel(out.detach(), "out", dev)
    if tuple(G.shape) != (n, W) or tuple(out.shape) != (n, W):
        raise ValueError(f"G and out must be [{n}, {W}], got {tuple(G.shape)} and {tuple(out.shape)}")
    a_src, a_dst, M, Z = (t.detach().contiguous() for t in (a_src, a_dst, M, Z))
    if tuple(M.shape) != (n, H) or tuple(Z.shape) != (n, H):
        raise ValueError(f"M and Z must be [{n}, {H}]")
    slope, s = float(negative_slope), _lib.stream(dev)
    dS = da_dst = da_src = dHf = None
    if need_s or need_d:
        D = torch.empty((n, H), dtype=torch.float32, device=dev)
        dS = torch.empty((nnz, H), dtype=torch.float32, device=dev)
        da_dst = torch.empty((n, H), dtype=torch.float32, device=dev)
        _lib.call(dev, "srg_gat_edge_grad_f32", _ptr(graph.indptr), _ptr(graph.indices), nnz, n, n, _ptr(a_src),
                  _ptr(a_dst), slope, _ptr(Hf), ldh, H, C, _ptr(out), ldo, _ptr(M), _ptr(Z), _ptr(G), ldg, _ptr(D),
                  _ptr(dS), _ptr(da_dst), s)
        del D
    if need_h or need_s:
        if need_h:
            dHf = torch.empty((n, W), dtype=torch.float32, device=dev)
        if need_s:
            da_src = torch.empty((n, H), dtype=torch.float32, device=dev)
        _lib.call(dev, "srg_gat_attend_adjoint_f32", _ptr(graph.indptr_t), _ptr(graph.indices_t), _ptr(graph.perm), nnz,
                  n, n, _ptr(a_src), _ptr(a_dst), slope, H, C, _ptr(M), _ptr(Z), _ptr(G), ldg,
                  _ptr(dS) if need_s else None, _ptr(dHf), W, _ptr(da_src), s)
    return dHf, da_src, (da_dst if need_d else None)


class _GatAttend(torch.autograd.Function):

    @staticmethod
    def forward(ctx, graph, Hf, a_src, a_dst, slope):
        out, M, Z = attend_forward(graph, Hf, a_src, a_dst, slope)
        ctx.graph, ctx.slope = graph, slope
        ctx.save_for_backward(Hf, a_src, a_dst, out, M, Z)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        Hf, a_src, a_dst, out, M, Z = ctx.saved_tensors
        dHf, da_src, da_dst = attend_backward(ctx.graph, Hf, a_src, a_dst, out, M, Z, grad, ctx.slope,
                                              need=ctx.needs_input_grad[1:4])
        return None, dHf, da_src, da_dst, None


class _GatAttendRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, graph, Hf, a_src, a_dst, slope, batch):
        H, C = a_src.shape[1], Hf.shape[1] // a_src.shape[1]
        out, M, Z = _attend_rows_forward(graph, Hf, a_src, a_dst, slope, H, C, batch)
        ctx.graph, ctx.slope, ctx.batch, ctx.hc = graph, slope, batch, (H, C)
        ctx.save_for_backward(Hf, a_src, a_dst, out, M, Z)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        Hf, a_src, a_dst, out, M, Z = ctx.saved_tensors
        dHf, da_src, da_dst = _attend_rows_backward(ctx.graph, Hf, a_src, a_dst, out, M, Z, grad, ctx.slope,
                                                    ctx.needs_input_grad[1:4], *ctx.hc, ctx.batch)
        return None, dHf, da_src, da_dst, None, None


def gat_attend(graph: GATGraph, Hf: torch.Tensor, a_src: torch.Tensor, a_dst: torch.Tensor,
               negative_slope: float = 0.2, rows=None) -> torch.Tensor:
    """out [n, H*C]: per target i and head h the softmax, over i's incoming edges, of
    leaky_relu(a_src[j,h] + a_dst[i,h]) applied to the rows Hf[j, h*C:(h+1)*C] of their sources.
    Hf: [n, H*C] fp32 (a column window of a wider panel passes as it is); a_src, a_dst: [n, H] fp32; all on
    the graph's device.  Differentiable (once) in Hf, a_src and a_dst; the backward runs only the entries
    the gradients autograd asks for need.  A node without incoming edges gets a row of +0 and contributes
    nothing to any gradient.  Deterministic: no atomics anywhere.

    rows (what graph_conv takes, through batch_rows: a tensor, a list or a range, on the host or the device;
    negative ids wrap; an id out of range raises IndexError before any launch): out [B, H*C] for those target
    rows only, the bits of gat_attend(...)[rows], and a backward that keeps nothing per edge outside the batch:
    dHf and da_src [n, .] and da_dst [n, H] (the batch's rows, +0 elsewhere) have, for finite operands, the
    bits of the full backward under a cotangent that is zero outside the batch.  A repeated id is computed once
    (torch.unique) and indexed with the inverse: that branch's backward sums the repeats' cotangents through
    torch's indexing backward and is only as deterministic as that is."""
    if rows is None:
        _check(graph, Hf, a_src, a_dst, negative_slope)
        return _GatAttend.apply(graph, Hf, a_src, a_dst, float(negative_slope))
    _, _, batch, inverse = _check(graph, Hf, a_src, a_dst, negative_slope, rows)
    out = _GatAttendRows.apply(graph, Hf, a_src, a_dst, float(negative_slope), batch)
    return out if inverse is None else out[inverse]


# ---- the layer and the model ------------------------------------------------------------------------
def _glorot(t: torch.Tensor) -> None:
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


class GATConv(nn.Module):
    """PyG's GATConv on a GATGraph: the same parameters under the same names and shapes (lin.weight
    [H*C, in], att_src and att_dst [1, H, C], bias [H*C] with concat, [C] without), Glorot for lin and both
    att, zeros for bias.  forward(x, graph): Hf = lin(x); the scores a_src = <Hf_h, att_src_h> and a_dst
    likewise stay dense torch ops; the aggregation is gat_attend; then the heads are concatenated or
    averaged and the bias added.  forward(x, graph, rows): lin and the scores run over all nodes, the
    aggregation, the head mean and the bias for the batch only (gat_attend's rows=); the result is [B, .].  Attention dropout needs the per-edge weights this layer never stores:
    dropout > 0 raises NotImplementedError in training mode."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True, bias: bool = True):
        super().__init__()
        if in_channels < 1 or out_channels < 1:
            raise ValueError(f"in_channels={in_channels} and out_channels={out_channels} must be positive")
        if heads < 1 or heads > _lib.SRG_GAT_MAX_HEADS:
            raise ValueError(f"heads={heads}, the fused layer takes 1 to {_lib.SRG_GAT_MAX_HEADS}")
        if heads * out_channels > _lib.SRG_GAT_MAX_WIDTH:
            raise ValueError(f"heads * out_channels = {heads * out_channels} exceeds {_lib.SRG_GAT_MAX_WIDTH}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout={dropout} must lie in [0, 1)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = bool(concat), float(negative_slope), float(dropout)
        self.add_self_loops = bool(add_self_loops)
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.lin.weight)
        _glorot(self.att_src)
        _glorot(self.att_dst)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _aggregate(self, graph, Hf, a_src, a_dst):
        return gat_attend(graph, Hf, a_src, a_dst, self.negative_slope)

    def _aggregate_rows(self, graph, Hf, a_src, a_dst, rows):
        return gat_attend(graph, Hf, a_src, a_dst, self.negative_slope, rows)

    def forward(self, x: torch.Tensor, graph: GATGraph, rows=None) -> torch.Tensor:
        if not isinstance(graph, GATGraph):
            raise TypeError("GATConv.forward takes a GATGraph (GATGraph.from_edge_index / from_scipy / from_torch_sparse)")
        if graph.has_self_loops != self.add_self_loops:
            raise ValueError(f"the layer has add_self_loops={self.add_self_loops}, the graph was built with "
                             f"add_self_loops={graph.has_self_loops}: build the GATGraph to match")
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError("attention dropout needs the per-edge weights, which the fused layer never "
                                      "stores: use dropout=0.0 (the reference's GAT does) or eval mode")
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"x must be [n, {self.in_channels}], got {tuple(x.shape)}")
        H, C = self.heads, self.out_channels
        Hf = self.lin(x)
        Hv = Hf.view(-1, H, C)
        a_src = torch.einsum("nhc,hc->nh", Hv, self.att_src[0])
        a_dst = torch.einsum("nhc,hc->nh", Hv, self.att_dst[0])
        if rows is None:
            out = self._aggregate(graph, Hf, a_src, a_dst)
        else:
            out = self._aggregate_rows(graph, Hf, a_src, a_dst, rows)
        if not self.concat:
            out = out.view(-1, H, C).mean(dim=1)
        if self.bias is not None:
            out = out + self.bias
        return out

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}, concat={self.concat}"


class GAT(nn.Module):
    """The reference runner's GAT baseline on GATGraphs: num_layers GATConv layers, the inner ones with
    num_heads concatenated heads of hidden_channels each followed by ReLU and feature dropout, the last one
    a single head of out_channels; forward(x, graph) returns log-probabilities, forward(x, graph, rows) those
    of a batch of rows [B, out] with the last layer restricted to it (the runner's model(x, adj)[train_idx])."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int, dropout: float,
                 num_heads: int):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"num_layers={num_layers}: the model has a first and a last layer at least")
        widths = [in_channels] + [hidden_channels * num_heads] * (num_layers - 1)
        self.convs = nn.ModuleList(GATConv(w, hidden_channels, num_heads) for w in widths[:-1])
        self.convs.append(GATConv(widths[-1], out_channels, 1))
        self.dropout = float(dropout)

    def reset_parameters(self) -> None:
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x: torch.Tensor, graph: GATGraph, rows=None) -> torch.Tensor:
        for conv in list(self.convs)[:-1]:
            x = nn.functional.dropout(torch.relu(conv(x, graph)), p=self.dropout, training=self.training)
        last = self.convs[-1](x, graph) if rows is None else self.convs[-1](x, graph, rows)
        return last.log_softmax(dim=-1)
