"""Graph convolution on the device: the exact hop made differentiable, for GCN training.

The reference's GCN (SSRG/models/gcn.py, Layer2GraphConvolution in models/base_scalable/simple_models.py)
keeps construct_adj's operator as a torch sparse COO tensor and calls torch.mm(adj, x) twice per forward;
autograd then runs two transposed sparse products per backward.  This module keeps the operator and its
transpose as DeviceCSRs and runs all four products through this library:

  Y  = A X      srgnn.spmm.hop(A, X)     one fma chain per element from +0 in the row's stored order
  dX = A^T G    srgnn.spmm.hop(At, G)    the same chain over the transpose's rows

and, for the last layer, whose output the loss reads at a batch of rows only,

  Y  = A[rows, :] X      srg_gconv_rows_f32          the hop's bits for those rows
  dX = A[rows, :]^T G    srg_gconv_rows_adjoint_f32  the chain over the transpose's member entries

GraphConvOperator answers torch.mm(op, X) and torch.sparse.mm(op, X), so the reference's own layer runs
with model.base_model.adj = GraphConvOperator.from_torch_sparse(model.base_model.adj) and nothing else
changed; GraphConvolution2 is the same layer with the row-restricted last product.  There is no torch
fallback: every product is a kernel of libsrgnn_hip.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, spmm
from .csr import DeviceCSR
from .sparse import _panel, csr_transpose

__all__ = ["GraphConvOperator", "graph_conv", "GraphConvolution2", "rows_product", "rows_adjoint", "batch_rows"]


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _transpose_of(A: DeviceCSR):
    """(At, kind) for A: the mirror's shortcut for a symmetric structure with sorted unique rows, else
    csr_transpose's stable sort by column.  The mirrored values in sorted rows are that sort's order."""
    from .construct import mirror_device
    ip, ix, v = A.indptr, A.indices, A.values
    n, nnz = A.n_rows, ix.numel()
    if n == A.n_cols:
        rows = torch.repeat_interleave(torch.arange(n, device=ip.device), ip[1:] - ip[:-1], output_size=nnz)
        key = rows * n + ix
        if nnz == 0 or bool((key[1:] > key[:-1]).all()):
            mirror = mirror_device(ip, ix, rows) if nnz else torch.zeros(0, dtype=torch.int64, device=ip.device)
            if nnz == 0 or bool((mirror >= 0).all()):
                vt = v[mirror]
                if torch.equal(vt.view(torch.int32), v.view(torch.int32)):
                    return A, "same"
                At = DeviceCSR(ip, ix, vt.contiguous(), n, n, A._order, A._n_heavy, A._n_hub, A._n_heavy_narrow,
                               thresholds=A.thresholds)
                return At, "mirrored"
    t_ip, t_ix, t_v, _ = csr_transpose(ip, ix, v, A.n_cols)
    At = DeviceCSR.from_tensors(t_ip, t_ix, t_v, n_cols=n, validate=False, device=A.device,
                                heavy_threshold=A.thresholds[0], hub_threshold=A.thresholds[1])
    return At, "sorted"


class GraphConvOperator:
    """Â and its transpose on one device, chosen once at construction:

      transpose_kind "same"      every row holds strictly increasing column ids, the structure is symmetric
                                 (srg_csr_mirror finds every entry) and values[mirror] equals values bit for
                                 bit: At is A, one operator and one plan (Â at r = 0.5 on an unweighted graph);
                     "mirrored"  the same structure with other values: At shares indptr and indices with A
                                 and owns values[mirror];
                     "sorted"    anything else (asymmetric, unsorted rows, duplicates):
                                 srgnn.sparse.csr_transpose, a stable sort by column.

    It is not a Tensor; it answers torch.mm(op, X), torch.sparse.mm(op, X) and op @ X with graph_conv, and
    has the few attributes the reference's model touches (to, shape, device).  It defines no __eq__: the
    reference tests `adj != None`."""

    def __init__(self, A: DeviceCSR):
        if not isinstance(A, DeviceCSR):
            raise TypeError("GraphConvOperator takes a DeviceCSR (see from_scipy / from_torch_sparse)")
        if A.is_span or A.schedules_subset:
            raise ValueError("GraphConvOperator takes a whole operator, not a column block or row group")
        self.A = A
        self.At, self.transpose_kind = _transpose_of(A)

    # -- constructors ---------------------------------------------------------------------------------
    @classmethod
    def from_device_csr(cls, A: DeviceCSR) -> "GraphConvOperator":
        return cls(A)

    @classmethod
    def from_scipy(cls, csr, device=None) -> "GraphConvOperator":
        """From a scipy sparse matrix (construct_adj's result); values are cast to fp32 as the reference's
        scipy_sparse_mat_to_torch_sparse_tensor casts them."""
        import scipy.sparse as sp
        if not sp.issparse(csr):
            raise TypeError(f"from_scipy takes a scipy sparse matrix, got {type(csr).__name__}")
        return cls(DeviceCSR.from_scipy(csr.tocsr(), device=device))

    @classmethod
    def from_torch_sparse(cls, t, device=None) -> "GraphConvOperator":
        """From a torch sparse COO tensor (what scipy_sparse_mat_to_torch_sparse_tensor returns), coalesced:
        entries sorted by (row, column), duplicates summed by torch."""
        if not isinstance(t, torch.Tensor) or t.layout != torch.sparse_coo:
            raise TypeError("from_torch_sparse takes a torch sparse COO tensor")
        if t.dim() != 2 or t.dense_dim() != 0:
            raise ValueError(f"from_torch_sparse takes a 2-D sparse matrix, got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"graph_conv computes in fp32, the operator is {t.dtype}")
        t = t.detach().coalesce()
        idx, val = t.indices(), t.values()
        m, n = t.shape
        counts = torch.bincount(idx[0], minlength=m) if idx.shape[1] else torch.zeros(m, dtype=torch.int64)
        ip = torch.zeros(m + 1, dtype=torch.int64, device=idx.device)
        torch.cumsum(counts, 0, out=ip[1:])
        if device is None and t.is_cuda:
            device = t.device
        return cls(DeviceCSR.from_tensors(ip, idx[1], val, n_cols=n, device=device))

    # -- the tensor-like protocol ---------------------------------------------------------------------
    @property
    def shape(self):
        return torch.Size((self.A.n_rows, self.A.n_cols))

    @property
    def device(self):
        return self.A.device

    def to(self, device=None, *args, **kwargs):
        """self on the device it lives on; an operator is not copied between devices."""
        if device is None or isinstance(device, torch.dtype):
            raise TypeError("GraphConvOperator.to takes a device")
        dev = torch.device(device)
        if dev.type == self.device.type and (dev.index is None or dev.index == self.device.index):
            return self
        raise RuntimeError(f"this GraphConvOperator lives on {self.device}; build another one for {dev}")

    def prepare(self, d: int, steps: int):
        """Lays both operators out for `steps` products over d-column panels (srgnn.spmm.prepare)."""
        a = spmm.prepare(self.A, d, steps)
        t = a if self.At is self.A else spmm.prepare(self.At, d, steps)
        return a, t

    def __matmul__(self, X):
        return graph_conv(self, X)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if func in (torch.mm, torch.sparse.mm) and not kwargs and len(args) == 2 and isinstance(args[0], cls) \
                and isinstance(args[1], torch.Tensor):
            return graph_conv(args[0], args[1])
        return NotImplemented

    def __repr__(self):
        return (f"GraphConvOperator({self.A.n_rows}x{self.A.n_cols}, nnz={self.A.indices.numel()}, "
                f"transpose={self.transpose_kind}, device={self.device})")


# ---- the two row-restricted entries -----------------------------------------------------------------
def rows_product(A: DeviceCSR, X: torch.Tensor, rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Y[b] = A[rows[b], :] X (srg_gconv_rows_f32): the hop's bits for those rows.  rows: int64 on A's
    device; an id outside [0, n_rows) gives a row of +0.  X may be a column window (row stride > d)."""
    dev = A.device
    X, ldx = _panel(X, "X", dev)
    if X.shape[0] < A.n_cols:
        raise ValueError(f"X has {X.shape[0]} rows, the operator {A.n_cols} columns")
    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.device != dev:
        raise ValueError(f"rows must be a 1-D int64 tensor on {dev}")
    rows = rows.contiguous()
    B, d = rows.numel(), X.shape[1]
    if out is None:
        out = torch.empty((B, d), dtype=torch.float32, device=dev)
    else:
        out, _ = _panel(out, "out", dev)
        if tuple(out.shape) != (B, d):
            raise ValueError(f"out must be [{B}, {d}], got {tuple(out.shape)}")
    ldy = out.stride(0) if B > 1 else d
    _lib.call(dev, "srg_gconv_rows_f32", A.indptr.data_ptr(), _ptr(A.indices), _ptr(A.values), A.n_rows, _ptr(rows),
              B, _ptr(X), ldx, _ptr(out), ldy, d, _lib.stream(dev))
    return out


def rows_adjoint(At: DeviceCSR, pos: torch.Tensor, G: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """dX = A[rows, :]^T G over the rows of the transposed operator At (srg_gconv_rows_adjoint_f32).
    pos: int32 [At.n_cols] on the device, pos[r] = b where rows[b] = r, else -1.  Entries outside the batch
    are skipped; all At.n_rows rows are written."""
    dev = At.device
    G, ldg = _panel(G, "G", dev)
    if pos.dtype != torch.int32 or pos.dim() != 1 or pos.device != dev or pos.numel() != At.n_cols:
        raise ValueError(f"pos must be an int32 [{At.n_cols}] tensor on {dev}")
    if At.n_rows != At.n_cols:
        raise ValueError("the row-restricted adjoint takes a square operator")
    pos = pos.contiguous()
    B, d, n = G.shape[0], G.shape[1], At.n_rows
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
    else:
        out, _ = _panel(out, "out", dev)
        if tuple(out.shape) != (n, d):
            raise ValueError(f"out must be [{n}, {d}], got {tuple(out.shape)}")
    ldx = out.stride(0) if n > 1 else d
    _lib.call(dev, "srg_gconv_rows_adjoint_f32", At.indptr.data_ptr(), _ptr(At.indices), _ptr(At.values), n, _ptr(pos),
              B, _ptr(G), ldg, _ptr(out), ldx, d, _lib.stream(dev))
    return out


def batch_rows(rows, n: int, device=None):
    """(ids, pos, unique) for a batch of row ids of an n-row operator.  rows: anything torch.as_tensor takes
    (a range included), on any device; negative ids wrap as torch indexing does; ids still outside [0, n)
    raise IndexError.  ids: int64 [B] on `device`; pos: int32 [n], pos[ids[b]] = b and -1 elsewhere;
    unique: False when an id repeats -- found without a sort: arange(B) scattered into pos and gathered
    back differs from arange(B) exactly then (pos is then not a map of the batch)."""
    if isinstance(rows, range):
        r = torch.arange(rows.start, rows.stop, rows.step, dtype=torch.int64)
    else:
        r = torch.as_tensor(rows)
    if r.numel() == 0 and r.dim() == 1:
        r = r.to(torch.int64)          # an empty list has no dtype of its own
    if r.dtype in (torch.bool,) or r.is_floating_point() or r.is_complex():
        raise TypeError(f"rows must hold integer ids, got {r.dtype}")
    if r.dim() != 1:
        raise ValueError(f"rows must be 1-D, got shape {tuple(r.shape)}")
    r = r.to(device=device if device is not None else r.device, dtype=torch.int64)
    r = torch.where(r < 0, r + n, r)
    B = r.numel()
    if B and (int(r.min()) < 0 or int(r.max()) >= n):
        raise IndexError(f"a row id is out of range for an operator of {n} rows")
    ar = torch.arange(B, dtype=torch.int32, device=r.device)
    pos = torch.full((n,), -1, dtype=torch.int32, device=r.device)
    pos[r] = ar
    unique = not bool((pos[r] != ar).any()) if B else True
    return r.contiguous(), pos, unique


# ---- autograd ---------------------------------------------------------------------------------------
def _hop(A: DeviceCSR, X: torch.Tensor) -> torch.Tensor:
    X, _ = _panel(X, "X", A.device)
    out = torch.empty((A.n_rows, X.shape[1]), dtype=torch.float32, device=A.device)
    if A.n_rows == 0 or X.shape[1] == 0:
        return out
    if A.indices.numel() == 0:
        return out.zero_()
    return spmm.hop(A, X, out)


class _GraphConv(torch.autograd.Function):

    @staticmethod
    def forward(ctx, op, X):
        ctx.op = op
        return _hop(op.A, X.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return None, _hop(ctx.op.At, grad)


class _GraphConvRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, op, X, ids, pos):
        ctx.op = op
        ctx.save_for_backward(pos)
        return rows_product(op.A, X.detach(), ids)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (pos,) = ctx.saved_tensors
        return None, rows_adjoint(ctx.op.At, pos, grad), None, None


def graph_conv(op: GraphConvOperator, X: torch.Tensor, rows=None) -> torch.Tensor:
    """Â X ([n, d] fp32), or with `rows` Â[rows, :] X ([B, d]); differentiable (once) in X only.

    rows None: Y = spmm.hop(A, X) and dX = spmm.hop(At, G), the planned exact hop both ways.
    rows given (batch_rows: a tensor, a list, a range; host or device; negative ids wrap; out of range
    raises IndexError before any launch): srg_gconv_rows_f32 and srg_gconv_rows_adjoint_f32.  Both are bit for
    bit run-to-run identical and equal to the full path's rows, forward and backward (a chain that skips
    the entries outside the batch equals one that adds v * (+0) for them, on finite operators).
    With a repeated id the product is computed for torch.unique(rows) and indexed with the inverse: that
    branch's backward goes through torch's indexing backward and is only as deterministic as that is.
    An X on another device is moved to the operator's and the result moved back."""
    if not isinstance(op, GraphConvOperator):
        raise TypeError("graph_conv takes a GraphConvOperator")
    if not isinstance(X, torch.Tensor):
        raise TypeError("X must be a tensor")
    if X.dtype != torch.float32:
        raise TypeError(f"graph_conv computes in fp32, X is {X.dtype}")
    if X.dim() != 2 or X.shape[0] != op.A.n_cols:
        raise ValueError(f"X must be [{op.A.n_cols}, d], got {tuple(X.shape)}")
    home = X.device
    x = X.to(op.device) if X.device != op.device else X
    if rows is None:
        return _GraphConv.apply(op, x).to(home)
    if op.A.n_rows != op.A.n_cols:
        raise ValueError("rows takes a square operator")
    ids, pos, unique = batch_rows(rows, op.A.n_rows, op.device)
    if unique:
        return _GraphConvRows.apply(op, x, ids, pos).to(home)
    uniq, inverse = torch.unique(ids, return_inverse=True)
    _, pos_u, _ = batch_rows(uniq, op.A.n_rows, op.device)
    return _GraphConvRows.apply(op, x, uniq, pos_u)[inverse].to(home)


# ---- the two-layer GCN head -------------------------------------------------------------------------
class GraphConvolution2(nn.Module):
    """The reference's two-layer graph convolution with the last product restricted to a batch.

    Same parameters under the same names as Layer2GraphConvolution (fc1_node_edge, fc2_node, fc2_edge,
    linear), so state dicts interchange; `adj` is a GraphConvOperator and `query_edges` selects the edge head.  forward(feature, rows): with query_edges None and
    rows given, the second product runs for those rows only and the result is what the reference's
    forward(feature)[rows] returns, bit for bit on the forward.  With query_edges set the edge head computes all
    rows and concatenates, as the reference does, unless fused_edge_head is set (False by default): then the second
    product runs for the batch's distinct endpoints only (rows=batch.n_id) and the head is srgnn.link.pair_linear,
    with no [E, 2h] buffer; query_edges may then be an srgnn.link.EdgeBatch, so that a static split builds its
    relabelling and incidence once."""

    def __init__(self, feat_dim, hidden_dim, output_dim, dropout=0.5):
        super().__init__()
        self.adj = None
        self.query_edges = None
        self.fused_edge_head = False
        self.fc1_node_edge = nn.Linear(feat_dim, hidden_dim)
        self.fc2_node = nn.Linear(hidden_dim, output_dim)
        self.fc2_edge = nn.Linear(hidden_dim, hidden_dim)
        self.linear = nn.Linear(2 * hidden_dim, output_dim)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(dropout)

    def _conv(self, x, rows=None):
        return graph_conv(self.adj, x, rows)

    def forward(self, feature, rows=None):
        if not isinstance(self.adj, GraphConvOperator):
            raise TypeError("GraphConvolution2.adj must be a GraphConvOperator (GraphConvOperator.from_torch_sparse "
                            "turns the reference's sparse tensor into one)")
        h = self.dropout(self.relu(self._conv(self.fc1_node_edge(feature))))
        if self.query_edges is None:
            return self._conv(self.fc2_node(h), rows)
        from .link import EdgeBatch, pair_linear
        q = self.query_edges
        if self.fused_edge_head:
            batch = q if isinstance(q, EdgeBatch) else EdgeBatch(q, self.adj.A.n_rows, self.adj.device)
            z = self._conv(self.fc2_edge(h), batch.n_id)
            return pair_linear(z, batch, self.linear.weight, self.linear.bias)
        if isinstance(q, EdgeBatch):
            q = q.edges
        z = self._conv(self.fc2_edge(h))
        return self.linear(torch.cat((z[q[:, 0]], z[q[:, 1]]), dim=-1))
