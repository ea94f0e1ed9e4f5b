"""GraphSAGE's mean layer on the device: the runner's SAGE baseline, full graph and on
neighbour-sampled blocks (srgnn.neighbor).

  mean_operator(csr)           the structure with values 1.0 as a GraphConvOperator, plus cnt = max(len, 1)
  sage_mean(op, x_src, rows)   mean of the sources' rows per target: the exact hop's chain fma(1, x, acc) from
                               +0 in stored order, then one correctly rounded division by cnt
                               (srg_row_divide_f32); backward A^T (G / cnt) through the operator's transpose
  SAGEConv(in, out)            PyG's layer: lin_l (with bias) on the mean, lin_r (without) on the root rows
  SAGE(in, hidden, out, L, p)  the runner's model, on one operator or on a NeighborBatch's blocks

No kernel of its own: every product is the hop of srgnn.graph_conv, rectangular for a block, row-restricted
(§5.10) with rows=.  An empty row's mean is +0.  There is no torch fallback.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .csr import DeviceCSR
from .graph_conv import GraphConvOperator, _hop, batch_rows, rows_adjoint, rows_product

__all__ = ["MeanOperator", "mean_operator", "sage_mean", "SAGEConv", "SAGE"]


class MeanOperator(GraphConvOperator):
    """A GraphConvOperator over a structure with every value 1.0, and cnt: fp32 [n_rows], max(row length, 1)."""

    def __init__(self, csr: DeviceCSR):
        if not isinstance(csr, DeviceCSR):
            raise TypeError("mean_operator takes a DeviceCSR")
        if csr.is_span or csr.schedules_subset:
            raise ValueError("mean_operator takes a whole operator, not a column block or row group")
        ones = torch.ones(csr.indices.numel(), dtype=torch.float32, device=csr.indptr.device)
        super().__init__(DeviceCSR(csr.indptr, csr.indices, ones, csr.n_rows, csr.n_cols, None, None, None, None,
                                   thresholds=csr.thresholds))
        self.cnt = (csr.indptr[1:] - csr.indptr[:-1]).clamp(min=1).to(torch.float32)


def mean_operator(csr: DeviceCSR) -> MeanOperator:
    """The mean aggregation over csr's structure (its values are ignored; indptr and indices are shared)."""
    return MeanOperator(csr)


def _divide(Y: torch.Tensor, cnt: torch.Tensor) -> torch.Tensor:
    """Y[r, :] /= cnt[r] in place (srg_row_divide_f32); Y contiguous fp32."""
    if Y.shape[0] and Y.shape[1]:
        _lib.call(Y.device, "srg_row_divide_f32", Y.data_ptr(), Y.stride(0), cnt.data_ptr(), Y.shape[0], Y.shape[1],
                  _lib.stream(Y.device))
    return Y


class _SageMean(torch.autograd.Function):

    @staticmethod
    def forward(ctx, op, X):
        ctx.op = op
        return _divide(_hop(op.A, X.detach()), op.cnt)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return None, _hop(ctx.op.At, _divide(grad.contiguous().clone(), ctx.op.cnt))


class _SageMeanRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, op, X, ids, pos):
        ctx.op = op
        cnt = op.cnt[ids]
        ctx.save_for_backward(pos, cnt)
        return _divide(rows_product(op.A, X.detach(), ids), cnt)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pos, cnt = ctx.saved_tensors
        return None, rows_adjoint(ctx.op.At, pos, _divide(grad.contiguous().clone(), cnt)), None, None


def sage_mean(op: MeanOperator, x_src: torch.Tensor, rows=None) -> torch.Tensor:
    """mean_{j in row i} x_src[j] for every row of op ([n_rows, d] fp32), or with `rows` (a square operator;
    graph_conv.batch_rows' ids, distinct) for those rows only ([B, d]); differentiable (once) in x_src.
    Forward: the hop's chain over the row's entries in stored order, then acc / cnt correctly rounded; a row
    without entries gives +0.  Backward: A^T (G / cnt), the same two steps over the transpose."""
    if not isinstance(op, MeanOperator):
        raise TypeError("sage_mean takes a mean_operator")
    if not isinstance(x_src, torch.Tensor):
        raise TypeError("x_src must be a tensor")
    if x_src.dtype != torch.float32:
        raise TypeError(f"sage_mean computes in fp32, x_src is {x_src.dtype}")
    if x_src.dim() != 2 or x_src.shape[0] != op.A.n_cols:
        raise ValueError(f"x_src must be [{op.A.n_cols}, d], got {tuple(x_src.shape)}")
    if x_src.device != op.device:
        raise ValueError(f"x_src is on {x_src.device}, the operator on {op.device}")
    if rows is None:
        return _SageMean.apply(op, x_src)
    if op.A.n_rows != op.A.n_cols:
        raise ValueError("rows takes a square operator")
    ids, pos, unique = batch_rows(rows, op.A.n_rows, op.device)
    if not unique:
        raise ValueError("rows repeats an id")
    return _SageMeanRows.apply(op, x_src, ids, pos)


class SAGEConv(nn.Module):
    """PyG's SAGEConv with mean aggregation under its parameter names: out = lin_l(mean of the sources) +
    lin_r(the target's own row); lin_l has the bias, lin_r none; both are torch.nn.Linear with its initialisation.
    forward(x, op, rows=None): x is [n_cols, in] (the targets are then the operator's first n_rows rows, as in a
    SampledBlock, or all of them on a square operator) or a pair (x_src, x_dst); rows restricts a square
    operator's output to a batch of rows."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.lin_l = nn.Linear(self.in_channels, self.out_channels, bias=True)
        self.lin_r = nn.Linear(self.in_channels, self.out_channels, bias=False)

    def reset_parameters(self) -> None:
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x, op: MeanOperator, rows=None) -> torch.Tensor:
        if isinstance(x, (tuple, list)):
            x_src, x_dst = x
        else:
            x_src, x_dst = x, x[:op.A.n_rows]
        if x_dst.shape[0] != op.A.n_rows:
            raise ValueError(f"x_dst has {x_dst.shape[0]} rows, the operator {op.A.n_rows}")
        if rows is not None:
            ids, _, _ = batch_rows(rows, op.A.n_rows, op.device)
            x_dst = x_dst[ids]
            rows = ids
        return self.lin_l(sage_mean(op, x_src, rows)) + self.lin_r(x_dst)

    def __repr__(self):
        return f"SAGEConv({self.in_channels}, {self.out_channels})"


class SAGE(nn.Module):
    """The reference runner's SAGE baseline: num_layers SAGEConv layers, the inner ones followed by ReLU and
    feature dropout; returns log-probabilities.
    forward(x, op, rows=None): full graph on one square MeanOperator, every layer on it, the last restricted to
    `rows` when given ([B, out], the runner's model(x, adj)[train_idx]).
    forward(x, blocks): sampled, on a NeighborBatch's blocks (one per layer, outermost first) with
    x = gather_rows(X, batch.n_id); layer i runs on blocks[i].mean_operator() with x_dst = x[:n_dst] and the
    result is [batch_size, out]."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, num_layers: int, dropout: float):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"num_layers={num_layers}: the model has a first and a last layer at least")
        widths = [in_channels] + [hidden_channels] * (num_layers - 1)
        self.convs = nn.ModuleList(SAGEConv(w, hidden_channels) for w in widths[:-1])
        self.convs.append(SAGEConv(widths[-1], out_channels))
        self.dropout = float(dropout)

    def reset_parameters(self) -> None:
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x: torch.Tensor, op, rows=None) -> torch.Tensor:
        if isinstance(op, (list, tuple)):
            if rows is not None:
                raise ValueError("rows goes with one operator: a batch's blocks end at its seed nodes")
            if len(op) != len(self.convs):
                raise ValueError(f"{len(op)} blocks for {len(self.convs)} layers")
            ops = [b.mean_operator() if hasattr(b, "mean_operator") else b for b in op]
        else:
            ops = [op] * len(self.convs)
        for i, (conv, o) in enumerate(zip(self.convs, ops)):
            last = i == len(self.convs) - 1
            x = conv((x, x[:o.A.n_rows]), o, rows if last else None)
            if not last:
                x = nn.functional.dropout(torch.relu(x), p=self.dropout, training=self.training)
        return x.log_softmax(dim=-1)
