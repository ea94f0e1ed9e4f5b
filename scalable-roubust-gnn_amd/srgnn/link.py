"""Link classification on the device: the fused edge-pair head and its batches.

Every base model of the reference (LogisticRegression, MultiLayerPerceptron, ResMultiLayerPerceptron,
Layer2GraphConvolution in SSRG/models/base_scalable/simple_models.py) ends its link-classification forward with

    x = cat(f[query_edges[:, 0]], f[query_edges[:, 1]], dim=-1)   # [E, 2h]
    out = linear(x)                                               # [E, C]

and the reference's mini-batch step (link_cls_mini_batch_train, SSRG/tasks/utils.py) relabels each batch of
pairs over its distinct endpoints with a host dict.  This module is that head and that relabelling without the
[E, 2h] buffer and without the host loop.  With W = linear.weight = [W0 | W1] and z the rows of the U distinct
endpoint nodes:

    P = z [W0; W1]^T                                        [U, 2C], torch's GEMM at node count
    out[e, c] = (P[q0[e], c] + P[q1[e], C + c]) + b[c]      srg_pair_gather_add_f32
    S[v, side C + c] = sum of g[e, c] over v's slots        srg_pair_segment_sum_f32, one chain per element
    dz = S0 W0 + S1 W1,  dW = [S0^T z | S1^T z],  db = g.sum(0)

  EdgeBatch(query_edges, n)          the distinct endpoints n_id, the pairs relabelled over them (local) and,
                                     on first use, the incidence of the backward pass
  pair_linear(z, q, weight, bias)    the head, differentiable once in z, weight and bias
  edge_head(linear, feature, q)      the head of the three MLP-style models, dropout on the concatenation included
  EdgeBatchLoader(...)               the reference's DataLoader(range(E)) plus the relabelling of each batch

On a HIP device the two passes over the pairs are kernels of libsrgnn_hip and there is no torch fallback; on
the CPU the same association runs in torch ops, in any float dtype, so that the wiring can be checked without
a device (gradcheck in fp64 included).
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .sparse import _panel

__all__ = ["EdgeBatch", "pair_linear", "edge_head", "EdgeBatchLoader", "pair_gather_add", "pair_segment_sum"]


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _ld(t, d):
    return t.stride(0) if t.shape[0] > 1 else d


# ---- the batch --------------------------------------------------------------------------------------
class EdgeBatch:
    """A set of query pairs over an n-node graph, relabelled over its distinct endpoints.

    edges   int64 [E, 2]: the pairs as given (negative ids wrapped), on `device`
    n_id    int64 [U]: the distinct endpoint nodes, ascending: torch.unique(edges.reshape(-1)), the reference's
            train_idx
    local   int64 [E, 2]: the pairs as positions in n_id, what the reference's node_idx_map_dict relabelling
            returns
    inc_ptr, inc_slot   the incidence of the pairs on n_id, built on first use and kept: slot 2 e + side is
            endpoint `side` of pair e; inc_slot[inc_ptr[v] : inc_ptr[v + 1]] are the slots of node n_id[v],
            ascending (a stable sort of the 2E positions, a count and a cumsum)

    Built with device ops and no host loop: a mark over n, its nonzero and a position table (as SampledBlock
    builds its frontier).  Ids follow graph_conv.batch_rows: anything torch.as_tensor takes; negative ids wrap;
    an id still outside [0, n) raises IndexError; bool or float ids raise TypeError; a shape other than [E, 2]
    raises ValueError; all before any work.  E = 0 is valid."""

    def __init__(self, query_edges, n: int, device=None):
        q = torch.as_tensor(query_edges)
        if q.numel() == 0 and q.dim() == 1:
            q = q.to(torch.int64).reshape(0, 2)      # an empty list has neither a dtype nor a shape of its own
        if q.dtype == torch.bool or q.is_floating_point() or q.is_complex():
            raise TypeError(f"query_edges must hold integer ids, got {q.dtype}")
        if q.dim() != 2 or q.shape[1] != 2:
            raise ValueError(f"query_edges must be [E, 2], got shape {tuple(q.shape)}")
        n = int(n)
        if n < 0:
            raise ValueError(f"n={n} < 0")
        q = q.to(device=device if device is not None else q.device, dtype=torch.int64)
        q = torch.where(q < 0, q + n, q)
        if q.numel() and (int(q.min()) < 0 or int(q.max()) >= n):
            raise IndexError(f"an endpoint id is out of range for a graph of {n} nodes")
        dev = q.device
        self.n = n
        self.edges = q.contiguous()
        flat = self.edges.reshape(-1)
        mark = torch.zeros(n, dtype=torch.bool, device=dev)
        mark[flat] = True
        self.n_id = mark.nonzero().reshape(-1)                      # ascending
        pos = torch.empty(n, dtype=torch.int64, device=dev)         # read at marked ids only
        pos[self.n_id] = torch.arange(self.n_id.numel(), dtype=torch.int64, device=dev)
        self.local = pos[flat].reshape(-1, 2)
        self._inc = None

    @property
    def device(self):
        return self.edges.device

    @property
    def num_edges(self) -> int:
        return self.edges.shape[0]

    @property
    def num_nodes(self) -> int:
        return self.n_id.numel()

    def incidence(self):
        """(inc_ptr int64 [U + 1], inc_slot int64 [2E]), built once."""
        if self._inc is None:
            flat = self.local.reshape(-1)                           # position of slot 2 e + side
            U = self.num_nodes
            inc_slot = torch.sort(flat, stable=True).indices if flat.numel() else flat.clone()
            inc_ptr = torch.zeros(U + 1, dtype=torch.int64, device=flat.device)
            if flat.numel():
                torch.cumsum(torch.bincount(flat, minlength=U), 0, out=inc_ptr[1:])
            self._inc = (inc_ptr, inc_slot.contiguous())
        return self._inc

    @property
    def inc_ptr(self):
        return self.incidence()[0]

    @property
    def inc_slot(self):
        return self.incidence()[1]

    def __repr__(self):
        return f"EdgeBatch(E={self.num_edges}, U={self.num_nodes}, n={self.n}, device={self.device})"


# ---- the two entries --------------------------------------------------------------------------------
def _on_device(t: torch.Tensor) -> bool:
    return t.is_cuda


def _ids(q, name, dev):
    if not isinstance(q, torch.Tensor) or q.dtype != torch.int64 or q.device != dev:
        raise ValueError(f"{name} must be an int64 tensor on {dev}")
    return q.contiguous()


def pair_gather_add(P: torch.Tensor, q: torch.Tensor, bias: torch.Tensor | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """out[e, c] = (P[q[e, 0], c] + P[q[e, 1], C + c]) + bias[c], P [U, 2C], q int64 [E, 2] of positions in
    [0, U) (a position outside reads as a row of +0).  On a HIP device: srg_pair_gather_add_f32, fp32, P and out
    may be column windows of wider panels.  On the CPU: the same association in torch ops, any float dtype,
    positions in range."""
    if P.dim() != 2 or P.shape[1] % 2:
        raise ValueError(f"P must be [U, 2C], got {tuple(P.shape)}")
    U, C = P.shape[0], P.shape[1] // 2
    q = _ids(q, "q", P.device)
    if q.dim() != 2 or q.shape[1] != 2:
        raise ValueError(f"q must be [E, 2], got {tuple(q.shape)}")
    E = q.shape[0]
    if bias is not None and (bias.shape != (C,) or bias.dtype != P.dtype or bias.device != P.device):
        raise ValueError(f"bias must be a [{C}] {P.dtype} tensor on {P.device}")
    if not _on_device(P):
        r = P[q[:, 0], :C] + P[q[:, 1], C:]
        if bias is not None:
            r = r + bias
        if out is not None:
            out.copy_(r)
            return out
        return r
    dev = P.device
    P, ldp = _panel(P, "P", dev)
    if out is None:
        out = torch.empty((E, C), dtype=torch.float32, device=dev)
    else:
        if tuple(out.shape) != (E, C) or out.dtype != torch.float32 or out.device != dev or (C > 1 and out.stride(1) != 1) \
                or (E > 1 and out.stride(0) < C):
            raise ValueError(f"out must be a float32 [{E}, {C}] panel with unit column stride on {dev}")
    b = bias.contiguous() if bias is not None else None
    _lib.call(dev, "srg_pair_gather_add_f32", _ptr(P), ldp if U > 1 else 2 * C, U, _ptr(q), _ptr(b), E, C, _ptr(out),
              _ld(out, C), _lib.stream(dev))
    return out


def pair_segment_sum(g: torch.Tensor, inc_ptr: torch.Tensor, inc_slot: torch.Tensor,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """S [U, 2C]: S[v, side C + c] = ((+0 + g[e_1, c]) + g[e_2, c]) + ... over the slots 2 e + side of
    inc_slot[inc_ptr[v] : inc_ptr[v + 1]] with that side, in stored order (EdgeBatch.incidence()).  On a HIP
    device: srg_pair_segment_sum_f32, fp32, g and out may be column windows of wider panels.  On the CPU:
    index_add_ over the slots in stored order, which adds sequentially there; any float dtype."""
    if g.dim() != 2:
        raise ValueError(f"g must be [E, C], got {tuple(g.shape)}")
    E, C = g.shape
    dev = g.device
    inc_ptr, inc_slot = _ids(inc_ptr, "inc_ptr", dev), _ids(inc_slot, "inc_slot", dev)
    if inc_ptr.dim() != 1 or inc_ptr.numel() < 1 or inc_slot.dim() != 1 or inc_slot.numel() != 2 * E:
        raise ValueError(f"inc_ptr must be [U + 1] and inc_slot [{2 * E}]")
    U = inc_ptr.numel() - 1
    if not _on_device(g):
        S = torch.zeros((2 * U, C), dtype=g.dtype, device=dev)
        node = torch.repeat_interleave(torch.arange(U, dtype=torch.int64), inc_ptr[1:] - inc_ptr[:-1],
                                       output_size=2 * E)
        S.index_add_(0, 2 * node + (inc_slot & 1), g[inc_slot >> 1])
        S = S.reshape(U, 2 * C)
        if out is not None:
            out.copy_(S)
            return out
        return S
    g, ldg = _panel(g, "g", dev)
    if out is None:
        out = torch.empty((U, 2 * C), dtype=torch.float32, device=dev)
    else:
        if tuple(out.shape) != (U, 2 * C) or out.dtype != torch.float32 or out.device != dev \
                or (C > 0 and out.stride(1) != 1) or (U > 1 and out.stride(0) < 2 * C):
            raise ValueError(f"out must be a float32 [{U}, {2 * C}] panel with unit column stride on {dev}")
    _lib.call(dev, "srg_pair_segment_sum_f32", _ptr(g), ldg if E > 1 else C, E, _ptr(inc_ptr), _ptr(inc_slot), U, C,
              _ptr(out), _ld(out, 2 * C), _lib.stream(dev))
    return out


# ---- autograd ---------------------------------------------------------------------------------------
def _stacked(weight, h):
    """[W0; W1], [2C, h]: the two sides of the head's weight, one under the other."""
    return torch.cat((weight[:, :h], weight[:, h:]), dim=0)


class _PairLinear(torch.autograd.Function):

    @staticmethod
    def forward(ctx, z, weight, bias, batch):
        z, weight = z.detach(), weight.detach()
        bias = bias.detach() if bias is not None else None
        h = z.shape[1]
        ctx.batch, ctx.has_bias = batch, bias is not None
        ctx.save_for_backward(z, weight)
        P = z @ _stacked(weight, h).t()
        return pair_gather_add(P, batch.local, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        z, weight = ctx.saved_tensors
        h, C = z.shape[1], weight.shape[0]
        need_z, need_w, need_b = ctx.needs_input_grad[:3]
        dz = dw = db = None
        if need_z or need_w:
            S = pair_segment_sum(grad, *ctx.batch.incidence())
            if need_z:
                # one product of C terms per side and one add (DESIGN.md 5.14's bound counts C + 1 roundings)
                dz = torch.addmm(S[:, :C] @ weight[:, :h], S[:, C:], weight[:, h:])
            if need_w:
                dw = torch.cat((S[:, :C].t() @ z, S[:, C:].t() @ z), dim=1)
        if need_b and ctx.has_bias:
            db = grad.sum(0)
        return dz, dw, db, None


class _GatherUnique(torch.autograd.Function):
    """z[n_id] for unique n_id: the backward writes every gradient row to its own row of a zero panel."""

    @staticmethod
    def forward(ctx, z, n_id):
        ctx.n = z.shape[0]
        ctx.save_for_backward(n_id)
        z = z.detach()
        if _on_device(z):
            from .spmm import gather_rows
            return gather_rows(_panel(z, "z", z.device)[0], n_id)
        return z.index_select(0, n_id)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (n_id,) = ctx.saved_tensors
        return grad.new_zeros((ctx.n, grad.shape[1])).index_copy_(0, n_id, grad), None


def pair_linear(z: torch.Tensor, q, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """linear(cat(z[q[:, 0]], z[q[:, 1]], dim=-1)) with linear = (weight [C, 2h], bias [C] or None), re-associated
    as the module docstring states: [E, C]; differentiable once in z, weight and bias.

    q an EdgeBatch: z is [U, h], the rows of q.n_id, and q.local addresses it (the row paths hand such a z over:
    graph_conv(..., rows=q.n_id), gather_rows, aggregate_rows).  q an int [E, 2] tensor (or anything EdgeBatch
    takes) of ids over a z of [n, h]: an EdgeBatch is built inside and z[n_id] is taken with gather_rows; the ids
    are unique, so that gather's backward is a plain row copy into zeros.
    On a HIP device the operands are fp32 (anything else raises TypeError: there is no torch fallback) and the
    two passes over the pairs are srg_pair_gather_add_f32 and srg_pair_segment_sum_f32: no [E, 2h] buffer, no
    atomics, bit for bit the same from run to run, whatever order torch's GEMMs sum in being fixed per shape.
    On the CPU the same association runs in torch ops in any float dtype."""
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or not z.is_floating_point():
        raise TypeError("z must be a 2-D float tensor")
    h = z.shape[1]
    if weight.dim() != 2 or weight.shape[1] != 2 * h:
        raise ValueError(f"weight must be [C, {2 * h}], got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"bias must be [{weight.shape[0]}], got {tuple(bias.shape)}")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and (t.dtype != z.dtype or t.device != z.device):
            raise TypeError(f"{name} is {t.dtype} on {t.device}, z is {z.dtype} on {z.device}")
    if _on_device(z) and z.dtype != torch.float32:
        raise TypeError(f"pair_linear computes in fp32 on the device, z is {z.dtype}")
    if isinstance(q, EdgeBatch):
        batch = q
        if batch.device != z.device:
            raise ValueError(f"the EdgeBatch is on {batch.device}, z on {z.device}")
        if z.shape[0] != batch.num_nodes:
            raise ValueError(f"z has {z.shape[0]} rows, the EdgeBatch {batch.num_nodes} endpoint nodes")
    else:
        batch = EdgeBatch(q, z.shape[0], z.device)
        z = _GatherUnique.apply(z, batch.n_id)
    return _PairLinear.apply(z, weight, bias, batch)


def edge_head(linear, feature: torch.Tensor, q, dropout=None) -> torch.Tensor:
    """The edge head of LogisticRegression, MultiLayerPerceptron and ResMultiLayerPerceptron:
    linear(dropout(cat(feature[q0], feature[q1]))) with `linear` an nn.Linear(2h, C), `q` as pair_linear takes
    it and `dropout` the model's nn.Dropout or None.

    MultiLayerPerceptron applies its dropout to the concatenation: a mask over [E, 2h] draws one number per
    (edge, side, column) and does not commute with the split into per-node products.  With `dropout` in training
    mode and p > 0 the helper therefore runs the reference's composition (two indexed gathers, cat, dropout,
    linear: the [E, 2h] buffer and torch's indexing backward); in every other case dropout is the identity and
    the head is pair_linear."""
    if dropout is not None and dropout.training and dropout.p > 0:
        idx = q.local if isinstance(q, EdgeBatch) else EdgeBatch(q, feature.shape[0], feature.device).edges
        x = torch.cat((feature[idx[:, 0]], feature[idx[:, 1]]), dim=-1)
        return linear(dropout(x))
    return pair_linear(feature, q, linear.weight, linear.bias)


# ---- the loader -------------------------------------------------------------------------------------
class EdgeBatchLoader:
    """Iterates over the E query pairs in batches of batch_size, as the reference's
    DataLoader(range(E), batch_size, shuffle) does, and relabels each batch as link_cls_mini_batch_train does:
    yields (batch, labels[idx], idx) with batch = EdgeBatch(query_edges[idx], n) and idx the int64 positions of
    the batch's pairs in query_edges, on query_edges' device.  len is ceil(E / batch_size); with shuffle the
    epoch's order is torch.randperm(E, generator=generator) on the host, drawn anew per epoch (as
    NeighborLoader's).  The pairs are checked once, here."""

    def __init__(self, query_edges, labels, n: int, batch_size: int, shuffle: bool = True, generator=None):
        whole = EdgeBatch(query_edges, n)        # the id checks, once; its relabelling is not used
        labels = torch.as_tensor(labels)
        if labels.shape[:1] != (whole.num_edges,):
            raise ValueError(f"labels has {tuple(labels.shape)} entries for {whole.num_edges} pairs")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} < 1")
        self.edges, self.labels, self.n, self.batch_size = whole.edges, labels, whole.n, batch_size
        self.shuffle, self.generator = bool(shuffle), generator

    def __len__(self):
        return math.ceil(self.edges.shape[0] / self.batch_size)

    def index_batches(self):
        """The epoch's batches of positions as host tensors (draws the epoch's permutation)."""
        E = self.edges.shape[0]
        order = torch.randperm(E, generator=self.generator) if self.shuffle else torch.arange(E)
        return [order[i:i + self.batch_size] for i in range(0, E, self.batch_size)]

    def __iter__(self):
        for idx in self.index_batches():
            idx = idx.to(self.edges.device)
            yield EdgeBatch(self.edges[idx], self.n), self.labels[idx.to(self.labels.device)], idx
