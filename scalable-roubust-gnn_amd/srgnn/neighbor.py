"""Neighbour-sampled mini-batches on the device: the sampled row slice of a node set, the bipartite block
around it and the loader that stacks blocks layer by layer.

The reference's runner imports PyG's NeighborSampler beside ClusterLoader: GraphSAGE is trained on
products- and papers-sized graphs by sampling, per layer, at most `size` in-neighbours of every node the
layer above needs.  This module is that path for a DeviceCSR over targets (row i: the sources of i):

  sample_neighbors(A, nodes, fanout, seed)   rows `nodes` of A, each cut to at most `fanout` entries by
                                             srg_csr_sample_f32: the sampled analogue of
                                             cluster.induced_subgraph(relabel=False)
  sample_block(A, nodes, fanout, seed)       the same rows as a bipartite SampledBlock [B, S] over the
                                             sources n_id, the targets first
  NeighborLoader(A, node_idx, sizes, ...)    per batch of seed nodes one block per entry of `sizes`, each
                                             sampled round the sources of the one before

A row with more than `fanout` entries keeps `fanout` of them, at distinct positions drawn by the keyed
bijection include/srgnn_hip.h states, keyed by (seed, node id) and emitted in stored order; every other row is
copied.  PyG is absent here: the loader restates PyG's NeighborSampler from its published description (the
layers are sampled from the seed nodes outwards and yielded outermost first, every block's targets are the
first of its sources); PyG's random stream is not reproduced and parity with its bits is not pinned.  There is
no torch fallback: the sampling is a kernel of libsrgnn_hip.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .cluster import _ptr
from .csr import DeviceCSR, _dev
from .graph_conv import batch_rows

__all__ = ["sample_neighbors", "sample_block", "SampledBlock", "NeighborLoader", "NeighborBatch", "layer_seed",
           "MAX_FANOUT"]

MAX_FANOUT = 64
_M64 = (1 << 64) - 1
_EPOCH_MUL, _BATCH_MUL, _LAYER_MUL = 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7, 0xDB4F0B9175AE2165


def layer_seed(seed: int, epoch: int, batch: int, layer: int) -> int:
    """The seed NeighborLoader samples layer `layer` (an index into `sizes`) of batch `batch` of epoch `epoch`
    with: (seed + 0xD1B54A32D192ED03 (epoch + 1) + 0x8CB92BA72F3D8DD7 (batch + 1) + 0xDB4F0B9175AE2165 (layer + 1))
    mod 2^64.  The multipliers are odd, so no two layers of one batch, and no two batches of one epoch, share a
    seed."""
    return ((seed & _M64) + _EPOCH_MUL * (epoch + 1) + _BATCH_MUL * (batch + 1) + _LAYER_MUL * (layer + 1)) & _M64


def _fanout(fanout) -> int:
    if isinstance(fanout, bool) or not isinstance(fanout, int):
        raise TypeError(f"fanout must be an int, got {type(fanout).__name__}")
    if fanout == 0 or fanout > MAX_FANOUT:
        raise ValueError(f"fanout={fanout}: 1 .. {MAX_FANOUT} entries per row, or a negative value for every entry")
    return fanout


def _seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"seed must be an int, got {type(seed).__name__}")
    return seed & _M64


def _sample(A: DeviceCSR, nodes, fanout, seed, eid: bool):
    if not isinstance(A, DeviceCSR):
        raise TypeError("neighbour sampling takes a DeviceCSR")
    if A.is_span or A.schedules_subset:
        raise ValueError("neighbour sampling takes a whole operator, not a column block or row group")
    fanout, seed = _fanout(fanout), _seed(seed)
    ids, pos, unique = batch_rows(nodes, A.n_rows, A.device)
    if not unique:
        raise ValueError("nodes repeats an id: a node set holds every node once")
    dev = _dev(A.device)
    B = ids.numel()
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    if B:
        cnt = A.indptr[ids + 1] - A.indptr[ids]
        if fanout > 0:
            cnt = cnt.clamp(max=fanout)
        torch.cumsum(cnt, 0, out=ptr[1:])
    nnz = int(ptr[-1]) if B else 0
    out_idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(nnz, dtype=torch.float32, device=dev)
    out_eid = torch.empty(nnz, dtype=torch.int64, device=dev) if eid else None
    if nnz:
        _lib.call(dev, "srg_csr_sample_f32", A.indptr.data_ptr(), _ptr(A.indices), _ptr(A.values), A.n_rows,
                  ids.data_ptr(), B, fanout, seed, ptr.data_ptr(), out_idx.data_ptr(), out_val.data_ptr(),
                  _ptr(out_eid), _lib.stream(dev))
    sub = DeviceCSR(ptr, out_idx, out_val, B, A.n_cols, None, None, None, None, thresholds=A.thresholds)
    return sub, ids, pos, out_eid


def sample_neighbors(A: DeviceCSR, nodes, fanout: int, seed: int, eid: bool = False):
    """(sub, ids[, eid]): row b of `sub` is row ids[b] of A cut to at most `fanout` entries.

    nodes: as cluster.induced_subgraph takes them (graph_conv.batch_rows: negative ids wrap, an id out of range
    raises IndexError, bool or float ids TypeError, a shape that is not 1-D ValueError, all before any launch; a
    repeated id raises ValueError).  fanout: 1 .. 64, or negative for every entry; seed: any int, taken mod 2^64.
    sub is a DeviceCSR [B, n_cols] in A's column ids: a row of at most `fanout` entries (any row, with a
    negative fanout) is scipy's A[S] row; a longer one holds `fanout` of its entries, at distinct positions
    that depend on (seed, ids[b], the row's length, fanout) only, in stored order, values bit for bit.
    eid=True also returns int64 [nnz(sub)]: entry t of sub is entry eid[t] of A.

    The row counts are closed form: ptr comes from A.indptr with torch ops and one cumsum, then one launch of
    srg_csr_sample_f32.  The one host read of ptr[-1], which sizes the outputs, is the only synchronisation."""
    sub, ids, _, out_eid = _sample(A, nodes, fanout, seed, eid)
    return (sub, ids, out_eid) if eid else (sub, ids)


class SampledBlock:
    """One bipartite layer of a sampled mini-batch.

    csr     DeviceCSR [n_dst, S]: row b holds the sampled sources of target n_id[b]; a column id is a position
            in n_id; values are the operator's, bit for bit (not renormalised over the sample)
    n_id    int64 [S]: the sources in original ids; n_id[:n_dst] are the targets in the order given,
            n_id[n_dst:] the sampled columns that are not targets, ascending
    n_dst   the number of targets
    eid     int64 [nnz(csr)], built when first asked for: entry t of csr is entry eid[t] of the operator

    mean_operator() is the layer GraphSAGE runs on it (srgnn.sage).  graph_conv_operator() and gat_graph() are
    the block as a square graph over its sources, [S, S] with the rows of the sources that are not targets
    empty: what GraphConvolution2 and GAT take, as they take a ClusterBatch's; the targets' outputs are the
    first n_dst rows (rows=range(n_dst) for the last layer)."""

    def __init__(self, A: DeviceCSR, nodes, fanout: int, seed: int):
        if not isinstance(A, DeviceCSR):
            raise TypeError("sample_block takes a DeviceCSR")
        if A.n_rows != A.n_cols:
            raise ValueError(f"sample_block takes a square operator, got {A.n_rows}x{A.n_cols}")
        sub, ids, pos, _ = _sample(A, nodes, fanout, seed, False)
        n, B = A.n_cols, ids.numel()
        cols = sub.indices.to(torch.int64)
        # the sampled ids are copies of A's: checked before one is used as an index
        if cols.numel() and bool(((cols < 0) | (cols >= n)).any()):
            raise ValueError(f"a sampled column id is outside [0, {n}): the operator is not a valid CSR")
        mark = torch.zeros(n, dtype=torch.bool, device=ids.device)
        mark[cols] = True
        mark[ids] = False
        frontier = mark.nonzero().reshape(-1)                       # ascending
        pos[frontier] = torch.arange(B, B + frontier.numel(), dtype=torch.int32, device=ids.device)
        self._A, self._fanout, self._seed, self._eid = A, fanout, seed, None
        self.n_id = torch.cat([ids, frontier])
        self.n_dst = B
        self.csr = DeviceCSR(sub.indptr, pos[cols], sub.values, B, self.n_id.numel(), None, None, None, None,
                             thresholds=A.thresholds)
        self._square = self._mean = None

    @property
    def eid(self) -> torch.Tensor:
        if self._eid is None:
            self._eid = _sample(self._A, self.n_id[:self.n_dst], self._fanout, self._seed, True)[3]
        return self._eid

    def square_csr(self) -> DeviceCSR:
        """csr padded to [S, S] with empty rows for the sources that are not targets (shares indices and values)."""
        if self._square is None:
            c, S = self.csr, self.n_id.numel()
            ip = torch.cat([c.indptr, c.indptr[-1:].expand(S - self.n_dst)])
            self._square = DeviceCSR(ip, c.indices, c.values, S, S, None, None, None, None, thresholds=c.thresholds)
        return self._square

    def mean_operator(self):
        """sage.mean_operator(csr), built on first use."""
        if self._mean is None:
            from .sage import mean_operator
            self._mean = mean_operator(self.csr)
        return self._mean

    def graph_conv_operator(self):
        """GraphConvOperator.from_device_csr(square_csr()): the sampled values, not renormalised."""
        from .graph_conv import GraphConvOperator
        return GraphConvOperator.from_device_csr(self.square_csr())

    def gat_graph(self, add_self_loops: bool = True):
        """GATGraph.from_device_csr(square_csr(), add_self_loops)."""
        from .gat import GATGraph
        return GATGraph.from_device_csr(self.square_csr(), add_self_loops)

    def __repr__(self):
        return f"SampledBlock(n_dst={self.n_dst}, n_src={self.n_id.numel()}, nnz={self.csr.indices.numel()})"


def sample_block(A: DeviceCSR, nodes, fanout: int, seed: int) -> SampledBlock:
    """The SampledBlock of `nodes` (see sample_neighbors for nodes, fanout and seed) of a square operator.
    The frontier is built with device ops: an n-sized mark of the sampled columns, its nonzero, and a gather of
    the column ids through batch_rows' position table extended by the frontier.  A column id outside
    [0, n_cols) (an operator built with validate=False) raises ValueError before it is used as an index."""
    return SampledBlock(A, nodes, fanout, seed)


class NeighborBatch:
    """One item of a NeighborLoader: n_id (int64, the outermost block's sources: gather the features with it),
    batch_size (the seed nodes, n_id[:batch_size]) and blocks, outermost first: blocks[i] is layer i's, its
    targets the first n_dst of its sources and the sources of blocks[i + 1]."""

    def __init__(self, n_id, batch_size, blocks):
        self.n_id, self.batch_size, self.blocks = n_id, batch_size, blocks

    def __repr__(self):
        return f"NeighborBatch(batch_size={self.batch_size}, n_id={self.n_id.numel()}, blocks={self.blocks})"


class NeighborLoader:
    """Iterates over `node_idx` in batches of batch_size seed nodes, as PyG's NeighborSampler does: for every
    size in `sizes` the current node set is sampled with that fanout (sample_block) and the block's sources
    become the next set; the blocks are yielded reversed, the first layer's first.  len is
    ceil(len(node_idx) / batch_size); with shuffle the epoch's order is torch.randperm(generator=generator) on
    the host, drawn anew per epoch.  Layer l of batch i of epoch e (counted from 0 per loader) is sampled with
    layer_seed(seed, e, i, l)."""

    def __init__(self, A: DeviceCSR, node_idx, sizes, batch_size: int, shuffle: bool = True, generator=None,
                 seed: int = 0):
        if not isinstance(A, DeviceCSR):
            raise TypeError("NeighborLoader takes a DeviceCSR")
        if A.n_rows != A.n_cols:
            raise ValueError(f"NeighborLoader takes a square operator, got {A.n_rows}x{A.n_cols}")
        sizes = [_fanout(s) for s in sizes]
        if not sizes:
            raise ValueError("sizes is empty: one fanout per layer")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} < 1")
        ids, _, unique = batch_rows(range(A.n_rows) if node_idx is None else node_idx, A.n_rows, "cpu")
        if not unique:
            raise ValueError("node_idx repeats an id")
        self.A, self.node_idx, self.sizes, self.batch_size = A, ids, sizes, batch_size
        self.shuffle, self.generator, self.seed, self.epoch = bool(shuffle), generator, _seed(seed), 0

    def __len__(self):
        return math.ceil(self.node_idx.numel() / self.batch_size)

    def seed_batches(self):
        """The epoch's batches of seed nodes as host tensors (draws the epoch's permutation)."""
        n = self.node_idx.numel()
        order = self.node_idx[torch.randperm(n, generator=self.generator)] if self.shuffle else self.node_idx
        return [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]

    def sample(self, seeds, epoch: int, batch: int) -> NeighborBatch:
        """The NeighborBatch of the seed nodes `seeds` as batch `batch` of epoch `epoch`."""
        nodes, blocks = seeds, []
        for layer, size in enumerate(self.sizes):
            blk = sample_block(self.A, nodes, size, layer_seed(self.seed, epoch, batch, layer))
            blocks.append(blk)
            nodes = blk.n_id
        return NeighborBatch(nodes, blocks[0].n_dst, blocks[::-1])

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        for i, seeds in enumerate(self.seed_batches()):
            yield self.sample(seeds, epoch, i)
