"""Edge augmentation on the device: every low-degree node gets edges to its nearest sampled candidates.

The reference repairs a sparsified graph before construct_adj reads it (SSRG/data_augument.py:73-103,
helpers utils.py:29-38): every node whose degree is below degree_level draws 100 x (degree_level - degree)
candidate nodes and gets edges to the (degree_level - degree) nearest of them, nearest in the L2 distance
between rows of the augmentation model's output; the edge list is then made symmetric and unique.  There
it is a Python loop over the nodes (a list.remove, a random.sample, a norm, a sort and a torch.cat onto the
growing edge list per node).  Here all low-degree nodes are served at once:

  degrees, the low-degree rows, the pointer arrays     torch on the device (bincount, cumsum)
  the candidates                                       srg_sample_distinct_i64, or the caller's, or a
                                                       host replay of the reference's own draw
  distances and the selection of the nearest           srg_knn_select_f32
  union, flip, sort by row * n + col, unique           torch on the device (srgnn.directed's idiom)

The contract: deg[i] counts i in cat(row, col) (duplicates count, a self loop twice);
dist = ||F[node] - F[cand]||_2 in fp32 in the fixed summation order of include/srgnn_hip.h; equal
distances go by position in the candidate list, NaN after +Inf; the result is int64 [2, E] sorted by
(row, col) without duplicates: torch.unique(dim=1) of the reference.  The device draw is not the
reference's random stream; candidates="reference" replays that stream on the host for parity on small
graphs.  No CPU fallback: without a HIP device the functions raise.
"""
from __future__ import annotations

import random
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .sparse import _panel

__all__ = ["edge_augment", "edge_augument", "knn_select", "sample_distinct", "reference_candidates", "Selected"]


class Selected(NamedTuple):
    """What edge_augment chose (return_selected=True), all on the device: row i is low-degree node
    nodes[i] (ascending ids), its candidates cand[cand_ptr[i]:cand_ptr[i+1]] in list order and the chosen
    ones sel[out_ptr[i]:out_ptr[i+1]], nearest first, at distances dist[...]."""
    nodes: torch.Tensor
    cand_ptr: torch.Tensor
    cand: torch.Tensor
    out_ptr: torch.Tensor
    sel: torch.Tensor
    dist: torch.Tensor


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("srgnn.augment needs a HIP device")
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _i64(t, name, dev):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int64 or t.device != dev:
        raise ValueError(f"{name} must be a 1-D int64 tensor on {dev}")
    return t.contiguous()


def knn_select(X: torch.Tensor, query: torch.Tensor, cand_ptr: torch.Tensor, cand: torch.Tensor,
               out_ptr: torch.Tensor, return_dist: bool = False):
    """srg_knn_select_f32: for row r the out_ptr[r+1] - out_ptr[r] nearest of cand[cand_ptr[r]:cand_ptr[r+1]]
    to node query[r], nearest first (ties by list position, NaN after +Inf, ids outside [0, n) last), in
    the L2 distance between rows of X (fp32 [n, d]; a column window is fine).  Returns the selected ids
    (int64 [out_ptr[-1]]) and, with return_dist, their distances.  Bad pointer arrays raise SrgError."""
    dev = X.device
    X, ldx = _panel(X, "X", dev)
    query, cand_ptr, cand, out_ptr = (_i64(t, s, dev) for t, s in ((query, "query"), (cand_ptr, "cand_ptr"),
                                                                  (cand, "cand"), (out_ptr, "out_ptr")))
    R = query.numel()
    if cand_ptr.numel() != R + 1 or out_ptr.numel() != R + 1:
        raise ValueError(f"{R} query rows need {R + 1} entries in cand_ptr and out_ptr")
    total = int(out_ptr[-1]) if R else 0
    if R and int(cand_ptr[-1]) > cand.numel():
        raise ValueError(f"cand_ptr ends at {int(cand_ptr[-1])}, cand has {cand.numel()} entries")
    sel = torch.empty(max(total, 0), dtype=torch.int64, device=dev)
    dist = torch.empty(max(total, 0), dtype=torch.float32, device=dev) if return_dist else None
    _lib.call(dev, "srg_knn_select_f32", _ptr(X), ldx, X.shape[0], X.shape[1], _ptr(query), cand_ptr.data_ptr(),
              _ptr(cand), out_ptr.data_ptr(), R, _ptr(sel), _ptr(dist), _lib.stream(dev))
    return (sel, dist) if return_dist else sel


def sample_distinct(query: torch.Tensor, cand_ptr: torch.Tensor, n: int, seed: int = 0) -> torch.Tensor:
    """srg_sample_distinct_i64: row r receives cand_ptr[r+1] - cand_ptr[r] distinct ids of [0, n) other than
    query[r], a function of (seed, r, position) only -- a keyed bijection, not the reference's random
    stream.  A row that asks for more than n - 1 raises SrgError."""
    dev = query.device
    query, cand_ptr = _i64(query, "query", dev), _i64(cand_ptr, "cand_ptr", dev)
    R = query.numel()
    if cand_ptr.numel() != R + 1:
        raise ValueError(f"{R} query rows need {R + 1} entries in cand_ptr")
    cand = torch.empty(int(cand_ptr[-1]) if R else 0, dtype=torch.int64, device=dev)
    _lib.call(dev, "srg_sample_distinct_i64", _ptr(query), cand_ptr.data_ptr(), R, int(n),
              int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(cand), _lib.stream(dev))
    return cand


def reference_candidates(edge_row, edge_col, n: int, degree_level: int = 1, per_edge: int = 100):
    """The reference's own draw, replayed on the host from Python's global `random` (seed it first):
    (nodes, ptr, ids) as numpy int64, rows in the reference's visiting order.

    Nodes are visited in ascending degree; equal degrees in the order of first occurrence in
    cat(row, col), then the nodes that occur nowhere in id order.  A pool list starts as 0..n-1; for each
    visited node of degree < degree_level the node is removed from the pool,
    random.sample(pool, per_edge * (degree_level - degree)) is drawn and the node is appended back, so the
    pool's changing order is part of the stream.  A draw larger than the pool raises ValueError, as the
    reference does.  O(n) per visited node (the list.remove): for parity on small graphs only."""
    total = np.concatenate([np.asarray(edge_row, dtype=np.int64).ravel(), np.asarray(edge_col, dtype=np.int64).ravel()])
    deg = np.bincount(total, minlength=n).astype(np.int64)
    present, first = np.unique(total, return_index=True)
    seen = np.zeros(n, dtype=bool)
    seen[present] = True
    order = np.concatenate([present[np.argsort(first, kind="stable")], np.nonzero(~seen)[0]])
    order = order[np.argsort(deg[order], kind="stable")]
    pool = list(range(n))
    nodes, ptr, ids = [], [0], []
    for node in order.tolist():
        if deg[node] >= degree_level:
            break
        pool.remove(node)
        drawn = random.sample(pool, per_edge * int(degree_level - deg[node]))
        pool.append(node)
        nodes.append(node)
        ids.extend(drawn)
        ptr.append(len(ids))
    return np.asarray(nodes, dtype=np.int64), np.asarray(ptr, dtype=np.int64), np.asarray(ids, dtype=np.int64)


def _rows_by_node_id(nodes, ptr, ids):
    """The lists of (nodes, ptr, ids) reordered so that their nodes ascend (each list keeps its order)."""
    perm = np.argsort(nodes, kind="stable")
    lens = np.diff(ptr)[perm]
    new_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.repeat(ptr[:-1][perm] - new_ptr[:-1], lens) + np.arange(int(new_ptr[-1]))
    return nodes[perm], new_ptr, ids[pos]


def _check_arguments(edge_row, edge_col, n, features, degree_level, per_edge, candidates):
    for t, name in ((edge_row, "edge_row"), (edge_col, "edge_col")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f"{name} must be a 1-D integer tensor")
    if edge_row.numel() != edge_col.numel():
        raise ValueError(f"edge_row has {edge_row.numel()} entries, edge_col {edge_col.numel()}")
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32:
        raise TypeError("features must be a float32 tensor")
    if int(n) < 0 or int(n) >= 2 ** 31:
        raise ValueError(f"n={n} outside [0, 2^31)")
    if features.dim() != 2 or features.shape[0] != n:
        raise ValueError(f"features must be [n={n}, d], got {tuple(features.shape)}")
    if features.shape[1] > _lib.SRG_KNN_MAX_D:
        raise ValueError(f"features have {features.shape[1]} columns, at most {_lib.SRG_KNN_MAX_D} are supported")
    if int(degree_level) < 0 or int(per_edge) < 1:
        raise ValueError(f"degree_level={degree_level} must be >= 0 and per_edge={per_edge} >= 1")
    if candidates is None or (isinstance(candidates, str) and candidates == "reference"):
        return
    if isinstance(candidates, str) or not isinstance(candidates, (tuple, list)) or len(candidates) != 2:
        raise ValueError('candidates must be None, "reference" or a pair (ptr, ids)')
    for t, name in zip(candidates, ("candidates ptr", "candidates ids")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f"{name} must be a 1-D integer tensor")


def edge_augment(edge_row: torch.Tensor, edge_col: torch.Tensor, n: int, features: torch.Tensor,
                 degree_level: int = 1, per_edge: int = 100, candidates=None, seed: int = 0,
                 return_selected: bool = False):
    """The repaired edge list of edge_augument (SSRG/data_augument.py:73-103) as int64 [2, E], sorted by
    (row, col) and unique, on edge_row's device.

    edge_row / edge_col: one entry per stored edge (host or device); features: fp32 [n, d], host or device,
    a strided column window is fine.  Every node of degree < degree_level (degree = occurrences in
    cat(row, col)) gets edges to the degree_level - degree nearest of its per_edge x (degree_level - degree)
    candidates; the old and the new pairs, all of them flipped as well, are returned.

    candidates=None draws them on the device from `seed` (sample_distinct; not the reference's stream).
    candidates=(ptr, ids): row i lists the candidates of the i-th low-degree node in ascending id; ids
    outside [0, n) raise IndexError, a list of the wrong length or one that holds its own node ValueError,
    before anything is launched.  candidates="reference" replays the reference's draw on the host from
    Python's global `random` (reference_candidates: O(n) per node, small graphs only).  More candidates
    than n - 1 for a node raise ValueError, as in the reference; more than SRG_KNN_MAX_CAND = 4096
    (degree_level 40 at per_edge 100) ValueError too.  return_selected also returns a Selected."""
    _check_arguments(edge_row, edge_col, n, features, degree_level, per_edge, candidates)
    n, L, per_edge = int(n), int(degree_level), int(per_edge)
    dev = _device()
    home = edge_row.device
    row = edge_row.to(dev, torch.int64)
    col = edge_col.to(dev, torch.int64)
    F, _ = _panel(features.to(dev), "features", dev)
    if row.numel():
        lo = torch.minimum(row.min(), col.min())
        hi = torch.maximum(row.max(), col.max())
        lo, hi = (int(v) for v in torch.stack([lo, hi]).tolist())
        if lo < 0 or hi >= n:
            raise IndexError(f"edge ids span [{lo}, {hi}], outside [0, {n})")
    deg = torch.bincount(torch.cat([row, col]), minlength=n) if n else torch.zeros(0, dtype=torch.int64, device=dev)
    nodes = torch.nonzero(deg < L).flatten()
    need = L - deg[nodes]
    R = nodes.numel()
    out_ptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum(need, 0, out=out_ptr[1:])
    cand_ptr = out_ptr * per_edge
    longest = int(need.max()) * per_edge if R else 0
    if longest > n - 1 and (candidates is None or isinstance(candidates, str)):
        raise ValueError(f"a node needs {longest} distinct candidates, the graph has {n - 1} other nodes")
    if longest > _lib.SRG_KNN_MAX_CAND:
        raise ValueError(f"a node has {longest} candidates, more than SRG_KNN_MAX_CAND={_lib.SRG_KNN_MAX_CAND}")
    if candidates is None:
        cand = sample_distinct(nodes, cand_ptr, n, seed)
    elif isinstance(candidates, str):
        ref_nodes, ref_ptr, ref_ids = _rows_by_node_id(*reference_candidates(row.cpu().numpy(), col.cpu().numpy(), n,
                                                                             L, per_edge))
        assert np.array_equal(ref_nodes, nodes.cpu().numpy()) and np.array_equal(ref_ptr, cand_ptr.cpu().numpy())
        cand = torch.from_numpy(ref_ids).to(dev)
    else:
        ptr = candidates[0].to(dev, torch.int64)
        cand = candidates[1].to(dev, torch.int64).contiguous()
        if ptr.numel() != R + 1 or not torch.equal(ptr, cand_ptr) or cand.numel() != int(cand_ptr[-1]):
            raise ValueError(f"candidates must hold per_edge x (degree_level - degree) ids for each of the {R} "
                             f"low-degree nodes in ascending id")
        if cand.numel():
            own = (cand == torch.repeat_interleave(nodes, need * per_edge)).any()
            lo, hi, own = (int(v) for v in torch.stack([cand.min(), cand.max(), own.to(torch.int64)]).tolist())
            if lo < 0 or hi >= n:
                raise IndexError(f"candidate ids span [{lo}, {hi}], outside [0, {n})")
            if own:
                raise ValueError("a candidate list holds its own node")
    sel, dist = knn_select(F, nodes, cand_ptr, cand, out_ptr, return_dist=True)
    new_row = torch.repeat_interleave(nodes, need)
    rows = torch.cat([row, new_row, col, sel])
    cols = torch.cat([col, sel, row, new_row])
    # union + flip, then torch.unique(dim=1): sorted by (row, col), one of each (srgnn.directed._coalesce's key)
    key = torch.unique_consecutive(torch.sort(rows * n + cols).values) if n else rows
    edge_index = torch.stack([key // n, key % n]) if n else torch.zeros((2, 0), dtype=torch.int64, device=dev)
    edge_index = edge_index.to(home)
    if return_selected:
        return edge_index, Selected(nodes, cand_ptr, cand, out_ptr, sel, dist)
    return edge_index


def edge_augument(dataset, soft_label: torch.Tensor, degree_level: int = 1) -> torch.Tensor:
    """The reference's spelling and argument shape (data_augument.py:73; its degree_level is a global of
    its config): dataset.edge.row / .col, dataset.x.shape[0] nodes, the reference's own draw replayed from
    Python's global `random`."""
    return edge_augment(dataset.edge.row, dataset.edge.col, int(dataset.x.shape[0]), soft_label,
                        degree_level=degree_level, candidates="reference")
