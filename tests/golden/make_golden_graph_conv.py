"""Golden fixture for srgnn.graph_conv: the REFERENCE's own GCN operator path on three small graphs
(development container only, on the CPU).

    python tests/golden/make_golden_graph_conv.py

What runs, unmodified, from the reference tree (make_golden.py's REF_SSRG):
  * SymLaplacianGraphOp.construct_adj (operators/graph_operator/symmetrical_simgraph_laplacian_operator.py),
    imported as make_golden.import_reference imports it;
  * models.utils.scipy_sparse_mat_to_torch_sparse_tensor, what BaseSGModel.preprocess applies to that operator;
  * torch.mm(adj, Z) on the result, as Layer2GraphConvolution.forward calls it, and torch's autograd for the
    gradient of (torch.mm(adj, Z) * G).sum() with respect to Z.
Packages that the imports reach at module top and that are absent here are stubbed from the fixed list of
make_golden_edge_augment.py (its finder answers for those names only, after every real finder has passed).
Only data leaves this script, to tests/golden/graph_conv.npz: per operator the coalesced operator as CSR
arrays (what torch.mm multiplies by), and per width d the product and the gradient; the inputs Z and G are
the same for the three operators, fixed-seed Gaussians rounded to multiples of 1/32 and stored as int8.

The operators: gc_sym05 (undirected, unweighted, r = 0.5: the two scalings commute, so the operator equals
its transpose bit for bit), gc_sym03 (the same graph at r = 0.3: symmetric structure, other values) and
gc_dir05 (a directed graph: asymmetric structure).  Each has a hub row, two isolated nodes (their self loop
only) and, the directed one, rows whose only entry is the diagonal.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_edge_augment as EA  # noqa: E402  (the stub finder and its fixed list)

N = 301
WIDTHS = (7, 47)
PANEL_SCALE = 32      # Z and G are multiples of 1/32 in [-4, 4): one int8 per element in the file


def undirected_graph(seed):
    rng = np.random.default_rng(seed)
    e = 900
    row, col = rng.integers(2, N, e), rng.integers(2, N, e)      # nodes 0 and 1 stay isolated
    keep = row != col
    row, col = row[keep], col[keep]
    hub = np.setdiff1d(rng.choice(np.arange(2, N), 140, replace=False), [17])
    row, col = np.r_[row, np.full(hub.size, 17)], np.r_[col, hub]
    a = sp.coo_matrix((np.ones(row.size), (row, col)), shape=(N, N)).tocsr()
    a = ((a + a.T) > 0).astype(np.float64)
    return sp.csr_matrix(a)


def directed_graph(seed):
    rng = np.random.default_rng(seed)
    e = 1400
    row, col = rng.integers(2, N, e), rng.integers(2, N, e)
    keep = row != col
    row, col = row[keep], col[keep]
    hub = np.setdiff1d(rng.choice(np.arange(2, N), 120, replace=False), [23])
    row, col = np.r_[row, np.full(hub.size, 23)], np.r_[col, hub]
    a = (sp.coo_matrix((np.ones(row.size), (row, col)), shape=(N, N)).tocsr() > 0).astype(np.float64)
    a = sp.csr_matrix(a)
    assert (a != a.T).nnz > 0
    return a


def import_to_torch_sparse():
    finder = EA._StubFinder()
    sys.meta_path.append(finder)
    try:
        from models.utils import scipy_sparse_mat_to_torch_sparse_tensor
    finally:
        sys.meta_path.remove(finder)
    print("stubbed:", sorted(set(n.split(".")[0] for n in finder.made)))
    return scipy_sparse_mat_to_torch_sparse_tensor


def panel(arrs, what, d):
    """The fp32 panel stored as int8 q: q / PANEL_SCALE, exact in fp32 (tests/graph_conv_ref.py reads it so)."""
    return arrs[f"{what}q{d}"].astype(np.float32) / np.float32(PANEL_SCALE)


def run_case(name, adj, r, Op, to_torch, arrs):
    a_hat = Op(prop_steps=None, r=r).construct_adj(adj)
    assert isinstance(a_hat, sp.csr_matrix)
    t = to_torch(a_hat)
    assert t.dtype == torch.float32 and t.layout == torch.sparse_coo
    c = t.coalesce()
    idx, val = c.indices().numpy(), c.values().numpy()
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(ptr, idx[0] + 1, 1)
    arrs.update({f"{name}__indptr": np.cumsum(ptr), f"{name}__indices": idx[1].astype(np.int32),
                 f"{name}__values": val.astype(np.float32), f"{name}__r": np.float64(r)})
    for d in WIDTHS:
        Z, G = panel(arrs, "Z", d), panel(arrs, "G", d)
        z = torch.from_numpy(Z).requires_grad_(True)
        y = torch.mm(t, z)                                   # the reference's own tensor, as its layer calls it
        (y * torch.from_numpy(G)).sum().backward()
        arrs.update({f"{name}__Y{d}": y.detach().numpy(), f"{name}__dZ{d}": z.grad.numpy()})
    deg = np.diff(arrs[f"{name}__indptr"])
    print(f"{name}: n={N} nnz={idx.shape[1]} longest row {deg.max()}, rows of one entry {(deg == 1).sum()}")


def main():
    Op = MG.import_reference()[0]
    to_torch = import_to_torch_sparse()
    arrs = {"panel_scale": np.int64(PANEL_SCALE)}
    rng = np.random.default_rng(20270)
    for d in WIDTHS:             # the same fixed-seed Z and G for the three operators
        for what in ("Z", "G"):
            arrs[f"{what}q{d}"] = np.clip(np.rint(rng.standard_normal((N, d)) * PANEL_SCALE), -128, 127).astype(np.int8)
    und = undirected_graph(20271)
    run_case("gc_sym05", und, 0.5, Op, to_torch, arrs)
    run_case("gc_sym03", und, 0.3, Op, to_torch, arrs)
    run_case("gc_dir05", directed_graph(20272), 0.5, Op, to_torch, arrs)
    path = os.path.join(HERE, "graph_conv.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
