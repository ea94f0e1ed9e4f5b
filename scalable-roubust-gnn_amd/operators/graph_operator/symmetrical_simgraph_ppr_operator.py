"""PprGraphOp: (1 - alpha) Â + alpha I (SSRG/operators/graph_operator/
symmetrical_simgraph_ppr_operator.py:7-21).  Same GraphOp path, different operator values."""
import scipy.sparse as sp

from operators.base_operator import GraphOp
from operators.utils import adj_to_symmetric_norm


class PprGraphOp(GraphOp):
    def __init__(self, prop_steps, r=0.5, alpha=0.15):
        super(PprGraphOp, self).__init__(prop_steps)
        self.r = r
        self.alpha = alpha

    def construct_adj(self, adj):
        if isinstance(adj, sp.csr_matrix):
            adj = adj.tocoo()
        elif not isinstance(adj, sp.coo_matrix):
            raise TypeError("The adjacency matrix must be a scipy.sparse.coo_matrix/csr_matrix!")
        norm = adj_to_symmetric_norm(adj, self.r)
        return ((1 - self.alpha) * norm + self.alpha * sp.eye(adj.shape[0])).tocsr()

    def construct_adj_device(self, adj, device):
        """construct_adj on the GPU (srgnn.construct.ppr_norm): the host construct_adj's fp64 values bit
        for bit for a canonical adj (sorted rows, no duplicates), weighted or not, zero and negative
        degrees included (NaN payloads apart); for a non-canonical weighted adj scipy adds a row of
        adj + I in its own merge order, so a degree may differ in the last bit."""
        from srgnn.construct import ppr_norm
        return ppr_norm(adj.indptr, adj.indices, adj.data, adj.shape[0], self.r, self.alpha, device=device)
