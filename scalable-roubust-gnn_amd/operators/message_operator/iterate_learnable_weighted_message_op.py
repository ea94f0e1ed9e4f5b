"""IterateLearnableWeightedMessageOp (SSRG/operators/message_operator/iterate_learnable_weighted_message_op.py:
8-51): 'recursive' combination -- hop i's per-node weight comes from Linear(2 feat_dim, 1) on
[hop i | the running combination], the weights so far are re-softmaxed, and the combination is
rebuilt from hop `start` with them.  Same parameters and arithmetic order as the reference.

`fused` (default False): with it set, start == 0 and float32 hop tensors held on a HIP device, none of which
requires grad, run srgnn.hop_attention.hop_attention_recursive (the device kernels of DESIGN.md §5.4.3: the same
weights within a derived rounding bound, gradients for the Linear's weight and bias, two streaming passes and a
scalar recurrence per row instead of (end - start)^2 panel-sized steps).  Everything else takes the composition
below, unchanged -- the IndexError the reference raises for start >= 1 included.

aggregate_rows(feat_list, idx) is the mini-batch step of the reference's training loop, aggregate over
[f[idx] for f in feat_list]; under `fused` it reads the batch's rows from the device panels in place.
"""
import torch
import torch.nn.functional as F
from torch.nn import Linear

from operators.base_operator import MessageOp


class IterateLearnableWeightedMessageOp(MessageOp):
    def __init__(self, start, end, combination_type, *args):
        super(IterateLearnableWeightedMessageOp, self).__init__(start, end)
        self.aggr_type = "iterate_learnable_weighted"
        if combination_type != "recursive":
            raise ValueError("Invalid weighted combination type! Type must be 'recursive'.")
        self.combination_type = combination_type
        if len(args) != 1:
            raise ValueError("Invalid parameter numbers for the recursive iterate weighted aggregator!")
        self.learnable_weight = Linear(2 * args[0], 1)
        self.fused = False

    def combine(self, feat_list):
        if (self.fused and self.start == 0 and isinstance(feat_list, (list, tuple)) and len(feat_list) > 0
                and all(isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.float32 and not f.requires_grad
                        for f in feat_list)):
            from srgnn.hop_attention import hop_attention_recursive
            return hop_attention_recursive(list(feat_list), self.end, self.learnable_weight.weight,
                                           self.learnable_weight.bias)
        base = feat_list[self.start]
        combined = base
        weights = None
        for i in range(self.start, self.end):
            w_i = torch.sigmoid(self.learnable_weight(torch.hstack((feat_list[i], combined))))
            weights = w_i if weights is None else torch.hstack((weights, w_i))
            weights = F.softmax(weights, dim=1)
            combined = torch.mul(base, weights[:, 0].view(-1, 1))
            for j in range(1, i + 1):
                combined = combined + torch.mul(feat_list[self.start + j], weights[:, j].view(-1, 1))
        return combined

    def aggregate_rows(self, feat_list, idx):
        """aggregate([f[idx] for f in feat_list]), the reference's mini-batch step (BaseSGModel.forward), with
        aggregate's type checks.  With `fused` set, start == 0, float32 2-d hop tensors held on a HIP device, none
        requiring grad, and idx a 1-d integer tensor, the kernels read the rows idx names from the panels
        themselves (srgnn.hop_attention.hop_attention_recursive(..., index=idx)): no
        [len(idx), d] copy per hop.  Everything else is exactly the two reference lines."""
        if not isinstance(feat_list, list):
            return TypeError("The input must be a list consists of feature matrices!")
        for feat in feat_list:
            if not isinstance(feat, torch.Tensor):
                raise TypeError("The feature matrices must be tensors!")
        if (self.fused and self.start == 0 and len(feat_list) > 0 and _is_row_index(idx)
                and all(f.is_cuda and f.dim() == 2 and f.dtype == torch.float32 and not f.requires_grad
                        for f in feat_list)):
            from srgnn.hop_attention import hop_attention_recursive
            return hop_attention_recursive(feat_list, self.end, self.learnable_weight.weight,
                                           self.learnable_weight.bias, index=idx)
        return self.aggregate([f[idx] for f in feat_list])


def _is_row_index(idx):
    """A 1-d integer tensor: the index the device path takes (a mask or a slice selects rows another way)."""
    return (isinstance(idx, torch.Tensor) and idx.dim() == 1 and idx.dtype != torch.bool
            and not idx.dtype.is_floating_point and not idx.dtype.is_complex)
