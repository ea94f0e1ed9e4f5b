"""LearnableWeightedMessageOp (SSRG/operators/message_operator/learnable_weighted_messahe_op.py:10-103,
the file name's spelling kept): GAMLP's learnable hop combination.  Consumes the hop list on whatever
device the model keeps it; same parameters (created in the reference's order, so a seeded run draws
the same initial values), same forward arithmetic.

    simple / simple_allow_neg  (prop_steps)           one weight per hop, softmax(sigmoid(w)) or w itself
    gate                       (feat_dim)             per-node weights from Linear(feat_dim, 1) on each hop
    ori_ref                    (feat_dim)             ... on [hop 0 | hop]
    jk                         (prop_steps, feat_dim) ... on [all hops | hop]

`fused` (default False): with it set, gate / ori_ref / jk over hop tensors held on a HIP device, none of
which requires grad, run srgnn.hop_attention (the device kernels of DESIGN.md §5.4.2: the same weights
within a derived rounding bound, gradients for the Linear's weight and bias, none of the composition's
[hops * n, in_dim] temporaries).  Everything else takes the composition below, unchanged.

aggregate_rows(feat_list, idx) is the mini-batch step of the reference's training loop, aggregate over
[f[idx] for f in feat_list]; under `fused` it reads the batch's rows from the device panels in place.
"""
import torch
import torch.nn.functional as F
from torch import nn

from operators.base_operator import MessageOp
from operators.utils import one_dim_weighted_add, squeeze_first_dimension, two_dim_weighted_add

_ARITY = {"simple": 1, "simple_allow_neg": 1, "gate": 1, "ori_ref": 1, "jk": 2}


class LearnableWeightedMessageOp(MessageOp):
    def __init__(self, start, end, combination_type, *args):
        super(LearnableWeightedMessageOp, self).__init__(start, end)
        self.aggr_type = "learnable_weighted"
        if combination_type not in _ARITY:
            raise ValueError(
                "Invalid weighted combination type! Type must be 'simple', 'simple_allow_neg', 'gate', 'ori_ref' or 'jk'.")
        self.combination_type = combination_type
        self.learnable_weight = None
        if len(args) != _ARITY[combination_type]:
            kind = "simple" if combination_type == "simple_allow_neg" else combination_type
            raise ValueError(f"Invalid parameter numbers for the {kind} learnable weighted aggregator!")
        if combination_type in ("simple", "simple_allow_neg"):
            # xavier_normal_ needs a 2-d tensor: draw [1, K+1], keep it flat
            w = torch.FloatTensor(1, args[0] + 1)
            nn.init.xavier_normal_(w)
            self.learnable_weight = nn.Parameter(w.view(-1))
        else:
            in_dim = {"gate": args[0], "ori_ref": 2 * args[0]}.get(combination_type)
            if combination_type == "jk":
                in_dim = args[1] + (args[0] + 1) * args[1]
            self.learnable_weight = nn.Linear(in_dim, 1)
        self.fused = False

    def _hop_weights(self, feat_list):
        hops = self.end - self.start
        kind = self.combination_type
        if kind == "simple":
            return F.softmax(torch.sigmoid(self.learnable_weight[self.start:self.end]), dim=0)
        if kind == "simple_allow_neg":
            return self.learnable_weight[self.start:self.end]
        stacked = torch.vstack(feat_list[self.start:self.end])
        if kind == "gate":
            scores = self.learnable_weight(stacked).view(hops, -1).T
        else:
            ref = feat_list[0] if kind == "ori_ref" else torch.hstack(feat_list)
            scores = self.learnable_weight(torch.hstack((ref.repeat(hops, 1), stacked))).view(-1, hops)
        return F.softmax(torch.sigmoid(scores), dim=1)

    def combine(self, feat_list):
        feat_list = squeeze_first_dimension(feat_list)
        if (self.fused and self.combination_type in ("gate", "ori_ref", "jk") and isinstance(feat_list, list)
                and all(isinstance(f, torch.Tensor) and f.is_cuda and not f.requires_grad for f in feat_list)):
            from srgnn.hop_attention import hop_attention
            return hop_attention(feat_list, self.start, self.end, self.combination_type,
                                 self.learnable_weight.weight, self.learnable_weight.bias)
        weights = self._hop_weights(feat_list)
        add = one_dim_weighted_add if self.combination_type in ("simple", "simple_allow_neg") else two_dim_weighted_add
        return add(feat_list[self.start:self.end], weight_list=weights)

    def aggregate_rows(self, feat_list, idx):
        """aggregate([f[idx] for f in feat_list]), the reference's mini-batch step (BaseSGModel.forward), with
        aggregate's type checks.  With `fused` set, gate / ori_ref / jk over 2-d hop tensors held on a HIP
        device, none requiring grad, and idx a 1-d integer tensor, the kernels read the rows idx names from the
        panels themselves (srgnn.hop_attention(..., index=idx)): no [len(idx), d] copy per hop.
        Everything else is exactly the two reference lines."""
        if not isinstance(feat_list, list):
            return TypeError("The input must be a list consists of feature matrices!")
        for feat in feat_list:
            if not isinstance(feat, torch.Tensor):
                raise TypeError("The feature matrices must be tensors!")
        if (self.fused and self.combination_type in ("gate", "ori_ref", "jk") and _is_row_index(idx)
                and len(feat_list) > 0 and all(f.is_cuda and f.dim() == 2 and not f.requires_grad for f in feat_list)):
            from srgnn.hop_attention import hop_attention
            return hop_attention(feat_list, self.start, self.end, self.combination_type,
                                 self.learnable_weight.weight, self.learnable_weight.bias, index=idx)
        return self.aggregate([f[idx] for f in feat_list])


def _is_row_index(idx):
    """A 1-d integer tensor: the index the device path takes (a mask or a slice selects rows another way)."""
    return (isinstance(idx, torch.Tensor) and idx.dim() == 1 and idx.dtype != torch.bool
            and not idx.dtype.is_floating_point and not idx.dtype.is_complex)
