"""Golden fixtures for the fused recursive hop attention (GAMLP-R): the REFERENCE's own
IterateLearnableWeightedMessageOp, seeded, on fixed hop lists, forward and autograd (development container only).

    python tests/golden/make_golden_hop_recursive.py

Imports, unmodified, iterate_learnable_weighted_message_op.IterateLearnableWeightedMessageOp from the reference
tree's operators/message_operator (make_golden.py's REF_SSRG) with make_golden.py's import stubs, as
make_golden_hop_attention.py does.  For each case of tests/hop_recursive_ref.py::CASES: torch.manual_seed(seed),
build the op with (0, end, "recursive", d), run aggregate on the stored hop list (T hops: those past `end` are
ignored), then loss = (out * C).sum() with a stored random panel C and backward.
Written to tests/golden/hop_recursive.npz: the parameters, the hops, C, the reference's out and its
weight.grad / bias.grad.  Only data leaves this script.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from hop_recursive_ref import HERE_CASES  # noqa: E402


def main():
    MG.import_reference()
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    rng = np.random.default_rng(92)
    arrs = {}
    for name, T, end, n, d, seed in HERE_CASES:
        feats = [torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)) for _ in range(T)]
        C = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
        torch.manual_seed(seed)
        op = IterateLearnableWeightedMessageOp(0, end, "recursive", d)
        out = op.aggregate(list(feats))
        (out * C).sum().backward()
        lin = op.learnable_weight
        arrs[f"{name}__weight"] = lin.weight.detach().numpy()
        arrs[f"{name}__bias"] = lin.bias.detach().numpy()
        for t, f in enumerate(feats):
            arrs[f"{name}__hop{t}"] = f.numpy()
        arrs[f"{name}__C"] = C.numpy()
        arrs[f"{name}__out"] = out.detach().numpy()
        # one hop: out is the hop itself and nothing reaches the parameters; autograd leaves their .grad unset
        arrs[f"{name}__grad_weight"] = (lin.weight.grad if lin.weight.grad is not None
                                        else torch.zeros_like(lin.weight)).numpy()
        arrs[f"{name}__grad_bias"] = (lin.bias.grad if lin.bias.grad is not None else torch.zeros_like(lin.bias)).numpy()
    path = os.path.join(HERE, "hop_recursive.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", len(HERE_CASES), "recursive hop attention cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
