"""Golden fixtures for the fused learnable hop attention (GAMLP): the REFERENCE's own
LearnableWeightedMessageOp, seeded, on fixed hop lists, forward and autograd (development container only).

    python tests/golden/make_golden_hop_attention.py

Imports, unmodified, learnable_weighted_messahe_op.LearnableWeightedMessageOp from the reference tree's
operators/message_operator (make_golden.py's REF_SSRG) with make_golden.py's import stubs, as
make_golden_msgops.py does.  For each case of tests/hop_attention_ref.py::CASES: torch.manual_seed(seed),
build the op, run aggregate on the stored hop list, then loss = (out * C).sum() with a stored random panel C
and backward.
Written to tests/golden/hop_attention.npz: the parameters, the hops, C, the reference's out and its
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
from hop_attention_ref import HERE_CASES  # noqa: E402


def main():
    MG.import_reference()
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    rng = np.random.default_rng(91)
    arrs = {}
    for name, kind, T, start, end, n, d, args, seed in HERE_CASES:
        feats = [torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)) for _ in range(T)]
        C = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
        torch.manual_seed(seed)
        op = LearnableWeightedMessageOp(start, end, kind, *args)
        out = op.aggregate(list(feats))
        (out * C).sum().backward()
        lin = op.learnable_weight
        arrs[f"{name}__weight"] = lin.weight.detach().numpy()
        arrs[f"{name}__bias"] = lin.bias.detach().numpy()
        for t, f in enumerate(feats):
            arrs[f"{name}__hop{t}"] = f.numpy()
        arrs[f"{name}__C"] = C.numpy()
        arrs[f"{name}__out"] = out.detach().numpy()
        arrs[f"{name}__grad_weight"] = lin.weight.grad.numpy()
        arrs[f"{name}__grad_bias"] = lin.bias.grad.numpy()
    path = os.path.join(HERE, "hop_attention.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", len(HERE_CASES), "hop attention cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
