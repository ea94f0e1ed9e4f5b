"""The row-indexed hop attention without a device: the operators' aggregate_rows on CPU tensors is the
reference's own two lines, aggregate over [f[idx] for f in feat_list], for every combination type and with
`fused` off and on; the Python entry points refuse host tensors with an index as they do without; and the
header, the binding and the built library agree on the eight srg_hop_*_rows_f32 entries.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hop_attention_ref as R
import hop_recursive_ref as RR

N_SRC, D, T = 40, 7, 4
LEARNABLE = {"simple": (T - 1,), "simple_allow_neg": (T - 1,), "gate": (D,), "ori_ref": (D,), "jk": (T - 1, D)}


def _hops():
    return [torch.from_numpy(h) for h in R.random_case("gate", N_SRC, D, T, 0, T, 41)[0]]


def _idx():
    return torch.from_numpy(np.random.default_rng(3).integers(0, N_SRC, 55))


def _make(kind, fused, seed=0):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    torch.manual_seed(seed)
    op = IterateLearnableWeightedMessageOp(0, T, "recursive", D) if kind == "recursive" else \
        LearnableWeightedMessageOp(0, T, kind, *LEARNABLE[kind])
    assert op.fused is False
    op.fused = fused
    return op


def _grads(op):
    return [p.grad.detach().numpy().copy() for p in op.parameters()]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", list(LEARNABLE) + ["recursive"])
def test_aggregate_rows_on_the_cpu_is_aggregate_on_the_indexed_list(kind, fused):
    hops, idx = _hops(), _idx()
    C = torch.from_numpy(np.random.default_rng(5).standard_normal((idx.numel(), D)).astype(np.float32))
    got = []
    for rows in (True, False):
        op = _make(kind, fused)
        o = op.aggregate_rows(list(hops), idx) if rows else op.aggregate([f[idx] for f in hops])
        assert o.shape == (idx.numel(), D) and "HopAttention" not in type(o.grad_fn).__name__
        (o * C).sum().backward()
        got.append([o.detach().numpy()] + _grads(op))
    for x, y in zip(*got):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["jk", "recursive"])
def test_aggregate_rows_makes_aggregates_type_checks(kind, fused):
    hops, idx = _hops(), _idx()
    op = _make(kind, fused)
    with pytest.raises(TypeError, match="must be tensors"):
        op.aggregate_rows(hops[:2] + [hops[2].numpy()] + hops[3:], idx)
    # a non-list is answered as aggregate answers it: the TypeError is returned, not raised
    assert isinstance(op.aggregate(tuple(hops)), TypeError)
    assert isinstance(op.aggregate_rows(tuple(hops), idx), TypeError)


@pytest.mark.parametrize("fused", [False, True])
def test_recursive_with_a_later_start_raises_through_aggregate_rows(fused):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    op = IterateLearnableWeightedMessageOp(1, T, "recursive", D)
    op.fused = fused
    with pytest.raises(IndexError):
        op.aggregate_rows(_hops(), _idx())


def test_an_index_does_not_let_host_tensors_in():
    from srgnn.hop_attention import hop_attention, hop_attention_recursive
    hops, w, b, _ = R.random_case("jk", N_SRC, D, T, 0, T, 43)
    feats = [torch.from_numpy(h) for h in hops]
    with pytest.raises(ValueError, match="not on a HIP device"):
        hop_attention(feats, 0, T, "jk", torch.from_numpy(w), torch.from_numpy(b), index=_idx())
    with pytest.raises(ValueError, match="not on a HIP device"):
        hop_attention(feats, 0, T, "jk", torch.from_numpy(w), torch.from_numpy(b), index=_idx(), check=False)
    _, wr, br, _ = RR.random_case(N_SRC, D, T, 44)
    with pytest.raises(ValueError, match="not on a HIP device"):
        hop_attention_recursive(feats, T, torch.from_numpy(wr), torch.from_numpy(br), index=_idx())


def test_entries_are_declared_exported_and_bound():
    import subprocess
    from srgnn import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_header()).read(), flags=re.S)
    bases = ("srg_hop_scores_f32", "srg_hop_attend_f32", "srg_hop_attend_grad_f32", "srg_hop_scores_grad_f32",
             "srg_hop_recur_scores_f32", "srg_hop_recur_attend_f32", "srg_hop_recur_attend_grad_f32",
             "srg_hop_recur_scores_grad_f32")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for base in bases:
        name = base.replace("_f32", "_rows_f32")
        m = re.search(rf"^int\s+{name}\s*\((.*?)\)\s*;", text, flags=re.M | re.S)
        assert m, f"include/srgnn_hip.h does not declare {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        mb = re.search(rf"^int\s+{base}\s*\((.*?)\)\s*;", text, flags=re.M | re.S)
        base_params = [" ".join(p.split()) for p in mb.group(1).split(",")]
        # the base entry's arguments with (rows, n_src) directly after ldp
        assert params == base_params[:2] + ["const int64_t* rows", "int64_t n_src"] + base_params[2:], name
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        fn, fb = getattr(_lib.lib(), name), getattr(_lib.lib(), base)
        assert list(fn.argtypes) == list(fb.argtypes[:2]) + [ctypes.c_void_p, ctypes.c_int64] + list(fb.argtypes[2:])
        assert fn.restype is ctypes.c_int


def _header():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srgnn_hip.h")
