"""The fused hop attention's yardstick, without a device: the fp64 restatement and its bound
(tests/hop_attention_ref.py) against the reference's own fp32 results (tests/golden/hop_attention.npz), the
negative controls that show the bound is tight enough to catch a wrong formula, and the operator's
`fused` switch on the CPU.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import golden_cases as G
import hop_attention_ref as R

MULTI_HOP = [n for n, c in R.CASES.items() if c["end"] - c["start"] > 1]


@pytest.fixture(scope="module")
def golden():
    return np.load(f"{G.GOLDEN}/hop_attention.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def exact(golden):
    """evaluate() of every fixture, computed once."""
    res = {}
    for name in R.CASES:
        c, hops, w, b, C, *_ = R.load_case(golden, name)
        res[name] = R.evaluate(c["kind"], hops, c["start"], c["end"], w, b, G=C)
    return res


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_results_lie_within_the_bound(golden, exact, name):
    """The reference's torch CPU out, weight.grad and bias.grad against the restatement: if these missed,
    the formula, the pairing or the bound would be wrong."""
    c, hops, w, b, C, out, dw, db = R.load_case(golden, name)
    assert hops[0].shape == (c["n"], c["d"]) and w.shape == (1, R.in_dim(c["kind"], c["T"], c["d"]))
    R.check(f"reference {name}", out, dw, db, exact[name])


def test_single_hop_slice_is_the_hop_itself(golden, exact):
    c, hops, w, b, C, out, dw, db = R.load_case(golden, "gate_h1")
    assert np.array_equal(out, hops[2])
    assert not dw.any() and not db.any()
    ref = exact["gate_h1"]
    assert np.array_equal(ref["out"], hops[2].astype(np.float64)) and not ref["dw"].any() and ref["db"] == 0.0


def _leaves_the_bound(ref, wrong):
    return max(R.worst_ratio(wrong["out"], ref["out"], ref["E_out"]), R.worst_ratio(wrong["dw"], ref["dw"], ref["E_dw"]),
               R.worst_ratio(wrong["db"], ref["db"], ref["E_db"]))


@pytest.mark.parametrize("name", MULTI_HOP)
def test_negative_controls_leave_the_bound(golden, exact, name):
    """A mistaken formula, evaluated exactly, is outside the bound in at least one element of out or of a
    gradient: the other pairing, two swapped hops, a backward without a(1 - a)."""
    c, hops, w, b, C, *_ = R.load_case(golden, name)
    kind, start, end = c["kind"], c["start"], c["end"]
    ref = exact[name]
    controls = {"pairing": R.evaluate(kind, hops, start, end, w, b, G=C, pairing="transpose" if kind != "gate" else "flat"),
                "no a(1-a)": R.evaluate(kind, hops, start, end, w, b, G=C, jacobian=False)}
    controls["swapped hops"] = R.evaluate(kind, hops, start, end, w, b, G=C, swap=(0, 1))
    if c["n"] == 1:
        del controls["pairing"]          # one node: both pairings read the same scores
    for what, wrong in controls.items():
        ratio = _leaves_the_bound(ref, wrong)
        print(f"{name} {what}: {ratio:.3g} of the bound")
        assert ratio > 1.0, f"{name}: the bound hides `{what}` ({ratio:.3g})"


def test_rows_per_group_is_a_function_of_n_alone():
    assert [R.rows_per_group(n) for n in (0, 1, 65536, 65537, 131072, 131073, 200000)] == [32, 32, 32, 64, 64, 128, 128]


@pytest.mark.parametrize("name", list(R.CASES))
def test_fused_switch_on_the_cpu_is_todays_code(golden, name):
    """`fused` defaults to False; with it set, CPU hop tensors take the same composition: the same bits,
    forward and backward, and the fixture's values within the bound (the same code the reference ran)."""
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    c, hops, w, b, C, out, dw, db = R.load_case(golden, name)
    got = []
    for fused in (False, True):
        op = LearnableWeightedMessageOp(c["start"], c["end"], c["kind"], *c["args"])
        assert op.fused is False
        op.fused = fused
        with torch.no_grad():
            op.learnable_weight.weight.copy_(torch.from_numpy(w))
            op.learnable_weight.bias.copy_(torch.from_numpy(b))
        o = op.aggregate([torch.from_numpy(h) for h in hops])
        (o * torch.from_numpy(C)).sum().backward()
        got.append((o.detach().numpy(), op.learnable_weight.weight.grad.numpy(), op.learnable_weight.bias.grad.numpy()))
    for x, y in zip(*got):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(got[1][0].view(np.uint32), out.view(np.uint32))


def test_hop_attention_refuses_host_tensors(golden):
    from srgnn.hop_attention import hop_attention
    c, hops, w, b, *_ = R.load_case(golden, "jk_t4")
    with pytest.raises(ValueError, match="not on a HIP device"):
        hop_attention([torch.from_numpy(h) for h in hops], 0, 4, "jk", torch.from_numpy(w), torch.from_numpy(b))


def test_entries_are_declared_exported_and_bound():
    import subprocess
    from srgnn import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_header()).read(), flags=re.S)
    names = {"srg_hop_scores_f32": 12, "srg_hop_attend_f32": 13, "srg_hop_attend_grad_f32": 15,
             "srg_hop_scores_grad_scratch_bytes": 6, "srg_hop_scores_grad_f32": 13}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, nargs in names.items():
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), f"include/srgnn_hip.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        fn = getattr(_lib.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int


def _header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srgnn_hip.h")
