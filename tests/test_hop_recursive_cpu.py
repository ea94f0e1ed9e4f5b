"""The fused recursive hop attention's yardstick, without a device: the fp64 restatement and its bound
(tests/hop_recursive_ref.py) against the reference's own fp32 results (tests/golden/hop_recursive.npz), the
negative controls that show the bound is tight enough to catch a wrong formula, and the operator's `fused`
switch on the CPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_cases as G
import hop_recursive_ref as R

DEEP = [n for n, c in R.CASES.items() if c["end"] >= 3]


@pytest.fixture(scope="module")
def golden():
    return np.load(f"{G.GOLDEN}/hop_recursive.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def exact(golden):
    """evaluate() of every fixture, computed once."""
    res = {}
    for name in R.CASES:
        c, hops, w, b, C, *_ = R.load_case(golden, name)
        res[name] = R.evaluate(hops, c["end"], w, b, G=C)
    return res


def test_the_fixtures_are_the_cases_of_the_issue():
    got = {(c["end"], c["T"], c["n"], c["d"]) for c in R.CASES.values()}
    assert got == {(4, 4, 37, 12), (11, 11, 33, 128), (3, 5, 50, 7), (5, 5, 129, 1), (2, 2, 40, 130), (1, 1, 20, 9),
                   (3, 3, 1, 5)}


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_results_lie_within_the_bound(golden, exact, name):
    """The reference's torch CPU out, weight.grad and bias.grad against the restatement: if these missed, the
    formula or the bound would be wrong.  (The reference combines, then takes the dot product; the bound
    covers that order and the device's.)"""
    c, hops, w, b, C, out, dw, db = R.load_case(golden, name)
    assert len(hops) == c["T"] and hops[0].shape == (c["n"], c["d"]) and w.shape == (1, 2 * c["d"])
    R.check(f"reference {name}", out, dw, db, exact[name])


def _leaves_the_bound(ref, wrong):
    return max(R.worst_ratio(wrong["out"], ref["out"], ref["E_out"]), R.worst_ratio(wrong["dw"], ref["dw"], ref["E_dw"]),
               R.worst_ratio(wrong["db"], ref["db"], ref["E_db"]))


@pytest.mark.parametrize("name", DEEP)
def test_negative_controls_leave_the_bound(golden, exact, name):
    """A mistaken formula, evaluated exactly, is outside the bound in at least one element of out or of a
    gradient: one plain softmax over the raw gates, the weight's halves swapped, a backward without
    g (1 - g), a backward that treats the running combination as a constant."""
    c, hops, w, b, C, *_ = R.load_case(golden, name)
    ref = exact[name]
    controls = {"plain softmax": dict(nested=False), "swapped halves": dict(swap_halves=True),
                "no g(1-g)": dict(jacobian=False), "dq dropped": dict(drop_dq=True)}
    for what, kw in controls.items():
        ratio = _leaves_the_bound(ref, R.evaluate(hops, c["end"], w, b, G=C, **kw))
        print(f"{name} {what}: {ratio:.3g} of the bound")
        assert ratio > 1.0, f"{name}: the bound hides `{what}` ({ratio:.3g})"


def test_the_backward_controls_leave_the_forward_alone(golden, exact):
    c, hops, w, b, C, *_ = R.load_case(golden, "rec_t4")
    for kw in (dict(jacobian=False), dict(drop_dq=True)):
        assert np.array_equal(R.evaluate(hops, c["end"], w, b, G=C, **kw)["out"], exact["rec_t4"]["out"])


def test_later_hops_are_ignored(golden, exact):
    c, hops, w, b, C, *_ = R.load_case(golden, "rec_end3of5")
    other = hops[:3] + [h + 1.0 for h in hops[3:]]
    again = R.evaluate(other, 3, w, b, G=C)
    for k in ("out", "dw", "db"):
        assert np.array_equal(again[k], exact["rec_end3of5"][k])


def test_single_hop_is_the_hop_itself(golden, exact):
    c, hops, w, b, C, out, dw, db = R.load_case(golden, "rec_h1")
    assert np.array_equal(out.view(np.uint32), hops[0].view(np.uint32))
    assert not dw.any() and not db.any()
    ref = exact["rec_h1"]
    assert np.array_equal(ref["out"], hops[0].astype(np.float64)) and not ref["dw"].any() and ref["db"] == 0.0
    assert not ref["E_dw"].any() and ref["E_db"] == 0.0


def test_the_weights_are_a_distribution_and_the_work_buffer_is_the_triangle(exact):
    for name, ref in exact.items():
        assert np.allclose(ref["P"].sum(axis=1), 1.0, atol=1e-12) and (ref["P"] > 0).all()
        H = R.CASES[name]["end"]
        assert sum(W.shape[0] for W in ref["Ws"]) + H == R.work_floats(H)
    assert R.work_floats(32) == 32 * 33 // 2 + 32


def _op(start, end, d, fused, w=None, b=None):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    op = IterateLearnableWeightedMessageOp(start, end, "recursive", d)
    assert op.fused is False
    op.fused = fused
    if w is not None:
        with torch.no_grad():
            op.learnable_weight.weight.copy_(torch.from_numpy(w))
            op.learnable_weight.bias.copy_(torch.from_numpy(b))
    return op


@pytest.mark.parametrize("name", list(R.CASES))
def test_fused_switch_on_the_cpu_is_todays_code(golden, name):
    """`fused` defaults to False; with it set, CPU hop tensors take the same composition: the same bits,
    forward and backward, and the fixture's own bits (the same code the reference ran)."""
    c, hops, w, b, C, out, dw, db = R.load_case(golden, name)
    got = []
    for fused in (False, True):
        op = _op(0, c["end"], c["d"], fused, w, b)
        o = op.aggregate([torch.from_numpy(h) for h in hops])
        assert type(o.grad_fn).__name__ != "_HopAttentionRecursiveBackward"
        (o * torch.from_numpy(C)).sum().backward()
        got.append((o.detach().numpy(), op.learnable_weight.weight.grad.numpy(), op.learnable_weight.bias.grad.numpy()))
    for x, y in zip(*got):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(got[1][0].view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("start", [1, 2])
def test_a_later_start_raises_as_the_reference_does(golden, start, fused):
    c, hops, w, b, *_ = R.load_case(golden, "rec_t4")
    op = _op(start, 4, c["d"], fused, w, b)
    with pytest.raises(IndexError):
        op.aggregate([torch.from_numpy(h) for h in hops])


def test_hop_attention_recursive_refuses_host_tensors(golden):
    from srgnn.hop_attention import hop_attention_recursive
    c, hops, w, b, *_ = R.load_case(golden, "rec_t4")
    with pytest.raises(ValueError, match="not on a HIP device"):
        hop_attention_recursive([torch.from_numpy(h) for h in hops], 4, torch.from_numpy(w), torch.from_numpy(b))


def test_entries_are_declared_exported_and_bound():
    import subprocess
    from srgnn import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_header()).read(), flags=re.S)
    names = {"srg_hop_recur_scores_f32": 10, "srg_hop_recur_attend_f32": 14, "srg_hop_recur_attend_grad_f32": 13,
             "srg_hop_recur_scores_grad_scratch_bytes": 4, "srg_hop_recur_scores_grad_f32": 12}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name, nargs in names.items():
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), f"include/srgnn_hip.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        fn = getattr(_lib.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int


def test_scratch_size_is_a_function_of_the_shape():
    from srgnn import _lib
    nbytes = ctypes.c_int64(-1)
    for n, d, H in ((0, 4, 1), (61, 3, 4), (70001, 16, 3), (200000, 128, 11)):
        _lib.check(_lib.lib().srg_hop_recur_scores_grad_scratch_bytes(n, d, H, ctypes.byref(nbytes)), "scratch")
        rpg = R.rows_per_group(n)
        assert nbytes.value == 4 * ((n + 3) // 4 * 4 + -(-n // rpg) * ((2 * d + 1 + 3) // 4 * 4))
    for bad in ((-1, 4, 1), (8, 0, 1), (8, 4, 0), (8, 4, 33)):
        assert _lib.lib().srg_hop_recur_scores_grad_scratch_bytes(*bad, ctypes.byref(nbytes)) != _lib.SRG_OK


def _header():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srgnn_hip.h")
