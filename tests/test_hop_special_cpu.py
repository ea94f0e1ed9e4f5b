"""The hop attention's yardstick at saturated scores and special values, without a device (the cases of
tests/hop_special_cases.py, DESIGN.md §5.4.2 - §5.4.4 "Special values and saturation").

First subject: the shipped torch composition (fused = False, fp32 on the host).  It has to lie inside every bound
the device is later held to -- if the reference's own arithmetic left a bound, the bound would be wrong.  Then
the negative controls: a numpy-fp32 evaluation of the formula with one mistake each, which has to leave it.  And
the rules for special values leave every bound on finite inputs where it was (tests/golden/hop_bounds_before.npz).
"""
import os
import sys

import numpy as np
import pytest
import torch

import golden_cases as G
import hop_attention_ref as R
import hop_recursive_ref as RR
import hop_special_cases as SC

N, T, START, END = 130, 5, 1, 4
CTOR = {"jk": lambda T, d: (T - 1, d), "ori_ref": lambda T, d: (d,), "gate": lambda T, d: (d,)}
LEARNABLE = ("gate", "ori_ref", "jk")


def _composition(case, hops=None, C=None):
    """(out, weight.grad, bias.grad) of the torch composition on the host, as numpy."""
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    kind, d = case["kind"], case["d"]
    if kind == "recursive":
        op = IterateLearnableWeightedMessageOp(0, case["end"], "recursive", d)
    else:
        op = LearnableWeightedMessageOp(case["start"], case["end"], kind, *CTOR[kind](case["T"], d))
    assert op.fused is False
    with torch.no_grad():
        op.learnable_weight.weight.copy_(torch.from_numpy(case["w"]))
        op.learnable_weight.bias.copy_(torch.from_numpy(case["b"]))
    out = op.aggregate([torch.from_numpy(h) for h in (case["hops"] if hops is None else hops)])
    out.backward(torch.from_numpy(case["C"] if C is None else C))
    lin = op.learnable_weight
    return out.detach().numpy(), lin.weight.grad.numpy(), lin.bias.grad.numpy()


def _check(case, what, got, ref):
    return (RR if case["kind"] == "recursive" else R).check(what, *got, ref)


def _ratios(got, ref):
    return tuple(R.worst_ratio(x, ref[k], ref["E_" + k]) for x, k in zip(got, ("out", "dw", "db")))


def test_classes_and_check_special():
    x = np.array([0.0, -0.0, 1e-45, np.nan, np.inf, -np.inf, 3.0], dtype=np.float32)
    assert R.classes(x).tolist() == [0, 0, 0, 1, 2, 3, 0]
    want = np.array([1.0, np.nan, np.inf, -np.inf])
    bound = np.array([0.5, np.nan, np.inf, 0.0])
    assert R.check_special("ok", np.array([1.25, np.nan, np.inf, -np.inf]), want, bound) == 0.5
    for wrong in ([1.75, np.nan, np.inf, -np.inf], [1.0, 0.0, np.inf, -np.inf], [1.0, np.nan, -np.inf, -np.inf],
                  [np.nan, np.nan, np.inf, -np.inf], [1.0, np.nan, np.inf, np.nan]):
        with pytest.raises(AssertionError):
            R.check_special("wrong", np.array(wrong), want, bound)
    with pytest.raises(AssertionError, match="bound is not finite"):
        R.check_special("bound", np.array([1.0]), np.array([1.0]), np.array([np.nan]))
    assert R.underflow_allowance(3) == 3 * 2.0 ** -150 and RR.underflow_allowance is R.underflow_allowance


def test_bounds_on_finite_inputs_are_unchanged():
    """Every bound of every fixture and of seven random cases, as recorded from the restatements before the
    0 * inf = 0 rules went in (tests/golden/make_hop_bounds.py), at relative 1e-12."""
    sys.path.insert(0, G.GOLDEN)
    try:
        import make_hop_bounds
    finally:
        sys.path.remove(G.GOLDEN)
    before = np.load(os.path.join(G.GOLDEN, "hop_bounds_before.npz"), allow_pickle=False)
    now = make_hop_bounds.bounds(R, RR)
    assert sorted(now) == sorted(before.files) and len(now) == 4 * (len(R.CASES) + len(RR.CASES) + 7)
    for key, value in now.items():
        assert value.shape == before[key].shape and np.isfinite(value).all(), key
        assert np.all(np.abs(value - before[key]) <= 1e-12 * before[key]), key


@pytest.mark.parametrize("d", [1, 6, 130])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_composition_at_saturated_scores(kind, d):
    """The builder asserts that every expf regime is reached with both signs; the composition's out, weight.grad
    and bias.grad are finite and inside the unchanged bound."""
    case = SC.saturated(kind, N, d, T, START, END, 40 + d)
    scores = SC.gate_scores(case, SC.exact(case))
    print(f"saturated {kind} d={d}: max |score| {np.abs(scores).max():.0f}, per regime and sign {sorted(case['regimes'].values())}")
    got = _composition(case)
    assert all(np.isfinite(x).all() for x in got)
    _check(case, f"composition saturated {kind} d={d}", got, SC.exact(case))


@pytest.mark.parametrize("d", [1, 6, 130])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_composition_with_planted_non_finite_cells(kind, d):
    """fp32 and fp64 agree in the class of every element of out, weight.grad and bias.grad, the finite part is
    inside its bound and that bound is finite; cells in panels the kind does not read change nothing."""
    case = SC.planted(kind, N, d, T, START, END, 50 + d)
    ref = SC.exact(case)
    got = _composition(case)
    for x, k in zip(got, ("out", "dw", "db")):
        R.check_special(f"composition planted {kind} d={d} {k}", x, ref[k], ref["E_" + k])
    rows = np.unique(np.nonzero(R.classes(ref["out"]))[0])
    print(f"planted {kind} d={d}: non-finite out rows {rows.tolist()}")
    assert {7, 40, 55, 90} <= set(rows.tolist()) and len(rows) < N // 2
    if kind == "recursive":
        # Inf cells of hop 0: s_0 = inf - inf = NaN makes the whole row NaN (the one-column softmax of a NaN gate),
        # s_0 = +-inf leaves W(0) = 1 and only the cell's own column not finite
        assert d == 1 or case["s0_nan_row"] == 100
        if case["s0_nan_row"] is not None:
            assert np.isnan(ref["out"][100]).all() and np.isnan(got[0][100]).all()
        if d > 1:
            assert (R.classes(ref["out"][110]) != 0).sum() == 1
    unread = [c for c in case["cells"] if c[0] not in SC.reads(kind, T, case["start"], END)]
    assert len(unread) == {"gate": 2, "ori_ref": 1, "jk": 0, "recursive": 1}[kind]
    hops = [h.copy() for h in case["hops"]]
    for t, i, c, _ in unread:
        hops[t][i, c] = 1.0
    for x, y in zip(got, _composition(case, hops=hops)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("kind", LEARNABLE)
def test_the_plain_evaluation_is_inside_every_bound(kind):
    """SC.emulate without a mistake: inside the bound on saturated, the same classes on planted, zeros for
    unreadable rows on row0_poison, inside bound + allowance on the subnormal row: what the controls below leave."""
    d = 6
    case = SC.saturated(kind, N, d, T, START, END, 46)
    R.check(f"emulate saturated {kind}", *SC.emulate(kind, case["hops"], START, END, case["w"], case["b"], case["C"]), SC.exact(case))
    case = SC.planted(kind, N, d, T, START, END, 56)
    ref = SC.exact(case)
    for x, k in zip(SC.emulate(kind, case["hops"], START, END, case["w"], case["b"], case["C"]), ("out", "dw", "db")):
        R.check_special(f"emulate planted {kind} {k}", x, ref[k], ref["E_" + k])
    case = SC.row0_poison(kind, 200, d, T, START, END, 66)
    ref = SC.exact(case, idx=case["index"])
    got = SC.emulate(kind, SC.gather(case["hops"], case["index"]), START, END, case["w"], case["b"], case["C"])
    R.check(f"emulate row0_poison {kind}", *got, ref)
    assert not got[0][case["bad"]].any() and not np.signbit(got[0][case["bad"]]).any()
    case = SC.denormal_row(kind, N, d, T, START, END, 76)
    ref = SC.exact(case)
    out, dw, db = SC.emulate(kind, case["hops"], START, END, case["w"], case["b"], case["C"])
    allowed = ref["E_out"] + R.underflow_allowance(END - START)
    assert out[SC.DENORMAL_ROW].all() and R.worst_ratio(out, ref["out"], allowed) <= 1.0
    R.check(f"emulate denormal_row {kind} (gradients)", np.where(np.abs(ref["out"]) < 2.0 ** -120, ref["out"], out), dw, db, ref)
    assert np.signbit(out[SC.NEG_ZERO_ROW]).all() and not out[SC.NEG_ZERO_ROW].any()
    assert not np.signbit(out[SC.POS_ZERO_ROW]).any() and not out[SC.POS_ZERO_ROW].any()


@pytest.mark.parametrize("kind", LEARNABLE)
def test_negative_controls_leave_the_bound(kind):
    """One mistake each, in the numpy-fp32 evaluation; every one of them is seen."""
    d = 6
    args = lambda case: (kind, case["hops"], START, END, case["w"], case["b"], case["C"])  # noqa: E731

    case = SC.saturated(kind, N, d, T, START, END, 46)
    ref = SC.exact(case)
    naive = SC.emulate(*args(case), sigmoid="naive")
    assert not np.isfinite(naive[0]).all(), "expf(s) / (1 + expf(s)) stayed finite"
    with pytest.raises(AssertionError):
        R.check("naive sigmoid", *naive, ref)
    no_jac = _ratios(SC.emulate(*args(case), jacobian=False), ref)
    print(f"saturated {kind}: a backward without a (1 - a) is at {no_jac[1]:.3g} (dw) and {no_jac[2]:.3g} (db) of the bound")
    assert no_jac[1] > 1.0 and no_jac[2] > 1.0

    case = SC.row0_poison(kind, 200, d, T, START, END, 66)
    mult = SC.emulate(kind, SC.gather(case["hops"], case["index"], select=False), START, END, case["w"], case["b"], case["C"])
    assert np.isnan(mult[0][case["bad"]]).all() and np.isnan(mult[1]).all() and np.isnan(mult[2]), "0 * NaN went unseen"

    case = SC.denormal_row(kind, N, d, T, START, END, 76)
    ref = SC.exact(case)
    flushed = SC.emulate(*args(case), flush=True)
    allowed = ref["E_out"] + R.underflow_allowance(END - START)
    ratio = R.worst_ratio(flushed[0][SC.DENORMAL_ROW], ref["out"][SC.DENORMAL_ROW], allowed[SC.DENORMAL_ROW])
    print(f"denormal_row {kind}: flushed subnormals are at {ratio:.3g} of bound + allowance")
    assert ratio > 1.0 and not flushed[0][SC.DENORMAL_ROW].any()


def test_transpose_pairing_moves_the_non_finite_rows_of_jk():
    case = SC.planted("jk", N, 6, T, START, END, 56)
    ref = SC.exact(case)
    wrong = SC.emulate("jk", case["hops"], START, END, case["w"], case["b"], case["C"], pairing="transpose")
    rows = lambda x: set(np.unique(np.nonzero(R.classes(x))[0]).tolist())  # noqa: E731
    print(f"planted jk: non-finite out rows {sorted(rows(ref['out']))}, under the transpose pairing {sorted(rows(wrong[0]))}")
    assert rows(wrong[0]) != rows(ref["out"])
    with pytest.raises(AssertionError, match="another class"):
        R.check_special("transpose pairing", wrong[0], ref["out"], ref["E_out"])


@pytest.mark.parametrize("kind", SC.KINDS)
def test_builders(kind):
    """unread_poison poisons exactly the panels the formula does not read (the restatement, which reads what the
    formula reads, stays finite); row0_poison's index keeps to its description."""
    case = SC.unread_poison(kind, N, 6, T, START, END, 86)
    assert case["unread"] == {"gate": [0, 4], "ori_ref": [4], "jk": [], "recursive": [4]}[kind]
    ref = SC.exact(case)
    assert all(np.isfinite(ref[k]).all() for k in ("out", "dw", "db"))
    case = SC.row0_poison(kind, 200, 6, T, START, END, 66)
    idx = case["index"]
    assert sorted(idx[case["bad"]].tolist()) == [-1, -1, 200, 200, 2 ** 40] and len(set(idx.tolist())) < idx.size - 10
    assert all(np.isnan(h[0]).all() and np.isposinf(h[-1]).all() for h in case["hops"])
    idx = SC.batch_index(200, 3)
    assert set(idx.tolist()) == set(range(200)) and idx.size == 230 and not np.array_equal(idx[:200], np.arange(200))
