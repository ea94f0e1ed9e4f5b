"""The fused min / max / concat / NAFS message operators, host side: combine_plan's hop slices, the
MIN / MAX update rule against torch's CPU reduction (bitwise), and the NAFS rounding bound against the
repository's CPU OverSmoothDistanceWeightedOp (pinned bit-equal to the reference by test_msgops_cpu.py)
on the inputs of the GPU tests -- the bound is one the reference itself meets."""
import numpy as np
import pytest
import torch

import golden_cases as G
import msgops_fused_ref as R
from srgnn import aggregate as A


class _Msg:
    def __init__(self, aggr, start=None, end=None):
        self.aggr_type, self.start, self.end = aggr, start, end


SLICES = [(None, None), (0, None), (None, 1), (0, 1), (1, None), (1, 3), (2, 4), (0, 4), (-2, None), (None, -1),
          (3, 2), (4, None), (5, 9)]


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("aggr", ["min", "max", "concat"])
def test_combine_plan_slices(aggr, K):
    for start, end in SLICES:
        want = list(range(K + 1))[start:end]
        if not want:
            with pytest.raises(ValueError):
                A.combine_plan(_Msg(aggr, start, end), K + 1)
            continue
        mode, terms, div = A.combine_plan(_Msg(aggr, start, end), K + 1)
        assert mode == aggr and div is None
        assert [k for k, _ in terms] == want


@pytest.mark.parametrize("K", [0, 3])
def test_combine_plan_over_smooth_takes_all_hops(K):
    from operators.message_operator.over_smooth_distance_op import OverSmoothDistanceWeightedOp
    mode, terms, div = A.combine_plan(OverSmoothDistanceWeightedOp(), K + 1)
    assert mode == "over_smooth" and div is None
    assert [k for k, _ in terms] == list(range(K + 1))


def test_combine_plan_reads_the_operators_own_attributes():
    from operators.message_operator.concat_message_op import ConcatMessageOp
    from operators.message_operator.max_message_op import SimMaxMessageOp
    from operators.message_operator.min_message_op import SimMinMessageOp
    assert A.combine_plan(SimMinMessageOp(1, 3), 4)[:2] == ("min", [(1, 1.0), (2, 1.0)])
    assert A.combine_plan(SimMaxMessageOp(2, None), 4)[:2] == ("max", [(2, 1.0), (3, 1.0)])
    assert A.combine_plan(ConcatMessageOp(None, None), 2)[:2] == ("concat", [(0, 1.0), (1, 1.0)])


def test_learnable_operators_still_have_no_fused_form():
    for aggr in ("learnable_weighted", "iterate_learnable_weighted", "proj_concat", None):
        with pytest.raises(ValueError):
            A.combine_plan(_Msg(aggr, 0, 4), 4)


@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("T", [1, 2, 4, 7])
def test_select_rule_is_torchs_reduction_bitwise(mode, T):
    panels = R.special_panels(61, 37, T, seed=10 * T + (mode == "max"))
    want = R.torch_select(panels, mode)
    got = R.select_rule(panels, mode)
    assert np.array_equal(R.bits(got), R.bits(want))
    # every pair of special values met in both orders, ties between -0 and +0 and NaNs included
    a, b = np.meshgrid(R.SPECIALS, R.SPECIALS, indexing="ij")
    assert np.array_equal(R.bits(R.select_rule([a, b], mode)), R.bits(R.torch_select([a, b], mode)))


@pytest.mark.parametrize("d", R.NAFS_D + R.NAFS_D_WIDE_VEC)
def test_reference_nafs_meets_the_bound(d):
    from operators.message_operator.over_smooth_distance_op import OverSmoothDistanceWeightedOp
    hops = R.nafs_hops(d)
    out = OverSmoothDistanceWeightedOp().combine([torch.from_numpy(h.copy()) for h in hops]).numpy()
    assert out.dtype == np.float32
    R.check_nafs(out, hops, f"torch cpu d={d}")


def test_golden_nafs_output_meets_the_bound():
    z = np.load(f"{G.GOLDEN}/msgops.npz", allow_pickle=False)
    hops = [z[f"osd__hop{k}"] for k in range(5)]
    R.check_nafs(z["osd__out"], hops, "golden osd")


def test_nafs_exact_weights_are_a_softmax():
    _, w, scale = R.nafs_exact(R.nafs_hops(9))
    assert np.allclose(w.sum(1), 1.0, rtol=0, atol=1e-14) and (w > 0).all()
    assert w.shape == (R.NAFS_N, R.NAFS_T) and (scale >= 0).all()
    # an all-zero hop-0 row makes every similarity 0: uniform weights
    assert np.array_equal(w[3], np.full(R.NAFS_T, 1.0 / R.NAFS_T))
