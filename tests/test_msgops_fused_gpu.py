"""The fused min / max / concat / NAFS message operators on the GPU.

min, max and concat: bit-identical (uint32 views: signs of zero and NaNs count) to the reference's
torch CPU combine on the same hops.  NAFS: deterministic -- the same bits on every call and under
every column blocking -- and within the derived rounding bound of the fp64 evaluation of the formula
on the same fp32 hops (tests/msgops_fused_ref.py).  Largest |got - exact| / bound observed on an
MI355X over this file: 0.113 (rand_d1_r05, K = 3; 0.101 at the kernel level, d = 1), falling with d to
0.001 at d = 1433; the reference's own torch CPU result sits at 0.05 on the d = 1..9 inputs.
"""
import numpy as np
import pytest
import torch

import golden_cases as G
import msgops_fused_ref as R

pytestmark = pytest.mark.gpu


class _Msg:
    def __init__(self, aggr, start=None, end=None):
        self.aggr_type, self.start, self.end = aggr, start, end


def _padded(a, pad, fill=7.5):
    """A device panel holding `a` in the first columns of a [n, d + pad] buffer (ld = d + pad)."""
    n, d = a.shape
    buf = torch.full((n, d + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :d] = torch.from_numpy(np.array(a)).cuda()
    return buf, buf[:, :d]


def _bits_equal(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


@pytest.mark.parametrize("d", [1, 7, 64, 130])
def test_accumulate_copy_min_max_bitwise(d):
    """srg_hop_accumulate_f32 COPY / MIN / MAX on special-value panels, lda = d + 3: the reference's
    torch.stack(...).min / max(dim=0)[0], bit for bit; the padding columns stay untouched."""
    from srgnn import _lib
    from srgnn.aggregate import _accumulate
    n, T = 61, 4
    panels = R.special_panels(n, d, T, seed=d)
    dev = [_padded(p, 3)[1] for p in panels]
    for mode, acc_mode in (("min", _lib.SRG_ACC_MIN), ("max", _lib.SRG_ACC_MAX)):
        buf, agg = _padded(np.full((n, d), np.nan, dtype=np.float32), 3)
        _accumulate(agg, dev[0], 123.0, _lib.SRG_ACC_COPY)
        assert _bits_equal(agg.cpu().numpy(), panels[0])
        for y in dev[1:]:
            _accumulate(agg, y, -5.0, acc_mode)
        assert _bits_equal(agg.cpu().numpy(), R.torch_select(panels, mode)), mode
        assert bool((buf[:, d:] == 7.5).all())
    _lib.call("cuda", "srg_hop_accumulate_f32", None, d, None, d, 0, d, 1.0, _lib.SRG_ACC_MIN, _lib.stream("cuda"))
    with pytest.raises(_lib.SrgError):
        _lib.call("cuda", "srg_hop_accumulate_f32", dev[0].data_ptr(), d + 3, None, d + 3, n, d, 1.0,
                  _lib.SRG_ACC_COPY, _lib.stream("cuda"))
    with pytest.raises(_lib.SrgError):
        _lib.call("cuda", "srg_hop_accumulate_f32", dev[0].data_ptr(), d + 3, dev[1].data_ptr(), d + 3, n, d, 1.0,
                  6, _lib.stream("cuda"))


def _nafs_steps(hops, pad):
    """The NAFS steps through the C-ABI on device copies of `hops` (ld = d + pad): (out, weights)."""
    from srgnn import _lib
    n, d = hops[0].shape
    T = len(hops)
    dev = [_padded(h, pad)[1] if pad else torch.from_numpy(np.array(h)).cuda() for h in hops]
    accbuf, acc = _padded(np.full((n, d), np.nan, dtype=np.float32), pad)
    n0 = torch.full((n,), float("nan"), device="cuda")
    z = torch.full((n,), float("nan"), device="cuda")
    E = torch.full((n, T), float("nan"), device="cuda")
    st = _lib.stream("cuda")
    for k, y in enumerate(dev):
        flags = (_lib.SRG_SIM_INIT | _lib.SRG_SIM_HOP0) if k == 0 else 0
        _lib.call("cuda", "srg_hop_simweight_f32", None if k == 0 else dev[0].data_ptr(), dev[0].stride(0),
                  y.data_ptr(), y.stride(0), n0.data_ptr(), acc.data_ptr(), acc.stride(0), z.data_ptr(),
                  E[:, k].data_ptr(), E.stride(0), n, d, flags, st)
    w = (E.double() / z.double()[:, None]).cpu().numpy()
    want_n0 = np.sqrt((hops[0].astype(np.float64) ** 2).sum(1)) + np.float64(np.float32(1e-10))
    np.testing.assert_allclose(n0.cpu().numpy(), want_n0, rtol=(d + 4) * R.EPS, atol=0)
    _lib.call("cuda", "srg_row_divide_f32", acc.data_ptr(), acc.stride(0), z.data_ptr(), n, d, st)
    if pad:
        assert bool((accbuf[:, d:] == 7.5).all()), "the step wrote past the row's d columns"
    return acc.cpu().numpy(), w


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", R.NAFS_D + R.NAFS_D_WIDE_VEC)
def test_nafs_step_kernel_within_bound(d, pad):
    """srg_hop_simweight_f32 + srg_row_divide_f32 over 5 correlated hops, n = 61 (no multiple of any
    rows-per-wave), contiguous (16- / 8- / 4-byte accesses by d) and ld = d + 3 (unaligned rows: 4-byte),
    rows within and past the register cut, all-zero rows in hop 0 and in a later hop."""
    hops = R.nafs_hops(d)
    out, w = _nafs_steps(hops, pad)
    R.check_nafs(out, hops, f"step kernel d={d} ld=d+{pad}")
    _, w_exact, _ = R.nafs_exact(hops)
    werr = float(np.abs(w - w_exact).max())
    print(f"nafs weights d={d} ld=d+{pad}: max |w - exact| = {werr:.3e}, bound {R.weight_bound(d, len(hops)):.3e}")
    assert werr <= R.weight_bound(d, len(hops))
    again, _ = _nafs_steps(hops, pad)
    assert _bits_equal(again, out)


def test_nafs_step_row_bits_do_not_depend_on_the_launch():
    """A row's result is the same bits alone, among 61 rows and among 5000 (another grid, other waves)."""
    d = 128
    hops = R.nafs_hops(d)
    base, _ = _nafs_steps(hops, 0)
    big = [np.tile(h, (82, 1))[:5000] for h in hops]
    out, _ = _nafs_steps(big, 0)
    assert _bits_equal(out, np.tile(base, (82, 1))[:5000])
    one, _ = _nafs_steps([h[7:8] for h in hops], 0)
    assert _bits_equal(one, base[7:8])


def test_nafs_step_argument_checks():
    from srgnn import _lib
    st = _lib.stream("cuda")
    _lib.call("cuda", "srg_hop_simweight_f32", None, 4, None, 4, None, None, 4, None, None, 0, 0, 4,
              _lib.SRG_SIM_INIT | _lib.SRG_SIM_HOP0, st)                 # n = 0: ok, nothing launched
    _lib.call("cuda", "srg_row_divide_f32", None, 4, None, 0, 4, st)
    x = torch.zeros((8, 4), device="cuda")
    acc, v = torch.zeros((8, 4), device="cuda"), torch.zeros(8, device="cuda")
    bad = [
        (None, 4, x.data_ptr(), 4, v.data_ptr(), acc.data_ptr(), 4, v.data_ptr(), None, 0, 8, 4, 0),         # no x0
        (x.data_ptr(), 4, x.data_ptr(), 4, v.data_ptr(), x.data_ptr(), 4, v.data_ptr(), None, 0, 8, 4, 0),   # acc is y
        (x.data_ptr(), 4, x.data_ptr(), 3, v.data_ptr(), acc.data_ptr(), 4, v.data_ptr(), None, 0, 8, 4, 0),  # ldy < d
        (x.data_ptr(), 4, x.data_ptr(), 4, None, acc.data_ptr(), 4, v.data_ptr(), None, 0, 8, 4, 0),         # no n0
        (x.data_ptr(), 4, x.data_ptr(), 4, v.data_ptr(), acc.data_ptr(), 4, v.data_ptr(), None, 0, 8, 4, 4),  # flags
    ]
    for args in bad:
        with pytest.raises(_lib.SrgError):
            _lib.call("cuda", "srg_hop_simweight_f32", *args, st)


def test_combine_device_golden_osd():
    """combine_device on the reference's own NAFS fixture (5 hops, n = 60, d = 9) against the output
    the reference computed from them, within the bound."""
    from operators.message_operator.over_smooth_distance_op import OverSmoothDistanceWeightedOp
    from srgnn.aggregate import combine_device
    z = np.load(f"{G.GOLDEN}/msgops.npz", allow_pickle=False)
    hops = [z[f"osd__hop{k}"] for k in range(5)]
    got = combine_device(OverSmoothDistanceWeightedOp(), [torch.from_numpy(h).cuda() for h in hops]).cpu().numpy()
    R.check_nafs(got, hops, "combine_device golden osd vs exact")
    R.check_nafs(got, hops, "combine_device golden osd vs reference output", against=z["osd__out"])


def test_combine_device_every_operator():
    """combine_device on held device panels == the operators' own CPU combine: bitwise for the
    selecting and the linear operators (their existing steps), the bound for NAFS."""
    from operators.message_operator.concat_message_op import ConcatMessageOp
    from operators.message_operator.last_message_op import LastMessageOp
    from operators.message_operator.max_message_op import SimMaxMessageOp
    from operators.message_operator.mean_message_op import MeanMessageOp
    from operators.message_operator.min_message_op import SimMinMessageOp
    from operators.message_operator.simple_weighted_message_op import SimpleWeightedMessageOp
    from operators.message_operator.sum_message_op import SumMessageOp
    from srgnn.aggregate import combine_device
    hops = R.nafs_hops(65)
    host = [torch.from_numpy(h.copy()) for h in hops]
    dev = [h.cuda() for h in host]
    for op in (LastMessageOp(), SumMessageOp(0, 5), MeanMessageOp(1, 5), SimpleWeightedMessageOp(0, 5, "alpha", 0.15),
               SimMinMessageOp(1, 4), SimMaxMessageOp(0, 5), ConcatMessageOp(1, None)):
        got = combine_device(op, dev).cpu().numpy()
        assert _bits_equal(got, op.aggregate(host).numpy()), op.aggr_type
    sp = R.special_panels(61, 65, 4, seed=2)
    for mode, op in (("min", SimMinMessageOp(0, 4)), ("max", SimMaxMessageOp(0, 4))):
        got = combine_device(op, [torch.from_numpy(p).cuda() for p in sp]).cpu().numpy()
        assert _bits_equal(got, R.torch_select(sp, mode)), mode
    got = combine_device(ConcatMessageOp(0, 4), [torch.from_numpy(p).cuda() for p in sp]).cpu().numpy()
    assert _bits_equal(got, np.hstack(sp))
    with pytest.raises(ValueError):
        combine_device(SimMinMessageOp(4, 2), dev)
    with pytest.raises(ValueError):
        combine_device(_Msg("learnable_weighted"), dev)
    with pytest.raises(ValueError):
        combine_device(SumMessageOp(0, 5), dev[:2] + [dev[2][:, :3]])


@pytest.mark.parametrize("n,d", R.LONG_SHAPES)
@pytest.mark.parametrize("T", R.LONG_T)
def test_combine_device_long_hop_lists(oracle_mod, n, d, T):
    """The weighted sum over 64 to 1,027 held panels: k_tail_rowsum's 16-row block loop (T >= 64) and its
    second level (T >= 1024), the ("fold", 2, 1) steps (T >= 256).  Three cases: hand-crafted weights on
    O(1) panels; alpha = 0.15, whose weights are subnormal from term 526 on and zero from 629 on (the order
    alone: terms 0 .. 525 swamp those products); and the hand-crafted weights on panels scaled by 2^-135,
    where every product and sum is an fp32 subnormal -- that one holds k_hop_accumulate, k_tail_record and
    k_tail_rowsum to unflushed arithmetic (flushed products change every element of the expected result:
    test_aggregate_cpu.py::test_long_hop_lists_bit_exact).  Against oracle.combine (the reference's own
    torch CPU operation), bit for bit; the planned order alone equals it on the CPU (the same test)."""
    from operators.message_operator.simple_weighted_message_op import SimpleWeightedMessageOp
    from srgnn.aggregate import combine_device, tail_range
    w = torch.from_numpy(R.long_weights(T))
    crafted, kw = SimpleWeightedMessageOp(0, T, "hand_crafted", w), dict(weight_list=w)
    plain, sub = R.long_hops(n, d, T), R.long_hops_subnormal(n, d, T)
    for what, hops, op, kw in (("hand_crafted", plain, crafted, kw),
                               ("alpha", plain, SimpleWeightedMessageOp(0, T, "alpha", R.LONG_ALPHA), dict(alpha=R.LONG_ALPHA)),
                               ("subnormal panels", sub, crafted, kw)):
        want = oracle_mod.combine("simple_weighted", [torch.from_numpy(h) for h in hops], 0, T, **kw).numpy()
        got = combine_device(op, list(torch.from_numpy(hops).cuda())).cpu().numpy()
        diff = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
        assert diff.size == 0, (f"{n}x{d} T={T} {what}: {diff.size} elements differ, first flat element {diff[0]} "
                                f"(the tail starts at {tail_range(n, d)[0]}): got {got.ravel()[diff[0]]!r}, "
                                f"want {want.ravel()[diff[0]]!r}")


def _select_ops(K):
    ops = [_Msg("min", 0, K + 1), _Msg("min", 1, K), _Msg("max", 0, K + 1), _Msg("max", 2, None),
           _Msg("concat", 0, K + 1), _Msg("concat", 1, K + 1), _Msg("concat", None, None)]
    return [m for m in ops if list(range(K + 1))[m.start:m.end]]


def _expected_select(msg, hops):
    part = hops[msg.start:msg.end]
    if msg.aggr_type == "concat":
        return torch.hstack([torch.from_numpy(h) for h in part]).numpy()
    return R.torch_select(part, msg.aggr_type)


@pytest.mark.parametrize("K", [0, 3, 10])
@pytest.mark.parametrize("name", ["cora_sym_k3", "rand_d1_r05", "rand_d130_r1", "rand_d1433_r05"])
def test_fused_combine_new_operators(oracle_mod, name, K):
    """fused_combine end to end on the oracle's hops (the reference's, pinned by the golden fixtures):
    min / max / concat bitwise against torch CPU, NAFS within the bound; every operator again with
    col_blocks = 2, and NAFS twice, bitwise equal to the first result."""
    from srgnn.aggregate import fused_combine
    from srgnn.csr import DeviceCSR
    c = G.Case(name)
    ip, ix, v = c.ahat()
    x = c.x()
    hops = oracle_mod.propagate(ip, ix, v, x, K)
    A = DeviceCSR.from_tensors(ip, ix, v, n_cols=c.n, device="cuda")
    X = torch.from_numpy(x).cuda()
    for msg in _select_ops(K):
        what = f"{name} K={K} {msg.aggr_type} {msg.start}:{msg.end}"
        got = fused_combine(A, X, K, msg).cpu().numpy()
        want = _expected_select(msg, hops)
        assert got.shape == want.shape, what
        assert _bits_equal(got, want), what
        assert _bits_equal(fused_combine(A, X, K, msg, col_blocks=2).cpu().numpy(), got), what + " col_blocks=2"
    nafs = _Msg("over_smooth_dis_weighted")
    got = fused_combine(A, X, K, nafs).cpu().numpy()
    R.check_nafs(got, hops, f"fused_combine {name} K={K}")
    assert _bits_equal(fused_combine(A, X, K, nafs).cpu().numpy(), got)
    assert _bits_equal(fused_combine(A, X, K, nafs, col_blocks=2).cpu().numpy(), got)


@pytest.mark.parametrize("to_host", [True, False])
def test_graphop_propagate_aggregate_new_operators(to_host):
    """operators API: GraphOp.propagate_aggregate(adj, x, op) against op.aggregate(GraphOp.propagate(adj, x))."""
    from operators.graph_operator.symmetrical_simgraph_laplacian_operator import SymLaplacianGraphOp
    from operators.message_operator.concat_message_op import ConcatMessageOp
    from operators.message_operator.max_message_op import SimMaxMessageOp
    from operators.message_operator.min_message_op import SimMinMessageOp
    from operators.message_operator.over_smooth_distance_op import OverSmoothDistanceWeightedOp
    c = G.Case("cora_sym_k3")
    x = c.x()
    gop = SymLaplacianGraphOp(3, r=0.5)
    feats = gop.propagate(c.adj(), x)
    for op in (SimMinMessageOp(0, 4), SimMaxMessageOp(1, None), ConcatMessageOp(0, 4), ConcatMessageOp(2, 4)):
        got = gop.propagate_aggregate(c.adj(), x, op, to_host=to_host)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.is_cuda == (not to_host)
        assert torch.equal(got.cpu(), op.aggregate(feats)), op.aggr_type
    got = gop.propagate_aggregate(c.adj(), x, OverSmoothDistanceWeightedOp(), to_host=to_host)
    assert got.is_cuda == (not to_host)
    hops = [f.numpy() for f in feats]
    R.check_nafs(got.cpu().numpy(), hops, f"propagate_aggregate cora to_host={to_host}")
    R.check_nafs(OverSmoothDistanceWeightedOp().aggregate(feats).numpy(), hops, "cpu operator cora")
