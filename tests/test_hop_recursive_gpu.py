"""The fused recursive hop attention on the GPU: srg_hop_recur_scores_f32 / srg_hop_recur_attend_f32 /
srg_hop_recur_attend_grad_f32 / srg_hop_recur_scores_grad_f32 behind srgnn.hop_attention.hop_attention_recursive
and IterateLearnableWeightedMessageOp.fused.  Deterministic, and within the derived rounding bound of the fp64
restatement on the same fp32 inputs (tests/hop_recursive_ref.py); the torch composition on the device is never
the expectation.  Largest |got - exact| / bound observed on an MI355X over this file: out 0.201 (H = 2, n = 65,
d = 4), weight gradient 0.040 and bias gradient 0.017 (the one-node fixture); the reference's own torch CPU
results sit at 0.141, 0.014 and 0.012 on the fixtures.
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_cases as G
import hop_recursive_ref as R

pytestmark = pytest.mark.gpu

FUSED = "_HopAttentionRecursiveBackward"


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _windows(arrays, pad):
    """Device copies of the [n, d] arrays; pad > 0: each a column window at offset 1 (4 bytes) of its own
    [n, d + pad] buffer (filled with 7.5), so rows are neither 8- nor 16-byte aligned for odd strides."""
    out = []
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if pad:
            buf = torch.full((a.shape[0], a.shape[1] + pad), 7.5, dtype=torch.float32, device="cuda")
            buf[:, 1:1 + a.shape[1]] = t
            t = buf[:, 1:1 + a.shape[1]]
        out.append(t)
    return out


def _run_op(hops, end, w, b, C):
    """The operator with fused = True on device tensors: (out, weight.grad, bias.grad) as device tensors."""
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    op = IterateLearnableWeightedMessageOp(0, end, "recursive", hops[0].shape[1]).cuda()
    op.fused = True
    with torch.no_grad():
        op.learnable_weight.weight.copy_(torch.as_tensor(w))
        op.learnable_weight.bias.copy_(torch.as_tensor(b))
    out = op.aggregate(list(hops))
    assert type(out.grad_fn).__name__ == FUSED, "the fused path did not run"
    out.backward(C)
    lin = op.learnable_weight
    assert lin.weight.grad.shape == lin.weight.shape and lin.bias.grad.shape == lin.bias.shape
    return out.detach(), lin.weight.grad, lin.bias.grad


@pytest.fixture(scope="module")
def golden():
    return np.load(f"{G.GOLDEN}/hop_recursive.npz", allow_pickle=False)


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixtures_through_the_fused_operator(golden, name):
    """Every fixture of the reference through op.fused = True: out, weight.grad and bias.grad within the
    bound of the restatement."""
    c, hops, w, b, C, r_out, r_dw, r_db = R.load_case(golden, name)
    ref = R.evaluate(hops, c["end"], w, b, G=C)
    dev = _windows(hops, 0)
    out, dw, db = _run_op(dev, c["end"], w, b, torch.from_numpy(C).cuda())
    R.check(f"fused {name}", out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    if c["end"] == 1:
        assert np.array_equal(_bits(out), hops[0].view(np.uint32))
        assert not dw.any() and not db.any()


def _capi(hops, end, w, b, Gd, ldo_pad):
    """The entries called directly on device tensors: (zp, zq, P, out, dw, db), dzp and the out buffer."""
    from srgnn import _lib
    n, d = hops[0].shape
    T, H = len(hops), end
    ptrs = (ctypes.c_void_p * T)(*[h.data_ptr() for h in hops])
    lds = (ctypes.c_int64 * T)(*[h.stride(0) for h in hops])
    wd, bd = torch.from_numpy(w).cuda().view(-1), torch.from_numpy(b).cuda()
    nan = float("nan")
    zp, zq = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
    dzp, dzq = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
    work = torch.full((R.work_floats(H) * n,), nan, device="cuda")
    P = torch.full((n, H), nan, device="cuda")
    buf = torch.full((n, d + ldo_pad), 7.5, device="cuda")
    out = buf[:, :d]
    dw, db = torch.full((2 * d,), nan, device="cuda"), torch.full((1,), nan, device="cuda")
    nbytes = ctypes.c_int64(-1)
    _lib.check(_lib.lib().srg_hop_recur_scores_grad_scratch_bytes(n, d, H, ctypes.byref(nbytes)), "scratch")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    st = _lib.stream("cuda")
    _lib.call("cuda", "srg_hop_recur_scores_f32", ptrs, lds, T, end, wd.data_ptr(), zp.data_ptr(), zq.data_ptr(), n, d, st)
    _lib.call("cuda", "srg_hop_recur_attend_f32", ptrs, lds, T, end, zp.data_ptr(), zq.data_ptr(), bd.data_ptr(),
              work.data_ptr(), P.data_ptr(), out.data_ptr(), out.stride(0) if n > 1 else d + ldo_pad, n, d, st)
    _lib.call("cuda", "srg_hop_recur_attend_grad_f32", ptrs, lds, T, end, Gd.data_ptr(), Gd.stride(0), zq.data_ptr(),
              work.data_ptr(), dzp.data_ptr(), dzq.data_ptr(), n, d, st)
    _lib.call("cuda", "srg_hop_recur_scores_grad_f32", ptrs, lds, T, end, dzp.data_ptr(), dzq.data_ptr(), dw.data_ptr(),
              db.data_ptr(), scratch.data_ptr(), n, d, st)
    # the bias alone (no weight gradient asked for): the same bits
    db1 = torch.full((1,), nan, device="cuda")
    _lib.call("cuda", "srg_hop_recur_scores_grad_f32", ptrs, lds, T, end, dzp.data_ptr(), dzq.data_ptr(), None,
              db1.data_ptr(), scratch.data_ptr(), n, d, st)
    assert np.array_equal(_bits(db1), _bits(db))
    assert not bool(torch.isnan(work).any()), "the work buffer has unwritten slots"
    return (zp, zq, P, out, dw, db), dzp, buf


def _check_entries(what, got, dzp, ref, n, H):
    zp, zq, P, out, dw, db = got
    assert R.worst_ratio(zp.cpu().numpy().reshape(H, n), ref["zp"], ref["E_zp"]) <= 1.0, what + " zp"
    assert R.worst_ratio(zq.cpu().numpy().reshape(H, n), ref["zq"], ref["E_zq"]) <= 1.0, what + " zq"
    assert R.worst_ratio(P.cpu().numpy(), ref["P"], ref["E_P"]) <= 1.0, what + " weights"
    R.check(what, out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    assert not dzp[:n].any(), "dzp of hop 0 is not zero"


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", [1, 3, 6, 64, 65, 257, 1028, 1433])
def test_entries_at_every_width(d, pad):
    """The C entries at n = 61 (no multiple of any rows-per-wave), H = 4 of T = 5: one lane per row up to 64
    lanes with several chunks each, 4-, 8- and 16-byte accesses, rows past one column tile of the parameter
    gradient (d = 1028: 257 chunks; d = 1433: 6 tiles), leading dimensions d and d + 3.  The dot products and
    the weights against their own bounds too; the padding of out stays untouched; twice: the same bits."""
    n, T, end = 61, 5, 4
    hops, w, b, C = R.random_case(n, d, T, 200 + d)
    ref = R.evaluate(hops, end, w, b, G=C)
    dev = [torch.nn.functional.pad(torch.from_numpy(h).cuda(), (0, pad), value=7.5)[:, :d] for h in hops]
    Gd = torch.nn.functional.pad(torch.from_numpy(C).cuda(), (0, pad), value=7.5)[:, :d]
    got, dzp, buf = _capi(dev, end, w, b, Gd, pad)
    _check_entries(f"entries d={d} ld=d+{pad}", got, dzp, ref, n, end)
    assert bool((buf[:, d:] == 7.5).all()), "the attend step wrote past the row's d columns"
    again, _, _ = _capi(dev, end, w, b, Gd, pad)
    for x, y in zip(got, again):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("H,T", [(32, 32), (2, 3), (1, 2)])
def test_wide_triangle_and_edges(H, T):
    """H = 32: the 528-vector triangle, every step of the recurrence; H = 2: one step; H = 1: none."""
    n, d = 65, 4
    hops, w, b, C = R.random_case(n, d, T, 300 + H)
    ref = R.evaluate(hops, H, w, b, G=C)
    dev = _windows(hops, 0)
    Gd = torch.from_numpy(C).cuda()
    got, dzp, _ = _capi(dev, H, w, b, Gd, 0)
    _check_entries(f"H={H}", got, dzp, ref, n, H)
    out, dw, db = _run_op(dev, H, w, b, Gd)
    for x, y in zip(got[3:], (out, dw.view(-1), db)):
        assert np.array_equal(_bits(x), _bits(y)), "the operator and the entries disagree"
    if H == 1:
        assert np.array_equal(_bits(got[3]), hops[0].view(np.uint32)) and bool((got[2] == 1.0).all())
        assert not got[4].any() and not got[5].any()


@pytest.fixture(scope="module")
def large():
    """n = 70,001 (1,094 groups of 64 rows in stage 1), d = 16, H = 3: made and restated once."""
    hops, w, b, C = R.random_case(70001, 16, 3, 7)
    return hops, w, b, C, R.evaluate(hops, 3, w, b, G=C)


@pytest.mark.parametrize("pad", [0, 5])
def test_large_shape_within_bound_and_deterministic(large, pad):
    """pad = 0: contiguous panels, 16-byte accesses.  pad = 5: every hop and G a column window at a 4-byte
    offset of a [n, 21] buffer, the 4-byte path.  Twice: the same bits; the first half of the rows alone: the
    same out bits."""
    hops, w, b, C, ref = large
    dev = _windows(hops, pad)
    Cd = _windows([C], pad)[0]
    out, dw, db = _run_op(dev, 3, w, b, Cd)
    R.check(f"large pad={pad}", out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    out2, dw2, db2 = _run_op(dev, 3, w, b, Cd)
    assert np.array_equal(_bits(out), _bits(out2))
    assert np.array_equal(_bits(dw), _bits(dw2)) and np.array_equal(_bits(db), _bits(db2))
    half = hops[0].shape[0] // 2
    first, _, _ = _run_op([h[:half] for h in dev], 3, w, b, Cd[:half])
    assert np.array_equal(_bits(first), _bits(out[:half]))


def test_peak_memory_at_the_gamlp_shape():
    """H = T = 11, d = 128, n = 20,000: forward plus backward allocate less than 4 n d floats beyond the hop
    list and G (out, the dot products, the triangle, the partials: about 2.1 n d); the composition's peak on
    the same tensors is printed beside it."""
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    n, d, T = 20000, 128, 11
    gen = torch.Generator(device="cuda").manual_seed(5)
    hops = [torch.randn((n, d), device="cuda", generator=gen) for _ in range(T)]
    Gd = torch.randn((n, d), device="cuda", generator=gen)
    w = torch.randn((1, 2 * d), generator=torch.Generator().manual_seed(6)) * 0.05
    _run_op([h[:64] for h in hops], T, w, [0.1], Gd[:64])     # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, dw, db = _run_op(hops, T, w, [0.1], Gd)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dw).all())
    del out, dw, db
    op = IterateLearnableWeightedMessageOp(0, T, "recursive", d).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    op.aggregate(list(hops)).backward(Gd)
    torch.cuda.synchronize()
    comp = torch.cuda.max_memory_allocated() - before
    print(f"peak beyond the hops and G: fused {extra / (n * d * 4):.3f}, composition {comp / (n * d * 4):.3f} n*d*4 bytes")
    assert extra < 4 * n * d * 4


def test_argument_checks_raise_before_any_launch(golden):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    from srgnn.hop_attention import hop_attention_recursive
    c, hops, w, b, *_ = R.load_case(golden, "rec_t4")
    dev = _windows(hops, 0)
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
    with pytest.raises(ValueError, match="requires grad"):
        hop_attention_recursive(dev[:2] + [dev[2].clone().requires_grad_()] + dev[3:], 4, wd, bd)
    with pytest.raises(TypeError, match="float32"):
        hop_attention_recursive(dev[:3] + [dev[3].double()], 4, wd, bd)
    with pytest.raises(ValueError, match="at most 32"):
        hop_attention_recursive([dev[0]] * 33, 33, wd, bd)
    with pytest.raises(ValueError, match="needs a weight of"):
        hop_attention_recursive(dev, 4, wd[:, :12], bd)
    with pytest.raises(ValueError, match="hop slice"):
        hop_attention_recursive(dev, 5, wd, bd)                     # end past the list
    with pytest.raises(ValueError, match="hop slice"):
        hop_attention_recursive(dev, 0, wd, bd)                     # no hop
    with pytest.raises(ValueError, match="hop 1 is"):
        hop_attention_recursive([dev[0], dev[1][:, :6]] + dev[2:], 4, wd, bd)
    with pytest.raises(TypeError, match="weight is"):
        hop_attention_recursive(dev, 4, wd.detach().double(), bd)
    # through the operator: a hop that requires grad or is not float32 takes the composition
    op = IterateLearnableWeightedMessageOp(0, 4, "recursive", 12).cuda()
    op.fused = True
    out = op.aggregate(dev[:3] + [dev[3].clone().requires_grad_()])
    assert type(out.grad_fn).__name__ != FUSED
    op64 = IterateLearnableWeightedMessageOp(0, 4, "recursive", 12).cuda().double()
    op64.fused = True
    assert type(op64.aggregate([h.double() for h in dev]).grad_fn).__name__ != FUSED
    # a later start raises as the reference does
    late = IterateLearnableWeightedMessageOp(1, 4, "recursive", 12).cuda()
    late.fused = True
    with pytest.raises(IndexError):
        late.aggregate(dev)
    # only the gradient autograd asks for
    op.learnable_weight.weight.requires_grad_(False)
    op.aggregate(dev).sum().backward()
    assert op.learnable_weight.weight.grad is None and op.learnable_weight.bias.grad is not None


def test_entries_with_no_rows_and_bad_arguments():
    from srgnn import _lib
    st = _lib.stream("cuda")
    one = (ctypes.c_void_p * 1)(None)
    ld = (ctypes.c_int64 * 1)(4)
    _lib.call("cuda", "srg_hop_recur_scores_f32", one, ld, 1, 1, None, None, None, 0, 4, st)
    _lib.call("cuda", "srg_hop_recur_attend_f32", one, ld, 1, 1, None, None, None, None, None, None, 4, 0, 4, st)
    _lib.call("cuda", "srg_hop_recur_attend_grad_f32", one, ld, 1, 1, None, 4, None, None, None, None, 0, 4, st)
    dw, db = torch.ones(8, device="cuda"), torch.ones(1, device="cuda")
    _lib.call("cuda", "srg_hop_recur_scores_grad_f32", one, ld, 1, 1, None, None, dw.data_ptr(), db.data_ptr(), None,
              0, 4, st)
    assert not dw.any() and not db.any()
    x = torch.zeros((8, 4), device="cuda")
    w = torch.zeros(8, device="cuda")
    v, u = torch.zeros(8 * 33, device="cuda"), torch.zeros(8 * 33, device="cuda")
    many = (ctypes.c_void_p * 33)(*[x.data_ptr()] * 33)
    lds = (ctypes.c_int64 * 33)(*[4] * 33)
    bad = [
        (many, lds, 33, 33, w.data_ptr(), v.data_ptr(), u.data_ptr(), 8, 4),      # T and H > 32
        (many, lds, 33, 4, w.data_ptr(), v.data_ptr(), u.data_ptr(), 8, 4),       # T > 32
        (many, lds, 4, 0, w.data_ptr(), v.data_ptr(), u.data_ptr(), 8, 4),        # empty slice
        (many, lds, 4, 5, w.data_ptr(), v.data_ptr(), u.data_ptr(), 8, 4),        # end > T
        (many, lds, 4, 4, w.data_ptr(), v.data_ptr(), u.data_ptr(), 8, 5),        # ld < d
        (many, lds, 4, 4, None, v.data_ptr(), u.data_ptr(), 8, 4),                # no weight
        (many, lds, 4, 4, w.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4),        # zp is zq
    ]
    for args in bad:
        with pytest.raises(_lib.SrgError):
            _lib.call("cuda", "srg_hop_recur_scores_f32", *args, st)
    work = torch.zeros(8 * R.work_floats(4), device="cuda")
    P = torch.zeros((8, 4), device="cuda")
    with pytest.raises(_lib.SrgError):                                              # out is a panel
        _lib.call("cuda", "srg_hop_recur_attend_f32", many, lds, 4, 4, v.data_ptr(), u.data_ptr(), w.data_ptr(),
                  work.data_ptr(), P.data_ptr(), x.data_ptr(), 4, 8, 4, st)
    with pytest.raises(_lib.SrgError):                                              # ldo < d
        _lib.call("cuda", "srg_hop_recur_attend_f32", many, lds, 4, 4, v.data_ptr(), u.data_ptr(), w.data_ptr(),
                  work.data_ptr(), P.data_ptr(), torch.zeros((8, 4), device="cuda").data_ptr(), 3, 8, 4, st)
    with pytest.raises(_lib.SrgError):                                              # dzp is dzq
        _lib.call("cuda", "srg_hop_recur_attend_grad_f32", many, lds, 4, 4, x.data_ptr(), 4, u.data_ptr(),
                  work.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4, st)
