"""The fused learnable hop attention on the GPU: srg_hop_scores_f32 / srg_hop_attend_f32 /
srg_hop_attend_grad_f32 / srg_hop_scores_grad_f32 behind srgnn.hop_attention and
LearnableWeightedMessageOp.fused.  Deterministic, and within the derived rounding bound of the fp64
restatement on the same fp32 inputs (tests/hop_attention_ref.py); the torch composition on the device is
never the expectation.  Largest |got - exact| / bound observed on an MI355X over this file: out 0.191 (gate,
n = 70,001), weight gradient 0.0092 and bias gradient 0.0095 (jk, d = 1); the reference's own torch CPU results
sit at 0.118, 0.0095 and 0.0035 on the fixtures.
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_cases as G
import hop_attention_ref as R

pytestmark = pytest.mark.gpu

CTOR = {"jk": lambda T, d: (T - 1, d), "ori_ref": lambda T, d: (d,), "gate": lambda T, d: (d,)}


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


def _run_op(kind, hops, start, end, w, b, C, T=None):
    """The operator with fused = True on device tensors: (out, weight.grad, bias.grad) as device tensors."""
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    T = len(hops) if T is None else T
    op = LearnableWeightedMessageOp(start, end, kind, *CTOR[kind](T, hops[0].shape[1])).cuda()
    op.fused = True
    with torch.no_grad():
        op.learnable_weight.weight.copy_(torch.as_tensor(w))
        op.learnable_weight.bias.copy_(torch.as_tensor(b))
    out = op.aggregate(list(hops))
    assert type(out.grad_fn).__name__ == "_HopAttentionBackward", "the fused path did not run"
    out.backward(C)
    lin = op.learnable_weight
    assert lin.weight.grad.shape == lin.weight.shape and lin.bias.grad.shape == lin.bias.shape
    return out.detach(), lin.weight.grad, lin.bias.grad


@pytest.fixture(scope="module")
def golden():
    return np.load(f"{G.GOLDEN}/hop_attention.npz", allow_pickle=False)


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixtures_through_the_fused_operator(golden, name):
    """Every fixture of the reference through op.fused = True: out, weight.grad and bias.grad within the
    bound of the restatement, the reference's own values within the same bound of it (as on the CPU)."""
    c, hops, w, b, C, r_out, r_dw, r_db = R.load_case(golden, name)
    ref = R.evaluate(c["kind"], hops, c["start"], c["end"], w, b, G=C)
    dev = _windows(hops, 0)
    out, dw, db = _run_op(c["kind"], dev, c["start"], c["end"], w, b, torch.from_numpy(C).cuda())
    R.check(f"fused {name}", out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    R.check(f"reference {name}", r_out, r_dw, r_db, ref)
    if c["end"] - c["start"] == 1:
        assert np.array_equal(_bits(out), hops[c["start"]].view(np.uint32))
        assert not dw.any() and not db.any()


@pytest.fixture(scope="module")
def large():
    """One larger shape per kind, made and restated once: n = 70,001 (1,094 groups of 64 rows in stage 1,
    a pairing that crosses the whole panel), d = 16, T = 3."""
    cases = {}
    for kind, start, end, seed in (("jk", 0, 3, 1), ("ori_ref", 1, 3, 2), ("gate", 0, 3, 3)):
        hops, w, b, C = R.random_case(kind, 70001, 16, 3, start, end, seed)
        cases[kind] = (start, end, hops, w, b, C, R.evaluate(kind, hops, start, end, w, b, G=C))
    return cases


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("kind", ["jk", "ori_ref", "gate"])
def test_large_shape_within_bound_and_deterministic(large, kind, pad):
    """pad = 0: contiguous panels, 16-byte accesses.  pad = 5: every hop and G a column window at a 4-byte
    offset of a [n, 21] buffer, the 4-byte path.  Twice: the same bits."""
    start, end, hops, w, b, C, ref = large[kind]
    dev = _windows(hops, pad)
    Cd = _windows([C], pad)[0]
    out, dw, db = _run_op(kind, dev, start, end, w, b, Cd)
    R.check(f"large {kind} pad={pad}", out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    out2, dw2, db2 = _run_op(kind, dev, start, end, w, b, Cd)
    assert np.array_equal(_bits(out), _bits(out2))
    assert np.array_equal(_bits(dw), _bits(dw2)) and np.array_equal(_bits(db), _bits(db2))
    if kind == "gate":
        half = hops[0].shape[0] // 2
        first, _, _ = _run_op(kind, [h[:half] for h in dev], start, end, w, b, Cd[:half])
        assert np.array_equal(_bits(first), _bits(out[:half]))


def _capi(kind, hops, start, end, w, b, Gd, ldo_pad):
    """The four entries called directly on device tensors: (z, P, out, dw, db) and the out buffer."""
    from srgnn import _lib
    from srgnn.hop_attention import KINDS, _pairing
    n, d = hops[0].shape
    T, H = len(hops), end - start
    ptrs = (ctypes.c_void_p * T)(*[h.data_ptr() for h in hops])
    lds = (ctypes.c_int64 * T)(*[h.stride(0) for h in hops])
    wd, bd = torch.from_numpy(w).cuda().view(-1), torch.from_numpy(b).cuda()
    nan = float("nan")
    z, dz = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
    P, dP = torch.full((n, H), nan, device="cuda"), torch.full((n, H), nan, device="cuda")
    buf = torch.full((n, d + ldo_pad), 7.5, device="cuda")
    out = buf[:, :d]
    dw, db = torch.full((wd.numel(),), nan, device="cuda"), torch.full((1,), nan, device="cuda")
    nbytes = ctypes.c_int64(-1)
    _lib.check(_lib.lib().srg_hop_scores_grad_scratch_bytes(n, d, T, H, KINDS[kind], ctypes.byref(nbytes)), "scratch")
    rpg = R.rows_per_group(n)
    assert nbytes.value == 4 * ((n + 3) // 4 * 4 + -(-n // rpg) * ((wd.numel() + 1 + 3) // 4 * 4))
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    st = _lib.stream("cuda")
    _lib.call("cuda", "srg_hop_scores_f32", ptrs, lds, T, start, end, KINDS[kind], wd.data_ptr(), bd.data_ptr(),
              z.data_ptr(), n, d, st)
    _lib.call("cuda", "srg_hop_attend_f32", ptrs, lds, T, start, end, z.data_ptr(), _pairing(kind), P.data_ptr(),
              out.data_ptr(), out.stride(0), n, d, st)
    _lib.call("cuda", "srg_hop_attend_grad_f32", ptrs, lds, T, start, end, Gd.data_ptr(), Gd.stride(0), z.data_ptr(),
              P.data_ptr(), _pairing(kind), dP.data_ptr(), dz.data_ptr(), n, d, st)
    _lib.call("cuda", "srg_hop_scores_grad_f32", ptrs, lds, T, start, end, KINDS[kind], dz.data_ptr(), dw.data_ptr(),
              db.data_ptr(), scratch.data_ptr(), n, d, st)
    # the bias alone (no weight gradient asked for): the same bits
    db1 = torch.full((1,), nan, device="cuda")
    _lib.call("cuda", "srg_hop_scores_grad_f32", ptrs, lds, T, start, end, KINDS[kind], dz.data_ptr(), None,
              db1.data_ptr(), scratch.data_ptr(), n, d, st)
    assert np.array_equal(_bits(db1), _bits(db))
    return z, P, out, dw, db, buf


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("kind,d", [("jk", 1), ("ori_ref", 3), ("gate", 6), ("jk", 64), ("ori_ref", 65), ("gate", 257),
                                    ("jk", 1028), ("ori_ref", 1433)])
def test_entries_at_every_width(kind, d, pad):
    """The C entries at n = 61 (no multiple of any rows-per-wave), T = 4, slice 1..4: one lane per row up
    to 64 lanes with several chunks each, 4-, 8- and 16-byte accesses, rows past one column tile of the
    parameter gradient (d = 1028: 257 chunks; d = 1433: 6 tiles), leading dimensions d + 3.  The scores and
    the weights against their own bounds too; the padding of out stays untouched."""
    n, T, start, end = 61, 4, 1, 4
    hops, w, b, C = R.random_case(kind, n, d, T, start, end, 100 + d)
    ref = R.evaluate(kind, hops, start, end, w, b, G=C)
    dev = [torch.nn.functional.pad(torch.from_numpy(h).cuda(), (0, pad), value=7.5)[:, :d] for h in hops]
    Gd = torch.nn.functional.pad(torch.from_numpy(C).cuda(), (0, pad), value=7.5)[:, :d]
    z, P, out, dw, db, buf = _capi(kind, dev, start, end, w, b, Gd, pad)
    what = f"entries {kind} d={d} ld=d+{pad}"
    assert R.worst_ratio(z.cpu().numpy().reshape(end - start, n), ref["z"], ref["E_z"]) <= 1.0, what + " scores"
    assert R.worst_ratio(P.cpu().numpy(), ref["P"], ref["E_P"]) <= 1.0, what + " weights"
    R.check(what, out.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), ref)
    assert bool((buf[:, d:] == 7.5).all()), "the attend step wrote past the row's d columns"
    again = _capi(kind, dev, start, end, w, b, Gd, pad)
    for x, y in zip((z, P, out, dw, db), again):
        assert np.array_equal(_bits(x), _bits(y))


def test_peak_memory_at_the_gamlp_shape():
    """jk, T = 11, d = 128, n = 20,000: forward plus backward allocate less than 4 n d floats beyond the
    hop list and G (out, the per-row vectors, the partials); the composition's temporaries alone are
    H (T + 1) n d = 132 n d floats."""
    n, d, T = 20000, 128, 11
    gen = torch.Generator(device="cuda").manual_seed(5)
    hops = [torch.randn((n, d), device="cuda", generator=gen) for _ in range(T)]
    Gd = torch.randn((n, d), device="cuda", generator=gen)
    w = torch.randn((1, R.in_dim("jk", T, d)), generator=torch.Generator().manual_seed(6)) * 0.02
    _run_op("jk", [h[:64] for h in hops], 0, T, w, [0.1], Gd[:64])     # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, dw, db = _run_op("jk", hops, 0, T, w, [0.1], Gd)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak beyond the hops and G: {extra / (n * d * 4):.3f} n*d*4 bytes")
    assert extra < 4 * n * d * 4
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dw).all())


def test_argument_checks_raise_before_any_launch(golden):
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    from srgnn.hop_attention import hop_attention
    c, hops, w, b, *_ = R.load_case(golden, "jk_t4")
    dev = _windows(hops, 0)
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
    with pytest.raises(ValueError, match="requires grad"):
        hop_attention(dev[:2] + [dev[2].clone().requires_grad_()] + dev[3:], 0, 4, "jk", wd, bd)
    with pytest.raises(TypeError, match="float32"):
        hop_attention(dev[:3] + [dev[3].double()], 0, 4, "jk", wd, bd)
    many = [dev[0]] * 33
    with pytest.raises(ValueError, match="at most 32"):
        hop_attention(many, 0, 33, "gate", torch.zeros((1, 12), device="cuda"), bd)
    with pytest.raises(ValueError, match="needs a weight of"):
        hop_attention(dev + [dev[0]], 0, 4, "jk", wd, bd)          # 5 hops, prop_steps + 1 = 4
    with pytest.raises(ValueError, match="hop slice"):
        hop_attention(dev, 0, 5, "gate", torch.zeros((1, 12), device="cuda"), bd)      # end past the list
    with pytest.raises(ValueError, match="kind"):
        hop_attention(dev, 0, 4, "simple", wd, bd)
    # through the operator: a hop that requires grad takes the composition, an fp64 hop raises
    op = LearnableWeightedMessageOp(0, 4, "jk", 3, 12).cuda()
    op.fused = True
    out = op.aggregate(dev[:3] + [dev[3].clone().requires_grad_()])
    assert type(out.grad_fn).__name__ != "_HopAttentionBackward"
    with pytest.raises(TypeError):
        op.aggregate([h.double() for h in dev])
    # only the gradient autograd asks for
    op.learnable_weight.weight.requires_grad_(False)
    op.aggregate(dev).sum().backward()
    assert op.learnable_weight.weight.grad is None and op.learnable_weight.bias.grad is not None


def test_entries_with_no_rows_and_bad_arguments():
    from srgnn import _lib
    st = _lib.stream("cuda")
    one = (ctypes.c_void_p * 1)(None)
    ld = (ctypes.c_int64 * 1)(4)
    _lib.call("cuda", "srg_hop_scores_f32", one, ld, 1, 0, 1, _lib.SRG_HOP_GATE, None, None, None, 0, 4, st)
    _lib.call("cuda", "srg_hop_attend_f32", one, ld, 1, 0, 1, None, _lib.SRG_HOP_PAIR_TRANSPOSE, None, None, 4, 0, 4, st)
    _lib.call("cuda", "srg_hop_attend_grad_f32", one, ld, 1, 0, 1, None, 4, None, None, _lib.SRG_HOP_PAIR_FLAT, None,
              None, 0, 4, st)
    dw, db = torch.ones(4, device="cuda"), torch.ones(1, device="cuda")
    _lib.call("cuda", "srg_hop_scores_grad_f32", one, ld, 1, 0, 1, _lib.SRG_HOP_GATE, None, dw.data_ptr(), db.data_ptr(),
              None, 0, 4, st)
    assert not dw.any() and not db.any()
    x = torch.zeros((8, 4), device="cuda")
    v = torch.zeros(8 * 33, device="cuda")
    many = (ctypes.c_void_p * 33)(*[x.data_ptr()] * 33)
    lds = (ctypes.c_int64 * 33)(*[4] * 33)
    bad = [
        (many, lds, 33, 0, 33, _lib.SRG_HOP_GATE, x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4),    # T > 32
        (many, lds, 4, 2, 2, _lib.SRG_HOP_GATE, x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4),      # empty slice
        (many, lds, 4, 0, 5, _lib.SRG_HOP_GATE, x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4),      # end > T
        (many, lds, 4, 0, 4, 3, x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 4),                      # kind
        (many, lds, 4, 0, 4, _lib.SRG_HOP_GATE, x.data_ptr(), v.data_ptr(), v.data_ptr(), 8, 5),      # ld < d
        (many, lds, 4, 0, 4, _lib.SRG_HOP_GATE, None, v.data_ptr(), v.data_ptr(), 8, 4),              # no weight
    ]
    for args in bad:
        with pytest.raises(_lib.SrgError):
            _lib.call("cuda", "srg_hop_scores_f32", *args, st)
    with pytest.raises(_lib.SrgError):                                                                 # out is a panel
        _lib.call("cuda", "srg_hop_attend_f32", many, lds, 4, 0, 4, v.data_ptr(), 0, v.data_ptr(), x.data_ptr(), 4, 8, 4, st)
