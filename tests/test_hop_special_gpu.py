"""The fused hop attention on the GPU where the O(1) draws of the other hop tests never go (the cases of
tests/hop_special_cases.py; DESIGN.md §5.4.2 - §5.4.4, "Special values and saturation"): saturated sigmoids, NaN /
Inf / subnormal / signed-zero panel cells, poisoned panels a kind must not read, a poisoned stand-in row behind
out-of-range indices, T = H = SRG_HOP_MAX for the learnable kinds, and n past the launch caps, where every
grid-stride loop takes another trip.  Every test runs the three learnable kinds and the recursive form, on whole
panels and under index= (shuffled, with duplicates).  The expectation is the fp64 restatement on the same fp32
values with its derived bound, the classes of non-finite results included, or the device's own bits on inputs
that must give the same result.  No bound here was chosen after a device result; the measured ratios are in DESIGN.
"""
import ctypes

import numpy as np
import pytest
import torch

import hop_attention_ref as R
import hop_recursive_ref as RR
import hop_special_cases as SC

pytestmark = pytest.mark.gpu

N, N_SRC, T, START, END = 130, 200, 5, 1, 4
WIDTHS = [1, 6, 64, 130, 260]     # lgS 0, 3, 4, 6, 6; 4-, 8-, 16-, 8-, 16-byte accesses; 65 chunks (two trips) at 130 and 260
N_BIG = 4194304 + 130             # past 256 * 64 blocks of 4 waves of 64 one-lane rows: the smallest n at which they all loop
NEG_ZERO, POS_ZERO = 0x80000000, 0


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _dev(arrays, pad=0):
    """Device copies of the [n, d] arrays; pad > 0: each a column window at offset 1 (4 bytes) of its own
    [n, d + pad] buffer (filled with 7.5): the 4-byte path whatever d is."""
    out = []
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if pad:
            buf = torch.full((a.shape[0], a.shape[1] + pad), 7.5, dtype=torch.float32, device="cuda")
            buf[:, 1:1 + a.shape[1]] = t
            t = buf[:, 1:1 + a.shape[1]]
        out.append(t)
    return out


def _run(case, feats, C, index=None, check=True):
    """(out, dw, db) of the Python path on device tensors."""
    from srgnn.hop_attention import hop_attention, hop_attention_recursive
    wd = torch.from_numpy(case["w"]).cuda().requires_grad_()
    bd = torch.from_numpy(case["b"]).cuda().requires_grad_()
    if case["kind"] == "recursive":
        out = hop_attention_recursive(feats, case["end"], wd, bd, index=index, check=check)
    else:
        out = hop_attention(feats, case["start"], case["end"], case["kind"], wd, bd, index=index, check=check)
    out.backward(C)
    return out.detach(), wd.grad, bd.grad


def _host(got):
    return tuple(x.cpu().numpy() for x in got)


def _check(case, what, got, ref):
    return (RR if case["kind"] == "recursive" else R).check(what, *_host(got), ref)


def _forms(builder, kind, d, seed):
    """(form, case, idx, C): the builder's case on whole panels of N rows, and on panels of N_SRC rows under an
    index that holds every row (so whatever was planted is in the batch), shuffled, with duplicates."""
    case = builder(kind, N, d, T, START, END, seed)
    yield "identity", case, None, case["C"]
    case = builder(kind, N_SRC, d, T, START, END, seed + 1)
    idx = SC.batch_index(N_SRC, seed + 2)
    C = SC.cotangent(idx.size, d, seed + 3)
    if builder is SC.planted:
        C[20, :] = np.nan
    yield "index", case, idx, C


def _index(idx):
    return None if idx is None else torch.from_numpy(idx).cuda()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_saturated_scores(kind, d, pad):
    """|score| from 0.01 to several thousand, every expf regime with both signs (the builder asserts it): out, dw
    and db finite and within the unchanged bound; twice: the same bits.  pad = 5: the 4-byte path at every d."""
    for form, case, idx, C in _forms(SC.saturated, kind, d, 400 + d):
        feats, Cd = _dev(case["hops"], pad), _dev([C], pad)[0]
        got = _run(case, feats, Cd, index=_index(idx))
        assert all(bool(torch.isfinite(x).all()) for x in got)
        _check(case, f"saturated {kind} d={d} pad={pad} {form}", got, SC.exact(case, C, idx))
        assert _same(got, _run(case, feats, Cd, index=_index(idx))), f"{kind} d={d} {form}: not deterministic"


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_planted_non_finite_cells(kind, d):
    """NaN, +Inf and -Inf cells, a NaN panel row and a NaN cotangent row: every element of out, dw and db has the
    class the restatement gives it and the finite ones are within their bound.  The rows of out the restatement
    leaves untouched by the planted cells (the same exact out and P with the cells set to 1.0: neither the row's own
    cells nor, through the pairing, its scores changed) have the bits of the run on those clean panels: nothing
    leaks between rows that share a wave."""
    for form, case, idx, C in _forms(SC.planted, kind, d, 500 + d):
        ref = SC.exact(case, C, idx)
        got = _run(case, _dev(case["hops"]), _dev([C])[0], index=_index(idx))
        for x, k in zip(_host(got), ("out", "dw", "db")):
            R.check_special(f"planted {kind} d={d} {form} {k}", x, ref[k], ref["E_" + k])
        if kind == "recursive" and d > 1:
            # hop 0's Inf cell where w_h and w_c disagree in sign: s_0 = inf - inf, the whole row is NaN
            src = np.arange(N) if idx is None else idx
            assert case["s0_nan_row"] == 100 and np.isnan(_host(got)[0][src == 100]).all()
        clean = SC.with_cells(case, 1.0)
        ref_clean = SC.exact(case, C, idx, hops=clean)
        untouched = (ref["out"] == ref_clean["out"]).all(axis=1) & (ref["P"] == ref_clean["P"]).all(axis=1)
        assert np.isfinite(ref["out"][untouched]).all() and untouched.sum() > untouched.size // 2
        assert not untouched.all()
        out_clean = _run(case, _dev(clean), _dev([C])[0], index=_index(idx))[0]
        assert np.array_equal(_bits(got[0])[untouched], _bits(out_clean)[untouched]), \
            f"planted {kind} d={d} {form}: a row the planted cells cannot reach changed"


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_unread_panels_are_not_touched(kind, d):
    """Every panel the kind does not read filled with NaN: the bits of the run with zeros there (jk reads every
    panel: the two runs are the same call), finite and within the bound."""
    for form, case, idx, C in _forms(SC.unread_poison, kind, d, 600 + d):
        assert (len(case["unread"]) > 0) == (kind != "jk")
        Cd = _dev([C])[0]
        got = _run(case, _dev(case["hops"]), Cd, index=_index(idx))
        assert all(bool(torch.isfinite(x).all()) for x in got), f"{kind} d={d} {form}: read a panel it should not"
        assert _same(got, _run(case, _dev(SC.with_unread(case, 0.0)), Cd, index=_index(idx)))
        _check(case, f"unread_poison {kind} d={d} {form}", got, SC.exact(case, C, idx))


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_subnormal_and_signed_zero_rows(kind, d):
    """A row of subnormal cells is combined, not flushed: nonzero, within the bound plus the format's underflow
    allowance (H products of absolute error 2^-150).  A row of -0.0 gives -0.0 in every column and a row of +0.0
    gives +0.0: the combination runs left to right from its first term as it is, and P > 0."""
    H = END - (0 if kind == "recursive" else START)
    for form, case, idx, C in _forms(SC.denormal_row, kind, d, 700 + d):
        ref = SC.exact(case, C, idx)
        out, dw, db = _host(_run(case, _dev(case["hops"]), _dev([C])[0], index=_index(idx)))
        src = np.arange(N) if idx is None else idx
        tiny, neg, pos = (np.nonzero(src == r)[0] for r in (SC.DENORMAL_ROW, SC.NEG_ZERO_ROW, SC.POS_ZERO_ROW))
        assert tiny.size and neg.size and pos.size
        what = f"denormal_row {kind} d={d} {form}"
        assert out[tiny].all(), f"{what}: a subnormal was flushed to zero"
        assert (np.abs(ref["out"][tiny]) < 2.0 ** -126).all()
        ratios = (R.worst_ratio(out, ref["out"], ref["E_out"] + R.underflow_allowance(H)),
                  R.worst_ratio(dw, ref["dw"], ref["E_dw"]), R.worst_ratio(db, ref["db"], ref["E_db"]))
        print(f"hop attention |got - exact| / (bound + allowance)  {what}: out {ratios[0]:.4f}  dw {ratios[1]:.4f}  db {ratios[2]:.4f}")
        assert max(ratios) <= 1.0, f"{what}: at {ratios} of the bound"
        assert (out.view(np.uint32)[neg] == NEG_ZERO).all(), f"{what}: a row of -0.0 did not give -0.0"
        assert (out.view(np.uint32)[pos] == POS_ZERO).all(), f"{what}: a row of +0.0 did not give +0.0"


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_unreadable_rows_are_selected_not_multiplied(kind, d):
    """check=False with -1, n_src and 2^40 in the index, over panels whose row 0 (the row whose address stands in for
    an unreadable index) is NaN and whose last row is +Inf: nothing is non-finite, the unreadable batch rows are
    +0.0, and out, dw and db have the bits of the run on panels whose two guard rows hold 1.0.  Every index the
    entries are handed here is one they document as a row of zeros; no address outside the panels is formed."""
    case = SC.row0_poison(kind, N_SRC, d, T, START, END, 800 + d)
    index, Cd = _index(case["index"]), _dev([case["C"]])[0]
    got = _run(case, _dev(case["hops"]), Cd, index=index, check=False)
    for x, k in zip(got, ("out", "dw", "db")):
        assert bool(torch.isfinite(x).all()), f"row0_poison {kind} d={d}: {k} saw a guard row"
    assert (_bits(got[0])[case["bad"]] == POS_ZERO).all()
    assert _same(got, _run(case, _dev(SC.with_guard_rows(case, 1.0)), Cd, index=index, check=False))
    _check(case, f"row0_poison {kind} d={d}", got, SC.exact(case, case["C"], case["index"]))


@pytest.mark.parametrize("d", [3, 64])
@pytest.mark.parametrize("kind", ["gate", "jk"])
def test_learnable_kinds_at_the_hop_limit(kind, d):
    """T = H = SRG_HOP_MAX = 32 at n = 70 (jk: a weight of 33 d elements), whole panels and under an index."""
    from srgnn import _lib
    H = _lib.SRG_HOP_MAX
    assert H == 32
    case = SC.base(kind, 70, d, H, 0, H, 900 + d)
    got = _run(case, _dev(case["hops"]), _dev([case["C"]])[0])
    _check(case, f"limit {kind} d={d} identity", got, SC.exact(case))
    idx = SC.batch_index(70, 901 + d, extra=15)
    C = SC.cotangent(idx.size, d, 902 + d)
    got = _run(case, _dev(case["hops"]), _dev([C])[0], index=_index(idx))
    _check(case, f"limit {kind} d={d} index", got, SC.exact(case, C, idx))


@pytest.mark.parametrize("kind", SC.KINDS)
def test_past_the_grid_caps(kind):
    """d = 1, T = 2, slice [0, 2), n = 4,194,304 + 130: one lane per row, so the row-streaming kernels' 16,384 blocks
    of 256 rows take a second trip, and the one-thread-per-row and recurrence kernels (1,048,576 rows a trip) a
    fifth.  Within the bound of the restatement, which is vectorised over n.  gate and recursive treat rows
    independently: out on the last 130 rows and on the 130 rows astride row 4,194,304 has the bits of a run on those
    rows alone (the same d and alignment, hence the same access width), and so have the scores and the backward's
    per-row vectors.  The entries called on NaN canaries leave no slot of any buffer unwritten."""
    case = SC.base(kind, N_BIG, 1, 2, 0, 2, 1000)
    feats, Cd = _dev(case["hops"]), _dev([case["C"]])[0]
    got = _run(case, feats, Cd)
    _check(case, f"grid caps {kind} identity", got, SC.exact(case))
    # the entries on NaN canaries: a trip a loop left out would leave its slots of the per-row vectors unwritten
    bufs = _entries(case, feats, None, Cd, False)
    for name, t in bufs.items():
        assert bool(torch.isfinite(t).all()), f"grid caps {kind}: {name} has unwritten slots"
    assert _same((bufs["out"], bufs["dw"].view(-1), bufs["db"]), (got[0], got[1].view(-1), got[2]))
    if kind in ("gate", "recursive"):
        per_row = ("zp", "zq", "dzp", "dzq") if kind == "recursive" else ("zflat", "dz")
        for lo in (N_BIG - 130, 4194304 - 65):
            sub = [f[lo:lo + 130] for f in feats]
            part = _run(case, sub, Cd[lo:lo + 130])[0]
            assert np.array_equal(_bits(part), _bits(got[0][lo:lo + 130])), f"{kind}: rows from {lo} differ from a run of their own"
            alone = _entries(case, sub, None, Cd[lo:lo + 130], False)
            for name in per_row:     # hop-major [H, n] vectors: the backward's per-row results too
                assert np.array_equal(_bits(bufs[name].view(2, N_BIG)[:, lo:lo + 130]), _bits(alone[name].view(2, 130))), \
                    f"{kind}: {name} of the rows from {lo} differs from a run of their own"


@pytest.mark.parametrize("kind", SC.KINDS)
def test_past_the_grid_caps_under_an_index(kind):
    """A batch of 4,194,304 + 130 rows over 1,000-row panels: the same second trips with rows[] in the way."""
    case = SC.base(kind, 1000, 1, 2, 0, 2, 1001)
    idx = np.random.default_rng(1002).integers(0, 1000, N_BIG)
    C = SC.cotangent(N_BIG, 1, 1003)
    feats, Cd = _dev(case["hops"]), _dev([C])[0]
    got = _run(case, feats, Cd, index=_index(idx))
    _check(case, f"grid caps {kind} index", got, SC.exact(case, C, idx))
    bufs = _entries(case, feats, _index(idx), Cd, True)
    for name, t in bufs.items():
        assert bool(torch.isfinite(t).all()), f"grid caps {kind} under an index: {name} has unwritten slots"
    assert _same((bufs["out"], bufs["dw"].view(-1), bufs["db"]), (got[0], got[1].view(-1), got[2]))


def _entries(case, feats, idx, Gd, twin):
    """The four entries of the case's kind called directly -- the *_rows_* twins on the rows idx, or the base
    entries -- with every buffer they fill set to NaN first.  Returns {name: tensor} of those buffers."""
    from srgnn import _lib
    from srgnn.hop_attention import KINDS as KIND_ID, _pairing
    k, start, end, d = case["kind"], case["start"], case["end"], case["d"]
    n = feats[0].shape[0] if idx is None else idx.numel()
    Tn, H = len(feats), end - start
    ptrs = (ctypes.c_void_p * Tn)(*[h.data_ptr() for h in feats])
    lds = (ctypes.c_int64 * Tn)(*[h.stride(0) for h in feats])
    wd, bd = torch.from_numpy(case["w"]).cuda().view(-1), torch.from_numpy(case["b"]).cuda()
    head = (ptrs, lds) + ((idx.data_ptr(), feats[0].shape[0]) if twin else ())
    st = _lib.stream("cuda")
    nbytes = ctypes.c_int64(-1)

    def canary(*shape):
        return torch.full(shape, float("nan"), device="cuda")

    def call(name, *rest):
        _lib.call("cuda", name.replace("_f32", "_rows_f32") if twin else name, *head, *rest, st)

    bufs = dict(P=canary(n, H), out=canary(n, d), dw=canary(wd.numel()), db=canary(1))
    if k == "recursive":
        bufs.update(zp=canary(H * n), zq=canary(H * n), dzp=canary(H * n), dzq=canary(H * n),
                    work=canary(RR.work_floats(H) * n))
        _lib.check(_lib.lib().srg_hop_recur_scores_grad_scratch_bytes(n, d, H, ctypes.byref(nbytes)), "scratch")
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
        p = {name: t.data_ptr() for name, t in bufs.items()}
        call("srg_hop_recur_scores_f32", Tn, end, wd.data_ptr(), p["zp"], p["zq"], n, d)
        call("srg_hop_recur_attend_f32", Tn, end, p["zp"], p["zq"], bd.data_ptr(), p["work"], p["P"], p["out"], d, n, d)
        call("srg_hop_recur_attend_grad_f32", Tn, end, Gd.data_ptr(), Gd.stride(0), p["zq"], p["work"], p["dzp"],
             p["dzq"], n, d)
        call("srg_hop_recur_scores_grad_f32", Tn, end, p["dzp"], p["dzq"], p["dw"], p["db"], scratch.data_ptr(), n, d)
    else:
        bufs.update(zflat=canary(H * n), dz=canary(H * n), dP=canary(n, H))
        _lib.check(_lib.lib().srg_hop_scores_grad_scratch_bytes(n, d, Tn, H, KIND_ID[k], ctypes.byref(nbytes)), "scratch")
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
        p = {name: t.data_ptr() for name, t in bufs.items()}
        call("srg_hop_scores_f32", Tn, start, end, KIND_ID[k], wd.data_ptr(), bd.data_ptr(), p["zflat"], n, d)
        call("srg_hop_attend_f32", Tn, start, end, p["zflat"], _pairing(k), p["P"], p["out"], d, n, d)
        call("srg_hop_attend_grad_f32", Tn, start, end, Gd.data_ptr(), Gd.stride(0), p["zflat"], p["P"], _pairing(k),
             p["dP"], p["dz"], n, d)
        call("srg_hop_scores_grad_f32", Tn, start, end, KIND_ID[k], p["dz"], p["dw"], p["db"], scratch.data_ptr(), n, d)
    return bufs


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_entries_directly_at_saturated_scores(kind, twin):
    """Each of the 16 C entries on `saturated` with raw pointers, every buffer they fill a NaN canary first: the
    scores, P, dP, dz (zp, zq, dzp, dzq and the work buffer of the recursive form), out, dw and db have no slot left
    unwritten and hold nothing non-finite, and out, dw and db are the Python path's bits."""
    d = 6
    if twin:
        case = SC.saturated(kind, N_SRC, d, T, START, END, 1100)
        idx = SC.batch_index(N_SRC, 1101)
        C = SC.cotangent(idx.size, d, 1102)
    else:
        case, idx = SC.saturated(kind, N, d, T, START, END, 1103), None
        C = case["C"]
    feats, Cd = _dev(case["hops"]), _dev([C])[0]
    bufs = _entries(case, feats, _index(idx), Cd, twin)
    for name, t in bufs.items():
        assert not bool(torch.isnan(t).any()), f"{kind} twin={twin}: {name} has unwritten or NaN slots"
        assert bool(torch.isfinite(t).all()), f"{kind} twin={twin}: {name} is not finite"
    want = _run(case, feats, Cd, index=_index(idx))
    for name, y in zip(("out", "dw", "db"), want):
        assert np.array_equal(_bits(bufs[name]).reshape(-1), _bits(y).reshape(-1)), f"{kind} twin={twin}: {name}"
    _check(case, f"entries saturated {kind} twin={twin}", (bufs["out"], bufs["dw"], bufs["db"]), SC.exact(case, C, idx))
