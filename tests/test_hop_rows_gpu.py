"""The row-indexed fused hop attention on the GPU: the srg_hop_*_rows_f32 entries behind
srgnn.hop_attention(..., index=) / hop_attention_recursive(..., index=) and the operators' aggregate_rows
(DESIGN.md §5.4.4).  The expectation is the fused path itself on gathered [B, d] copies of the indexed rows,
bit for bit, where both have the same access width; and the fp64 restatements of tests/hop_attention_ref.py /
tests/hop_recursive_ref.py on the numpy rows hop[idx], within their derived bounds, everywhere.  No index here
can address memory outside an allocation of the test's own.
"""
import ctypes

import numpy as np
import pytest
import torch

import hop_attention_ref as R
import hop_recursive_ref as RR

pytestmark = pytest.mark.gpu

N_SRC = 300
KINDS = ("gate", "ori_ref", "jk", "jk_inner", "recursive")
CTOR = {"jk": lambda T, d: (T - 1, d), "ori_ref": lambda T, d: (d,), "gate": lambda T, d: (d,)}


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _slice(kind, T):
    return (1, T - 1) if kind == "jk_inner" else (0, T)


def _case(kind, d, T, seed, n=N_SRC):
    """(kernel kind, start, end, hops, w, b) with numpy hops of n rows; None where the slice would be empty."""
    start, end = _slice(kind, T)
    if end <= start:
        return None
    if kind == "recursive":
        hops, w, b, _ = RR.random_case(n, d, T, seed)
        return "recursive", 0, T, hops, w, b
    k = "jk" if kind == "jk_inner" else kind
    hops, w, b, _ = R.random_case(k, n, d, T, start, end, seed)
    return k, start, end, hops, w, b


def _index_cases(n_src, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_src)
    return {"one": np.array([n_src * 173 // 300]), "shuffled37": perm[:37], "shuffled129": perm[:129],
            "duplicates700": rng.integers(0, n_src, 700), "identity": np.arange(n_src),
            "sorted": np.sort(rng.choice(n_src, n_src // 2, replace=False))}


def _cotangent(B, d, seed):
    return np.random.default_rng(seed).standard_normal((B, d)).astype(np.float32)


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


def _run(k, feats, start, end, w, b, C, index=None, check=True):
    """(out, dw, db) of the Python path on device tensors; k: gate / ori_ref / jk / recursive."""
    from srgnn.hop_attention import hop_attention, hop_attention_recursive
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
    if k == "recursive":
        out = hop_attention_recursive(feats, end, wd, bd, index=index, check=check)
    else:
        out = hop_attention(feats, start, end, k, wd, bd, index=index, check=check)
    out.backward(C)
    return out.detach(), wd.grad, bd.grad


def _exact(k, rows, start, end, w, b, C, **kw):
    if k == "recursive":
        return RR.evaluate(rows, end, w, b, G=C, **kw)
    return R.evaluate(k, rows, start, end, w, b, G=C, **kw)


def _check(k, what, got, ref):
    out, dw, db = (x.cpu().numpy() for x in got)
    return (RR if k == "recursive" else R).check(what, out, dw, db, ref)


def _ratio(ref, out, dw, db):
    return max(R.worst_ratio(out, ref["out"], ref["E_out"]), R.worst_ratio(dw, ref["dw"], ref["E_dw"]),
               R.worst_ratio(db, ref["db"], ref["E_db"]))


@pytest.mark.parametrize("d", [1, 3, 6, 64, 65, 128, 130, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_for_bit_against_the_gathered_run(kind, d):
    """index= against the same call on [f[idx].contiguous() for f in feats]: out, dw and db bit for bit, for
    T = 1, 4, 11 and every index case (B = 129: five parameter-gradient groups of 32, the last of one row;
    B = 700 > n_src with duplicates).  Both sides are contiguous fresh allocations of the same d, so both take
    the same access width.  Twice: the same bits."""
    ran = 0
    for T in (1, 4, 11):
        case = _case(kind, d, T, 1000 + 13 * d + T)
        if case is None:
            continue
        k, start, end, hops, w, b = case
        feats = _windows(hops, 0)
        for name, idx in _index_cases(N_SRC, d + T).items():
            what = f"{kind} d={d} T={T} {name}"
            index = torch.from_numpy(idx).cuda()
            C = torch.from_numpy(_cotangent(idx.size, d, idx.size + d)).cuda()
            got = _run(k, feats, start, end, w, b, C, index=index)
            want = _run(k, [f[index].contiguous() for f in feats], start, end, w, b, C)
            assert got[0].shape == (idx.size, d), what
            for x, y, part in zip(got, want, ("out", "dw", "db")):
                assert np.array_equal(_bits(x), _bits(y)), f"{what}: {part} differs from the gathered run"
            assert _same(got, _run(k, feats, start, end, w, b, C, index=index)), f"{what}: not deterministic"
            ran += 1
    assert ran >= 12


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("d", [6, 65, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_within_the_derived_bound_of_the_exact_formula(kind, d, pad):
    """The restatement on the numpy rows hop[idx] is the expectation, for contiguous panels and for column
    windows at an odd element offset of wider buffers (the 4-byte path: the bits need not be the gathered
    run's, the bound holds all the same).  The negative controls, evaluated exactly on the same rows, leave
    the bound, and the device's result is outside theirs: the other pairing and two swapped hops (recursive:
    a plain softmax and the weight's halves swapped); and, for the .view(-1, H) pairing, scores paired relative
    to the source panels instead of the batch."""
    T = 4
    k, start, end, hops, w, b = _case(kind, d, T, 2000 + d)
    feats = _windows(hops, pad)
    cases = _index_cases(N_SRC, 7 * d)
    for name in ("shuffled129", "duplicates700"):
        idx = cases[name]
        C = _cotangent(idx.size, d, 31 + idx.size)
        rows = [h[idx] for h in hops]
        ref = _exact(k, rows, start, end, w, b, C)
        Cd = _windows([C], pad)[0]
        got = _run(k, feats, start, end, w, b, Cd, index=torch.from_numpy(idx).cuda())
        what = f"rows {kind} d={d} pad={pad} {name}"
        _check(k, what, got, ref)
        if k == "recursive":
            controls = {"plain softmax": dict(nested=False), "swapped halves": dict(swap_halves=True)}
        else:
            controls = {"pairing": dict(pairing="flat" if k == "gate" else "transpose"), "swapped hops": dict(swap=(0, 1))}
        g = [x.cpu().numpy() for x in got]
        for cname, kw in controls.items():
            wrong = _exact(k, rows, start, end, w, b, C, **kw)
            assert _ratio(ref, wrong["out"], wrong["dw"], wrong["db"]) > 1.0, f"{what}: the bound hides `{cname}`"
            assert _ratio(wrong, *g) > 1.0, f"{what}: the result fits `{cname}`"
        if k in ("ori_ref", "jk"):
            # the pairing taken relative to the n_src source rows: whole panels, then the batch's rows picked
            Cfull = np.zeros((N_SRC, d), dtype=np.float32)
            full = R.evaluate(k, hops, start, end, w, b, G=Cfull)
            assert R.worst_ratio(full["out"][idx], ref["out"], ref["E_out"]) > 1.0, f"{what}: source-relative pairing"


def _capi(k, hops, idx, n_src, start, end, w, b, Gd, ldo_pad, twin=True):
    """The four entries of kind k (gate / ori_ref / jk / recursive) called directly: the *_rows_* twins with
    rows = idx (None: NULL), or the base entries (twin=False).  Returns (out, dw, db) and the out buffer."""
    from srgnn import _lib
    from srgnn.hop_attention import KINDS as KIND_ID, _pairing
    d = hops[0].shape[1]
    n = hops[0].shape[0] if idx is None else idx.numel()
    T, H = len(hops), end - start
    ptrs = (ctypes.c_void_p * T)(*[h.data_ptr() for h in hops])
    lds = (ctypes.c_int64 * T)(*[h.stride(0) for h in hops])
    wd, bd = torch.from_numpy(w).cuda().view(-1), torch.from_numpy(b).cuda()
    nan = float("nan")
    buf = torch.full((n, d + ldo_pad), 7.5, device="cuda")
    out = buf[:, :d]
    dw, db = torch.full((wd.numel(),), nan, device="cuda"), torch.full((1,), nan, device="cuda")
    P = torch.full((n, H), nan, device="cuda")
    st = _lib.stream("cuda")
    head = (ptrs, lds) + ((idx.data_ptr() if idx is not None else None, n_src) if twin else ())
    nbytes = ctypes.c_int64(-1)

    def call(name, *rest):
        _lib.call("cuda", name.replace("_f32", "_rows_f32") if twin else name, *head, *rest, st)

    if k == "recursive":
        zp, zq = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
        dzp, dzq = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
        work = torch.full((RR.work_floats(H) * n,), nan, device="cuda")
        _lib.check(_lib.lib().srg_hop_recur_scores_grad_scratch_bytes(n, d, H, ctypes.byref(nbytes)), "scratch")
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
        call("srg_hop_recur_scores_f32", T, end, wd.data_ptr(), zp.data_ptr(), zq.data_ptr(), n, d)
        call("srg_hop_recur_attend_f32", T, end, zp.data_ptr(), zq.data_ptr(), bd.data_ptr(), work.data_ptr(),
             P.data_ptr(), out.data_ptr(), d + ldo_pad, n, d)
        call("srg_hop_recur_attend_grad_f32", T, end, Gd.data_ptr(), Gd.stride(0), zq.data_ptr(), work.data_ptr(),
             dzp.data_ptr(), dzq.data_ptr(), n, d)
        call("srg_hop_recur_scores_grad_f32", T, end, dzp.data_ptr(), dzq.data_ptr(), dw.data_ptr(), db.data_ptr(),
             scratch.data_ptr(), n, d)
    else:
        z, dz = torch.full((H * n,), nan, device="cuda"), torch.full((H * n,), nan, device="cuda")
        dP = torch.full((n, H), nan, device="cuda")
        _lib.check(_lib.lib().srg_hop_scores_grad_scratch_bytes(n, d, T, H, KIND_ID[k], ctypes.byref(nbytes)), "scratch")
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
        call("srg_hop_scores_f32", T, start, end, KIND_ID[k], wd.data_ptr(), bd.data_ptr(), z.data_ptr(), n, d)
        call("srg_hop_attend_f32", T, start, end, z.data_ptr(), _pairing(k), P.data_ptr(), out.data_ptr(), d + ldo_pad,
             n, d)
        call("srg_hop_attend_grad_f32", T, start, end, Gd.data_ptr(), Gd.stride(0), z.data_ptr(), P.data_ptr(),
             _pairing(k), dP.data_ptr(), dz.data_ptr(), n, d)
        call("srg_hop_scores_grad_f32", T, start, end, KIND_ID[k], dz.data_ptr(), dw.data_ptr(), db.data_ptr(),
             scratch.data_ptr(), n, d)
    return (out, dw, db), buf


@pytest.mark.parametrize("d", [1, 65, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_entries_directly(kind, d):
    """The eight *_rows_* entries on their own, out and G with leading dimensions d + 4 (a multiple of every
    access width, so the width is the panels'): the Python path's bits; rows = NULL: the base entries' bits;
    the padding of out stays untouched."""
    T, pad = 4, 4
    k, start, end, hops, w, b = _case(kind, d, T, 3000 + d)
    feats = _windows(hops, 0)
    idx = torch.from_numpy(_index_cases(N_SRC, d)["duplicates700"][:333]).cuda()
    C = torch.from_numpy(_cotangent(idx.numel(), d, 5)).cuda()
    Gd = torch.nn.functional.pad(C, (0, pad), value=7.5)[:, :d]
    got, buf = _capi(k, feats, idx, N_SRC, start, end, w, b, Gd, pad)
    want = _run(k, feats, start, end, w, b, C, index=idx)
    for x, y, part in zip(got, want, ("out", "dw", "db")):
        assert np.array_equal(_bits(x), _bits(y).reshape(_bits(x).shape)), f"{kind} d={d}: {part} differs from the Python path"
    assert bool((buf[:, d:] == 7.5).all()), "the attend step wrote past the row's d columns"
    Cn = torch.from_numpy(_cotangent(N_SRC, d, 6)).cuda()
    Gn = torch.nn.functional.pad(Cn, (0, pad), value=7.5)[:, :d]
    null, _ = _capi(k, feats, None, 0, start, end, w, b, Gn, pad)
    base, _ = _capi(k, feats, None, 0, start, end, w, b, Gn, pad, twin=False)
    assert _same(null, base), f"{kind} d={d}: rows = NULL is not the base entry"


def test_entries_with_no_rows_and_bad_arguments():
    """n = 0 is a no-op (the parameter gradient stores zeros); the base entries' argument checks hold for the
    twins, before any launch."""
    from srgnn import _lib
    st = _lib.stream("cuda")
    one = (ctypes.c_void_p * 1)(None)
    ld = (ctypes.c_int64 * 1)(4)
    ix = torch.zeros(8, dtype=torch.int64, device="cuda")
    r = ix.data_ptr()
    G = _lib.SRG_HOP_GATE
    _lib.call("cuda", "srg_hop_scores_rows_f32", one, ld, r, 8, 1, 0, 1, G, None, None, None, 0, 4, st)
    _lib.call("cuda", "srg_hop_attend_rows_f32", one, ld, r, 8, 1, 0, 1, None, 0, None, None, 4, 0, 4, st)
    _lib.call("cuda", "srg_hop_attend_grad_rows_f32", one, ld, r, 8, 1, 0, 1, None, 4, None, None, 1, None, None, 0, 4, st)
    _lib.call("cuda", "srg_hop_recur_scores_rows_f32", one, ld, r, 8, 1, 1, None, None, None, 0, 4, st)
    _lib.call("cuda", "srg_hop_recur_attend_rows_f32", one, ld, r, 8, 1, 1, None, None, None, None, None, None, 4, 0, 4, st)
    _lib.call("cuda", "srg_hop_recur_attend_grad_rows_f32", one, ld, r, 8, 1, 1, None, 4, None, None, None, None, 0, 4, st)
    dw, db = torch.ones(8, device="cuda"), torch.ones(1, device="cuda")
    _lib.call("cuda", "srg_hop_scores_grad_rows_f32", one, ld, r, 8, 1, 0, 1, G, None, dw.data_ptr(), db.data_ptr(), None, 0, 4, st)
    assert not dw[:4].any() and not db.any()
    dw, db = torch.ones(8, device="cuda"), torch.ones(1, device="cuda")
    _lib.call("cuda", "srg_hop_recur_scores_grad_rows_f32", one, ld, r, 8, 1, 1, None, None, dw.data_ptr(), db.data_ptr(), None, 0, 4, st)
    assert not dw.any() and not db.any()

    x = torch.zeros((8, 4), device="cuda")
    w = torch.zeros(8, device="cuda")
    v, u = torch.zeros(8 * 33, device="cuda"), torch.zeros(8 * 33, device="cuda")
    many = (ctypes.c_void_p * 33)(*[x.data_ptr()] * 33)
    lds = (ctypes.c_int64 * 33)(*[4] * 33)
    X, W, V, U = x.data_ptr(), w.data_ptr(), v.data_ptr(), u.data_ptr()
    bad = [
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 33, 0, 33, G, X, V, V, 8, 4)),             # T > 32
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 4, 2, 2, G, X, V, V, 8, 4)),               # empty slice
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 4, 0, 5, G, X, V, V, 8, 4)),               # end > T
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 4, 0, 4, 3, X, V, V, 8, 4)),               # kind
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 4, 0, 4, G, X, V, V, 8, 5)),               # ld < d
        ("srg_hop_scores_rows_f32", (many, lds, r, 8, 4, 0, 4, G, None, V, V, 8, 4)),            # no weight
        ("srg_hop_scores_rows_f32", (many, lds, r, -1, 4, 0, 4, G, X, V, V, 8, 4)),              # n_src < 0
        ("srg_hop_attend_rows_f32", (many, lds, r, 8, 4, 0, 4, V, 0, U, X, 4, 8, 4)),            # out is a panel
        ("srg_hop_attend_rows_f32", (many, lds, r, 8, 4, 0, 4, V, 0, U, W, 3, 8, 4)),            # ldo < d
        ("srg_hop_attend_grad_rows_f32", (many, lds, r, 8, 4, 0, 4, X, 4, V, U, 0, U, V, 8, 4)),  # dzflat is zflat
        ("srg_hop_scores_grad_rows_f32", (many, lds, r, 8, 4, 0, 4, G, None, W, W, V, 8, 4)),    # no dzflat
        ("srg_hop_recur_scores_rows_f32", (many, lds, r, 8, 33, 4, W, V, U, 8, 4)),              # T > 32
        ("srg_hop_recur_scores_rows_f32", (many, lds, r, 8, 4, 0, W, V, U, 8, 4)),               # empty slice
        ("srg_hop_recur_scores_rows_f32", (many, lds, r, 8, 4, 4, W, V, V, 8, 4)),               # zp is zq
        ("srg_hop_recur_attend_rows_f32", (many, lds, r, 8, 4, 4, V, U, W, V, U, X, 4, 8, 4)),   # out is a panel
        ("srg_hop_recur_attend_grad_rows_f32", (many, lds, r, 8, 4, 4, X, 4, U, V, V, V, 8, 4)),  # dzp is dzq
        ("srg_hop_recur_scores_grad_rows_f32", (many, lds, r, 8, 4, 4, None, U, W, W, V, 8, 4)),  # no dzp
    ]
    for name, args in bad:
        with pytest.raises(_lib.SrgError):
            _lib.call("cuda", name, *args, st)


@pytest.mark.parametrize("d", [6, 65, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_out_of_range_indices_read_as_zero_rows(kind, d):
    """Every panel is 100 rows inside a 300-row buffer whose other rows hold 1e30; n_src = 100 is declared and the
    index holds 150 and -1 among valid entries, unchecked.  The result is, bit for bit, the gathered run in
    which those two batch rows are rows of +0.0, and nothing is non-finite or of the order of 1e30.  The panel
    starts at the buffer's row 1, so the rows the two indices would name if they were used as addresses (151
    and 0) are the buffer's own: no address this test could reach lies outside an allocation."""
    T, n_src = 4, 100
    k, start, end, hops, w, b = _case(kind, d, T, 4000 + d, n=n_src)
    feats = []
    for h in hops:
        buf = torch.full((300, d), 1e30, dtype=torch.float32, device="cuda")
        buf[1:1 + n_src] = torch.from_numpy(h).cuda()
        feats.append(buf[1:1 + n_src])
    idx = np.random.default_rng(d).integers(0, n_src, 77)
    idx[5], idx[40] = 150, -1
    bad = torch.from_numpy((idx < 0) | (idx >= n_src)).cuda()
    index = torch.from_numpy(idx).cuda()
    C = torch.from_numpy(_cotangent(idx.size, d, 9)).cuda()
    got = _run(k, feats, start, end, w, b, C, index=index, check=False)
    gathered = []
    for f in feats:
        g = f[index.clamp(0, n_src - 1)].contiguous()
        g[bad] = 0.0
        gathered.append(g)
    want = _run(k, gathered, start, end, w, b, C)
    for x, y, part in zip(got, want, ("out", "dw", "db")):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 1e6, f"{kind} d={d}: {part} saw the guard rows"
        assert np.array_equal(_bits(x), _bits(y)), f"{kind} d={d}: {part} differs from the run on zero rows"
    assert not got[0][bad].any()


def test_checked_index_raises_before_any_launch():
    from srgnn.hop_attention import hop_attention, hop_attention_recursive
    d, T = 6, 3
    _, _, _, hops, w, b = _case("jk", d, T, 77)
    feats = _windows(hops, 0)
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
    _, _, _, _, wr, br = _case("recursive", d, T, 78)
    wrd, brd = torch.from_numpy(wr).cuda(), torch.from_numpy(br).cuda()
    for wrong in (N_SRC, -N_SRC - 1):
        index = torch.tensor([3, wrong, 5], device="cuda")
        with pytest.raises(IndexError):
            hop_attention(feats, 0, T, "jk", wd, bd, index=index)
        with pytest.raises(IndexError):
            hop_attention_recursive(feats, T, wrd, brd, index=index)
    with pytest.raises(TypeError):
        hop_attention(feats, 0, T, "jk", wd, bd, index=torch.tensor([0.0, 1.0], device="cuda"))
    with pytest.raises(TypeError):
        hop_attention(feats, 0, T, "jk", wd, bd, index=torch.zeros((2, 2), dtype=torch.int64, device="cuda"))
    # negative indices wrap as in torch; an int32 index on the host is taken too
    neg = torch.tensor([-1, 4, -N_SRC, 299], dtype=torch.int32)
    out = hop_attention(feats, 0, T, "jk", wd, bd, index=neg)
    want = hop_attention([f[neg.long().cuda()].contiguous() for f in feats], 0, T, "jk", wd, bd)
    assert np.array_equal(_bits(out), _bits(want)) and out.shape == (4, d)
    # index gets no gradient; an empty index gives an empty output and zero gradients
    for fn, args in ((hop_attention, (feats, 0, T, "jk", wd, bd)), (hop_attention_recursive, (feats, T, wrd.requires_grad_(), brd.requires_grad_()))):
        empty = fn(*args, index=torch.zeros(0, dtype=torch.int64))
        assert empty.shape == (0, d)
        gw, gb = torch.autograd.grad(empty.sum(), args[-2:])
        assert not gw.any() and not gb.any() and gw.shape == args[-2].shape


def _op(kind, T, d, w, b, fused=True):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    start, end = _slice(kind, T)
    if kind == "recursive":
        op = IterateLearnableWeightedMessageOp(0, T, "recursive", d).cuda()
    else:
        k = "jk" if kind == "jk_inner" else kind
        op = LearnableWeightedMessageOp(start, end, k, *CTOR[k](T, d)).cuda()
    op.fused = fused
    with torch.no_grad():
        op.learnable_weight.weight.copy_(torch.as_tensor(w))
        op.learnable_weight.bias.copy_(torch.as_tensor(b))
    return op


@pytest.mark.parametrize("kind", KINDS)
def test_operators_aggregate_rows(kind):
    """fused: aggregate_rows is hop_attention(..., index=idx), and its parameter gradients are the gathered
    fused run's, bit for bit.  Not fused: exactly aggregate([f[idx] for f in feats])."""
    d, T = 65, 4
    k, start, end, hops, w, b = _case(kind, d, T, 5000)
    feats = _windows(hops, 0)
    idx = torch.from_numpy(_index_cases(N_SRC, 3)["shuffled129"]).cuda()
    C = torch.from_numpy(_cotangent(idx.numel(), d, 4)).cuda()
    op = _op(kind, T, d, w, b)
    out = op.aggregate_rows(list(feats), idx)
    assert type(out.grad_fn).__name__ in ("_HopAttentionBackward", "_HopAttentionRecursiveBackward"), "the device path did not run"
    out.backward(C)
    direct = _run(k, feats, start, end, w, b, C, index=idx)
    gathered = _run(k, [f[idx].contiguous() for f in feats], start, end, w, b, C)
    lin = op.learnable_weight
    assert lin.weight.grad.shape == lin.weight.shape and lin.bias.grad.shape == lin.bias.shape
    assert _same((out, lin.weight.grad, lin.bias.grad), direct)
    assert _same((lin.weight.grad, lin.bias.grad), gathered[1:])
    plain = _op(kind, T, d, w, b, fused=False)
    a = plain.aggregate_rows(list(feats), idx)
    assert "HopAttention" not in type(a.grad_fn).__name__
    a.backward(C)
    ga, gb = plain.learnable_weight.weight.grad.clone(), plain.learnable_weight.bias.grad.clone()
    plain.zero_grad(set_to_none=True)
    c = plain.aggregate([f[idx] for f in feats])
    c.backward(C)
    assert _same((a, ga, gb), (c, plain.learnable_weight.weight.grad, plain.learnable_weight.bias.grad))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["simple", "simple_allow_neg"])
def test_operators_aggregate_rows_of_the_kinds_without_a_device_path(kind, fused):
    from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp
    d, T = 6, 4
    hops = _case("gate", d, T, 5100)[3]
    feats = _windows(hops, 0)
    idx = torch.from_numpy(_index_cases(N_SRC, 3)["shuffled37"]).cuda()
    op = LearnableWeightedMessageOp(0, T, kind, T - 1).cuda()
    op.fused = fused
    a = op.aggregate_rows(list(feats), idx)
    c = op.aggregate([f[idx] for f in feats])
    assert a.shape == (37, d) and np.array_equal(_bits(a), _bits(c))


@pytest.mark.parametrize("fused", [False, True])
def test_recursive_operator_with_a_later_start_raises_through_aggregate_rows(fused):
    from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp
    hops = _case("recursive", 6, 4, 5200)[3]
    feats = _windows(hops, 0)
    late = IterateLearnableWeightedMessageOp(1, 4, "recursive", 6).cuda()
    late.fused = fused
    with pytest.raises(IndexError):
        late.aggregate_rows(list(feats), torch.arange(5, device="cuda"))


def test_peak_memory_without_the_gathered_copies():
    """jk, T = 11, d = 128, n_src = 100,000, B = 20,000: forward + backward under an index raise the peak by at
    least 0.9 T B d 4 bytes less than gather-then-fused does (the T copies it no longer makes; the 0.1 is the
    caching allocator's block rounding), and by less than T B d 4 bytes in all: no [B, d] per hop."""
    n_src, B, d, T = 100000, 20000, 128, 11
    gen = torch.Generator(device="cuda").manual_seed(5)
    feats = [torch.randn((n_src, d), device="cuda", generator=gen) for _ in range(T)]
    idx = torch.randperm(n_src, device="cuda", generator=gen)[:B]
    C = torch.randn((B, d), device="cuda", generator=gen)
    w = (torch.randn((1, R.in_dim("jk", T, d)), generator=torch.Generator().manual_seed(6)) * 0.02).numpy()
    b = np.array([0.1], dtype=np.float32)

    def indexed():
        return _run("jk", feats, 0, T, w, b, C, index=idx, check=False)

    def gathered():
        return _run("jk", [f[idx].contiguous() for f in feats], 0, T, w, b, C)

    rise = {}
    for name, fn in (("indexed", indexed), ("gathered", gathered)):
        _run("jk", [f[:64] for f in feats], 0, T, w, b, C[:64])        # library loaded, allocator warm
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        got = fn()
        torch.cuda.synchronize()
        rise[name] = torch.cuda.max_memory_allocated() - before
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        del got
    copies = T * B * d * 4
    print(f"peak rise in T*B*d*4 bytes: indexed {rise['indexed'] / copies:.3f}, gather-then-fused {rise['gathered'] / copies:.3f}")
    assert rise["gathered"] - rise["indexed"] >= 0.9 * copies
    assert rise["indexed"] < copies
