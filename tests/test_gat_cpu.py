"""srgnn.gat without a device: the fp64 restatement and its bound (tests/gat_ref.py) against the torch
composition and gradcheck, the negative controls, GATGraph's structure, and every argument check that
returns before a launch."""
import numpy as np
import pytest
import torch

import gat_ref as R
from srgnn import _lib
from srgnn import gat as GT

CASES = [(k, sl, H, C) for k in R.GRAPHS for sl in (False, True) for (H, C) in R.SHAPES]
_refs = {}


def reference(kind, sl, H, C):
    """(ip, ix, inputs, evaluate's result), computed once and never changed."""
    key = (kind, sl, H, C)
    if key not in _refs:
        ip, ix = R.graph(kind, sl)
        Hf, a_src, a_dst, G = R.inputs(R.N, H, C, R.case_seed(kind, sl, H, C))
        _refs[key] = (ip, ix, (Hf, a_src, a_dst, G), R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G))
    return _refs[key]


def composed(ip, ix, Hf, a_src, a_dst, G, dtype, slope=0.2):
    """out and the three gradients of the torch composition on the host in `dtype`, as numpy arrays."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (Hf, a_src, a_dst)]
    out = R.compose(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), *t, slope)
    out.backward(torch.from_numpy(np.asarray(G)).to(dtype))
    return dict(out=out.detach().numpy(), dHf=t[0].grad.numpy(), da_src=t[1].grad.numpy(), da_dst=t[2].grad.numpy())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize("kind,sl,H,C", CASES)
def test_restatement_equals_the_composition_in_fp64(kind, sl, H, C):
    ip, ix, (Hf, a_src, a_dst, G), ref = reference(kind, sl, H, C)
    got = composed(ip, ix, Hf, a_src, a_dst, G, torch.float64)
    for k, v in got.items():
        assert rel(v, ref[k]) <= 1e-12, k


def small_graph():
    rng = np.random.default_rng(3)
    dst, src = rng.integers(0, 12, 40), rng.integers(0, 12, 40)
    return R.csr_of(dst, src, 12, True)


def test_gradcheck_on_a_small_graph():
    ip, ix = small_graph()
    H, C = 2, 3
    Hf, a_src, a_dst, G = R.inputs(12, H, C, 4)
    tip, tix = torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64))
    t = [torch.from_numpy(a).double().requires_grad_(True) for a in (Hf, a_src, a_dst)]
    assert torch.autograd.gradcheck(lambda x, s, d: R.compose(tip, tix, x, s, d, 0.2), t, eps=1e-6, atol=1e-7)
    ref = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G)
    got = composed(ip, ix, Hf, a_src, a_dst, G, torch.float64)
    for k, v in got.items():
        assert rel(v, ref[k]) <= 1e-12, k


@pytest.mark.parametrize("kind,sl,H,C", CASES)
def test_fp32_composition_lies_within_the_bound(kind, sl, H, C):
    ip, ix, (Hf, a_src, a_dst, G), ref = reference(kind, sl, H, C)
    R.check(f"host fp32 {kind} loops={sl} H={H} C={C}", ref, composed(ip, ix, Hf, a_src, a_dst, G, torch.float32))


@pytest.mark.parametrize("kind,sl,H,C", CASES)
def test_no_entry_lies_in_the_leaky_relu_band(kind, sl, H, C):
    assert reference(kind, sl, H, C)[3]["band"] == 0


@pytest.mark.parametrize("kind,sl,H,C", CASES)
def test_negative_controls_leave_the_bound(kind, sl, H, C):
    ip, ix, (Hf, a_src, a_dst, G), ref = reference(kind, sl, H, C)
    wrong = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G, mistake="softmax_over_sources")
    assert R.worst_ratio(wrong["out"], ref["out"], ref["E_out"]) >= 50
    for mistake in ("no_D", "derivative_one"):
        wrong = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, G, mistake=mistake)
        assert R.worst_ratio(wrong["da_src"], ref["da_src"], ref["E_da_src"]) >= 50, mistake
        assert R.worst_ratio(wrong["da_dst"], ref["da_dst"], ref["E_da_dst"]) >= 50, mistake


def test_zero_score_takes_the_slope():
    """s = 0 exactly (zero attention halves): torch's leaky_relu has the derivative `slope` there, and so has
    the restatement (autograd's own convention, in fp64)."""
    ip, ix = R.graph("asym", True)
    H, C = 2, 5
    Hf, _, _, G = R.inputs(R.N, H, C, 9)
    zero = np.zeros((R.N, H), dtype=np.float32)
    ref = R.evaluate(ip, ix, Hf, zero, zero, 0.2, G)
    got = composed(ip, ix, Hf, zero, zero, G, torch.float64)
    assert ref["band"] == ix.size * H                      # every entry sits on the kink: pinned, not bounded
    assert rel(got["da_src"], ref["da_src"]) <= 1e-12
    # with one derivative for every entry of a row, da_dst = slope * sum_e alpha_e (dalpha_e - D) = 0
    assert np.abs(got["da_dst"]).max() <= 1e-12 and np.abs(ref["da_dst"]).max() <= 1e-12
    one = R.evaluate(ip, ix, Hf, zero, zero, 0.2, G, mistake="derivative_one")
    assert rel(one["da_src"], ref["da_src"]) > 1.0


def test_pinned_restatements_agree_with_the_formula():
    ip, ix = R.graph("sym", False)
    Hf = R.inputs(R.N, 3, 7, 12)[0]
    zero = np.zeros((R.N, 3), dtype=np.float32)
    ref = R.evaluate(ip, ix, Hf, zero, zero)
    assert R.worst_ratio(R.zero_att_ref(ip, ix, Hf), ref["out"], ref["E_out"]) <= 1.0
    loops = np.arange(R.N, dtype=np.int32)
    assert np.array_equal(R.single_entry_ref(loops, Hf), Hf)


# ---- GATGraph ---------------------------------------------------------------------------------------
def messy_edges():
    """Unsorted, with existing self-loops and duplicate pairs (a duplicate self-loop too)."""
    rng = np.random.default_rng(8)
    n = 30
    dst, src = rng.integers(0, n, 150), rng.integers(0, n, 150)
    dst, src = np.r_[dst, dst[:20], 4, 4, 9], np.r_[src, src[:20], 4, 4, 9]
    return n, dst, src


def test_self_loops_against_scipy():
    import scipy.sparse as sp
    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n)
    ip, ix = R.csr_of(dst, src, n, True)
    assert g.has_self_loops and np.array_equal(g.indptr.numpy(), ip) and np.array_equal(g.indices.numpy(), ix)
    # scipy's own words for it: drop the diagonal, add the identity, sort the rows; scipy merges duplicates,
    # so the structures agree as sets and the duplicates are counted apart
    A = sp.coo_matrix((np.ones(dst.size), (dst, src)), shape=(n, n)).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A = (A + sp.identity(n, format="csr")).tocsr()
    A.sort_indices()
    rows = R.entry_rows(ip)
    keys = rows * n + ix
    assert np.array_equal(np.unique(keys), R.entry_rows(A.indptr) * n + A.indices)
    off = dst != src
    assert keys.size == int(off.sum()) + n                  # every off-diagonal duplicate kept, one loop per node
    assert (np.diff(keys) >= 0).all()                       # rows sorted by source
    # the same structure through the other constructors
    B = sp.csr_matrix((np.ones(ix.size), ix, ip), shape=(n, n))
    for other in (GT.GATGraph.from_scipy(B), GT.GATGraph.from_scipy(B, add_self_loops=False)):
        assert np.array_equal(other.indptr.numpy(), ip) and np.array_equal(other.indices.numpy(), ix)
    coo = torch.sparse_coo_tensor(torch.from_numpy(np.stack([dst, src])), torch.ones(dst.size), (n, n))
    t = GT.GATGraph.from_torch_sparse(coo)
    assert np.array_equal(t.indptr.numpy(), A.indptr) and np.array_equal(t.indices.numpy(), A.indices)


def test_without_self_loops_the_stored_order_is_kept():
    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(torch.from_numpy(np.stack([src, dst])), n, add_self_loops=False)
    ip, ix = R.csr_of(dst, src, n, False)
    assert not g.has_self_loops
    assert np.array_equal(g.indptr.numpy(), ip) and np.array_equal(g.indices.numpy(), ix)
    assert g.nnz == dst.size


def test_empty_graphs():
    for n in (0, 5):
        for sl in (False, True):
            g = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), n, add_self_loops=sl)
            assert g.nnz == (n if sl else 0) and g.indptr.numel() == n + 1 and g.perm.numel() == g.nnz
            assert g.indptr_t.numel() == n + 1 and g.indptr.dtype == torch.int64 and g.indices.dtype == torch.int32


@pytest.mark.parametrize("sl", (False, True))
def test_transpose_and_perm_follow_csr_transpose(sl):
    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n, add_self_loops=sl)
    tp, tx, perm = R.transpose_of(g.indptr.numpy(), g.indices.numpy(), n)
    assert np.array_equal(g.indptr_t.numpy(), tp) and np.array_equal(g.indices_t.numpy(), tx)
    assert np.array_equal(g.perm.numpy(), perm)
    # entry t of At is entry perm[t] of A: its source is the row of At, its target the stored id
    rows_t = R.entry_rows(tp)
    assert np.array_equal(g.indices.numpy()[perm], rows_t)
    assert np.array_equal(R.entry_rows(g.indptr.numpy())[perm], tx)


def test_constructor_checks():
    with pytest.raises(ValueError):
        GT.GATGraph.from_edge_index(np.array([[0, 5], [1, 1]]), 5)
    with pytest.raises(ValueError):
        GT.GATGraph.from_edge_index(np.array([[0, -1], [1, 1]]), 5)
    with pytest.raises(ValueError):
        GT.GATGraph.from_edge_index(np.zeros((3, 4), dtype=np.int64), 5)
    with pytest.raises(TypeError):
        GT.GATGraph.from_scipy(np.eye(3))
    with pytest.raises(TypeError):
        GT.GATGraph.from_torch_sparse(torch.eye(3))
    with pytest.raises(TypeError):
        GT.GATGraph.from_device_csr(object())


# ---- argument checks --------------------------------------------------------------------------------
def test_gat_attend_argument_checks():
    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n)
    Hf, a = torch.zeros(n, 6), torch.zeros(n, 2)
    with pytest.raises(TypeError):
        GT.gat_attend(object(), Hf, a, a)
    with pytest.raises(TypeError, match="fp32"):
        GT.gat_attend(g, Hf.double(), a, a)
    with pytest.raises(TypeError, match="fp32"):
        GT.gat_attend(g, Hf, a.half(), a)
    with pytest.raises(ValueError):
        GT.gat_attend(g, Hf[:-1], a, a)
    with pytest.raises(ValueError):
        GT.gat_attend(g, Hf, a, torch.zeros(n, 3))
    with pytest.raises(ValueError, match="multiple"):
        GT.gat_attend(g, torch.zeros(n, 7), a, a)
    with pytest.raises(ValueError, match="heads"):
        GT.gat_attend(g, torch.zeros(n, 66), torch.zeros(n, 33), torch.zeros(n, 33))
    with pytest.raises(ValueError, match="exceeds"):
        GT.gat_attend(g, torch.zeros(n, _lib.SRG_GAT_MAX_WIDTH + 2), a, a)
    with pytest.raises(ValueError, match="finite"):
        GT.gat_attend(g, Hf, a, a, float("nan"))
    with pytest.raises(RuntimeError, match="HIP device"):       # no fall-back to the host
        GT.gat_attend(g, Hf, a, a)


def test_layer_checks_names_and_shapes():
    conv = GT.GATConv(10, 4, heads=3)
    shapes = {k: tuple(v.shape) for k, v in conv.named_parameters()}
    assert shapes == {"att_src": (1, 3, 4), "att_dst": (1, 3, 4), "bias": (12,), "lin.weight": (12, 10)}
    assert set(conv.state_dict()) == set(shapes)
    assert not conv.bias.detach().any()
    lim = np.sqrt(6.0 / (12 + 10))
    assert float(conv.lin.weight.detach().abs().max()) <= lim
    assert float(conv.att_src.detach().abs().max()) <= np.sqrt(6.0 / 7)
    mean = GT.GATConv(10, 4, heads=3, concat=False, bias=True)
    assert tuple(mean.bias.shape) == (4,)
    assert GT.GATConv(10, 4, bias=False).bias is None
    model = GT.GAT(10, 8, 5, 3, 0.5, 2)
    assert [tuple(c.lin.weight.shape) for c in model.convs] == [(16, 10), (16, 16), (5, 16)]
    assert [c.heads for c in model.convs] == [2, 2, 1]
    for bad in (dict(heads=0), dict(heads=33), dict(dropout=1.0), dict(heads=32, out_channels=4096)):
        kw = dict(in_channels=4, out_channels=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            GT.GATConv(**kw)
    with pytest.raises(ValueError):
        GT.GAT(4, 4, 4, 1, 0.0, 2)

    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n)
    plain = GT.GATGraph.from_edge_index(np.stack([src, dst]), n, add_self_loops=False)
    x = torch.zeros(n, 10)
    with pytest.raises(ValueError, match="add_self_loops"):
        conv(x, plain)
    with pytest.raises(ValueError, match="add_self_loops"):
        GT.GATConv(10, 4, add_self_loops=False)(x, g)
    with pytest.raises(TypeError):
        conv(x, None)
    with pytest.raises(ValueError):
        conv(torch.zeros(n, 9), g)


def test_attention_dropout_is_not_implemented():
    n, dst, src = messy_edges()
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n)
    conv = GT.GATConv(10, 4, heads=2, dropout=0.6)
    with pytest.raises(NotImplementedError, match="dropout"):
        conv(torch.zeros(n, 10), g)
    conv.eval()
    with pytest.raises(RuntimeError, match="HIP device"):       # eval mode passes the dropout check
        conv(torch.zeros(n, 10), g)


def test_entries_are_bound_and_reject_bad_sizes():
    """The C entries' argument checks return before any HIP call."""
    L = _lib.lib()
    E = _lib.SRG_ERR_INVALID
    for name in ("srg_gat_attend_f32", "srg_gat_edge_grad_f32", "srg_gat_attend_adjoint_f32"):
        assert name in _lib.EXPORTED_SYMBOLS

    def attend(nnz=8, n=4, ns=4, ldh=8, H=2, C=4, ldo=8):
        return L.srg_gat_attend_f32(None, None, nnz, n, ns, None, None, 0.2, None, ldh, H, C, None, ldo, None, None, None)

    def edge(nnz=8, n=4, ns=4, ldh=8, H=2, C=4, ldo=8, ldg=8):
        return L.srg_gat_edge_grad_f32(None, None, nnz, n, ns, None, None, 0.2, None, ldh, H, C, None, ldo, None, None,
                                       None, ldg, None, None, None, None)

    def adjoint(nnz=8, n=4, ns=4, H=2, C=4):
        return L.srg_gat_attend_adjoint_f32(None, None, None, nnz, n, ns, None, None, 0.2, H, C, None, None, None, 8,
                                            None, None, 8, None, None)

    for fn in (attend, edge, adjoint):
        assert fn(H=0) == E and fn(H=_lib.SRG_GAT_MAX_HEADS + 1) == E
        assert "H=" in _lib.last_error()
        assert fn(C=0) == E
        assert fn(H=32, C=_lib.SRG_GAT_MAX_WIDTH // 32 + 1) == E
        assert fn(n=-1) == E and fn(ns=-1) == E and fn(nnz=-1) == E and fn(n=2 ** 31) == E
    assert attend(ldh=7) == E and "ldh" in _lib.last_error()
    assert attend(ldo=7) == E and edge(ldg=7) == E and edge(ldo=7) == E and edge(ldh=7) == E
    assert attend() == E and "null" in _lib.last_error()        # no output to write
    assert edge() == E
    assert attend(n=0) == _lib.SRG_OK and edge(n=0) == _lib.SRG_OK and adjoint(ns=0) == _lib.SRG_OK
    assert adjoint() == _lib.SRG_OK                             # neither result asked for


def test_two_layer_bound_holds_for_the_fp32_composition_on_the_host():
    """The composed two-layer bound (gat_ref.two_layer_bound) checked without a device: the GAT model with the
    fp32 torch composition as its aggregation against the same model with the fp64 composition, logits and all
    eight parameter gradients; no ReLU input and no score in its kink band."""
    n = R.MODEL_N
    dst, src = R.model_edges()
    ip, ix = R.csr_of(dst, src, n, True)
    g = GT.GATGraph.from_edge_index(np.stack([src, dst]), n)
    models = []
    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(R.MODEL_SEED)
        m = GT.GAT(19, 8, 5, 2, 0.0, 4)
        for conv in m.convs:
            conv.__class__ = R.composed_conv(dtype)
        models.append(m)
    ours, theirs = models
    with torch.no_grad():
        for conv in ours.convs:
            conv.bias.uniform_(-0.5, 0.5)
    theirs.load_state_dict(ours.state_dict())
    x = torch.from_numpy(np.random.default_rng(22).standard_normal((n, 19)).astype(np.float32))
    Cot = np.random.default_rng(23).standard_normal((n, 5)).astype(np.float32)
    y, y2 = ours(x, g), theirs(x, g)
    (y * torch.from_numpy(Cot)).sum().backward()
    (y2 * torch.from_numpy(Cot)).sum().backward()
    L1, L2 = R.model_layers(ours, x, lambda conv, Hf, a_s, a_d: conv._aggregate(g, Hf, a_s, a_d))
    bound = R.two_layer_bound(ip, ix, x.numpy(), L1, L2, Cot)
    R.check_model("host fp32 composition", bound, y, y2, list(ours.named_parameters()), list(theirs.named_parameters()))
    # the bound is a bound on rounding, not on mistakes: a first layer with the slope 0.3 leaves it, the logits by
    # a factor >= 50 and every parameter gradient by > 2 (the gradients' bounds sum worst cases over n rows and
    # two dense stages and are looser than the logits': 5 to 285 times here)
    for q in theirs.parameters():
        q.grad = None
    theirs.convs[0].negative_slope = 0.3
    y3 = theirs(x, g)
    (y3 * torch.from_numpy(Cot)).sum().backward()
    assert R.worst_ratio(y.detach().numpy(), y3.detach().numpy().astype(np.float64), bound["logits"]) >= 50
    for (k, p), (_, q) in zip(ours.named_parameters(), theirs.named_parameters()):
        assert R.worst_ratio(p.grad.numpy(), q.grad.numpy().astype(np.float64), bound["grads"][k]) > 2, k
