"""srgnn.gat's rows= without a device: the argument checks of gat_attend, GATConv, GAT and the three rows
entries that return before a launch, batch_rows' repeated-id path as gat_attend uses it, and the fp64 rows
reference (tests/gat_rows_ref.py) against gat_ref.evaluate under the padded cotangent."""
import numpy as np
import pytest
import torch

import gat_ref as R
import gat_rows_ref as RR
from srgnn import _lib
from srgnn import gat as GT


def small():
    rng = np.random.default_rng(8)
    n = 30
    dst, src = rng.integers(0, n, 150), rng.integers(0, n, 150)
    return n, GT.GATGraph.from_edge_index(np.stack([src, dst]), n)


# ---- argument checks --------------------------------------------------------------------------------
def test_gat_attend_checks_rows_before_the_device():
    n, g = small()
    Hf, a = torch.zeros(n, 6), torch.zeros(n, 2)
    with pytest.raises(IndexError):
        GT.gat_attend(g, Hf, a, a, rows=[0, n])
    with pytest.raises(IndexError):
        GT.gat_attend(g, Hf, a, a, rows=torch.tensor([-n - 1]))
    with pytest.raises(TypeError, match="integer"):
        GT.gat_attend(g, Hf, a, a, rows=torch.tensor([0.0, 1.0]))
    with pytest.raises(TypeError, match="integer"):
        GT.gat_attend(g, Hf, a, a, rows=torch.tensor([True, False]))
    with pytest.raises(ValueError, match="1-D"):
        GT.gat_attend(g, Hf, a, a, rows=torch.zeros((2, 2), dtype=torch.int64))
    # the other operands are checked as without rows
    with pytest.raises(TypeError, match="fp32"):
        GT.gat_attend(g, Hf.double(), a, a, rows=[0])
    with pytest.raises(ValueError):
        GT.gat_attend(g, Hf[:-1], a, a, rows=[0])
    # good ids of every accepted kind reach the device check: no fall-back to the host
    for rows in ([0, 3], range(0, 10, 2), torch.tensor([1, -1]), np.array([2, 5]), torch.tensor([4], dtype=torch.int32), []):
        with pytest.raises(RuntimeError, match="HIP device"):
            GT.gat_attend(g, Hf, a, a, rows=rows)
    with pytest.raises(RuntimeError, match="HIP device"):
        GT.attend_forward(g, Hf, a, a, rows=[0, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        GT.attend_backward(g, Hf, a, a, Hf[:2], a[:2], a[:2], Hf[:2], rows=[0, 1])
    with pytest.raises(IndexError):
        GT.attend_forward(g, Hf, a, a, rows=[n])


def test_layer_and_model_pass_rows_down():
    n, g = small()
    conv = GT.GATConv(10, 4, heads=3)
    x = torch.zeros(n, 10)
    with pytest.raises(IndexError):
        conv(x, g, rows=[n])
    with pytest.raises(IndexError):
        conv(x, g, [0, -n - 1])
    with pytest.raises(TypeError, match="integer"):
        conv(x, g, rows=[0.5])
    with pytest.raises(RuntimeError, match="HIP device"):
        conv(x, g, rows=[0, 1])
    with pytest.raises(ValueError):                           # the layer's own checks come first
        conv(torch.zeros(n, 9), g, rows=[0])
    model = GT.GAT(10, 8, 5, 2, 0.0, 2)
    with pytest.raises(RuntimeError, match="HIP device"):     # the first layer runs over all nodes
        model(x, g, rows=[n])

    class Last(GT.GATConv):                                   # a last layer alone sees the ids
        def _aggregate(self, graph, Hf, a_src, a_dst):
            return torch.zeros_like(Hf)

    model.convs[0].__class__ = Last
    with pytest.raises(IndexError):
        model(x, g, rows=[n])
    with pytest.raises(RuntimeError, match="HIP device"):
        model(x, g, rows=[1, 2])


def test_repeated_ids_are_computed_once():
    """gat_attend's use of batch_rows: a repeat makes `unique` False, the batch then holds torch.unique's ids
    and the inverse indexes them back."""
    n, g = small()
    batch, inverse = GT._batch_of(g, [5, 2, 5, -1, 2])
    assert batch.ids.tolist() == [2, 5, n - 1] and inverse.tolist() == [1, 0, 1, 2, 0]
    assert batch.ids[inverse].tolist() == [5, 2, 5, n - 1, 2]
    pos = batch.pos.tolist()
    assert [pos[2], pos[5], pos[n - 1]] == [0, 1, 2] and sorted(pos)[:n - 3] == [-1] * (n - 3)
    assert batch.pos.dtype == torch.int32 and batch.pos.numel() == n and batch.ids.dtype == torch.int64
    batch, inverse = GT._batch_of(g, [5, 2, -1])
    assert inverse is None and batch.ids.tolist() == [5, 2, n - 1] and batch.B == 3
    eptr, nnzB = batch.eptr()
    ip = g.indptr.numpy()
    assert np.array_equal(eptr.numpy(), RR.eptr_of(ip, batch.ids.numpy())) and nnzB == int(eptr[-1])
    again, _ = GT._batch_of(g, batch)
    assert again is batch
    with pytest.raises(ValueError, match="another graph"):
        GT._batch_of(small()[1], batch)
    with pytest.raises(ValueError, match="unique"):
        GT._unique_batch(*GT._batch_of(g, [1, 1]), "attend_forward")
    empty, inverse = GT._batch_of(g, [])
    assert empty.B == 0 and inverse is None and empty.eptr()[0].tolist() == [0] and empty.eptr()[1] == 0


def test_entries_are_bound_and_reject_bad_sizes():
    """The rows entries' argument checks return before any HIP call."""
    L = _lib.lib()
    E = _lib.SRG_ERR_INVALID
    for name in ("srg_gat_attend_rows_f32", "srg_gat_edge_grad_rows_f32", "srg_gat_attend_rows_adjoint_f32"):
        assert name in _lib.EXPORTED_SYMBOLS

    def attend(nnz=8, n=4, ns=4, B=2, ldh=8, H=2, C=4, ldo=8):
        return L.srg_gat_attend_rows_f32(None, None, nnz, n, ns, None, B, None, None, 0.2, None, ldh, H, C, None, ldo,
                                         None, None, None)

    def edge(nnz=8, n=4, ns=4, B=2, nnzB=3, ldh=8, H=2, C=4, ldo=8, ldg=8):
        return L.srg_gat_edge_grad_rows_f32(None, None, nnz, n, ns, None, B, None, nnzB, None, None, 0.2, None, ldh, H,
                                            C, None, ldo, None, None, None, ldg, None, None, None, None)

    def adjoint(nnz=8, n=4, ns=4, B=2, nnzB=3, H=2, C=4):
        return L.srg_gat_attend_rows_adjoint_f32(None, None, None, nnz, n, ns, None, B, None, None, nnzB, None, None,
                                                 0.2, H, C, None, None, None, 8, None, None, 8, None, None)

    for fn in (attend, edge, adjoint):
        assert fn(H=0) == E and fn(H=_lib.SRG_GAT_MAX_HEADS + 1) == E
        assert "H=" in _lib.last_error()
        assert fn(C=0) == E
        assert fn(H=32, C=_lib.SRG_GAT_MAX_WIDTH // 32 + 1) == E
        assert fn(n=-1) == E and fn(ns=-1) == E and fn(nnz=-1) == E and fn(n=2 ** 31) == E
        assert fn(B=-1) == E and "B=" in _lib.last_error()
        assert fn(B=2 ** 31) == E
    assert edge(nnzB=-1) == E and "nnzB" in _lib.last_error()
    assert adjoint(nnzB=-1) == E
    assert attend(ldh=7) == E and "ldh" in _lib.last_error()
    assert attend(ldo=7) == E and edge(ldg=7) == E and edge(ldo=7) == E and edge(ldh=7) == E
    assert attend() == E and "null" in _lib.last_error()        # no output to write
    assert edge() == E
    assert attend(B=0) == _lib.SRG_OK and edge(B=0) == _lib.SRG_OK and adjoint(ns=0) == _lib.SRG_OK
    assert adjoint() == _lib.SRG_OK                             # neither result asked for


def test_pos_must_cover_the_graph():
    """The Python side hands the adjoint a pos of n entries: batch_rows builds it for the graph's n, and a batch
    made for another graph is refused."""
    n, g = small()
    batch, _ = GT._batch_of(g, range(0, n, 3))
    assert batch.pos.numel() == g.n
    other = GT.GATGraph.from_edge_index(np.zeros((2, 0), dtype=np.int64), n + 1)
    with pytest.raises(ValueError, match="another graph"):
        GT.gat_attend(other, torch.zeros(n + 1, 6), torch.zeros(n + 1, 2), torch.zeros(n + 1, 2), rows=batch)


# ---- the fp64 rows reference ------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize("name", RR.BATCHES)
@pytest.mark.parametrize("kind,sl", RR.GRAPHS)
def test_rows_reference_equals_the_formula_under_the_padded_cotangent(kind, sl, name):
    H, C = 3, 7
    ip, ix = R.graph(kind, sl)
    Hf, a_src, a_dst, G = R.inputs(R.N, H, C, R.case_seed(kind, sl, H, C))
    rows = RR.batch(name, kind, sl)
    assert np.unique(rows).size == rows.size
    Gb = G[rows]
    full = R.evaluate(ip, ix, Hf, a_src, a_dst, 0.2, RR.pad(Gb, rows, R.N))
    assert full["band"] == 0
    want = RR.index_ref(full, rows, ip)
    got = RR.evaluate_rows(ip, ix, Hf, a_src, a_dst, rows, 0.2, Gb)
    assert got["band"] == 0
    for k in ("out", "M", "Z", "da_dst", "dHf", "da_src"):
        assert got[k].shape == want[k].shape and rel(got[k], want[k]) <= 1e-12, k
        assert (got["E_" + k] <= want["E_" + k] * (1 + 1e-12) + 1e-300).all(), k    # fewer terms, no looser
    assert rel(got["ds"], full["ds"][RR.entries_of(ip, rows)]) <= 1e-12
    eptr = RR.eptr_of(ip, rows)
    assert got["ds"].shape == (eptr[-1], H) and got["out"].shape == (rows.size, H * C)
    # outside the batch the padded full backward's da_dst and ds vanish
    outside = np.setdiff1d(np.arange(R.N), rows)
    assert not full["da_dst"][outside].any()
    member = np.zeros(R.N, bool)
    member[rows] = True
    assert not full["ds"][~member[R.entry_rows(ip)]].any()


def test_the_named_batches_hold_what_they_say():
    for kind, sl in RR.GRAPHS:
        ip, ix = R.graph(kind, sl)
        mixed = RR.batch("mixed37", kind, sl)
        nb = RR.star_neighbour(kind, sl)
        assert mixed.size == 37 and {R.STAR, R.ISOLATED[0], nb} <= set(mixed.tolist())
        assert nb in ix[ip[R.STAR]:ip[R.STAR + 1]] and not np.array_equal(mixed, np.sort(mixed))
        assert RR.batch("past_blocks129", kind, sl).size == 129 and 129 % 4 == 1
        assert ip[R.STAR + 1] - ip[R.STAR] >= 320
        if not sl:
            assert ip[R.ISOLATED[0] + 1] == ip[R.ISOLATED[0]]
