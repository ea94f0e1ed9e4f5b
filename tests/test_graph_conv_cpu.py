"""srgnn.graph_conv without a device: the host restatement of the two row-restricted entries against
oracle.spmm, the fixture (the reference's own torch.mm path) against the restatement within the derived
bound, and the wrapper's argument checks that run before anything touches a device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graph_conv_ref as R
from oracle import oracle as O
from srgnn import _lib
from srgnn import graph_conv as GC


def _shuffled(n, B, seed):
    return np.random.default_rng(seed).permutation(n)[:B].astype(np.int64)


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_rows_forward_ref_is_the_oracle_rows(name, d):
    ip, ix, v = R.case(name)
    n = ip.size - 1
    Z, _ = R.panels(d)
    full = O.spmm(ip, ix, v, Z)
    for B in (0, 1, 63, 64, 65, n):
        rows = _shuffled(n, B, 100 + B)
        got = R.rows_forward_ref(ip, ix, v, rows, Z)
        assert got.shape == (B, d)
        assert np.array_equal(got.view(np.int32), full[rows].view(np.int32))
    # ids outside [0, n): a row of +0, sign bit clear
    got = R.rows_forward_ref(ip, ix, v, np.array([-1, 5, n]), Z)
    assert np.array_equal(got[[0, 2]].view(np.int32), np.zeros((2, d), np.int32))
    assert np.array_equal(got[1].view(np.int32), full[5].view(np.int32))


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_rows_adjoint_ref_of_every_row_is_the_transposed_product(name, d):
    ip, ix, v = R.case(name)
    n = ip.size - 1
    _, G = R.panels(d)
    tp, tx, tv = R.transpose_stable(ip, ix, v, n)
    # the stable sort by column is the transpose
    A = sp.csr_matrix((v, ix, ip), shape=(n, n))
    assert (sp.csr_matrix((tv, tx, tp), shape=(n, n)) != A.T).nnz == 0
    want = O.spmm(tp, tx, tv, G)
    got = R.rows_adjoint_ref(tp, tx, tv, np.arange(n, dtype=np.int32), G)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # a shuffled full batch: the same rows of G through pos
    rows = _shuffled(n, n, 9)
    got = R.rows_adjoint_ref(tp, tx, tv, R.pos_of(rows, n), G[rows])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_rows_adjoint_ref_skips_and_scatter_agree():
    """On a finite operator the skipping chain equals the full chain over G scattered into n rows of +0; an
    empty batch gives +0 with the sign bit clear; an Inf outside the batch never enters."""
    ip, ix, v = R.star_graph()
    n = ip.size - 1
    tp, tx, tv = R.transpose_stable(ip, ix, v, n)
    rng = np.random.default_rng(3)
    rows = np.r_[7, 3, _shuffled(n, 80, 4)]
    rows = rows[np.sort(np.unique(rows, return_index=True)[1])]
    G = rng.standard_normal((rows.size, 7)).astype(np.float32)
    pos = R.pos_of(rows, n)
    got = R.rows_adjoint_ref(tp, tx, tv, pos, G)
    scattered = np.zeros((n, 7), np.float32)
    scattered[rows] = G
    assert np.array_equal(got.view(np.int32), O.spmm(tp, tx, tv, scattered).view(np.int32))
    empty = R.rows_adjoint_ref(tp, tx, tv, np.full(n, -1, np.int32), np.zeros((0, 7), np.float32))
    assert np.array_equal(empty.view(np.int32), np.zeros((n, 7), np.int32))
    outside = np.flatnonzero(pos[tx] < 0)
    tv_inf = tv.copy()
    tv_inf[outside[0]] = np.inf
    assert np.array_equal(R.rows_adjoint_ref(tp, tx, tv_inf, pos, G).view(np.int32), got.view(np.int32))
    assert not np.isfinite(O.spmm(tp, tx, tv_inf, scattered)).all()      # multiplying by zero would not do


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_fixture_within_the_bound_of_the_restatement(name, d):
    """The reference's torch.mm and its autograd against the fma chains: 2 gamma_len sum |v||z|."""
    g = R.golden()
    ip, ix, v = R.case(name)
    n = ip.size - 1
    Z, G = R.panels(d)
    err = np.abs(O.spmm(ip, ix, v, Z).astype(np.float64) - g[f"{name}__Y{d}"].astype(np.float64))
    assert (err <= R.chain_bound(ip, ix, v, Z)).all()
    tp, tx, tv = R.transpose_stable(ip, ix, v, n)
    err = np.abs(O.spmm(tp, tx, tv, G).astype(np.float64) - g[f"{name}__dZ{d}"].astype(np.float64))
    assert (err <= R.chain_bound(tp, tx, tv, G)).all()


def test_fixture_operators_are_the_three_kinds():
    for name in R.CASES:
        ip, ix, v = R.case(name)
        n = ip.size - 1
        tp, tx, tv = R.transpose_stable(ip, ix, v, n)
        sym = np.array_equal(tp, ip) and np.array_equal(tx, ix)
        same = sym and np.array_equal(tv.view(np.int32), v.view(np.int32))
        assert {"same": same, "mirrored": sym and not same, "sorted": not sym}[R.KINDS[name]]
        rows = R.entry_rows(ip)
        key = rows * n + ix
        assert (key[1:] > key[:-1]).all()                     # coalesced: sorted, unique


# ---- the wrapper, before any device -----------------------------------------------------------------
def test_batch_rows_on_the_host():
    ids, pos, unique = GC.batch_rows(range(2, 7), 10)
    assert ids.dtype == torch.int64 and ids.tolist() == [2, 3, 4, 5, 6] and unique
    assert pos.dtype == torch.int32 and pos.tolist() == [-1, -1, 0, 1, 2, 3, 4, -1, -1, -1]
    ids, pos, unique = GC.batch_rows([-1, 0, -10], 10)
    assert ids.tolist() == [9, 0, 0] and not unique
    ids, pos, unique = GC.batch_rows(torch.tensor([4, 1], dtype=torch.int32), 5)
    assert ids.dtype == torch.int64 and unique and pos.tolist() == [-1, 1, -1, -1, 0]
    ids, pos, unique = GC.batch_rows([], 5)
    assert ids.numel() == 0 and unique and pos.tolist() == [-1] * 5
    for bad in ([10], [-11], np.array([0, 3, 12])):
        with pytest.raises(IndexError):
            GC.batch_rows(bad, 10)
    with pytest.raises(TypeError):
        GC.batch_rows(torch.tensor([0.5]), 10)
    with pytest.raises(TypeError):
        GC.batch_rows(torch.tensor([True, False]), 10)
    with pytest.raises(ValueError):
        GC.batch_rows(torch.zeros((2, 2), dtype=torch.int64), 10)


def test_argument_checks_without_a_device():
    X = torch.zeros(4, 3)
    with pytest.raises(TypeError):
        GC.graph_conv("not an operator", X)
    with pytest.raises(TypeError):
        GC.GraphConvOperator(object())
    with pytest.raises(TypeError):
        GC.GraphConvOperator.from_scipy(np.eye(3))
    with pytest.raises(TypeError):
        GC.GraphConvOperator.from_torch_sparse(torch.eye(3))
    with pytest.raises(TypeError):
        GC.GraphConvOperator.from_torch_sparse(torch.eye(3, dtype=torch.float64).to_sparse())
    assert "__eq__" not in vars(GC.GraphConvOperator)


def test_layer_has_the_reference_parameter_names():
    layer = GC.GraphConvolution2(5, 8, 3, dropout=0.0)
    assert sorted(layer.state_dict()) == sorted(
        f"{m}.{p}" for m in ("fc1_node_edge", "fc2_node", "fc2_edge", "linear") for p in ("weight", "bias"))
    assert layer.adj is None and layer.query_edges is None
    assert tuple(layer.linear.weight.shape) == (3, 16) and tuple(layer.fc2_edge.weight.shape) == (8, 8)
    with pytest.raises(TypeError):
        layer(torch.zeros(4, 5))


def test_entries_are_bound_and_reject_bad_sizes():
    """The C entries' argument checks return before any HIP call."""
    L = _lib.lib()
    for name in ("srg_gconv_rows_f32", "srg_gconv_rows_adjoint_f32"):
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert len(fn.argtypes) == 12
        # (ip, ix, v, n, rows | pos, B, X | G, ld, Y | dX, ld, d, stream)
        assert fn(None, None, None, -1, None, 0, None, 4, None, 4, 4, None) == _lib.SRG_ERR_INVALID
        assert fn(None, None, None, 4, None, -1, None, 4, None, 4, 4, None) == _lib.SRG_ERR_INVALID
        assert fn(None, None, None, 4, None, 2, None, 3, None, 4, 4, None) == _lib.SRG_ERR_INVALID
        assert "< d=4" in _lib.last_error()
        assert fn(None, None, None, 4, None, 2, None, 4, None, 3, 4, None) == _lib.SRG_ERR_INVALID
        assert fn(None, None, None, 4, None, 2, None, 4, None, 4, -1, None) == _lib.SRG_ERR_INVALID
        assert fn(None, None, None, 0, None, 0, None, 4, None, 4, 0, None) == _lib.SRG_OK
