"""srgnn.link without a device: EdgeBatch against the restated relabelling (tests/link_ref.py) with every error
case, the CPU path of pair_linear under gradcheck in fp64 and within the derived bounds of DESIGN.md 5.14 in fp32,
the loader, edge_head's fallback under training dropout, and the two new entries in the header and the binding."""
import re

import numpy as np
import pytest
import torch
from torch import nn

import link_ref as LR
from srgnn import link as LK

N = 23


def edge_cases():
    """name -> pairs over N nodes."""
    rng = np.random.default_rng(3)
    return {
        "empty": np.zeros((0, 2), dtype=np.int64),
        "one": np.array([[5, 2]]),
        "self_pair": np.array([[4, 4], [1, 4], [9, 9]]),
        "repeated": np.array([[3, 7], [3, 7], [7, 3], [3, 7]]),
        "one_sided": np.array([[0, 11], [0, 12], [0, 13], [2, 11]]),      # 0 and 2 left only, 11 .. 13 right only
        "negative": np.array([[-1, 0], [-23, 5], [5, -2]]),
        "random": rng.integers(0, N, (57, 2)),
        "all_nodes": np.stack([np.arange(N), np.arange(N)[::-1]], axis=1),
    }


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edge_batch_is_the_restated_relabelling(name):
    e = edge_cases()[name]
    b = LK.EdgeBatch(torch.from_numpy(e), N)
    n_id, local = LR.relabel(e, N)
    wrapped = np.where(e < 0, e + N, e)
    assert b.n_id.dtype == b.local.dtype == b.edges.dtype == torch.int64
    assert np.array_equal(b.n_id.numpy(), n_id) and np.array_equal(b.local.numpy(), local)
    assert np.array_equal(b.edges.numpy(), wrapped) and tuple(b.local.shape) == (e.shape[0], 2)
    # torch's own unique, and the round trip through n_id
    assert torch.equal(b.n_id, torch.unique(torch.from_numpy(wrapped).reshape(-1)))
    assert torch.equal(b.n_id[b.local], b.edges)
    inc_ptr, inc_slot = LR.incidence(local, n_id.size)
    assert b._inc is None, "the incidence is built on first use"
    assert np.array_equal(b.inc_ptr.numpy(), inc_ptr) and np.array_equal(b.inc_slot.numpy(), inc_slot)
    assert b.incidence() is b.incidence(), "and kept"
    assert b.num_edges == e.shape[0] and b.num_nodes == n_id.size


def test_edge_batch_takes_lists_and_int32():
    want = LR.relabel([[1, 2], [2, 5]], N)
    for q in ([[1, 2], [2, 5]], torch.tensor([[1, 2], [2, 5]], dtype=torch.int32), np.array([[1, 2], [2, 5]])):
        b = LK.EdgeBatch(q, N)
        assert np.array_equal(b.n_id.numpy(), want[0]) and np.array_equal(b.local.numpy(), want[1])
    assert LK.EdgeBatch([], N).num_edges == 0 and LK.EdgeBatch([], N).num_nodes == 0


@pytest.mark.parametrize("q, exc", [
    (torch.tensor([[0, N]]), IndexError),
    (torch.tensor([[-N - 1, 0]]), IndexError),
    (torch.tensor([[0.0, 1.0]]), TypeError),
    (torch.tensor([[True, False]]), TypeError),
    (torch.tensor([0, 1, 2]), ValueError),
    (torch.zeros((2, 3), dtype=torch.int64), ValueError),
    (torch.zeros((2, 2, 2), dtype=torch.int64), ValueError),
])
def test_edge_batch_errors_come_before_any_work(q, exc, monkeypatch):
    def no_work(*a, **k):
        raise AssertionError("work before the check")
    monkeypatch.setattr(torch, "zeros", no_work)      # the mark over n is the first thing built
    with pytest.raises(exc):
        LK.EdgeBatch(q, N)


# ---- pair_linear on the CPU -------------------------------------------------------------------------
def composition(z, q, W, b):
    return nn.functional.linear(torch.cat((z[q[:, 0]], z[q[:, 1]]), dim=-1), W, b)


@pytest.mark.parametrize("h, C", [(1, 1), (5, 3)])
@pytest.mark.parametrize("as_batch", (False, True))
def test_gradcheck_fp64(h, C, as_batch):
    g = torch.Generator().manual_seed(7)
    e = torch.from_numpy(edge_cases()["random"][:19])
    batch = LK.EdgeBatch(e, N)
    rows = batch.num_nodes if as_batch else N
    z = torch.randn(rows, h, dtype=torch.float64, generator=g, requires_grad=True)
    W = torch.randn(C, 2 * h, dtype=torch.float64, generator=g, requires_grad=True)
    b = torch.randn(C, dtype=torch.float64, generator=g, requires_grad=True)
    q = batch if as_batch else e
    assert torch.autograd.gradcheck(lambda z, W, b: LK.pair_linear(z, q, W, b), (z, W, b))
    assert torch.autograd.gradcheck(lambda z, W: LK.pair_linear(z, q, W), (z, W))
    ids = batch.local if as_batch else e
    assert torch.allclose(LK.pair_linear(z, q, W, b), composition(z, ids, W, b), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ("random", "self_pair", "repeated", "one_sided", "one", "empty"))
@pytest.mark.parametrize("h, C", [(1, 1), (5, 3), (64, 47)])
def test_cpu_fp32_within_the_derived_bounds(name, h, C):
    e = edge_cases()[name]
    E = e.shape[0]
    rng = np.random.default_rng(11)
    z, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((N, h), (C, 2 * h), (C,)))
    g = rng.standard_normal((E, C)).astype(np.float32)
    zt, Wt, bt = (torch.from_numpy(a).requires_grad_() for a in (z, W, b))
    out = LK.pair_linear(zt, torch.from_numpy(e), Wt, bt)
    assert tuple(out.shape) == (E, C) and out.dtype == torch.float32
    out.backward(torch.from_numpy(g))
    o64, T_out, dz, T_z, dW, T_W, db, T_b = LR.reference64(z, e, W, b, g)
    bz, bW, bb = LR.backward_bounds(T_z, T_W, T_b, LR.slot_counts(e, N), C, E)
    for what, got, want, bound in (("out", out, o64, LR.forward_bound(T_out, h)), ("dz", zt.grad, dz, bz),
                                   ("dW", Wt.grad, dW, bW), ("db", bt.grad, db, bb)):
        err = np.abs(got.detach().numpy().astype(np.float64) - want)
        assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    # a node without a slot has a gradient of exactly +0
    untouched = np.setdiff1d(np.arange(N), e.reshape(-1))
    assert not zt.grad.numpy()[untouched].any()


def test_cpu_segment_sum_is_the_chain_bit_for_bit():
    """index_add_ in slot order on the CPU is the restatement's sequential chain, specials included."""
    e = edge_cases()["random"]
    n_id, local = LR.relabel(e, N)
    inc_ptr, inc_slot = LR.incidence(local, n_id.size)
    g = np.random.default_rng(5).standard_normal((e.shape[0], 3)).astype(np.float32)
    g[0, 0], g[1, 1], g[2, 2], g[3, 0], g[4, 1] = np.nan, np.inf, -np.inf, -0.0, 1e-41
    S = LK.pair_segment_sum(torch.from_numpy(g), torch.from_numpy(inc_ptr), torch.from_numpy(inc_slot))
    assert LR.same_bits(S.numpy(), LR.segment_sum(g, inc_ptr, inc_slot, n_id.size))
    P = np.random.default_rng(6).standard_normal((n_id.size, 6)).astype(np.float32)
    b = np.float32([0.5, -0.0, 3.0])
    out = LK.pair_gather_add(torch.from_numpy(P), torch.from_numpy(local), torch.from_numpy(b))
    assert LR.same_bits(out.numpy(), LR.gather_add(P, local, b))


def test_pair_linear_argument_errors():
    z, W = torch.zeros(4, 3), torch.zeros(2, 6)
    q = torch.tensor([[0, 1]])
    with pytest.raises(ValueError):
        LK.pair_linear(z, q, torch.zeros(2, 5))
    with pytest.raises(ValueError):
        LK.pair_linear(z, q, W, torch.zeros(3))
    with pytest.raises(TypeError):
        LK.pair_linear(z, q, W.double())
    with pytest.raises(TypeError):
        LK.pair_linear(z.long(), q, W)
    with pytest.raises(ValueError):
        LK.pair_linear(z, LK.EdgeBatch(q, 4), W)          # z is not [U, h]
    with pytest.raises(IndexError):
        LK.pair_linear(z, torch.tensor([[0, 4]]), W)


# ---- the loader -------------------------------------------------------------------------------------
def test_loader_covers_every_edge_once_and_relabels_each_batch():
    e = edge_cases()["random"]
    E = e.shape[0]
    labels = torch.arange(E) * 10
    for shuffle in (False, True):
        ld = LK.EdgeBatchLoader(torch.from_numpy(e), labels, N, 16, shuffle=shuffle, generator=torch.Generator().manual_seed(1))
        assert len(ld) == 4
        seen = []
        for k, (batch, lab, idx) in enumerate(ld):
            assert idx.dtype == torch.int64 and idx.numel() == (16 if k < 3 else E - 48)
            n_id, local = LR.relabel(e[idx.numpy()], N)
            assert np.array_equal(batch.n_id.numpy(), n_id) and np.array_equal(batch.local.numpy(), local)
            assert torch.equal(lab, labels[idx])
            seen.append(idx)
        seen = torch.cat(seen)
        assert torch.equal(torch.sort(seen).values, torch.arange(E))
        if not shuffle:
            assert torch.equal(seen, torch.arange(E))


def test_loader_order_is_the_generators():
    e = torch.from_numpy(edge_cases()["random"])
    E = e.shape[0]
    labels = torch.zeros(E)

    def epochs(seed, k):
        ld = LK.EdgeBatchLoader(e, labels, N, 10, generator=torch.Generator().manual_seed(seed))
        return [torch.cat([idx for _, _, idx in ld]) for _ in range(k)]
    a, b = epochs(4, 2), epochs(4, 2)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "a seeded generator fixes the order"
    assert not torch.equal(a[0], a[1]), "drawn anew per epoch"
    gen = torch.Generator().manual_seed(4)
    assert torch.equal(a[0], torch.randperm(E, generator=gen)) and torch.equal(a[1], torch.randperm(E, generator=gen))
    with pytest.raises(ValueError):
        LK.EdgeBatchLoader(e, labels[:-1], N, 10)
    with pytest.raises(ValueError):
        LK.EdgeBatchLoader(e, labels, N, 0)
    with pytest.raises(IndexError):
        LK.EdgeBatchLoader(e + N, labels, N, 10)


# ---- edge_head --------------------------------------------------------------------------------------
def test_edge_head_falls_back_under_training_dropout(monkeypatch):
    torch.manual_seed(2)
    lin = nn.Linear(10, 3)
    f = torch.randn(N, 5)
    q = torch.from_numpy(edge_cases()["random"])
    calls = []
    real = LK.pair_linear
    monkeypatch.setattr(LK, "pair_linear", lambda *a, **k: calls.append(1) or real(*a, **k))
    drop = nn.Dropout(0.5)

    # training, p > 0: the reference's composition with the same mask
    torch.manual_seed(9)
    got = LK.edge_head(lin, f, q, drop)
    torch.manual_seed(9)
    want = lin(drop(torch.cat((f[q[:, 0]], f[q[:, 1]]), dim=-1)))
    assert not calls and torch.equal(got, want)
    batch = LK.EdgeBatch(q, N)
    torch.manual_seed(9)
    assert torch.equal(LK.edge_head(lin, f[batch.n_id], batch, drop), want) and not calls

    # eval, p = 0 and no dropout at all: the fused head, within rounding of the composition
    plain = lin(torch.cat((f[q[:, 0]], f[q[:, 1]]), dim=-1))
    for d in (drop.eval(), nn.Dropout(0.0), None):
        n_calls = len(calls)
        out = LK.edge_head(lin, f, q, d)
        assert len(calls) == n_calls + 1
        assert torch.allclose(out, plain, rtol=1e-5, atol=1e-5)


def test_graph_convolution2_has_the_switch_off_by_default():
    from srgnn.graph_conv import GraphConvolution2
    assert GraphConvolution2(4, 8, 3).fused_edge_head is False


# ---- the C-ABI --------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_check_their_arguments():
    import ctypes
    import os
    from srgnn import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srgnn_hip.h")).read()
    for name in ("srg_pair_gather_add_f32", "srg_pair_segment_sum_f32"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(const float\* " % name, header)
    L = _lib.lib()
    assert L.srg_pair_gather_add_f32.argtypes[6] is ctypes.c_int32 and len(L.srg_pair_gather_add_f32.argtypes) == 10
    assert L.srg_pair_segment_sum_f32.argtypes[6] is ctypes.c_int32 and len(L.srg_pair_segment_sum_f32.argtypes) == 10
    E, some = _lib.SRG_ERR_INVALID, ctypes.c_void_p(16)

    def gather(P=some, ldp=6, U=4, q=some, b=None, n=2, C=3, out=some, ldo=3):
        return L.srg_pair_gather_add_f32(P, ldp, U, q, b, n, C, out, ldo, None)

    def segsum(g=some, ldg=3, n=2, ptr=some, slot=some, U=4, C=3, S=some, lds=6):
        return L.srg_pair_segment_sum_f32(g, ldg, n, ptr, slot, U, C, S, lds, None)

    # every rejection comes before a launch: the pointers above are not memory
    assert gather(n=-1) == E and "out of range" in _lib.last_error()
    assert gather(U=-1) == E and gather(n=2 ** 31) == E and gather(C=-1) == E
    assert gather(ldp=5) == E and "ldp" in _lib.last_error()
    assert gather(ldo=2) == E and gather(q=None) == E and gather(out=None) == E and gather(P=None) == E
    assert "null P" in _lib.last_error()
    assert segsum(n=-1) == E and segsum(U=2 ** 31) == E and segsum(C=-1) == E
    assert segsum(ldg=2) == E and segsum(lds=5) == E and "lds" in _lib.last_error()
    assert segsum(ptr=None) == E and segsum(S=None) == E and segsum(g=None) == E and segsum(slot=None) == E
    for ok in (gather(n=0), gather(C=0, ldp=0, ldo=0), gather(n=0, q=None, out=None), segsum(U=0), segsum(C=0, ldg=0, lds=0)):
        assert ok == _lib.SRG_OK                                        # launches nothing
    assert L.srg_last_error_code() == _lib.SRG_OK
