"""srgnn.sage on the device.  sage_mean, forward and backward, equals the CPU oracle's hop followed by an fp32
division bit for bit (a square operator with unsorted rows, duplicates and empty rows, a rectangular sampled block,
a symmetric operator whose transpose is itself, and rows=).  SAGEConv and the two-layer SAGE, on a NeighborBatch
and on the full graph, lie within the first-order bound of tests/sage_ref.py of the same layers
in fp64 over dense mean matrices, and equal bit for bit the same layers on operators built from the restatement's
blocks; GraphConvolution2 and GAT train on a NeighborBatch's block as on the restatement's."""
import functools

import numpy as np
import pytest
import torch

import neighbor_ref as NR
import sage_ref as SR

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(x):
    return x.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def features(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x[::7, ::3] = np.float32(-0.0)
    return x


@functools.lru_cache(maxsize=None)
def operators():
    """name -> (ptr, idx, n_cols): the 400-node test operator of the sampler (unsorted, duplicates, empty rows, a row
    of 5,000), a sampled block of it (rectangular), and the R-MAT operator's structure (symmetric, sorted)."""
    ip, ix, v = NR.graph()
    S = NR.node_sets(ip)["shuffled37"]
    ptr, cols, _, n_id, _ = NR.block(ip, ix, v, NR.N, S, 10, 21)
    n, _, r_ip, r_ix, _ = rmat()
    return {"square": (ip, ix, NR.N), "block": (ptr, cols, n_id.size), "symmetric": (r_ip, r_ix, n)}


@functools.lru_cache(maxsize=None)
def rmat():
    from srgnn import synth
    from srgnn.csr import DeviceCSR
    from srgnn.normalize import sym_norm_binary
    n = 2000
    u, v = synth.rmat_undirected_t(n, 9000, seed=synth.RMAT_SEED, device=dev())
    ip, ix = synth.symmetric_csr_t(n, u, v)
    ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
    A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev())
    return n, A, ip.cpu().numpy(), ix.cpu().numpy(), vals.cpu().numpy()


def mean_op(ptr, idx, n_cols):
    from srgnn.csr import DeviceCSR
    from srgnn.sage import mean_operator
    vals = np.full(idx.size, 3.5, dtype=np.float32)                 # ignored: the mean's values are 1.0
    return mean_operator(DeviceCSR.from_tensors(ptr, idx, vals, n_cols=n_cols, device=dev()))


@pytest.mark.parametrize("d", (1, 24, 130))
@pytest.mark.parametrize("name", ("square", "block", "symmetric"))
def test_sage_mean_is_the_oracles_hop_and_one_division(name, d):
    from srgnn.sage import sage_mean
    ptr, idx, n_cols = operators()[name]
    n_rows = ptr.size - 1
    op = mean_op(ptr, idx, n_cols)
    assert op.transpose_kind == ("same" if name == "symmetric" else "sorted")
    assert (np.diff(ptr) == 0).any() or name == "symmetric"
    assert np.array_equal(host(op.cnt), np.maximum(np.diff(ptr), 1).astype(np.float32)) and op.A.indices.data_ptr() != 0
    x = features(n_cols, d, 1)
    G = features(n_rows, d, 2)
    xd = t(x).requires_grad_(True)
    y = sage_mean(op, xd)
    y.backward(t(G))
    want = SR.mean_forward(ptr, idx, x)
    assert np.array_equal(bits(host(y)), bits(want)), "forward"
    empty = np.flatnonzero(np.diff(ptr) == 0)
    assert (bits(host(y))[empty] == 0).all()                        # an empty row is +0
    assert np.array_equal(bits(host(xd.grad)), bits(SR.mean_backward(ptr, idx, n_cols, G))), "backward"
    if name == "block":
        return
    # rows=: the same bits for a batch of rows, the gradient that of the batch's rows alone
    rows = np.random.default_rng(4).permutation(n_rows)[:(37 * n_rows) // 100]
    Gb = features(rows.size, d, 3)
    xd = t(x).requires_grad_(True)
    yb = sage_mean(op, xd, rows=t(rows))
    yb.backward(t(Gb))
    assert np.array_equal(bits(host(yb)), bits(want[rows])) and np.array_equal(bits(host(yb)), bits(SR.mean_forward(ptr, idx, x, rows)))
    assert np.array_equal(bits(host(xd.grad)), bits(SR.mean_backward(ptr, idx, n_cols, Gb, rows))), "backward, rows"


def test_sage_mean_checks_its_arguments():
    from srgnn.graph_conv import GraphConvOperator
    from srgnn.sage import sage_mean
    ptr, idx, n_cols = operators()["block"]
    op = mean_op(ptr, idx, n_cols)
    x = torch.zeros((n_cols, 4), device=dev())
    with pytest.raises(ValueError, match="square"):
        sage_mean(op, x, rows=[0, 1])
    with pytest.raises(ValueError, match="x_src must be"):
        sage_mean(op, x[:-1])
    with pytest.raises(TypeError, match="fp32"):
        sage_mean(op, x.double())
    with pytest.raises(TypeError, match="mean_operator"):
        sage_mean(GraphConvOperator(op.A), x)
    sq = mean_op(*operators()["square"])
    with pytest.raises(ValueError, match="repeats"):
        sage_mean(sq, torch.zeros((NR.N, 4), device=dev()), rows=[3, 3])
    with pytest.raises(IndexError):
        sage_mean(sq, torch.zeros((NR.N, 4), device=dev()), rows=[NR.N])


# ---- the layers against fp64 over dense mean matrices -----------------------------------------------
def params_of(module):
    return {k: host(p).astype(np.float64) for k, p in module.named_parameters()}


def cotangent(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def train(module, forward, cot):
    module.zero_grad(set_to_none=True)
    out = forward()
    (out * t(cot)).sum().backward()
    res = {"out": host(out)}
    res.update({k: host(p.grad) for k, p in module.named_parameters()})
    return res


def check_within(got, want, what):
    assert sorted(got) == sorted(want), what
    worst = {}
    for k in want:
        assert np.isfinite(got[k]).all() and got[k].shape == want[k].val.shape, (what, k)
        worst[k] = SR.worst_ratio(got[k], want[k])
        print(f"{what} {k}: {worst[k]:.4f} of the bound")
    assert all(r <= 1.0 for r in worst.values()), (what, worst)
    assert np.abs(got["out"]).sum() > 0 and all(np.abs(got[k]).sum() > 0 for k in want)


@functools.lru_cache(maxsize=None)
def batch():
    """One NeighborBatch of 50 seeds with sizes [10, 5] over the R-MAT operator, the restatement's blocks of the same
    seeds, and the features."""
    from srgnn import neighbor as NB
    n, A, ip, ix, vals = rmat()
    idx = torch.from_numpy(np.random.default_rng(3).permutation(n)[:50])
    loader = NB.NeighborLoader(A, idx, [10, 5], 50, shuffle=False, seed=99)
    (b,) = list(loader)
    w_n_id, w_blocks = NR.loader_batch(ip, ix, vals, n, idx.numpy(), [10, 5], 99, 0, 0)
    assert np.array_equal(host(b.n_id), w_n_id)
    return b, w_blocks, features(n, 24, 6)


@pytest.mark.parametrize("where", ("block", "full", "full_rows"))
def test_sage_conv_within_the_bound_of_fp64(where):
    from srgnn.sage import SAGEConv
    from srgnn.spmm import gather_rows
    b, w_blocks, X = batch()
    n, A, ip, ix, vals = rmat()
    torch.manual_seed(7)
    conv = SAGEConv(24, 9).to(dev())
    assert [k for k, _ in conv.named_parameters()] == ["lin_l.weight", "lin_l.bias", "lin_r.weight"]
    assert conv.lin_l.weight.shape == (9, 24) and conv.lin_r.bias is None
    if where == "block":
        ptr, cols, _, n_id, _ = w_blocks[0]
        x = X[n_id]
        xd = gather_rows(t(X), b.n_id)
        assert np.array_equal(bits(host(xd)), bits(x))
        op = b.blocks[0].mean_operator()
        M, lens, lens_t = SR.dense_mean(ptr, cols, n_id.size)
        cot = cotangent((ptr.size - 1, 9), 8)
        got = train(conv, lambda: conv((xd, xd[:op.A.n_rows]), op), cot)
        again = train(conv, lambda: conv(xd, op), cot)               # x alone: the targets are the first rows
        assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in got)
        want = SR.one_layer(params_of(conv), M, lens, lens_t, x, cot)
    else:
        op = mean_op(ip, ix, n)
        M, lens, lens_t = SR.dense_mean(ip, ix, n)
        rows = np.random.default_rng(5).permutation(n)[:300] if where == "full_rows" else None
        cot = cotangent((n if rows is None else rows.size, 9), 8)
        got = train(conv, lambda: conv(t(X), op, None if rows is None else t(rows)), cot)
        full_cot = cot
        if rows is not None:                                        # the same loss over all rows: zero outside the batch
            full_cot = np.zeros((n, 9), dtype=np.float32)
            full_cot[rows] = cot
        want = SR.one_layer(params_of(conv), M, lens, lens_t, X, full_cot)
        if rows is not None:
            want["out"] = want["out"][rows]
    check_within(got, want, f"sage conv, {where}")


@pytest.mark.parametrize("where", ("batch", "full", "full_rows"))
def test_two_layer_sage_within_the_bound_of_fp64(where):
    from srgnn.sage import SAGE
    from srgnn.spmm import gather_rows
    b, w_blocks, X = batch()
    n, A, ip, ix, vals = rmat()
    torch.manual_seed(8)
    model = SAGE(24, 16, 5, 2, 0.0).to(dev())
    p = params_of(model)
    p1 = {k[len("convs.0."):]: v for k, v in p.items() if k.startswith("convs.0.")}
    p2 = {k[len("convs.1."):]: v for k, v in p.items() if k.startswith("convs.1.")}
    assert len(p) == 6 and len(p1) == 3 and len(p2) == 3
    if where == "batch":
        mats = [SR.dense_mean(blk[0], blk[1], blk[3].size) for blk in w_blocks]
        x = X[w_blocks[0][3]]
        xd = gather_rows(t(X), b.n_id)
        cot = cotangent((b.batch_size, 5), 9)
        got = train(model, lambda: model(xd, b.blocks), cot)
        assert got["out"].shape == (50, 5)
        want = SR.two_layer(p1, p2, mats, x, cot)
        # the same model on operators built from the restatement's blocks: the same chains, the same bits
        ops = [mean_op(blk[0], blk[1], blk[3].size) for blk in w_blocks]
        again = train(model, lambda: model(xd, ops), cot)
        for k in got:
            assert np.array_equal(bits(got[k]), bits(again[k])), k
    else:
        op = mean_op(ip, ix, n)
        mats = [SR.dense_mean(ip, ix, n)] * 2
        rows = np.random.default_rng(5).permutation(n)[:300] if where == "full_rows" else None
        cot = cotangent((n if rows is None else rows.size, 5), 9)
        got = train(model, lambda: model(t(X), op, None if rows is None else t(rows)), cot)
        full_cot = cot
        if rows is not None:
            full_cot = np.zeros((n, 5), dtype=np.float32)
            full_cot[rows] = cot
        want = SR.two_layer(p1, p2, mats, X, full_cot)
        if rows is not None:
            want["out"] = want["out"][rows]
    assert np.allclose(np.exp(got["out"].astype(np.float64)).sum(1), 1.0, atol=1e-5)      # log-probabilities
    check_within(got, want, f"two-layer sage, {where}")


def test_sage_runs_the_number_of_blocks_it_has_layers_for():
    from srgnn.sage import SAGE
    b, _, X = batch()
    model = SAGE(24, 16, 5, 3, 0.5).to(dev())
    with pytest.raises(ValueError, match="blocks"):
        model(t(X)[b.n_id], b.blocks)
    with pytest.raises(ValueError, match="rows"):
        SAGE(24, 16, 5, 2, 0.5).to(dev())(t(X)[b.n_id], b.blocks, rows=[0])
    with pytest.raises(ValueError, match="num_layers"):
        SAGE(24, 16, 5, 1, 0.5)


# ---- GCN and GAT on a NeighborBatch -----------------------------------------------------------------
def _train_step(model, forward, params):
    model.zero_grad(set_to_none=True)
    out = forward()
    G = torch.linspace(-1.0, 1.0, out.numel(), device=out.device).reshape(out.shape)
    (out * G).sum().backward()
    return [host(out)] + [host(p.grad) for p in params(model)]


def restated_square(blk):
    """The restatement's block as a square DeviceCSR over its sources: the rows past the targets are empty."""
    from srgnn.csr import DeviceCSR
    ptr, cols, val, n_id, _ = blk
    S = n_id.size
    ip = np.concatenate([ptr, np.full(S - (ptr.size - 1), ptr[-1], dtype=np.int64)])
    return DeviceCSR.from_tensors(ip, cols, val, n_cols=S, device=dev())


def test_graph_convolution_trains_on_a_neighbor_batch_as_on_the_restatements_block():
    from srgnn.graph_conv import GraphConvolution2, GraphConvOperator
    b, w_blocks, X = batch()
    blk = b.blocks[-1]
    xb = t(X)[blk.n_id].contiguous()
    torch.manual_seed(3)
    model = GraphConvolution2(24, 16, 5, dropout=0.0).to(dev())
    used = lambda m: [p for k, p in m.named_parameters() if k.split(".")[0] in ("fc1_node_edge", "fc2_node")]   # noqa: E731
    got_op, want_op = blk.graph_conv_operator(), GraphConvOperator.from_device_csr(restated_square(w_blocks[-1]))
    assert got_op.shape == want_op.shape == (blk.n_id.numel(), blk.n_id.numel()) and got_op.transpose_kind == want_op.transpose_kind
    res = []
    for op in (got_op, want_op):
        model.adj = op
        res.append(_train_step(model, lambda: model(xb, range(blk.n_dst)), used))
    assert len(res[0]) == 5 and res[0][0].shape == (50, 5) and np.abs(res[0][1]).sum() > 0
    for g, w in zip(*res):
        assert np.array_equal(bits(g), bits(w))


def test_gat_trains_on_a_neighbor_batch_as_on_the_restatements_block():
    from srgnn.gat import GAT, GATGraph
    b, w_blocks, X = batch()
    blk = b.blocks[-1]
    xb = t(X)[blk.n_id].contiguous()
    torch.manual_seed(4)
    model = GAT(24, 8, 5, 2, 0.0, 2).to(dev())
    got_g, want_g = blk.gat_graph(), GATGraph.from_device_csr(restated_square(w_blocks[-1]))
    for k in ("indptr", "indices", "indptr_t", "indices_t", "perm"):
        assert torch.equal(getattr(got_g, k), getattr(want_g, k)), k
    res = [_train_step(model, lambda: model(xb, g, range(blk.n_dst)), lambda m: list(m.parameters())) for g in (got_g, want_g)]
    assert res[0][0].shape == (50, 5) and np.abs(res[0][1]).sum() > 0
    for g, w in zip(*res):
        assert np.array_equal(bits(g), bits(w))
