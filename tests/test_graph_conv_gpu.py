"""srgnn.graph_conv on the GPU: the full products bit for bit the oracle's chains (and within the derived
bound of the reference's own torch.mm, tests/golden/graph_conv.npz), the row-restricted product and its
adjoint bit for bit the host restatement (tests/graph_conv_ref.py), and the reference's two-layer
convolution, restated here, running on a GraphConvOperator against GraphConvolution2."""
import numpy as np
import pytest
import torch
from torch import nn

import graph_conv_ref as R
from oracle import oracle as O
from srgnn import _lib
from srgnn import graph_conv as GC
from srgnn.csr import DeviceCSR

pytestmark = pytest.mark.gpu

OPS = R.CASES + ("star",)
D_SWEEP = (1, 7, 47, 64, 65, 130)
_ops = {}


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32)


def arrays(name):
    return R.star_graph() if name == "star" else R.case(name)


def operator(name):
    """(GraphConvOperator, host CSR, host transpose), built once per operator."""
    if name not in _ops:
        ip, ix, v = arrays(name)
        n = ip.size - 1
        if name == "star":
            op = GC.GraphConvOperator.from_device_csr(DeviceCSR.from_tensors(ip, ix, v, n_cols=n, device=dev()))
        else:                      # the reference's tensor layout: sparse COO, here in the fixture's order
            rows = torch.from_numpy(R.entry_rows(ip))
            coo = torch.sparse_coo_tensor(torch.stack([rows, torch.from_numpy(ix.astype(np.int64))]),
                                          torch.from_numpy(v), (n, n))
            op = GC.GraphConvOperator.from_torch_sparse(coo, device=dev())
        _ops[name] = (op, (ip, ix, v), R.transpose_stable(ip, ix, v, n))
    return _ops[name]


def batch(name, n, B, seed):
    """B shuffled unique ids; on the star graph the star row and an isolated node lead when they fit."""
    rows = np.random.default_rng(seed).permutation(n)[:B].astype(np.int64)
    if name == "star" and B >= 2:
        rest = rows[~np.isin(rows, (7, 3))]
        rows = np.r_[7, 3, rest][:B].astype(np.int64)
    return rows


def panel(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


# ---- full product -----------------------------------------------------------------------------------
def test_transpose_kinds():
    for name in R.CASES:
        op = operator(name)[0]
        assert op.transpose_kind == R.KINDS[name]
    same, mirrored, sorted_ = (operator(nm)[0] for nm in R.CASES)
    assert same.At is same.A
    assert mirrored.At is not mirrored.A and mirrored.At.indices.data_ptr() == mirrored.A.indices.data_ptr() \
        and mirrored.At.indptr.data_ptr() == mirrored.A.indptr.data_ptr() \
        and mirrored.At.values.data_ptr() != mirrored.A.values.data_ptr()
    assert sorted_.At.indices.data_ptr() != sorted_.A.indices.data_ptr()
    assert operator("star")[0].transpose_kind == "mirrored"
    for name in OPS:               # whatever the kind, At is the stable sort by column
        op, _, (tp, tx, tv) = operator(name)
        assert np.array_equal(op.At.indptr.cpu().numpy(), tp) and np.array_equal(op.At.indices.cpu().numpy(), tx)
        assert np.array_equal(bits(op.At.values), bits(tv))


def test_from_scipy_builds_the_same_operator():
    import scipy.sparse as sp
    for name in R.CASES:
        op, (ip, ix, v), _ = operator(name)
        n = ip.size - 1
        other = GC.GraphConvOperator.from_scipy(sp.csr_matrix((v, ix, ip), shape=(n, n)), device=dev())
        assert other.transpose_kind == op.transpose_kind
        assert np.array_equal(bits(other.A.values), bits(op.A.values))
        assert np.array_equal(bits(other.At.values), bits(op.At.values))
        assert np.array_equal(other.A.indices.cpu().numpy(), ix)


@pytest.mark.parametrize("name", OPS)
@pytest.mark.parametrize("d", (7, 47, 130))
def test_full_product_and_gradient_are_the_oracle_chains(name, d):
    op, (ip, ix, v), (tp, tx, tv) = operator(name)
    n = ip.size - 1
    Z, G = (R.panels(d) if name != "star" and d in R.WIDTHS else (panel(n, d, 1), panel(n, d, 2)))
    z = t(Z).requires_grad_(True)
    y = GC.graph_conv(op, z)
    y.backward(t(G))
    assert np.array_equal(bits(y), bits(O.spmm(ip, ix, v, Z)))
    assert np.array_equal(bits(z.grad), bits(O.spmm(tp, tx, tv, G)))


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("d", R.WIDTHS)
def test_full_product_within_the_bound_of_the_reference(name, d):
    """Against torch.mm on the reference's sparse tensor and its autograd: 2 gamma_len sum |v||z|."""
    g = R.golden()
    op, (ip, ix, v), (tp, tx, tv) = operator(name)
    Z, G = R.panels(d)
    z = t(Z).requires_grad_(True)
    y = torch.mm(op, z)
    (y * t(G)).sum().backward()
    err = np.abs(y.detach().cpu().numpy().astype(np.float64) - g[f"{name}__Y{d}"].astype(np.float64))
    assert (err <= R.chain_bound(ip, ix, v, Z)).all()
    err = np.abs(z.grad.cpu().numpy().astype(np.float64) - g[f"{name}__dZ{d}"].astype(np.float64))
    assert (err <= R.chain_bound(tp, tx, tv, G)).all()


def test_protocol():
    op = operator("gc_sym05")[0]
    n = op.shape[0]
    x = t(panel(n, 7, 3))
    want = bits(GC.graph_conv(op, x))
    assert np.array_equal(bits(torch.mm(op, x)), want)
    assert np.array_equal(bits(torch.sparse.mm(op, x)), want)
    assert np.array_equal(bits(op @ x), want)
    assert op.to(dev()) is op and op.to("cuda") is op and op.device == dev() and tuple(op.shape) == (n, n)
    with pytest.raises(RuntimeError):
        op.to("cpu")
    assert (op != None) is True        # noqa: E711  the reference's own test of `adj`
    with pytest.raises(TypeError):
        torch.add(op, x)
    a, b = op.prepare(7, 2)
    assert a >= 1 and b >= 1
    host = GC.graph_conv(op, x.cpu())
    assert host.device.type == "cpu" and np.array_equal(bits(host), want)


# ---- row product ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPS)
@pytest.mark.parametrize("d", D_SWEEP)
def test_rows_product_and_adjoint_are_the_restatement(name, d):
    op, (ip, ix, v), (tp, tx, tv) = operator(name)
    n = ip.size - 1
    X = panel(n, d, 10 + d)
    Xd = t(X)
    for B in (0, 1, 63, 64, 65, n):
        rows = batch(name, n, B, 7 * B + d)
        G = panel(B, d, B + 1)
        x = Xd.clone().requires_grad_(True)
        y = GC.graph_conv(op, x, rows)
        assert tuple(y.shape) == (B, d)
        assert np.array_equal(bits(y), bits(R.rows_forward_ref(ip, ix, v, rows, X)))
        y.backward(t(G))
        pos = R.pos_of(rows, n)
        want = R.rows_adjoint_ref(tp, tx, tv, pos, G)
        assert np.array_equal(bits(x.grad), bits(want))
        # the full path on G scattered into n rows of +0: the same bits on a finite operator
        scattered = torch.zeros((n, d), device=dev())
        scattered[t(rows)] = t(G)
        assert np.array_equal(bits(GC._hop(op.At, scattered)), bits(want))
        if B == 0:
            assert not bits(x.grad).any()                    # +0: the sign bit too


@pytest.mark.parametrize("name", ("gc_sym03", "star"))
def test_strided_views_take_the_4_byte_path(name):
    """d = 64 contiguous may take 16-byte loads; the same columns as a window of a 67-wide panel cannot.
    Both give the restatement's bits."""
    op, (ip, ix, v), (tp, tx, tv) = operator(name)
    n = ip.size - 1
    d = 64
    rows = batch(name, n, 65, 2)
    X, G = panel(n, d, 4), panel(rows.size, d, 5)
    wide_x = torch.zeros((n, 67), device=dev())
    wide_x[:, 1:65] = t(X)
    wide_g = torch.zeros((rows.size, 67), device=dev())
    wide_g[:, 2:66] = t(G)
    want_y = R.rows_forward_ref(ip, ix, v, rows, X)
    want_dx = R.rows_adjoint_ref(tp, tx, tv, R.pos_of(rows, n), G)
    pos = t(R.pos_of(rows, n))
    for xv, gv in ((t(X), t(G)), (wide_x[:, 1:65], wide_g[:, 2:66])):
        assert np.array_equal(bits(GC.rows_product(op.A, xv, t(rows))), bits(want_y))
        assert np.array_equal(bits(GC.rows_adjoint(op.At, pos, gv)), bits(want_dx))
    out = torch.full((n, 67), 9.0, device=dev())
    GC.rows_adjoint(op.At, pos, wide_g[:, 2:66], out=out[:, 3:67])
    assert np.array_equal(bits(out[:, 3:67]), bits(want_dx)) and bool((out[:, :3] == 9.0).all())


def test_two_16_byte_tiles():
    """d = 260: two 256-column tiles of the 16-byte path (the sweep's widths stay within one)."""
    op, (ip, ix, v), (tp, tx, tv) = operator("star")
    n = ip.size - 1
    rows = batch("star", n, 65, 30)
    X, G = panel(n, 260, 31), panel(65, 260, 32)
    assert np.array_equal(bits(GC.rows_product(op.A, t(X), t(rows))), bits(R.rows_forward_ref(ip, ix, v, rows, X)))
    pos = R.pos_of(rows, n)
    assert np.array_equal(bits(GC.rows_adjoint(op.At, t(pos), t(G))), bits(R.rows_adjoint_ref(tp, tx, tv, pos, G)))


def test_out_of_range_ids():
    """Straight to the C entry, -1 and n give rows of +0; the wrapper raises IndexError for them."""
    op, (ip, ix, v), _ = operator("gc_dir05")
    n = ip.size - 1
    X = panel(n, 47, 6)
    rows = np.array([5, -1, n, 0], dtype=np.int64)
    y = torch.full((4, 47), 3.0, device=dev())
    GC.rows_product(op.A, t(X), t(rows), out=y)
    assert np.array_equal(bits(y), bits(R.rows_forward_ref(ip, ix, v, rows, X)))
    assert not bits(y[1:3]).any()
    for bad in ([n], [-n - 1], torch.tensor([0, n], device=dev())):
        with pytest.raises(IndexError):
            GC.graph_conv(op, t(X), bad)
    # negative ids wrap; a range and a host list are taken as they are
    want = bits(R.rows_forward_ref(ip, ix, v, np.array([n - 1, 0, n - 2]), X))
    assert np.array_equal(bits(GC.graph_conv(op, t(X), [-1, 0, -2])), want)
    want = bits(R.rows_forward_ref(ip, ix, v, np.arange(3, 40), X))
    assert np.array_equal(bits(GC.graph_conv(op, t(X), range(3, 40))), want)


def test_non_finite_values_outside_the_batch_stay_outside():
    """NaN and Inf in X rows that no batch row reads do not reach Y; an Inf operator value in an entry whose
    column is outside the batch does not reach dX (skipped, not multiplied by zero)."""
    op, (ip, ix, v), (tp, tx, tv) = operator("star")
    n = ip.size - 1
    rows = batch("star", n, 64, 11)
    touched = np.zeros(n, bool)
    for r in rows:
        touched[ix[ip[r]:ip[r + 1]]] = True
    free = np.flatnonzero(~touched)
    assert free.size >= 2
    X = panel(n, 7, 12)
    clean = R.rows_forward_ref(ip, ix, v, rows, X)
    X[free[0]], X[free[1]] = np.nan, np.inf
    y = GC.graph_conv(op, t(X), rows)
    assert np.array_equal(bits(y), bits(clean)) and np.isfinite(clean).all()

    pos = R.pos_of(rows, n)
    outside = np.flatnonzero(pos[tx] < 0)
    tv_inf = tv.copy()
    tv_inf[outside[::7]] = np.inf
    At = DeviceCSR.from_tensors(tp, tx, tv_inf, n_cols=n, device=dev())
    G = panel(rows.size, 7, 13)
    dx = GC.rows_adjoint(At, t(pos), t(G))
    want = R.rows_adjoint_ref(tp, tx, tv, pos, G)
    assert np.array_equal(bits(dx), bits(want)) and np.isfinite(want).all()


def test_run_to_run_identical():
    op, (ip, ix, v), _ = operator("star")
    n = ip.size - 1
    rows = t(batch("star", n, 200, 14))
    X, G = t(panel(n, 47, 15)), t(panel(200, 47, 16))
    pos = t(R.pos_of(rows.cpu().numpy(), n))
    y0, d0 = bits(GC.rows_product(op.A, X, rows)), bits(GC.rows_adjoint(op.At, pos, G))
    for _ in range(3):
        assert np.array_equal(bits(GC.rows_product(op.A, X, rows)), y0)
        assert np.array_equal(bits(GC.rows_adjoint(op.At, pos, G)), d0)


@pytest.mark.parametrize("name", ("gc_sym03", "gc_dir05"))
def test_duplicate_rows_match_torch_indexing(name):
    """rows with repeats against torch's Y_full[rows]: the same bits forward, the bound backward."""
    op, (ip, ix, v), (tp, tx, tv) = operator(name)
    n = ip.size - 1
    d = 47
    rows = np.r_[batch(name, n, 40, 17), [5, 5, 9], batch(name, n, 40, 17)[:3]].astype(np.int64)
    X, G = panel(n, d, 18), panel(rows.size, d, 19)
    x = t(X).requires_grad_(True)
    y = GC.graph_conv(op, x, rows)
    y.backward(t(G))
    x2 = t(X).requires_grad_(True)
    y2 = GC.graph_conv(op, x2)[t(rows)]              # torch's indexing of the full product
    y2.backward(t(G))
    assert np.array_equal(bits(y), bits(y2))
    assert np.array_equal(bits(y), bits(O.spmm(ip, ix, v, X)[rows]))
    # Both gradients are fp32 evaluations of sum_e v_e sum_{b: rows[b] = col_e} G[b]: the repeats' rows of G
    # are added first (at most m - 1 additions for an id that occurs m times), then the row's chain runs.
    # A term thus passes at most len + m - 1 roundings on either side: the same bound with that length and
    # with |G| summed over the repeats.
    absG = np.zeros((n, d))
    np.add.at(absG, rows, np.abs(G.astype(np.float64)))
    m = int(np.bincount(rows).max())
    err = np.abs(x.grad.cpu().numpy().astype(np.float64) - x2.grad.cpu().numpy().astype(np.float64))
    assert (err <= R.chain_bound(tp, tx, tv, absG, extra=m - 1)).all()


# ---- the reference's layer, restated ----------------------------------------------------------------
class ReferenceLayer(nn.Module):
    """Layer2GraphConvolution's node head restated (SSRG/models/base_scalable/simple_models.py:214-240):
    fc -> torch.mm(adj, .) -> relu -> dropout -> fc -> torch.mm(adj, .); the caller indexes [idx]."""

    def __init__(self, feat_dim, hidden_dim, output_dim, dropout):
        super().__init__()
        self.adj = None
        self.query_edges = None
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(dropout)
        self.fc1_node_edge = nn.Linear(feat_dim, hidden_dim)
        self.fc2_node = nn.Linear(hidden_dim, output_dim)
        self.fc2_edge = nn.Linear(hidden_dim, hidden_dim)
        self.linear = nn.Linear(2 * hidden_dim, output_dim)

    def forward(self, feature):
        x = self.fc1_node_edge(feature)
        x = torch.mm(self.adj, x)
        x = self.dropout(self.relu(x))
        if self.query_edges == None:      # noqa: E711  as the reference writes it
            return torch.mm(self.adj, self.fc2_node(x))
        x = torch.mm(self.adj, self.fc2_edge(x))
        return self.linear(torch.cat((x[self.query_edges[:, 0]], x[self.query_edges[:, 1]]), dim=-1))


@pytest.mark.parametrize("name", R.CASES)
def test_reference_layer_runs_on_the_operator_and_equals_graphconvolution2(name):
    op, (ip, ix, v), _ = operator(name)
    n = ip.size - 1
    feat, hidden, classes = 19, 32, 7
    torch.manual_seed(5)
    ref = ReferenceLayer(feat, hidden, classes, 0.0).to(dev())
    ours = GC.GraphConvolution2(feat, hidden, classes, dropout=0.0).to(dev())
    ours.load_state_dict(ref.state_dict())          # the names interchange
    ref.adj = op.to(dev())
    ours.adj = op
    x = t(panel(n, feat, 21))
    idx = t(batch(name, n, 70, 22))
    labels = torch.from_numpy(np.random.default_rng(23).integers(0, classes, 70)).to(dev())

    out_ref = ref(x)[idx]
    nn.functional.cross_entropy(out_ref, labels).backward()
    out = ours(x, rows=idx)
    nn.functional.cross_entropy(out, labels).backward()
    assert np.array_equal(bits(out), bits(out_ref))
    # sparse side bit for bit (rows adjoint == full adjoint of the scattered gradient), then the same GEMMs
    for (k, p), (_, q) in zip(ref.named_parameters(), ours.named_parameters()):
        if k.startswith(("fc1_node_edge", "fc2_node")):
            assert p.grad is not None and np.array_equal(bits(q.grad), bits(p.grad)), k
        else:
            assert p.grad is None and q.grad is None, k
    # all rows and the edge head: the reference's own branches
    assert np.array_equal(bits(ours(x)), bits(ref(x)))
    edges = t(np.random.default_rng(24).integers(0, n, (30, 2)))
    ref.query_edges = ours.query_edges = edges
    assert np.array_equal(bits(ours(x, rows=idx)), bits(ref(x)))
