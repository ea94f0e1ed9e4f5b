"""srgnn.link on the device: srg_pair_gather_add_f32 bit for bit torch's (P[q0, :C] + P[q1, C:]) + b
on the same P, srg_pair_segment_sum_f32 bit for bit the host restatement (tests/link_ref.py) with NaN, +-Inf, -0 and a
subnormal in g, the 16-byte path against the 4-byte path, ids and slots out of range, run-to-run identity, pair_linear
within the derived first-order bounds of the reference's formula in fp64, GraphConvolution2's fused edge head against
pair_linear on full rows (bit for bit) and against the unfused head (within the bounds), and the memory condition the
feature exists for.

Shapes: U = 9 nodes, E in {0, 1, 257}; at E = 257 node 0 holds about 200 slots (longer than any in-flight group of its
chain), node 8 a single one, with a self pair and duplicates; C on every edge of the lane layout (fewer lanes than a
wave, one wave, one over, more than two)."""
import functools

import numpy as np
import pytest
import torch

import link_ref as LR

pytestmark = pytest.mark.gpu

U = 9
ES = (0, 1, 257)
CS = (1, 3, 47, 64, 65, 130)
HS = (1, 5, 64)
SENT = np.float32(-7.5)
_worst = {}


def dev():
    return torch.device("cuda", 0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(x):
    return x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def pairs(E):
    """int64 [E, 2] of positions in [0, U): see the module docstring.  Computed once, never written to."""
    if E == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if E == 1:
        return np.array([[8, 0]], dtype=np.int64)
    rng = np.random.default_rng(41)
    flat = rng.integers(1, 8, 2 * E)
    flat[rng.permutation(2 * E)[:200]] = 0
    q = flat.reshape(E, 2).astype(np.int64)
    q[5] = (3, 3)                      # a self pair
    q[6] = q[7] = q[200] = (2, 4)      # duplicates
    q[8] = (4, 2)
    q[10] = (8, 1)                     # node 8's only slot
    return q


def test_the_fixture_holds_what_it_says():
    q = pairs(257)
    m = LR.slot_counts(q, U)
    assert m.sum() == 514 and 180 <= m[0] <= 200 and m[8] == 1 and (m > 0).all()
    assert (q[:, 0] == q[:, 1]).any() and q.min() == 0 and q.max() == 8


def odd_ld(w):
    """The smallest row stride > w that is no multiple of 4: such a view takes the 4-byte path."""
    return w + 1 if (w + 1) % 4 else w + 2


def window(rows, w, strided):
    """A sentinel-filled [rows, w] device panel: contiguous, or a column window of a wider one (row stride
    odd_ld(w)); returns (view, whole)."""
    whole = torch.full((max(rows, 1), odd_ld(w) if strided else w), float(SENT), dtype=torch.float32, device=dev())
    return whole[:rows, :w], whole


def untouched(whole, w):
    return bool((host(whole)[:, w:] == SENT).all())


def specials(g):
    """NaN, +Inf, -Inf, -0 and a subnormal in chosen cells of g [E, C] (E = 257: edges of the long node and the
    single-slot edge 10)."""
    E, C = g.shape
    if E == 0:
        return g
    cells = ((0, 0, np.nan), (3, 1, np.inf), (4, 2, -np.inf), (6, 3, -0.0), (10, 4, 1e-41), (10, 0, -0.0),
             (6, 5, np.inf), (7, 5, -np.inf))          # pairs 6 and 7 are both (2, 4): the two meet in one chain
    for e, c, v in cells:
        g[e % E, c % C] = v
    return g


# ---- the two entries against torch and the restatement ----------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_gather_add_is_torchs_association_bit_for_bit(C):
    from srgnn import link as LK
    rng = np.random.default_rng(100 + C)
    P_h = rng.standard_normal((U, 2 * C)).astype(np.float32)
    P_h[2, 0], P_h[4, C], P_h[3, C - 1], P_h[3, 2 * C - 1] = -0.0, -0.0, np.inf, -np.inf     # -0 + -0, inf - inf at (3, 3)
    b_h = rng.standard_normal(C).astype(np.float32)
    b_h[0] = -0.0
    for E in ES:
        q_h = pairs(E)
        q = t(q_h)
        for bias in (b_h, None):
            b = t(bias) if bias is not None else None
            got = {}
            for strided in (False, True):
                Pv, Pw = window(U, 2 * C, strided)
                Pv.copy_(t(P_h))
                out, whole = window(E, C, strided)
                r = LK.pair_gather_add(Pv, q, b, out=out)
                torch.cuda.synchronize()
                assert r.data_ptr() == out.data_ptr() and (not strided or untouched(whole, C))
                want = Pv[q[:, 0], :C] + Pv[q[:, 1], C:]
                if b is not None:
                    want = want + b
                got[strided] = host(out).copy()
                assert LR.same_bits(got[strided], host(want)), (C, E, strided, bias is None)
                assert LR.same_bits(got[strided], LR.gather_add(P_h, q_h, bias))
            # the 16-byte path (contiguous, C % 4 == 0) against the 4-byte path
            assert LR.same_bits(got[False], got[True])
    # pair 6 is (2, 4): -0 + -0 stays -0 without a bias, and is b[0] + -0 = -0 with b[0] = -0 too
    for b in (None, t(b_h)):
        first = host(LK.pair_gather_add(t(P_h), t(pairs(257)), b))[6, 0]
        assert first == 0 and np.signbit(first)


@pytest.mark.parametrize("C", CS)
def test_segment_sum_is_the_restated_chain_bit_for_bit(C):
    from srgnn import link as LK
    rng = np.random.default_rng(200 + C)
    for E in ES:
        q_h = pairs(E)
        inc_ptr, inc_slot = LR.incidence(q_h, U)
        g_h = specials(rng.standard_normal((E, C)).astype(np.float32))
        want = LR.segment_sum(g_h, inc_ptr, inc_slot, U)
        got = {}
        for strided in (False, True):
            gv, _ = window(E, C, strided)
            gv.copy_(t(g_h))
            S, whole = window(U, 2 * C, strided)
            LK.pair_segment_sum(gv, t(inc_ptr), t(inc_slot), out=S)
            torch.cuda.synchronize()
            assert not strided or untouched(whole, 2 * C)
            got[strided] = host(S).copy()
            assert LR.same_bits(got[strided], want), (C, E, strided)
        assert LR.same_bits(got[False], got[True])
        if E == 0:
            assert not got[False].any() and not np.signbit(got[False]).any(), "an empty segment is +0"
        if E == 257 and C >= 47:
            assert got[False][8, 4] == np.float32(1e-41), "the subnormal of the single slot survives"
            assert np.isnan(want[2, 5]) and np.isnan(want[4, C + 5]), "+Inf and -Inf met in one chain"


def test_ids_and_slots_out_of_range_read_as_nothing():
    """The contract of the entries on valid memory: a position outside [0, U) is a row of +0 and a slot outside
    [0, 2E) is skipped; neither is used as an address.  inc_ptr's end is clamped to the 2E slots there are."""
    from srgnn import link as LK
    rng = np.random.default_rng(7)
    for C in (3, 64):
        P_h = rng.standard_normal((U, 2 * C)).astype(np.float32)
        b_h = rng.standard_normal(C).astype(np.float32)
        q_h = pairs(257).copy()
        q_h[0], q_h[1], q_h[2], q_h[3] = (-1, 2), (3, U), (2 ** 40, -2 ** 40), (np.iinfo(np.int64).min, np.iinfo(np.int64).max)
        out = LK.pair_gather_add(t(P_h), t(q_h), t(b_h))
        torch.cuda.synchronize()
        got = host(out)
        assert LR.same_bits(got, LR.gather_add(P_h, q_h, b_h, U))
        assert LR.same_bits(got[2], b_h + np.float32(0)) and LR.same_bits(got[0], P_h[2, C:] + b_h)

        inc_ptr, inc_slot = LR.incidence(pairs(257), U)
        g_h = rng.standard_normal((257, C)).astype(np.float32)
        bad = inc_slot.copy()
        bad[0], bad[7], bad[300], bad[513] = -1, 514, 2 ** 40, np.iinfo(np.int64).min
        ptr = inc_ptr.copy()
        ptr[U] = 514 + 1000
        S = LK.pair_segment_sum(t(g_h), t(ptr), t(bad))
        torch.cuda.synchronize()
        assert LR.same_bits(host(S), LR.segment_sum(g_h, ptr, bad, U))


# ---- pair_linear ------------------------------------------------------------------------------------
def run_pair_linear(z_h, q, W_h, b_h, g_h, n=None):
    from srgnn import link as LK
    z, W, b = (t(a).requires_grad_() for a in (z_h, W_h, b_h))
    out = LK.pair_linear(z, q, W, b)
    out.backward(t(g_h))
    torch.cuda.synchronize()
    return [host(x) for x in (out, z.grad, W.grad, b.grad)]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("h", HS)
def test_pair_linear_within_the_derived_bounds_and_run_to_run_identical(h, C):
    from srgnn import link as LK
    rng = np.random.default_rng(1000 * h + C)
    z_h, W_h, b_h = (rng.standard_normal(s).astype(np.float32) for s in ((U, h), (C, 2 * h), (C,)))
    for E in ES:
        q_h = pairs(E)
        g_h = rng.standard_normal((E, C)).astype(np.float32)
        batch = LK.EdgeBatch(t(q_h), U)
        if E == 257:
            assert np.array_equal(host(batch.n_id), np.arange(U)) and np.array_equal(host(batch.local), q_h)
        if E == 1:                       # the one pair (8, 0) relabels to (1, 0) over n_id = [0, 8]
            assert host(batch.n_id).tolist() == [0, 8] and host(batch.local).tolist() == [[1, 0]]
        first = run_pair_linear(z_h, t(q_h), W_h, b_h, g_h)
        again = run_pair_linear(z_h, t(q_h), W_h, b_h, g_h)
        for a, c in zip(first, again):
            assert LR.same_bits(a, c), "two runs of forward plus backward differ"
        # the EdgeBatch form on the gathered rows: the same bits as the form that gathers inside
        zb = z_h[host(batch.n_id)]
        as_batch = run_pair_linear(zb, batch, W_h, b_h, g_h)
        assert LR.same_bits(as_batch[0], first[0]) and LR.same_bits(as_batch[1], first[1][host(batch.n_id)])
        assert LR.same_bits(as_batch[2], first[2]) and LR.same_bits(as_batch[3], first[3])
        o64, T_out, dz, T_z, dW, T_W, db, T_b = LR.reference64(z_h, q_h, W_h, b_h, g_h)
        bz, bW, bb = LR.backward_bounds(T_z, T_W, T_b, LR.slot_counts(q_h, U), C, E)
        for what, got, want, bound in zip(("out", "dz", "dW", "db"), first, (o64, dz, dW, db),
                                          (LR.forward_bound(T_out, h), bz, bW, bb)):
            err = np.abs(got.astype(np.float64) - want)
            frac = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
            _worst[what] = max(_worst.get(what, 0.0), frac)
            print(f"h={h} C={C} E={E} {what}: worst fraction of the bound {frac:.4f}")
            assert (err <= bound).all(), (what, h, C, E, frac)
    print("worst fractions so far:", {k: round(v, 4) for k, v in _worst.items()})


def test_device_operands_are_fp32():
    from srgnn import link as LK
    z, W = torch.zeros(4, 3, dtype=torch.float64, device=dev()), torch.zeros(2, 6, dtype=torch.float64, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        LK.pair_linear(z, torch.tensor([[0, 1]], device=dev()), W)


# ---- GraphConvolution2 with the fused edge head -----------------------------------------------------
N_G, FEAT, HID, CLS, E_G = 300, 19, 32, 7, 500


@functools.lru_cache(maxsize=None)
def graph():
    """A 300-node random operator (about 5 entries a row, positive and negative values), dense in fp64 too."""
    import scipy.sparse as sp
    from srgnn import graph_conv as GC
    rng = np.random.default_rng(61)
    rows, cols = rng.integers(0, N_G, 1500), rng.integers(0, N_G, 1500)
    A = sp.coo_matrix((rng.standard_normal(1500).astype(np.float32) * 0.5, (rows, cols)), shape=(N_G, N_G)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return GC.GraphConvOperator.from_scipy(A, device=dev()), A.toarray().astype(np.float64)


def models():
    from srgnn import graph_conv as GC
    torch.manual_seed(5)
    a = GC.GraphConvolution2(FEAT, HID, CLS, dropout=0.0).to(dev())
    b = GC.GraphConvolution2(FEAT, HID, CLS, dropout=0.0).to(dev())
    b.load_state_dict(a.state_dict())
    a.adj = b.adj = graph()[0]
    return a, b


def grads(model):
    return {k: host(p.grad) for k, p in model.named_parameters() if p.grad is not None}


def test_fused_edge_head_equals_pair_linear_on_full_rows_bit_for_bit():
    from srgnn import graph_conv as GC
    from srgnn import link as LK
    fused, plain = models()
    rng = np.random.default_rng(62)
    x = t(rng.standard_normal((N_G, FEAT)).astype(np.float32))
    q_h = rng.integers(0, 120, (E_G, 2))                   # endpoints among the first 120 nodes only
    q_h[:3] = ((7, 7), (-1, 5), (5, -1))
    G = t(rng.standard_normal((E_G, CLS)).astype(np.float32))
    batch = LK.EdgeBatch(t(q_h), N_G)
    assert batch.num_nodes < N_G
    fused.fused_edge_head, fused.query_edges = True, batch
    out = fused(x)
    (out * G).sum().backward()

    h = plain.relu(GC.graph_conv(plain.adj, plain.fc1_node_edge(x)))
    z = GC.graph_conv(plain.adj, plain.fc2_edge(h))         # every row
    want = LK.pair_linear(z[batch.n_id], batch, plain.linear.weight, plain.linear.bias)
    (want * G).sum().backward()
    torch.cuda.synchronize()
    assert LR.same_bits(host(out), host(want))
    gf, gp = grads(fused), grads(plain)
    assert sorted(gf) == sorted(gp) == sorted(k for k, _ in fused.named_parameters() if not k.startswith("fc2_node"))
    for k in gf:
        assert LR.same_bits(gf[k], gp[k]), k
    # a tensor of pairs builds the same batch inside; the switch off is the composition as before
    fused.query_edges = t(q_h)
    assert LR.same_bits(host(fused(x)), host(out))
    fused.fused_edge_head = False
    plain.query_edges = t(np.where(q_h < 0, q_h + N_G, q_h))
    assert LR.same_bits(host(fused(x)), host(plain(x)))
    fused.query_edges = batch                                # an EdgeBatch with the switch off: its pairs
    assert LR.same_bits(host(fused(x)), host(plain(x)))


def test_fused_edge_head_against_the_unfused_head_within_the_bounds():
    """Both heads round the same exact value, from the same z (the row path's rows are the full path's, bit for bit):
    they differ by at most the sum of their bounds.  Forward: (h + 3) u T for the fused head, (2h + 2) u T for one
    product of 2h terms plus the bias.  With loss = sum(out * G) both see g = G.  dz: (m + C + 2) u T_z each (the
    unfused one is a product of C terms and an index backward of m terms).  linear.weight: (max m + U + 2) u T_W and
    E u T_W; linear.bias: E u T_b each.  The parameters upstream see J (dz_a - dz_b) plus the roundings of two
    evaluations of the linear map J (adjoint, product with fc2_edge's weight, relu mask, adjoint, products with the
    layer inputs) on inputs no larger than T_z: K = 2 Lmax + hidden + n + 4 roundings along the longest path, so
    |difference| <= |J| ((2 (m + C + 2) + 2 K) u T_z), |J| being J with every factor replaced by its absolute
    value, evaluated in fp64."""
    from srgnn import graph_conv as GC
    from srgnn import link as LK
    fused, plain = models()
    op, A64 = graph()
    rng = np.random.default_rng(63)
    x_h = rng.standard_normal((N_G, FEAT)).astype(np.float32)
    x = t(x_h)
    q_h = rng.integers(0, N_G, (E_G, 2))
    q_h[:2] = ((9, 9), (9, 9))
    G_h = rng.standard_normal((E_G, CLS)).astype(np.float32)
    G = t(G_h)
    fused.fused_edge_head = True
    fused.query_edges = plain.query_edges = t(q_h)
    out_f, out_p = fused(x), plain(x)
    (out_f * G).sum().backward()
    (out_p * G).sum().backward()
    with torch.no_grad():
        c1 = GC.graph_conv(op, plain.fc1_node_edge(x))
        z = GC.graph_conv(op, plain.fc2_edge(plain.relu(c1)))
    torch.cuda.synchronize()
    z_h, c1_h = host(z), host(c1)
    W_h, b_h = host(plain.linear.weight), host(plain.linear.bias)
    u = LR.U32
    _, T_out, _, T_z, _, T_W, _, T_b = LR.reference64(z_h, q_h, W_h, b_h, G_h)
    m = LR.slot_counts(q_h, N_G).astype(np.float64)
    n_u = np.count_nonzero(m)

    def within(what, a, b, bound):
        err = np.abs(host(a).astype(np.float64) - host(b).astype(np.float64))
        frac = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what}: worst fraction of the bound {frac:.4f}")
        assert (err <= bound).all(), (what, frac)

    within("out", out_f, out_p, (HID + 3 + 2 * HID + 2) * u * T_out)
    pf, pp = dict(fused.named_parameters()), dict(plain.named_parameters())
    within("linear.weight", pf["linear.weight"].grad, pp["linear.weight"].grad, (m.max() + n_u + 2 + E_G) * u * T_W)
    within("linear.bias", pf["linear.bias"].grad, pp["linear.bias"].grad, 2 * E_G * u * T_b)
    # upstream: |J| applied to the bound on the two dz
    absA = np.abs(A64)
    Lmax = int((A64 != 0).sum(0).max())
    K = 2 * Lmax + HID + N_G + 4
    D = (2 * (m[:, None] + CLS + 2) + 2 * K) * u * T_z                       # [n, hidden]
    r = np.maximum(c1_h, 0).astype(np.float64)
    da2 = absA.T @ D
    W2 = np.abs(host(plain.fc2_edge.weight).astype(np.float64))
    dc1 = (da2 @ W2) * (c1_h > 0)
    da1 = absA.T @ dc1
    bounds = {"fc2_edge.weight": da2.T @ r, "fc2_edge.bias": da2.sum(0),
              "fc1_node_edge.weight": da1.T @ np.abs(x_h.astype(np.float64)), "fc1_node_edge.bias": da1.sum(0)}
    for k, bound in bounds.items():
        within(k, pf[k].grad, pp[k].grad, bound)
    assert pf["fc2_node.weight"].grad is None and pp["fc2_node.weight"].grad is None


# ---- the memory condition ---------------------------------------------------------------------------
def test_no_buffer_of_the_concatenations_size():
    """At E = 4096, h = 64, C = 3 the rise of max_memory_allocated over forward plus backward of pair_linear, beyond
    the operands (z, the pairs, weight, bias, d out; the EdgeBatch where one is handed over) and the results (out and
    the three gradients), stays below E 2h 4 bytes, the [E, 2h] buffer of the composition; the composition's own rise
    exceeds it, so the condition is not vacuous."""
    from srgnn import link as LK
    E, h, C, n = 4096, 64, 3, 600
    limit = E * 2 * h * 4
    rng = np.random.default_rng(71)
    q = t(rng.integers(0, n, (E, 2)))
    g = t(rng.standard_normal((E, C)).astype(np.float32))
    z0, W0, b0 = (t(rng.standard_normal(s).astype(np.float32)) for s in ((n, h), (C, 2 * h), (C,)))
    batch = LK.EdgeBatch(q, n)
    batch.incidence()
    zb0 = z0[batch.n_id].contiguous()

    def fused_tensor(z, W, b):
        return LK.pair_linear(z, q, W, b)

    def fused_batch(z, W, b):
        return LK.pair_linear(z, batch, W, b)

    def composition(z, W, b):
        return torch.nn.functional.linear(torch.cat((z[q[:, 0]], z[q[:, 1]]), dim=-1), W, b)

    def rise(fn, zsrc):
        for measured in (False, True):                      # once to warm the GEMMs' workspaces up, once measured
            z, W, b = (a.clone().requires_grad_() for a in (zsrc, W0, b0))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn(z, W, b)
            out.backward(g)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            results = sum(x.numel() * x.element_size() for x in (out, z.grad, W.grad, b.grad))
        return peak - base - results

    r_tensor, r_batch, r_comp = rise(fused_tensor, z0), rise(fused_batch, zb0), rise(composition, z0)
    print(f"rise beyond operands and results: pairs as a tensor {r_tensor} B, as an EdgeBatch {r_batch} B, "
          f"the composition {r_comp} B; E 2h 4 = {limit} B")
    assert r_comp > limit, "the composition no longer builds its [E, 2h] buffer: the condition below is vacuous"
    assert r_tensor < limit and r_batch < limit
