"""The recursive hop attention (IterateLearnableWeightedMessageOp, combination type recursive, start == 0)
restated in numpy fp64, with a first-order rounding bound carried beside every value: the expected values and
the tolerances of tests/test_hop_recursive_{cpu,gpu}.py.  The derivation is DESIGN.md §5.4.3; the rules are
those of tests/hop_attention_ref.py, with eps = 2^-24:

  a k-term sum of products, in any order, is within   k * eps * sum |terms|   of its exact value (a product of
  three factors rounds once more: k + 1);
  a 1-ulp expf is 2 eps relative; a correctly rounded add, multiply or divide 1 eps relative;
  an input's error goes through a differentiable step multiplied by the step's derivative.

The reference combines the panels and then takes the dot product with w_c; the device takes the dot products
q_j = w_c . F_j and then combines them.  Both are sums of the i * d triple products W_j * w_c[c] * F_j[., c], in
different orders, so r_i is bounded as such a sum taken in any order, plus the error carried in W(i-1).
Nothing here is fitted to a result: every constant counts operations of the formula.

Special values ("Special values and saturation").  A bound is finite wherever its value is
finite; the zero factors that meet an infinite bound are exact for the reasons of hop_attention_ref: at
s = +-inf (an Inf cell in a panel) g = 1 / (1 + exp(-s)) is exactly 1 or 0 in both precisions, so
g (1 - g) (E_s + 2 eps) and g (1 - g) times a bound are 0; and W(0) = softmax([g_0]) is the constant 1 for every g_0
that is not NaN, so its zero bound times |q_0| = inf is 0.  Where s_0 = p_0 + q_0 + b is NaN the reference's
one-column softmax is NaN and so is the whole row: W(0) = NaN there, not 1.  classes, check_special and underflow_allowance are hop_attention_ref's.
"""
import numpy as np

from hop_attention_ref import (EPS, _zmul, check_special, classes, rows_per_group, underflow_allowance,  # noqa: F401
                               worst_ratio)

HERE_CASES = (
    # name, T, end, n, d, seed
    ("rec_t4", 4, 4, 37, 12, 21),
    ("rec_gamlp", 11, 11, 33, 128, 22),
    ("rec_end3of5", 5, 3, 50, 7, 23),
    ("rec_d1", 5, 5, 129, 1, 24),
    ("rec_h2", 2, 2, 40, 130, 25),
    ("rec_h1", 1, 1, 20, 9, 26),
    ("rec_n1", 3, 3, 1, 5, 27),
)
CASES = {c[0]: dict(zip(("name", "T", "end", "n", "d", "seed"), c)) for c in HERE_CASES}


def work_floats(H):
    """Floats per row of the recurrence's work buffer: the triangle of weights and the H gates."""
    return H * (H + 1) // 2 + H


def evaluate(hops, end, w, b, G=None, nested=True, swap_halves=False, jacobian=True, drop_dq=False):
    """The formula in fp64 on the given fp32 values over hops[0 : end].  Returns a dict of values and, under
    "E_<name>", the bound on |fp32 result - value| of a computation that follows the formula with the operation
    counts above: zp / zq / E_zp / E_zq [H, n], P / E_P [n, H], out / E_out [n, d] and, with G = dL/dout,
    dw / E_dw [2d], db / E_db.  The keyword arguments put in the mistakes of the negative controls:
    nested=False: one plain softmax over the raw gates g_0 .. g_i at every step; swap_halves: w_c meets the hop
    and w_h the combination; jacobian=False: a backward without g (1 - g); drop_dq: a backward that treats
    the running combination as a constant."""
    H = int(end)
    F = [np.asarray(h, dtype=np.float64) for h in hops[:H]]
    A = [np.abs(f) for f in F]
    n, d = F[0].shape
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    b = float(np.asarray(b, dtype=np.float64).reshape(-1)[0])
    assert w.size == 2 * d
    wh, wc = (w[d:], w[:d]) if swap_halves else (w[:d], w[d:])

    # the 2H dot products: d-term sums of products
    p = np.stack([f @ wh for f in F])
    q = np.stack([f @ wc for f in F])
    pa = np.stack([a @ np.abs(wh) for a in A])
    qa = np.stack([a @ np.abs(wc) for a in A])
    E_zp, E_zq = d * EPS * pa, d * EPS * qa

    # forward recurrence; Ws[i] / EWs[i]: [i + 1, n]
    # W(0) = softmax([g_0]): exactly 1 for every g_0 but NaN, which the reference's one-column softmax hands on
    s0 = p[0] + q[0] + b
    Ws, EWs = [np.where(np.isnan(s0), np.nan, 1.0)[None]], [np.zeros((1, n))]
    g, E_g = np.zeros((H, n)), np.zeros((H, n))
    sc = np.zeros((H, n))           # the gate scores s_1 .. s_{H-1} (row 0 unused)
    graw = None
    if not nested:
        graw = [1.0 / (1.0 + np.exp(-(p[0] + q[0] + b)))]
    for i in range(1, H):
        W, EW = Ws[-1], EWs[-1]
        # s = p_i + sum_{j<i} W_j q_j + b: d products, i d triple products and the bias, in any order
        r = (W * q[:i]).sum(axis=0)
        s = p[i] + r + b
        sc[i] = s
        E_s = (d + i * d + 2) * EPS * (pa[i] + (W * qa[:i]).sum(axis=0) + abs(b)) + _zmul(EW, np.abs(q[:i])).sum(axis=0)
        # g = 1 / (1 + u), u = exp(-s): as a of hop_attention_ref
        g[i] = 1.0 / (1.0 + np.exp(-s))
        E_g[i] = _zmul(g[i] * (1.0 - g[i]), E_s + 2 * EPS) + 2 * EPS * g[i]
        if nested:
            x, E_x = np.vstack([W, g[i][None]]), np.vstack([EW, E_g[i][None]])
        else:
            graw.append(g[i])
            x, E_x = np.stack(graw), np.zeros((i + 1, n))
        # e = exp(x): relative x's error and 2 eps; W' = e_j / sum e: its own relative error, the sum's (a
        # W'-weighted mean of the terms', i adds), the divide
        e = np.exp(x)
        r_e = E_x + 2 * EPS
        Wn = e / e.sum(axis=0, keepdims=True)
        Ws.append(Wn)
        EWs.append(Wn * (r_e + (Wn * r_e).sum(axis=0, keepdims=True) + (i + 1) * EPS))
    P, E_P = Ws[-1].T, EWs[-1].T
    # out: P's error on each term; H products and H - 1 adds: H terms
    out = sum(P[:, h:h + 1] * F[h] for h in range(H))
    scale = sum(P[:, h:h + 1] * A[h] for h in range(H))
    E_out = sum(E_P[:, h:h + 1] * A[h] for h in range(H)) + H * EPS * scale
    res = dict(zp=p, zq=q, E_zp=E_zp, E_zq=E_zq, P=P, E_P=E_P, out=out, E_out=E_out, scale=scale, g=g, Ws=Ws, s=sc)
    if G is None:
        return res

    G = np.asarray(G, dtype=np.float64)
    # dW(H-1)_j = G . F_j: d terms
    dW = np.stack([(G * F[h]).sum(axis=1) for h in range(H)])
    E_dW = d * EPS * np.stack([(np.abs(G) * A[h]).sum(axis=1) for h in range(H)])
    dp, E_dp = np.zeros((H, n)), np.zeros((H, n))
    dq, E_dq, dq_abs = np.zeros((H, n)), np.zeros((H, n)), np.zeros((H, n))
    for i in range(H - 1, 0, -1):
        W, EW, Wp, EWp = Ws[i], EWs[i], Ws[i - 1], EWs[i - 1]
        # t = sum_j W_j dW_j: i + 1 terms on top of the factors' errors
        t = (W * dW).sum(axis=0)
        E_t = (EW * np.abs(dW) + W * E_dW).sum(axis=0) + (i + 1) * EPS * np.abs(W * dW).sum(axis=0)
        u = dW - t
        E_u = E_dW + E_t + EPS * np.abs(u)
        dx = W * u
        E_dx = EW * np.abs(u) + W * E_u + EPS * np.abs(dx)
        # jac = g (1 - g): |d jac / dg| <= 1; the subtraction and the product round once each
        if jacobian:
            jac = g[i] * (1.0 - g[i])
            E_jac = E_g[i] + 2 * EPS * jac
        else:
            jac, E_jac = np.ones(n), np.zeros(n)
        ds = dx[i] * jac
        E_ds = _zmul(jac, E_dx[i]) + np.abs(dx[i]) * E_jac + EPS * np.abs(ds)
        dp[i], E_dp[i] = ds, E_ds
        if drop_dq:
            dW, E_dW = dx[:i], E_dx[:i]
            continue
        # dq_j gathers ds_i W(i-1)_j over the steps i > j: the factors' errors now, the H - 1 - j terms'
        # roundings (a product each, the adds between them) below
        m = ds * Wp
        dq[:i] += m
        dq_abs[:i] += np.abs(m)
        E_dq[:i] += E_ds * Wp + np.abs(ds) * EWp
        # dW(i-1)_j = dx_j + ds q_j: ds (w_c . F_j) is a d-term sum of triple products in any order, then the add
        dWn = dx[:i] + ds * q[:i]
        E_dW = E_dx[:i] + E_ds * np.abs(q[:i]) + (d + 1) * EPS * np.abs(ds) * qa[:i] + EPS * np.abs(dWn)
        dW = dWn
    terms = (H - 1 - np.arange(H))[:, None]
    E_dq = E_dq + terms * EPS * dq_abs

    # the two reduction stages: a term passes through at most (rows of its group) adds in stage 1 and (number
    # of groups) adds in stage 2; each half of dw adds the group's H panel chains besides
    rpg = min(rows_per_group(n), n)
    groups = -(-n // rows_per_group(n))
    depth = rpg + groups
    s = dp.sum(axis=0)
    E_s = E_dp.sum(axis=0) + H * EPS * np.abs(dp).sum(axis=0)
    db = s.sum()
    E_db = E_s.sum() + depth * EPS * np.abs(s).sum()
    dw, E_dw = np.zeros(2 * d), np.zeros(2 * d)
    for half, (dz, E_dz) in enumerate(((dp, E_dp), (dq, E_dq))):
        dw[half * d:(half + 1) * d] = sum(dz[h] @ F[h] for h in range(H))
        E_dw[half * d:(half + 1) * d] = sum(E_dz[h] @ A[h] for h in range(H)) + \
            (depth + H) * EPS * sum(np.abs(dz[h]) @ A[h] for h in range(H))
    if swap_halves:     # the gradients go back to the halves they were taken from
        dw, E_dw = np.concatenate([dw[d:], dw[:d]]), np.concatenate([E_dw[d:], E_dw[:d]])
    res.update(dzp=dp, dzq=dq, E_dzp=E_dp, E_dzq=E_dq, dw=dw, E_dw=E_dw, db=db, E_db=np.float64(E_db))
    return res


def check(what, got_out, got_dw, got_db, ref):
    """Asserts out, dw and db within their bounds of `ref` (evaluate's result); prints the three ratios."""
    assert np.isfinite(np.asarray(got_out)).all(), f"{what}: non-finite out"
    r = (worst_ratio(got_out, ref["out"], ref["E_out"]), worst_ratio(got_dw, ref["dw"], ref["E_dw"]),
         worst_ratio(got_db, ref["db"], ref["E_db"]))
    print(f"recursive hop attention |got - exact| / bound  {what}: out {r[0]:.4f}  dw {r[1]:.4f}  db {r[2]:.4f}")
    assert r[0] <= 1.0, f"{what}: out at {r[0]:.3f} of the bound"
    assert r[1] <= 1.0, f"{what}: weight gradient at {r[1]:.3f} of the bound"
    assert r[2] <= 1.0, f"{what}: bias gradient at {r[2]:.3f} of the bound"
    return r


def load_case(z, name):
    """(case, hops, w, b, C, out, dw, db) of fixture `name` from the loaded hop_recursive.npz."""
    c = CASES[name]
    hops = [z[f"{name}__hop{t}"] for t in range(c["T"])]
    return (c, hops, z[f"{name}__weight"], z[f"{name}__bias"], z[f"{name}__C"], z[f"{name}__out"],
            z[f"{name}__grad_weight"], z[f"{name}__grad_bias"])


def random_case(n, d, T, seed):
    """Seeded hops (correlated, O(1)), parameters drawn as Linear's default init, and a cotangent."""
    rng = np.random.default_rng(seed)
    hops = [rng.standard_normal((n, d)).astype(np.float32)]
    for _ in range(1, T):
        hops.append((0.6 * hops[-1] + 0.4 * rng.standard_normal((n, d))).astype(np.float32))
    lim = 1.0 / np.sqrt(2 * d)
    w = rng.uniform(-lim, lim, (1, 2 * d)).astype(np.float32)
    b = rng.uniform(-lim, lim, (1,)).astype(np.float32)
    C = rng.standard_normal((n, d)).astype(np.float32)
    return hops, w, b, C
