"""The learnable hop attention (LearnableWeightedMessageOp gate / ori_ref / jk) restated in numpy fp64, with
a first-order rounding bound carried beside every value: the expected values and the tolerances of
tests/test_hop_attention_{cpu,gpu}.py.  The derivation is DESIGN.md §5.4.2; in short, with eps = 2^-24,

  a k-term sum of products, in any order, is within   k * eps * sum |terms|   of its exact value;
  a 1-ulp expf is 2 eps relative; a correctly rounded add, multiply or divide 1 eps relative;
  an input's error goes through a differentiable step multiplied by the step's derivative.

Nothing here is fitted to a result: every constant counts operations of the formula.

Special values ("Special values and saturation").  A bound is finite wherever its value is
finite.  The only place a zero factor meets an infinite bound is the sigmoid at S = +-inf (an Inf cell in a
panel the score reads): both precisions give a = 1 / (1 + exp(-S)) = 1 or 0 EXACTLY there (exp gives 0 or +inf,
1 + 0 = 1, 1 / inf = 0), so a carries no error of the score and a (1 - a) (E_S + 2 eps) is 0, not 0 * inf = NaN;
the same holds for the Jacobian j = a (1 - a) = 0 times an infinite bound of its other factor.  _zmul is that
product.  classes / check_special compare results that hold NaN or +-Inf on purpose: the class of every
element (finite, NaN, +Inf, -Inf) must be the restatement's, and the finite ones lie within their bound.

Underflow.  eps-relative error holds for an fp32 operation whose exact result is at least 2^-126 in magnitude;
below that the result is rounded to a multiple of 2^-149, an ABSOLUTE error of at most 2^-150.  out is H
products (the adds of subnormal terms are exact), so a row of subnormal panel cells adds at most
underflow_allowance(H) = H * 2^-150 to E_out.  It is a property of the format, used by the denormal-row tests
only; evaluate's bounds are unchanged by it.
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -150          # half the spacing of the fp32 subnormals: the absolute error of an underflowing operation
FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3
HERE_CASES = (
    # name, kind, T, start, end, n, d, constructor arguments after (start, end, kind), seed
    ("jk_t4", "jk", 4, 0, 4, 37, 12, (3, 12), 11),
    ("jk_gamlp", "jk", 11, 0, 11, 33, 128, (10, 128), 12),
    ("jk_inner", "jk", 4, 1, 3, 50, 7, (3, 7), 13),
    ("ori_ref_d130", "ori_ref", 5, 1, 5, 40, 130, (130,), 14),
    ("gate_d1", "gate", 5, 0, 5, 129, 1, (1,), 15),
    ("gate_h1", "gate", 4, 2, 3, 20, 9, (9,), 16),
    ("jk_n1", "jk", 3, 0, 3, 1, 5, (2, 5), 17),
)
CASES = {c[0]: dict(zip(("name", "kind", "T", "start", "end", "n", "d", "args", "seed"), c)) for c in HERE_CASES}


def in_dim(kind, T, d):
    return {"gate": d, "ori_ref": 2 * d, "jk": T * d + d}[kind]


def underflow_allowance(ops):
    """What `ops` fp32 operations whose exact results may lie below 2^-126 add to an absolute bound."""
    return ops * TINY


def _zmul(x, y):
    """x * y for a value x >= 0 and a bound y >= 0, with 0 * inf = 0: the cases where x is exactly 0 in fp32 and
    in fp64 alike (the module docstring says why each is exact), so nothing of y reaches the result."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((x == 0) & np.isposinf(y), 0.0, x * y)


def classes(x):
    """An int array of x's shape: FINITE 0, NAN 1, POS_INF 2, NEG_INF 3."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), NAN, np.where(np.isposinf(x), POS_INF, np.where(np.isneginf(x), NEG_INF, FINITE))).astype(np.int8)


def rows_per_group(n):
    """Stage 1 of the parameter gradient: the smallest 32 * 2^k with rpg * 2048 >= n (include/srgnn_hip.h)."""
    rpg = 32
    while rpg * 2048 < n:
        rpg *= 2
    return rpg


def _pair(z, flat):
    """S [n, H] from the hop-major scores z [H, n]: the reference's .view(-1, H) or the transpose."""
    H, n = z.shape
    return z.reshape(-1).reshape(n, H) if flat else z.T


def _unpair(S, flat):
    n, H = S.shape
    return S.reshape(-1).reshape(H, n) if flat else S.T


def evaluate(kind, hops, start, end, w, b, G=None, pairing=None, jacobian=True, swap=None):
    """The formula in fp64 on the given fp32 values.  Returns a dict of values and, under "E_<name>", the
    bound on |fp32 result - value| of a computation that follows the formula with the operation counts
    above: out / E_out [n, d], P / E_P [n, H] and, with G = dL/dout, dw / E_dw [in_dim], db / E_db.
    pairing ("flat" / "transpose"), jacobian=False and swap=(h, k) -- the weights of slice positions h and k
    applied to each other's panels -- put in the mistakes of the negative controls."""
    F = [np.asarray(h, dtype=np.float64) for h in hops]
    A = [np.abs(f) for f in F]
    T, (n, d) = len(F), F[0].shape
    H = end - start
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    b = float(np.asarray(b, dtype=np.float64).reshape(-1)[0])
    R = in_dim(kind, T, d) - d
    assert w.size == R + d
    refs = list(range(T)) if kind == "jk" else [0] if kind == "ori_ref" else []
    flat = (kind != "gate") if pairing is None else pairing == "flat"
    pos = list(range(H))
    if swap is not None:
        pos[swap[0]], pos[swap[1]] = pos[swap[1]], pos[swap[0]]
    Fc, Ac = [F[start + p] for p in pos], [A[start + p] for p in pos]      # the panels the weights meet

    # scores: in_dim products, the adds between them and the bias: (in_dim + 2) terms
    hop = np.stack([F[start + h] @ w[R:] for h in range(H)])
    hop_abs = np.stack([A[start + h] @ np.abs(w[R:]) for h in range(H)])
    ref = sum((F[t] @ w[t * d:(t + 1) * d] for t in refs), np.zeros(n))
    ref_abs = sum((A[t] @ np.abs(w[t * d:(t + 1) * d]) for t in refs), np.zeros(n))
    z = ref[None, :] + hop + b
    E_z = (R + d + 2) * EPS * (ref_abs[None, :] + hop_abs + abs(b))
    S, E_S = _pair(z, flat), _pair(E_z, flat)

    # a = 1 / (1 + u), u = exp(-S): u is off by the score's error and the exp's 2 eps, relative, which
    # reach a scaled by u / (1 + u) = 1 - a; the add and the divide round once each
    a = 1.0 / (1.0 + np.exp(-S))
    E_a = _zmul(a * (1.0 - a), E_S + 2 * EPS) + 2 * EPS * a
    # e = exp(a), relative: a's error, 2 eps
    e = np.exp(a)
    r_e = E_a + 2 * EPS
    # P = e_h / sum e: own relative error, the sum's (a P-weighted mean of the terms', H - 1 adds), the divide
    P = e / e.sum(axis=1, keepdims=True)
    E_P = P * (r_e + (P * r_e).sum(axis=1, keepdims=True) + H * EPS)
    # out: P's error on each term; H products and H - 1 adds: H terms
    out = sum(P[:, h:h + 1] * Fc[h] for h in range(H))
    scale = sum(P[:, h:h + 1] * Ac[h] for h in range(H))
    E_out = sum(E_P[:, h:h + 1] * Ac[h] for h in range(H)) + H * EPS * scale
    res = dict(z=z, E_z=E_z, P=P, E_P=E_P, out=out, E_out=E_out, scale=scale)
    if G is None:
        return res

    G = np.asarray(G, dtype=np.float64)
    # dP = G . F_h: d terms
    dP = np.stack([(G * Fc[h]).sum(axis=1) for h in range(H)], axis=1)
    E_dP = d * EPS * np.stack([(np.abs(G) * Ac[h]).sum(axis=1) for h in range(H)], axis=1)
    # t = sum_h P_h dP_h: H terms on top of the factors' errors
    t = (P * dP).sum(axis=1, keepdims=True)
    E_t = (E_P * np.abs(dP) + P * E_dP).sum(axis=1, keepdims=True) + H * EPS * np.abs(P * dP).sum(axis=1, keepdims=True)
    u = dP - t
    E_u = E_dP + E_t + EPS * np.abs(u)
    da = P * u
    E_da = E_P * np.abs(u) + P * E_u + EPS * np.abs(da)
    # j = a (1 - a): |dj/da| = |1 - 2a| <= 1; the subtraction and the product round once each
    if jacobian:
        j = a * (1.0 - a)
        E_j = E_a + 2 * EPS * j
    else:
        j, E_j = np.ones_like(a), np.zeros_like(a)
    dS = da * j
    E_dS = _zmul(j, E_da) + np.abs(da) * E_j + EPS * np.abs(dS)
    dz, E_dz = _unpair(dS, flat), _unpair(E_dS, flat)

    # the two reduction stages: a term passes through at most (rows of its group) adds in stage 1 and
    # (number of groups) adds in stage 2; the hop part adds the group's H hop chains besides
    rpg = min(rows_per_group(n), n)
    groups = -(-n // rows_per_group(n))
    depth = rpg + groups
    s = dz.sum(axis=0)
    E_s = E_dz.sum(axis=0) + H * EPS * np.abs(dz).sum(axis=0)
    db = s.sum()
    E_db = E_s.sum() + depth * EPS * np.abs(s).sum()
    dw, E_dw = np.zeros(R + d), np.zeros(R + d)
    for t_ in refs:
        dw[t_ * d:(t_ + 1) * d] = s @ F[t_]
        E_dw[t_ * d:(t_ + 1) * d] = E_s @ A[t_] + depth * EPS * (np.abs(s) @ A[t_])
    dw[R:] = sum(dz[h] @ F[start + h] for h in range(H))
    E_dw[R:] = sum(E_dz[h] @ A[start + h] for h in range(H)) + \
        (depth + H) * EPS * sum(np.abs(dz[h]) @ A[start + h] for h in range(H))
    res.update(dP=dP, dz=dz, E_dz=E_dz, dw=dw, E_dw=E_dw, db=db, E_db=np.float64(E_db))
    return res


def worst_ratio(got, want, bound):
    """max |got - want| / bound (0 / 0 counts as 0, x / 0 as inf)."""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(want))
    err = np.abs(got - want)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


def check(what, got_out, got_dw, got_db, ref):
    """Asserts out, dw and db within their bounds of `ref` (evaluate's result); prints the three ratios."""
    assert np.isfinite(np.asarray(got_out)).all(), f"{what}: non-finite out"
    r = (worst_ratio(got_out, ref["out"], ref["E_out"]), worst_ratio(got_dw, ref["dw"], ref["E_dw"]),
         worst_ratio(got_db, ref["db"], ref["E_db"]))
    print(f"hop attention |got - exact| / bound  {what}: out {r[0]:.4f}  dw {r[1]:.4f}  db {r[2]:.4f}")
    assert r[0] <= 1.0, f"{what}: out at {r[0]:.3f} of the bound"
    assert r[1] <= 1.0, f"{what}: weight gradient at {r[1]:.3f} of the bound"
    assert r[2] <= 1.0, f"{what}: bias gradient at {r[2]:.3f} of the bound"
    return r


def check_special(what, got, want, bound):
    """For results that hold non-finite values on purpose: the class of every element of `got` is `want`'s, and
    where that class is finite |got - want| <= bound (which must be finite there).  Prints and returns the worst
    finite ratio."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    cg, cw = classes(got), classes(want)
    bad = np.argwhere(cg != cw)
    assert bad.size == 0, (f"{what}: {len(bad)} elements of another class (0 finite, 1 NaN, 2 +Inf, 3 -Inf), first at "
                           f"{tuple(bad[0])}: got {cg[tuple(bad[0])]}, expected {cw[tuple(bad[0])]}")
    fin = cw == FINITE
    assert np.isfinite(bound[fin]).all(), f"{what}: a bound is not finite where its value is"
    r = worst_ratio(got[fin], want[fin], bound[fin])
    print(f"special values |got - exact| / bound  {what}: {r:.4f} over {int(fin.sum())} finite of {fin.size} elements")
    assert r <= 1.0, f"{what}: a finite element at {r:.3f} of the bound"
    return r


def load_case(z, name):
    """(case, hops, w, b, C, out, dw, db) of fixture `name` from the loaded hop_attention.npz."""
    c = CASES[name]
    hops = [z[f"{name}__hop{t}"] for t in range(c["T"])]
    return (c, hops, z[f"{name}__weight"], z[f"{name}__bias"], z[f"{name}__C"], z[f"{name}__out"],
            z[f"{name}__grad_weight"], z[f"{name}__grad_bias"])


def random_case(kind, n, d, T, start, end, seed):
    """Seeded hops (correlated, O(1)), parameters drawn as Linear's default init, and a cotangent."""
    rng = np.random.default_rng(seed)
    hops = [rng.standard_normal((n, d)).astype(np.float32)]
    for _ in range(1, T):
        hops.append((0.6 * hops[-1] + 0.4 * rng.standard_normal((n, d))).astype(np.float32))
    k = in_dim(kind, T, d)
    lim = 1.0 / np.sqrt(k)
    w = rng.uniform(-lim, lim, (1, k)).astype(np.float32)
    b = rng.uniform(-lim, lim, (1,)).astype(np.float32)
    C = rng.standard_normal((n, d)).astype(np.float32)
    return hops, w, b, C
