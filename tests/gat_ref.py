"""The fused GAT aggregation (srgnn.gat) restated: in numpy fp64 with a first-order rounding
bound carried beside every value (evaluate), in numpy fp32 bit for bit where the bits are pinned (one entry
per row; zero attention vectors), and as the torch composition from primitives that the fused layer replaces
(compose).  The expected values and tolerances of tests/test_gat_{cpu,gpu}.py.

The rules of the bound are those of tests/hop_attention_ref.py, with eps = 2^-24:
  a k-term sum of products, in any order, is within k * eps * sum |terms| of its exact value;
  a 1-ulp expf is 2 eps relative; a correctly rounded add, subtract, multiply or divide 1 eps relative;
  an input's error goes through a differentiable step multiplied by the step's derivative.
Nothing is fitted to a result: every constant counts operations of the formula.

Per row i (length len), head h, entry e with source j_e; x_e = Hf[j_e, h*C:(h+1)*C]:
  s = a_src[j] + a_dst[i]                       E_s = E_asrc + E_adst + eps |s|
  l = s > 0 ? s : slope s                       E_l = E_s + eps |l|           (|dl/ds| <= 1)
  m = max l                                     E_M = max E_l                 (kept for M only: the softmax is
                                                                               shift-invariant, m's error cancels)
  p = exp(l - m)                                r = E_l + eps |l - m| + 2 eps (relative)
  z = sum p                                     E_Z = sum p (r + E_M + len eps)   (M's error shifts every p alike)
  alpha = p / z                                 E_alpha = alpha (r + sum_k alpha_k r_k + (len + 1) eps)
  out = sum alpha x                             E_out = sum (E_alpha |x| + alpha E_x) + (len + 1) eps sum alpha |x|
  D = sum_c G out                               E_D = sum_c (|G| E_out + E_G |out|) + C eps sum_c |G out|
  dalpha = sum_c G x                            E_dalpha = sum_c (E_G |x| + |G| E_x) + C eps sum_c |G x|
  u = dalpha - D                                E_u = E_dalpha + E_D + eps |u|
  t = alpha u                                   E_t = E_alpha |u| + alpha E_u + eps |t|
  ds = t (s > 0 ? 1 : slope)                    E_ds = E_t deriv + eps |ds|   (outside the band |s| <= 4 E_s)
  da_dst[i] = sum over row i of ds              E = sum E_ds + len eps sum |ds|
  da_src[j] = sum over row j of At of ds        E = sum E_ds + len_t eps sum |ds|
  dHf[j] = sum over row j of At of alpha G[i]   E = sum (E_alpha |G| + alpha E_G) + len_t eps sum alpha |G|
The device divides the chain of p x by z instead of summing alpha x; its error, sum alpha |x| (r + sum alpha r
+ (len + 1) eps) + len eps sum alpha |x|, lies within E_out.
"""
import numpy as np
import torch

EPS = 2.0 ** -24
TINY = 2.0 ** -150
N = 400
STAR, ISOLATED = 7, (3, 11)
SHAPES = ((1, 1), (1, 47), (3, 7), (8, 16), (4, 64), (2, 65), (1, 260))       # (H, C)
GRAPHS = ("asym", "sym")


# ---- graphs -----------------------------------------------------------------------------------------
def base_edges(kind, n=N, seed=5):
    """(dst, src) of the base graph: node 7 has 320 incoming edges, nodes 3 and 11 touch no edge, the rest a
    thin random directed graph with a few existing self-loops; "sym" adds every edge's reverse.  Pairs are
    unique, in a shuffled order (rows come out unsorted)."""
    rng = np.random.default_rng(seed)
    live = np.setdiff1d(np.arange(n), ISOLATED)
    e = 900
    dst, src = rng.choice(live, e), rng.choice(live, e)
    star = rng.choice(np.setdiff1d(live, [STAR]), 319, replace=False)
    dst, src = np.r_[dst, np.full(star.size, STAR), STAR, 20, 21], np.r_[src, star, STAR, 20, 21]
    if kind == "sym":
        dst, src = np.r_[dst, src], np.r_[src, dst]
    key = np.unique(dst.astype(np.int64) * n + src)
    key = key[rng.permutation(key.size)]
    return key // n, key % n


def csr_of(dst, src, n, self_loops):
    """The scipy-free restatement of GATGraph's structure: (indptr int64, indices int32).  Without self-loops
    a stable sort by target (entries keep their order); with them the diagonal entries are dropped, one is
    added per node and every row is sorted by source (stable, so duplicates stay)."""
    dst, src = np.asarray(dst, dtype=np.int64), np.asarray(src, dtype=np.int64)
    if self_loops:
        keep = dst != src
        dst, src = np.r_[dst[keep], np.arange(n)], np.r_[src[keep], np.arange(n)]
        order = np.lexsort((src, dst))
    else:
        order = np.argsort(dst, kind="stable")
    dst, src = dst[order], src[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, dst + 1, 1)
    return np.cumsum(ptr), src.astype(np.int32)


def transpose_of(ip, ix, n):
    """(indptr_t, indices_t, perm): csr_transpose's definition, a stable sort of the entries by column."""
    rows = entry_rows(ip)
    perm = np.argsort(ix.astype(np.int64), kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ptr, ix.astype(np.int64) + 1, 1)
    return np.cumsum(ptr), rows[perm].astype(np.int32), perm.astype(np.int64)


def entry_rows(ip):
    return np.repeat(np.arange(ip.size - 1, dtype=np.int64), np.diff(ip))


_graphs = {}


def graph(kind, self_loops):
    """(indptr, indices) of a base graph, built once."""
    key = (kind, bool(self_loops))
    if key not in _graphs:
        dst, src = base_edges(kind)
        _graphs[key] = csr_of(dst, src, N, self_loops)
    return _graphs[key]


def inputs(n, H, C, seed, scale=1.0):
    """(Hf [n, H*C], a_src, a_dst [n, H], G [n, H*C]) fp32, O(1), seeded."""
    rng = np.random.default_rng(seed)
    Hf = rng.standard_normal((n, H * C)).astype(np.float32)
    a_src = (scale * rng.standard_normal((n, H))).astype(np.float32)
    a_dst = (scale * rng.standard_normal((n, H))).astype(np.float32)
    G = rng.standard_normal((n, H * C)).astype(np.float32)
    return Hf, a_src, a_dst, G


def case_seed(kind, self_loops, H, C):
    return 1000 * (GRAPHS.index(kind) + 1) + 100 * int(self_loops) + 7 * H + C


# ---- the fp64 restatement with its bound ------------------------------------------------------------
def _seg(vals, rows, n, op=np.add, init=0.0):
    out = np.full((n,) + vals.shape[1:], init, dtype=np.float64)
    op.at(out, rows, vals)
    return out


def evaluate(ip, ix, Hf, a_src, a_dst, slope=0.2, G=None, E_x=None, E_asrc=None, E_adst=None, E_G=None,
             mistake=None):
    """Values and bounds (under "E_<name>") of out, M, Z and, with G, ds, da_dst, da_src, dHf; "band" counts
    the entries with |s| <= 4 E_s, which the bound does not cover.  E_x, E_asrc, E_adst, E_G: bounds on the
    errors the inputs already carry (default: exact).  mistake: "softmax_over_sources", "no_D" or
    "derivative_one" put in the mistakes of the negative controls."""
    ip, ix = np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int64)
    n = ip.size - 1
    a_src, a_dst = np.asarray(a_src, dtype=np.float64), np.asarray(a_dst, dtype=np.float64)
    H = a_src.shape[1]
    X = np.asarray(Hf, dtype=np.float64).reshape(n, H, -1)
    C = X.shape[2]
    zero = np.zeros((n, H))
    E_asrc = zero if E_asrc is None else np.asarray(E_asrc, dtype=np.float64)
    E_adst = zero if E_adst is None else np.asarray(E_adst, dtype=np.float64)
    E_x = np.zeros_like(X) if E_x is None else np.asarray(E_x, dtype=np.float64).reshape(X.shape)
    rows = entry_rows(ip)
    ln = np.diff(ip).astype(np.float64)[:, None]                       # [n, 1]
    seg = rows if mistake != "softmax_over_sources" else ix            # what the softmax normalises over

    s = a_src[ix] + a_dst[rows]                                        # [nnz, H]
    E_s = E_asrc[ix] + E_adst[rows] + EPS * np.abs(s)
    band = int((np.abs(s) <= 4 * E_s).sum())
    l = np.where(s > 0, s, slope * s)
    E_l = E_s + EPS * np.abs(l)
    m = _seg(l, seg, n, np.maximum, -np.inf)
    E_M = _seg(E_l, seg, n, np.maximum, 0.0)
    has = np.isfinite(m)
    m = np.where(has, m, 0.0)
    p = np.exp(l - m[seg])
    r = E_l + EPS * np.abs(l - m[seg]) + 2 * EPS
    z = _seg(p, seg, n)
    lz = ln if mistake != "softmax_over_sources" else _seg(np.ones((ix.size, 1)), ix, n)
    E_Z = _seg(p * (r + E_M[seg]), seg, n) + lz * EPS * z
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(z[seg] > 0, p / z[seg], 0.0)
    ar = _seg(alpha * r, seg, n)
    E_alpha = alpha * (r + ar[seg] + (lz[seg] + 1) * EPS)
    msg = alpha[:, :, None] * X[ix]                                    # [nnz, H, C]
    out = _seg(msg, rows, n)
    scale = _seg(np.abs(msg), rows, n)
    E_out = _seg(E_alpha[:, :, None] * np.abs(X[ix]) + alpha[:, :, None] * E_x[ix], rows, n) + \
        (ln[:, :, None] + 1) * EPS * scale
    res = dict(out=out.reshape(n, -1), E_out=E_out.reshape(n, -1), M=m, E_M=E_M, Z=z, E_Z=E_Z, alpha=alpha,
               E_alpha=E_alpha, s=s, E_s=E_s, band=band, H=H, C=C)
    if G is None:
        return res

    Gd = np.asarray(G, dtype=np.float64).reshape(n, H, C)
    E_Gd = np.zeros_like(Gd) if E_G is None else np.asarray(E_G, dtype=np.float64).reshape(Gd.shape)
    D = (Gd * out).sum(axis=2)
    E_D = (np.abs(Gd) * E_out + E_Gd * np.abs(out)).sum(axis=2) + C * EPS * np.abs(Gd * out).sum(axis=2)
    if mistake == "no_D":
        D = np.zeros_like(D)
    Gi, E_Gi = Gd[rows], E_Gd[rows]
    da = (Gi * X[ix]).sum(axis=2)
    E_da = (E_Gi * np.abs(X[ix]) + np.abs(Gi) * E_x[ix]).sum(axis=2) + C * EPS * np.abs(Gi * X[ix]).sum(axis=2)
    u = da - D[rows]
    E_u = E_da + E_D[rows] + EPS * np.abs(u)
    t = alpha * u
    E_t = E_alpha * np.abs(u) + alpha * E_u + EPS * np.abs(t)
    deriv = np.where(s > 0, 1.0, 1.0 if mistake == "derivative_one" else slope)
    ds = t * deriv
    E_ds = E_t * deriv + EPS * np.abs(ds)
    lt = _seg(np.ones((ix.size, 1)), ix, n)                            # the transpose's row lengths
    da_dst = _seg(ds, rows, n)
    E_da_dst = _seg(E_ds, rows, n) + ln * EPS * _seg(np.abs(ds), rows, n)
    da_src = _seg(ds, ix, n)
    E_da_src = _seg(E_ds, ix, n) + lt * EPS * _seg(np.abs(ds), ix, n)
    back = alpha[:, :, None] * Gi
    dHf = _seg(back, ix, n)
    E_dHf = _seg(E_alpha[:, :, None] * np.abs(Gi) + alpha[:, :, None] * E_Gi, ix, n) + \
        lt[:, :, None] * EPS * _seg(np.abs(back), ix, n)
    res.update(ds=ds, E_ds=E_ds, da_dst=da_dst, E_da_dst=E_da_dst, da_src=da_src, E_da_src=E_da_src,
               dHf=dHf.reshape(n, -1), E_dHf=E_dHf.reshape(n, -1), D=D)
    return res


def worst_ratio(got, want, bound):
    """max |got - want| / bound (0 / 0 counts as 0, x / 0 as inf)."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err = np.abs(got - want)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


FORWARD, BACKWARD = ("out", "M", "Z"), ("dHf", "da_src", "da_dst")


def ratios(ref, got):
    """{name: worst |got - exact| / bound} for the results in `got` (a dict of arrays)."""
    return {k: worst_ratio(v, ref[k], ref["E_" + k]) for k, v in got.items()}


def check(what, ref, got):
    """Asserts every result of `got` within its bound; prints and returns the ratios."""
    r = ratios(ref, got)
    print(f"gat |got - exact| / bound  {what}: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()))
    for k, v in r.items():
        assert np.isfinite(np.asarray(got[k], dtype=np.float64)).all(), f"{what}: non-finite {k}"
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of the bound"
    return r


# ---- the two pinned cases, bit for bit in fp32 ------------------------------------------------------
def single_entry_ref(ix, Hf):
    """One entry per row: p = expf(0) = 1, z = 1, out[i] = fmaf(1, Hf[ix[i]], +0) / 1 = Hf[ix[i]] (a -0 of Hf
    becomes +0: 1 * -0 + +0 = +0)."""
    return np.asarray(Hf, dtype=np.float32)[np.asarray(ix, dtype=np.int64)] + np.float32(0.0)


def zero_att_ref(ip, ix, Hf):
    """att_src = att_dst = 0: every p is exactly 1 and z = len exactly, so out[i] is the sequential fp32 sum
    of the row's source rows in stored order from +0 (fmaf(1, x, acc) = acc + x), divided by len; an empty
    row is +0."""
    Hf = np.asarray(Hf, dtype=np.float32)
    n = ip.size - 1
    out = np.zeros((n, Hf.shape[1]), dtype=np.float32)
    for i in range(n):
        acc = np.zeros(Hf.shape[1], dtype=np.float32)
        for e in range(ip[i], ip[i + 1]):
            acc = acc + Hf[ix[e]]
        if ip[i + 1] > ip[i]:
            out[i] = acc / np.float32(ip[i + 1] - ip[i])
    return out


# ---- the torch composition the fused layer replaces -------------------------------------------------
def compose(ip, ix, Hf, a_src, a_dst, slope=0.2):
    """The aggregation from torch primitives (index_select, scatter_reduce amax, index_add), differentiable
    by autograd, in the dtype and on the device of its inputs.  ip, ix: int64 tensors.  Materialises the
    [nnz, H] scores and the [nnz, H, C] messages."""
    n, H = a_src.shape
    C = Hf.shape[1] // H
    rows = torch.repeat_interleave(torch.arange(n, device=ip.device), ip[1:] - ip[:-1])
    s = a_src.index_select(0, ix) + a_dst.index_select(0, rows)
    l = torch.nn.functional.leaky_relu(s, slope)
    m = torch.full((n, H), -torch.inf, dtype=l.dtype, device=l.device)
    m = m.scatter_reduce(0, rows[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(l - m.index_select(0, rows))
    z = torch.zeros((n, H), dtype=p.dtype, device=p.device).index_add(0, rows, p)
    alpha = p / z.index_select(0, rows)
    msg = alpha[:, :, None] * Hf.view(n, H, C).index_select(0, ix)
    out = torch.zeros((n, H, C), dtype=msg.dtype, device=msg.device).index_add(0, rows, msg)
    return out.reshape(n, H * C)


# ---- the layer and the two-layer model: bounds composed from evaluate's -----------------------------
MODEL_N, MODEL_SEED = 64, 103


def model_edges(n=MODEL_N, seed=6):
    """(dst, src) of the two-layer model's graph: 64 nodes, 160 random pairs and their reverses (duplicates and
    self-loops among them; GATGraph's self-loop handling sorts them out).  Small on purpose: the composed
    bound sums worst cases over the n rows of every dense backward step, so it loosens linearly with n (the
    kernels' long rows and row counts are the aggregation tests' business).  MODEL_SEED draws parameters with
    no ReLU input and no score in its kink band (margins of 336 and 135 bounds against the band's 4)."""
    rng = np.random.default_rng(seed)
    dst, src = rng.integers(0, n, 160), rng.integers(0, n, 160)
    return np.r_[dst, src], np.r_[src, dst]


def composed_conv(dtype):
    """GATConv with gat_attend replaced by the torch composition in `dtype` on the layer's own fp32 Hf, a_src
    and a_dst, its result cast back to fp32; lin, the scores and the bias stay the layer's fp32 torch code."""
    from srgnn import gat as GT

    class ComposedConv(GT.GATConv):
        def _aggregate(self, graph, Hf, a_src, a_dst):
            out = compose(graph.indptr, graph.indices.long(), Hf.to(dtype), a_src.to(dtype), a_dst.to(dtype),
                          self.negative_slope)
            return out.float()

    return ComposedConv


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _dense_backward(r, n, Hf, E_Hf, att_s, att_d, xin, E_xin, W, E_G):
    """Bounds on the difference of the two sides' parameter gradients of one GATConv, and (dx, E_dx) for the
    layer below.  r: evaluate's result with G and its E_G.  Both sides run the same fp32 dense code on inputs
    that differ by the bounds given, so each dense step adds the inputs' bounds times the other factor and
    its own k-term rounding once on either side (2 k eps sum |terms|); the composition's fp64 gradients are
    cast to fp32 (1 eps).  dHf in total: the aggregation's part plus da_src x att_src + da_dst x att_dst, a
    product each and two adds on either side (6 eps)."""
    H, C = att_s.shape
    absH, EH = np.abs(_f64(Hf)).reshape(n, H, C), _f64(E_Hf).reshape(n, H, C)
    att_s, att_d, W, xin, E_xin = _f64(att_s), _f64(att_d), _f64(W), _f64(xin), _f64(E_xin)
    e_s = r["E_da_src"] + EPS * np.abs(r["da_src"])
    e_d = r["E_da_dst"] + EPS * np.abs(r["da_dst"])
    out = {}
    for name, e_a, da in (("att_src", e_s, r["da_src"]), ("att_dst", e_d, r["da_dst"])):
        out[name] = (np.einsum("nh,nhc->hc", e_a, absH) + np.einsum("nh,nhc->hc", np.abs(da), EH) +
                     2 * n * EPS * np.einsum("nh,nhc->hc", np.abs(da), absH))[None]
    dH = r["dHf"].reshape(n, H, C)
    total = dH + r["da_src"][:, :, None] * att_s + r["da_dst"][:, :, None] * att_d
    parts = np.abs(dH) + np.abs(r["da_src"])[:, :, None] * np.abs(att_s) + np.abs(r["da_dst"])[:, :, None] * np.abs(att_d)
    e_H = r["E_dHf"].reshape(n, H, C) + EPS * np.abs(dH) + e_s[:, :, None] * np.abs(att_s) + \
        e_d[:, :, None] * np.abs(att_d) + 6 * EPS * parts
    e_H, parts, total = e_H.reshape(n, H * C), parts.reshape(n, H * C), total.reshape(n, H * C)
    out["lin.weight"] = e_H.T @ np.abs(xin) + parts.T @ E_xin + 2 * n * EPS * (parts.T @ np.abs(xin))
    G = _f64(r["G"])
    out["bias"] = _f64(E_G).sum(axis=0) + 2 * n * EPS * np.abs(G).sum(axis=0)
    dx = total @ W
    E_dx = e_H @ np.abs(W) + 2 * W.shape[0] * EPS * (parts @ np.abs(W))
    return out, dx, E_dx


def two_layer_bound(ip, ix, x, L1, L2, Cot, slope=0.2):
    """Bounds on |fused - composed| for the two-layer GAT (concatenated heads, ReLU, no dropout, log_softmax)
    under the loss sum(logits * Cot): {"logits": [n, K], "grads": {"convs.i.<name>": bound}, "bands": counts}.
    L1, L2: dicts of the fused model's own fp32 arrays per layer: W [H*C, in], att_s, att_d [H, C], b [H*C],
    Hf [n, H*C], a_s, a_d [n, H].  Both models share every dense fp32 step, so:
      layer 1 forward   Hf, a_src, a_dst are bit-identical; y1 differs by E_out + the cast + the two bias adds
      ReLU              |d relu| <= 1; its derivative jumps at 0: entries with |y1| <= 4 E_y1 are counted
      layer 2 forward   Hf2 = h W2^T: E_h |W2|^T + 2 k eps |h| |W2|^T; the scores likewise over C terms;
                        evaluate with E_x, E_asrc, E_adst; the bias adds
      log_softmax       d lsm_k = d z_k - sum_j sm_j d z_j, and on either side its own rounding
                        R = eps (|z - m| + max |z - m| + 2 + K + 2 |log S| + |lsm|)
                        (the subtraction, expf through its argument and itself, the K-term sum, log, the last
                        subtraction)
      its backward      dz = Cot - exp(lsm) sum_k Cot_k: exp(lsm) differs by sm (E_lsm + 4 eps), the sum is K terms
      layer 2 backward  evaluate with E_G = E_dz as well; _dense_backward
      ReLU backward     the mask is the same on both sides outside the band
      layer 1 backward  evaluate with E_G only; _dense_backward."""
    n = x.shape[0]
    x = _f64(x)
    b1, b2 = _f64(L1["b"]), _f64(L2["b"])
    r1 = evaluate(ip, ix, L1["Hf"], L1["a_s"], L1["a_d"], slope)
    y1 = r1["out"] + b1
    E_y1 = r1["E_out"] + EPS * np.abs(r1["out"]) + 2 * EPS * (np.abs(r1["out"]) + np.abs(b1))
    relu_band = int((np.abs(y1) <= 4 * E_y1).sum())
    h, E_h = np.maximum(y1, 0.0), E_y1
    W2 = _f64(L2["W"])
    E_Hf2 = E_h @ np.abs(W2).T + 2 * W2.shape[1] * EPS * (np.abs(h) @ np.abs(W2).T)
    H2, C2 = L2["att_s"].shape
    Hv, Ev = np.abs(_f64(L2["Hf"])).reshape(n, H2, C2), E_Hf2.reshape(n, H2, C2)
    E_a = [np.einsum("nhc,hc->nh", Ev, np.abs(_f64(a))) + 2 * C2 * EPS * np.einsum("nhc,hc->nh", Hv, np.abs(_f64(a)))
           for a in (L2["att_s"], L2["att_d"])]
    fwd = evaluate(ip, ix, L2["Hf"], L2["a_s"], L2["a_d"], slope, E_x=E_Hf2, E_asrc=E_a[0], E_adst=E_a[1])
    z = fwd["out"] + b2
    E_z = fwd["E_out"] + EPS * np.abs(fwd["out"]) + 2 * EPS * (np.abs(fwd["out"]) + np.abs(b2))
    K = z.shape[1]
    m = z.max(axis=1, keepdims=True)
    logS = np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    lsm = z - m - logS
    sm = np.exp(lsm)
    R_l = EPS * (np.abs(z - m) + np.abs(z - m).max(axis=1, keepdims=True) + 2 + K + 2 * np.abs(logS) + np.abs(lsm))
    E_lsm = E_z + (sm * E_z).sum(axis=1, keepdims=True) + 2 * R_l

    Cot = _f64(Cot)
    Cs, Ca = Cot.sum(axis=1, keepdims=True), np.abs(Cot).sum(axis=1, keepdims=True)
    E_sm = sm * (E_lsm + 4 * EPS)
    T = sm * Cs
    E_T = np.abs(Cs) * E_sm + sm * 2 * K * EPS * Ca + 2 * EPS * np.abs(T)
    dz = Cot - T
    E_dz = E_T + 2 * EPS * np.abs(dz)
    r2 = evaluate(ip, ix, L2["Hf"], L2["a_s"], L2["a_d"], slope, G=dz, E_x=E_Hf2, E_asrc=E_a[0], E_adst=E_a[1],
                  E_G=E_dz)
    r2["G"] = dz
    g2, dh, E_dh = _dense_backward(r2, n, L2["Hf"], E_Hf2, L2["att_s"], L2["att_d"], h, E_h, W2, E_dz)
    mask = y1 > 0
    dy1, E_dy1 = dh * mask, E_dh * mask
    r1b = evaluate(ip, ix, L1["Hf"], L1["a_s"], L1["a_d"], slope, G=dy1, E_G=E_dy1)
    r1b["G"] = dy1
    g1, _, _ = _dense_backward(r1b, n, L1["Hf"], np.zeros_like(_f64(L1["Hf"])), L1["att_s"], L1["att_d"], x,
                               np.zeros_like(x), _f64(L1["W"]), E_dy1)
    grads = {f"convs.0.{k}": v for k, v in g1.items()}
    grads.update({f"convs.1.{k}": v for k, v in g2.items()})
    with np.errstate(divide="ignore"):
        margins = dict(relu=float((np.abs(y1) / E_y1).min()), scores1=float((np.abs(r1b["s"]) / r1b["E_s"]).min()),
                       scores2=float((np.abs(r2["s"]) / r2["E_s"]).min()))
    return dict(logits=E_lsm, lsm=lsm, grads=grads, margins=margins,
                bands=dict(relu=relu_band, scores1=r1b["band"], scores2=r2["band"]))


def model_layers(model, x, aggregate):
    """The fused model's own fp32 arrays per layer, as two_layer_bound takes them: aggregate(conv, Hf, a_s, a_d)
    is the aggregation that model runs."""
    layers = []
    with torch.no_grad():
        hcur = x
        for i, conv in enumerate(model.convs):
            H, C = conv.heads, conv.out_channels
            Hf = conv.lin(hcur)
            Hv = Hf.view(-1, H, C)
            a_s = torch.einsum("nhc,hc->nh", Hv, conv.att_src[0])
            a_d = torch.einsum("nhc,hc->nh", Hv, conv.att_dst[0])
            layers.append({k: v.detach().cpu().numpy() for k, v in dict(
                W=conv.lin.weight, att_s=conv.att_src[0], att_d=conv.att_dst[0], b=conv.bias, Hf=Hf, a_s=a_s,
                a_d=a_d).items()})
            if i + 1 < len(model.convs):
                hcur = torch.relu(aggregate(conv, Hf, a_s, a_d) + conv.bias)
    return layers


def check_model(what, bound, y, y2, named, named2):
    """Asserts the logits and every parameter gradient of the two models within two_layer_bound's result;
    prints the ratios."""
    assert bound["bands"] == dict(relu=0, scores1=0, scores2=0), bound["bands"]
    print(f"gat model kink margins |value| / bound (the band is <= 4)  {what}: {bound['margins']}")
    r = {"logits": worst_ratio(y.detach().cpu().numpy(), y2.detach().cpu().numpy().astype(np.float64), bound["logits"])}
    for (k, p), (k2, q) in zip(named, named2):
        assert k == k2 and p.grad is not None and q.grad is not None, k
        r[k] = worst_ratio(p.grad.cpu().numpy(), q.grad.cpu().numpy().astype(np.float64), bound["grads"][k])
    print(f"gat model |fused - composed| / bound  {what}: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert len(r) == 9
    for k, v in r.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of the composed bound"
    return r
