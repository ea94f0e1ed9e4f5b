"""Shared inputs and expected values of the fused min / max / concat / NAFS tests (CPU and GPU files).

NAFS bound.  Per element, against the formula of over_smooth_distance_op.py evaluated in fp64 on the
same fp32 hops (T = K + 1 hops, eps = 2^-24, w_k the exact softmax weights):

    |got - exact| <= (4d + 2T + 32) * eps * sum_k w_k |X_k[i, c]|

Derivation (first order in eps; any summation order of the d terms).
  s_k = ((x0 . x_k) / (|x_k| + 1e-10)) / n0.  The d-term dot product is off by at most
  d eps sum_i |x0_i x_ki| <= d eps |x0||x_k| (Cauchy-Schwarz): d eps absolute in s_k.  Each norm is a
  d-term sum of squares (d eps relative) under a square root (halved, + 1 eps) plus one rounding for
  the + 1e-10: (d/2 + 2) eps relative, twice; the two divides round once each.  With |s_k| <= 1:
      |ds_k| <= (d + 2 (d/2 + 2) + 2) eps = (2d + 6) eps.
  w_k = e_k / sum_j e_j:  dw_k / w_k = ds_k - sum_j w_j ds_j, at most 2 max|ds| = (4d + 12) eps; a
  1-ulp expf is 2 eps relative in e_k and as much in the denominator: 4 eps; the T - 1 additions of
  the positive e_j into z: (T - 1) eps.  Weights: |dw_k| <= w_k (4d + T + 15) eps, which is below the
  (4d + 2T + 16) eps absolute bound of the weight check since w_k <= 1.
  acc: one rounding per product e_k x_k, T additions, one divide by z: (T + 2) eps on sum_k w_k |X_k|.
  Total (4d + 2T + 17) eps sum_k w_k |X_k| <= (4d + 2T + 32) eps sum_k w_k |X_k|.
The tests hold the larger, stated constant; the reference's torch CPU result meets it too
(tests/test_msgops_fused_cpu.py), with the worst element near 0.05 of it.
"""
import functools

import numpy as np

EPS = 2.0 ** -24
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 2.5, np.inf, -np.inf, np.nan], dtype=np.float32)
NAFS_D = (1, 3, 9, 63, 64, 65, 128, 130, 257, 1433)
NAFS_D_WIDE_VEC = (514, 1028)          # rows past the register cut at 8- and 16-byte accesses
NAFS_N, NAFS_T = 61, 5

_ratios = {}


def special_panels(n, d, T, seed):
    """T panels [n, d] drawn from {+-0, +-1, 2.5, +-inf, NaN}."""
    rng = np.random.default_rng(seed)
    return [SPECIALS[rng.integers(0, SPECIALS.size, size=(n, d))] for _ in range(T)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def select_rule(panels, mode):
    """SRG_ACC_COPY then SRG_ACC_MIN / SRG_ACC_MAX hop by hop, restated in numpy."""
    agg = panels[0].copy()
    with np.errstate(invalid="ignore"):
        for y in panels[1:]:
            keep = (y >= agg) if mode == "min" else (y <= agg)
            take = ~np.isnan(agg) & ~keep
            agg = np.where(take, y, agg)
    return agg


def torch_select(panels, mode):
    """The reference's combine: torch.stack(feat_list[start:end]).min / max(dim=0)[0] on the CPU."""
    import torch
    st = torch.stack([torch.from_numpy(np.ascontiguousarray(p)) for p in panels], dim=0)
    return (st.min(dim=0)[0] if mode == "min" else st.max(dim=0)[0]).numpy()


@functools.lru_cache(maxsize=None)
def nafs_hops(d, n=NAFS_N, T=NAFS_T):
    """T correlated random hops [n, d]; three all-zero rows in hop 0, two in hop 3."""
    rng = np.random.default_rng(1000 + d)
    hops = [rng.standard_normal((n, d)).astype(np.float32)]
    for _ in range(1, T):
        hops.append((0.6 * hops[-1] + 0.4 * rng.standard_normal((n, d))).astype(np.float32))
    hops[0][[3, 17, 60]] = 0.0
    hops[3][[5, 17]] = 0.0
    for h in hops:
        h.setflags(write=False)
    return tuple(hops)


def nafs_exact(hops):
    """(out fp64 [n, d], weights fp64 [n, T], scale = sum_k w_k |X_k| [n, d]) of the NAFS formula."""
    H = [np.asarray(h, dtype=np.float64) for h in hops]
    tiny = np.float64(np.float32(1e-10))
    n0 = np.sqrt((H[0] * H[0]).sum(1)) + tiny
    s = np.stack([((H[0] * h).sum(1) / (np.sqrt((h * h).sum(1)) + tiny)) / n0 for h in H], axis=1)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)
    out = sum(w[:, k:k + 1] * H[k] for k in range(len(H)))
    scale = sum(w[:, k:k + 1] * np.abs(H[k]) for k in range(len(H)))
    return out, w, scale


def nafs_bound(d, T, scale):
    return (4 * d + 2 * T + 32) * EPS * scale


def weight_bound(d, T):
    return (4 * d + 2 * T + 16) * EPS


def check_nafs(got, hops, what, against=None):
    """Asserts |got - (against or exact)| <= bound element-wise; prints and returns the worst ratio."""
    out, _, scale = nafs_exact(hops)
    d, T = out.shape[1], len(hops)
    bound = nafs_bound(d, T, scale)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == out.shape, f"{what}: shape {got.shape} != {out.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got - (out if against is None else np.asarray(against, dtype=np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    _ratios[what] = worst
    print(f"nafs |got - exact| / bound  {what}: {worst:.4f}   (running max {max(_ratios.values()):.4f})")
    assert worst <= 1.0, f"{what}: {worst:.3f} of the bound"
    return worst


# ------------------------------------------------------------------------------------------------
# long hop lists through the weighted sum (test_aggregate_cpu.py, test_msgops_fused_gpu.py): torch's
# multi_row_sum over the last n*d mod 32 elements takes its 16-row blocks from 64 terms on (16 per
# interleaved partial sum) and its second level from 1024; combine_steps folds level 1 into level 2
# from 256 terms on
# ------------------------------------------------------------------------------------------------
LONG_T = (64, 65, 255, 256, 257, 1024, 1027)
LONG_SHAPES = ((5, 7), (2, 33), (3, 3))       # n*d = 35, 66, 9: tails of 3, 2 and all 9 elements
LONG_ALPHA = 0.15                             # 0.15 * 0.85^k: an fp32 subnormal from term 526 on, zero from 629
                                              # (an order-only case: those terms are swamped by terms 0 .. 525)


def long_hops(n, d, T):
    """T panels [n, d] as one [T, n, d] fp32 array, standard normal, seeded by the case."""
    return np.random.default_rng([n, d, T]).standard_normal((T, n, d)).astype(np.float32)


def long_hops_subnormal(n, d, T):
    """long_hops scaled by 2^-135 (rounded once): every element, every product with a weight in [0.5, 1.5)
    and every partial sum of up to 1,027 of them is an fp32 subnormal, so the result's bits are the
    products' bits -- a step that flushes them returns zeros."""
    return (long_hops(n, d, T).astype(np.float64) * 2.0 ** -135).astype(np.float32)


def long_weights(T):
    """T hand-crafted fp32 weights in [0.5, 1.5)."""
    return np.random.default_rng([17, T]).uniform(0.5, 1.5, T).astype(np.float32)
