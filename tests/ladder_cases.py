"""The ladder operator: one small CSR whose rows hold every length the hand-scheduled SpMM kernels
treat differently, with data on which the order of a row's fma chain shows in the result bits.

  rows     n = 4096, positions shuffled with a fixed seed:
             ladder  one row of every length 0 .. 1064 (every `nb` of a first, second and third
                     512-entry hub window; every id-chunk, unroll and slice-wave residue);
             edge    for W in {256, 512}, k in {3, 4, 5, 6}, t in {-9, -8, -7, -1, 0, 1, 7, 8, 9} one row
                     of k W + t entries (the parity of n_win, full last windows, the DPP-to-partial
                     switch); the longest has 3,081;
             filler  the rest, lengths cycling 0 .. 64 (the planner's 32- / 48-entry whole-row limits).
           Column ids are sorted and unique within a row (the column-block paths take the operator).
  values   "bounded walk": magnitudes U[0.5, 1.5), each entry's sign chosen so that the row's running
           sum stays near zero (negative when the running sum is positive, else positive; the running
           sum is tracked with the panel's nominal factor 1.0625).
  panels   X[c, j] = w_j (1 + eps_cj), w_j = U[1, 2), eps_cj = U[0, 1/8): every column's partial sums
           stay O(1) (max |Y| ~ 12), so a rounding difference made early in a row survives to its
           end, and the noise in eps keeps a gather from the wrong row visible.
The fp64 variant is the same construction in float64 with the walk kept near 3 instead of 0 (WALK_CENTRE
below says why); the fp32 arrays are float64 draws rounded once.

Also here: the special-value panels derived from that data (NaN, Inf, overflow, subnormals, a start
panel of special words) with their NaN-aware comparison, the link-swap mutations the CPU tests hold
the data to, the schedules the GPU tests run, and plain numpy references of the kernels' epilogues
(one rounded operation at a time, in the working precision; the modes and operation order are those
of cheby_epi_at's comment in csrc/srg_cheby.hip).  Test infrastructure only.
"""
from __future__ import annotations

import functools

import numpy as np

N = 4096
LADDER_MAX = 1064
EDGE_W = (256, 512)
EDGE_K = (3, 4, 5, 6)
EDGE_T = (-9, -8, -7, -1, 0, 1, 7, 8, 9)
FILLER_CYCLE = 65            # filler lengths 0 .. 64
NOMINAL = 1.0625             # E[X[c, j] / w_j]: the factor the bounded walk tracks its sum with
SEED = 1064
# where the bounded walk keeps a row's running sum: an entry is negative when the running sum exceeds
# the centre.  fp32: 0, as designed.  fp64: 3 -- around 0 the fp64 chain (separately rounded product
# and sum, no fma) adds entries of opposite sign and like magnitude, and such sums are exact, so a
# swapped pair changed only 58 % (links 1, 2) to 92 % (last two) of the rows; centres 0 / 1 / 2 / 3 / 4 / 6
# give at worst 58 / 88 / 95 / 96.5 / 93 / 86 % over the five mutations (d = 32), so 3 it is (max |Y| 18)
WALK_CENTRE = {"float32": 0.0, "float64": 3.0}
D_MAX = 288                  # the widest panel any test asks for

# the Chebyshev modes (include/srgnn_hip.h)
INIT, STEP, INIT_T, STEP_FIRST, NO_T = 0, 1, 2, 3, 0x10


def edge_lengths():
    return [k * w + t for w in EDGE_W for k in EDGE_K for t in EDGE_T]


@functools.lru_cache(maxsize=None)
def lengths() -> np.ndarray:
    """Row lengths, int64 [N], in row order (shuffled)."""
    fixed = list(range(LADDER_MAX + 1)) + edge_lengths()
    filler = [i % FILLER_CYCLE for i in range(N - len(fixed))]
    lens = np.array(fixed + filler, dtype=np.int64)
    np.random.default_rng(SEED).shuffle(lens)
    lens.setflags(write=False)
    return lens


@functools.lru_cache(maxsize=None)
def structure():
    """(indptr int64 [N + 1], indices int32 [nnz]): sorted unique ids per row."""
    lens = lengths()
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    rng = np.random.default_rng(SEED + 1)
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for r in range(N):
        if lens[r]:
            indices[indptr[r]:indptr[r + 1]] = np.sort(rng.choice(N, int(lens[r]), replace=False))
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return indptr, indices


@functools.lru_cache(maxsize=None)
def _walk(centre: float) -> np.ndarray:
    lens = lengths()
    indptr, _ = structure()
    mag = np.random.default_rng(SEED + 2).uniform(0.5, 1.5, int(indptr[-1]))
    vals = np.empty_like(mag)
    run = np.zeros(N)                       # the rows' running sums, link k of every row at once
    for k in range(int(lens.max())):
        rows = np.flatnonzero(lens > k)
        p = indptr[rows] + k
        v = np.where(run[rows] > centre, -mag[p], mag[p])
        vals[p] = v
        run[rows] += v * NOMINAL
    vals.setflags(write=False)
    return vals


def np_dtype(dtype):
    return np.dtype(dtype).type


@functools.lru_cache(maxsize=None)
def operator(dtype="float32"):
    """(indptr, indices, values) of the ladder operator, values in `dtype`."""
    indptr, indices = structure()
    v = _walk(WALK_CENTRE[np.dtype(dtype).name]).astype(np_dtype(dtype))
    v.setflags(write=False)
    return indptr, indices, v


@functools.lru_cache(maxsize=None)
def _x64() -> np.ndarray:
    rng = np.random.default_rng(SEED + 3)
    w = rng.uniform(1.0, 2.0, D_MAX)
    eps = rng.uniform(0.0, 0.125, (N, D_MAX))
    return w[None, :] * (1.0 + eps)


def x_panel(dtype, d) -> np.ndarray:
    """The gathered panel [N, d] (contiguous): the first d columns of one master panel."""
    return np.ascontiguousarray(_x64()[:, :d]).astype(np_dtype(dtype))


def side_panel(dtype, d, tag: int, rows=N) -> np.ndarray:
    """An O(1) signed panel [rows, d] for the operands beside the chain (Y to accumulate into, the
    aggregation panel, T_{k-1}, the scales' outputs): uniform in [-2, 2), seeded by (tag, d)."""
    return np.random.default_rng([SEED, 77, tag, d]).uniform(-2.0, 2.0, (rows, d)).astype(np_dtype(dtype))


# ------------------------------------------------------------------------------------------------
# special-value panels: what the finite O(1) data cannot show -- a lane without an entry folded into
# the chain as 0 * X[0], a flushed subnormal, a chain that does not start from Y's own bits
# ------------------------------------------------------------------------------------------------
KINDS = ("poison", "inf", "overflow", "sub_deep", "sub_edge", "sub_x")
QNAN = {"float32": 0x7FC00000, "float64": 0x7FF8000000000000}
POISON_ROWS = (0, N - 1)     # row 0 is the id a lane without an entry gathers with
# (log2 of the values' factor, log2 of X's): products and sums deep in the subnormal range; results on
# both sides of FLT_MIN; a subnormal X under normal values
SUB_SCALES = {"sub_deep": (-100, -40), "sub_edge": (-90, -37), "sub_x": (12, -140)}
Y0_WORDS = (0x80000000, 0x00000000, 0x7FC01234, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF)


def uint_of(dtype):
    return np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64


def special(kind, dtype, d):
    """(values, X) of one special-value case: the ladder operator's values and the gathered panel
    [N, d], both in `dtype`.  The scaled kinds scale the float64 masters and round once."""
    T = np_dtype(dtype)
    centre = WALK_CENTRE[np.dtype(dtype).name]
    if kind in SUB_SCALES:
        sv, sx = SUB_SCALES[kind]
        return (_walk(centre) * 2.0 ** sv).astype(T), np.ascontiguousarray(_x64()[:, :d] * 2.0 ** sx).astype(T)
    v = operator(dtype)[2]
    X = x_panel(dtype, d)
    if kind == "poison":
        X.view(uint_of(dtype))[list(POISON_ROWS)] = QNAN[np.dtype(dtype).name]
    elif kind == "inf":
        k = (31 * np.arange(N)[:, None] + 7 * np.arange(d)[None, :]) % 257
        X[k == 0] = np.inf
        X[k == 1] = -np.inf
    elif kind == "overflow":
        X *= T(2.0 ** 126)       # exact: X stays finite, the partial sums do not
    else:
        raise KeyError(kind)
    return v, X


def y0_special(d) -> np.ndarray:
    """A [N, d] fp32 panel to accumulate into: element (r, c) is word (r + c) mod 8 of Y0_WORDS (-0, +0,
    two quiet NaNs with payloads, +inf, -inf, the smallest and the largest negative subnormal)."""
    words = np.array(Y0_WORDS, dtype=np.uint32)
    return words[(np.arange(N)[:, None] + np.arange(d)[None, :]) % words.size].view(np.float32).copy()


def poison_free_rows() -> np.ndarray:
    """bool [N]: the rows that reference neither poisoned column."""
    _, indices = structure()
    hit = np.zeros(N, dtype=bool)
    hit[np.repeat(np.arange(N), lengths())[np.isin(indices, POISON_ROWS)]] = True
    return ~hit


def special_diff(got, want, lens, sentinel, exact=None):
    """The comparison for [N, ld] buffers that may hold NaN: None when they agree, else a message as
    first_diff's.  Where the expected word is no NaN the bits must be equal; where it is a NaN the
    result must be a NaN other than `sentinel` (payloads are not pinned: an invalid operation gives
    0xFFC00000 on x86 and 0x7FC00000 on the GPU).  An expected sentinel (guard columns, rows a launch
    does not schedule) must come back bit for bit, and so must every row of the bool [N] mask `exact`
    (values a kernel only moves)."""
    u = uint_of(got.dtype)
    g, w = got.view(u), want.view(u)
    free = np.isnan(want) & (w != u(sentinel))
    if exact is not None:
        free &= ~np.asarray(exact, dtype=bool)[:, None]
    wrong = np.where(free, ~np.isnan(got) | (g == u(sentinel)), g != w)
    bad = np.argwhere(wrong)
    if not bad.size:
        return None
    r, c = (int(v) for v in bad[0])
    rl = np.asarray(lens)[np.unique(bad[:, 0])]
    return (f"{bad.shape[0]} elements of {rl.size} rows differ; first at row {r} (length {int(lens[r])}), "
            f"buffer column {c}: got {got[r, c]!r} ({int(g[r, c]):#x}), want {want[r, c]!r} ({int(w[r, c]):#x}); "
            f"lengths of the differing rows: {sorted(set(int(x) for x in rl))[:40]}")


# ------------------------------------------------------------------------------------------------
# link swaps: what a transposed pair in a tile swizzle, a quad broadcast or a ring of register sets does
# ------------------------------------------------------------------------------------------------
def swap_links(indptr, indices, values, first):
    """Swaps links first[r] and first[r] + 1 of every row r with first[r] >= 0 (and at least
    first[r] + 2 entries).  Returns (indices, values, rows): copies with the pairs swapped and the ids
    of the rows that were changed."""
    lens = np.diff(indptr)
    first = np.broadcast_to(np.asarray(first, dtype=np.int64), lens.shape)
    rows = np.flatnonzero((first >= 0) & (lens >= first + 2))
    p = indptr[rows] + first[rows]
    ix, v = indices.copy(), values.copy()
    ix[p], ix[p + 1] = indices[p + 1], indices[p]
    v[p], v[p + 1] = values[p + 1], values[p]
    return ix, v, rows


def mutations(lens, commuting_head: bool):
    """name -> first link of the swapped pair per row (-1: the mutation does not apply to the row).
    The cases: links (0, 1), the two middle links, the last two, and (W - 1, W) for W = 256 and 512.

    commuting_head (the fp64 chain: acc = acc + a x from +0, product and sum rounded separately): the
    chain's first sum 0 + p0 is exact and p0 + p1 == p1 + p0, so swapping links 0 and 1 is the same
    chain, bit for bit -- not an error a kernel can make.  There the first-links case swaps (1, 2), the
    first pair whose order the chain can show, and a middle / last pair that is (0, 1) does not apply.
    (The fp32 chain is fma(a1, x1, round(a0 x0)): its first two links do not commute.)"""
    lens = np.asarray(lens, dtype=np.int64)
    lo = 1 if commuting_head else 0
    no = np.full(lens.shape, -1, dtype=np.int64)
    out = {}
    out["first"] = np.where(lens >= lo + 2, lo, no)
    mid = lens // 2 - 1
    out["middle"] = np.where((lens >= 2) & (mid >= lo), mid, no)
    out["last"] = np.where((lens >= 2) & (lens - 2 >= lo), lens - 2, no)
    for w in EDGE_W:
        out[f"window{w}"] = np.where(lens >= w + 1, w - 1, no)
    return out


# ------------------------------------------------------------------------------------------------
# schedules: (order int32, n_hub, n_heavy) -- the first n_hub rows of order are hub rows, the next
# n_heavy slice-wave rows, the rest light rows
# ------------------------------------------------------------------------------------------------
def sched_desc(lens, heavy_threshold, hub_threshold):
    """The project's own schedule (srgnn.csr.schedule_from_degrees): decreasing length, hub rows
    longer than hub_threshold, slice-wave rows longer than heavy_threshold (negative: none)."""
    lens = np.asarray(lens)
    order = np.argsort(-lens, kind="stable").astype(np.int32)
    n_hub = int((lens > hub_threshold).sum()) if hub_threshold >= 0 else 0
    n_big = int((lens > heavy_threshold).sum()) if heavy_threshold >= 0 else 0
    return order, n_hub, max(0, n_big - n_hub)


def sched_asc(lens, n_hub, n_heavy, empty_first=False):
    """Increasing length: the shortest non-empty rows are the hub rows, the next shortest the
    slice-wave rows, the longest rows light; the empty rows go last (empty_first: first, so that the
    hub prefix starts with them)."""
    lens = np.asarray(lens)
    asc = np.argsort(lens, kind="stable")
    empty, full = asc[lens[asc] == 0], asc[lens[asc] > 0]
    order = np.concatenate([empty, full] if empty_first else [full, empty]).astype(np.int32)
    return order, n_hub, n_heavy


def sched_rand(lens, seed, n_hub, n_heavy, leave_out=0, empty_hubs=False):
    """A seeded random permutation of the rows, without its last `leave_out` rows (which the launch
    then does not schedule).  Unless empty_hubs, an empty row drawn into the hub prefix changes places
    with the first non-empty row after the prefix."""
    lens = np.asarray(lens)
    order = np.random.default_rng([SEED, 5, seed]).permutation(lens.size)
    if not empty_hubs:
        later = [i for i in range(n_hub, order.size) if lens[order[i]] > 0]
        for i in range(n_hub):
            if lens[order[i]] == 0:
                j = later.pop(0)
                order[i], order[j] = order[j], order[i]
    order = order[: order.size - leave_out].astype(np.int32)
    return order, n_hub, n_heavy


def w512_sweep(lens, n_slices, seed=0):
    """The launches of a sweep that runs every non-empty row as a hub row with 512-entry windows: a
    launch takes 512-entry windows only with at most 256 hub workgroups, so each launch makes another
    group of at most 256 // n_slices non-empty rows its hub prefix and the other rows light rows."""
    lens = np.asarray(lens)
    rows = np.random.default_rng([SEED, 6, seed]).permutation(lens.size)
    full, empty = rows[lens[rows] > 0], rows[lens[rows] == 0]
    g = 256 // n_slices
    out = []
    for i in range(0, full.size, g):
        hub = full[i:i + g]
        order = np.concatenate([hub, full[:i], full[i + g:], empty]).astype(np.int32)
        out.append((order, int(hub.size), 0))
    return out


# ------------------------------------------------------------------------------------------------
# numpy references of the epilogues (one rounded operation at a time in the arrays' precision)
# ------------------------------------------------------------------------------------------------
def agg_ref(prev, w, y, init=False):
    """agg = (0 if init else prev) + w * y, product and sum rounded separately."""
    T = y.dtype.type
    p = T(w) * y
    return (np.zeros_like(y) if init else prev) + p


def cheby_ref(mode, acc, Tc, To, R, a1, a2, coef_prev, coef):
    """The fused step's epilogue on acc = A Tc (all [rows, d], R [n_scales, rows, d]): returns
    (Tn or None with NO_T, R after the step or the R given for INIT_T).
      INIT:       Tn = (acc - a2 Tc) / a1;  R_s = (c0_s / 2) Tc + c1_s Tn       coef_prev = c0, coef = c1
      INIT_T:     Tn = (acc - a2 Tc) / a1
      STEP_FIRST: Tn = acc - To;  R_s = ((c0_s / 2) To + c1_s Tc) + c2_s Tn     coef_prev = c0 then c1, coef = c2
      STEP:       Tn = acc - To;  R_s = R_s + ck_s Tn                           coef = ck"""
    T = acc.dtype.type
    m = mode & 0xF
    ns = R.shape[0]
    R = R.copy()
    if m in (INIT, INIT_T):
        tn = (acc - T(a2) * Tc) / T(a1)
        if m == INIT:
            for s in range(ns):
                R[s] = (T(0.5) * T(coef_prev[s])) * Tc + T(coef[s]) * tn
    elif m == STEP_FIRST:
        tn = acc - To
        for s in range(ns):
            R[s] = ((T(0.5) * T(coef_prev[s])) * To + T(coef_prev[ns + s]) * Tc) + T(coef[s]) * tn
    elif m == STEP:
        tn = acc - To
        for s in range(ns):
            R[s] = R[s] + T(coef[s]) * tn
    else:
        raise ValueError(mode)
    return (None if mode & NO_T else tn), R


def cheby_filter_ref(spmm, L, coeffs, S, lmax, lean):
    """A whole filter bank from `spmm(indptr, indices, values, X)` and cheby_ref: R [n_scales, n, d].
    L = (indptr, indices, values) with every diagonal entry stored; coeffs [n_scales, order + 1].
    lean: INIT_T, STEP_FIRST, STEP ..., STEP | NO_T instead of INIT, STEP, ..."""
    ip, ix, lv = L
    T = S.dtype.type
    coeffs = np.atleast_2d(coeffs)
    ns, nc = coeffs.shape
    n = ip.size - 1
    a1 = a2 = T(lmax) / T(2)
    rows = np.repeat(np.arange(n), np.diff(ip))
    fv = (T(2) / a1) * np.where(rows == ix, lv - a2, lv)     # F = (2 / a1) (L - a2 I)
    R = np.zeros((ns,) + S.shape, dtype=S.dtype)
    lean = lean and nc > 2
    t_old = S
    t_cur, R = cheby_ref(INIT_T if lean else INIT, spmm(ip, ix, lv, S), S, None, R, a1, a2, coeffs[:, 0], coeffs[:, 1])
    for k in range(2, nc):
        mode = STEP_FIRST if (lean and k == 2) else STEP
        if lean and k == nc - 1:
            mode |= NO_T
        cp = np.concatenate([coeffs[:, 0], coeffs[:, 1]]) if (mode & 0xF) == STEP_FIRST else None
        t_new, R = cheby_ref(mode, spmm(ip, ix, fv, t_cur), t_cur, t_old, R, a1, a2, cp, coeffs[:, k])
        t_old, t_cur = t_cur, t_new
    return R


def first_diff(got, want, lens):
    """Where two [N, ld] buffers first differ, for a failure message: the row, its length, the column
    (of the buffer: the panel's window starts at its guard width) and the lengths of all differing rows."""
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    bad = np.argwhere(got.view(u) != want.view(u))
    if not bad.size:
        return "no difference"
    r, c = (int(v) for v in bad[0])
    rl = np.asarray(lens)[np.unique(bad[:, 0])]
    return (f"{bad.shape[0]} elements of {rl.size} rows differ; first at row {r} (length {int(lens[r])}), "
            f"buffer column {c}: got {got[r, c]!r}, want {want[r, c]!r}; lengths of the differing rows: "
            f"{sorted(set(int(x) for x in rl))[:40]}")
