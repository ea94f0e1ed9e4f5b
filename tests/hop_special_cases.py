"""Inputs that put the hop attention (gate / ori_ref / jk), its recursive form (§5.4.3) and their
row-indexed entries (§5.4.4) where the O(1) draws of hop_attention_ref.random_case never go: saturated sigmoids,
NaN / Inf / subnormal / signed-zero panel cells, poisoned panels a kind must not read, a poisoned stand-in row for
out-of-range indices.  Builders only: numpy in, numpy out, shared by tests/test_hop_special_{cpu,gpu}.py.  The
expectation is always the fp64 restatement (hop_attention_ref / hop_recursive_ref) on the same fp32 values.

A case is a dict: kind ("gate" / "ori_ref" / "jk" / "recursive"), T, start, end, hops (T float32 [n, d] arrays),
w, b, C (a cotangent for the identity form) and what the builder planted.  `emulate` is a plain numpy-fp32
evaluation of the learnable kinds' formula whose keyword arguments put in the mistakes of the negative controls.
"""
import numpy as np

import hop_attention_ref as R
import hop_recursive_ref as RR

F32 = np.float32
KINDS = ("gate", "ori_ref", "jk", "recursive")
GAINS = (0.01, 1.0, 30.0, 300.0, 3000.0)
# |s| ranges of a = 1 / (1 + expf(-s)) in fp32 (expf(-88.72) = 2^-128, expf(-87.34) = 2^-126, expf(-103.97) = 2^-150,
# expf(88.72) = 2^128, and 1 + u rounds to 1 for u < 2^-25 = expf(-17.33)), each wanted with both signs of s
REGIMES = {"1 + expf(-s) rounds to 1": (17.4, 87.0), "expf(-s) is subnormal (s > 0)": (87.4, 88.7),
           "expf(-s) overflows (s < 0)": (88.8, 104.0), "expf(-s) is exactly 0 (s > 0)": (104.0, np.inf)}
TARGETS = (50.0, 88.0, 96.0, 150.0)            # one score of each sign is steered into each range
DENORMAL_ROW, NEG_ZERO_ROW, POS_ZERO_ROW = 11, 23, 37
DENORMAL_UNIT = 2.0 ** -135


def reads(kind, T, start, end):
    """The panels a kind reads: the slice; hop 0 besides for ori_ref; every panel for jk; [0, end) for recursive."""
    if kind == "jk":
        return list(range(T))
    if kind == "recursive":
        return list(range(end))
    return sorted(set(range(start, end)) | ({0} if kind == "ori_ref" else set()))


def slice_panels(kind, start, end):
    """The panels out is combined from."""
    return list(range(0 if kind == "recursive" else start, end))


def base(kind, n, d, T, start, end, seed):
    """The O(1) case of the restatements' random_case as a dict (recursive: start = 0)."""
    if kind == "recursive":
        hops, w, b, C = RR.random_case(n, d, T, seed)
        start = 0
    else:
        hops, w, b, C = R.random_case(kind, n, d, T, start, end, seed)
    return dict(kind=kind, T=T, start=start, end=end, n=n, d=d, hops=hops, w=w, b=b, C=C)


def cotangent(B, d, seed):
    return np.random.default_rng(seed).standard_normal((B, d)).astype(F32)


def batch_index(n_src, seed, extra=30):
    """Every panel row once plus `extra` duplicates, shuffled: whatever a builder planted is in the batch."""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.concatenate([np.arange(n_src), rng.integers(0, n_src, extra)])).astype(np.int64)


def gather(hops, idx, select=True):
    """The batch rows hop[idx] of every panel; an index outside [0, n_src) reads as a row of +0.0 (§5.4.4).
    select=False makes those zeros the wrong way: row 0 is loaded in their place and multiplied by 0."""
    idx = np.asarray(idx, dtype=np.int64)
    n_src = hops[0].shape[0]
    ok = (idx >= 0) & (idx < n_src)
    safe = np.where(ok, idx, 0)
    rows = []
    for h in hops:
        g = h[safe].copy()
        if select:
            g[~ok] = 0.0
        else:
            with np.errstate(invalid="ignore"):
                g = g * ok[:, None].astype(F32)
        rows.append(g)
    return rows


def exact(case, C=None, idx=None, hops=None, **kw):
    """The fp64 restatement of the case (on the batch rows hop[idx] under an index), G = C."""
    hops = case["hops"] if hops is None else hops
    rows = hops if idx is None else gather(hops, idx)
    C = case["C"] if C is None else C
    with np.errstate(all="ignore"):
        if case["kind"] == "recursive":
            return RR.evaluate(rows, case["end"], case["w"], case["b"], G=C, **kw)
        return R.evaluate(case["kind"], rows, case["start"], case["end"], case["w"], case["b"], G=C, **kw)


def gate_scores(case, ref):
    """The arguments of the sigmoids, flat: z of the learnable kinds, s_1 .. s_{H-1} of the recursive form."""
    return (ref["s"][1:] if case["kind"] == "recursive" else ref["z"]).reshape(-1)


def regime_counts(scores):
    """{(regime, sign): how many scores fall into it}."""
    s = np.asarray(scores, dtype=np.float64)
    return {(name, sign): int(((np.abs(s) > lo) & (np.abs(s) < hi) & (np.sign(s) == sign)).sum())
            for name, (lo, hi) in REGIMES.items() for sign in (1, -1)}


def saturated(kind, n, d, T, start, end, seed):
    """random_case with row i of every panel scaled by GAINS[i mod 5], so |score| runs from 0.01 to several
    thousand with both signs (the features are symmetric about 0, so the bias as drawn leaves both signs
    saturated; the assertion below is the condition).  The narrow ranges of REGIMES are not left to chance: the
    first eight rows of gain 1 (rows 1, 6, .. 36) are scaled once more, each by the factor that carries its first
    score (slice position 0; step 1 of the recursive form), which is linear in the row's scale, to +-TARGETS.
    Asserts on the fp64 scores that every range holds a score of each sign."""
    assert n >= 40
    case = base(kind, n, d, T, start, end, seed)
    gain = np.array([GAINS[i % len(GAINS)] for i in range(n)], dtype=F32)[:, None]
    hops = [(h * gain).astype(F32) for h in case["hops"]]
    b = float(case["b"][0])
    probe = exact(dict(case, hops=hops))
    first = probe["s"][1] if kind == "recursive" else probe["z"][0]
    targets = [sign * t for t in TARGETS for sign in (1.0, -1.0)]
    for k, target in enumerate(targets):
        row = 1 + 5 * k
        assert abs(first[row] - b) > 1e-6
        c = F32((target - b) / (first[row] - b))
        for h in hops:
            h[row] = (h[row] * c).astype(F32)
    case["hops"] = hops
    counts = regime_counts(gate_scores(case, exact(case)))
    assert all(v > 0 for v in counts.values()), f"saturated {kind} d={d}: a range is not reached: {counts}"
    case["regimes"] = counts
    return case


def planted(kind, n, d, T, start, end, seed):
    """The O(1) case with single non-finite cells: NaN, +Inf and -Inf in panels inside the slice, +Inf in hop 0
    (outside the slice: a reference panel of ori_ref and jk, unread by gate; inside for the recursive form), NaN in
    the last panel (past the slice: a reference panel of jk, unread by the others), a whole NaN row in one slice
    panel, and one NaN row of the cotangent.  No finite magnitude exceeds 2^20, so no finite fp32 intermediate
    overflows and the classes of fp32 and fp64 results agree.  case["cells"]: (panel, row, column, value)."""
    lo = max(start, 1)
    assert n > 120 and end - lo >= 3 and end < T
    case = base(kind, n, d, T, start, end, seed)
    hops = [h.copy() for h in case["hops"]]
    cells = [(lo + 1, 7, 0, np.nan), (lo, 40, 3 % d, np.inf), (end - 1, 90, d - 1, -np.inf), (0, 100, 2 % d, np.inf),
             (T - 1, 120, 1 % d, np.nan)] + [(lo + 1, 55, c, np.nan) for c in range(d)]
    if kind == "recursive":
        # hop 0's Inf cells, one in a column where w_h and w_c have opposite signs (s_0 = p_0 + q_0 + b is
        # inf - inf = NaN: the reference's one-column softmax makes the whole row NaN) and one where they agree
        # (s_0 = +-inf, W(0) = 1: only the cell's own column of out is not finite), where d has such columns
        w = case["w"].reshape(-1)
        agree = w[:d] * w[d:] > 0
        case["s0_nan_row"] = 100 if (~agree).any() else None
        cells[3] = (0, 100, int(np.argmin(agree)), np.inf)
        cells.append((0, 110, int(np.argmax(agree)), -np.inf))
    for t, i, c, v in cells:
        hops[t][i, c] = v
    C = case["C"].copy()
    C[20, :] = np.nan
    assert max(float(np.abs(h[np.isfinite(h)]).max()) for h in hops) < 2.0 ** 20
    case.update(hops=hops, C=C, cells=cells)
    return case


def with_cells(case, value):
    """The panels of a planted case with every planted cell set to `value`."""
    hops = [h.copy() for h in case["hops"]]
    for t, i, c, _ in case["cells"]:
        hops[t][i, c] = value
    return hops


def unread_poison(kind, n, d, T, start, end, seed):
    """Every panel the kind does not read is NaN throughout (case["unread"]; jk reads every panel: none)."""
    case = base(kind, n, d, T, start, end, seed)
    read = reads(kind, T, case["start"], end)
    case["unread"] = [t for t in range(T) if t not in read]
    case["hops"] = [np.full_like(h, np.nan) if t in case["unread"] else h for t, h in enumerate(case["hops"])]
    return case


def with_unread(case, value):
    return [np.full_like(h, value) if t in case["unread"] else h for t, h in enumerate(case["hops"])]


def denormal_row(kind, n, d, T, start, end, seed):
    """Row DENORMAL_ROW of every slice panel holds (-1)^k k 2^-135 in column k - 1 (the same in every panel, so out
    there is about that value: subnormal, far above 2^-149 and nonzero unless something flushes it); row
    NEG_ZERO_ROW is all -0.0 and row POS_ZERO_ROW all +0.0 in every slice panel."""
    assert n > POS_ZERO_ROW
    case = base(kind, n, d, T, start, end, seed)
    k = np.arange(1, d + 1, dtype=np.float64)
    tiny = (np.where(k % 2 == 0, 1.0, -1.0) * k * DENORMAL_UNIT).astype(F32)
    assert (np.abs(tiny) < 2.0 ** -126).all() and tiny.all()
    hops = [h.copy() for h in case["hops"]]
    for t in slice_panels(kind, case["start"], end):
        hops[t][DENORMAL_ROW] = tiny
        hops[t][NEG_ZERO_ROW] = -0.0
        hops[t][POS_ZERO_ROW] = 0.0
    case["hops"] = hops
    return case


def row0_poison(kind, n_src, d, T, start, end, seed, B=230):
    """For the row-indexed form with check=False: row 0 of every panel is NaN (the row whose address stands in for
    an unreadable index) and the last row +Inf.  case["index"]: B entries, valid rows in [1, n_src - 2] with
    duplicates, and -1, n_src and 2^40 at case["bad"] -- indices the entries document as rows of zeros."""
    case = base(kind, n_src, d, T, start, end, seed)
    hops = [h.copy() for h in case["hops"]]
    for h in hops:
        h[0] = np.nan
        h[-1] = np.inf
    rng = np.random.default_rng(seed + 1)
    index = rng.integers(1, n_src - 1, B).astype(np.int64)
    index[B // 2:B // 2 + 20] = index[:20]
    for pos, v in ((3, -1), (64, n_src), (65, 2 ** 40), (B - 1, -1), (130, n_src)):
        index[pos] = v
    bad = (index < 0) | (index >= n_src)
    assert not np.isin(index[~bad], (0, n_src - 1)).any() and bad.sum() == 5
    case.update(hops=hops, index=index, bad=bad, C=cotangent(B, d, seed + 2))
    return case


def with_guard_rows(case, value):
    hops = [h.copy() for h in case["hops"]]
    for h in hops:
        h[0] = value
        h[-1] = value
    return hops


def _ftz(x):
    x = np.asarray(x, dtype=F32)
    return np.where(np.abs(x) < F32(2.0 ** -126), F32(0), x).astype(F32)


def emulate(kind, rows, start, end, w, b, G, sigmoid="stable", jacobian=True, pairing=None, flush=False):
    """(out, dw, db) of the learnable kinds' formula (§5.4.2) in plain numpy fp32 on the batch rows: not the
    kernels' order of operations, the same formula.  The keyword arguments are the negative controls:
    sigmoid="naive": expf(s) / (1 + expf(s)); jacobian=False: a backward without a (1 - a); pairing="transpose"
    for a kind the reference pairs with .view(-1, H); flush: subnormal inputs and results read as zero."""
    rows = [_ftz(h) if flush else np.asarray(h, dtype=F32) for h in rows]
    T, (n, d), H = len(rows), rows[0].shape, end - start
    w = np.asarray(w, dtype=F32).reshape(-1)
    b = F32(np.asarray(b).reshape(-1)[0])
    G = np.asarray(G, dtype=F32)
    Rr = R.in_dim(kind, T, d) - d
    refs = list(range(T)) if kind == "jk" else [0] if kind == "ori_ref" else []
    flat = (kind != "gate") if pairing is None else pairing == "flat"
    with np.errstate(all="ignore"):
        ref = np.zeros(n, F32)
        for t in refs:
            ref = (ref + rows[t] @ w[t * d:(t + 1) * d]).astype(F32)
        z = np.stack([ref + rows[start + h] @ w[Rr:] + b for h in range(H)]).astype(F32)
        S = R._pair(z, flat)
        if sigmoid == "naive":
            u = np.exp(S)
            a = (u / (F32(1) + u)).astype(F32)
        else:
            a = (F32(1) / (F32(1) + np.exp(-S))).astype(F32)
        e = np.exp(a)
        P = (e / e.sum(axis=1, keepdims=True)).astype(F32)
        out = P[:, 0:1] * rows[start]              # left to right, the first term as it is: -0.0 rows stay -0.0
        for h in range(1, H):
            out = (out + P[:, h:h + 1] * rows[start + h]).astype(F32)
        dP = np.stack([(G * rows[start + h]).sum(axis=1) for h in range(H)], axis=1).astype(F32)
        t = (P * dP).sum(axis=1, keepdims=True)
        da = P * (dP - t)
        dS = (da * (a * (F32(1) - a)) if jacobian else da).astype(F32)
        dz = R._unpair(dS, flat)
        s = dz.sum(axis=0)
        dw = np.zeros(Rr + d, F32)
        for t_ in refs:
            dw[t_ * d:(t_ + 1) * d] = s @ rows[t_]
        dw[Rr:] = sum(dz[h] @ rows[start + h] for h in range(H))
        db = s.sum()
    if flush:
        out, dw, db = _ftz(out), _ftz(dw), _ftz(db)
    return out, dw, db
