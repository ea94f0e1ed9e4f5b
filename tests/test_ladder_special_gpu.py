"""NaN, Inf, -0 and subnormals through every SpMM kernel role: the ladder operator (tests/ladder_cases.py)
with its special-value panels through the entries, schedules and widths of test_ladder_gpu.py, against
the CPU oracle's chains on the same inputs and the numpy epilogues (never another GPU result).

What the finite O(1) ladder cannot show and these inputs do:
  poison    X rows 0 and N - 1 are NaN.  A lane without an entry gathers with column id 0 and value 0; a
            guard (j + u < len, q < nb, nb) keeps it out of the chain.  fma(0, x, acc) == acc for finite x,
            so a dropped guard changes no bit on finite data -- and turns every short row NaN here.
  inf       +-Inf scattered over X: 0 * Inf is NaN too, and Inf - Inf depends on the chain's order.
  overflow  finite X, partial sums that cross FLT_MAX: which elements end infinite is the chain's order.
  sub_*     products, sums, results and X in the subnormal range: a kernel that flushes them (a changed
            denormal mode of one translation unit) returns zeros where the oracle has values.
  y0        ACCUMULATE from -0, +0, NaNs with payloads, +-Inf and subnormals: an empty row returns Y's bits
            (0.0f + y would turn -0 into +0), every other chain starts from them.

The comparison is ladder_cases.special_diff: bits wherever the expected word is no NaN; a NaN other than
the sentinel where it is one (payloads are not pinned); the guard columns, the rows a launch does not
schedule and the rows a kernel only moves bit for bit.  ladder_cases' CPU self-checks (test_ladder_cpu.py)
hold the references to the conditions that make these tests mean something.
"""
import functools

import numpy as np
import pytest
import torch

import ladder_cases as LC
import test_ladder_gpu as TL
from test_ladder_gpu import Panel, device_csr, no_empty_hub, rows_of, schedule

pytestmark = pytest.mark.gpu

N = LC.N
WIDTHS = [4, 20, 32, 36, 64, 100, 128, 256]


# ------------------------------------------------------------------------------------------------
# inputs and references, computed once per (kind, dtype, d) and never changed
# ------------------------------------------------------------------------------------------------
_SREF = {}


def case(oracle, kind, dtype, d):
    """(X, A X) of a special-value kind (None: the plain ladder panel) on the CPU oracle."""
    key = (kind, dtype, d)
    if key not in _SREF:
        if kind is None:
            X, y = LC.x_panel(dtype, d), TL.product(oracle, dtype, d)
        else:
            ip, ix, _ = LC.operator(dtype)
            v, X = LC.special(kind, dtype, d)
            with np.errstate(all="ignore"):
                y = oracle.spmm(ip, ix, v, X) if dtype == "float32" else oracle.spmm64(ip, ix, v, X)
        X.setflags(write=False)
        y.setflags(write=False)
        _SREF[key] = (X, y)
    return _SREF[key]


@functools.lru_cache(maxsize=None)
def dev_arrays(kind, dtype="float32"):
    """The device operator of a kind: the ladder's, with the scaled values for the subnormal kinds."""
    ip, ix, v = TL.dev_operator(dtype)
    if kind in LC.SUB_SCALES:
        v = torch.from_numpy(LC.special(kind, dtype, 1)[0]).cuda()
    return ip, ix, v


def check(panel, expected, what, sched=None, moved_empty=False):
    """Panel.check with the NaN-aware comparison.  Rows `sched` leaves out must come back bit for bit;
    moved_empty: the empty rows too (ACCUMULATE only moves them)."""
    exact = np.zeros(N, dtype=bool)
    if sched is not None:
        exact[np.setdiff1d(np.arange(N), sched[0])] = True
    if moved_empty:
        exact |= LC.lengths() == 0
    got = panel.dev.cpu().numpy()
    lens = LC.lengths()
    msg = [LC.special_diff(g, w, lens, TL.SENTINEL[panel.dtype], exact)
           for g, w in zip(got.reshape(-1, N, panel.ld), expected.reshape(-1, N, panel.ld))]
    if any(msg):
        raise AssertionError(f"{what}: window columns [{panel.off}, {panel.off + panel.d}) of {panel.ld}: "
                             + " | ".join(m or "no difference" for m in msg))


def agg_ref(prev, w, y, init=False):
    with np.errstate(all="ignore"):
        return LC.agg_ref(prev, w, y, init)


# ------------------------------------------------------------------------------------------------
# srg_spmm_csr_f32
# ------------------------------------------------------------------------------------------------
def run_csr(oracle, kind, d, sched, y_ld=None, y_off=TL.GUARD, **flags):
    from srgnn.spmm import spmm
    s = schedule(sched)
    no_empty_hub(s)
    x, y = case(oracle, kind, "float32", d)
    X = Panel("float32", d, x)
    Y = Panel("float32", d, ld=y_ld, off=y_off)
    spmm(device_csr(s, arrays=dev_arrays(kind)), X.win, out=Y.win, **flags)
    check(Y, Y.expect(y, rows_of(s)), f"srg_spmm_csr_f32 {kind} d={d} {sched} {flags}", s)
    X.check(X.host, "the gathered panel")


@pytest.mark.parametrize("sched", ["desc_hub", "rand1", "all_heavy", "all_light"])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", LC.KINDS)
def test_csr_special_every_width(oracle_mod, kind, d, sched):
    """Narrow rows with 4 and 32 lanes (unfull, full), the unfull slice, packed rows with 8 / 4 / 2 rows per
    wave beside the XCD-aware slice waves, row waves; every non-empty row a hub row with full DPP windows
    and partial windows of every length (desc_hub), a mixed bag (rand1), every row a slice-wave row, every
    row a light row."""
    run_csr(oracle_mod, kind, d, sched)


@pytest.mark.parametrize("flag", ["packed_u2", "wide_rows", "hub_w256"])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("kind", LC.KINDS)
def test_csr_special_flags(oracle_mod, kind, d, flag):
    run_csr(oracle_mod, kind, d, "rand1", **{flag: True})


@pytest.mark.parametrize("kind", LC.KINDS)
def test_csr_special_vec2_row_waves(oracle_mod, kind):
    """d = 128 into a panel of leading dimension 130: no packed rows, two columns per lane."""
    run_csr(oracle_mod, kind, 128, "rand1", y_ld=130, y_off=2)


@pytest.mark.parametrize("sched", ["rand1", "all_heavy"])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", [None, "sub_deep"])
def test_accumulate_from_special_words(oracle_mod, kind, d, sched):
    """ACCUMULATE from y0_special: the empty rows (and the rows rand1 leaves out) come back bit for bit,
    payloads and -0 included; every other chain starts from Y's word and is the oracle's."""
    from srgnn.spmm import spmm
    s = schedule(sched)
    no_empty_hub(s)
    x, _ = case(oracle_mod, kind, "float32", d)
    y0 = LC.y0_special(d)
    key = ("acc", kind, d)
    if key not in _SREF:
        ip, ix, _ = LC.operator("float32")
        v = dev_arrays(kind)[2].cpu().numpy()
        with np.errstate(all="ignore"):
            _SREF[key] = oracle_mod.spmm(ip, ix, v, x, out=y0.copy(), accumulate=True)
    X = Panel("float32", d, x)
    Y = Panel("float32", d, y0)
    spmm(device_csr(s, arrays=dev_arrays(kind)), X.win, out=Y.win, accumulate=True)
    check(Y, Y.expect(_SREF[key], rows_of(s)), f"ACCUMULATE from y0_special, {kind} d={d} {sched}", s, moved_empty=True)
    X.check(X.host, "the gathered panel")


# ------------------------------------------------------------------------------------------------
# srg_spmm_span_f32 and the planned hop: between column blocks the chain's state is a stored fp32
# ------------------------------------------------------------------------------------------------
BLOCK_KINDS = ["poison", "inf", "overflow", "sub_edge"]


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("kind", BLOCK_KINDS)
def test_span_blocks_special(oracle_mod, kind, d):
    """test_span_blocks_of_random_cuts' construction: block 0 plain, block 1 ACCUMULATE (then with the
    aggregation epilogue) is the oracle's whole-row chain -- infinities, NaNs and subnormals survive
    the round trip through Y."""
    from srgnn.spmm import spmm, spmm_agg
    arrays = dev_arrays(kind)
    ip = arrays[0]
    indptr = LC.structure()[0]
    cut = TL.random_cuts(d)
    mid = torch.from_numpy(indptr[:-1] + cut).cuda()
    beg, end = ip[:-1].contiguous(), ip[1:].contiguous()
    l0, l1 = cut, LC.lengths() - cut
    s0 = LC.sched_rand(l0, 6, *TL.rand_counts(6))
    s1 = LC.sched_rand(l1, 7, *TL.rand_counts(7))
    for s, l in ((s0, l0), (s1, l1)):
        assert l[s[0][:s[1]]].min() > 0 and l[s[0][:s[1]]].max() > 100
    B0, B1 = device_csr(s0, spans=(beg, mid), arrays=arrays), device_csr(s1, spans=(mid, end), arrays=arrays)
    x, y = case(oracle_mod, kind, "float32", d)
    prev = LC.side_panel("float32", d, 3)
    X = Panel("float32", d, x)
    for agg in (False, True):
        Y, G = Panel("float32", d), Panel("float32", d, prev)
        spmm(B0, X.win, out=Y.win)
        if agg:
            spmm_agg(B1, X.win, Y.win, G.win, TL.W_AGG, False, accumulate=True)
        else:
            spmm(B1, X.win, out=Y.win, accumulate=True)
        check(Y, Y.expect(y), f"srg_spmm_span_f32 {kind} d={d} agg={agg}")
        check(G, G.expect(agg_ref(prev, TL.W_AGG, y)) if agg else G.host, f"srg_spmm_span_f32 agg panel {kind} d={d} agg={agg}")


@pytest.mark.parametrize("agg", [False, True])
@pytest.mark.parametrize("col_blocks", [None, 2, 5])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kind", BLOCK_KINDS)
def test_planned_hop_special(oracle_mod, kind, d, col_blocks, agg):
    """spmm.hop through the native plan (the planner's own schedules and column blocks)."""
    from srgnn.csr import DeviceCSR
    from srgnn.spmm import hop
    ip, ix, v = dev_arrays(kind)
    A = DeviceCSR(ip, ix, v, N, N, None, None, None, None)
    x, y = case(oracle_mod, kind, "float32", d)
    prev = LC.side_panel("float32", d, 4)
    X = Panel("float32", d, x)
    Y, G = Panel("float32", d), Panel("float32", d, prev)
    try:
        hop(A, X.win, Y.win, col_blocks=col_blocks, agg=(G.win, TL.W_AGG, False) if agg else None)
        torch.cuda.synchronize()
        check(Y, Y.expect(y), f"hop {kind} d={d} col_blocks={col_blocks} agg={agg}")
        check(G, G.expect(agg_ref(prev, TL.W_AGG, y)) if agg else G.host, f"hop agg panel {kind} d={d} col_blocks={col_blocks}")
    finally:
        A.drop_blocks()


# ------------------------------------------------------------------------------------------------
# srg_spmm_agg_f32: agg = aprev + w * acc, product and sum rounded separately
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["desc_hub", "rand1"])
@pytest.mark.parametrize("d", [32, 64, 100])
@pytest.mark.parametrize("kind", ["poison", "inf", "sub_deep"])
def test_agg_special(oracle_mod, kind, d, sched):
    """INIT (the panel's content, y0_special, must not reach the result) and ADD from y0_special.  With
    sub_deep the products 0.37 acc are subnormal (test_ladder_cpu.py holds the reference to that), and
    they meet y0_special's zeros and subnormals in the sum."""
    from srgnn.spmm import spmm_agg
    s = schedule(sched)
    no_empty_hub(s)
    x, y = case(oracle_mod, kind, "float32", d)
    prev = LC.y0_special(d)
    X = Panel("float32", d, x)
    A = device_csr(s, arrays=dev_arrays(kind))
    for init in (True, False):
        Y, G = Panel("float32", d), Panel("float32", d, prev)
        spmm_agg(A, X.win, Y.win, G.win, TL.W_AGG, init)
        what = f"srg_spmm_agg_f32 {kind} d={d} {sched} init={init}"
        check(Y, Y.expect(y, rows_of(s)), what + " Y", s)
        check(G, G.expect(agg_ref(prev, TL.W_AGG, y, init), rows_of(s)), what + " agg", s)


# ------------------------------------------------------------------------------------------------
# the Chebyshev family (its own translation unit): special values in the gathered panel only
# ------------------------------------------------------------------------------------------------
def cheby_case(oracle, kind, dtype, d, mode, ns, rows, alias=False):
    x, acc = case(oracle, kind, dtype, d)
    with np.errstate(all="ignore"):
        return TL.cheby_case(oracle, dtype, d, mode, ns, rows, alias, acc=acc, tc=x)


@pytest.mark.parametrize("d,sched", [(32, "desc_hub"), (64, "asc"), (100, "rand1")])
@pytest.mark.parametrize("kind", LC.KINDS)
def test_spmm_cheby_f32_special(oracle_mod, kind, d, sched):
    """srg_spmm_cheby_f32 as test_spmm_cheby_f32 runs it: narrow, packed and one column per lane, hub
    windows of 256 and 512 entries.  Of the subnormal kinds only sub_x shows a flushed chain here: the
    epilogue subtracts a2 Tc (INIT) or the O(1) To (STEP) from acc, and sub_deep's and sub_edge's acc lies
    a hundred binades below their Tc -- the result does not depend on it.  With sub_x, Tc is subnormal too."""
    from srgnn.spmm import spmm_cheby
    s = schedule(sched)
    no_empty_hub(s)
    A = device_csr(s, arrays=dev_arrays(kind))
    a1, a2 = TL.scalar("float32", TL.A1), TL.scalar("float32", TL.A2)
    for mode, ns, alias in ((LC.INIT, 1, False), (LC.INIT, 3, False), (LC.STEP, 1, False), (LC.STEP, 3, False),
                            (LC.STEP, 3, True)):
        Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, kind, "float32", d, mode, ns, rows_of(s), alias)
        spmm_cheby(A, Tc.win, Tn.win, mode, a1, a2, To.win if mode == LC.STEP else None, cp, cc, R.win)
        what = f"srg_spmm_cheby_f32 {kind} d={d} {sched} mode={mode} scales={ns} alias={alias}"
        check(Tn, want_t, what + " Tn", s)
        check(R, want_r, what + " R", s)
        Tc.check(Tc.host, what + " Tc")


def run_cheby_step(oracle, entry, kind, dtype, d, s, what):
    no_empty_hub(s)
    for mode in TL.ALL_MODES:
        Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle, kind, dtype, d, mode, 3, rows_of(s))
        TL.cheby_step(entry, dtype, s, Tc, To, Tn, R, d, mode, cp, cc, 3)
        check(Tn, want_t, f"{entry} {kind} d={d} {what} mode={mode:#x} Tn", s)
        check(R, want_r, f"{entry} {kind} d={d} {what} mode={mode:#x} R", s)
        Tc.check(Tc.host, f"{entry} {kind} d={d} {what} mode={mode:#x} Tc")


@pytest.mark.parametrize("d", [5, 64, 130])
@pytest.mark.parametrize("kind", ["poison", "inf"])
def test_cheby_step_f32_special(oracle_mod, kind, d):
    s = LC.sched_rand(LC.lengths(), 8, 0, 0, leave_out=64)
    run_cheby_step(oracle_mod, "srg_cheby_step_f32", kind, "float32", d, s, "random order")


@pytest.mark.parametrize("sched", ["rows", "desc", "rand_w512", "all_hub"])
@pytest.mark.parametrize("d", [5, 16, 64, 130])
@pytest.mark.parametrize("kind", ["poison", "inf"])
def test_cheby_step_f64_special(oracle_mod, kind, d, sched):
    """srg_cheby_step_f64 (sched = rows) and srg_cheby_step_hub_f64 (512- and 256-entry windows; d = 5 runs
    the hub rows as row waves) against oracle.spmm64 on the fp64 panels."""
    entry = "srg_cheby_step_f64" if sched == "rows" else "srg_cheby_step_hub_f64"
    run_cheby_step(oracle_mod, entry, kind, "float64", d, TL.schedule64(sched, d), sched)
