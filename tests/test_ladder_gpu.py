"""Every SpMM kernel role at every row length and under any schedule: the ladder operator
(tests/ladder_cases.py) through the C-ABI's SpMM and Chebyshev entries, bit for bit against the CPU
oracle's chains and the numpy epilogues.

Every comparison is of bits, against a CPU reference (never another GPU result).  Every panel a launch
writes is a column window of a wider buffer filled with a sentinel; the whole buffer is compared, so
the guard columns and the rows a launch does not schedule must come back untouched.  A failure names
the first differing row, its length and column: with the schedule that locates the window or chunk.

Which case reaches which instantiation (the SpMM kernels of csrc/srg_spmm_kernels.h, instantiated with the
plain and span epilogues by csrc/srg_spmm.hip and with the Chebyshev one by csrc/srg_cheby.hip, which also
holds k_cheby*; the device entries pass int64 row pointers, the int32 ones belong to the host drop-in
entries and are not run here):

  launch_spmm -> k_spmm, epilogue plain (test_csr_*), Chebyshev (test_spmm_cheby_f32: d = 32 narrow, 64
  packed, 100 one column per lane) and span (test_span_blocks_of_random_cuts: d = 32, 64, 128;
  test_planned_hop); light rows by width, slice waves beside them wherever the schedule has heavy rows:
    narrow rows, 1 / 2 / 8 / 16 lanes per row      test_csr_other_row_wave_shapes d = 1, 2, 8, 16
    narrow rows, 4 lanes; 32 lanes unfull / full   test_csr_every_width_and_schedule d = 4; 20; 32
    packed rows 8 / 4 / 2 per wave, 4 gathers      test_csr_every_width_and_schedule d = 64 / 128 / 256
      (always with the XCD-aware slice waves: a packed width has 2, 4 or 8 slices, so the packed
      instantiation without them cannot be reached through any entry)
    packed rows, 2 gathers (PACKED_U2)             test_csr_flags[*-packed_u2] d = 64, 128, 256
    row waves <VEC 1, full tile, full slice>       test_csr_flags[64-wide_rows]
    row waves <1, unfull, full slice>              test_csr_other_row_wave_shapes d = 96
    row waves <1, unfull, unfull slice>            test_csr_every_width_and_schedule d = 36, 100
    row waves <2, full, full>                      test_csr_vec2_row_waves (d = 128, ld 130), test_csr_flags[128-wide_rows]
    row waves <2, unfull, full> / <2, unfull, unfull>   test_csr_other_row_wave_shapes d = 160 / 130
    row waves <4, full, full>                      test_csr_flags[256-wide_rows]
    row waves <4, unfull, full> / <4, unfull, unfull>   test_csr_other_row_wave_shapes d = 288 / 260
    slice waves, 8 / 4 groups in flight            every schedule with heavy rows; 4 at d = 128 / 256 packed
  k_spmm_hub<full slice | unfull, epilogue, W>:
    plain, W = 512     rand1 / rand2 up to d = 128 and asc up to d = 64 (n_hub * n_slices <= 256; unfull: d = 4, 20, 36, 100);
                       test_hub_window_512_every_length d = 32 (full), 36 (unfull): every length
    plain, W = 256     desc_hub / all_hub (4,049 hub rows: every length), rand at d = 256, test_csr_flags[*-hub_w256]
    Chebyshev          test_spmm_cheby_f32: W = 256 desc_hub, asc at d = 100; W = 512 asc d = 32, 64 and rand1
    span               test_span_blocks_of_random_cuts: W = 512 (<= 64 hub rows); W = 256 is reached by
                       test_aggregate_gpu.py::test_span_blocks_every_path with thresholds (0, 0), not here
  k_cheby<float, 1 | 2>     test_cheby_step_f32_random_order d = 5, 64 | 130
  k_cheby<double, 1 | 2>    test_cheby_step_f64 d = 2, 5, 16, 20, 64 | 130 (every schedule's row-wave rows; all rows
                            at d = 5 and with sched = rows)
  k_cheby_hub64<512>        test_cheby_step_f64 desc (d <= 20), asc (d <= 64), rand_w512; test_hub64_window_512_every_length
  k_cheby_hub64<256>        test_cheby_step_f64 rand_w256, all_hub (every length), desc (d >= 64), asc (d = 130)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ladder_cases as LC

pytestmark = pytest.mark.gpu

GUARD = 4                                   # guard columns on each side of a panel's window (16 / 32 bytes)
SENTINEL = {"float32": 0x7FC0DEAD, "float64": 0x7FF8DEADBEEF0BAD}     # quiet NaNs no kernel produces
A1, A2 = 1.37, 0.81                         # the Chebyshev epilogue's scalars (fp32-exact after rounding)
COEF = np.array([[0.73, -1.19, 0.57], [-0.41, 0.88, 1.31], [1.07, 0.29, -0.66]])   # [c0 | c1 | ck][scale]
N = LC.N


# ------------------------------------------------------------------------------------------------
# references, computed once per (dtype, d) and never changed
# ------------------------------------------------------------------------------------------------
_REF = {}


def product(oracle, dtype, d):
    """A X on the CPU oracle: one chain per element in CSR order."""
    key = (dtype, d)
    if key not in _REF:
        ip, ix, v = LC.operator(dtype)
        X = LC.x_panel(dtype, d)
        y = oracle.spmm(ip, ix, v, X) if dtype == "float32" else oracle.spmm64(ip, ix, v, X)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


@functools.lru_cache(maxsize=None)
def dev_operator(dtype):
    return tuple(torch.from_numpy(a.copy()).cuda() for a in LC.operator(dtype))


def scalar(dtype, x):
    return float(np.dtype(dtype).type(x))


def coefs(dtype, row, ns):
    return np.array([scalar(dtype, c) for c in COEF[row, :ns]])


# ------------------------------------------------------------------------------------------------
# guarded panels
# ------------------------------------------------------------------------------------------------
class Panel:
    """A [lead, N, d] panel as the column window [off, off + d) of a sentinel-filled [lead, N, ld] buffer,
    on the host (.host) and the device (.dev; .win is the window: [N, d], or [lead, N, d] with lead)."""

    def __init__(self, dtype, d, content=None, lead=None, ld=None, off=GUARD):
        self.dtype, self.d, self.off = dtype, d, off
        self.ld = ld if ld is not None else d + 2 * GUARD
        u = np.uint32 if dtype == "float32" else np.uint64
        shape = (N, self.ld) if lead is None else (lead, N, self.ld)
        self.host = np.full(shape, SENTINEL[dtype], dtype=u).view(np.dtype(dtype))
        if content is not None:
            self.host[..., off:off + d] = content
        self.dev = torch.from_numpy(self.host).cuda()
        self.win = self.dev[..., off:off + d]

    def expect(self, want, rows=None):
        """The buffer after a launch that writes `want` (a [.., N, d] panel) into the window at `rows`
        (all rows when None) and nothing else."""
        e = self.host.copy()
        if rows is None:
            e[..., self.off:self.off + self.d] = want
        else:
            e[..., rows, self.off:self.off + self.d] = want[..., rows, :]
        return e

    def check(self, expected, what):
        it = torch.int32 if self.dtype == "float32" else torch.int64
        want = torch.from_numpy(expected).cuda()
        if torch.equal(self.dev.view(it), want.view(it)):
            return
        got = self.dev.cpu().numpy()
        lens = LC.lengths()
        msg = [LC.first_diff(g, w, lens) for g, w in zip(got.reshape(-1, N, self.ld), expected.reshape(-1, N, self.ld))]
        raise AssertionError(f"{what}: window columns [{self.off}, {self.off + self.d}) of {self.ld}: " + " | ".join(msg))


# ------------------------------------------------------------------------------------------------
# schedules
# ------------------------------------------------------------------------------------------------
def rand_counts(seed):
    """(n_hub, n_heavy) of a random schedule: a mixed bag of lengths for every role, few enough hub
    rows for 512-entry windows up to d = 128 (4 slices) and 256-entry ones at d = 256."""
    rng = np.random.default_rng([LC.SEED, 9, seed])
    return int(rng.integers(40, 65)), int(rng.integers(600, 1800))


def schedule(name):
    lens = LC.lengths()
    n_full = int((lens > 0).sum())
    if name == "desc_light":
        return LC.sched_desc(lens, -1, -1)
    if name == "desc_heavy":
        return LC.sched_desc(lens, 0, -1)
    if name == "desc_hub":
        return LC.sched_desc(lens, 0, 0)
    if name == "asc":
        return LC.sched_asc(lens, 96, 700)
    if name in ("rand1", "rand2"):
        seed = int(name[-1])
        return LC.sched_rand(lens, seed, *rand_counts(seed), leave_out=100 if seed == 1 else 37)
    if name == "all_hub":         # a random order of the non-empty rows, every one a hub row; the empty rows light
        order, _, _ = LC.sched_rand(lens, 3, 0, 0)
        order = np.concatenate([order[lens[order] > 0], order[lens[order] == 0]]).astype(np.int32)
        return order, n_full, 0
    if name == "all_heavy":       # every row (the empty ones too) a slice-wave row, random order
        return LC.sched_rand(lens, 4, 0, N)
    if name == "all_light":
        return LC.sched_rand(lens, 5, 0, 0)
    raise KeyError(name)


SCHEDULES = ["desc_light", "desc_heavy", "desc_hub", "asc", "rand1", "rand2", "all_hub", "all_heavy", "all_light"]


def no_empty_hub(sched):
    order, n_hub, _ = sched
    assert LC.lengths()[order[:n_hub]].min(initial=1) > 0, "an empty row in the hub prefix"


def device_csr(sched, dtype="float32", spans=None, arrays=None):
    from srgnn.csr import DeviceCSR
    order, n_hub, n_heavy = sched
    ip, ix, v = dev_operator(dtype) if arrays is None else arrays
    o = torch.from_numpy(order).cuda()
    if spans is None:
        return DeviceCSR(ip, ix, v, int(order.size), N, o, n_heavy, n_hub, None, row_space=N)
    beg, end = spans
    return DeviceCSR(beg, ix, v, int(order.size), N, o, n_heavy, n_hub, None, row_end=end, row_space=N)


def rows_of(sched):
    order = sched[0]
    return None if order.size == N else np.sort(order)


# ------------------------------------------------------------------------------------------------
# srg_spmm_csr_f32
# ------------------------------------------------------------------------------------------------
def run_csr(oracle, d, sched, what, x_ld=None, y_ld=None, y_off=GUARD, **flags):
    from srgnn.spmm import spmm
    no_empty_hub(sched)
    A = device_csr(sched)
    X = Panel("float32", d, LC.x_panel("float32", d), ld=x_ld)
    Y = Panel("float32", d, ld=y_ld, off=y_off)
    spmm(A, X.win, out=Y.win, **flags)
    Y.check(Y.expect(product(oracle, "float32", d), rows_of(sched)), f"srg_spmm_csr_f32 d={d} {what} {flags}")
    X.check(X.host, "the gathered panel")


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("d", [4, 20, 32, 36, 64, 100, 128, 256])
def test_csr_every_width_and_schedule(oracle_mod, d, sched):
    """Plain and NT_STORE launches over the widths that select narrow rows (4 and 32 lanes per row), the
    unfull slice (20, 36, 100), packed rows with 8 / 4 / 2 rows per wave (64 / 128 / 256, with the
    XCD-aware slice waves) and the plain vector path (36, 100), under the project's schedules, an
    increasing one, two random ones and the one-role sweeps."""
    s = schedule(sched)
    run_csr(oracle_mod, d, s, sched)
    run_csr(oracle_mod, d, s, sched, nt_store=True)


@pytest.mark.parametrize("sched", ["desc_hub", "rand1", "all_heavy"])
def test_csr_vec2_row_waves(oracle_mod, sched):
    """d = 128 into a panel of leading dimension 130: no packed rows, two columns per lane."""
    run_csr(oracle_mod, 128, schedule(sched), sched, y_ld=130, y_off=2)


@pytest.mark.parametrize("d", [1, 2, 8, 16, 96, 130, 160, 260, 288])
def test_csr_other_row_wave_shapes(oracle_mod, d):
    """The remaining row-wave instantiations: narrow rows with 1 / 2 / 8 / 16 lanes per row, one column
    per lane with full slices (96), two (130: no slice paths; 160) and four (260, 288) in an unfull tile."""
    run_csr(oracle_mod, d, schedule("rand2"), "rand2")


@pytest.mark.parametrize("flag", ["accumulate", "wide_rows", "packed_u2", "hub_w256"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_csr_flags(oracle_mod, d, flag):
    from srgnn.spmm import spmm
    sched = schedule("rand1")
    if flag != "accumulate":
        return run_csr(oracle_mod, d, sched, "rand1", **{flag: True})
    ip, ix, v = LC.operator("float32")
    y0 = LC.side_panel("float32", d, 1)
    key = ("acc", d)
    if key not in _REF:
        _REF[key] = oracle_mod.spmm(ip, ix, v, LC.x_panel("float32", d), out=y0.copy(), accumulate=True)
    X = Panel("float32", d, LC.x_panel("float32", d))
    Y = Panel("float32", d, y0)
    spmm(device_csr(sched), X.win, out=Y.win, accumulate=True)
    Y.check(Y.expect(_REF[key], rows_of(sched)), f"ACCUMULATE d={d}")


@pytest.mark.parametrize("sched", ["desc_hub", "all_heavy", "all_light"])
def test_comparison_sees_a_swapped_pair(oracle_mod, sched):
    """The check itself: the kernels run the operator with the last two links of every row swapped, and
    the comparison with the unswapped oracle then fails in at least 95 % of those rows -- while the
    result is the swapped operator's oracle chain, bit for bit."""
    from srgnn.spmm import spmm
    d = 32
    ip, ix, v = LC.operator("float32")
    mix, mv, rows = LC.swap_links(ip, ix, v, LC.mutations(LC.lengths(), False)["last"])
    arrays = (dev_operator("float32")[0], torch.from_numpy(mix).cuda(), torch.from_numpy(mv).cuda())
    X = Panel("float32", d, LC.x_panel("float32", d))
    Y = Panel("float32", d)
    spmm(device_csr(schedule(sched), arrays=arrays), X.win, out=Y.win)
    Y.check(Y.expect(oracle_mod.spmm(ip, mix, mv, LC.x_panel("float32", d))), "the swapped operator")
    with pytest.raises(AssertionError, match="rows differ"):
        Y.check(Y.expect(product(oracle_mod, "float32", d)), "expected to differ")
    got = Y.dev.cpu().numpy()[:, GUARD:GUARD + d]
    changed = (got.view(np.uint32) != product(oracle_mod, "float32", d).view(np.uint32)).any(axis=1)
    assert not changed[np.setdiff1d(np.arange(N), rows)].any() and changed[rows].sum() >= 0.95 * rows.size


@pytest.mark.parametrize("d", [32, 36])
def test_hub_window_512_every_length(oracle_mod, d):
    """Every non-empty row once through the 512-entry hub windows: launches whose hub prefix is another
    group of at most 256 // n_slices rows (more hub workgroups than 256 would take 256-entry windows)."""
    from srgnn.spmm import spmm
    n_slices = -(-d // 32)
    launches = LC.w512_sweep(LC.lengths(), n_slices)
    X = Panel("float32", d, LC.x_panel("float32", d))
    Y = Panel("float32", d)
    want = torch.from_numpy(Y.expect(product(oracle_mod, "float32", d))).cuda().view(torch.int32)
    blank = torch.from_numpy(Y.host).cuda()
    for i, s in enumerate(launches):
        assert s[1] * n_slices <= 256 and s[1] > 0
        no_empty_hub(s)
        Y.dev.copy_(blank)
        spmm(device_csr(s), X.win, out=Y.win)
        if not torch.equal(Y.dev.view(torch.int32), want):
            hub = LC.lengths()[s[0][:s[1]]]
            Y.check(Y.expect(product(oracle_mod, "float32", d)), f"launch {i}, hub rows of lengths {sorted(hub.tolist())}")


# ------------------------------------------------------------------------------------------------
# srg_spmm_agg_f32, srg_spmm_span_f32, the planned hop
# ------------------------------------------------------------------------------------------------
W_AGG = 0.37


@pytest.mark.parametrize("sched", ["desc_hub", "rand1"])
@pytest.mark.parametrize("d", [32, 64, 100])
def test_agg_init_and_add(oracle_mod, d, sched):
    from srgnn.spmm import spmm_agg
    s = schedule(sched)
    y = product(oracle_mod, "float32", d)
    prev = LC.side_panel("float32", d, 2)
    X = Panel("float32", d, LC.x_panel("float32", d))
    for init in (True, False):
        Y, G = Panel("float32", d), Panel("float32", d, prev)
        spmm_agg(device_csr(s), X.win, Y.win, G.win, W_AGG, init)
        Y.check(Y.expect(y, rows_of(s)), f"srg_spmm_agg_f32 Y d={d} {sched} init={init}")
        G.check(G.expect(LC.agg_ref(prev, W_AGG, y, init), rows_of(s)), f"srg_spmm_agg_f32 agg d={d} {sched} init={init}")


def random_cuts(seed):
    """Every row cut at a seeded random point, 0 and the full length included (and both often)."""
    lens = LC.lengths()
    rng = np.random.default_rng([LC.SEED, 11, seed])
    cut = rng.integers(0, lens + 1)
    pick = rng.random(N)
    cut = np.where(pick < 0.1, 0, np.where(pick > 0.9, lens, cut))
    return cut.astype(np.int64)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_span_blocks_of_random_cuts(oracle_mod, d):
    """Two span operators from a random cut of every row, each with its own random schedule of its span
    lengths: block 0 plain, block 1 ACCUMULATE -- the oracle's whole-row chain; then block 1 with the
    aggregation epilogue."""
    from srgnn.spmm import spmm, spmm_agg
    ip, _, _ = dev_operator("float32")
    indptr = LC.structure()[0]
    cut = random_cuts(d)
    mid = torch.from_numpy(indptr[:-1] + cut).cuda()
    beg, end = ip[:-1].contiguous(), ip[1:].contiguous()
    l0, l1 = cut, LC.lengths() - cut
    s0 = LC.sched_rand(l0, 6, *rand_counts(6))
    s1 = LC.sched_rand(l1, 7, *rand_counts(7))
    for s, l in ((s0, l0), (s1, l1)):
        assert l[s[0][:s[1]]].min() > 0 and l[s[0][:s[1]]].max() > 100
    B0, B1 = device_csr(s0, spans=(beg, mid)), device_csr(s1, spans=(mid, end))
    y = product(oracle_mod, "float32", d)
    prev = LC.side_panel("float32", d, 3)
    X = Panel("float32", d, LC.x_panel("float32", d))
    for agg in (False, True):
        Y, G = Panel("float32", d), Panel("float32", d, prev)
        spmm(B0, X.win, out=Y.win)
        if agg:
            spmm_agg(B1, X.win, Y.win, G.win, W_AGG, False, accumulate=True)
        else:
            spmm(B1, X.win, out=Y.win, accumulate=True)
        Y.check(Y.expect(y), f"srg_spmm_span_f32 d={d} agg={agg}")
        G.check(G.expect(LC.agg_ref(prev, W_AGG, y)) if agg else G.host, f"srg_spmm_span_f32 agg panel d={d} agg={agg}")


@pytest.mark.parametrize("agg", [False, True])
@pytest.mark.parametrize("col_blocks", [None, 2, 5])
@pytest.mark.parametrize("d", [64, 128])
def test_planned_hop(oracle_mod, d, col_blocks, agg):
    """spmm.hop through the native plan (the planner's own schedules and column blocks)."""
    from srgnn.csr import DeviceCSR
    from srgnn.spmm import hop
    ip, ix, v = dev_operator("float32")
    A = DeviceCSR(ip, ix, v, N, N, None, None, None, None)
    y = product(oracle_mod, "float32", d)
    prev = LC.side_panel("float32", d, 4)
    X = Panel("float32", d, LC.x_panel("float32", d))
    Y, G = Panel("float32", d), Panel("float32", d, prev)
    try:
        hop(A, X.win, Y.win, col_blocks=col_blocks, agg=(G.win, W_AGG, False) if agg else None)
        torch.cuda.synchronize()
        Y.check(Y.expect(y), f"hop d={d} col_blocks={col_blocks} agg={agg}")
        G.check(G.expect(LC.agg_ref(prev, W_AGG, y)) if agg else G.host, f"hop agg panel d={d} col_blocks={col_blocks}")
    finally:
        A.drop_blocks()


# ------------------------------------------------------------------------------------------------
# the Chebyshev entries
# ------------------------------------------------------------------------------------------------
def cheby_case(oracle, dtype, d, mode, ns, rows, alias=False, acc=None, tc=None):
    """The operands and the expected buffers of one step over the ladder operator: acc = A Tc is the
    oracle's, the epilogue numpy's.  Returns (Tc, To, Tn, R panels, expected Tn buffer, expected R buffer,
    coef_prev, coef).  acc, tc: another gathered panel and its product (the special-value cases)."""
    m = mode & 0xF
    if acc is None:
        acc, tc = product(oracle, dtype, d), LC.x_panel(dtype, d)
    to = LC.side_panel(dtype, d, 5)
    r0 = np.stack([LC.side_panel(dtype, d, 6 + s) for s in range(ns)])
    cp = None
    if m == LC.INIT:
        cp = coefs(dtype, 0, ns)
    elif m == LC.STEP_FIRST:
        cp = np.concatenate([coefs(dtype, 0, ns), coefs(dtype, 1, ns)])
    cc = None if m == LC.INIT_T else coefs(dtype, 1 if m == LC.INIT else 2, ns)
    tn, r = LC.cheby_ref(mode, acc, tc, to, r0, scalar(dtype, A1), scalar(dtype, A2), cp, cc)
    Tc, To, R = Panel(dtype, d, tc), Panel(dtype, d, to), Panel(dtype, d, r0, lead=ns)
    Tn = To if alias else Panel(dtype, d)
    want_t = Tn.host if tn is None else Tn.expect(tn, rows)
    return Tc, To, Tn, R, want_t, R.expect(r, rows), cp, cc


@pytest.mark.parametrize("sched", ["desc_hub", "asc", "rand1"])
@pytest.mark.parametrize("d", [32, 64, 100])
def test_spmm_cheby_f32(oracle_mod, d, sched):
    """srg_spmm_cheby_f32: INIT and STEP with 1 and 3 scales (the third scale's output is read after the
    chain), and a STEP whose Tn is To itself."""
    from srgnn.spmm import spmm_cheby
    s = schedule(sched)
    no_empty_hub(s)
    A = device_csr(s)
    for mode, ns, alias in ((LC.INIT, 1, False), (LC.INIT, 3, False), (LC.STEP, 1, False), (LC.STEP, 3, False),
                            (LC.STEP, 3, True)):
        Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, "float32", d, mode, ns, rows_of(s), alias)
        spmm_cheby(A, Tc.win, Tn.win, mode, scalar("float32", A1), scalar("float32", A2),
                   To.win if mode == LC.STEP else None, cp, cc, R.win)
        what = f"srg_spmm_cheby_f32 d={d} {sched} mode={mode} scales={ns} alias={alias}"
        Tn.check(want_t, what + " Tn")
        R.check(want_r, what + " R")
        Tc.check(Tc.host, what + " Tc")


def cheby_step(entry, dtype, sched, Tc, To, Tn, R, d, mode, cp, cc, ns):
    from srgnn import _lib
    ct = ctypes.c_float if dtype == "float32" else ctypes.c_double
    order, n_hub, _ = sched
    ip, ix, v = dev_operator(dtype)
    o = torch.from_numpy(order).cuda()
    arr = lambda a: (ct * len(a))(*a) if a is not None else None    # noqa: E731
    assert Tc.ld == To.ld == Tn.ld == R.ld
    args = [ip.data_ptr(), ix.data_ptr(), v.data_ptr(), int(order.size), o.data_ptr()]
    if entry == "srg_cheby_step_hub_f64":
        args.append(n_hub)
    args += [Tc.win.data_ptr(), To.win.data_ptr(), Tn.win.data_ptr(), Tc.ld, d, mode, scalar(dtype, A1), scalar(dtype, A2),
             arr(cp), arr(cc), ns, R.win.data_ptr(), N * R.ld, _lib.stream(ip.device)]
    _lib.call(ip.device, entry, *args)
    torch.cuda.synchronize()


ALL_MODES = [LC.INIT, LC.STEP, LC.INIT_T, LC.STEP_FIRST, LC.STEP | LC.NO_T]


@pytest.mark.parametrize("d", [5, 64, 130])
def test_cheby_step_f32_random_order(oracle_mod, d):
    """srg_cheby_step_f32 (row waves, one and -- at 130 -- two columns per lane) under a random row_order."""
    s = LC.sched_rand(LC.lengths(), 8, 0, 0, leave_out=64)
    for mode in ALL_MODES:
        Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, "float32", d, mode, 3, rows_of(s))
        cheby_step("srg_cheby_step_f32", "float32", s, Tc, To, Tn, R, d, mode, cp, cc, 3)
        what = f"srg_cheby_step_f32 d={d} mode={mode:#x}"
        Tn.check(want_t, what + " Tn")
        R.check(want_r, what + " R")


def schedule64(name, d):
    """The fp64 steps' schedules: hub rows are workgroups of 16-column slices."""
    lens = LC.lengths()
    n_slices = -(-d // 16)
    if name == "rows":            # srg_cheby_step_f64: every row a row wave, random order
        return LC.sched_rand(lens, 8, 0, 0, leave_out=64)
    if name == "desc":            # the project's: rows longer than a threshold, longest first
        return LC.sched_desc(lens, -1, 1000)
    if name == "asc":             # the shortest non-empty rows as hub rows
        return LC.sched_asc(lens, 40, 0)
    if name == "rand_w512":       # a mixed bag of hub rows, at most 256 workgroups: 512-entry windows
        return LC.sched_rand(lens, 9, max(1, min(60, 256 // n_slices)), 0, leave_out=100)
    if name == "rand_w256":       # more than 256 workgroups: 256-entry windows
        return LC.sched_rand(lens, 10, 256 // n_slices + 300, 0, leave_out=100)
    if name == "all_hub":
        return schedule("all_hub")
    raise KeyError(name)


@pytest.mark.parametrize("sched", ["rows", "desc", "asc", "rand_w512", "rand_w256", "all_hub"])
@pytest.mark.parametrize("d", [2, 5, 16, 20, 64, 130])
def test_cheby_step_f64(oracle_mod, d, sched):
    """srg_cheby_step_f64 (sched = rows) and srg_cheby_step_hub_f64: every mode with 1 and 3 scales
    against oracle.spmm64 plus the numpy fp64 epilogue.  d = 5: odd, so the hub rows run as row waves
    with the same bits; d = 20 / 130: a partial last slice."""
    s = schedule64(sched, d)
    no_empty_hub(s)
    entry = "srg_cheby_step_f64" if sched == "rows" else "srg_cheby_step_hub_f64"
    n_items = s[1] * -(-d // 16)
    if sched == "rand_w512":
        assert 0 < n_items <= 256
    if sched in ("rand_w256", "all_hub"):
        assert n_items > 256
    for mode in ALL_MODES:
        for ns in (1, 3):
            Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, "float64", d, mode, ns, rows_of(s))
            cheby_step(entry, "float64", s, Tc, To, Tn, R, d, mode, cp, cc, ns)
            what = f"{entry} d={d} {sched} mode={mode:#x} scales={ns}"
            Tn.check(want_t, what + " Tn")
            R.check(want_r, what + " R")
            Tc.check(Tc.host, what + " Tc")


@pytest.mark.parametrize("d", [16, 20])
def test_hub64_window_512_every_length(oracle_mod, d):
    """Every non-empty row once through k_cheby_hub64's 512-entry windows (at most 256 workgroups of
    16-column slices per launch)."""
    n_slices = -(-d // 16)
    mode, ns = LC.STEP, 2
    Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, "float64", d, mode, ns, None)
    blank_t, blank_r = Tn.dev.clone(), R.dev.clone()
    wt, wr = (torch.from_numpy(a).cuda().view(torch.int64) for a in (want_t, want_r))
    for i, s in enumerate(LC.w512_sweep(LC.lengths(), n_slices, seed=1)):
        assert 0 < s[1] * n_slices <= 256
        no_empty_hub(s)
        Tn.dev.copy_(blank_t)
        R.dev.copy_(blank_r)
        cheby_step("srg_cheby_step_hub_f64", "float64", s, Tc, To, Tn, R, d, mode, cp, cc, ns)
        if not (torch.equal(Tn.dev.view(torch.int64), wt) and torch.equal(R.dev.view(torch.int64), wr)):
            hub = sorted(LC.lengths()[s[0][:s[1]]].tolist())
            Tn.check(want_t, f"launch {i} Tn, hub rows of lengths {hub}")
            R.check(want_r, f"launch {i} R, hub rows of lengths {hub}")


# ------------------------------------------------------------------------------------------------
# empty rows as hub rows (no schedule of the project's makes one; the C-ABI takes any permutation)
# ------------------------------------------------------------------------------------------------
def empty_hub_schedules():
    lens = LC.lengths()
    n_empty = int((lens == 0).sum())
    asc = LC.sched_asc(lens, n_empty + 50, 0, empty_first=True)
    rnd = LC.sched_rand(lens, 3, 400, 0, empty_hubs=True)
    for s in (asc, rnd):
        assert (lens[s[0][:s[1]]] == 0).any() and (lens[s[0][:s[1]]] > 0).any()
    return {"asc": asc, "rand": rnd}


@pytest.mark.parametrize("sched", ["asc", "rand"])
@pytest.mark.parametrize("d", [32, 100])
def test_empty_hub_rows_f32(oracle_mod, d, sched):
    """A hub workgroup of an empty row stores zeros (or Y's content with ACCUMULATE, and the epilogue's
    value) and ends: its consumer passes no barrier, and its producers leave before theirs."""
    from srgnn.spmm import spmm, spmm_agg
    s = empty_hub_schedules()[sched]
    A = device_csr(s)
    y = product(oracle_mod, "float32", d)
    prev = LC.side_panel("float32", d, 2)
    X = Panel("float32", d, LC.x_panel("float32", d))
    for w256 in (False, True):
        Y = Panel("float32", d)
        spmm(A, X.win, out=Y.win, hub_w256=w256)
        Y.check(Y.expect(y), f"empty hub rows d={d} {sched} w256={w256}")
    Y, G = Panel("float32", d), Panel("float32", d, prev)
    spmm_agg(A, X.win, Y.win, G.win, W_AGG, False)
    Y.check(Y.expect(y), f"empty hub rows, agg: Y d={d} {sched}")
    G.check(G.expect(LC.agg_ref(prev, W_AGG, y)), f"empty hub rows, agg d={d} {sched}")


@pytest.mark.parametrize("sched", ["asc", "rand"])
@pytest.mark.parametrize("d", [16, 64])
def test_empty_hub_rows_f64(oracle_mod, d, sched):
    s = empty_hub_schedules()[sched]
    for mode, ns in ((LC.INIT, 3), (LC.STEP, 1), (LC.STEP_FIRST, 3)):
        Tc, To, Tn, R, want_t, want_r, cp, cc = cheby_case(oracle_mod, "float64", d, mode, ns, None)
        cheby_step("srg_cheby_step_hub_f64", "float64", s, Tc, To, Tn, R, d, mode, cp, cc, ns)
        Tn.check(want_t, f"empty fp64 hub rows d={d} {sched} mode={mode} Tn")
        R.check(want_r, f"empty fp64 hub rows d={d} {sched} mode={mode} R")
