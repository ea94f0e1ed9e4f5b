"""Every chunked launch across a chunk boundary, every clipped grid round its stride loop, at test sizes.

The library sends a large grid out in several launches (launch_chunks_capped, csrc/srg_internal.h) and hands
each later chunk its start in the family's own way: a block_base kernel argument, shifted pointers, an entry
base.  The caps are 2^23 / 2^24 blocks (4M rows for GAT and KNN), so without help a second chunk runs only at
tens of millions of rows.  srg_debug_launch_cap (srgnn._lib.launch_cap) bounds the blocks of one launch: here
every entry runs unbounded and then under a bound of 1 (every block its own launch), 3 (ragged chunks, unaligned
to the 8-block XCD round) and 8 (aligned to it); the widest cases keep 3 only.

Every bounded run is held to the CPU reference the family's own tests use (bits, or gat_ref's bound for GAT,
which then also has the unbounded run's bits), over the whole sentinel-guarded buffer, and must have made at
least twice the chunk launches of the unbounded run (srg_debug_chunk_launches): a bound that changed nothing
fails.  The grid-stride kernels have no counter; their sizes guarantee a second trip (more than 256 c
segments, and so on).  A failure names the bound, the launch counts, the first differing row and, where one
block holds a fixed number of rows, the block and the chunk it falls in.

Where a family's own test module already builds the operands, the guarded buffers and the comparison, that
code runs here under the bound (the modules are imported, their functions called); the references are the
same objects, computed once.

What this cannot reach: the narrowing of a chunk's b0 to int and wave_slot's int arithmetic near 2^31 rows."""
import contextlib
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import construct_cases as CC
import edge_augment_ref as ER
import gat_ref as GR
import graph_conv_ref as GCR
import ladder_cases as LC
import sparse_product_cases as SPC
import wavelet_conv_ref as WR
import wavelet_sparsify_ref as WS
from sddmm_ref import csr_rows, sddmm_ref

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8)
SENT = -12345.0
PAD = 11


def dev():
    return torch.device("cuda", 0)


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype.itemsize == 4 else np.uint64)


def across(run, caps=CAPS, launches=True):
    """run(cap) unbounded (cap None), then under every bound.  run compares with its CPU reference itself;
    launches: a bounded run must make at least twice the chunk launches of the unbounded one."""
    from srgnn import _lib
    with _lib.launch_cap(0) as base:
        run(None)
        torch.cuda.synchronize()
    assert not launches or base.launches >= 1, "the entry made no chunk launch at all"
    for c in caps:
        with _lib.launch_cap(c) as m:
            try:
                run(c)
                torch.cuda.synchronize()
            except AssertionError as e:
                raise AssertionError(f"under a bound of {c} blocks per launch ({m.launches} chunk launches, "
                                     f"{base.launches} unbounded): {e}") from e
        assert _lib.lib().srg_debug_launch_cap(0) == 0, "the bound outlived its block"
        if launches:
            assert m.launches >= 2 * base.launches, \
                f"a bound of {c} made {m.launches} chunk launches, unbounded {base.launches}: no chunk edge was crossed"


@contextlib.contextmanager
def counted(cap, blocks, what):
    """Around one entry whose chunk walks cover `blocks` (the grid of each walk, in blocks): the entry makes
    exactly ceil(b / cap) launches per walk -- one each without a bound -- so every walk of the entry split
    wherever its grid is larger than the bound, and `split` below says which do."""
    from srgnn import _lib
    before = _lib.lib().srg_debug_chunk_launches()
    yield
    made = _lib.lib().srg_debug_chunk_launches() - before
    want = sum(-(-b // cap) if cap else 1 for b in blocks)
    assert made == want, f"{what}: {made} chunk launches for walks of {list(blocks)} blocks under a bound of {cap}, expected {want}"


def split(cap, blocks):
    """Every walk of `blocks` blocks goes out in at least two launches under `cap`."""
    return all(b > cap for b in blocks)


def placing(fn, place):
    """run(cap) for across(): fn(), and a failure that names its first differing row ("first at row N", as
    test_ladder_gpu's Panel.check does) also says where place(N, cap) puts that row: its block and chunk."""
    def run(cap):
        try:
            fn()
        except AssertionError as e:
            m = re.search(r"first at row (\d+)", str(e))
            if m and cap:
                raise AssertionError(f"{e} -- row {m.group(1)} is {place(int(m.group(1)), cap)}") from e
            raise
    return run


def wave_place(sched, hubs=False, rows_per_block=4):
    """place() for kernels that give every scheduled row one wave, four to a block, in the schedule's order
    (k_cheby; hubs: the schedule's hub prefix runs as hub workgroups, which are not chunked)."""
    order, n_hub, _ = sched
    n_hub = n_hub if hubs else 0

    def place(row, cap):
        pos = np.flatnonzero(order == row)
        if not pos.size:
            return "a row the launch does not schedule"
        p = int(pos[0])
        if p < n_hub:
            return f"hub row {p} (hub workgroups are not chunked)"
        b = (p - n_hub) // rows_per_block
        return f"row wave {p - n_hub}: block {b}, chunk {b // cap} (blocks [{b // cap * cap}, {b // cap * cap + cap}))"
    return place


def same(got, want, what, cap=None, rows_per_block=None):
    """Bitwise equality of two arrays whose first axis is the row; names the first differing row and, with
    rows_per_block, its block and chunk under `cap`."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (u32(got), u32(want)) if got.dtype.kind == "f" else (got, want)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        diff = np.where(nan, ~np.isnan(got), g != w)
    else:
        diff = g != w
    if not diff.any():
        return
    rows = np.flatnonzero(diff.reshape(diff.shape[0], -1).any(axis=1))
    r = int(rows[0])
    where = ""
    if rows_per_block:
        b = r // rows_per_block
        where = f", block {b}" + (f", chunk {b // cap} (blocks [{b // cap * cap}, {b // cap * cap + cap}))" if cap else "")
    raise AssertionError(f"{what}: {rows.size} of {diff.shape[0]} rows differ; first row {r}{where}: "
                         f"got {got[r].ravel()[:4]}, want {want[r].ravel()[:4]}")


def guarded(shape, dtype=torch.float32, first=1, extra=3, rows_below=2, fill=SENT):
    """(buffer, window): the window [shape] starts at column `first` of a sentinel-filled buffer `extra` columns
    wider with rows_below more rows (1-D: PAD cells on both sides)."""
    if len(shape) == 1:
        buf = torch.full((shape[0] + 2 * PAD,), fill, dtype=dtype, device=dev())
        return buf, buf[PAD:PAD + shape[0]]
    buf = torch.full((shape[0] + rows_below, shape[1] + extra), fill, dtype=dtype, device=dev())
    return buf, buf[:shape[0], first:first + shape[1]]


def untouched(buf, win_shape, what, first=1, fill=SENT):
    """Every cell of the buffer outside the window still holds the sentinel."""
    h = buf.cpu().numpy()
    if h.ndim == 1:
        ok = (h[:PAD] == fill).all() and (h[PAD + win_shape[0]:] == fill).all()
    else:
        n, d = win_shape
        ok = (h[:n, :first] == fill).all() and (h[:n, first + d:] == fill).all() and (h[n:] == fill).all()
    assert ok, f"{what}: a sentinel outside the window was overwritten"


# ------------------------------------------------------------------------------------------------------
# the SpMM ladder (launch_spmm): block_base, the heavy / light split on block_base + blockIdx.x
# ------------------------------------------------------------------------------------------------------
def ladder_schedule(name):
    """mixed: the project's descending schedule with hub rows (longer than 900), slice-wave rows (longer than
    48) and light rows; rand1: test_ladder_gpu's random one (hub, heavy and light rows in any order, 100 rows
    left unscheduled); light: no hub and no heavy row."""
    import test_ladder_gpu as TL
    lens = LC.lengths()
    if name == "mixed":
        s = LC.sched_desc(lens, 48, 900)
        assert s[1] > 0 and s[2] > 0 and s[1] + s[2] < LC.N
        return s
    return TL.schedule("desc_light" if name == "light" else name)


def ladder_place(d, sched, row, cap):
    """For a failure message: the role of `row` in the schedule and, for a light row of a launch without
    XCD-aware slice waves, its block and chunk (launch_spmm's arithmetic, csrc/srg_spmm_kernels.h)."""
    order, n_hub, n_heavy = sched
    pos = np.flatnonzero(order == row)
    if not pos.size:
        return "a row the launch does not schedule"
    p = int(pos[0])
    if d % 4:
        n_hub = n_heavy = 0
    if p < n_hub:
        return f"hub row {p} (hub workgroups are not chunked)"
    if p < n_hub + n_heavy:
        return f"slice-wave row {p - n_hub} of {n_heavy}"
    lr = {64: 8, 128: 4, 256: 2}.get(d, 0)
    ns = next((w for w in (1, 2, 4, 8, 16, 32) if d <= w), 0) if not lr else 0
    per_block = 4 * (64 // ns if ns else lr if lr else 1)
    light = p - n_hub - n_heavy
    if lr:
        return f"light row {light} (packed, {per_block} rows per block, behind the XCD-rounded heavy blocks)"
    b = -(-(n_heavy * -(-d // 32)) // 4) + light // per_block
    return f"light row {light}: block {b}, chunk {b // cap} of {cap} blocks"


def run_ladder(fn, d, sched, caps):
    across(placing(fn, lambda row, cap: ladder_place(d, sched, row, cap)), caps)


@pytest.mark.parametrize("sched", ["mixed", "rand1", "light"])
@pytest.mark.parametrize("d", [1, 4, 32, 64, 100, 128, 130, 256])
def test_spmm_csr_across_chunks(oracle_mod, d, sched):
    """srg_spmm_csr_f32 at one width per light-row role: narrow rows with 256 rows per block (1) and fewer (4,
    32), packed rows 8 / 4 / 2 per wave beside the XCD-aware slice waves (64 / 128 / 256), row waves unfull (100)
    and two-wide (130).  With hub, heavy and light rows the chunk edges of bounds 1, 3 and 8 fall inside the
    heavy blocks, on the heavy / light boundary and inside the light blocks."""
    import test_ladder_gpu as TL
    s = ladder_schedule(sched)
    caps = (3,) if d in (128, 130, 256) else CAPS
    run_ladder(lambda: TL.run_csr(oracle_mod, d, s, sched), d, s, caps)


@pytest.mark.parametrize("entry", ["agg", "span", "cheby"])
def test_spmm_epilogues_across_chunks(oracle_mod, entry):
    """srg_spmm_agg_f32, srg_spmm_span_f32 and srg_spmm_cheby_f32 (the other instantiations of launch_spmm's
    kernels) at d = 64 under the random schedule: test_ladder_gpu's own cases, run under the bound."""
    import test_ladder_gpu as TL
    fn = {"agg": lambda: TL.test_agg_init_and_add(oracle_mod, 64, "rand1"),
          "span": lambda: TL.test_span_blocks_of_random_cuts(oracle_mod, 64),
          "cheby": lambda: TL.test_spmm_cheby_f32(oracle_mod, 64, "rand1")}[entry]
    run_ladder(fn, 64, TL.schedule("rand1"), CAPS)


# ------------------------------------------------------------------------------------------------------
# the Chebyshev steps: wave_slot(block_base)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 64, 130])
def test_cheby_step_f32_across_chunks(oracle_mod, d):
    """srg_cheby_step_f32, every mode (STEP accumulates into R) with three scales, random row order."""
    import test_ladder_gpu as TL
    s = LC.sched_rand(LC.lengths(), 8, 0, 0, leave_out=64)            # the schedule of TL's case
    across(placing(lambda: TL.test_cheby_step_f32_random_order(oracle_mod, d), wave_place(s)),
           (3,) if d == 130 else CAPS)


@pytest.mark.parametrize("sched", ["rows", "desc"])
@pytest.mark.parametrize("d", [5, 64, 130])
def test_cheby_step_f64_across_chunks(oracle_mod, d, sched):
    """srg_cheby_step_f64 (rows) and srg_cheby_step_hub_f64 on the schedule with hub rows (desc: the rows
    longer than 1000 are hub workgroups, the others row waves), every mode with 1 and 3 scales."""
    import test_ladder_gpu as TL
    s = TL.schedule64(sched, d)
    place = wave_place(s, hubs=sched == "desc" and d % 2 == 0)        # an odd width runs the hub rows as row waves
    across(placing(lambda: TL.test_cheby_step_f64(oracle_mod, d, sched), place), (3,) if d == 130 else CAPS)


def test_planned_fp64_steps_across_chunks(oracle_mod):
    """srg_plan_cheby_step_f64 (k_cheby_blk64: block_base as an int) through a plan of 4 column blocks on the
    3,000-node hub graph under a bound of 3, the plan built under it too (the planner's clipped grids come round
    again): test_wavelet_gpu's own case, bit for bit the oracle's cheby_op.  (A failure names the differing
    elements; the plan orders its launches' rows itself, so no block is named here.)"""
    from srgnn import _lib
    import test_wavelet_gpu as TWV
    with _lib.launch_cap(0) as base:
        TWV.test_heat_filter_f64_column_blocked_bit_exact(oracle_mod, 4, None, None, 64)
    with _lib.launch_cap(3) as m:
        TWV.test_heat_filter_f64_column_blocked_bit_exact(oracle_mod, 4, None, None, 64)
    assert m.launches >= 2 * base.launches >= 2, (m.launches, base.launches)


def test_cheby_epilogue_takes_further_trips(oracle_mod):
    """srg_cheby_epilogue_f32 (a grid clipped at 4,096 blocks of 4 rows, grid-stride) over the ladder's 4,096 rows
    under bounds of 1, 3 and 8: Tn holds A Tc on entry; INIT and STEP with three scales against the numpy
    epilogue, guard columns included."""
    import ctypes
    from srgnn import _lib
    import test_ladder_gpu as TL
    d, ns = 36, 3
    acc = t(TL.product(oracle_mod, "float32", d).copy())      # (the shared reference is read-only)
    arr = lambda a: (ctypes.c_float * len(a))(*a) if a is not None else None    # noqa: E731

    def run(cap):
        for mode in (LC.INIT, LC.STEP):
            Tc, To, Tn, R, want_t, want_r, cp, cc = TL.cheby_case(oracle_mod, "float32", d, mode, ns, None)
            Tn.win.copy_(acc)
            _lib.call(dev(), "srg_cheby_epilogue_f32", Tn.win.data_ptr(), Tn.ld, Tc.win.data_ptr(), Tc.ld,
                      To.win.data_ptr(), To.ld, LC.N, d, mode, TL.scalar("float32", TL.A1), TL.scalar("float32", TL.A2),
                      arr(cp), arr(cc), ns, R.win.data_ptr(), R.ld, LC.N * R.ld, _lib.stream(dev()))
            Tn.check(want_t, f"srg_cheby_epilogue_f32 mode={mode} Tn")
            R.check(want_r, f"srg_cheby_epilogue_f32 mode={mode} R")
            Tc.check(Tc.host, f"srg_cheby_epilogue_f32 mode={mode} Tc")

    def place(row, cap):                                     # the grid is `cap` blocks of 4 row waves, striding
        return f"in block {row // 4 % cap} of {cap}, trip {row // 4 // cap} of its stride loop"
    across(placing(lambda: run(None), place), launches=False)


# ------------------------------------------------------------------------------------------------------
# srg_spmm_muladd_f32: indptr + r0, Y + r0 * ldy
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_rows", [False, True], ids=["stored_order", "sorted"])
def test_spmm_muladd_across_chunks(sorted_rows):
    """37 rows (10 blocks of 4, the last ragged), d = 7 into a window with ldy = 10."""
    from srgnn import sparse as S
    n_rows, d = 37, 7
    A, X = SPC.spmm_case(n_rows, d, sorted_rows)
    want = SPC.spmm_loops(A, X)
    ip, ix, v = t(A.indptr.astype(np.int64)), t(A.indices.astype(np.int32)), t(A.data.astype(np.float32))
    xw = torch.zeros((X.shape[0], d + 5), device=dev())
    xw[:, 2:2 + d] = t(X)

    def run(cap):
        buf, win = guarded((n_rows, d))
        assert win.stride(0) == d + 3
        S.spmm_scatter(ip, ix, v, xw[:, 2:2 + d], out=win)
        same(win.cpu().numpy(), want, "srg_spmm_muladd_f32", cap, 4)
        untouched(buf, (n_rows, d), "srg_spmm_muladd_f32")
    across(run)


# ------------------------------------------------------------------------------------------------------
# srg_sddmm_f32: the entry base b0 * 64
# ------------------------------------------------------------------------------------------------------
def _lengths_csr(lengths, n_cols, seed):
    rng = np.random.default_rng(seed)
    ip = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=ip[1:])
    ix = rng.integers(0, n_cols, int(ip[-1])).astype(np.int32)
    v = (rng.standard_normal(ix.size) * 2).astype(np.float32)
    return ip, ix, v


@pytest.mark.parametrize("aligned", [True, False], ids=["16-byte aligned", "odd offset"])
@pytest.mark.parametrize("with_perm", [False, True])
def test_sddmm_across_chunks(with_perm, aligned):
    """Rows of 0, 1, 63, 64, 65 and 300 entries, three times over: 1,479 entries in 24 tiles of 64, the last
    partial; rows straddle chunk edges and chunks start inside a row.  A 16-byte aligned panel, and a window at
    an odd offset of a wider one (the 4-byte path)."""
    from srgnn.sparse import sddmm
    ip, ix, _ = _lengths_csr([0, 1, 63, 64, 65, 300] * 3, 90, 64)
    m, nnz, d = ip.size - 1, ix.size, 20
    assert nnz % 64 and nnz // 64 + 1 > 2 * max(CAPS)
    first, extra = (4, 8) if aligned else (1, 3)
    rng = np.random.default_rng(2 * d + first)
    Gw = rng.standard_normal((m, d + extra)).astype(np.float32)
    Xw = rng.standard_normal((90, d + extra)).astype(np.float32)
    want = sddmm_ref(csr_rows(ip), ix, Gw[:, first:first + d], Xw[:, first:first + d])
    perm = rng.permutation(nnz)
    tperm = t(perm.astype(np.int64)) if with_perm else None
    tip, tix, tG, tX = t(ip), t(ix), t(Gw)[:, first:first + d], t(Xw)[:, first:first + d]
    assert (tG.data_ptr() % 16 == 0) == aligned

    def run(cap):
        buf, out = guarded((nnz,))
        sddmm(tip, tix, tG, tX, perm=tperm, out=out)
        got = out.cpu().numpy()
        same(got[perm] if with_perm else got, want, "srg_sddmm_f32 (entries in CSR order)", cap, 64)
        untouched(buf, (nnz,), "srg_sddmm_f32")
    across(run)


# ------------------------------------------------------------------------------------------------------
# srg_spmm_scaled_f32: indptr + r0, Y + r0 * ldy, and scale + r0 for the row axis only
# ------------------------------------------------------------------------------------------------------
SCALED_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 257]


@pytest.mark.parametrize("mode", ["none", "col", "row"])
@pytest.mark.parametrize("d", [1, 2, 4, 8, 16, 32, 64, 100])
def test_spmm_scaled_across_chunks(d, mode):
    """Every lane-group width W; 8 blocks and 5 rows more, so the row count is no multiple of the rows per
    block (256 at d = 1 down to 4 past d = 32) and a bound of 8 still makes a second chunk.  Every scale
    entry differs: a column scale that was shifted, or a row scale that was not, shows in every later chunk."""
    from srgnn.wavelet_conv import spmm_scaled
    W = next(w for w in (1, 2, 4, 8, 16, 32, 64) if d <= w or w == 64)
    per_block = 4 * (64 // W)
    n_rows, n_cols = 8 * per_block + 5, 300
    lengths = [SCALED_LENGTHS[r % len(SCALED_LENGTHS)] if r % 64 < 9 else r % 5 for r in range(n_rows)]
    ip, ix, v = _lengths_csr(lengths, n_cols, 100 + d)
    rng = np.random.default_rng(300 + d)
    X = rng.standard_normal((n_cols, d)).astype(np.float32)
    axis = 1 if mode == "row" else 0
    scale = None if mode == "none" else (0.5 + rng.permutation(n_rows if axis else n_cols) / 4096.0).astype(np.float32)
    assert scale is None or np.unique(scale).size == scale.size
    want = WR.spmm_scaled_ref(ip, ix, v, scale, axis, X)
    tip, tix, tv, tX, ts = t(ip), t(ix), t(v), t(X), t(scale)

    def run(cap):
        buf, win = guarded((n_rows, d))
        spmm_scaled(tip, tix, tv, tX, scale=ts, scale_axis=axis, out=win)
        same(win.cpu().numpy(), want, f"srg_spmm_scaled_f32 d={d} {mode}", cap, per_block)
        untouched(buf, (n_rows, d), "srg_spmm_scaled_f32")
    across(run)


# ------------------------------------------------------------------------------------------------------
# srg_sddmm_rowsum_f32: indptr + r0, P + r0 * ldp, out + r0 (a row per block)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 16, 33])
def test_sddmm_rowsum_across_chunks(d):
    from srgnn.wavelet_conv import sddmm_rowsum
    n_rows, n_cols = 50, 300
    ip, ix, v = _lengths_csr([(0, 1, 64, 65, 3)[r % 5] for r in range(n_rows)], n_cols, 50 + d)
    rng = np.random.default_rng(500 + d)
    Gw = rng.standard_normal((n_cols, d + 3)).astype(np.float32)
    Pw = rng.standard_normal((n_rows, d + 3)).astype(np.float32)
    want = WR.sddmm_rowsum_ref(ip, ix, v, Gw[:, 1:1 + d], Pw[:, 1:1 + d])
    tip, tix, tv, tG, tP = t(ip), t(ix), t(v), t(Gw)[:, 1:1 + d], t(Pw)[:, 1:1 + d]

    def run(cap):
        buf, out = guarded((n_rows,))
        sddmm_rowsum(tip, tix, tv, tG, tP, out=out)
        same(out.cpu().numpy(), want, f"srg_sddmm_rowsum_f32 d={d}", cap, 1)
        untouched(buf, (n_rows,), "srg_sddmm_rowsum_f32")
    across(run)


# ------------------------------------------------------------------------------------------------------
# srg_gconv_rows_f32 / srg_gconv_rows_adjoint_f32: wave_slot(block_base)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 48])
def test_gconv_rows_across_chunks(d):
    """The star graph (400 rows, one of 320 entries, two empty): a batch of 67 shuffled rows (17 blocks of 4
    waves, the last with three) forward, all 400 rows of the transpose in the adjoint."""
    from srgnn import graph_conv as GC
    from srgnn.csr import DeviceCSR
    ip, ix, v = GCR.star_graph()
    n = ip.size - 1
    tp, tx, tv = GCR.transpose_stable(ip, ix, v, n)
    A = DeviceCSR.from_tensors(ip, ix, v, n_cols=n, device=dev())
    At = DeviceCSR.from_tensors(tp, tx, tv, n_cols=n, device=dev())
    rng = np.random.default_rng(d)
    rows = np.r_[7, 3, np.setdiff1d(rng.permutation(n)[:70], (7, 3))[:65]].astype(np.int64)
    B = rows.size
    assert B == 67 and B % 4
    X = rng.standard_normal((n, d)).astype(np.float32)
    G = rng.standard_normal((B, d)).astype(np.float32)
    want_y = GCR.rows_forward_ref(ip, ix, v, rows, X)
    pos = GCR.pos_of(rows, n)
    want_dx = GCR.rows_adjoint_ref(tp, tx, tv, pos, G)
    tX, tG, trows, tpos = t(X), t(G), t(rows), t(pos)
    assert all(split(c, [-(-B // 4), n // 4]) for c in CAPS)

    def run(cap):
        buf, win = guarded((B, d))
        with counted(cap, [-(-B // 4)], "srg_gconv_rows_f32"):
            GC.rows_product(A, tX, trows, out=win)
        same(win.cpu().numpy(), want_y, f"srg_gconv_rows_f32 d={d}", cap, 4)
        untouched(buf, (B, d), "srg_gconv_rows_f32")
        buf, win = guarded((n, d))
        with counted(cap, [n // 4], "srg_gconv_rows_adjoint_f32"):
            GC.rows_adjoint(At, tpos, tG, out=win)
        same(win.cpu().numpy(), want_dx, f"srg_gconv_rows_adjoint_f32 d={d}", cap, 4)
        untouched(buf, (n, d), "srg_gconv_rows_adjoint_f32")
    across(run)


# ------------------------------------------------------------------------------------------------------
# the sparsify utilities: an int64 block_base
# ------------------------------------------------------------------------------------------------------
def test_dense_sparsify_across_chunks():
    """70 rows x 129 columns (18 blocks of 4 row waves), both phases, guard words behind every output."""
    import test_wavelet_sparsify_gpu as TW
    n, w = 70, 129
    block = WS.planted_block(n, w, seed=70)
    want_cnt, _, want_idx, want_val = WS.sparsify_block(block, 1e-4, 1000)
    want_ptr = np.r_[0, np.cumsum(want_cnt)]

    def run(cap):
        for ldr, offset in ((w, 0), (w + 3, 1)):
            with counted(cap, [18, 18], "srg_dense_sparsify_f64, count and fill"):
                cnt, idx, val = TW._sparsify(TW._window(block, ldr, offset), 1e-4, 1000)
            same(cnt, want_cnt, "srg_dense_sparsify_f64 phase 0 (counts)", cap, 4)
            rows = np.repeat(np.arange(n), want_cnt)
            bad = np.flatnonzero((idx != want_idx) | (u32(val) != u32(want_val)))
            assert bad.size == 0, (f"srg_dense_sparsify_f64 phase 1: entries of row {rows[bad[0]]} (block "
                                   f"{rows[bad[0]] // 4}) differ, {bad.size} of {want_ptr[-1]} entries")
    across(run)


def test_csr_append_rows_across_chunks():
    """Three block-local CSRs over 130 rows (9 blocks of 16 rows, so that a bound of 8 still makes a second
    chunk), among them a row of 200 entries (the whole-wave copy) and empty rows == sp.hstack(blocks).tocsr();
    the cursor ends at indptr[1:]."""
    from srgnn import _lib
    import test_wavelet_sparsify_gpu as TW
    n = 130
    rng = np.random.default_rng(70)
    counts = [[(0, 3, 1, 17, 2, 64, 0, 5, 65, 33)[(r + 3 * b) % 10] for r in range(n)] for b in range(3)]
    counts[2][38] = 200
    blocks = [TW._random_rows(rng, c, 300) for c in counts]
    want = sp.hstack(blocks).tocsr()
    indptr = t(want.indptr.astype(np.int64))
    dev_blocks = [(t(m.indptr.astype(np.int64)), t((m.indices + 300 * b).astype(np.int32)), t(m.data))
                  for b, m in enumerate(blocks)]
    entry_row = np.repeat(np.arange(n), np.diff(want.indptr))

    def run(cap):
        cursor = indptr[:-1].clone()
        indices = torch.full((want.nnz + 64,), -7, dtype=torch.int32, device=dev())
        values = torch.full((want.nnz + 64,), -7.0, dtype=torch.float32, device=dev())
        for ptr, idx, val in dev_blocks:
            with counted(cap, [9], "srg_csr_append_rows_f32"):
                _lib.call(dev(), "srg_csr_append_rows_f32", ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), n,
                          cursor.data_ptr(), indices.data_ptr(), values.data_ptr(), _lib.stream(dev()))
        gi, gv = indices.cpu().numpy(), values.cpu().numpy()
        bad = np.flatnonzero((gi[:want.nnz] != want.indices) | (u32(gv[:want.nnz]) != u32(want.data)))
        assert bad.size == 0, (f"srg_csr_append_rows_f32: entries of row {entry_row[bad[0]]} (block "
                               f"{entry_row[bad[0]] // 16}) differ, {bad.size} of {want.nnz} entries")
        assert torch.equal(cursor, indptr[1:]), "the cursor does not stand at indptr[1:]"
        assert (gi[want.nnz:] == -7).all() and (gv[want.nnz:] == -7.0).all(), "wrote past nnz"
    across(run)


def test_csr_row_normalize_l1_across_chunks():
    """One block normalises 256 rows, so 2,100 rows (9 blocks) for a second chunk under a bound of 8: short
    rows, an empty row, a row of zeros and whole-wave rows of 70 and 300 entries in every block."""
    from srgnn import _lib
    n = 2100
    rng = np.random.default_rng(21)
    lens = np.array([(3, 0, 1, 64, 65, 10, 7)[r % 7] for r in range(n)], dtype=np.int64)
    lens[5::256] = 300
    lens[77::256] = 70
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    data = (rng.random(int(indptr[-1])) * 3 - 1).astype(np.float32)
    data[indptr[10]:indptr[11]] = 0.0                        # a row of explicit zeros stays as it is
    want = WS.l1_normalize(indptr, data)
    tip = t(indptr)
    entry_row = np.repeat(np.arange(n), lens)

    def run(cap):
        v = torch.cat([t(data), torch.full((64,), -7.0, device=dev())])
        with counted(cap, [9], "srg_csr_row_normalize_l1_f32"):
            _lib.call(dev(), "srg_csr_row_normalize_l1_f32", tip.data_ptr(), v.data_ptr(), n, _lib.stream(dev()))
        got = v.cpu().numpy()
        bad = np.flatnonzero(u32(got[:data.size]) != u32(want))
        assert bad.size == 0, (f"srg_csr_row_normalize_l1_f32: row {entry_row[bad[0]]} (block "
                               f"{entry_row[bad[0]] // 256}) differs, {bad.size} entries")
        assert (got[data.size:] == -7.0).all(), "wrote past the values"
    across(run)


def _mid_graph(n=800, seed=8):
    rng = np.random.default_rng(seed)
    m = np.triu(rng.random((n, n)) < 0.01, 1)
    return sp.csr_matrix((m + m.T).astype(float))


@pytest.mark.parametrize("gname,batch", [("small", 25), ("mid800", 400)])
def test_wavelet_basis_device_under_a_bound(gname, batch):
    """End to end: wavelet_basis_device under a bound of 3 returns the host-assembled wavelet_basis's bits, with
    at least twice the chunk launches.  Every column block sparsifies, appends and the basis is normalised over
    all n rows.  small (60 rows): 15 blocks to sparsify and 4 to append split, the one block that normalises
    cannot.  mid800 (a random symmetric graph of 800 nodes): 200, 50 and 4 blocks -- all three walks split."""
    from srgnn import _lib
    from srgnn.wavelet import wavelet_basis, wavelet_basis_device
    import test_wavelet_sparsify_gpu as TW
    a = TW._graphs()["small"] if gname == "small" else _mid_graph()
    n = a.shape[0]
    assert split(3, [-(-n // 4), -(-n // 16)]) and split(3, [-(-n // 256)]) == (gname == "mid800")
    kw = dict(scale=0.5, order=3, tolerance=1e-4, batch=batch, device="cuda")
    want = wavelet_basis(a, **kw)
    with _lib.launch_cap(0) as base:
        wavelet_basis_device(a, **kw)
    with _lib.launch_cap(3) as m:
        got = wavelet_basis_device(a, **kw)
    assert got[2] == want[2]
    TW._same_csr(got[0].to_scipy(), want[0])
    TW._same_csr(got[1].to_scipy(), want[1])
    assert m.launches >= 2 * base.launches >= 2, (m.launches, base.launches)


# ------------------------------------------------------------------------------------------------------
# GAT and KNN: general data past a chunk edge (their own past-the-cap tests use H = C = 1, exact integers)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", ((3, 7), (4, 64)))
def test_gat_across_chunks(H, C):
    """The symmetric base graph with self-loops (400 rows: 100 blocks of 4 row waves; the row-dot kernel takes
    n H items, 256 to a block: 5 or 7 blocks, which a bound of 8 holds in one launch), forward and backward.
    Through autograd: within gat_ref's bound of the fp64 restatement, and the unbounded run's bits.  Then the
    three entries on raw pointers, every output (out, M, Z; D, dS, da_dst; dHf, da_src) a window of a sentinel
    buffer: the same bits, gat_ref's bound again, the sentinels untouched, and per entry exactly the launches
    its walks make under the bound.  (4, 64) is the wide case: a bound of 3 only."""
    import test_gat_gpu as TG
    from srgnn import _lib
    kind, sl = "sym", True
    ip, ix, (Hf, a_src, a_dst, G), ref = TG.reference(kind, sl, H, C)
    g = TG.device_graph(kind, sl)
    args = (t(Hf), t(a_src), t(a_dst), t(G))
    x, s_, d_, g_ = args
    n, nnz, W = GR.N, ix.size, H * C
    tip, tix = t(ip), t(ix)
    rows, dot = n // 4, -(-(n * H) // 256)
    caps = CAPS if C == 7 else (3,)
    assert all(split(c, [rows]) for c in caps) and split(3, [dot]) and not split(8, [dot])
    first = {}

    def run(cap):
        got = TG.run(g, *args)
        GR.check(f"GAT H={H} C={C}", ref, got)
        if cap is None:
            first.update(got)
        for k in got:
            same(got[k], first[k], f"GAT {k} against the unbounded run", cap, 4)
        st = _lib.stream(dev())
        ob, out = guarded((n, W), first=4, extra=8)
        mb, M = guarded((n * H,))
        zb, Z = guarded((n * H,))
        with counted(cap, [rows, rows], "srg_gat_attend_f32"):
            _lib.call(dev(), "srg_gat_attend_f32", tip.data_ptr(), tix.data_ptr(), nnz, n, n, s_.data_ptr(),
                      d_.data_ptr(), 0.2, x.data_ptr(), W, H, C, out.data_ptr(), out.stride(0), M.data_ptr(),
                      Z.data_ptr(), st)
        Db, D = guarded((n * H,))
        sb, dS = guarded((nnz * H,))
        ab, da_dst = guarded((n * H,))
        with counted(cap, [dot, rows, rows], "srg_gat_edge_grad_f32"):
            _lib.call(dev(), "srg_gat_edge_grad_f32", tip.data_ptr(), tix.data_ptr(), nnz, n, n, s_.data_ptr(),
                      d_.data_ptr(), 0.2, x.data_ptr(), W, H, C, out.data_ptr(), out.stride(0), M.data_ptr(), Z.data_ptr(),
                      g_.data_ptr(), W, D.data_ptr(), dS.data_ptr(), da_dst.data_ptr(), st)
        hb, dHf = guarded((n, W), first=4, extra=8)
        cb, da_src = guarded((n * H,))
        with counted(cap, [rows, rows], "srg_gat_attend_adjoint_f32"):
            _lib.call(dev(), "srg_gat_attend_adjoint_f32", g.indptr_t.data_ptr(), g.indices_t.data_ptr(), g.perm.data_ptr(),
                      nnz, n, n, s_.data_ptr(), d_.data_ptr(), 0.2, H, C, M.data_ptr(), Z.data_ptr(), g_.data_ptr(), W,
                      dS.data_ptr(), dHf.data_ptr(), dHf.stride(0), da_src.data_ptr(), st)
        raw = {"out": (ob, out, (n, W)), "M": (mb, M, (n, H)), "Z": (zb, Z, (n, H)), "D": (Db, D, (n, H)),
               "dS": (sb, dS, (nnz, H)), "da_dst": (ab, da_dst, (n, H)), "dHf": (hb, dHf, (n, W)),
               "da_src": (cb, da_src, (n, H))}
        host = {k: win.cpu().numpy().reshape(shape) for k, (_, win, shape) in raw.items()}
        if cap is None:
            first.update(D=host["D"], dS=host["dS"])
        GR.check(f"GAT H={H} C={C} on raw pointers", ref, {k: host[k] for k in GR.FORWARD + GR.BACKWARD})
        assert GR.worst_ratio(host["dS"], ref["ds"], ref["E_ds"]) <= 1.0, "dS outside gat_ref's bound"
        for k, (buf, win, shape) in raw.items():
            per_block = None if k == "dS" else 4              # (dS: a row per entry of A)
            same(host[k], first[k], f"GAT {k} on raw pointers against the unbounded run", cap, per_block)
            untouched(buf, (shape[0] * shape[1],) if buf.dim() == 1 else shape, f"GAT {k} on raw pointers", first=4)
    across(run, caps)


def test_knn_across_chunks():
    """srg_sample_distinct_i64 and srg_knn_select_f32 on 300 ragged rows (75 blocks of 4 waves; the argument
    check's grid-stride loop takes a second trip under a bound of 1): ids and distance bits exact."""
    from srgnn import _lib
    import test_edge_augment_gpu as TE
    rng = np.random.default_rng(300)
    n, d, rows = 400, 7, 300
    X, query, cand_ptr, cand, out_ptr = TE.ragged_problem(rng, n, d, rows)
    want_sel, want_bits = ER.select(X, query, cand_ptr, cand, out_ptr)
    draw_ptr = TE.ptr_of([(r * 7) % 90 for r in range(rows)])
    want_draw = ER.sample_distinct(query, draw_ptr, n, 99)
    tX, tq, tcp, tc, top, tdp = t(X), t(query), t(cand_ptr), t(cand), t(out_ptr), t(draw_ptr)
    row_of_out = np.repeat(np.arange(rows), np.diff(out_ptr))
    row_of_draw = np.repeat(np.arange(rows), np.diff(draw_ptr))
    st = _lib.stream(dev())

    def run(cap):
        k = int(out_ptr[-1])
        sb, sel = guarded((k,), dtype=torch.int64, fill=-7)
        db, dist = guarded((k,))
        with counted(cap, [rows // 4], "srg_knn_select_f32"):
            _lib.call(dev(), "srg_knn_select_f32", tX.data_ptr(), d, n, d, tq.data_ptr(), tcp.data_ptr(), tc.data_ptr(),
                      top.data_ptr(), rows, sel.data_ptr(), dist.data_ptr(), st)
        gs, gb = sel.cpu().numpy(), dist.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((gs != want_sel) | (gb != want_bits))
        assert bad.size == 0, f"srg_knn_select_f32: row {row_of_out[bad[0]]} (block {row_of_out[bad[0]] // 4}) differs"
        untouched(sb, (k,), "srg_knn_select_f32 sel", fill=-7)
        untouched(db, (k,), "srg_knn_select_f32 dist")
        m = int(draw_ptr[-1])
        cb, drawn = guarded((m,), dtype=torch.int64, fill=-7)
        with counted(cap, [rows // 4], "srg_sample_distinct_i64"):
            _lib.call(dev(), "srg_sample_distinct_i64", tq.data_ptr(), tdp.data_ptr(), rows, n, 99, drawn.data_ptr(), st)
        bad = np.flatnonzero(drawn.cpu().numpy() != want_draw)
        assert bad.size == 0, f"srg_sample_distinct_i64: row {row_of_draw[bad[0]]} (block {row_of_draw[bad[0]] // 4}) differs"
        untouched(cb, (m,), "srg_sample_distinct_i64", fill=-7)
    across(run)


# ------------------------------------------------------------------------------------------------------
# the grid-stride kernels of srg_csr.hip: a bound clips the grid, the stride loop takes further trips
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,vals,oracle", [("srg_segment_sum_numpy_f64", np.float64, "row_sum_numpy"),
                                               ("srg_segment_sum_f64", np.float64, "segment_sum"),
                                               ("srg_segment_sum_f32", np.float32, "segment_sum")])
def test_segment_sums_take_a_second_trip(oracle_mod, entry, vals, oracle):
    """test_construct_scipy_gpu's ladder: more than 256 shuffled segments, so under a bound of 1 (one block:
    four waves of 64 segments) every wave comes round again, short and whole-wave segments in both trips."""
    import test_construct_scipy_gpu as TC
    ptr, v = CC.ladder("decades", seed=60, extra=(4097, 20000), shuffle=True, empty_ends=True)
    v = v.astype(vals)
    n = ptr.size - 1
    lens = np.diff(ptr)
    assert n > 256 and (lens[256:] > 128).any() and (lens[:256] > 128).any()
    want = getattr(oracle_mod, oracle)(ptr, v)

    def run(cap):
        got = TC._windowed(entry, ptr, v, n)
        bad = np.flatnonzero(CC.bits(got) != CC.bits(want))
        assert bad.size == 0, (f"{entry}: segment {bad[0]} (trip {bad[0] // 256 if cap == 1 else 0}, length "
                               f"{lens[bad[0]]}) differs; {bad.size} segments in all")
    across(run, (1,), launches=False)


def _symmetric_graph(n, seed):
    rng = np.random.default_rng(seed)
    m = np.triu(rng.random((n, n)) < 0.05, 1)
    a = sp.csr_matrix((m + m.T).astype(np.float32))
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int32)


def test_csr_mirror_and_copy_spans_take_a_second_trip():
    """A symmetric 300-node graph (about 4,400 entries: 18 blocks of 256 for the mirror, 19 blocks of 16 rows
    for the span copy) against numpy: mirror[e] of entry (r, c) is the position of (c, r); the spans of a
    shuffled row order copied to their new positions."""
    from srgnn import _lib
    n = 300
    ip, ix = _symmetric_graph(n, 3)
    nnz = ix.size
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
    assert nnz > 256 * 8
    key = rows * n + ix
    want_mirror = np.searchsorted(key, ix.astype(np.int64) * n + rows)
    assert np.array_equal(key[want_mirror], ix.astype(np.int64) * n + rows)
    rng = np.random.default_rng(4)
    order = rng.permutation(n)[:n - 7].astype(np.int32)            # seven rows are not copied
    v = rng.standard_normal(nnz).astype(np.float32)
    lens = np.diff(ip)[order]
    pos = np.r_[0, np.cumsum(lens)][:-1].astype(np.int64)
    want_ix = np.concatenate([ix[ip[r]:ip[r + 1]] for r in order])
    want_v = np.concatenate([v[ip[r]:ip[r + 1]] for r in order])
    want_beg = np.full(n, -7, np.int64)
    want_end = np.full(n, -7, np.int64)
    want_beg[order], want_end[order] = pos, pos + lens
    tip, tix, trows, tv, torder, tpos = t(ip), t(ix), t(rows), t(v), t(order), t(pos)
    beg, end = tip[:-1].contiguous(), tip[1:].contiguous()
    st = _lib.stream(dev())

    def run(cap):
        mb, mirror = guarded((nnz,), dtype=torch.int64, fill=-7)
        _lib.call(dev(), "srg_csr_mirror", tip.data_ptr(), tix.data_ptr(), trows.data_ptr(), n, nnz, mirror.data_ptr(), st)
        same(mirror.cpu().numpy(), want_mirror, "srg_csr_mirror (by entry)", cap, 256)
        untouched(mb, (nnz,), "srg_csr_mirror", fill=-7)
        k = int(lens.sum())
        ib, oix = guarded((k,), dtype=torch.int32, fill=-7)
        vb, ov = guarded((k,))
        obeg = torch.full((n,), -7, dtype=torch.int64, device=dev())
        oend = torch.full((n,), -7, dtype=torch.int64, device=dev())
        _lib.call(dev(), "srg_csr_copy_spans", torder.data_ptr(), order.size, beg.data_ptr(), end.data_ptr(), tix.data_ptr(),
                  tv.data_ptr(), tpos.data_ptr(), oix.data_ptr(), ov.data_ptr(), obeg.data_ptr(), oend.data_ptr(), st)
        same(oix.cpu().numpy(), want_ix, "srg_csr_copy_spans indices (by entry)")
        same(ov.cpu().numpy(), want_v, "srg_csr_copy_spans values (by entry)")
        same(obeg.cpu().numpy(), want_beg, "srg_csr_copy_spans out_beg")
        same(oend.cpu().numpy(), want_end, "srg_csr_copy_spans out_end")
        untouched(ib, (k,), "srg_csr_copy_spans indices", fill=-7)
        untouched(vb, (k,), "srg_csr_copy_spans values")
    across(run, launches=False)


def test_spmm_csr_f64_takes_a_second_trip(oracle_mod):
    """The fp64 product over the first 700 rows of the ladder operator at d = 5: 3,500 elements, 14 blocks."""
    from srgnn import _lib
    n, d = 700, 5
    ip, ix, v = LC.operator("float64")
    ip, ix, v = ip[:n + 1].copy(), ix[:ip[n]].copy(), v[:ip[n]].copy()
    X = LC.x_panel("float64", d)
    want = oracle_mod.spmm64(ip, ix, v, X)
    assert n * d > 256 * 8
    tip, tix, tv, tX = t(ip), t(ix), t(v), t(X)

    def run(cap):
        buf, win = guarded((n, d), dtype=torch.float64)
        _lib.call(dev(), "srg_spmm_csr_f64", tip.data_ptr(), tix.data_ptr(), tv.data_ptr(), n, tX.data_ptr(), d,
                  win.data_ptr(), win.stride(0), d, _lib.stream(dev()))
        same(win.cpu().numpy(), want, "srg_spmm_csr_f64", cap)
        untouched(buf, (n, d), "srg_spmm_csr_f64")
    across(run, launches=False)


def test_csr_validate_reports_a_bad_id_in_the_second_trip():
    """Under a bound of 1 the first trip checks entries [0, 256): a column id out of range at entry 1,000, and a
    decreasing indptr at row 280, are found in later trips; the clean operator passes."""
    from srgnn import _lib
    n = 300
    ip, ix = _symmetric_graph(n, 3)
    bad = ix.copy()
    bad[1000] = n
    bad_ip = ip.copy()
    bad_ip[280] = bad_ip[279] - 1
    tip, tix, tbad, tbad_ip = t(ip), t(ix), t(bad), t(bad_ip)
    st = _lib.stream(dev())
    for cap in (0, 1, 3):
        with _lib.launch_cap(cap):
            _lib.call(dev(), "srg_csr_validate", tip.data_ptr(), tix.data_ptr(), n, ix.size, n, st)
            with pytest.raises(_lib.SrgError, match="column id"):
                _lib.call(dev(), "srg_csr_validate", tip.data_ptr(), tbad.data_ptr(), n, ix.size, n, st)
            with pytest.raises(_lib.SrgError, match="indptr decreases"):
                _lib.call(dev(), "srg_csr_validate", tbad_ip.data_ptr(), tix.data_ptr(), n, ix.size, n, st)
    _lib.lib().srg_clear_error()


# ------------------------------------------------------------------------------------------------------
# end to end, and the default path
# ------------------------------------------------------------------------------------------------------
def test_propagate_end_to_end_under_a_bound():
    """SymLaplacianGraphOp(3).propagate on the Cora fixture under a bound of 3 -- construct_adj on the device,
    the plan's build and its hops -- returns the reference's hop bits."""
    import golden_cases as G
    from operators.graph_operator.symmetrical_simgraph_laplacian_operator import SymLaplacianGraphOp
    from srgnn import _lib
    c = G.Case("cora_sym_k3")
    x = c.x()
    with _lib.launch_cap(0) as base:
        SymLaplacianGraphOp(c.k, r=c.meta["r"]).propagate(c.adj(), x)
    with _lib.launch_cap(3) as m:
        op = SymLaplacianGraphOp(c.k, r=c.meta["r"])
        out = op.propagate(c.adj(), x)
    np.testing.assert_array_equal(op.adj.data, c["ahat_data64"])
    for k in range(1, c.k + 1):
        c.check_hop(k, out[k].numpy())
    assert m.launches >= 2 * base.launches >= 2, (m.launches, base.launches)


def test_the_default_path_issues_one_launch_per_kernel():
    """Without a bound the walk changes nothing: K hops of a planned propagate make K times the plan's launches
    through the chunk walk, one each, and the hook reports and restores the bound it replaces."""
    from srgnn import _lib, synth
    from srgnn.csr import DeviceCSR
    from srgnn.normalize import sym_norm_binary
    from srgnn.plan import cached
    from srgnn.spmm import propagate
    L = _lib.lib()
    assert L.srg_debug_launch_cap(0) == 0
    n, e, d, K = 5000, 40000, 128, 3
    u, v = synth.rmat_undirected_t(n, e, seed=synth.RMAT_SEED, device=dev())
    ip, ix = synth.symmetric_csr_t(n, u, v)
    ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
    x = synth.uniform_features_t(n, d, device=dev())
    A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev())
    propagate(A, x, K)                                       # builds and caches the plan
    P = cached(A, d)
    before = L.srg_debug_chunk_launches()
    hops = propagate(A, x, K)
    torch.cuda.synchronize()
    made = L.srg_debug_chunk_launches() - before
    # (a launch of whole hub rows alone runs hub workgroups on the side stream, which are not chunked)
    assert made == K * P.spmm_launches, f"{made} chunk launches for {K} hops of {P.spmm_launches} SpMM launch(es)"
    with _lib.launch_cap(5) as outer:
        with _lib.launch_cap(2):
            assert L.srg_debug_launch_cap(2) == 2
        assert L.srg_debug_launch_cap(5) == 5
        with pytest.raises(RuntimeError), _lib.launch_cap(1):
            raise RuntimeError("leaves the block by an exception")
        assert L.srg_debug_launch_cap(5) == 5
        again = propagate(A, x, K)
        torch.cuda.synchronize()
    assert L.srg_debug_launch_cap(0) == 0 and outer.launches >= 2 * K * P.spmm_launches
    for k in range(1, K + 1):
        assert torch.equal(again[k].view(torch.int32), hops[k].view(torch.int32)), f"hop {k} under a bound"
