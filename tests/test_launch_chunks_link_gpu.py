"""The edge head's two passes across a chunk boundary at test sizes (see tests/test_launch_chunks_gpu.py):
srg_pair_gather_add_f32 and srg_pair_segment_sum_f32 send their rows out through launch_chunks_capped, each later
chunk with its block_base.  Under srg_debug_launch_cap (srgnn._lib.launch_cap) of 1, 3 and 8 blocks the 1,200 pairs
and the 700 nodes go out in several launches: the results are the unbounded run's bits, which are the restatement's,
in exactly ceil(blocks / bound) launches.  C = 3 packs 16 rows into a wave (64 a block), C = 64 contiguous takes the
16-byte path with 4 rows a wave (16 a block), C = 65 gives a wave one row and two column tiles (4 a block)."""
import functools

import numpy as np
import pytest
import torch

import link_ref as LR

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8)
E, U = 1200, 700
ROWS_PER_BLOCK = {3: 64, 64: 16, 65: 4}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def fixture(C):
    """Host operands and the restatement's results, computed once."""
    rng = np.random.default_rng(300 + C)
    q = rng.integers(0, U, (E, 2))
    q[:50, 0] = 3                                    # one longer segment
    P = rng.standard_normal((U, 2 * C)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    g = rng.standard_normal((E, C)).astype(np.float32)
    inc_ptr, inc_slot = LR.incidence(q, U)
    return q, P, b, g, inc_ptr, inc_slot, LR.gather_add(P, q, b), LR.segment_sum(g, inc_ptr, inc_slot, U)


@pytest.mark.parametrize("entry", ("gather_add", "segment_sum"))
@pytest.mark.parametrize("C", sorted(ROWS_PER_BLOCK))
def test_link_entries_across_chunks(C, entry):
    from srgnn import _lib
    from srgnn import link as LK
    q, P, b, g, inc_ptr, inc_slot, want_out, want_S = fixture(C)
    if entry == "gather_add":
        args, want, rows = (t(P), t(q), t(b)), want_out, E
        run = lambda: LK.pair_gather_add(*args).cpu().numpy()          # noqa: E731
    else:
        args, want, rows = (t(g), t(inc_ptr), t(inc_slot)), want_S, U
        run = lambda: LK.pair_segment_sum(*args).cpu().numpy()         # noqa: E731
    blocks = -(-rows // ROWS_PER_BLOCK[C])
    L = _lib.lib()
    prev = L.srg_debug_launch_cap(0)
    try:
        with _lib.launch_cap(0) as base:
            full = run()
        # the unbounded run is the restatement: what is compared below is not two wrong runs
        assert LR.same_bits(full, want), "the unbounded run against the restatement"
        assert base.launches == 1, base.launches
        for cap in CAPS:
            with _lib.launch_cap(cap) as m:
                got = run()
            assert L.srg_debug_launch_cap(0) == 0
            assert m.launches >= 2 * base.launches, (cap, m.launches, base.launches)
            assert m.launches == -(-blocks // cap), (cap, m.launches, blocks)
            assert LR.same_bits(got, full), f"{entry}, C={C} under a bound of {cap} blocks ({m.launches} launches)"
    finally:
        L.srg_debug_launch_cap(prev)
