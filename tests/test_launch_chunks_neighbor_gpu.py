"""The sampled row slice across a chunk boundary at test sizes (see tests/test_launch_chunks_gpu.py):
srg_csr_sample_f32 sends its walk out through launch_chunks_capped, each later chunk with its block_base.  Under
srg_debug_launch_cap (srgnn._lib.launch_cap) of 1, 3 and 8 blocks the 400 rows, 25 blocks of 16, go out in several
launches: the results are the unbounded run's bytes over the sentinel-guarded buffers, with at least twice its chunk
launches."""
import pytest

import neighbor_ref as NR

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8)


@pytest.mark.parametrize("fanout", (10, 64, -1))
@pytest.mark.parametrize("name", ("all", "reversed"))
def test_sampler_across_chunks(name, fanout):
    import test_neighbor_gpu as TN
    from srgnn import _lib
    ip, ix, v, sets, A = TN.fixture()
    S = sets[name]
    assert S.size == 400
    seed = NR.SEEDS[1]
    L = _lib.lib()
    prev = L.srg_debug_launch_cap(0)
    try:
        with _lib.launch_cap(0) as base:
            want = TN.raw(A, S, fanout, seed)
        # the unbounded run is the restatement: what is compared below is not two wrong runs
        TN.same(want, TN.want_of(name, fanout, seed), "the unbounded run against the restatement")
        assert base.launches == 1, base.launches
        for cap in CAPS:
            with _lib.launch_cap(cap) as m:
                got = TN.raw(A, S, fanout, seed)
            assert L.srg_debug_launch_cap(0) == 0
            assert m.launches >= 2 * base.launches, (cap, m.launches, base.launches)
            assert m.launches == -(-25 // cap)
            TN.same(got, want, f"{name}, fanout={fanout} under a bound of {cap} blocks ({m.launches} launches)")
    finally:
        L.srg_debug_launch_cap(prev)
