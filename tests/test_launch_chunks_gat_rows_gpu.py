"""The row-restricted GAT entries across a chunk boundary at test sizes (see tests/test_launch_chunks_gpu.py):
srg_gat_attend_rows_f32, srg_gat_edge_grad_rows_f32 and srg_gat_attend_rows_adjoint_f32 send their walks out
through launch_chunks_capped in chunks of SRG_GAT_LAUNCH_ROWS rows, each later chunk with its block_base.  Under
srg_debug_launch_cap (srgnn._lib.launch_cap) of 1, 3 and 8 blocks every walk of the 400-row batch, and the
transpose's walks of any batch, go out in several launches: the results are the unbounded run's bits over the
sentinel-guarded buffers, with at least twice its chunk launches."""
import numpy as np
import pytest

import gat_ref as R
import gat_rows_ref as RR

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 8)


@pytest.mark.parametrize("name", ("mixed37", "all"))
@pytest.mark.parametrize("H,C", ((3, 7), (4, 64)))
def test_gat_rows_across_chunks(H, C, name):
    import test_gat_rows_gpu as TG
    from srgnn import _lib
    kind, sl = "sym", True
    g = TG.device_graph(kind, sl)
    x, s_, d_, G = TG.inputs(kind, sl, H, C)
    rows = RR.batch(name, kind, sl)
    Gb = G[TG.t(rows)].contiguous()
    L = _lib.lib()
    prev = L.srg_debug_launch_cap(0)
    try:
        with _lib.launch_cap(0) as base:
            want = TG.Raw(g, rows, x, s_, d_, Gb).run()
        # the unbounded run is the full path's rows: what is compared below is not two wrong runs
        out_f, M_f, Z_f = TG.full_forward(kind, sl, H, C)
        TG.same(want["out"], out_f[TG.t(rows)], "the unbounded run against the full path")
        assert base.launches == 7, base.launches              # stats, gather; row-dot, edge, row sum; adjoint, row sum
        for cap in CAPS:
            with _lib.launch_cap(cap) as m:
                got = TG.Raw(g, rows, x, s_, d_, Gb).run()
            assert L.srg_debug_launch_cap(0) == 0
            assert m.launches >= 2 * base.launches, (cap, m.launches, base.launches)
            for k in want:
                TG.same(got[k], want[k], f"{k} under a bound of {cap} blocks ({m.launches} launches)")
    finally:
        L.srg_debug_launch_cap(prev)
    assert np.isfinite(want["dHf"]).all() and np.abs(want["dHf"]).sum() > 0 and R.N == g.n
