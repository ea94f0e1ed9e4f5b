"""construct_adj on weighted graphs against scipy's own arithmetic (GPU): the numpy-order row sum
(srg_segment_sum_numpy_f64) against the oracle's restatement, which the CPU suite pins to scipy;
the sequential entries on the same ladder; srgnn.construct and the two operators against the cw_*
fixtures (the reference's own Â and hops, tests/golden/make_golden_construct.py)."""
import numpy as np
import pytest
import torch

import construct_cases as CC

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
PAD = 8


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ladder(oracle_mod):
    """The segment ladder plus 4,097 and 20,000, shuffled (a wave gets short and long segments),
    empty segments at both ends; fp64 values, their fp32 cast, and the oracle's sums -- once."""
    ptr, v = CC.ladder("decades", seed=60, extra=(4097, 20000), shuffle=True, empty_ends=True)
    lens = np.diff(ptr)
    assert lens[0] == 0 and lens[-1] == 0 and lens.size % 64 != 0 and lens.size > 256
    v32 = v.astype(np.float32)
    return {"ptr": ptr, "v": v, "v32": v32,
            "numpy": oracle_mod.row_sum_numpy(ptr, v),
            "seq64": oracle_mod.segment_sum(ptr, v), "seq32": oracle_mod.segment_sum(ptr, v32)}


def _windowed(entry, ptr, v, n_seg):
    """entry on the first n_seg segments, out being a window of a sentinel-filled buffer."""
    from srgnn import _lib
    dev = _dev()
    tdt = torch.float64 if v.dtype == np.float64 else torch.float32
    p = torch.from_numpy(ptr[:n_seg + 1].copy()).to(dev)
    vals = torch.from_numpy(v[:int(ptr[n_seg])].copy()).to(dev)
    buf = torch.full((n_seg + 2 * PAD,), SENTINEL, dtype=tdt, device=dev)
    _lib.call(dev, entry, p.data_ptr(), vals.data_ptr() if vals.numel() else None, n_seg,
              buf.data_ptr() + PAD * buf.element_size(), _lib.stream(dev))
    got = buf.cpu().numpy()
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + n_seg:] == SENTINEL).all(), "wrote outside out[0:n_seg]"
    return got[PAD:PAD + n_seg]


@pytest.mark.parametrize("n_seg", [0, 1, 63, 64, 65, None])
def test_numpy_order_row_sum_equals_oracle(ladder, n_seg):
    """a[0] + pairwise(a[1:]) per segment, bit for bit: every length 0..300, the 128-element and
    halving-point boundaries, 4,097 and 20,000 (whole-wave path, several leaf batches)."""
    n = ladder["ptr"].size - 1 if n_seg is None else n_seg
    got = _windowed("srg_segment_sum_numpy_f64", ladder["ptr"], ladder["v"], n)
    bad = np.flatnonzero(CC.bits(got) != CC.bits(ladder["numpy"][:n]))
    assert bad.size == 0, f"segment lengths {np.diff(ladder['ptr'])[bad][:20].tolist()} differ"


@pytest.mark.parametrize("entry,vals,want", [("srg_segment_sum_f64", "v", "seq64"), ("srg_segment_sum_f32", "v32", "seq32")])
@pytest.mark.parametrize("n_seg", [0, 65, None])
def test_sequential_entries_on_the_ladder(ladder, entry, vals, want, n_seg):
    """The left-to-right entries (duplicate merging, the directed families, the wavelet rows) on
    every length of the same ladder, against the sequential oracle."""
    n = ladder["ptr"].size - 1 if n_seg is None else n_seg
    got = _windowed(entry, ladder["ptr"], ladder[vals], n)
    bad = np.flatnonzero(CC.bits(got) != CC.bits(ladder[want][:n]))
    assert bad.size == 0, f"segment lengths {np.diff(ladder['ptr'])[bad][:20].tolist()} differ"


def test_row_sum_device_wrapper(ladder):
    from srgnn.construct import row_sum_device
    dev = _dev()
    got = row_sum_device(torch.from_numpy(ladder["ptr"]).to(dev), torch.from_numpy(ladder["v"]).to(dev))
    assert np.array_equal(CC.bits(got.cpu().numpy()), CC.bits(ladder["numpy"]))
    empty = row_sum_device(torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev))
    assert np.array_equal(CC.bits(empty.cpu().numpy()), CC.bits(np.zeros(3)))


@pytest.fixture(scope="module")
def fixtures():
    return {name: CC.load(name) for name in CC.CW}


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name,variant,kind,r", CC.variants())
def test_device_construct_equals_reference(fixtures, name, variant, kind, r, fast):
    from srgnn import construct as C
    z = fixtures[name]
    args = (z["adj_indptr"], z["adj_indices"], z["adj_data"], z["adj_indptr"].size - 1, r)
    got = (C.sym_norm(*args, device=_dev(), fast=fast) if kind == "sym"
           else C.ppr_norm(*args, 0.15, device=_dev(), fast=fast))
    CC.assert_csr_bits([t.cpu().numpy() for t in got], CC.want_of(z, variant), f"{name} {variant} fast={fast}")


def test_operator_end_to_end_equals_reference(fixtures):
    """SymLaplacianGraphOp(3).propagate on cw_sym: op.adj's fp64 values and the three hops."""
    from operators.graph_operator.symmetrical_simgraph_laplacian_operator import SymLaplacianGraphOp
    z = fixtures["cw_sym"]
    op = SymLaplacianGraphOp(3)
    hops = op.propagate(CC.adj_of(z), z["x"])
    assert op._adj_dev is not None, "Â was not built on the device"
    CC.assert_csr_bits((op.adj.indptr, op.adj.indices, op.adj.data), CC.want_of(z, "sym_r05"), "op.adj")
    for k in (1, 2, 3):
        assert np.array_equal(CC.bits(hops[k].numpy()), CC.bits(z[f"hop{k}"])), f"hop {k}"


@pytest.mark.parametrize("name", CC.CW)
@pytest.mark.parametrize("kind", ["sym", "ppr"])
def test_device_and_host_entries_agree(fixtures, name, kind):
    """construct_adj_device and the host construct_adj (scipy itself) of both operators, and the
    reference's Â, are one matrix."""
    from operators.graph_operator.symmetrical_simgraph_laplacian_operator import SymLaplacianGraphOp
    from operators.graph_operator.symmetrical_simgraph_ppr_operator import PprGraphOp
    z = fixtures[name]
    adj = CC.adj_of(z)
    op = SymLaplacianGraphOp(3) if kind == "sym" else PprGraphOp(3)
    host = op.construct_adj(adj).tocsr()
    host.sort_indices()
    dev = [t.cpu().numpy() for t in op.construct_adj_device(adj, _dev())]
    CC.assert_csr_bits(dev, (host.indptr, host.indices, host.data), f"{name} {kind}: device vs host")
    CC.assert_csr_bits(dev, CC.want_of(z, f"{kind}_r05"), f"{name} {kind}: device vs reference")
