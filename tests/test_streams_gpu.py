"""Streams, devices and host threads around the C-ABI (device guard, per-stream hub
fork/join events, overlapping row strides).  Results must stay bit-identical to the oracle."""
import threading

import numpy as np
import pytest
import torch

import golden_cases as G

pytestmark = pytest.mark.gpu


def _hub_csr(c):
    from srgnn.csr import DeviceCSR
    ip, ix, v = c.ahat()
    A = DeviceCSR.from_tensors(ip, ix, v, n_cols=c.n, heavy_threshold=2, hub_threshold=8, device="cuda")
    assert A.n_hub > 0 and A.n_heavy > 0
    return A


def test_spmm_on_a_side_torch_stream_bit_exact(oracle_mod):
    """A non-default caller stream: the library resolves its device from the stream and forks the
    hub rows from THAT stream (its own side stream and events)."""
    from srgnn.spmm import propagate, spmm
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    X = torch.from_numpy(x).cuda()
    want = oracle_mod.propagate(*c.ahat(), x, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hops = propagate(A, X, 3)
        y = spmm(A, X)
    s.synchronize()
    for k in (1, 2, 3):
        np.testing.assert_array_equal(hops[k].cpu().numpy(), want[k])
    np.testing.assert_array_equal(y.cpu().numpy(), want[1])


def test_hub_nojoin_then_join_per_stream(oracle_mod):
    """SRG_SPMM_HUB_NOJOIN on two caller streams in turn: each srg_hub_join waits on its own
    stream's hub launch."""
    from srgnn import _lib
    from srgnn.spmm import spmm
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    X = torch.from_numpy(x).cuda()
    want = oracle_mod.spmm(*c.ahat(), x)
    outs = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        with torch.cuda.stream(s):
            outs.append(spmm(A, X, hub_nojoin=True))
    for s in streams:
        with torch.cuda.stream(s):
            _lib.call(X.device, "srg_hub_join", _lib.stream(X.device))
            outs.append(outs.pop(0).clone())      # read after the join, on the same stream
    torch.cuda.synchronize()
    for y in outs:
        np.testing.assert_array_equal(y.cpu().numpy(), want)


def _join(device):
    from srgnn import _lib
    _lib.call(device, "srg_hub_join", _lib.stream(device))


def test_hub_join_with_nothing_forked(oracle_mod):
    """srg_hub_join on a stream that never forked: SRG_OK, no side stream made for it, and the stream's
    next hop is the oracle's."""
    from srgnn import _lib
    from srgnn.spmm import spmm
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    X = torch.from_numpy(x).cuda()
    want = oracle_mod.spmm(*c.ahat(), x)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        before = _lib.query("srg_hub_side_streams")
        assert _lib.lib().srg_hub_join(_lib.stream(X.device)) == _lib.SRG_OK
        assert _lib.query("srg_hub_side_streams") == before
        y = spmm(A, X)
    s.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_hub_pending_then_joined_launch_on_one_stream(oracle_mod):
    """An unjoined fork, then a launch that joins its own fork, then srg_hub_join, all on one stream:
    the side stream runs in order, so either join covers the first launch's hub rows too."""
    from srgnn.spmm import spmm
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    X = torch.from_numpy(x).cuda()
    want = oracle_mod.spmm(*c.ahat(), x)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y0 = spmm(A, X, hub_nojoin=True)
        y1 = spmm(A, X)
        _join(X.device)
        outs = [y0.clone(), y1.clone()]       # read after the join, on the same stream
    s.synchronize()
    for y in outs:
        np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_hub_continue_without_and_with_a_pending_fork(oracle_mod):
    """SRG_SPMM_HUB_CONTINUE with nothing pending is a real fork; a second such launch before the join
    is the true continue (appended to the side stream, no new fork)."""
    from srgnn.spmm import spmm
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    X = torch.from_numpy(x).cuda()
    want = oracle_mod.spmm(*c.ahat(), x)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # the outputs exist before the first fork: a continued launch's hub rows are ordered after that fork only
        ys = [torch.empty((c.n, x.shape[1]), dtype=torch.float32, device="cuda") for _ in range(3)]
        spmm(A, X, out=ys[0], hub_nojoin=True, hub_continue=True)
        _join(X.device)
        first = ys[0].clone()
        spmm(A, X, out=ys[1], hub_nojoin=True, hub_continue=True)
        spmm(A, X, out=ys[2], hub_nojoin=True, hub_continue=True)
        _join(X.device)
        outs = [first, ys[1].clone(), ys[2].clone()]
    s.synchronize()
    for y in outs:
        np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_two_host_threads_two_streams(oracle_mod):
    """Two host threads issue hub-forking hops concurrently on their own streams."""
    from srgnn.spmm import propagate
    c = G.Case("rand_d128_r05")
    A = _hub_csr(c)
    x = c.x()
    want = oracle_mod.propagate(*c.ahat(), x, 4)
    errors, results = [], [None, None]

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                X = torch.from_numpy(x).cuda()
                for _ in range(20):
                    hops = propagate(A, X, 4)
                results[i] = [h.cpu() for h in hops]
            s.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    for r in results:
        for k in range(1, 5):
            np.testing.assert_array_equal(r[k].numpy(), want[k])


def test_expanded_panels_rejected():
    """An expanded (stride(0) == 0) source would make the kernel read past its allocation."""
    from srgnn.spmm import gather_rows
    src = torch.ones((1, 16), device="cuda").expand(8, 16)
    with pytest.raises(ValueError, match="overlap"):
        gather_rows(src, torch.zeros(4, dtype=torch.int64, device="cuda"))
    one = torch.ones((1, 16), device="cuda")
    out = gather_rows(one, torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert bool((out == 1).all())
