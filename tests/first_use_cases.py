"""Run in a fresh child process per case by tests/test_first_use_gpu.py: `python first_use_cases.py CASE`.
The process's first call into the library is one launch with hub rows, so the hub kernels of that
family run before any other entry could have raised their dynamic-LDS limit; the same call with
n_hub = 0 (the hub rows as row waves, the path the ladder tests hold to the oracle) must then give the
same bits, and the library's status must be clean.  The ladder operator (tests/ladder_cases.py) in
decreasing row length, the longest rows (3,081 entries: more than one 512-entry window) the hub prefix."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scalable-roubust-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ladder_cases as LC  # noqa: E402

N = LC.N
A1, A2, C0, C1 = 1.37, 0.81, 0.73, -1.19
HUB_W256 = 0x8                 # SRG_SPMM_HUB_W256 (include/srgnn_hip.h)
# n_hub per case: one slice per row at these widths, so n_hub hub workgroups; at most 256 of them take
# 512-entry windows, more take 256-entry ones
CASES = {
    "cheby_hub_f64_w512": ("float64", 16, 8),
    "cheby_hub_f64_w256": ("float64", 16, 300),
    "spmm_cheby_f32": ("float32", 32, 8),
    "spmm_csr_f32_hub_w256": ("float32", 32, 8),
    "spmm_span_f32": ("float32", 32, 8),
}


def main(case):
    from srgnn import _lib
    dtype, d, n_hub = CASES[case]
    lens = LC.lengths()
    order, _, _ = LC.sched_desc(lens, -1, -1)
    assert lens[order[0]] > 512 and lens[order[n_hub - 1]] > 0
    dev = torch.device("cuda", 0)
    ip, ix, v = (torch.from_numpy(a.copy()).to(dev) for a in LC.operator(dtype))
    o = torch.from_numpy(order).to(dev)
    X = torch.from_numpy(LC.x_panel(dtype, d)).to(dev)
    tdt = X.dtype
    ct = ctypes.c_float if dtype == "float32" else ctypes.c_double
    c0, c1 = (ct * 1)(C0), (ct * 1)(C1)
    a1, a2 = (float(np.dtype(dtype).type(x)) for x in (A1, A2))
    s = _lib.stream(dev)
    L = _lib.lib()                # loads the library; no entry point is called

    def run(nh):
        """The case's one library call with nh hub rows; returns (status, outputs)."""
        Y = torch.zeros((N, d), dtype=tdt, device=dev)
        R = torch.zeros((N, d), dtype=tdt, device=dev)
        csr = (ip.data_ptr(), ix.data_ptr(), v.data_ptr(), N, o.data_ptr())
        if case.startswith("cheby_hub_f64"):
            rc = L.srg_cheby_step_hub_f64(*csr, nh, X.data_ptr(), None, Y.data_ptr(), d, d, LC.INIT, a1, a2, c0, c1, 1,
                                          R.data_ptr(), N * d, s)
        elif case == "spmm_cheby_f32":
            rc = L.srg_spmm_cheby_f32(*csr, nh, 0, X.data_ptr(), d, Y.data_ptr(), d, d, 0, LC.INIT, a1, a2, None, 0, c0, c1,
                                      1, R.data_ptr(), d, N * d, s)
        elif case == "spmm_csr_f32_hub_w256":
            rc = L.srg_spmm_csr_f32(*csr, nh, 0, X.data_ptr(), d, Y.data_ptr(), d, d, HUB_W256, s)
        else:
            beg, end = ip[:-1].contiguous(), ip[1:].contiguous()
            rc = L.srg_spmm_span_f32(beg.data_ptr(), end.data_ptr(), ix.data_ptr(), v.data_ptr(), N, o.data_ptr(), nh, 0,
                                     X.data_ptr(), d, Y.data_ptr(), d, d, 0, None, 0, 0.0, 0, s)
        torch.cuda.synchronize()
        return rc, (Y, R)

    rc_hub, hub = run(n_hub)      # the process's first library call
    assert rc_hub == 0, f"{case}: first call, {n_hub} hub rows: status {rc_hub}: {_lib.last_error()}"
    rc_rows, rows = run(0)
    assert rc_rows == 0, f"{case}: n_hub = 0: status {rc_rows}: {_lib.last_error()}"
    it = torch.int32 if dtype == "float32" else torch.int64
    for name, a, b in zip(("Y / Tn", "R"), hub, rows):
        assert torch.equal(a.view(it), b.view(it)), f"{case}: {name} with {n_hub} hub rows differs from n_hub = 0"
    assert hub[0].abs().max().item() > 0, f"{case}: nothing was computed"
    assert L.srg_last_error_code() == 0, _lib.last_error()
    print(f"first_use ok: {case}")


if __name__ == "__main__":
    main(sys.argv[1])
