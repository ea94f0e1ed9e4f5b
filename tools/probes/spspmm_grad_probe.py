#!/usr/bin/env python3
"""Timing of the sparse product's adjoint beside its forward (srg_spgemm_grad_f32, srg_spgemm_f32).

One synthetic basis pair, the shape of the wavelet layer's second product C2 = C1 @ phi^-1:
  N = 8192;  A = scipy.sparse.random(N, N, density=0.02, format="csr", dtype=float32,
  random_state=numpy.random.default_rng(8192)) and B the next draw of the same generator, both with
  values (generator.random(nnz) + 0.5) as fp32 and sort_indices() (column-sorted rows); G =
  generator.standard_normal(nnz(C)) as fp32.
Timed with device events after warm-up runs, the median of --reps runs each:
  forward_ms        srgnn.sparse.spgemm: both passes with the host work between them
  forward_kernels_ms the two srg_spgemm_f32 launches alone (count pass + fill pass, C preallocated)
  grad_a_ms         srg_spgemm_grad_f32 with P = A, D = G on C, R = B
  grad_b_ms         srg_spgemm_grad_f32 with P = B^T, D = G^T, R = A^T (the transposes prebuilt)
  transposes_ms     the three csr_transpose calls of the B side and the permutation back
(*_gmadds_per_s: multiply-adds done per second, the forward's counted in both of its passes)
and, from the operands alone, what a lane-per-chain schedule can use of a wave: chain_efficiency =
sum of chain lengths / sum over the waves of 64 * the wave's longest chain (entries of a pattern row
taken 256 at a time, 64 per wave), and lanes_active = pattern entries / (64 * waves that have any).
Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "scalable-roubust-gnn_amd"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from srgnn import _lib  # noqa: E402
from srgnn.sparse import csr_transpose, spgemm, spgemm_grad  # noqa: E402


def basis(n, density, rng):
    M = sp.random(n, n, density=density, format="csr", random_state=rng, dtype=np.float32)
    M.data = (rng.random(M.nnz) + 0.5).astype(np.float32)
    M.sort_indices()
    return M


def dev_csr(M):
    return (torch.from_numpy(M.indptr.astype(np.int64)).cuda(), torch.from_numpy(M.indices.astype(np.int32)).cuda(),
            torch.from_numpy(M.data.astype(np.float32)).cuda())


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times)), float(min(times)), float(max(times))


def wave_use(p_ip, p_ix, r_ip):
    """(chain_efficiency, lanes_active) of one chain per lane, pattern entries 64 per wave."""
    length = np.diff(r_ip)[p_ix]
    work = waves = longest = 0
    for r in range(p_ip.size - 1):
        row = length[p_ip[r]:p_ip[r + 1]]
        for w0 in range(0, row.size, 64):
            part = row[w0:w0 + 64]
            work += int(part.sum())
            longest += 64 * int(part.max())
            waves += 1
    return work / max(longest, 1), p_ix.size / max(64 * waves, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spspmm_grad_probe needs a HIP device")
    n = args.n
    rng = np.random.default_rng(8192)
    A, B = basis(n, args.density, rng), basis(n, args.density, rng)
    a, b = dev_csr(A), dev_csr(B)
    dev = a[0].device
    c_ip, c_ix, c_v = spgemm(*a, *b, n)
    g = torch.from_numpy(rng.standard_normal(c_v.numel()).astype(np.float32)).cuda()
    madds = int(np.diff(B.indptr)[A.indices].sum())

    fwd = median_ms(lambda: spgemm(*a, *b, n), args.reps)
    cnt = torch.empty(n, dtype=torch.int64, device=dev)
    o_ix, o_v = torch.empty_like(c_ix), torch.empty_like(c_v)

    def forward_kernels():
        for phase, ptr, ix, v in ((0, None, None, None), (1, c_ip.data_ptr(), o_ix.data_ptr(), o_v.data_ptr())):
            _lib.call(dev, "srg_spgemm_f32", phase, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, b[0].data_ptr(),
                      b[1].data_ptr(), b[2].data_ptr(), n, cnt.data_ptr(), ptr, ix, v, None, 0, 0, _lib.stream(dev))
    if n > 16384:
        raise SystemExit("the kernel-only forward timing of this probe covers the LDS accumulator (n <= 16384)")
    fwd_k = median_ms(forward_kernels, args.reps)
    assert torch.equal(o_v, c_v) and torch.equal(o_ix, c_ix)

    grad_a = median_ms(lambda: spgemm_grad(a[0], a[1], c_ip, c_ix, g, *b, n, check=False), args.reps)

    def transposes():
        bt = csr_transpose(*b, n)
        gt = csr_transpose(c_ip, c_ix, g, n)
        at = csr_transpose(*a, n)
        return bt, gt, at
    bt, gt, at = transposes()
    out_t = spgemm_grad(bt[0], bt[1], gt[0], gt[1], gt[2], at[0], at[1], at[2], n, check=False)

    def transposes_and_back():
        t = transposes()
        back = torch.empty_like(out_t)
        back[t[0][3]] = out_t
        return back
    tr = median_ms(transposes_and_back, args.reps)
    grad_b = median_ms(lambda: spgemm_grad(bt[0], bt[1], gt[0], gt[1], gt[2], at[0], at[1], at[2], n, check=False),
                       args.reps)
    eff_a = wave_use(A.indptr, A.indices, B.indptr)
    Bt, At = sp.csr_matrix(B.T), sp.csr_matrix(A.T)
    eff_b = wave_use(Bt.indptr, Bt.indices, At.indptr)
    res = {"probe": "spspmm_grad", "n": n, "density": args.density, "seed": 8192, "reps": args.reps,
           "nnz_a": int(A.nnz), "nnz_b": int(B.nnz), "nnz_c": int(c_v.numel()), "multiply_adds": madds,
           "forward_ms": fwd[0], "forward_ms_min_max": fwd[1:], "forward_kernels_ms": fwd_k[0],
           "forward_kernels_ms_min_max": fwd_k[1:], "grad_a_ms": grad_a[0], "grad_a_ms_min_max": grad_a[1:],
           "grad_b_ms": grad_b[0], "grad_b_ms_min_max": grad_b[1:], "transposes_ms": tr[0],
           "transposes_ms_min_max": tr[1:], "grad_a_over_forward_kernels": grad_a[0] / fwd_k[0],
           "grad_b_over_forward_kernels": grad_b[0] / fwd_k[0], "grad_b_over_grad_a": grad_b[0] / grad_a[0],
           "grad_a_gmadds_per_s": madds / grad_a[0] / 1e6, "grad_b_gmadds_per_s": madds / grad_b[0] / 1e6,
           "forward_kernels_gmadds_per_s": 2 * madds / fwd_k[0] / 1e6,
           "chain_efficiency_a": eff_a[0], "lanes_active_a": eff_a[1], "chain_efficiency_b": eff_b[0],
           "lanes_active_b": eff_b[1], "device": torch.cuda.get_device_name(dev), "lib": _lib.version()}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
