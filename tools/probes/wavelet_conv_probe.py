#!/usr/bin/env python3
"""Timing of the fused graph-wavelet filter (srgnn.wavelet_conv) beside the composition it replaces.

Operands as tools/probes/spspmm_grad_probe.py: N = 8192, phi = scipy.sparse.random(N, N, density=0.02,
format="csr", dtype=float32, random_state=numpy.random.default_rng(8192)) and phi^-1 the next draw of the
same generator, values (generator.random(nnz) + 0.5) as fp32, sort_indices(); theta uniform in
[0.9, 1.1], Z and G standard normal [N, d], d = 16 and d = 7, all device tensors.
Both paths run in one process on the same tensors, alternating, timed with device events after warm-up;
every figure is the median (min - max) of --reps runs:
  fused_ms        wavelet_conv(op, theta, Z).backward(G), theta and Z requiring grad
  composition_ms  the shims in the reference's call order: spspmm(phi, diag theta), spspmm(., phi^-1),
                  spmm(., Z), then .backward(G)
  *_peak_bytes    torch.cuda.max_memory_allocated above the operands over one such run
and, kernel against kernel on phi^-1 and Z (raw C entries, no Python checks):
  scaled_ms       srg_spmm_scaled_f32 with scale == NULL
  muladd_ms       srg_spmm_muladd_f32
for d = 7, 16, 32, 64.  --large-n repeats the fused / composition pair at d = 16 on a larger basis of
the same generator.  Prints one JSON line; --out also writes it to a file."""
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

import torch_sparse  # noqa: E402
from srgnn import _lib  # noqa: E402
from srgnn.wavelet_conv import WaveletOperator, wavelet_conv  # noqa: E402


def basis(n, density, rng):
    M = sp.random(n, n, density=density, format="csr", random_state=rng, dtype=np.float32)
    M.data = (rng.random(M.nnz) + 0.5).astype(np.float32)
    M.sort_indices()
    return M


def coo(M):
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return torch.from_numpy(np.vstack([rows, M.indices]).astype(np.int64)).cuda(), torch.from_numpy(M.data).cuda()


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def alternate(fns, reps, warmup=2):
    """{name: (median, min, max) ms} of the functions run in turn, `reps` rounds after `warmup`."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(timed(f))
    return {k: (float(np.median(t)), float(min(t)), float(max(t))) for k, t in times.items()}


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def layer_pair(n, density, d, reps, rng_seed=8192):
    rng = np.random.default_rng(rng_seed)
    phi, phi_inv = basis(n, density, rng), basis(n, density, rng)
    (pi, pv), (qi, qv) = coo(phi), coo(phi_inv)
    op = WaveletOperator(pi, pv, qi, qv, n)
    theta = torch.from_numpy(rng.uniform(0.9, 1.1, n).astype(np.float32)).cuda().requires_grad_(True)
    Z = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda().requires_grad_(True)
    G = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    di = torch.arange(n, device="cuda").repeat(2, 1)

    def fused():
        theta.grad = Z.grad = None
        wavelet_conv(op, theta, Z).backward(G)

    def composition():
        theta.grad = Z.grad = None
        ri, rv = torch_sparse.spspmm(pi, pv, di, theta, n, n, n)
        ci, cv = torch_sparse.spspmm(ri, rv, qi, qv, n, n, n)
        torch_sparse.spmm(ci, cv, n, n, Z).backward(G)
    t = alternate({"fused": fused, "composition": composition}, reps)
    ci = torch_sparse.spspmm(*torch_sparse.spspmm(pi, pv, di, theta.detach(), n, n, n), qi, qv, n, n, n)[0]
    nnz_c = int(ci.shape[1])
    del ci
    products_fused = (phi.nnz + phi_inv.nnz) * d            # forward; the backward is three more of this size
    products_comp = int(np.diff(phi_inv.indptr)[phi.indices].sum()) + nnz_c * d
    res = {"n": n, "d": d, "nnz_phi": int(phi.nnz), "nnz_phi_inverse": int(phi_inv.nnz), "nnz_product": nnz_c,
           "fused_ms": t["fused"][0], "fused_ms_min_max": t["fused"][1:], "composition_ms": t["composition"][0],
           "composition_ms_min_max": t["composition"][1:], "composition_over_fused": t["composition"][0] / t["fused"][0],
           "forward_products_fused": products_fused, "forward_products_composition": products_comp,
           "fused_peak_bytes": peak_above(fused), "composition_peak_bytes": peak_above(composition)}
    return res, op, Z.detach()


def kernel_pair(op, Z, d, reps):
    ip, ix, v = op.phi_inv
    n = op.n
    X = Z[:, :d].contiguous() if d <= Z.shape[1] else torch.randn(n, d, device="cuda")
    ya, yb = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    dev = X.device
    st = _lib.stream(dev)

    def scaled():
        _lib.call(dev, "srg_spmm_scaled_f32", ip.data_ptr(), ix.data_ptr(), v.data_ptr(), None, 0, n, X.data_ptr(), d,
                  ya.data_ptr(), d, d, st)

    def muladd():
        _lib.call(dev, "srg_spmm_muladd_f32", ip.data_ptr(), ix.data_ptr(), v.data_ptr(), n, X.data_ptr(), d,
                  yb.data_ptr(), d, d, st)
    t = alternate({"scaled": scaled, "muladd": muladd}, reps, warmup=3)
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    return {"d": d, "scaled_ms": t["scaled"][0], "scaled_ms_min_max": t["scaled"][1:], "muladd_ms": t["muladd"][0],
            "muladd_ms_min_max": t["muladd"][1:], "muladd_over_scaled": t["muladd"][0] / t["scaled"][0],
            "gmadds_per_s_scaled": ix.numel() * d / t["scaled"][0] / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--large-n", type=int, nargs="*", default=[], help="also time these larger bases at d = 16")
    ap.add_argument("--large-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wavelet_conv_probe needs a HIP device")
    layers, kernels = [], []
    for d in (16, 7):
        res, op, Z = layer_pair(args.n, args.density, d, args.reps)
        layers.append(res)
        if d == 16:
            for dk in (7, 16, 32, 64):
                kernels.append(kernel_pair(op, Z, dk, 5 * args.reps))
        del op, Z
        torch.cuda.empty_cache()
    out = {"probe": "wavelet_conv", "density": args.density, "seed": 8192, "reps": args.reps, "layers": layers,
           "kernels": kernels, "device": torch.cuda.get_device_name(0), "lib": _lib.version()}
    out["large"] = []
    for n in args.large_n:                                  # a size the composition cannot hold is recorded as such
        try:
            out["large"].append(layer_pair(n, args.density, 16, args.large_reps)[0])
        except torch.cuda.OutOfMemoryError as e:
            out["large"].append({"n": n, "d": 16, "composition": "out of memory", "error": str(e)[:200]})
            break
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
