#!/usr/bin/env python3
"""Timing and peak memory of spmm's value gradient: srgnn.sparse.sddmm (srg_sddmm_f32) beside the
composition it replaced, (grad[row] * matrix[col]).sum(-1), on the same device tensors in one process.

Shapes (--shape):
  wav_rand   the wavelet network's own call on the committed fixture: the pattern of
             spspmm(spspmm(phi0, diag theta), phi1) (n = 130, 15810 entries), d = 16 filters;
  large16    m = n = 4096, scipy.sparse.random(density = 0.24, random_state = default_rng(4096)), about
  large64    4 * 10^6 entries in rows of about 1000 (a phi * phi^-1 of that size), d = 16 and d = 64.
G and X are standard normal fp32 from the same generator; perm is the identity's shuffle (the shim always
passes one).  Per shape, alternating the two paths, the median of --reps device-event timings each, and
torch.cuda.max_memory_allocated above the operands for one call of each.  Also counted from the shapes:
  compulsory_bytes   nnz * (4 d + 4 + 4 + 8) + n_rows * d * 4   (X's row per entry, the column id, the
                     result, perm; G's rows once) -- what the kernel must move if nothing is reused;
  composition_bytes  5 * nnz * d * 4  (two gathers written, both read back, the product written; the sum
                     reads it once more, not counted).
--only sddmm|composition runs one path alone (for a counter pass under a profiler).
Prints one JSON line per shape; --out writes them to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "scalable-roubust-gnn_amd"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from srgnn import _lib  # noqa: E402
from srgnn.sparse import sddmm  # noqa: E402


def wav_rand_pattern():
    z = np.load(os.path.join(REPO, "tests", "golden", "wav_rand.npz"), allow_pickle=False)
    n = z["phi0_indptr"].size - 1
    phi = [sp.csr_matrix((np.ones(z[f"phi{i}_data"].size, np.float32), z[f"phi{i}_indices"], z[f"phi{i}_indptr"]),
                         shape=(n, n)) for i in (0, 1)]
    C = (phi[0] @ phi[1]).tocsr()           # positive values: the product drops nothing
    C.sort_indices()
    return C.indptr.astype(np.int64), C.indices.astype(np.int32), n


def large_pattern():
    n = 4096
    A = sp.random(n, n, density=0.24, format="csr", random_state=np.random.default_rng(4096), dtype=np.float32)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), n


SHAPES = {"wav_rand": (wav_rand_pattern, 16), "large16": (large_pattern, 16), "large64": (large_pattern, 64)}


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def run(shape, reps, warmup, only):
    build, d = SHAPES[shape]
    ip, ix, n = build()
    nnz = ix.size
    rng = np.random.default_rng(nnz + d)
    G = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    X = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
    perm = torch.from_numpy(rng.permutation(nnz).astype(np.int64)).cuda()
    tip, tix = torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda()
    # the composition's operands in the caller's COO order, as the shim's backward held them
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(nnz, device=perm.device)
    row = torch.repeat_interleave(torch.arange(n, device=perm.device), tip[1:] - tip[:-1])[inv]
    col = tix.to(torch.int64)[inv]

    def kernel():
        return sddmm(tip, tix, G, X, perm=perm, check=False)

    def composition():
        return (G[row] * X[col]).sum(dim=-1)

    paths = {"sddmm": kernel, "composition": composition}
    if only:
        paths = {only: paths[only]}
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):                   # alternating, so drift hits both alike
        for k, fn in paths.items():
            times[k].append(timed(fn))
    res = {"probe": "sddmm", "shape": shape, "n": n, "nnz": int(nnz), "d": d, "reps": reps, "warmup": warmup,
           "compulsory_bytes": int(nnz * (4 * d + 16) + n * d * 4), "composition_bytes": int(5 * nnz * d * 4),
           "device": torch.cuda.get_device_name(0), "lib": _lib.version()}
    for k, fn in paths.items():
        res[k] = stats(times[k])
        res[k]["peak_bytes"] = peak_above(fn)
    if not only:
        a, b = kernel(), composition()
        scale = float(b.abs().max())
        res["max_abs_difference_over_max"] = float((a - b).abs().max()) / scale
        res["composition_over_sddmm"] = res["composition"]["median_ms"] / res["sddmm"]["median_ms"]
        res["sddmm_compulsory_gb_per_s"] = res["compulsory_bytes"] / res["sddmm"]["median_ms"] / 1e6
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["sddmm", "composition"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_probe needs a HIP device")
    lines = []
    for shape in (sorted(SHAPES) if args.shape == "all" else [args.shape]):
        lines.append(json.dumps(run(shape, args.reps, args.warmup, args.only)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
