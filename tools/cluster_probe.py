#!/usr/bin/env python3
"""The Cluster-GCN batch extraction (srgnn.cluster) on the products-shaped and arxiv-shaped
synthetic graphs (R-MAT, symmetric, Â at r = 0.5) at the reference runner's loader settings, num_parts = 128 and
batch_size = 32 (contiguous row blocks of near-equal rows + entries as parts), in one process on the same
tensors, windows alternating:

  fused_kernels    srg_csr_induced_f32 phase 0, torch.cumsum, the read of ptr[-1], the allocation, phase 1, for
                   one batch whose ids and pos table are already built
  torch_kernels    the same extraction from the same ids and pos composed of torch ops on the same device:
                   repeat_interleave, gathers, the pos lookup, mask, nonzero, segment counts, cumsum
  fused_call       induced_subgraph(A, nodes): batch_rows' checks and table, then the above
  torch_call       batch_rows, then the composition
  fused_epoch      list(ClusterLoader): the four batches of one shuffled epoch (the same permutation every time)
  torch_epoch      the same node lists through batch_rows and the composition
  copy             dst.copy_(src) of 4 L bytes: what a plain device copy reaches in this run
  peak bytes       torch.cuda.max_memory_allocated beyond what is allocated before the call

Rates are over the byte model of the extraction, L = entries of the batch's rows, nnzB = kept entries:
reads 8 (B + 1) + 8 B, per phase 4 L ids and 4 L table gathers, writes (4 + 4) nnzB + 8 B.  They are end-to-end
rates of the whole call, cumsum and host read included, not a kernel's.  Device-event timing after a warm-up of
every run, at least `launches` calls per window and enough of them for a window of about 20 ms (calls_per_window
in the file); spread = (max - min) / median.  Nothing is fixed in advance: the file
records what was measured, also where the fused path is not the faster one.  Needs a HIP device.

    python tools/cluster_probe.py [--out profiles/cluster_probe.json] [--graphs products,arxiv]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "scalable-roubust-gnn_amd"))

import torch  # noqa: E402

from srgnn import _lib, synth  # noqa: E402
from srgnn import cluster as CL  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402
from srgnn.graph_conv import batch_rows  # noqa: E402
from srgnn.normalize import sym_norm_binary  # noqa: E402

NUM_PARTS, BATCH_SIZE, EPOCH_SEED = 128, 32, 5


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def summary(ms_list, model_bytes=None):
    ms = statistics.median(ms_list)
    out = {"ms": ms, "ms_windows": ms_list, "spread": (max(ms_list) - min(ms_list)) / ms}
    if model_bytes is not None:
        out["model_bytes"] = model_bytes
        out["tb_per_s_over_model"] = model_bytes / (ms * 1e-3) / 1e12
    return out


def alternate(runs, launches, windows, min_window_ms=20.0):
    """Per run the windows' times and the calls per window: at least `launches`, and enough of them that a
    window lasts about min_window_ms (a window of a fraction of a millisecond measures the clock)."""
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    calls = {name: max(launches, min(2000, int(min_window_ms / max(window(fn, launches), 1e-4)) + 1))
             for name, fn in runs.items()}
    times = {name: [] for name in runs}
    for _ in range(windows):
        for name, fn in runs.items():
            times[name].append(window(fn, calls[name]))
    return times, calls


def fused_kernels(A, ids, pos):
    """induced_subgraph after batch_rows: (ptr, idx, val)."""
    dev, B = A.device, ids.numel()
    cnt = torch.empty(B, dtype=torch.int64, device=dev)
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    args = (A.indptr.data_ptr(), A.indices.data_ptr(), A.values.data_ptr(), A.n_rows, A.n_cols, ids.data_ptr(), B,
            pos.data_ptr())
    _lib.call(dev, "srg_csr_induced_f32", 0, *args, cnt.data_ptr(), None, None, None, None, _lib.stream(dev))
    torch.cumsum(cnt, 0, out=ptr[1:])
    nnz = int(ptr[-1])
    idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call(dev, "srg_csr_induced_f32", 1, *args, None, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), None,
              _lib.stream(dev))
    return ptr, idx, val


def torch_kernels(A, ids, pos):
    """The same extraction composed of torch ops: (ptr, idx, val)."""
    dev, B = A.device, ids.numel()
    beg = A.indptr[ids]
    ln = A.indptr[ids + 1] - beg
    start = torch.cumsum(ln, 0) - ln
    row = torch.repeat_interleave(torch.arange(B, device=dev), ln)               # [L]
    j = beg[row] + (torch.arange(row.numel(), device=dev) - start[row])           # [L] the entry of the operator
    p = pos[A.indices[j].long()]                                                  # [L]
    sel = torch.nonzero(p >= 0).squeeze(1)                                        # [nnzB]
    idx = p[sel]
    val = A.values[j[sel]]
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(row[sel], minlength=B), 0, out=ptr[1:])
    return ptr, idx, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "cluster_probe.json"))
    ap.add_argument("--graphs", default="products,arxiv")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"what": "induced_subgraph / ClusterLoader against the torch composition of the same extraction; same "
                   "process, same tensors, alternating windows",
           "num_parts": NUM_PARTS, "batch_size": BATCH_SIZE, "launches_per_window": a.launches, "windows": a.windows,
           "library": _lib.version(), "device": torch.cuda.get_device_name(0), "graphs": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name in a.graphs.split(","):
        cfg = synth.CONFIGS[name]
        n = cfg["n"]
        u, v = synth.rmat_undirected_t(n, cfg["n_edges"], seed=synth.RMAT_SEED, device=dev)
        ip, ix = synth.symmetric_csr_t(n, u, v)
        del u, v
        ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
        A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev)
        del ip, ix, vals
        cd = CL.ClusterData(A, NUM_PARTS)
        cd.perm, cd.partptr = cd.perm.to(dev), cd.partptr.to(dev)                 # node lists cut on the device

        def loader():
            return CL.ClusterLoader(cd, BATCH_SIZE, shuffle=True, generator=torch.Generator().manual_seed(EPOCH_SEED))

        part_batches = loader().part_batches()
        node_lists = [cd.nodes_of(p).contiguous() for p in part_batches]
        nodes = node_lists[0]
        ids, pos, unique = batch_rows(nodes, n, dev)
        assert unique
        B = ids.numel()
        L = int((A.indptr[ids + 1] - A.indptr[ids]).sum())
        want = fused_kernels(A, ids, pos)
        got = torch_kernels(A, ids, pos)
        nnzB = int(want[0][-1])
        same = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
                    and torch.equal(want[2].view(torch.int32), got[2].view(torch.int32)))
        del want, got
        src = torch.empty(L, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)

        runs = {
            "fused_kernels": lambda: fused_kernels(A, ids, pos),
            "torch_kernels": lambda: torch_kernels(A, ids, pos),
            "fused_call": lambda: CL.induced_subgraph(A, nodes),
            "torch_call": lambda: torch_kernels(A, *batch_rows(nodes, n, dev)[:2]),
            "fused_epoch": lambda: [b.csr for b in loader()],
            "torch_epoch": lambda: [torch_kernels(A, *batch_rows(s, n, dev)[:2]) for s in node_lists],
            "copy": lambda: dst.copy_(src),
        }
        tm, calls = alternate(runs, a.launches, a.windows)
        model = 8 * (B + 1) + 8 * B + 2 * (4 * L + 4 * L) + 8 * nnzB + 8 * B
        lens = A.indptr[1:] - A.indptr[:-1]
        r = {"n": n, "nnz": int(A.indices.numel()), "B": B, "L": L, "nnzB": nnzB, "longest_row": int(lens.max()),
             "longest_row_in_batch": int(lens[ids].max()), "batch_share_of_rows": B / n,
             "kept_share_of_batch_entries": nnzB / max(L, 1), "pos_table_bytes": 4 * n,
             "batches_per_epoch": len(node_lists), "torch_composition_bits_equal": same, "calls_per_window": calls}
        for k in ("fused_kernels", "fused_call"):
            r[k] = summary(tm[k], model)
        for k in ("torch_kernels", "torch_call", "fused_epoch", "torch_epoch"):
            r[k] = summary(tm[k])
        r["copy"] = summary(tm["copy"], 8 * L)
        for k, fn in runs.items():
            if k != "copy":
                r[k + "_peak_bytes"] = peak_of(fn)
        for k in ("kernels", "call", "epoch"):
            r[f"torch_{k}_over_fused_{k}"] = r[f"torch_{k}"]["ms"] / r[f"fused_{k}"]["ms"]
            r[f"torch_{k}_peak_over_fused_{k}_peak"] = r[f"torch_{k}_peak_bytes"] / max(r[f"fused_{k}_peak_bytes"], 1)
        r["fused_kernels_rate_over_copy_rate"] = r["fused_kernels"]["tb_per_s_over_model"] / r["copy"]["tb_per_s_over_model"]
        res["graphs"][name] = r
        print(json.dumps({name: {k: (round(v["ms"], 3) if isinstance(v, dict) and "ms" in v else v) for k, v in r.items()}}), flush=True)
        save()
        del A, cd, src, dst, ids, pos, nodes, node_lists, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
