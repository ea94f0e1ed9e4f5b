#!/usr/bin/env python3
"""The row-restricted GAT last layer (srgnn.gat's rows=) on the products-shaped and
arxiv-shaped synthetic graphs (R-MAT, symmetric, one self-loop per node), at the reference runner's last-layer
shapes and train-split sizes, in one process on the same tensors, windows alternating:

  rows_fwd / rows_fwd_bwd     gat_attend(..., rows=idx) forward, and forward + backward for all three gradients
  full_fwd / full_fwd_bwd     gat_attend(...)[idx], what model(x, adj_t)[train_idx] runs for the last layer
  gconv_fwd / gconv_fwd_bwd   graph_conv(op, X, rows=idx) on the same structure (unit values) at the same width:
                              the hop family's row path, the yardstick
  peak bytes                  torch.cuda.max_memory_allocated beyond what is allocated before the call

  products   (H, C) = (1, 47), a shuffled batch of 196,615 rows (8 % of the nodes)
  arxiv      (H, C) = (1, 40), a shuffled batch of 90,941 rows (54 %)

Rates are over a byte model of the rows path: forward 4 nnzB (ids) + 4 nnzB H (a_src gathers) + 4 nnzB H C
(gathered rows of Hf) + 4 B H C (out) + 16 B H; backward, over the transpose, 4 nnz (its ids) + 4 nnz (pos of
every target) + 4 nnzB H C (the member rows of G gathered) + 12 nnzB H (a_dst, M, Z) + 4 n H C (dHf written),
plus the edge pass 4 nnzB + 4 nnzB H C (Hf gathered again) + 8 nnzB H (dS written and read back): end-to-end
rates of the whole call, not a kernel's.  Device-event timing, `launches` back-to-back calls per window after a
warm-up; spread = (max - min) / median.  Nothing is fixed in advance: the file records what was measured, also
where the rows path is not the faster one.  Needs a HIP device.

    python tools/gat_rows_probe.py [--out profiles/gat_rows_probe.json] [--graphs products,arxiv]
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
from srgnn import gat as GT  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402
from srgnn.graph_conv import GraphConvOperator, graph_conv  # noqa: E402

CASES = {"products": dict(H=1, C=47, B=196615), "arxiv": dict(H=1, C=40, B=90941)}


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


def alternate(runs, launches, windows):
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(windows):
        for name, fn in runs.items():
            times[name].append(window(fn, launches))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "gat_rows_probe.json"))
    ap.add_argument("--graphs", default="products,arxiv")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_rows_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"what": "gat_attend with rows= against gat_attend(...)[idx] and graph_conv(..., rows=) at the same width; "
                   "same process, same tensors, alternating windows",
           "launches_per_window": a.launches, "windows": a.windows, "library": _lib.version(),
           "device": torch.cuda.get_device_name(0), "graphs": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name in a.graphs.split(","):
        cfg, case = synth.CONFIGS[name], CASES[name]
        n, H, C, B = cfg["n"], case["H"], case["C"], case["B"]
        W = H * C
        u, v = synth.rmat_undirected_t(n, cfg["n_edges"], seed=synth.RMAT_SEED, device=dev)
        ip, ix = synth.symmetric_csr_t(n, u, v)
        del u, v
        rows = torch.repeat_interleave(torch.arange(n, device=dev), ip[1:] - ip[:-1])
        g = GT.GATGraph.from_edge_index(torch.stack([ix.long(), rows]), n, add_self_loops=True, device=dev)
        del rows, ip, ix
        nnz = g.nnz
        op = GraphConvOperator(DeviceCSR.from_tensors(g.indptr, g.indices, torch.ones(nnz, device=dev), n_cols=n,
                                                      device=dev))
        gen = torch.Generator(device=dev).manual_seed(11)
        idx = torch.randperm(n, device=dev, generator=gen)[:B].contiguous()
        nnzB = int((g.indptr[idx + 1] - g.indptr[idx]).sum())
        Hf = torch.randn((n, W), device=dev, generator=gen).requires_grad_(True)
        a_s = torch.randn((n, H), device=dev, generator=gen).requires_grad_(True)
        a_d = torch.randn((n, H), device=dev, generator=gen).requires_grad_(True)
        G = torch.randn((B, W), device=dev, generator=gen)

        def clear():
            Hf.grad = a_s.grad = a_d.grad = None

        def rows_fwd():
            with torch.no_grad():
                GT.gat_attend(g, Hf, a_s, a_d, rows=idx)

        def rows_fwd_bwd():
            clear()
            GT.gat_attend(g, Hf, a_s, a_d, rows=idx).backward(G)

        def full_fwd():
            with torch.no_grad():
                GT.gat_attend(g, Hf, a_s, a_d)[idx]

        def full_fwd_bwd():
            clear()
            GT.gat_attend(g, Hf, a_s, a_d)[idx].backward(G)

        def gconv_fwd():
            with torch.no_grad():
                graph_conv(op, Hf, rows=idx)

        def gconv_fwd_bwd():
            clear()
            graph_conv(op, Hf, rows=idx).backward(G)

        runs = {"rows_fwd": rows_fwd, "rows_fwd_bwd": rows_fwd_bwd, "full_fwd": full_fwd, "full_fwd_bwd": full_fwd_bwd,
                "gconv_fwd": gconv_fwd, "gconv_fwd_bwd": gconv_fwd_bwd}
        tm = alternate(runs, a.launches, a.windows)
        fwd_model = 4 * nnzB + 4 * nnzB * H + 4 * nnzB * W + 4 * B * W + 16 * B * H
        bwd_model = (8 * nnz + 4 * nnzB * W + 12 * nnzB * H + 4 * n * W) + (4 * nnzB + 4 * nnzB * W + 8 * nnzB * H)
        r = {"n": n, "nnz": nnz, "H": H, "C": C, "B": B, "nnzB": nnzB, "batch_share_of_rows": B / n,
             "batch_share_of_entries": nnzB / nnz,
             "rows_fwd": summary(tm["rows_fwd"], fwd_model),
             "rows_fwd_bwd": summary(tm["rows_fwd_bwd"], fwd_model + bwd_model)}
        for k in ("full_fwd", "full_fwd_bwd", "gconv_fwd", "gconv_fwd_bwd"):
            r[k] = summary(tm[k])
        for k, fn in runs.items():
            r[k + "_peak_bytes"] = peak_of(fn)
        for k in ("fwd", "fwd_bwd"):
            r[f"full_{k}_over_rows_{k}"] = r[f"full_{k}"]["ms"] / r[f"rows_{k}"]["ms"]
            r[f"rows_{k}_over_gconv_{k}"] = r[f"rows_{k}"]["ms"] / r[f"gconv_{k}"]["ms"]
            r[f"full_{k}_peak_over_rows_{k}_peak"] = r[f"full_{k}_peak_bytes"] / max(r[f"rows_{k}_peak_bytes"], 1)
        with torch.no_grad():
            same = torch.equal(GT.gat_attend(g, Hf, a_s, a_d, rows=idx).view(torch.int32),
                               GT.gat_attend(g, Hf, a_s, a_d)[idx].view(torch.int32))
        r["forward_bits_equal_full_path"] = bool(same)
        res["graphs"][name] = r
        print(json.dumps({name: {k: (round(v["ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}}), flush=True)
        save()
        clear()
        del Hf, a_s, a_d, G, op, g, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
