#!/usr/bin/env python3
"""The fused GAT aggregation (srgnn.gat) on the arxiv-shaped and products-shaped synthetic
graphs (R-MAT, symmetric, one self-loop per node), in one process on the same tensors, windows alternating:

  gat_fwd / gat_fwd_bwd   gat_attend forward, and forward + backward for all three gradients, at
                          (H, C) = (8, 32), (1, 47) and, where memory allows, (8, 256)
  hop                     srgnn.spmm.hop on the same structure (unit values) at width H*C: the yardstick -- a GAT
                          aggregation is a hop plus H small gathers and an expf per entry
  torch_fwd / _fwd_bwd    the torch composition from primitives on the same device, where its [nnz, H, C]
                          message tensor fits in --torch-limit-gb
  peak bytes              torch.cuda.max_memory_allocated beyond what is allocated before the call

Rates are over the forward's byte model -- 4 nnz (ids) + 4 nnz H (a_src gathers) + 4 nnz H C (gathered rows)
+ 4 n H C (out) + 16 n H (a_dst, M, Z and back) -- and the hop's over 8 nnz + 4 nnz d + 4 n d: end-to-end rates of
the whole call, not a kernel's.  Device-event timing, `launches` back-to-back calls per window after a warm-up;
spread = (max - min) / median.  Nothing is fixed in advance: the file records what was measured.  Results are
written after every section, so a run cut short keeps what it has.  Needs a HIP device.

    python tools/gat_probe.py [--out profiles/gat_probe.json] [--graphs arxiv,products]
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

from srgnn import _lib, spmm, synth  # noqa: E402
from srgnn import gat as GT  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402


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


def compose(g, rows, Hf, a_src, a_dst, slope):
    """The aggregation from torch primitives: [nnz, H] scores and [nnz, H, C] messages."""
    n, H = a_src.shape
    C = Hf.shape[1] // H
    ix = g.indices.long()
    l = torch.nn.functional.leaky_relu(a_src.index_select(0, ix) + a_dst.index_select(0, rows), slope)
    m = torch.full((n, H), -torch.inf, device=l.device).scatter_reduce(0, rows[:, None].expand(-1, H), l.detach(), "amax")
    p = torch.exp(l - m.index_select(0, rows))
    z = torch.zeros((n, H), device=l.device).index_add(0, rows, p)
    msg = (p / z.index_select(0, rows))[:, :, None] * Hf.view(n, H, C).index_select(0, ix)
    return torch.zeros((n, H, C), device=l.device).index_add(0, rows, msg).reshape(n, H * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "gat_probe.json"))
    ap.add_argument("--graphs", default="arxiv,products")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--torch-limit-gb", type=float, default=24.0,
                    help="run the torch composition where 4 nnz H C bytes stay below this")
    ap.add_argument("--wide-limit-gb", type=float, default=64.0,
                    help="run (8, 256) where its panels (Hf, out, G, dHf) stay below this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"what": "gat_attend forward and forward + backward, spmm.hop at width H*C on the same structure, the torch "
                   "composition where its per-edge tensor fits; same process, same tensors, alternating windows",
           "launches_per_window": a.launches, "windows": a.windows, "library": _lib.version(),
           "device": torch.cuda.get_device_name(0), "graphs": {}}

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
        rows = torch.repeat_interleave(torch.arange(n, device=dev), ip[1:] - ip[:-1])
        g = GT.GATGraph.from_edge_index(torch.stack([ix.long(), rows]), n, add_self_loops=True, device=dev)
        del rows, ip, ix
        nnz = g.nnz
        deg = g.indptr[1:] - g.indptr[:-1]
        A = DeviceCSR.from_tensors(g.indptr, g.indices, torch.ones(nnz, device=dev), n_cols=n, device=dev)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), deg)
        gr = {"n": n, "nnz": nnz, "longest_row": int(deg.max()), "median_row": int(deg.median()), "shapes": {}}
        res["graphs"][name] = gr
        gen = torch.Generator(device=dev).manual_seed(11)
        for (H, C) in ((8, 32), (1, 47), (8, 256)):
            W = H * C
            key = f"H{H}_C{C}"
            if 4 * 4 * n * W > a.wide_limit_gb * 2 ** 30:
                gr["shapes"][key] = {"skipped": "the four [n, H*C] panels exceed --wide-limit-gb"}
                save()
                continue
            Hf = torch.randn((n, W), device=dev, generator=gen).requires_grad_(True)
            a_s = torch.randn((n, H), device=dev, generator=gen).requires_grad_(True)
            a_d = torch.randn((n, H), device=dev, generator=gen).requires_grad_(True)
            G = torch.randn((n, W), device=dev, generator=gen)
            out_hop = torch.empty((n, W), device=dev)
            spmm.prepare(A, W, 1)

            def fwd():
                with torch.no_grad():
                    GT.gat_attend(g, Hf, a_s, a_d)

            def fwd_bwd():
                Hf.grad = a_s.grad = a_d.grad = None
                GT.gat_attend(g, Hf, a_s, a_d).backward(G)

            def hop():
                spmm.hop(A, Hf.detach(), out_hop)

            runs = {"gat_fwd": fwd, "gat_fwd_bwd": fwd_bwd, "hop": hop}
            with_torch = 4 * nnz * W <= a.torch_limit_gb * 2 ** 30
            if with_torch:
                def t_fwd():
                    with torch.no_grad():
                        compose(g, rows, Hf, a_s, a_d, 0.2)

                def t_fwd_bwd():
                    Hf.grad = a_s.grad = a_d.grad = None
                    compose(g, rows, Hf, a_s, a_d, 0.2).backward(G)

                runs.update({"torch_fwd": t_fwd, "torch_fwd_bwd": t_fwd_bwd})
            tm = alternate(runs, a.launches, a.windows)
            fwd_model = 4 * nnz + 4 * nnz * H + 4 * nnz * W + 4 * n * W + 16 * n * H
            hop_model = 8 * nnz + 4 * nnz * W + 4 * n * W
            r = {"gat_fwd": summary(tm["gat_fwd"], fwd_model), "gat_fwd_bwd": summary(tm["gat_fwd_bwd"]),
                 "hop": summary(tm["hop"], hop_model),
                 "gat_fwd_peak_bytes": peak_of(fwd), "gat_fwd_bwd_peak_bytes": peak_of(fwd_bwd),
                 "per_edge_message_bytes": 4 * nnz * W}
            r["gat_fwd_over_hop"] = r["gat_fwd"]["ms"] / r["hop"]["ms"]
            r["gat_fwd_bwd_over_hop"] = r["gat_fwd_bwd"]["ms"] / r["hop"]["ms"]
            if with_torch:
                r.update({"torch_fwd": summary(tm["torch_fwd"]), "torch_fwd_bwd": summary(tm["torch_fwd_bwd"]),
                          "torch_fwd_peak_bytes": peak_of(t_fwd), "torch_fwd_bwd_peak_bytes": peak_of(t_fwd_bwd)})
                r["torch_fwd_over_gat_fwd"] = r["torch_fwd"]["ms"] / r["gat_fwd"]["ms"]
                r["torch_fwd_bwd_over_gat_fwd_bwd"] = r["torch_fwd_bwd"]["ms"] / r["gat_fwd_bwd"]["ms"]
                with torch.no_grad():
                    r["max_abs_difference_to_torch"] = float((compose(g, rows, Hf, a_s, a_d, 0.2) -
                                                              GT.gat_attend(g, Hf, a_s, a_d)).abs().max())
            else:
                r["torch"] = "skipped: 4 nnz H C bytes exceed --torch-limit-gb"
            gr["shapes"][key] = r
            print(json.dumps({name: {key: {k: (round(v["ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}}}),
                  flush=True)
            save()
            Hf.grad = a_s.grad = a_d.grad = None
            del Hf, a_s, a_d, G, out_hop
            torch.cuda.empty_cache()
        del A, g, rows, deg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
