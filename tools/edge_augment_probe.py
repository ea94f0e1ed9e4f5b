#!/usr/bin/env python3
"""Edge augmentation at products scale (panels of n = 2,449,029 rows, d = 263 and 303; R = 1e5 and 1e6
low-degree query rows; M = 100 and 300 candidates per row, k = M / 100 selected): in one process, on the
same tensors and the same candidate ids, windows of the three alternating,

  (a) select       srg_knn_select_f32 (srgnn.augment.knn_select): one call, argument check included;
  (b) gather       srgnn.spmm.gather_rows over the identical id stream (cand, in order) into a [chunk, d]
                   buffer reused chunk after chunk: the ceiling the select kernel's rate is quoted against.
                   It reads the same R*M*d*4 bytes and, unlike the select kernel, writes them again;
  (c) composition  torch on the device, chunked over query rows to fit memory: index_select of the
                   candidates' rows, subtract the query row, norm(dim=2), topk(k, largest=False);

and srg_sample_distinct_i64 on the same pointer array.  Device-event timing; every window is `launches`
back-to-back calls after a warm-up of the same shape; spread = (max - min) / median over the windows.  The
byte model of (a) is R*M*d*4 + R*d*4 (every candidate row once, every query row once); rates are the model's
bytes over the time of the whole call: end-to-end rates, not a kernel's.  The composition's ids are compared
with the kernel's at the timed size (they may differ where the two summation orders round a near-tie apart).
Then edge_augment end to end (host clock around a device synchronise) on a random graph of the same n whose
edge count leaves about R nodes without an edge, and, on the small fixtures of tests/golden, the
candidates="reference" path: the O(n)-per-node host replay of the reference's draw plus the device selection
(labelled as such; the reference's own loop is not part of this tree).  Needs a HIP device.

    python tools/edge_augment_probe.py [--out profiles/edge_augment_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "scalable-roubust-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from srgnn import _lib  # noqa: E402
from srgnn import augment as A  # noqa: E402
from srgnn.spmm import gather_rows  # noqa: E402


def window(fn, launches):
    """ms per call over `launches` back-to-back calls (device events)."""
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
        out["tb_per_s_over_model"] = model_bytes / (ms * 1e-3) / 1e12
    return out


def point(F, R, M, k, seed, launches, windows, chunk_bytes):
    dev = F.device
    n, d = F.shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    query = torch.randperm(n, device=dev, generator=gen)[:R].sort().values.contiguous()
    ptr = torch.arange(R + 1, device=dev, dtype=torch.int64)
    cand_ptr, out_ptr = ptr * M, ptr * k
    cand = A.sample_distinct(query, cand_ptr, n, seed)
    gather_bytes = R * M * d * 4
    model = gather_bytes + R * d * 4
    ids_per_chunk = max(M, chunk_bytes // (d * 4) // M * M)
    buf = torch.empty((min(ids_per_chunk, R * M), d), dtype=torch.float32, device=dev)
    rows_per_chunk = ids_per_chunk // M

    def select():
        return A.knn_select(F, query, cand_ptr, cand, out_ptr)

    def gather():
        for a in range(0, R * M, ids_per_chunk):
            ids = cand[a:a + ids_per_chunk]
            gather_rows(F, ids, out=buf[:ids.numel()])

    def composition():
        out = []
        for a in range(0, R, rows_per_chunk):
            q = query[a:a + rows_per_chunk]
            c = cand[a * M:(a + q.numel()) * M]
            diff = F.index_select(0, c).view(q.numel(), M, d)
            diff -= F.index_select(0, q).unsqueeze(1)
            pos = torch.linalg.vector_norm(diff, dim=2).topk(k, dim=1, largest=False, sorted=True).indices
            out.append(c.view(q.numel(), M).gather(1, pos))
            del diff
        return torch.cat(out).flatten()

    def sampler():
        return A.sample_distinct(query, cand_ptr, n, seed)

    runs = {"select": select, "gather": gather, "composition": composition, "sampler": sampler}
    res = {"d": d, "R": R, "M": M, "k": k, "gathered_bytes": gather_bytes, "model_bytes": model,
           "gather_chunk_ids": ids_per_chunk, "composition_chunk_rows": rows_per_chunk}
    sel = select()
    ref = composition()
    res["composition_ids_equal_fraction"] = float((sel == ref).double().mean())
    del sel, ref
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(windows):
        for name, fn in runs.items():
            times[name].append(window(fn, launches))
    res["select"] = summary(times["select"], model)
    res["gather"] = summary(times["gather"], gather_bytes)
    res["gather"]["note"] = "rate over the bytes read; the same bytes are written again"
    res["composition"] = summary(times["composition"], model)
    res["sampler"] = summary(times["sampler"])
    res["sampler"]["ids_per_s"] = R * M / (res["sampler"]["ms"] * 1e-3)
    res["select"]["peak_bytes"] = peak_of(select)
    res["composition"]["peak_bytes"] = peak_of(composition)
    res["select_rate_over_gather_rate"] = res["select"]["tb_per_s_over_model"] / res["gather"]["tb_per_s_over_model"]
    res["composition_over_select"] = res["composition"]["ms"] / res["select"]["ms"]
    return res


def end_to_end(F, edges, L, seed, runs):
    dev = F.device
    n = F.shape[0]
    gen = torch.Generator(device=dev).manual_seed(seed)
    row = torch.randint(0, n, (edges,), device=dev, generator=gen)
    col = torch.randint(0, n, (edges,), device=dev, generator=gen)
    out, chosen = A.edge_augment(row, col, n, F, degree_level=L, seed=seed, return_selected=True)
    torch.cuda.synchronize()
    secs = []
    for _ in range(runs):
        t0 = time.perf_counter()
        A.edge_augment(row, col, n, F, degree_level=L, seed=seed)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return {"n": n, "d": F.shape[1], "input_edges": edges, "degree_level": L, "low_degree_rows": chosen.nodes.numel(),
            "candidates": chosen.cand.numel(), "selected": chosen.sel.numel(), "output_edges": out.shape[1],
            "seconds": statistics.median(secs), "seconds_runs": secs,
            "what": "edge_augment(candidates=None) on device inputs, host clock around a device synchronise"}


def replay_points(runs):
    path = os.path.join(HERE, "..", "tests", "golden", "edge_augment.npz")
    if not os.path.exists(path):
        return []
    g = np.load(path)
    out = []
    for name in sorted({k.split("__", 1)[0] for k in g.files}):
        row = torch.from_numpy(g[name + "__row"].astype(np.int64))
        col = torch.from_numpy(g[name + "__col"].astype(np.int64))
        F = torch.from_numpy(g[name + "__features"])
        n, L = int(g[name + "__n"]), int(g[name + "__L"])
        secs, host = [], []
        for _ in range(runs + 1):
            random.seed(int(g[name + "__seed"]))
            t0 = time.perf_counter()
            e = A.edge_augment(row, col, n, F, degree_level=L, candidates="reference")
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            random.seed(int(g[name + "__seed"]))
            t0 = time.perf_counter()
            A.reference_candidates(row.numpy(), col.numpy(), n, L)
            host.append(time.perf_counter() - t0)
        out.append({"case": name, "n": n, "degree_level": L, "low_degree_rows": int(g[name + "__nodes"].size),
                    "equals_reference_edge_index": bool(np.array_equal(e.numpy(), g[name + "__edge_index"].astype(np.int64))),
                    "seconds": statistics.median(secs[1:]), "host_replay_seconds": statistics.median(host[1:]),
                    "what": 'edge_augment(candidates="reference") on host inputs: the host replay of the reference\'s '
                            "draw (host_replay_seconds of it) plus copies and the device selection; not the "
                            "reference's own loop"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "edge_augment_probe.json"))
    ap.add_argument("--n", type=int, default=2449029)
    ap.add_argument("--d", type=int, nargs="+", default=[263, 303])
    ap.add_argument("--R", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--M", type=int, nargs="+", default=[100, 300])
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--chunk-gib", type=float, default=8.0, help="gather buffer / composition chunk, GiB")
    ap.add_argument("--e2e-edges", type=int, default=1200000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_augment_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    points, e2e = [], []
    for d in a.d:
        gen = torch.Generator(device=dev).manual_seed(d)
        F = torch.randn((a.n, d), device=dev, generator=gen)
        for R in a.R:
            for M in a.M:
                r = point(F, min(R, a.n), M, max(1, M // 100), 1000 + M, a.launches, a.windows,
                          int(a.chunk_gib * 2 ** 30))
                points.append(r)
                print(json.dumps({k: (round(v["ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
                torch.cuda.empty_cache()
        e2e.append(end_to_end(F, a.e2e_edges, 1, 7, 3))
        print(json.dumps(e2e[-1]), flush=True)
        del F
        torch.cuda.empty_cache()
    res = {"what": "edge augmentation: srg_knn_select_f32 vs srg_gather_rows_f32 over the same ids vs the torch "
                   "composition, the sampler, and edge_augment end to end; same process, same tensors, alternating windows",
           "n": a.n, "launches_per_window": a.launches, "windows": a.windows, "library": _lib.version(),
           "device": torch.cuda.get_device_name(0), "points": points, "end_to_end": e2e,
           "reference_replay": replay_points(3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
