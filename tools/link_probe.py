#!/usr/bin/env python3
"""Link classification's edge head (srgnn.link) on the products-shaped and arxiv-shaped synthetic
graphs (R-MAT, symmetric, Â at r = 0.5), in one process on the same tensors.  The query pairs are a random 10 % of
the stored entries (row, column); h = 256, C in {2, 47}.  Every case is warmed with 20 runs, then timed in windows
with device events: the median window and spread = (max - min) / median.

  (1) head_fwd / head_step      pair_linear forward and forward plus backward (EdgeBatch handed over) against the
      comp_fwd / comp_step      torch composition linear(cat(z[q0], z[q1])), with the peak temporaries of one step;
                                a composition that does not fit is recorded as such
  (2) gather_add / segment_sum  each entry alone over its byte model, beside gather_rows of P over the same 2E ids:
                                  gather_add   16 E (pairs) + 2 E C 4 (two half rows of P) + E C 4 (out) + 4 C
                                  segment_sum  8 (U + 1) + 16 E (slots) + 2 E C 4 (g, every row twice) + U 2C 4 (S)
                                  gather_rows  2E (8 + 2 * 2C 4)
  (3) gcn_off / gcn_on          GraphConvolution2's edge-head step (forward, loss, backward) with fused_edge_head off
                                and on (an EdgeBatch as query_edges)
  (4) loader_epoch              one EdgeBatchLoader epoch at batch 65,536 (every batch built, its incidence too), with
                                the build of one EdgeBatch and of its incidence stated separately

Nothing is fixed in advance: the file records what was measured.  Needs a HIP device.

    python tools/link_probe.py [--out profiles/link_probe.json] [--graphs products,arxiv]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "scalable-roubust-gnn_amd"))

import torch  # noqa: E402

from srgnn import _lib, synth  # noqa: E402
from srgnn import link as LK  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402
from srgnn.graph_conv import GraphConvOperator, GraphConvolution2  # noqa: E402
from srgnn.normalize import sym_norm_binary  # noqa: E402
from srgnn.spmm import gather_rows  # noqa: E402

HIDDEN, CLASSES, FRACTION, BATCH, WARM, SEED = 256, (2, 47), 0.1, 65_536, 20, 5


def timed(fn, windows, min_window_ms=20.0):
    """{ms, ms_windows, spread, calls}: WARM warm-up runs, then `windows` windows of enough calls to last about
    min_window_ms each."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window(k):
        ev[0].record()
        for _ in range(k):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / k

    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    calls = max(1, min(2000, int(min_window_ms / max(window(1), 1e-4)) + 1))
    ms = [window(calls) for _ in range(windows)]
    med = statistics.median(ms)
    return {"ms": med, "ms_windows": ms, "spread": (max(ms) - min(ms)) / med, "calls_per_window": calls}


def with_model(r, model_bytes):
    r["model_bytes"] = model_bytes
    r["tb_per_s_over_model"] = model_bytes / (r["ms"] * 1e-3) / 1e12
    return r


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def guarded(fn, windows):
    """timed(fn), or what kept it from running (a composition that does not fit in memory)."""
    try:
        r = timed(fn, windows)
        r["peak_bytes"] = peak_of(fn)
        return r
    except torch.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"does_not_fit": str(e).splitlines()[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "link_probe.json"))
    ap.add_argument("--graphs", default="products,arxiv")
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("link_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"what": "pair_linear against the torch composition, the two entries over their byte models beside gather_rows, "
                   "GraphConvolution2's edge-head step with the switch off and on, one EdgeBatchLoader epoch; same "
                   "process, same tensors",
           "hidden": HIDDEN, "classes": list(CLASSES), "query_fraction": FRACTION, "loader_batch": BATCH, "warm_up_runs": WARM,
           "windows": a.windows, "library": _lib.version(), "device": torch.cuda.get_device_name(0), "graphs": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for name in a.graphs.split(","):
        cfg = synth.CONFIGS[name]
        n, d = cfg["n"], cfg["d"]
        u, v = synth.rmat_undirected_t(n, cfg["n_edges"], seed=synth.RMAT_SEED, device=dev)
        ip, ix = synth.symmetric_csr_t(n, u, v)
        del u, v
        ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
        A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev)
        del ip, ix, vals
        nnz = A.indices.numel()
        E = int(nnz * FRACTION)
        gen = torch.Generator().manual_seed(SEED)
        pick = torch.randperm(nnz, generator=gen)[:E].to(dev)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), A.indptr[1:] - A.indptr[:-1], output_size=nnz)
        q = torch.stack([rows[pick], A.indices[pick].to(torch.int64)], dim=1).contiguous()
        del rows, pick
        t0 = time.perf_counter()
        batch = LK.EdgeBatch(q, n)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        batch.incidence()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        U = batch.num_nodes
        m = batch.inc_ptr[1:] - batch.inc_ptr[:-1]
        r = {"n": n, "nnz": nnz, "d": d, "E": E, "U": U, "E_over_U": E / U, "slots_max": int(m.max()), "slots_median": float(m.median()),
             "edge_batch_build_ms_first": (t1 - t0) * 1e3, "incidence_build_ms_first": (t2 - t1) * 1e3,
             "composition_buffer_bytes": E * 2 * HIDDEN * 4, "C": {}}
        r["edge_batch_build"] = timed(lambda: LK.EdgeBatch(q, n), a.windows)

        def build_incidence():
            batch._inc = None
            batch.incidence()
        r["incidence_build"] = timed(build_incidence, a.windows)
        torch.manual_seed(SEED)
        z0 = torch.randn(U, HIDDEN, device=dev)
        X = synth.uniform_features_t(n, d, device=dev)
        op = GraphConvOperator(A)
        local = batch.local

        for C in CLASSES:
            W0 = torch.randn(C, 2 * HIDDEN, device=dev) / (2 * HIDDEN) ** 0.5
            b0 = torch.randn(C, device=dev)
            g = torch.randn(E, C, device=dev)
            z, W, b = (x.clone().requires_grad_() for x in (z0, W0, b0))

            def head_fwd():
                with torch.no_grad():
                    return LK.pair_linear(z, batch, W, b)

            def comp_fwd():
                with torch.no_grad():
                    return torch.nn.functional.linear(torch.cat((z[local[:, 0]], z[local[:, 1]]), dim=-1), W, b)

            def step(fwd):
                def run():
                    z.grad = W.grad = b.grad = None
                    fwd().backward(g)
                return run
            head_step = step(lambda: LK.pair_linear(z, batch, W, b))
            comp_step = step(lambda: torch.nn.functional.linear(torch.cat((z[local[:, 0]], z[local[:, 1]]), dim=-1), W, b))
            c = {"head_fwd": guarded(head_fwd, a.windows), "comp_fwd": guarded(comp_fwd, a.windows),
                 "head_step": guarded(head_step, a.windows), "comp_step": guarded(comp_step, a.windows)}
            z.grad = W.grad = b.grad = None
            for k in ("fwd", "step"):
                if "ms" in c["comp_" + k]:
                    c[f"comp_{k}_over_head_{k}"] = c["comp_" + k]["ms"] / c["head_" + k]["ms"]

            P = torch.randn(U, 2 * C, device=dev)
            out = torch.empty(E, C, device=dev)
            S = torch.empty(U, 2 * C, device=dev)
            flat = local.reshape(-1).contiguous()
            rows_out = torch.empty(2 * E, 2 * C, device=dev)
            inc_ptr, inc_slot = batch.incidence()
            c["gather_add"] = with_model(timed(lambda: LK.pair_gather_add(P, local, b0, out=out), a.windows),
                                         16 * E + 2 * E * C * 4 + E * C * 4 + 4 * C)
            c["segment_sum"] = with_model(timed(lambda: LK.pair_segment_sum(g, inc_ptr, inc_slot, out=S), a.windows),
                                          8 * (U + 1) + 16 * E + 2 * E * C * 4 + U * 2 * C * 4)
            c["gather_rows"] = with_model(timed(lambda: gather_rows(P, flat, rows_out), a.windows), 2 * E * (8 + 2 * 2 * C * 4))
            del P, out, S, rows_out, flat

            torch.manual_seed(SEED)
            model = GraphConvolution2(d, HIDDEN, C, dropout=0.5).to(dev)
            model.adj = op

            def gcn(fused, qe):
                def run():
                    model.fused_edge_head, model.query_edges = fused, qe
                    model.zero_grad(set_to_none=True)
                    (model(X) * g).sum().backward()
                return run
            c["gcn_off"] = guarded(gcn(False, q), a.windows)
            c["gcn_on"] = guarded(gcn(True, batch), a.windows)
            if "ms" in c["gcn_off"]:
                c["gcn_off_over_gcn_on"] = c["gcn_off"]["ms"] / c["gcn_on"]["ms"]
            r["C"][str(C)] = c
            print(json.dumps({name: {C: {k: (round(v["ms"], 4) if isinstance(v, dict) and "ms" in v else v) for k, v in c.items()}}}),
                  flush=True)
            res["graphs"][name] = r
            save()
            del model, g, z, W, b
            torch.cuda.empty_cache()

        labels = torch.randint(0, 2, (E,), device=dev)
        loader = LK.EdgeBatchLoader(q, labels, n, BATCH, shuffle=True, generator=torch.Generator().manual_seed(SEED))
        one = q[:BATCH].contiguous()
        small = LK.EdgeBatch(one, n)

        def small_incidence():
            small._inc = None
            small.incidence()
        r["loader_batches"] = len(loader)
        r["loader_one_edge_batch"] = timed(lambda: LK.EdgeBatch(one, n), a.windows)
        r["loader_one_incidence"] = timed(small_incidence, a.windows)
        epochs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for bt, _, _ in loader:
                bt.incidence()
            torch.cuda.synchronize()
            epochs.append((time.perf_counter() - t0) * 1e3)
        r["loader_epoch_ms"] = {"ms": statistics.median(epochs), "ms_epochs": epochs}
        res["graphs"][name] = r
        print(json.dumps({name: {k: (round(v["ms"], 4) if isinstance(v, dict) and "ms" in v else v) for k, v in r.items() if k != "C"}}),
              flush=True)
        save()
        del A, X, op, batch, loader, q, z0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
