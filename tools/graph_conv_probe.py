#!/usr/bin/env python3
"""GCN's sparse products at products scale (an R-MAT graph of n = 2,449,029 nodes and 61,859,012 undirected
edges, Â at r = 0.5; hidden 256, 47 classes; a batch of 196,615 unique shuffled rows, 8 % of the nodes), in
one process on the same tensors, windows of the alternatives alternating:

  step       the four sparse products of a training step -- Â·[n, 256], Â·[n, 47] forward and the two
             transposed products backward -- through GraphConvOperator (graph_conv with autograd) against
             torch.sparse.mm on the coalesced COO tensor on the same device, forward and backward: the
             reference's own path.  Time and peak temporaries (torch.cuda.max_memory_allocated beyond what
             is allocated before the call).
  rows       srg_gconv_rows_f32 against the full hop it replaces, and srg_gconv_rows_adjoint_f32 against the
             full transposed hop of the gradient scattered into n rows (the scatter timed on its own), d = 47;
             and forward + backward of graph_conv(op, x, rows) against graph_conv(op, x)[rows].
  adjoint    its achieved rate over the byte model 4·nnz + 4·n bytes of ids and positions plus 4·d bytes per
             member entry, and the member bytes alone against srg_gather_rows_f32 over the same member ids.

Device-event timing; every window is `launches` back-to-back calls after a warm-up of the same shape; spread =
(max - min) / median over the windows.  Rates are model bytes over the time of the whole call: end-to-end
rates, not a kernel's.  Before timing, the row entries are compared bit for bit with the full path at the
timed size.  Nothing is fixed in advance: the file records what was measured, also where the row path does
not win.  Results are written after every section, so a run cut short keeps what it has.  Needs a HIP device.

    python tools/graph_conv_probe.py [--out profiles/graph_conv_probe.json]
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
from srgnn import graph_conv as GC  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402
from srgnn.normalize import sym_norm_binary  # noqa: E402
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


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "graph_conv_probe.json"))
    ap.add_argument("--n", type=int, default=synth.CONFIGS["products"]["n"])
    ap.add_argument("--edges", type=int, default=synth.CONFIGS["products"]["n_edges"])
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--batch", type=int, default=196615)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-torch-sparse", action="store_true", help="skip the torch.sparse.mm side of `step`")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_conv_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    n, B, dc, dh = a.n, min(a.batch, a.n), a.classes, a.hidden

    u, v = synth.rmat_undirected_t(n, a.edges, seed=synth.RMAT_SEED, device=dev)
    ip, ix = synth.symmetric_csr_t(n, u, v)
    del u, v
    ip, ix, vals = sym_norm_binary(ip, ix, n, 0.5)
    op = GC.GraphConvOperator.from_device_csr(DeviceCSR.from_tensors(ip, ix, vals, n_cols=n, device=dev))
    nnz = int(ix.numel())
    deg = ip[1:] - ip[:-1]
    res = {"what": "GCN's sparse products: GraphConvOperator vs torch.sparse.mm (COO), the row-restricted product "
                   "and its adjoint vs the full hops, the adjoint over its byte model and over gather_rows; same "
                   "process, same tensors, alternating windows",
           "n": n, "nnz": nnz, "longest_row": int(deg.max()), "median_row": int(deg.median()), "hidden": dh,
           "classes": dc, "batch": B, "transpose_kind": op.transpose_kind, "launches_per_window": a.launches,
           "windows": a.windows, "library": _lib.version(), "device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    gen = torch.Generator(device=dev).manual_seed(11)
    rows = torch.randperm(n, device=dev, generator=gen)[:B].contiguous()
    ids, pos, unique = GC.batch_rows(rows, n, dev)
    assert unique
    Xc = torch.randn((n, dc), device=dev, generator=gen)
    Gb = torch.randn((B, dc), device=dev, generator=gen)
    op.prepare(dc, 1)
    op.prepare(dh, 1)

    # ---- rows: the two entries against the full hops they replace ----------------------------------
    full_y = GC._hop(op.A, Xc)
    scattered = torch.zeros((n, dc), device=dev)
    scattered[ids] = Gb
    full_dx = GC._hop(op.At, scattered)
    res["rows_product_equals_full_rows_bitwise"] = same_bits(GC.rows_product(op.A, Xc, ids), full_y[ids])
    res["rows_adjoint_equals_full_adjoint_bitwise"] = same_bits(GC.rows_adjoint(op.At, pos, Gb), full_dx)
    del full_y, full_dx
    member = pos[op.At.indices.long()] >= 0
    n_member = int(member.sum())
    member_ids = pos[op.At.indices.long()][member].long().contiguous()
    del member
    in_batch = int(deg[ids].sum())
    out_y = torch.empty((B, dc), device=dev)
    out_n = torch.empty((n, dc), device=dev)
    gbuf = torch.empty((n_member, dc), device=dev)

    def scatter():
        scattered.zero_()
        scattered[ids] = Gb

    runs = {"rows_product": lambda: GC.rows_product(op.A, Xc, ids, out=out_y),
            "full_hop": lambda: GC.spmm.hop(op.A, Xc, out_n),
            "rows_adjoint": lambda: GC.rows_adjoint(op.At, pos, Gb, out=out_n),
            "full_adjoint_hop": lambda: GC.spmm.hop(op.At, scattered, out_n),
            "scatter_into_n_rows": scatter,
            "gather_member_rows": lambda: gather_rows(Gb, member_ids, out=gbuf)}
    tm = alternate(runs, a.launches, a.windows)
    adj_model = 4 * nnz + 4 * n + 4 * dc * n_member
    fwd_model = 8 * in_batch + 4 * dc * in_batch + 8 * B + 4 * dc * B
    r = {"d": dc, "entries_in_batch_rows": in_batch, "member_entries": n_member,
         "rows_product": summary(tm["rows_product"], fwd_model),
         "full_hop": summary(tm["full_hop"]),
         "rows_adjoint": summary(tm["rows_adjoint"], adj_model),
         "full_adjoint_hop": summary(tm["full_adjoint_hop"]),
         "scatter_into_n_rows": summary(tm["scatter_into_n_rows"]),
         "gather_member_rows": summary(tm["gather_member_rows"], 4 * dc * n_member)}
    r["gather_member_rows"]["note"] = "rate over the bytes read; the same bytes are written again"
    r["rows_product"]["model"] = "ids and values of the batch rows' entries, 4·d per entry gathered, rows and Y"
    r["rows_adjoint"]["model"] = "4·nnz + 4·n ids and positions, 4·d per member entry (values and dX not counted)"
    r["full_hop_over_rows_product"] = r["full_hop"]["ms"] / r["rows_product"]["ms"]
    r["full_adjoint_over_rows_adjoint"] = (r["full_adjoint_hop"]["ms"] + r["scatter_into_n_rows"]["ms"]) / r["rows_adjoint"]["ms"]
    r["adjoint_member_tb_per_s"] = 4 * dc * n_member / (r["rows_adjoint"]["ms"] * 1e-3) / 1e12
    r["adjoint_member_rate_over_gather_rows_rate"] = r["adjoint_member_tb_per_s"] / r["gather_member_rows"]["tb_per_s_over_model"]
    res["rows"] = r
    print(json.dumps({k: (round(v["ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}), flush=True)
    save()
    del gbuf, member_ids, out_y, out_n, scattered

    # ---- rows through autograd: the last layer's forward + backward ---------------------------------
    x = Xc.clone().requires_grad_(True)

    def layer_rows():
        x.grad = None
        GC.graph_conv(op, x, ids).backward(Gb)

    def layer_full():
        x.grad = None
        GC.graph_conv(op, x)[ids].backward(Gb)

    tm = alternate({"rows": layer_rows, "full_then_index": layer_full}, a.launches, a.windows)
    res["last_layer_fwd_bwd"] = {"rows": summary(tm["rows"]), "full_then_index": summary(tm["full_then_index"]),
                                 "rows_peak_bytes": peak_of(layer_rows), "full_then_index_peak_bytes": peak_of(layer_full)}
    res["last_layer_fwd_bwd"]["full_over_rows"] = res["last_layer_fwd_bwd"]["full_then_index"]["ms"] / \
        res["last_layer_fwd_bwd"]["rows"]["ms"]
    print(json.dumps({"last_layer_fwd_bwd": {k: (round(v["ms"], 3) if isinstance(v, dict) else v)
                                               for k, v in res["last_layer_fwd_bwd"].items()}}), flush=True)
    save()

    # ---- step: the four products, ours against torch.sparse.mm on the COO tensor --------------------
    Xh = torch.randn((n, dh), device=dev, generator=gen).requires_grad_(True)
    Gh = torch.randn((n, dh), device=dev, generator=gen)
    Gc = torch.randn((n, dc), device=dev, generator=gen)

    def step_with(mm):
        def step():
            Xh.grad = None
            x.grad = None
            mm(Xh).backward(Gh)
            mm(x).backward(Gc)
        return step

    ours = step_with(lambda t: GC.graph_conv(op, t))
    tm = alternate({"graph_conv": ours}, a.launches, a.windows)
    res["step"] = {"products": f"Â·[n,{dh}], Â·[n,{dc}] and their two transposed products",
                   "graph_conv": summary(tm["graph_conv"]), "graph_conv_peak_bytes": peak_of(ours)}
    save()
    if not a.no_torch_sparse:
        rows_e = torch.repeat_interleave(torch.arange(n, device=dev), deg, output_size=nnz)
        coo = torch.sparse_coo_tensor(torch.stack([rows_e, op.A.indices.long()]), op.A.values, (n, n)).coalesce()
        del rows_e
        theirs = step_with(lambda t: torch.sparse.mm(coo, t))
        y_ref = torch.sparse.mm(coo, Xc)
        y_our = GC._hop(op.A, Xc)
        res["step"]["max_abs_difference_to_torch_d47"] = float((y_ref - y_our).abs().max())
        del y_ref, y_our
        tm = alternate({"graph_conv": ours, "torch_sparse_mm": theirs}, a.launches, a.windows)
        res["step"].update({"graph_conv": summary(tm["graph_conv"]), "torch_sparse_mm": summary(tm["torch_sparse_mm"]),
                            "torch_sparse_mm_peak_bytes": peak_of(theirs)})
        res["step"]["torch_over_graph_conv"] = res["step"]["torch_sparse_mm"]["ms"] / res["step"]["graph_conv"]["ms"]
    print(json.dumps({"step": {k: (round(v["ms"], 3) if isinstance(v, dict) else v) for k, v in res["step"].items()}}),
          flush=True)
    save()


if __name__ == "__main__":
    main()
