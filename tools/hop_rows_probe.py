#!/usr/bin/env python3
"""Mini-batch hop attention over device-resident hop panels (GAMLP "jk" and GAMLP-R "recursive", T = 11 hops,
d = 128, panels of n = 2,449,029 rows, the products graph): forward + backward of one batch of B rows through

  (a) indexed      hop_attention(..., index=idx, check=False): the srg_hop_*_rows_f32 entries read the batch's
                   rows from the panels in place; `indexed_checked` is the same through the
                   operator's aggregate_rows, with the aminmax validation and its host sync;
  (b) gathered     srg_gather_rows_f32 of the T panels into fresh [B, d] copies, then the fused call on the
                   copies: the only way to feed a batch to the fused path before the index;
  (c) composition  index_select of the T panels, then the operator's unchanged torch composition.

In one process, on the same tensors, windows of the three alternating; for each B a shuffled and a sorted index.
Device-event timing; every window is `launches` back-to-back calls after a warm-up of the same shape; the
spread is (max - min) / median over the windows.  The byte model counts T*B*d*4 bytes as one unit: the indexed
path's four passes (scores, attend, attend gradient, parameter gradient) are 4 units, the gathers add 2 (one
random read, one streaming write).  GB/s is 4 units over the time of the whole call, autograd and allocations
included: an end-to-end rate, not a kernel's.  Before timing, the indexed and the gathered results are compared
bit for bit at the timed size.  Needs a HIP device.

    python tools/hop_rows_probe.py [--out profiles/hop_rows_probe.json] [--B 50000 200000]
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

from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp  # noqa: E402
from operators.message_operator.learnable_weighted_messahe_op import LearnableWeightedMessageOp  # noqa: E402
from srgnn import _lib  # noqa: E402
from srgnn.hop_attention import hop_attention, hop_attention_recursive  # noqa: E402


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
    """Peak allocation of one call beyond what is allocated before it, bytes (torch.cuda.max_memory_allocated)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def gather(feats, idx):
    """The parent's batch: T srg_gather_rows_f32 calls into fresh [B, d] copies."""
    dev = feats[0].device
    n, d = feats[0].shape
    st = _lib.stream(dev)
    out = []
    for f in feats:
        g = torch.empty((idx.numel(), d), dtype=torch.float32, device=dev)
        _lib.call(dev, "srg_gather_rows_f32", f.data_ptr(), f.stride(0), n, idx.data_ptr(), idx.numel(), g.data_ptr(), d,
                  d, st)
        out.append(g)
    return out


def point(kind, op, feats, idx, G, launches, windows, composition):
    T, d, B = len(feats), feats[0].shape[1], idx.numel()
    lin = op.learnable_weight

    def fused(panels, index):
        if kind == "recursive":
            return hop_attention_recursive(panels, T, lin.weight, lin.bias, index=index, check=False)
        return hop_attention(panels, 0, T, kind, lin.weight, lin.bias, index=index, check=False)

    def step(make):
        op.zero_grad(set_to_none=True)
        out = make()
        out.backward(G)
        return out

    def composed():
        op.fused = False
        return op.aggregate([f.index_select(0, idx) for f in feats])

    def checked():
        op.fused = True
        return op.aggregate_rows(feats, idx)

    runs = {"indexed": lambda: step(lambda: fused(feats, idx)),
            "indexed_checked": lambda: step(checked),
            "gathered": lambda: step(lambda: fused(gather(feats, idx), None))}
    unit = T * B * d * 4
    res = {"kind": kind, "B": B, "unit_bytes": unit, "model_bytes_indexed": 4 * unit, "model_bytes_gathered": 6 * unit}

    # faster and different is not faster: the same bits at the timed size
    a = runs["indexed"]().detach()
    ga = (lin.weight.grad.clone(), lin.bias.grad.clone())
    b = runs["gathered"]().detach()
    res["indexed_equals_gathered_bit_for_bit"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                      and torch.equal(ga[0].view(torch.int32), lin.weight.grad.view(torch.int32))
                                                      and torch.equal(ga[1].view(torch.int32), lin.bias.grad.view(torch.int32)))
    del a, b, ga
    if composition:
        try:
            step(composed)
            torch.cuda.synchronize()
            runs["composition"] = lambda: step(composed)
        except torch.OutOfMemoryError as e:
            res["composition"] = f"does not fit: {str(e).splitlines()[0]}"
            op.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():
            times[k].append(window(fn, launches))
    for k, fn in runs.items():
        ms = statistics.median(times[k])
        res[k] = {"ms": ms, "ms_windows": times[k], "spread": (max(times[k]) - min(times[k])) / ms,
                  "peak_bytes": peak_of(fn), "gb_per_s_over_4_units": 4 * unit / (ms * 1e-3) / 1e9}
        op.zero_grad(set_to_none=True)
    res["gathered_over_indexed"] = res["gathered"]["ms"] / res["indexed"]["ms"]
    res["peak_saved_bytes"] = res["gathered"]["peak_bytes"] - res["indexed"]["peak_bytes"]
    if "composition" in runs:
        res["composition_over_indexed"] = res["composition"]["ms"] / res["indexed"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "hop_rows_probe.json"))
    ap.add_argument("--n", type=int, default=2449029)
    ap.add_argument("--B", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--T", type=int, default=11)
    ap.add_argument("--kinds", nargs="+", default=["jk", "recursive"])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--no-composition", action="store_true", help="time the two fused paths alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hop_rows_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(a.n)
    feats = [torch.randn((a.n, a.d), device=dev, generator=gen)]
    for _ in range(1, a.T):
        nxt = torch.randn((a.n, a.d), device=dev, generator=gen)
        nxt.mul_(0.4).add_(feats[-1], alpha=0.6)
        feats.append(nxt)
    points = []
    for kind in a.kinds:
        torch.manual_seed(0)
        op = (IterateLearnableWeightedMessageOp(0, a.T, "recursive", a.d) if kind == "recursive"
              else LearnableWeightedMessageOp(0, a.T, kind, a.T - 1, a.d)).to(dev)
        for B in a.B:
            shuffled = torch.randperm(a.n, device=dev, generator=gen)[:B].contiguous()
            G = torch.randn((B, a.d), device=dev, generator=gen)
            for order, idx in (("shuffled", shuffled), ("sorted", shuffled.sort().values)):
                r = point(kind, op, feats, idx, G, a.launches, a.windows, not a.no_composition)
                r["order"] = order
                points.append(r)
                print(json.dumps({k: v for k, v in r.items() if not isinstance(v, dict)} |
                                 {k: round(v["ms"], 4) for k, v in r.items() if isinstance(v, dict)}), flush=True)
                torch.cuda.empty_cache()
    res = {"what": "forward + backward of one mini-batch over device-resident hop panels: indexed (in place) vs "
                   "gather-then-fused vs index_select + torch composition; same process, same tensors, alternating windows",
           "n_src": a.n, "d": a.d, "T": a.T, "launches_per_window": a.launches, "windows": a.windows,
           "library": _lib.version(), "device": torch.cuda.get_device_name(0), "points": points}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
