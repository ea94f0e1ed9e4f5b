#!/usr/bin/env python3
"""GAMLP's recursive hop attention (IterateLearnableWeightedMessageOp "recursive", H = 11 hops, d = 128): the
fused device path (op.fused = True: srg_hop_recur_scores_f32, srg_hop_recur_attend_f32,
srg_hop_recur_attend_grad_f32, srg_hop_recur_scores_grad_f32) next to the unchanged torch composition on the
same device tensors, forward and forward + backward, in one process, windows of the two alternating; each fused
entry on its own; and srg_hop_accumulate_f32 ADD over a panel as large as the whole hop list, the streaming rate
of the same run.

Bytes of the fused path, by its panel passes (n * d * 4 each): forward H (scores) + H (attend) + 1 (out);
backward H + 1 (attend gradient: the hops and G) + H (parameter gradient).  The per-row vectors (the dot
products, the triangle of weights, the gradients) are not in the model.  Device-event timing; every window is
`launches` back-to-back calls after a warm-up of the same shape.  Needs a HIP device.

    python tools/hop_recursive_probe.py [--out profiles/hop_recursive_probe.json] [--n 20000 200000]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "scalable-roubust-gnn_amd"))

import torch  # noqa: E402

from operators.message_operator.iterate_learnable_weighted_message_op import IterateLearnableWeightedMessageOp  # noqa: E402
from srgnn import _lib  # noqa: E402


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
    """Peak allocation of one call beyond what is allocated before it, bytes."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def entries(hops, op, G, launches, windows):
    """ms per call of each C entry on its own (the fused path's four steps)."""
    dev = hops[0].device
    n, d = hops[0].shape
    T = H = len(hops)
    ptrs = (ctypes.c_void_p * T)(*[h.data_ptr() for h in hops])
    lds = (ctypes.c_int64 * T)(*[h.stride(0) for h in hops])
    w, b = op.learnable_weight.weight.detach().view(-1), op.learnable_weight.bias.detach()
    zp, zq = torch.empty(H * n, device=dev), torch.empty(H * n, device=dev)
    dzp, dzq = torch.empty(H * n, device=dev), torch.empty(H * n, device=dev)
    work = torch.empty((H * (H + 1) // 2 + H) * n, device=dev)
    P = torch.empty((n, H), device=dev)
    out = torch.empty((n, d), device=dev)
    dw, db = torch.empty(2 * d, device=dev), torch.empty(1, device=dev)
    nbytes = ctypes.c_int64(0)
    _lib.check(_lib.lib().srg_hop_recur_scores_grad_scratch_bytes(n, d, H, ctypes.byref(nbytes)), "scratch")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    st = _lib.stream(dev)
    steps = {
        "scores": lambda: _lib.call(dev, "srg_hop_recur_scores_f32", ptrs, lds, T, H, w.data_ptr(), zp.data_ptr(),
                                    zq.data_ptr(), n, d, st),
        "attend": lambda: _lib.call(dev, "srg_hop_recur_attend_f32", ptrs, lds, T, H, zp.data_ptr(), zq.data_ptr(),
                                    b.data_ptr(), work.data_ptr(), P.data_ptr(), out.data_ptr(), d, n, d, st),
        "attend_grad": lambda: _lib.call(dev, "srg_hop_recur_attend_grad_f32", ptrs, lds, T, H, G.data_ptr(), d,
                                         zq.data_ptr(), work.data_ptr(), dzp.data_ptr(), dzq.data_ptr(), n, d, st),
        "scores_grad": lambda: _lib.call(dev, "srg_hop_recur_scores_grad_f32", ptrs, lds, T, H, dzp.data_ptr(),
                                         dzq.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), n, d, st),
    }
    passes = {"scores": H, "attend": H + 1, "attend_grad": H + 1, "scores_grad": H}
    for fn in steps.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(windows):
        for k, fn in steps.items():
            times[k].append(window(fn, launches))
    res = {}
    for k in steps:
        ms = statistics.median(times[k])
        res[k] = {"ms": ms, "panel_passes": passes[k], "tb_per_s": passes[k] * n * d * 4 / (ms * 1e-3) / 1e12}
    return res


def shape(n, d, H, launches, windows, composition):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(n)
    hops = [torch.randn((n, d), device=dev, generator=gen)]
    for _ in range(1, H):
        hops.append(0.6 * hops[-1] + 0.4 * torch.randn((n, d), device=dev, generator=gen))
    G = torch.randn((n, d), device=dev, generator=gen)
    torch.manual_seed(0)
    op = IterateLearnableWeightedMessageOp(0, H, "recursive", d).to(dev)

    def fwd(fused):
        op.fused = fused
        with torch.no_grad():
            return op.aggregate(list(hops))

    def fwd_bwd(fused):
        op.fused = fused
        op.zero_grad(set_to_none=True)
        op.aggregate(list(hops)).backward(G)

    panel = n * d * 4
    work_bytes = (H * (H + 1) // 2 + H) * n * 4
    res = {"n": n, "d": d, "H": H, "kind": "recursive", "hop_list_bytes": H * panel,
           "fused_forward_bytes": (2 * H + 1) * panel, "fused_backward_bytes": (2 * H + 1) * panel,
           "fused_work_buffer_bytes": work_bytes}
    runs = {"fused_forward": lambda: fwd(True), "fused_forward_backward": lambda: fwd_bwd(True)}
    if composition:
        try:
            fwd_bwd(False)
            torch.cuda.synchronize()
            runs["composition_forward"] = lambda: fwd(False)
            runs["composition_forward_backward"] = lambda: fwd_bwd(False)
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
        res[k + "_ms"] = statistics.median(times[k])
        res[k + "_ms_windows"] = times[k]
    res["fused_forward_backward_peak_bytes"] = peak_of(runs["fused_forward_backward"])
    if "composition_forward_backward" in runs:
        res["composition_forward_backward_peak_bytes"] = peak_of(runs["composition_forward_backward"])
        res["speedup_forward"] = res["composition_forward_ms"] / res["fused_forward_ms"]
        res["speedup_forward_backward"] = res["composition_forward_backward_ms"] / res["fused_forward_backward_ms"]
    res["fused_forward_tb_per_s"] = res["fused_forward_bytes"] / (res["fused_forward_ms"] * 1e-3) / 1e12
    res["fused_forward_backward_tb_per_s"] = (res["fused_forward_bytes"] + res["fused_backward_bytes"]) / \
        (res["fused_forward_backward_ms"] * 1e-3) / 1e12
    op.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()
    res["entries"] = entries(hops, op, G, launches, windows)

    # the streaming yardstick of this run: accumulate ADD over a panel as large as the hop list
    rows = H * n
    acc, y = torch.zeros((rows, d), device=dev), torch.randn((rows, d), device=dev, generator=gen)
    st = _lib.stream(dev)

    def add():
        _lib.call(dev, "srg_hop_accumulate_f32", acc.data_ptr(), d, y.data_ptr(), d, rows, d, 1e-3, _lib.SRG_ACC_ADD, st)

    add()
    torch.cuda.synchronize()
    t_add = [window(add, launches) for _ in range(windows)]
    ms = statistics.median(t_add)
    res["accumulate_add"] = {"rows": rows, "ms": ms, "bytes": 3 * rows * d * 4,
                             "tb_per_s": 3 * rows * d * 4 / (ms * 1e-3) / 1e12}
    res["fused_forward_backward_over_accumulate_rate"] = res["fused_forward_backward_tb_per_s"] / \
        res["accumulate_add"]["tb_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "hop_recursive_probe.json"))
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--H", type=int, default=11)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--no-composition", action="store_true", help="time the fused path alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hop_recursive_probe needs a HIP device")
    res = {"what": "IterateLearnableWeightedMessageOp recursive: fused device path vs the torch composition, same "
                   "process, same tensors, alternating windows", "launches_per_window": a.launches,
           "windows": a.windows, "library": _lib.version(),
           "shapes": [shape(n, a.d, a.H, a.launches, a.windows, not a.no_composition) for n in a.n]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
