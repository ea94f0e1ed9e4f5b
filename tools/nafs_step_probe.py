#!/usr/bin/env python3
"""The NAFS step kernel (srg_hop_simweight_f32) next to srg_hop_accumulate_f32 ADD on a products-shaped
panel (n = 2,449,029, d = 128), in one process on the same panels, windows of the two alternating;
and one fused NAFS combination at K = 10 next to the `last` mode on the same operator.

By bytes the step is 4 panel passes (reads x0, y, acc; writes acc) against ADD's 3, so the expected
time ratio is 4/3.  Device-event timing; every window is `launches` back-to-back launches after a
warm-up of the same shape.  Needs a HIP device: there is no CPU path.

    python tools/nafs_step_probe.py [--out profiles/nafs_step_products.json] [--n N] [--d D]
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


def window(fn, launches):
    """ms per launch over `launches` back-to-back launches (device events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "nafs_step_products.json"))
    ap.add_argument("--n", type=int, default=synth.CONFIGS["products"]["n"])
    ap.add_argument("--d", type=int, default=synth.CONFIGS["products"]["d"])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--no-fused", action="store_true", help="skip the K = 10 fused combination on the products graph")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nafs_step_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    n, d = a.n, a.d
    x0 = synth.uniform_features_t(n, d, device=dev)
    y = synth.uniform_features_t(n, d, seed=7, device=dev)
    acc = torch.zeros((n, d), dtype=torch.float32, device=dev)
    n0, z = torch.empty(n, device=dev), torch.empty(n, device=dev)
    st = _lib.stream(dev)

    def step(flags=0):
        _lib.call(dev, "srg_hop_simweight_f32", x0.data_ptr(), d, y.data_ptr(), d, n0.data_ptr(), acc.data_ptr(), d,
                  z.data_ptr(), None, 0, n, d, flags, st)

    def add():
        _lib.call(dev, "srg_hop_accumulate_f32", acc.data_ptr(), d, y.data_ptr(), d, n, d, 1e-3, _lib.SRG_ACC_ADD, st)

    _lib.call(dev, "srg_hop_simweight_f32", None, d, x0.data_ptr(), d, n0.data_ptr(), acc.data_ptr(), d, z.data_ptr(),
              None, 0, n, d, _lib.SRG_SIM_INIT | _lib.SRG_SIM_HOP0, st)
    for _ in range(3):
        step()
        add()
    torch.cuda.synchronize()
    t_step, t_add = [], []
    for _ in range(a.windows):
        t_add.append(window(add, a.launches))
        t_step.append(window(step, a.launches))
    panel = n * d * 4
    m_step, m_add = statistics.median(t_step), statistics.median(t_add)
    res = {
        "what": "srg_hop_simweight_f32 (NAFS step) vs srg_hop_accumulate_f32 ADD, same process, same panels",
        "n": n, "d": d, "launches_per_window": a.launches, "windows": a.windows,
        "step_ms": m_step, "step_ms_windows": t_step,
        "accumulate_add_ms": m_add, "accumulate_add_ms_windows": t_add,
        "accumulate_add_spread": (max(t_add) - min(t_add)) / m_add,
        "ratio_step_over_add": m_step / m_add, "ratio_expected_by_bytes": 4.0 / 3.0,
        "step_bytes": 4 * panel, "step_tb_per_s": 4 * panel / (m_step * 1e-3) / 1e12,
        "accumulate_add_bytes": 3 * panel, "accumulate_add_tb_per_s": 3 * panel / (m_add * 1e-3) / 1e12,
        "library": _lib.version(),
    }
    del x0, y, acc, n0, z
    torch.cuda.empty_cache()
    if not a.no_fused:
        from srgnn import graphs
        from srgnn.aggregate import fused_combine
        from srgnn.csr import DeviceCSR

        class Msg:
            def __init__(self, aggr):
                self.aggr_type, self.start, self.end = aggr, None, None

        ip, ix, vals, gn, gd, K = graphs.build("products", dev)
        A = DeviceCSR.from_tensors(ip, ix, vals, n_cols=gn, device=dev)
        del ip, ix, vals
        X = synth.uniform_features_t(gn, gd, device=dev)
        K = 10
        runs = {"last": Msg("last"), "over_smooth": Msg("over_smooth_dis_weighted")}
        times = {k: [] for k in runs}
        for k, m in runs.items():
            fused_combine(A, X, K, m)               # warm-up: plan build, allocator
        torch.cuda.synchronize()
        for _ in range(3):
            for k, m in runs.items():
                times[k].append(window(lambda: fused_combine(A, X, K, m), 1))
        res["fused_K10_products"] = {
            "what": "srgnn.aggregate.fused_combine (the device part of GraphOp.propagate_aggregate), ms per call",
            "n": gn, "d": gd, "K": K, "nnz": A.nnz,
            "last_ms": statistics.median(times["last"]), "last_ms_runs": times["last"],
            "over_smooth_ms": statistics.median(times["over_smooth"]), "over_smooth_ms_runs": times["over_smooth"],
        }
        res["fused_K10_products"]["ratio_over_smooth_over_last"] = \
            res["fused_K10_products"]["over_smooth_ms"] / res["fused_K10_products"]["last_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
