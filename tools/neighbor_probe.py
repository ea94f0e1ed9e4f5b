#!/usr/bin/env python3
"""Neighbour sampling and the GraphSAGE step (srgnn.neighbor, srgnn.sage) on the products-shaped
and arxiv-shaped synthetic graphs (R-MAT, symmetric, Â at r = 0.5), in one process on the same tensors, warmed,
windows alternating as tools/cluster_probe.py takes them:

  (a) sample_f10 / sample_f25   srg_csr_sample_f32 alone (ptr formed, outputs allocated before the window) over a
      slice                     shuffled batch of min(200,000, n) rows without the longest row; `slice` is
      *_longest                 srg_csr_induced_f32's two phases as a row slice (pos NULL) of the same rows, the
      copy                      copy-everything bound; *_longest the same for a batch that holds the longest row;
                                copy is dst.copy_(src) of the sampler's model bytes at fanout 10
  (b) neighbors_call / block    sample_neighbors and sample_block end to end on that batch at fanout 10 (batch_rows,
                                the counts, cumsum, the host read, the launch; block adds the frontier)
  (c) loader_batch              one NeighborLoader batch of 1,024 seeds, sizes = [25, 10]
  (d) sage_step                 forward, loss and backward of the two-layer SAGE (d -> 256 -> 47) on that batch
                                (features gathered with gather_rows), with its peak temporaries

The sampler's byte model: 16 B (nodes and ptr) + 4 nnzB ids read + (4 + 4) nnzB written (+ 8 nnzB with entry ids;
the values' 4 nnzB read are counted with the ids' as the issue's model counts them: 16 B + 4 nnzB + 8 nnzB).
Device-event timing; spread = (max - min) / median.  Nothing is fixed in advance: the file records what was
measured.  Needs a HIP device.

    python tools/neighbor_probe.py [--out profiles/neighbor_probe.json] [--graphs products,arxiv]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "scalable-roubust-gnn_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from cluster_probe import alternate, peak_of, summary  # noqa: E402
from srgnn import _lib, synth  # noqa: E402
from srgnn import neighbor as NB  # noqa: E402
from srgnn.csr import DeviceCSR  # noqa: E402
from srgnn.normalize import sym_norm_binary  # noqa: E402
from srgnn.sage import SAGE  # noqa: E402
from srgnn.spmm import gather_rows  # noqa: E402

BATCH_ROWS, SEEDS, SIZES, HIDDEN, CLASSES, SEED = 200_000, 1024, [25, 10], 256, 47, 5


def sampler(A, ids, fanout):
    """(run, nnzB): the one launch over preallocated outputs."""
    dev, B = A.device, ids.numel()
    cnt = A.indptr[ids + 1] - A.indptr[ids]
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt.clamp(max=fanout), 0, out=ptr[1:])
    nnz = int(ptr[-1])
    idx = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)

    def run():
        _lib.call(dev, "srg_csr_sample_f32", A.indptr.data_ptr(), A.indices.data_ptr(), A.values.data_ptr(), A.n_rows,
                  ids.data_ptr(), B, fanout, SEED, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), None, _lib.stream(dev))
    return run, nnz


def row_slice(A, ids):
    """(run, L): srg_csr_induced_f32 as a row slice, both phases over preallocated arrays."""
    dev, B = A.device, ids.numel()
    cnt = torch.empty(B, dtype=torch.int64, device=dev)
    ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(A.indptr[ids + 1] - A.indptr[ids], 0, out=ptr[1:])
    L = int(ptr[-1])
    idx = torch.empty(L, dtype=torch.int32, device=dev)
    val = torch.empty(L, dtype=torch.float32, device=dev)
    args = (A.indptr.data_ptr(), A.indices.data_ptr(), A.values.data_ptr(), A.n_rows, A.n_cols, ids.data_ptr(), B, None)

    def run():
        _lib.call(dev, "srg_csr_induced_f32", 0, *args, cnt.data_ptr(), None, None, None, None, _lib.stream(dev))
        _lib.call(dev, "srg_csr_induced_f32", 1, *args, None, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), None,
                  _lib.stream(dev))
    return run, L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "neighbor_probe.json"))
    ap.add_argument("--graphs", default="products,arxiv")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_probe needs a HIP device")
    dev = torch.device("cuda", 0)
    res = {"what": "srg_csr_sample_f32 against the row slice of the same rows and a plain copy; sample_block, a "
                   "NeighborLoader batch and a SAGE step; same process, same tensors, alternating windows",
           "batch_rows": BATCH_ROWS, "seeds": SEEDS, "sizes": SIZES, "hidden": HIDDEN, "classes": CLASSES,
           "launches_per_window": a.launches, "windows": a.windows, "library": _lib.version(),
           "device": torch.cuda.get_device_name(0), "graphs": {}}

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
        lens = A.indptr[1:] - A.indptr[:-1]
        longest = int(lens.argmax())
        B = min(BATCH_ROWS, n - 1)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(SEED)).to(dev)
        perm = perm[perm != longest]
        ids = perm[:B].contiguous()
        ids_long = torch.cat([ids[:B // 2], torch.tensor([longest], device=dev), ids[B // 2:B - 1]]).contiguous()
        X = synth.uniform_features_t(n, d, device=dev)

        s10, nnz10 = sampler(A, ids, 10)
        s25, nnz25 = sampler(A, ids, 25)
        sl, L = row_slice(A, ids)
        s10l, nnz10l = sampler(A, ids_long, 10)
        s25l, _ = sampler(A, ids_long, 25)
        sll, Ll = row_slice(A, ids_long)
        model = lambda nnz: 16 * B + 4 * nnz + 8 * nnz   # noqa: E731
        src = torch.empty(model(nnz10) // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)

        loader = NB.NeighborLoader(A, perm[:SEEDS].cpu(), SIZES, SEEDS, shuffle=False, seed=SEED)
        seeds = loader.seed_batches()[0].to(dev)
        batch = loader.sample(seeds, 0, 0)
        torch.manual_seed(SEED)
        model_nn = SAGE(d, HIDDEN, CLASSES, 2, 0.5).to(dev)
        y = torch.randint(0, CLASSES, (SEEDS,), device=dev)

        def sage_step():
            model_nn.zero_grad(set_to_none=True)
            out = model_nn(gather_rows(X, batch.n_id), batch.blocks)
            torch.nn.functional.nll_loss(out, y).backward()

        runs = {
            "sample_f10": s10, "sample_f25": s25, "slice": sl,
            "sample_f10_longest": s10l, "sample_f25_longest": s25l, "slice_longest": sll,
            "copy": lambda: dst.copy_(src),
            "neighbors_call": lambda: NB.sample_neighbors(A, ids, 10, SEED),
            "block": lambda: NB.sample_block(A, ids, 10, SEED),
            "loader_batch": lambda: loader.sample(seeds, 0, 0),
            "sage_step": sage_step,
        }
        tm, calls = alternate(runs, a.launches, a.windows)
        r = {"n": n, "nnz": int(A.indices.numel()), "d": d, "B": B, "L": L, "L_longest": Ll, "nnzB_f10": nnz10,
             "nnzB_f25": nnz25, "longest_row": int(lens.max()), "longest_row_in_batch": int(lens[ids].max()),
             "rows_cut_f10": int((lens[ids] > 10).sum()), "rows_cut_f25": int((lens[ids] > 25).sum()),
             "batch_n_id": int(batch.n_id.numel()), "batch_block_shapes": [[b.csr.n_rows, b.csr.n_cols, int(b.csr.indices.numel())] for b in batch.blocks],
             "calls_per_window": calls}
        r["sample_f10"] = summary(tm["sample_f10"], model(nnz10))
        r["sample_f25"] = summary(tm["sample_f25"], model(nnz25))
        r["sample_f10_longest"] = summary(tm["sample_f10_longest"], model(nnz10l))
        r["copy"] = summary(tm["copy"], model(nnz10) // 8 * 8)
        for k in ("sample_f25_longest", "slice", "slice_longest", "neighbors_call", "block", "loader_batch", "sage_step"):
            r[k] = summary(tm[k])
        for k in ("neighbors_call", "block", "loader_batch", "sage_step"):
            r[k + "_peak_bytes"] = peak_of(runs[k])
        r["slice_over_sample_f10"] = r["slice"]["ms"] / r["sample_f10"]["ms"]
        r["slice_over_sample_f25"] = r["slice"]["ms"] / r["sample_f25"]["ms"]
        r["slice_longest_over_sample_f10_longest"] = r["slice_longest"]["ms"] / r["sample_f10_longest"]["ms"]
        r["sample_f10_longest_over_sample_f10"] = r["sample_f10_longest"]["ms"] / r["sample_f10"]["ms"]
        r["sample_f10_rate_over_copy_rate"] = r["sample_f10"]["tb_per_s_over_model"] / r["copy"]["tb_per_s_over_model"]
        r["frontier_ms"] = r["block"]["ms"] - r["neighbors_call"]["ms"]
        r["frontier_over_kernel"] = r["frontier_ms"] / r["sample_f10"]["ms"]
        res["graphs"][name] = r
        print(json.dumps({name: {k: (round(v["ms"], 4) if isinstance(v, dict) and "ms" in v else v) for k, v in r.items()}}), flush=True)
        save()
        del A, X, runs, batch, loader, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
