"""Golden fixtures for edge augmentation: the REFERENCE's own edge_augument, seeded, on small graphs
(development container only).

    python tests/golden/make_golden_edge_augment.py

Imports data_augument.edge_augument, unmodified, from the reference tree (make_golden.py's REF_SSRG).  Three
things happen outside the reference's files:
  * stub modules stand in for packages that data_augument.py imports at module top but edge_augument never
    calls and that are absent here: the fixed list ABSENT below and nothing else.  A finder at the end of
    sys.meta_path answers for those names only, and only after every real finder has passed; any other
    missing package fails the import, so that nothing edge_augument needs is ever replaced by a stub;
  * sys.argv is cut to one element before the import, because configs/*.py parse it;
  * data_augument.generate_numbers is wrapped to record what it returns (the wrapper calls the reference's
    function and changes nothing), and data_augument_args.degree_level is set per case.
Per case random.seed(seed) is called, then edge_augument(dataset, features), then random.random() once.
Only data leaves this script, to tests/golden/edge_augment.npz: the edges, features, degree_level and
seed, the recorded candidate lists in visiting order, the reference's edge_index, that next
random.random(), and ref_seconds: the wall time of the reference's call on the CPU that generated the file
(the recording wrapper included; one run, a label for DESIGN.md §5.9 and no test's input).

Every low-degree row of every case must be separated, so that the selection does not depend on the
summation order of the distance: with distances recomputed in fp64 from the fp32 inputs, the need-th and
(need+1)-th smallest differ by more than 2 (d + 4) 2^-24 relative to the larger -- twice the bound
(d/2 + 2) 2^-24 that any fp32 evaluation of the formula obeys -- and no two of the need + 1
smallest are equal.  A case that fails gets another seed, never a weaker check.
"""
import importlib.abc
import importlib.machinery
import os
import random
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N_SYNTH, D_GAUSS, D_SOFT = 600, 16, 7
# packages the reference imports at module top on this path and that are not installed here: a fixed list
ABSENT = frozenset({"torch_geometric", "ogb", "datasets", "torch_sparse", "torch_scatter", "munkres", "pygsp"})


class _Anything:
    """What a stub module hands out for any name: callable, subclassable, never used."""
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return _Anything()


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: asked only for modules nothing else found; answers for ABSENT only."""
    made = []

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] not in ABSENT:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        self.made.append(spec.name)
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass


def import_reference_edge_augument():
    sys.dont_write_bytecode = True
    sys.argv = sys.argv[:1]
    sys.path.insert(0, MG.REF_SSRG)
    finder = _StubFinder()
    sys.meta_path.append(finder)
    try:
        import data_augument      # a package missing beyond ABSENT raises ModuleNotFoundError here
    finally:
        sys.meta_path.remove(finder)
    print("stubbed:", sorted(set(n.split(".")[0] for n in finder.made)))
    return data_augument


class _Edge:
    def __init__(self, row, col):
        self.row, self.col = row, col


class _Dataset:
    def __init__(self, row, col, n):
        self.edge = _Edge(torch.from_numpy(row), torch.from_numpy(col))
        self.x = np.zeros((n, 1), dtype=np.float32)


def synthetic_graph(seed):
    """600 nodes: 40 isolated, the rest on a random graph thin enough to leave degree-1 and degree-2
    nodes, one self loop and one duplicate edge; features = 16 Gaussian columns and a 7-column softmax."""
    rng = np.random.default_rng(seed)
    n = N_SYNTH
    live = np.arange(40, n)
    e = 520
    row = rng.choice(live, e)
    col = rng.choice(live, e)
    keep = row != col
    row, col = row[keep], col[keep]
    row = np.concatenate([row, [57], [row[0]]]).astype(np.int64)      # a self loop, a duplicate edge
    col = np.concatenate([col, [57], [col[0]]]).astype(np.int64)
    hidden = rng.standard_normal((n, D_GAUSS)).astype(np.float32)
    logits = torch.from_numpy(rng.standard_normal((n, D_SOFT)).astype(np.float32))
    feats = np.concatenate([hidden, torch.softmax(logits, dim=1).numpy()], axis=1).astype(np.float32)
    return row, col, n, feats


def cora_graph(seed):
    torch.serialization.add_safe_globals([range])
    raw = os.path.join(MG.DATA, "cora_0_0.7", "raw")
    e = torch.load(os.path.join(raw, "edge_index.pt"), weights_only=True).numpy().astype(np.int64)
    n = int(torch.load(os.path.join(raw, "label.pt"), weights_only=True).shape[0])
    rng = np.random.default_rng(seed)
    hidden = rng.standard_normal((n, D_GAUSS)).astype(np.float32)
    logits = torch.from_numpy(rng.standard_normal((n, D_SOFT)).astype(np.float32))
    feats = np.concatenate([hidden, torch.softmax(logits, dim=1).numpy()], axis=1).astype(np.float32)
    return e[0].copy(), e[1].copy(), n, feats


def check_separated(feats, L, row, col, n, recorded):
    deg = np.bincount(np.concatenate([row, col]), minlength=n)
    X = feats.astype(np.float64)
    d = feats.shape[1]
    worst = np.inf
    for node, ids in recorded:
        need = int(L - deg[node])
        assert need > 0 and len(ids) == 100 * need and node not in ids and len(set(ids)) == len(ids)
        dist = np.sort(np.sqrt(((X[node] - X[np.asarray(ids)]) ** 2).sum(axis=1)))
        head = dist[:need + 1]
        assert np.all(np.diff(head) > 0), f"node {node}: equidistant candidates at the boundary"
        gap = (head[need] - head[need - 1]) / head[need]
        assert gap > 2 * (d + 4) * 2.0 ** -24, f"node {node}: boundary gap {gap:.3e} not separated"
        worst = min(worst, gap)
    return worst


def run_case(DA, recorded, name, graph, L, seed, arrs, ids_dtype):
    row, col, n, feats = graph
    DA.data_augument_args.degree_level = L
    recorded.clear()
    random.seed(seed)
    t0 = time.perf_counter()
    edge_index = DA.edge_augument(_Dataset(row, col, n), torch.from_numpy(feats))
    seconds = time.perf_counter() - t0
    after = random.random()
    worst = check_separated(feats, L, row, col, n, recorded)
    nodes = np.asarray([node for node, _ in recorded], dtype=np.int64)
    lens = np.asarray([len(ids) for _, ids in recorded], dtype=np.int64)
    ids = np.concatenate([np.asarray(i, dtype=np.int64) for _, i in recorded]) if recorded else np.zeros(0, np.int64)
    assert ids.max(initial=0) <= np.iinfo(ids_dtype).max
    arrs.update({f"{name}__row": row.astype(np.int16 if n < 32768 else np.int32),
                 f"{name}__col": col.astype(np.int16 if n < 32768 else np.int32),
                 f"{name}__features": feats, f"{name}__n": np.int64(n), f"{name}__L": np.int64(L),
                 f"{name}__seed": np.int64(seed), f"{name}__nodes": nodes.astype(ids_dtype),
                 f"{name}__cand_ptr": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                 f"{name}__cand": ids.astype(ids_dtype),
                 f"{name}__edge_index": edge_index.numpy().astype(np.int16 if n < 32768 else np.int32),
                 f"{name}__random_after": np.float64(after), f"{name}__ref_seconds": np.float64(seconds)})
    print(f"{name}: n={n} L={L} seed={seed}: {len(recorded)} low-degree nodes, {ids.size} candidates, "
          f"E={edge_index.shape[1]}, smallest boundary gap {worst:.3e} "
          f"(bound {2 * (feats.shape[1] + 4) * 2.0 ** -24:.3e}); the reference's host loop took {seconds:.3f} s "
          f"on this CPU (recording included)")


def main():
    DA = import_reference_edge_augument()
    recorded = []
    ref_generate = DA.generate_numbers

    def recording(count, node, numbers):
        out = ref_generate(count, node, numbers)
        recorded.append((int(node), [int(v) for v in out]))
        return out

    DA.generate_numbers = recording
    arrs = {}
    synth = synthetic_graph(20261)
    run_case(DA, recorded, "warm_up", synth, 1, 10, {}, np.int16)     # torch's first calls: kept out of ref_seconds
    run_case(DA, recorded, "synth600_L3", synth, 3, 11, arrs, np.int16)
    run_case(DA, recorded, "synth600_L1", synth, 1, 12, arrs, np.int16)
    path = os.path.join(HERE, "edge_augment.npz")
    np.savez_compressed(path, **arrs)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                  if f.endswith(".npz") and f != "edge_augment.npz")
    with_cora = dict(arrs)
    run_case(DA, recorded, "cora_0_0.7_L2", cora_graph(20262), 2, 13, with_cora, np.int16)
    np.savez_compressed(path, **with_cora)
    if os.path.getsize(path) > largest:      # the cora case only if the file stays within the largest fixture
        np.savez_compressed(path, **arrs)
        print("cora_0_0.7 left out: the file would exceed", largest, "bytes")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
