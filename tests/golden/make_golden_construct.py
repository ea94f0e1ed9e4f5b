"""Golden fixtures for construct_adj on weighted graphs: the REFERENCE's own Â where its fp64
arithmetic shows -- non-dyadic weights (the order of scipy's row sums), zero and negative degrees
(what sp.diags does with a zero factor).

    make -C oracle && python tests/golden/make_golden_construct.py      (development container only)

Runs, unmodified, operators.utils.adj_to_symmetric_norm and the construct_adj / propagate of
SymLaplacianGraphOp and PprGraphOp, imported as in make_golden.py.  Only data is written:
tests/golden/cw_*.npz (input CSR; per variant <kind>_r<r>_{indptr,indices,data} with kind sym /
ppr (alpha = 0.15) and fp64 data; for cw_sym the panel x and hop1..hop3 of SymLaplacianGraphOp(3,
r=0.5).propagate; the scipy and numpy versions) and their manifest.json entries.  The archives are
written with a fixed timestamp, so a re-run reproduces them byte for byte.

  cw_ladder      canonical, asymmetric, weights signed U[0.5, 1.5) (one sign in four negative, so
                 that the ladder rows keep a positive degree: a negative one makes its row and
                 column of Â NaN, whose bits pin nothing).  Row lengths of A + I walk
                 numpy's pairwise-sum boundaries (a row sum is a[0] + pairwise(a[1:])): every length
                 1..40, then 63..66, 72, 73, 120..131, 136..138, 256..259, 300, 511, 512, 513, 1023,
                 1024, 1025, 1032, 1033; the other rows hold the diagonal and at most one entry.
                 Every length 0..300 would take 45 k entries, past the 12 k a fixture here may hold; every length
                 is covered without a fixture by tests/test_construct_scipy_cpu.py against the
                 installed scipy.  No row of A + I is empty here (that takes a diagonal of -1, which
                 would keep the whole graph off the in-place A + I merge); cw_degenerate has them.
  cw_sym         canonical, structurally symmetric (srg_csr_mirror's fast path) with independent
                 weights U[0.1, 1) in both directions, n = 300, three isolated nodes, a stored
                 diagonal on some rows; carries the hop panels.
  cw_degenerate  signed integer weights, explicit zeros, diagonals of -1, rows of A + I that are
                 empty, sum to zero or sum to a negative degree; entries whose one factor is NaN
                 (negative degree, fractional r) and the other 0 (zero degree), which the reference
                 does not store.
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np
import scipy
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

ALPHA = 0.15
LADDER_LENGTHS = (list(range(1, 41)) + [63, 64, 65, 66, 72, 73] + list(range(120, 132)) + [136, 137, 138]
                  + [256, 257, 258, 259, 300, 511, 512, 513, 1023, 1024, 1025, 1032, 1033])


def save_npz(path, arrs):
    """np.savez_compressed with a fixed member timestamp (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def csr_from_rows(n, rows):
    """Canonical CSR from {row: (sorted column ids, values)}."""
    ptr = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for i in range(n):
        c, v = rows.get(i, ((), ()))
        ptr[i + 1] = ptr[i] + len(c)
        cols.extend(c)
        vals.extend(v)
    return sp.csr_matrix((np.array(vals, dtype=np.float64), np.array(cols, dtype=np.int32), ptr.astype(np.int32)),
                         shape=(n, n))


def ladder_adj(seed=700, n=1300):
    rng = np.random.default_rng(seed)
    where = rng.permutation(n)[:len(LADDER_LENGTHS)]
    rows = {}
    want = dict(zip(where.tolist(), LADDER_LENGTHS))
    for i in range(n):
        k = want[i] - 1 if i in want else int(rng.integers(0, 2))      # entries beside the diagonal
        others = np.delete(np.arange(n), i)
        c = np.sort(rng.choice(others, size=k, replace=False))
        v = (rng.random(k) + 0.5) * np.where(rng.random(k) < 0.25, -1.0, 1.0)
        rows[i] = (c.tolist(), v.tolist())
    a = csr_from_rows(n, rows)
    lens = np.diff((a + sp.identity(n, format="csr")).tocsr().indptr)
    assert all(lens[i] == L for i, L in want.items())
    # a negative degree turns its row and column of Â into NaN: one sign in four is negative, so
    # the ladder rows keep positive degrees and their sums stay visible in Â's bits
    deg = np.asarray((a + sp.identity(n, format="csr")).sum(1)).ravel()
    assert all(deg[i] > 0 for i in want) and (deg < 0).any()
    return a


def sym_adj(seed=701, n=300):
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((n, n)) < 19.0 / n, 1)
    mask = mask | mask.T
    isolated = [7, n // 2, n - 1]
    mask[isolated, :] = False
    mask[:, isolated] = False
    diag = rng.random(n) < 0.25
    diag[isolated] = False
    np.fill_diagonal(mask, diag)
    w = rng.random((n, n)) * 0.9 + 0.1                    # independent in the two directions
    a = sp.csr_matrix(np.where(mask, w, 0.0))
    a.sort_indices()
    assert (a != a.T).nnz > 0 and ((a != 0) != (a.T != 0)).nnz == 0
    return a


def degenerate_adj(seed=702, n=76):
    rng = np.random.default_rng(seed)
    M = np.where(rng.random((n, n)) < 0.12, rng.integers(-3, 4, size=(n, n)), 0).astype(np.float64)
    stored = M != 0
    zeros = rng.random((n, n)) < 0.02                     # explicit zeros (stored, value 0)
    stored |= zeros & (M == 0)
    np.fill_diagonal(M, np.where(rng.random(n) < 0.15, -1.0, np.diag(M)))
    M[5, :] = 0.0
    M[5, 5] = -1.0                                        # A + I loses row 5 altogether
    stored[5, :] = False
    stored |= M != 0
    deg = (M + np.eye(n)).sum(1)
    neg = np.flatnonzero(deg < 0)
    assert neg.size >= 6
    # rows whose degree is brought to zero by an entry in the column of a negative-degree node
    for z, c in zip([i for i in range(10, n, 9) if deg[i] >= 0][:7], neg.tolist()):
        M[z, c] -= deg[z]
        assert M[z, c] != 0 or deg[z] == 0
        stored[z, c] = True
    r, c = np.nonzero(stored)
    ptr = np.r_[0, np.cumsum(np.bincount(r, minlength=n))]
    return sp.csr_matrix((M[r, c], c.astype(np.int32), ptr.astype(np.int32)), shape=(n, n))


def csr_arrays(prefix, m):
    m = sp.csr_matrix(m)
    s = m.copy()
    s.has_sorted_indices = False
    s.sort_indices()
    assert (s.indices == m.indices).all(), "the reference's Â is not in column order"
    return {f"{prefix}_indptr": m.indptr.astype(np.int64), f"{prefix}_indices": m.indices.astype(np.int32),
            f"{prefix}_data": m.data.astype(np.float64)}


def rtag(r):
    return "r" + str(r).replace(".", "")


def main():
    SymLap, Ppr, _, _ = MG.import_reference()
    from operators.utils import adj_to_symmetric_norm
    synth = MG._load_synth()
    manifest = {}
    versions = {"scipy": scipy.__version__, "numpy": np.__version__}
    for name, adj, rs in (("cw_ladder", ladder_adj(), (0.3, 0.5)), ("cw_sym", sym_adj(), (0.3, 0.5)),
                          ("cw_degenerate", degenerate_adj(), (0.5, 0.3))):
        n = adj.shape[0]
        assert n <= 1300 and adj.nnz <= 12000, (name, n, adj.nnz)
        arrs = {"adj_indptr": adj.indptr.astype(np.int64), "adj_indices": adj.indices.astype(np.int32),
                "adj_data": adj.data.astype(np.float64),
                "scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
        variants = []
        with np.errstate(all="ignore"):
            for r in rs:
                ahat = SymLap(3, r=r).construct_adj(adj.copy())
                direct = adj_to_symmetric_norm(adj.tocoo(), r).tocsr()
                assert (ahat.indptr == direct.indptr).all() and (ahat.indices == direct.indices).all()
                assert ahat.data.tobytes() == direct.data.tobytes() or np.isnan(ahat.data).any()
                arrs.update(csr_arrays(f"sym_{rtag(r)}", ahat))
                arrs.update(csr_arrays(f"ppr_{rtag(r)}", Ppr(3, r=r, alpha=ALPHA).construct_adj(adj.copy())))
                variants += [f"sym_{rtag(r)}", f"ppr_{rtag(r)}"]
                if name == "cw_degenerate":
                    # entries (j, i) of A + I whose factors left[i], right[j] are (NaN, 0) or (0, NaN)
                    api = sp.csr_matrix(adj + sp.eye(n))
                    deg = np.array(api.sum(1)).flatten()
                    assert (np.diff(api.indptr) == 0).any() and (deg == 0).any() and (deg < 0).any()
                    left, right = np.power(deg, r - 1), np.power(deg, -r)
                    left[np.isinf(left)] = 0.0
                    right[np.isinf(right)] = 0.0
                    j, i = api.nonzero()
                    hit = (np.isnan(left[i]) & (right[j] == 0)) | ((left[i] == 0) & np.isnan(right[j]))
                    assert hit.sum() >= 5, hit.sum()
                    stored = np.zeros((n, n), dtype=bool)
                    stored[np.repeat(np.arange(n), np.diff(ahat.indptr)), ahat.indices] = True
                    assert not stored[i[hit], j[hit]].any(), "the reference stores a zero-factor entry"
                    assert np.isnan(ahat.data).any()
                    print(name, r, "zero-factor entries absent from the reference's Â:", int(hit.sum()), flush=True)
        meta = {"n": n, "op": "construct_weighted", "nnz": int(adj.nnz), "rs": list(rs), "alpha": ALPHA,
                "variants": variants, **versions}
        if name == "cw_sym":
            X = synth.uniform_features_np(n, 16, seed=90)
            op = SymLap(3, r=0.5)
            hops = op.propagate(adj.copy(), X)
            assert op.adj.data.tobytes() == arrs["sym_r05_data"].tobytes()
            arrs["x"] = X
            for k in (1, 2, 3):
                arrs[f"hop{k}"] = np.ascontiguousarray(hops[k].numpy(), dtype=np.float32)
            meta.update({"d": 16, "k": 3, "hops_of": "sym_r05", "features": "uniform(seed=90)"})
        save_npz(os.path.join(MG.OUT, f"{name}.npz"), arrs)
        manifest[name] = meta
        print(name, "n", n, "nnz", adj.nnz, variants, os.path.getsize(os.path.join(MG.OUT, f"{name}.npz")), "bytes",
              flush=True)
    path = os.path.join(MG.OUT, "manifest.json")
    with open(path) as f:
        full = json.load(f)
    full = {k: v for k, v in full.items() if not k.startswith("cw_")}
    full.update(manifest)
    with open(path, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
    print("wrote", len(manifest), "weighted construct cases")


if __name__ == "__main__":
    main()
