"""The induced sub-graph of a node set in numpy: what srg_csr_induced_f32 and srgnn.cluster.induced_subgraph
must return, entry for entry.  Both modes, forged column ids included, and the entry ids.

    induced(indptr, indices, values, n_cols, nodes, relabel) -> (ptr, idx, val, eid)

Row b of the result is row nodes[b]; with relabel an entry with column id c is kept iff 0 <= c < n_cols and c is
in `nodes`, and stored as c's position in `nodes`; without, every entry is kept and its id copied.  Kept entries
keep the stored order, duplicates stay, val is values[eid].  A nodes[b] outside [0, n_rows) is an empty row.
One plain loop over rows and entries: no vectorised trick shared with the code under test.  For valid input it
equals scipy's A[S][:, S] and A[S] (tests/test_cluster_cpu.py)."""
import numpy as np


def pos_of(nodes, n_cols):
    """pos[nodes[b]] = b, -1 elsewhere (graph_conv.batch_rows' table)."""
    pos = np.full(n_cols, -1, dtype=np.int32)
    for b, r in enumerate(np.asarray(nodes).tolist()):
        if 0 <= r < n_cols:
            pos[r] = b
    return pos


def induced(indptr, indices, values, n_cols, nodes, relabel=True):
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    n_rows = indptr.size - 1
    nodes = np.asarray(nodes, dtype=np.int64)
    pos = pos_of(nodes, n_cols) if relabel else None
    ptr = np.zeros(nodes.size + 1, dtype=np.int64)
    idx, eid = [], []
    for b, r in enumerate(nodes.tolist()):
        if 0 <= r < n_rows:
            for j in range(int(indptr[r]), int(indptr[r + 1])):
                c = int(indices[j])
                if not relabel:
                    idx.append(c)
                    eid.append(j)
                elif 0 <= c < n_cols and pos[c] >= 0:
                    idx.append(int(pos[c]))
                    eid.append(j)
        ptr[b + 1] = len(idx)
    eid = np.asarray(eid, dtype=np.int64)
    val = None if values is None else np.asarray(values)[eid]
    return ptr, np.asarray(idx, dtype=np.int32), val, eid


def scipy_slice(A, nodes, relabel=True):
    """(indptr, indices, data) of scipy's A[S][:, S] (relabel) or A[S], as scipy stores them."""
    S = np.asarray(nodes, dtype=np.int64)
    M = A[S]
    if relabel:
        M = M[:, S]
    return np.asarray(M.indptr, dtype=np.int64), np.asarray(M.indices, dtype=np.int32), np.asarray(M.data)


# ---- the test graph of tests/test_cluster_gpu.py ----------------------------------------------------
N = 300
# the edges of a 16-lane group (one to four steps of it), a 64-entry id block, two blocks, a row of every column,
# and (rows may repeat a column) the edges of the long rows' trip of eight blocks and a row of three trips
TRIP = 512
ROW_LENGTHS = list(range(0, 18)) + [31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200, 300,
                                    TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 52]


def graph(seed=5):
    """(indptr, indices, values) of the N x N test operator: row i < len(ROW_LENGTHS) has ROW_LENGTHS[i] entries,
    the rest 0 .. 12 in turn; ids drawn with replacement (duplicates) and left in drawn order (unsorted)."""
    rng = np.random.default_rng(seed)
    lens = np.array([ROW_LENGTHS[i] if i < len(ROW_LENGTHS) else (i * 7) % 13 for i in range(N)], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, N, int(indptr[-1])).astype(np.int32)
    values = rng.standard_normal(indices.size).astype(np.float32)
    values[::17] = np.float32(-0.0)
    return indptr, indices, values


def node_sets(indptr, indices, seed=6):
    """The named node sets.  `dropped`: rows whose every entry points outside the set."""
    rng = np.random.default_rng(seed)
    lens = np.diff(indptr)
    empty_rows = np.flatnonzero(lens == 0)
    # a set no entry of which survives: greedily, nodes none of whose entries hit the set or themselves
    chosen, member = [], np.zeros(N, bool)
    for r in rng.permutation(N).tolist():
        cols = indices[indptr[r]:indptr[r + 1]]
        if lens[r] == 0 or lens[r] > 12 or member[cols].any() or (cols == r).any():
            continue
        if any((indices[indptr[q]:indptr[q + 1]] == r).any() for q in chosen):
            continue
        chosen.append(r)
        member[r] = True
    # 37 % of the nodes in drawn order, the rows past a step, a block and a trip among them
    must = [ROW_LENGTHS.index(k) for k in (17, 65, 129, TRIP + 1, 2 * TRIP + 52)]
    rest = [r for r in rng.permutation(N).tolist() if r not in must]
    shuffled = np.asarray(must + rest[:(37 * N) // 100 - len(must)], dtype=np.int64)
    rng.shuffle(shuffled)
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "one": np.array([ROW_LENGTHS.index(300)], dtype=np.int64),
        "all": np.arange(N, dtype=np.int64),
        "reversed": np.arange(N, dtype=np.int64)[::-1].copy(),
        "shuffled37": shuffled,
        "empty_rows": empty_rows.astype(np.int64),
        "dropped": np.asarray(chosen, dtype=np.int64),
    }


SETS = ("empty", "one", "all", "reversed", "shuffled37", "empty_rows", "dropped")


def check_fixtures(ip, ix, v, sets):
    """The graph and the node sets hold what the tests rely on: no test passes on trivial batches."""
    lens = np.diff(ip)
    assert N == 300 and set(ROW_LENGTHS) <= set(lens.tolist()) and lens.max() > 2 * TRIP
    assert {0, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 300} <= set(lens.tolist())
    assert sorted(sets) == sorted(SETS)
    assert sets["empty"].size == 0 and sets["one"].size == 1 and sets["shuffled37"].size == 111
    assert np.array_equal(sets["all"], np.arange(N)) and np.array_equal(sets["reversed"], np.arange(N)[::-1])
    assert sets["empty_rows"].size >= 2 and (lens[sets["empty_rows"]] == 0).all()
    ptr = induced(ip, ix, v, N, sets["dropped"])[0]
    assert sets["dropped"].size >= 3 and lens[sets["dropped"]].sum() > 0 and ptr[-1] == 0     # no entry survives
    # the identity batch returns the operator itself
    ptr, idx, val, eid = induced(ip, ix, v, N, sets["all"])
    assert np.array_equal(ptr, ip) and np.array_equal(idx, ix) and np.array_equal(eid, np.arange(ix.size))
    # the shuffled batch: entries kept on both sides of a 64-entry block edge of one row (of a 16-lane step and of
    # a long row's trip as well), a row fully kept, one fully dropped, one partly kept
    S = sets["shuffled37"]
    assert np.unique(S).size == S.size and not np.array_equal(S, np.sort(S))
    ptr, idx, val, eid = induced(ip, ix, v, N, S)
    kept = np.diff(ptr)
    off = eid - np.repeat(ip[S], kept)                          # a kept entry's offset in its row
    row = np.repeat(np.arange(S.size), kept)
    for edge in (16, 64, TRIP, 2 * TRIP):
        assert any((off[row == b] < edge).any() and (off[row == b] >= edge).any() for b in range(S.size)), \
            f"no row keeps entries on both sides of offset {edge}"
    full = lens[S]
    assert ((kept == full) & (full > 0)).any() and ((kept == 0) & (full > 0)).any() and ((kept > 0) & (kept < full)).any()
