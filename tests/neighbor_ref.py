"""Neighbour sampling on the host: what srg_csr_sample_f32, srgnn.neighbor.sample_neighbors, sample_block and
NeighborLoader must return, entry for entry (include/srgnn_hip.h and DESIGN.md 5.13 state all of it; nothing
here is read from the library).

    positions(seed, v, m, k)                        the k sampled positions of a row of m > k entries, ascending
    sample(indptr, indices, values, nodes, fanout, seed) -> (ptr, idx, val, eid)
    block(indptr, indices, values, n, nodes, fanout, seed) -> (ptr, cols, val, n_id, eid)
    layer_seed(seed, epoch, batch, layer)           the loader's seed of one layer of one batch
    loader_batch(indptr, indices, values, n, seeds, sizes, seed, epoch, batch) -> (n_id, blocks)

The draw is the keyed bijection of srg_sample_distinct_i64 (tests/edge_augment_ref.py restates that entry) over
m = the row's length, keyed by the node id: plain Python integers masked to 64 bits in draws_int, one loop per
draw; draws_many is the same arithmetic on numpy uint64 arrays, many keys at once, for the uniformity checks.
Both count the applications of the permutation and assert that the walk's bound 4^h is never reached."""
import numpy as np

from edge_augment_ref import _mix

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ROUND = 0xD6E8FEB86659FD93
MAX_FANOUT = 64


def mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(seed, v):
    return mix(((seed & M64) + GOLDEN * ((v + 1) & M64)) & M64)


def half_bits(m):
    h = 1
    while (1 << (2 * h)) < m:
        h += 1
    return h


def draws_int(seed, v, m, k):
    """[walk(t) for t < k] over [0, m): draw order, not sorted."""
    assert 0 <= k <= m
    key, h = key_of(seed, v), half_bits(m)
    mask, bound = (1 << h) - 1, 1 << (2 * h)
    rk = [key ^ ((ROUND * (i + 1)) & M64) for i in range(4)]

    def perm(x):
        L, R = x >> h, x & mask
        for i in range(4):
            L, R = R, L ^ (mix(rk[i] ^ R) & mask)
        return (L << h) | R

    out = []
    for t in range(k):
        x, steps = perm(t), 1
        while x >= m:
            assert steps < bound, "the cycle walk reached its bound"
            x, steps = perm(x), steps + 1
        out.append(x)
    return out


def positions(seed, v, m, k):
    p = sorted(draws_int(seed, v, m, k))
    assert all(a < b for a, b in zip(p, p[1:])), "the draws are distinct"
    return p


def draws_many(seeds, nodes, m, k):
    """draws_int for every (seed, node) pair of two broadcastable integer arrays: uint64 [R, k]."""
    U = np.uint64
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1)
    nodes = np.asarray(nodes, dtype=np.uint64).reshape(-1)
    seeds, nodes = np.broadcast_arrays(seeds, nodes)
    h = half_bits(m)
    hh, mask, bound = U(h), U((1 << h) - 1), 1 << (2 * h)
    with np.errstate(over="ignore"):
        key = _mix(seeds + U(GOLDEN) * (nodes + U(1)))
        rk = [np.repeat((key ^ (U(ROUND) * U(i + 1)))[:, None], k, axis=1).reshape(-1) for i in range(4)]
        x = np.tile(np.arange(k, dtype=np.uint64), seeds.size)
        todo = np.ones(x.size, dtype=bool)
        steps = 0
        while todo.any():
            assert steps < bound, "the cycle walk reached its bound"
            idx = np.nonzero(todo)[0]
            L, R = x[idx] >> hh, x[idx] & mask
            for i in range(4):
                L, R = R, L ^ (_mix(rk[i][idx] ^ R) & mask)
            x[idx] = (L << hh) | R
            todo[idx] = x[idx] >= U(m)
            steps += 1
    return x.reshape(seeds.size, k)


def count_of(length, fanout):
    return length if fanout < 0 or length <= fanout else fanout


def sample(indptr, indices, values, nodes, fanout, seed):
    """srg_csr_sample_f32 over well-formed ptr: one plain loop over rows and entries."""
    assert fanout < 0 or 1 <= fanout <= MAX_FANOUT
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    n_rows = indptr.size - 1
    nodes = np.asarray(nodes, dtype=np.int64)
    ptr = np.zeros(nodes.size + 1, dtype=np.int64)
    eid = []
    for b, v in enumerate(nodes.tolist()):
        if 0 <= v < n_rows:
            beg, m = int(indptr[v]), int(indptr[v + 1] - indptr[v])
            pos = range(m) if count_of(m, fanout) == m else positions(seed, v, m, fanout)
            eid.extend(beg + p for p in pos)
        ptr[b + 1] = len(eid)
    eid = np.asarray(eid, dtype=np.int64)
    val = None if values is None else np.asarray(values)[eid]
    return ptr, indices[eid].astype(np.int32), val, eid


def block(indptr, indices, values, n, nodes, fanout, seed):
    """sample_block: n_id = the targets in the order given, then the sampled columns not among them, ascending;
    a column id becomes its position in n_id."""
    nodes = np.asarray(nodes, dtype=np.int64)
    ptr, idx, val, eid = sample(indptr, indices, values, nodes, fanout, seed)
    assert ((idx >= 0) & (idx < n)).all()
    target = set(nodes.tolist())
    frontier = sorted(set(idx.tolist()) - target)
    n_id = np.concatenate([nodes, np.asarray(frontier, dtype=np.int64)])
    where = {int(v): i for i, v in enumerate(n_id.tolist())}
    cols = np.asarray([where[int(c)] for c in idx.tolist()], dtype=np.int32)
    return ptr, cols, val, n_id, eid


# the loader's seeds: three odd multipliers, so the seeds of one batch's layers differ (an odd multiple of a
# non-zero difference of layers below 2^64 is not 0 mod 2^64), as do those of one epoch's batches
EPOCH_MUL, BATCH_MUL, LAYER_MUL = 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7, 0xDB4F0B9175AE2165


def layer_seed(seed, epoch, batch, layer):
    return ((seed & M64) + EPOCH_MUL * (epoch + 1) + BATCH_MUL * (batch + 1) + LAYER_MUL * (layer + 1)) & M64


def loader_batch(indptr, indices, values, n, seeds, sizes, seed, epoch, batch):
    """One NeighborLoader item: (n_id, blocks) with blocks[0] the outermost; every block is block()'s tuple."""
    n_id = np.asarray(seeds, dtype=np.int64)
    blocks = []
    for layer, size in enumerate(sizes):
        blk = block(indptr, indices, values, n, n_id, size, layer_seed(seed, epoch, batch, layer))
        blocks.append(blk)
        n_id = blk[3]
    return n_id, blocks[::-1]


# ---- the test operator of tests/test_neighbor_gpu.py ------------------------------------------------
N = 400
# the edges of a 16-lane group, of the copy / sample switch at the fanouts 1, 2, 10, 25, 63 and 64, of 4^h
# (4, 16, 64, 256, 1024), and a row whose draws take several walk steps
ROW_LENGTHS = [0, 1, 2, 3, 4, 5, 9, 10, 11, 15, 16, 17, 24, 25, 26, 63, 64, 65, 127, 128, 129, 255, 256, 257,
               1023, 1024, 1025, 5000]
FANOUTS = (1, 2, 10, 25, 63, 64, -1)
SEEDS = (0, 0x1234567, M64)


def graph(seed=9):
    """(indptr, indices, values) of the N x N test operator: row i < len(ROW_LENGTHS) has ROW_LENGTHS[i] entries,
    the rest 0 .. 12 in turn; ids drawn with replacement (duplicates) and left in drawn order (unsorted)."""
    rng = np.random.default_rng(seed)
    lens = np.array([ROW_LENGTHS[i] if i < len(ROW_LENGTHS) else (i * 7) % 13 for i in range(N)], dtype=np.int64)
    lens = lens[rng.permutation(N)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, N, int(indptr[-1])).astype(np.int32)
    values = rng.standard_normal(indices.size).astype(np.float32)
    values[::17] = np.float32(-0.0)
    return indptr, indices, values


SETS = ("empty", "one", "all", "reversed", "shuffled37", "empty_rows", "long_rows")


def node_sets(indptr, seed=10):
    rng = np.random.default_rng(seed)
    lens = np.diff(indptr)
    must = [int(np.flatnonzero(lens == k)[0]) for k in (17, 65, 257, 1025, 5000)]
    rest = [r for r in rng.permutation(N).tolist() if r not in must]
    shuffled = np.asarray(must + rest[:(37 * N) // 100 - len(must)], dtype=np.int64)
    rng.shuffle(shuffled)
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "one": np.flatnonzero(lens == 5000).astype(np.int64),
        "all": np.arange(N, dtype=np.int64),
        "reversed": np.arange(N, dtype=np.int64)[::-1].copy(),
        "shuffled37": shuffled,
        "empty_rows": np.flatnonzero(lens == 0).astype(np.int64),
        "long_rows": rng.permutation(np.flatnonzero(lens > 64)).astype(np.int64),
    }


def check_fixtures(ip, ix, v, sets):
    """The graph and the node sets hold what the tests rely on."""
    lens = np.diff(ip)
    assert set(ROW_LENGTHS) <= set(lens.tolist()) and lens.max() == 5000 and ip.size == N + 1
    assert any((np.diff(ix[ip[r]:ip[r + 1]]) < 0).any() for r in range(N)), "the rows are meant to be unsorted"
    assert any(np.unique(ix[ip[r]:ip[r + 1]]).size < lens[r] for r in range(N)), "and to hold duplicates"
    assert sorted(sets) == sorted(SETS)
    assert sets["empty"].size == 0 and sets["one"].size == 1 and sets["shuffled37"].size == 148
    assert np.unique(sets["shuffled37"]).size == 148 and not np.array_equal(sets["shuffled37"], np.sort(sets["shuffled37"]))
    assert sets["empty_rows"].size >= 2 and (lens[sets["empty_rows"]] == 0).all()
    assert sets["long_rows"].size == 11 and (lens[sets["long_rows"]] > 64).all()
