"""The device-built wavelet basis restated in numpy (the yardstick of tests/test_wavelet_sparsify_*.py):
the threshold mask of SpectralModel.calculate_wavelet (SSRG/models/base_scalable/base_model.py:251-254:
sub[sub < tol] = 0; csr_matrix(sub.astype(float32))), the block order of sp.hstack(blocks).tocsr() and
sklearn's _inplace_csr_row_normalize_l1 (a sequential fp64 sum of |x|, an fp64 divide rounded to fp32).
tests/test_wavelet_sparsify_cpu.py pins it to the reference's own lines and to the golden wav_* bases."""
import numpy as np

# the values the kernels' edge cases turn on: NaN (kept by a negated <), +-Inf (follow the comparison), -0
# (dropped), 1e-50 (rounds to fp32 zero: dropped), 1e-40 (rounds to an fp32 subnormal: kept)
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 1e-50, 1e-40)
TOLERANCES = (1e-4, 0.0, -1.0, float("nan"), float("inf"))


def survivors(R, tol):
    """(mask, fp32 values) of a dense fp64 block: !(R < tol) && (float)R != 0."""
    R = np.asarray(R, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        f = R.astype(np.float32)
        mask = ~(R < tol) & (f != 0)
    return mask, f


def sparsify_block(R, tol, col0):
    """(cnt int64 [n], ptr int64 [n + 1], idx int32, val fp32) of the block that holds columns col0 ..:
    survivors row by row, columns ascending."""
    mask, f = survivors(R, tol)
    cnt = mask.sum(axis=1).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    cols = np.nonzero(mask)[1]                     # row-major: columns ascend inside a row
    return cnt, ptr, (cols + col0).astype(np.int32), f[mask]


def hstack_blocks(blocks, n):
    """(indptr, indices, data) of the block-local CSRs (ptr, idx, val) appended row by row in block order."""
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(p)) for p, _, _ in blocks] + [np.zeros(0, np.int64)])
    order = np.argsort(rows, kind="stable")        # by row; block order, then storage order, inside a row
    idx = np.concatenate([i for _, i, _ in blocks] + [np.zeros(0, np.int32)])[order]
    val = np.concatenate([v for _, _, v in blocks] + [np.zeros(0, np.float32)])[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows.astype(np.int64), minlength=n))]).astype(np.int64)
    return indptr, idx.astype(np.int32), val.astype(np.float32)


def l1_normalize(indptr, data):
    """Per row: acc = |x0| + |x1| + ... in fp64, left to right from +0; acc != 0 (NaN included):
    x -> (float)((double)x / acc); acc == 0: the row as it is."""
    out = np.array(data, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for i in range(len(indptr) - 1):
            lo, hi = int(indptr[i]), int(indptr[i + 1])
            acc = 0.0
            for a in np.abs(out[lo:hi].astype(np.float64)).tolist():
                acc += a
            if acc != 0.0:
                out[lo:hi] = (out[lo:hi].astype(np.float64) / acc).astype(np.float32)
    return out


def basis(dense_blocks, tol, n):
    """(indptr, indices, data) of the normalised basis from (col0, R) dense blocks in block order."""
    blocks = [sparsify_block(R, tol, c0)[1:] for c0, R in dense_blocks]
    indptr, idx, val = hstack_blocks(blocks, n)
    return indptr, idx, l1_normalize(indptr, val)


def planted_block(n_rows, w, seed, specials=SPECIALS):
    """A [n_rows, w] fp64 block of values around the tolerances with the special values planted, one row
    of zeros (no survivor), one row far above every finite tolerance (every column survives) and one
    whose only survivor at the finite tolerances is its last column."""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((n_rows, w)) * 10.0 ** rng.integers(-6, 1, size=(n_rows, w))
    first = 3 if n_rows > 3 else 0                 # the special values go below the structured rows
    flat = R[first:].reshape(-1)                   # a view: R is contiguous
    where = rng.choice(flat.size, size=min(flat.size, 3 * len(specials)), replace=False)
    for k, p in enumerate(where):
        flat[p] = specials[k % len(specials)]
    if n_rows > 3:
        R[0, :] = 0.0
        R[1, :] = 1.0 + rng.random(w)
        R[2, :] = -2.0
        R[2, w - 1] = 3.0
    return R
