// srg_csr.hip -- CSR utilities on the device: construct_adj's segment sums (storage order and numpy's
// pairwise order), structure validation, the column splits, span copy and mirror positions behind the
// planner and construct_adj, the fp64 product, and the induced sub-graph of a node set (srgnn.cluster).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// construct_adj on the device: sequential fp64 segment sums (duplicate merging in storage order,
// starting from +0 -- scipy's csr_binop / sum_duplicates accumulation order; the directed families'
// scatter sums and the wavelet row normalisation).  The row degrees are k_segment_sum_numpy's.
// ------------------------------------------------------------------------------------------------
// One wave per 64 consecutive segments.  A segment of at most kSegShort entries is summed by its
// own lane; a longer one (a hub row: 155,868 entries on the products-shaped graph, 30 ms as a
// one-lane loop of dependent loads) by the whole wave: the values are read 64 at a time
// with one coalesced load, the next block prefetched, and the sequential sum runs over them
// through v_readlane -- the same adds in the same order.
constexpr int64_t kSegShort = 64;

template <typename T>
__global__ void __launch_bounds__(256)
k_segment_sum(const int64_t* __restrict__ seg_ptr, const T* __restrict__ vals, int64_t n_seg,
              T* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave_stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w * 64 < n_seg;
         w += wave_stride) {
        const int64_t s = w * 64 + lane;
        const bool valid = s < n_seg;
        const int64_t beg = valid ? seg_ptr[s] : 0;
        const int64_t end = valid ? seg_ptr[s + 1] : 0;
        const bool wide = end - beg > kSegShort;
        if (valid && !wide) {
            T acc = T(0);
            for (int64_t j = beg; j < end; ++j) acc = e_add(acc, vals[j]);
            out[s] = acc;
        }
        unsigned long long todo = __ballot(wide);   // wave-uniform
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t b = bcast_lane(beg, l), e = bcast_lane(end, l);
            T acc = T(0);
            int64_t j0 = b + lane;
            T v_nxt = j0 < e ? vals[j0] : T(0);
            for (int64_t jb = b; jb < e; jb += 64) {
                const T v = v_nxt;
                const int64_t jn = jb + 64 + lane;
                v_nxt = jn < e ? vals[jn] : T(0);
                const int nb = (e - jb) < 64 ? (int)(e - jb) : 64;   // wave-uniform
                for (int q = 0; q < nb; ++q) acc = e_add(acc, bcast_lane(v, q));
            }
            if (lane == 0) out[w * 64 + l] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// construct_adj on the device: row degrees in numpy's order.  scipy's csr.sum(1) is
// np.add.reduceat over the non-empty rows, and per row that is a[0] + pairwise(a[1:]) with numpy's
// pairwise sum: fewer than 8 elements sequentially; up to kNpLeaf in eight strided accumulators
// folded as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus a sequential remainder; anything longer
// split at n/2 rounded down to a multiple of 8, left half first.
// ------------------------------------------------------------------------------------------------
constexpr int64_t kNpLeaf = 128;

__device__ __forceinline__ int64_t np_split(int64_t n) { return (n >> 1) & ~(int64_t)7; }

// 1 <= n <= kNpLeaf (numpy starts from -0.0, and -0.0 + a[0] is a[0])
__device__ __forceinline__ double np_leaf_sum(const double* __restrict__ a, int n)
{
    if (n < 8) {
        double res = a[0];
        for (int i = 1; i < n; ++i) res = e_add(res, a[i]);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i = 8;
    for (; i < n - (n & 7); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = e_add(r[k], a[i + k]);
    }
    double res = e_add(e_add(e_add(r[0], r[1]), e_add(r[2], r[3])), e_add(e_add(r[4], r[5]), e_add(r[6], r[7])));
    for (; i < n; ++i) res = e_add(res, a[i]);
    return res;
}

// One wave per 64 consecutive segments, as k_segment_sum.  A segment whose pairwise part fits one
// leaf is summed by its own lane.  A longer one is taken by the whole wave: every leaf of the
// recursion holds 64..128 elements, so it contains a multiple of 64 and lane l looks up the leaf
// around element 64 * (t0 + l) and, if that is the leaf's first multiple, sums it -- up to 64
// independent leaves at a time.  The wave then walks the leaves left to right (uniform control
// flow) and folds the tree in the recursion's order: a finished left child waits in lane `depth`
// of `pend` until its right sibling is complete.
__global__ void __launch_bounds__(256)
k_segment_sum_numpy(const int64_t* __restrict__ seg_ptr, const double* __restrict__ vals, int64_t n_seg,
                    double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave_stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w * 64 < n_seg;
         w += wave_stride) {
        const int64_t s = w * 64 + lane;
        const bool valid = s < n_seg;
        const int64_t beg = valid ? seg_ptr[s] : 0;
        const int64_t end = valid ? seg_ptr[s + 1] : 0;
        const int64_t len = end - beg;
        const bool wide = len - 1 > kNpLeaf;
        const double head = len > 0 ? vals[beg] : 0.0;
        if (valid && !wide)
            out[s] = len > 1 ? e_add(head, np_leaf_sum(vals + beg + 1, (int)(len - 1))) : head;
        unsigned long long todo = __ballot(wide);   // wave-uniform
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t b = bcast_lane(beg, l) + 1;
            const int64_t m = bcast_lane(end, l) - b;        // the pairwise part a[1:], m > kNpLeaf
            const double* __restrict__ a = vals + b;
            double pend = 0.0, leaf = 0.0, v = 0.0;
            int64_t t0 = -64;                                // first multiple of 64 the lanes hold
            for (int64_t pos = 0; pos < m;) {
                int64_t o = 0, k = m;
                unsigned long long path = 0;                 // bit d: went right at depth d
                int depth = 0;
                while (k > kNpLeaf) {
                    const int64_t n2 = np_split(k);
                    if (pos < o + n2) {
                        k = n2;
                    } else {
                        o += n2;
                        k -= n2;
                        path |= 1ull << depth;
                    }
                    ++depth;
                }
                const int64_t t = (o + 63) >> 6;             // o == pos
                if (t - t0 >= 64) {
                    t0 = t;
                    const int64_t p = (t0 + lane) << 6;
                    leaf = 0.0;
                    if (p < m) {
                        int64_t lo = 0, lk = m;
                        while (lk > kNpLeaf) {
                            const int64_t n2 = np_split(lk);
                            if (p < lo + n2) {
                                lk = n2;
                            } else {
                                lo += n2;
                                lk -= n2;
                            }
                        }
                        if (p - lo < 64) leaf = np_leaf_sum(a + lo, (int)lk);
                    }
                }
                v = bcast_lane(leaf, (int)(t - t0));
                while (depth > 0 && ((path >> (depth - 1)) & 1)) {
                    --depth;
                    v = e_add(bcast_lane(pend, depth), v);
                }
                if (depth > 0 && lane == depth - 1) pend = v;
                pos = o + k;
            }
            const double h = bcast_lane(head, l);
            if (lane == 0) out[w * 64 + l] = e_add(h, v);
        }
    }
}

// fp64 product Y = A * X in scipy's csr_matvec(s) order (sparsetools csr.h): each element starts
// from 0 and adds the separately rounded product of every stored entry, in storage order.  One
// thread per output element (row-major, so neighbouring threads share a row's entries); used by
// the construct_adj power iterations (srgnn/directed.py), not by the hop loop.
__global__ void __launch_bounds__(256)
k_spmm_f64(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
           const double* __restrict__ vals, int64_t n_rows, const double* __restrict__ X, int64_t ldx,
           double* __restrict__ Y, int64_t ldy, int d)
{
    const int64_t total = n_rows * (int64_t)d;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t row = e / d;
        const int c = (int)(e - row * d);
        double acc = 0.0;
        for (int64_t j = indptr[row]; j < indptr[row + 1]; ++j)
            acc = __dadd_rn(acc, __dmul_rn(vals[j], X[(int64_t)indices[j] * ldx + c]));
        Y[row * ldy + c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// validation kernel
// ------------------------------------------------------------------------------------------------
__global__ void k_validate(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                           int64_t n_rows, int64_t nnz, int64_t n_cols, unsigned int* __restrict__ bad)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const int32_t c = indices[i];
        if (c < 0 || (int64_t)c >= n_cols) b |= 1u;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += stride) {
        if (indptr[i + 1] < indptr[i]) b |= 2u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (indptr[0] != 0) b |= 4u;
        if (indptr[n_rows] != nnz) b |= 8u;
    }
    if (b) atomicOr(bad, b);
}

// Column-block split points: splits[(b-1) * n_rows + r] = the first entry of row r whose column id
// is >= ceil(b * n_cols / B) (a lower bound over the row's sorted ids), b = 1 .. B-1.  One thread per
// (row, boundary).  For a row whose ids are not sorted the result is still a position in
// [indptr[r], indptr[r+1]] and the split points of a row never decrease with b, so the spans still
// partition the row in CSR order: the hop stays exact, only the blocks' locality is lost.
__global__ void __launch_bounds__(256)
k_col_splits(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
             int64_t n_cols, int n_blocks, int64_t* __restrict__ splits)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * (n_blocks - 1)) return;
    const int b = (int)(t / n_rows) + 1;
    const int64_t r = t % n_rows;
    const int64_t bound = (b * n_cols + n_blocks - 1) / n_blocks;
    int64_t lo = indptr[r], hi = indptr[r + 1];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)indices[mid] < bound)
            lo = mid + 1;
        else
            hi = mid;
    }
    splits[t] = lo;
}

// Span copy (DeviceCSR compact copies: the entries of a launch laid out in the order it takes its
// rows): row order[i]'s span [beg, end) of (indices, values) goes to [pos[i], pos[i] + len) of the
// output arrays, and out_beg / out_end of that row get the new span.  16 lanes per row, each lane
// copying every 16th entry (coalesced runs of the row); 4 rows per wave, a grid stride over rows.
__global__ void __launch_bounds__(256)
k_copy_spans(const int32_t* __restrict__ order, int64_t n, const int64_t* __restrict__ beg,
             const int64_t* __restrict__ end, const int32_t* __restrict__ ix, const float* __restrict__ v,
             const int64_t* __restrict__ pos, int32_t* __restrict__ oix, float* __restrict__ ov,
             int64_t* __restrict__ obeg, int64_t* __restrict__ oend)
{
    const int l = threadIdx.x & 15;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x / 16);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4); i < n; i += stride) {
        const int r = order[i];
        const int64_t b = beg[r], len = end[r] - b, p = pos[i];
        for (int64_t e = l; e < len; e += 16) {
            oix[p + e] = ix[b + e];
            ov[p + e] = v[b + e];
        }
        if (l == 0) {
            obeg[r] = p;
            oend[r] = p + len;
        }
    }
}

// Mirror positions of a CSR with sorted rows: mirror[e] = the position of entry (c, r) in row c for
// entry e = (r, c), or -1 when row c holds no column r (one binary search per entry).  All entries
// found <=> the structure is symmetric, and then the transpose of the matrix is the same structure
// with values[mirror] -- construct_adj's (A+I)^T without a sort (srgnn/construct.py).
__global__ void __launch_bounds__(256)
k_csr_mirror(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
             const int64_t* __restrict__ rows, int64_t nnz, int64_t* __restrict__ mirror)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t r = rows[e];
        const int32_t c = indices[e];
        int64_t lo = indptr[c], hi = indptr[c + 1];
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if ((int64_t)indices[mid] < r)
                lo = mid + 1;
            else
                hi = mid;
        }
        mirror[e] = (lo < indptr[c + 1] && (int64_t)indices[lo] == r) ? lo : -1;
    }
}

// ------------------------------------------------------------------------------------------------
// the induced sub-graph of a node set: rows nodes[b] of the operator, filtered through pos
// ------------------------------------------------------------------------------------------------
// One wave per kInducedRowsPerWave = 4 consecutive batch rows, 16 lanes each (lane l of group g holds entry
// beg + 16 t + l of row 4 w + g in step t).  A row of at most kInducedShort entries is walked by its group,
// all four steps' ids and table entries in flight at once; a longer one afterwards by the whole wave,
// kInducedWide blocks of 64 ids per trip with the next trip's ids issued behind them.  Either way a kept
// entry's slot in its row is its rank among the kept ones: one ballot per step, the popcount of the lanes
// below (inside the group's 16 bits for a short row) plus the running count of the steps before.  So the
// output is a function of the inputs alone, whichever path a row takes, and nothing is added atomically.
// FILL false: cnt[b] = kept entries of row b.  FILL true: the kept entries go to ptr[b] .. of the outputs.
// POS false: a row slice, every entry is kept and its id copied.  An id outside [0, n_cols) is rejected
// before pos is read; a nodes[b] outside [0, n_rows) is an empty row and never an address.
// Cost of a long row: it is one wave's serial walk, 6 - 8 ns per entry on the products-shaped graph with eight
// and with sixteen blocks per trip alike, and the batch's longest row sets the kernel's time.
constexpr int kInducedRowsPerWave = 4;
constexpr int kInducedSteps = 4;
constexpr int64_t kInducedShort = 16 * kInducedSteps;
constexpr int kInducedWide = 8;

template <bool POS>
__device__ __forceinline__ bool induced_keep(int c, bool in, int64_t n_cols, const int32_t* __restrict__ pos, int& id)
{
    if constexpr (POS) {
        const bool ok = in && c >= 0 && (int64_t)c < n_cols;
        const int p = ok ? pos[c] : -1;
        id = p;
        return p >= 0;
    } else {
        id = c;
        return in;
    }
}

__device__ __forceinline__ void induced_store(int64_t o, int id, int64_t j, const float* __restrict__ values,
                                              int32_t* __restrict__ out_idx, float* __restrict__ out_val,
                                              int64_t* __restrict__ out_eid)
{
    out_idx[o] = id;
    if (out_val) out_val[o] = values[j];
    if (out_eid) out_eid[o] = j;
}

template <bool FILL, bool POS>
__global__ void __launch_bounds__(kBlock)
k_csr_induced(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
              const float* __restrict__ values, int64_t n_rows, int64_t n_cols, const int64_t* __restrict__ nodes,
              int64_t B, const int32_t* __restrict__ pos, int64_t* __restrict__ cnt, const int64_t* __restrict__ ptr,
              int32_t* __restrict__ out_idx, float* __restrict__ out_val, int64_t* __restrict__ out_eid,
              int block_base)
{
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, l = lane & 15;
    const int64_t b = (int64_t)wave_slot(block_base) * kInducedRowsPerWave + g;
    const bool valid = b < B;
    const int64_t r = valid ? nodes[b] : -1;
    const bool has_row = r >= 0 && r < n_rows;
    const int64_t beg = has_row ? indptr[r] : 0;
    const int64_t end = has_row ? indptr[r + 1] : 0;
    int64_t row_out = 0;
    if constexpr (FILL) row_out = valid ? ptr[b] : 0;
    const bool wide = end - beg > kInducedShort;

    // ---- short rows: the four groups side by side ----
    {
        int c[kInducedSteps], id[kInducedSteps];
        bool kept[kInducedSteps];
#pragma unroll
        for (int t = 0; t < kInducedSteps; ++t) {
            const int64_t j = beg + 16 * t + l;
            c[t] = (!wide && j < end) ? indices[j] : -1;
        }
#pragma unroll
        for (int t = 0; t < kInducedSteps; ++t) {
            const int64_t j = beg + 16 * t + l;
            kept[t] = induced_keep<POS>(c[t], !wide && j < end, n_cols, pos, id[t]);
        }
        int base = 0;
#pragma unroll
        for (int t = 0; t < kInducedSteps; ++t) {
            const unsigned gm = (unsigned)(__ballot(kept[t]) >> (16 * g)) & 0xffffu;
            if constexpr (FILL) {
                if (kept[t])
                    induced_store(row_out + base + __builtin_popcount(gm & ((1u << l) - 1u)), id[t], beg + 16 * t + l,
                                  values, out_idx, out_val, out_eid);
            }
            base += __builtin_popcount(gm);
        }
        if constexpr (!FILL) {
            if (valid && !wide && l == 0) cnt[b] = base;
        }
    }

    // ---- long rows: the whole wave, one row after the other ----
    unsigned long long todo = __ballot(wide && l == 0);   // wave-uniform
    while (todo) {
        const int q = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t wb = bcast_lane(beg, q), we = bcast_lane(end, q), wo = bcast_lane(row_out, q);
        const unsigned long long below = (1ull << lane) - 1ull;
        int64_t base = 0;
        int c_nxt[kInducedWide];
#pragma unroll
        for (int u = 0; u < kInducedWide; ++u) {
            const int64_t j = wb + 64 * u + lane;
            c_nxt[u] = j < we ? indices[j] : -1;
        }
        for (int64_t jb = wb; jb < we; jb += 64 * kInducedWide) {
            int id[kInducedWide];
            bool kept[kInducedWide];
#pragma unroll
            for (int u = 0; u < kInducedWide; ++u) {
                const int c = c_nxt[u];
                const int64_t jn = jb + 64 * (kInducedWide + u) + lane;
                c_nxt[u] = jn < we ? indices[jn] : -1;
                kept[u] = induced_keep<POS>(c, jb + 64 * u + lane < we, n_cols, pos, id[u]);
            }
#pragma unroll
            for (int u = 0; u < kInducedWide; ++u) {
                const unsigned long long m = __ballot(kept[u]);
                if constexpr (FILL) {
                    if (kept[u])
                        induced_store(wo + base + __builtin_popcountll(m & below), id[u], jb + 64 * u + lane, values,
                                      out_idx, out_val, out_eid);
                }
                base += __builtin_popcountll(m);
            }
        }
        if constexpr (!FILL) {
            if (lane == q) cnt[b] = base;   // lane q is lane 0 of the row's group: its b is the row's
        }
    }
}

template <typename T>
int launch_segment_sum(const int64_t* seg_ptr, const T* vals, int64_t n_seg, T* out, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_seg < 0) return srg_fail(SRG_ERR_INVALID, "n_seg=%lld < 0", (long long)n_seg);
    if (n_seg == 0) return srg_ok();
    if (!seg_ptr || !out) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_seg + 255) / 256, launch_cap(1 << 16));   // 64 segments per wave
    hipLaunchKernelGGL(k_segment_sum<T>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seg_ptr, vals, n_seg, out);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

}  // namespace

extern "C" {

int srg_segment_sum_f64(const int64_t* seg_ptr, const double* vals, int64_t n_seg, double* out, void* stream)
{
    return launch_segment_sum<double>(seg_ptr, vals, n_seg, out, stream);
}

int srg_segment_sum_f32(const int64_t* seg_ptr, const float* vals, int64_t n_seg, float* out, void* stream)
{
    return launch_segment_sum<float>(seg_ptr, vals, n_seg, out, stream);
}

int srg_segment_sum_numpy_f64(const int64_t* seg_ptr, const double* vals, int64_t n_seg, double* out, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_seg < 0) return srg_fail(SRG_ERR_INVALID, "n_seg=%lld < 0", (long long)n_seg);
    if (n_seg == 0) return srg_ok();
    if (!seg_ptr || !out) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_seg + 255) / 256, launch_cap(1 << 16));   // 64 segments per wave
    hipLaunchKernelGGL(k_segment_sum_numpy, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seg_ptr, vals, n_seg, out);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_spmm_csr_f64(const int64_t* indptr, const int32_t* indices, const double* values, int64_t n_rows,
                     const double* X, int64_t ldx, double* Y, int64_t ldy, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_spmm_args(indptr, indices, values, n_rows, X, ldx, Y, ldy, d);
    if (rc) return rc;
    if (n_rows == 0 || d == 0) return srg_ok();
    const int64_t total = n_rows * (int64_t)d;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, launch_cap(1 << 20));
    hipLaunchKernelGGL(k_spmm_f64, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       indptr, indices, values, n_rows, X, ldx, Y, ldy, d);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_csr_validate(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                     int64_t n_cols, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0 || nnz < 0 || n_cols < 0) return srg_fail(SRG_ERR_INVALID, "negative size");
    if (!indptr) return srg_fail(SRG_ERR_INVALID, "null indptr");
    if (nnz > 0 && !indices) return srg_fail(SRG_ERR_INVALID, "null indices");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned int* d_bad = nullptr;
    SRG_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&d_bad), sizeof(unsigned int), s));
    SRG_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(unsigned int), s));
    const int64_t work = std::max(nnz, n_rows);
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((work + 255) / 256, 1), launch_cap(8192));
    hipLaunchKernelGGL(k_validate, dim3(blocks), dim3(256), 0, s, indptr, indices, n_rows, nnz, n_cols, d_bad);
    SRG_HIP_CHECK(hipGetLastError());
    unsigned int bad = 0;
    SRG_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    SRG_HIP_CHECK(hipFreeAsync(d_bad, s));
    SRG_HIP_CHECK(hipStreamSynchronize(s));
    if (bad & 1u) return srg_fail(SRG_ERR_INVALID, "column id outside [0, %lld)", (long long)n_cols);
    if (bad & 2u) return srg_fail(SRG_ERR_INVALID, "indptr decreases");
    if (bad & 4u) return srg_fail(SRG_ERR_INVALID, "indptr[0] != 0");
    if (bad & 8u) return srg_fail(SRG_ERR_INVALID, "indptr[n_rows] != nnz=%lld", (long long)nnz);
    return srg_ok();
}

int srg_csr_col_splits(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                       int32_t n_blocks, int64_t* splits, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0 || n_cols < 0) return srg_fail(SRG_ERR_INVALID, "negative size");
    if (n_blocks < 2 || n_blocks > 64) return srg_fail(SRG_ERR_INVALID, "n_blocks=%d not in [2, 64]", n_blocks);
    const int64_t work = n_rows * (n_blocks - 1);
    if (work == 0) return srg_ok();
    if (!indptr || !splits) return srg_fail(SRG_ERR_INVALID, "null indptr or splits");
    if ((work + 255) / 256 > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "grid too large");
    hipLaunchKernelGGL(k_col_splits, dim3((unsigned)((work + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), indptr, indices, n_rows, n_cols, (int)n_blocks, splits);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_csr_copy_spans(const int32_t* order, int64_t n_order, const int64_t* beg, const int64_t* end,
                       const int32_t* indices, const float* values, const int64_t* pos, int32_t* out_indices,
                       float* out_values, int64_t* out_beg, int64_t* out_end, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_order < 0) return srg_fail(SRG_ERR_INVALID, "n_order=%lld < 0", (long long)n_order);
    if (n_order == 0) return srg_ok();
    if (!order || !beg || !end || !pos || !out_beg || !out_end)
        return srg_fail(SRG_ERR_INVALID, "null order / span / position array");
    const int64_t rows_per_block = 256 / 16;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_order + rows_per_block - 1) / rows_per_block, launch_cap(1 << 20));
    hipLaunchKernelGGL(k_copy_spans, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), order, n_order,
                       beg, end, indices, values, pos, out_indices, out_values, out_beg, out_end);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_csr_mirror(const int64_t* indptr, const int32_t* indices, const int64_t* rows, int64_t n_rows,
                   int64_t nnz, int64_t* mirror, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0 || nnz < 0) return srg_fail(SRG_ERR_INVALID, "negative size");
    if (nnz == 0) return srg_ok();
    if (!indptr || !indices || !rows || !mirror) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((nnz + 255) / 256, launch_cap(1 << 20));
    hipLaunchKernelGGL(k_csr_mirror, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), indptr, indices,
                       rows, nnz, mirror);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_csr_induced_f32(int phase, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                        int64_t n_cols, const int64_t* nodes, int64_t B, const int32_t* pos, int64_t* cnt,
                        const int64_t* ptr, int32_t* out_idx, float* out_val, int64_t* out_eid, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (phase != 0 && phase != 1) return srg_fail(SRG_ERR_INVALID, "phase %d is neither 0 (count) nor 1 (fill)", phase);
    if (n_rows < 0 || n_cols < 0 || B < 0)
        return srg_fail(SRG_ERR_INVALID, "negative size (n_rows=%lld, n_cols=%lld, B=%lld)", (long long)n_rows,
                        (long long)n_cols, (long long)B);
    if (n_cols > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "n_cols=%lld >= 2^31", (long long)n_cols);
    if (B > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "B=%lld >= 2^31", (long long)B);
    if (B == 0) return srg_ok();
    if (!nodes) return srg_fail(SRG_ERR_INVALID, "null nodes");
    if (n_rows > 0 && !indptr) return srg_fail(SRG_ERR_INVALID, "null indptr");
    if (phase == 0 && !cnt) return srg_fail(SRG_ERR_INVALID, "null cnt in phase 0");
    if (phase == 1 && (!ptr || !out_idx)) return srg_fail(SRG_ERR_INVALID, "null ptr or out_idx in phase 1");
    if (phase == 1 && out_val && !values) return srg_fail(SRG_ERR_INVALID, "out_val without values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows_per_block = (int64_t)kWavesPerBlock * kInducedRowsPerWave;
    const int rc = launch_chunks_capped((B + rows_per_block - 1) / rows_per_block, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nb), dim3(kBlock), 0, s, indptr, indices, values, n_rows, n_cols, nodes, B,
                               pos, cnt, ptr, out_idx, out_val, out_eid, (int)b0);
        };
        if (phase == 0)
            pos ? go(k_csr_induced<false, true>) : go(k_csr_induced<false, false>);
        else
            pos ? go(k_csr_induced<true, true>) : go(k_csr_induced<true, false>);
        return launch_status();
    });
    if (rc) return rc;
    return srg_ok();
}

}  // extern "C"
