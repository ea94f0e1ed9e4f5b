// srg_gconv.hip -- the last layer of a GCN restricted to a batch of rows (srgnn.graph_conv;
// Layer2GraphConvolution, SSRG/models/simple_models.py): the row-restricted product Y = A[rows, :] X
// (srg_gconv_rows_f32) and its adjoint dX = A[rows, :]^T G (srg_gconv_rows_adjoint_f32), the latter over
// the rows of the transposed operator with the batch as a position table.
//
// Both keep the hop's arithmetic: one output element is one chain acc = fmaf(v_e, x_e, acc) from +0.0f
// over the entries of its row in stored order.  The adjoint runs that chain over the member entries only
// (pos[indices_t[e]] in [0, B)); every other entry is skipped, never folded in as v * 0.  A wave owns one
// row and a tile of 64 * VEC columns, so the bits depend on neither the tile, the load path (VEC 4: 16-byte
// loads, VEC 1: 4-byte loads) nor the launch.  No atomics, no scratch; every store is a plain vector store.
//
// Cost of a long row: a row is one wave's serial chain.  Forward, a batch row of L entries costs L / 8
// rounds of 8 gathers in flight (row_gather); the adjoint's cost is the filtered row walk's (row_walk_kept).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// Y[b, col ..] = A[rows[b], :] X[:, col ..]: the row-wave gather of the hop (srg_device.h) on row rows[b].
// A row id outside [0, n_rows) stores +0 and is never used as an address.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_gconv_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
             const float* __restrict__ values, int64_t n_rows, const int64_t* __restrict__ rows, int64_t B,
             const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int d, int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int b = wave_slot(block_base);
    if (b >= B) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int col = ((int)blockIdx.y * 64 + lane) * VEC;
    const bool act = col < d;
    const int64_t r = rows[b];
    V acc = vzero<float, VEC>();
    if (r >= 0 && r < n_rows) {
        const int row = __builtin_amdgcn_readfirstlane((int)r);
        row_gather<float, VEC, kUnroll, false, int64_t>(acc, indptr, indices, values, row, X, ldx, col, act);
    }
    if (act) vstore<float, VEC>(Y + (int64_t)b * ldy + col, acc, false);
}

// dX[c, col ..] = the chain over row c of the transposed operator, member entries only: the filtered row
// walk (srg_device.h).  keep: the entry's position pos[id] and value, kept when the position is a member's;
// fetch: that member's row of G; fold: the chain link.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_gconv_rows_adjoint(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                     const float* __restrict__ values, int64_t n, const int32_t* __restrict__ pos, int64_t B,
                     const float* __restrict__ G, int64_t ldg, float* __restrict__ dX, int64_t ldx, int d,
                     int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int c = wave_slot(block_base);
    if (c >= n) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int col = ((int)blockIdx.y * 64 + lane) * VEC;
    const bool act = col < d;
    V acc = vzero<float, VEC>();
    struct Entry { bool kept; int p; float a; };
    struct Slot { V x; float a; };
    row_walk_kept<Slot, kUnroll>(
        indices, indptr[c], indptr[c + 1],
        [&](int id, int64_t j) {
            // an id outside [0, n) is never an address; a position outside [0, B) is no member
            int p = -1;
            if (id >= 0 && id < n) p = pos[id];
            const bool member = p >= 0 && p < B;
            return Entry{member, p, member ? values[j] : 0.0f};
        },
        [&](const Entry& mine, int q) {
            // (the value first: its readlane waits for the lane's load of values[j], which must not come to
            // stand behind a gather that is already in flight)
            const int pq = __builtin_amdgcn_readlane(mine.p, q);
            const float a = bcast_lane(mine.a, q);
            return Slot{act ? gload<float, VEC>(G + (int64_t)pq * ldg + col) : vzero<float, VEC>(), a};
        },
        [&](const Slot& s) { chain<float, VEC>(acc, s.a, s.x); });
    if (act) vstore<float, VEC>(dX + (int64_t)c * ldx + col, acc, false);
}

int check_sizes(int64_t n, int64_t B, int d, int64_t lda, int64_t ldb, const char* na, const char* nb)
{
    if (n < 0 || n > INT32_MAX - 64 || B < 0 || B > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "n=%lld, B=%lld out of range [0, 2^31-64)", (long long)n, (long long)B);
    if (d < 0) return srg_fail(SRG_ERR_INVALID, "d=%d < 0", d);
    if (lda < d || ldb < d)
        return srg_fail(SRG_ERR_INVALID, "leading dimensions (%s=%lld, %s=%lld) < d=%d", na, (long long)lda, nb,
                        (long long)ldb, d);
    return SRG_OK;
}

}  // namespace

extern "C" {

int srg_gconv_rows_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                       const int64_t* rows, int64_t B, const float* X, int64_t ldx, float* Y, int64_t ldy,
                       int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_sizes(n_rows, B, d, ldx, ldy, "ldx", "ldy");
    if (rc) return rc;
    if (B == 0 || d == 0) return srg_ok();
    if (!rows || !Y) return srg_fail(SRG_ERR_INVALID, "null rows or Y");
    if (n_rows > 0 && !indptr) return srg_fail(SRG_ERR_INVALID, "null indptr");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool v4 = rows_aligned(4, sizeof(float), d, {{X, ldx}, {Y, ldy}});
    const int tile = v4 ? 256 : 64;
    const unsigned tiles = (unsigned)((d + tile - 1) / tile);
    rc = launch_chunks_capped((B + kWavesPerBlock - 1) / kWavesPerBlock, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (v4)
            hipLaunchKernelGGL(k_gconv_rows<4>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr, indices, values, n_rows,
                               rows, B, X, ldx, Y, ldy, d, (int)b0);
        else
            hipLaunchKernelGGL(k_gconv_rows<1>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr, indices, values, n_rows,
                               rows, B, X, ldx, Y, ldy, d, (int)b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_gconv_rows_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const float* values_t, int64_t n,
                               const int32_t* pos, int64_t B, const float* G, int64_t ldg, float* dX, int64_t ldx,
                               int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_sizes(n, B, d, ldg, ldx, "ldg", "ldx");
    if (rc) return rc;
    if (n == 0 || d == 0) return srg_ok();
    if (!indptr_t || !pos || !dX) return srg_fail(SRG_ERR_INVALID, "null indptr_t, pos or dX");
    if (B > 0 && !G) return srg_fail(SRG_ERR_INVALID, "null G with B=%lld", (long long)B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool v4 = rows_aligned(4, sizeof(float), d, {{G, ldg}, {dX, ldx}});
    const int tile = v4 ? 256 : 64;
    const unsigned tiles = (unsigned)((d + tile - 1) / tile);
    rc = launch_chunks_capped((n + kWavesPerBlock - 1) / kWavesPerBlock, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (v4)
            hipLaunchKernelGGL(k_gconv_rows_adjoint<4>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t,
                               values_t, n, pos, B, G, ldg, dX, ldx, d, (int)b0);
        else
            hipLaunchKernelGGL(k_gconv_rows_adjoint<1>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t,
                               values_t, n, pos, B, G, ldg, dX, ldx, d, (int)b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
