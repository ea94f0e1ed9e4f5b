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
// rounds of 8 gathers in flight (row_gather); in the adjoint a row of L entries with M members costs
// L / 64 rounds of (ids -> positions -> ballot) plus M / 8 gather rounds, whatever the other waves do.
#include <hip/hip_runtime.h>

#include <algorithm>
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

// dX[c, col ..] = the chain over row c of the transposed operator, member entries only.  Lanes across
// entries for the membership test (64 ids, their positions, one ballot), lanes across columns for the
// chain: the ballot is walked from its lowest set bit, so the chain keeps the stored order.  kUnroll member
// rows of G are in flight; slots past the last member repeat it (always a valid address) and are skipped
// by a wave-uniform predicate.  The next 64 ids are loaded while this block is walked.
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
    const int64_t beg = indptr[c], end = indptr[c + 1];
    if (beg < end) {
        int64_t j0 = beg + lane;
        int id_nxt = j0 < end ? indices[j0] : -1;
        for (int64_t jb = beg; jb < end; jb += 64) {
            const int id = id_nxt;
            const int64_t j = jb + lane, jn = jb + 64 + lane;
            id_nxt = jn < end ? indices[jn] : -1;
            // an id outside [0, n) is never an address; a position outside [0, B) is no member
            int p = -1;
            if (id >= 0 && id < n) p = pos[id];
            const bool member = p >= 0 && p < B;
            const float a_blk = member ? values[j] : 0.0f;
            unsigned long long mask = __ballot(member);
            while (mask) {
                const int m = __builtin_popcountll(mask);
                const int cnt = m < kUnroll ? m : kUnroll;   // wave-uniform
                V x[kUnroll];
                float a[kUnroll];
                int q = 0;
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    if (mask) {
                        q = __builtin_ctzll(mask);
                        mask &= mask - 1;
                    }
                    const int pq = __builtin_amdgcn_readlane(p, q);
                    a[u] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a_blk), q));
                    if (act)
                        x[u] = gload<float, VEC>(G + (int64_t)pq * ldg + col);
                    else
                        x[u] = vzero<float, VEC>();
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u)
                    if (u < cnt) chain<float, VEC>(acc, a[u], x[u]);
            }
        }
    }
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

bool vec4_ok(int d, const void* a, int64_t lda, const void* b, int64_t ldb)
{
    return d % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && aligned(a, 16) && aligned(b, 16);
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
    const bool v4 = vec4_ok(d, X, ldx, Y, ldy);
    const int tile = v4 ? 256 : 64;
    const unsigned tiles = (unsigned)((d + tile - 1) / tile);
    const int64_t blocks = (B + kWavesPerBlock - 1) / kWavesPerBlock, per_launch = kMaxLaunchBlocks;
    for (int64_t b0 = 0; b0 < blocks; b0 += per_launch) {
        const dim3 grid((unsigned)std::min<int64_t>(per_launch, blocks - b0), tiles);
        if (v4)
            hipLaunchKernelGGL(k_gconv_rows<4>, grid, dim3(kBlock), 0, s, indptr, indices, values, n_rows, rows, B, X,
                               ldx, Y, ldy, d, (int)b0);
        else
            hipLaunchKernelGGL(k_gconv_rows<1>, grid, dim3(kBlock), 0, s, indptr, indices, values, n_rows, rows, B, X,
                               ldx, Y, ldy, d, (int)b0);
        SRG_HIP_CHECK(hipGetLastError());
    }
    return srg_ok();
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
    const bool v4 = vec4_ok(d, G, ldg, dX, ldx);
    const int tile = v4 ? 256 : 64;
    const unsigned tiles = (unsigned)((d + tile - 1) / tile);
    const int64_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock, per_launch = kMaxLaunchBlocks;
    for (int64_t b0 = 0; b0 < blocks; b0 += per_launch) {
        const dim3 grid((unsigned)std::min<int64_t>(per_launch, blocks - b0), tiles);
        if (v4)
            hipLaunchKernelGGL(k_gconv_rows_adjoint<4>, grid, dim3(kBlock), 0, s, indptr_t, indices_t, values_t, n, pos,
                               B, G, ldg, dX, ldx, d, (int)b0);
        else
            hipLaunchKernelGGL(k_gconv_rows_adjoint<1>, grid, dim3(kBlock), 0, s, indptr_t, indices_t, values_t, n, pos,
                               B, G, ldg, dX, ldx, d, (int)b0);
        SRG_HIP_CHECK(hipGetLastError());
    }
    return srg_ok();
}

}  // extern "C"
