// srg_link.hip -- the edge head of link classification (srgnn.link): the reference ends every
// base model with linear(cat(f[q0], f[q1])).  Re-associated, the dense products run at node count through
// torch and the two passes over the query pairs are C wide:
//
//   srg_pair_gather_add_f32     out[e, c] = (P[q0[e], c] + P[q1[e], C + c]) + b[c]          forward
//   srg_pair_segment_sum_f32    S[v, side C + c] = sum of g[e, c] over the slots (e, side)   backward
//                               of node v, one add chain from +0.0f in ascending e
//
// Lanes by columns, rows by lane groups (the layout of the packed light rows): a row of C columns is
// ceil(C / VEC) chunks; L, the power of two >= the chunks and at most 64, lanes take one chunk each, and
// 64 / L edges (or nodes) share a wave.  Past 64 chunks a wave owns one row and blockIdx.y walks tiles of
// 64 chunks.  An element's bits depend on neither L, the tile, the load path (VEC 4: 16-byte accesses,
// VEC 1: 4-byte accesses) nor the launch.  No atomics, no scratch, no LDS; every store is a plain vector store.
//
// Cost of a long segment: a node's slots are one lane group's serial chain, kPairSlots loads in flight;
// the other groups of its wave wait for the longest of them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

constexpr int kPairSlots = 4;   // slots of one segment in flight

template <int VEC>
__device__ __forceinline__ typename Vec<float, VEC>::type vadd(const typename Vec<float, VEC>::type& a,
                                                               const typename Vec<float, VEC>::type& b)
{
    typename Vec<float, VEC>::type r;
    if constexpr (VEC == 1) {
        r = __fadd_rn(a, b);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) r[i] = __fadd_rn(a[i], b[i]);
    }
    return r;
}

// group g = lane >> lgL holds row (wave slot) * (64 >> lgL) + g; lane c0 = lane & (L - 1) its chunk
// blockIdx.y * 64 + c0.  An id outside [0, U) is a row of +0 and never an address.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_pair_gather_add(const float* __restrict__ P, int64_t ldp, int64_t U, const int64_t* __restrict__ q,
                  const float* __restrict__ b, int64_t E, int C, float* __restrict__ out, int64_t ldo, int lgL,
                  int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)wave_slot(block_base) * (64 >> lgL) + (lane >> lgL);
    const int col = ((int)blockIdx.y * 64 + (lane & ((1 << lgL) - 1))) * VEC;
    if (e >= E || col >= C) return;   // the kernel has neither a barrier nor a cross-lane operation
    const int64_t q0 = q[2 * e], q1 = q[2 * e + 1];
    V p0 = vzero<float, VEC>(), p1 = vzero<float, VEC>();
    if (q0 >= 0 && q0 < U) p0 = gload<float, VEC>(P + q0 * ldp + col);
    if (q1 >= 0 && q1 < U) p1 = gload<float, VEC>(P + q1 * ldp + C + col);
    V r = vadd<VEC>(p0, p1);
    if (b) r = vadd<VEC>(r, vload<float, VEC>(b + col));
    vstore<float, VEC>(out + e * ldo + col, r, false);
}

// group g holds node v; its lanes walk inc_slot[inc_ptr[v] .. inc_ptr[v + 1]) in stored order, kPairSlots
// rows of g in flight, and keep one accumulator per side.  A slot is added to its own side's chain only
// (never as + 0 to the other).  A slot outside [0, 2E) is skipped and never an address; the segment's
// bounds are clamped to the 2E slots there are.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_pair_segment_sum(const float* __restrict__ g, int64_t ldg, int64_t E, const int64_t* __restrict__ inc_ptr,
                   const int64_t* __restrict__ inc_slot, int64_t U, int C, float* __restrict__ S, int64_t lds,
                   int lgL, int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)wave_slot(block_base) * (64 >> lgL) + (lane >> lgL);
    const int col = ((int)blockIdx.y * 64 + (lane & ((1 << lgL) - 1))) * VEC;
    if (v >= U || col >= C) return;   // the kernel has neither a barrier nor a cross-lane operation
    const int64_t n_slots = 2 * E;
    int64_t beg = inc_ptr[v], end = inc_ptr[v + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > n_slots ? n_slots : end;
    V acc0 = vzero<float, VEC>(), acc1 = vzero<float, VEC>();
    for (int64_t j = beg; j < end; j += kPairSlots) {
        int64_t sl[kPairSlots];
        V x[kPairSlots];
#pragma unroll
        for (int u = 0; u < kPairSlots; ++u) sl[u] = j + u < end ? inc_slot[j + u] : -1;
#pragma unroll
        for (int u = 0; u < kPairSlots; ++u) {
            const bool ok = sl[u] >= 0 && sl[u] < n_slots;
            if (!ok) sl[u] = -1;
            x[u] = ok ? gload<float, VEC>(g + (sl[u] >> 1) * ldg + col) : vzero<float, VEC>();
        }
#pragma unroll
        for (int u = 0; u < kPairSlots; ++u) {
            if (sl[u] < 0) continue;
            if (sl[u] & 1)
                acc1 = vadd<VEC>(acc1, x[u]);
            else
                acc0 = vadd<VEC>(acc0, x[u]);
        }
    }
    float* row = S + v * lds + col;
    vstore<float, VEC>(row, acc0, false);
    vstore<float, VEC>(row + C, acc1, false);
}

struct PairGrid {
    int lgL;
    unsigned tiles;
    int64_t blocks;
};

// rows of C columns in VEC-wide chunks over n rows: the lanes of a row, the column tiles and the blocks
PairGrid pair_grid(int C, int vec, int64_t n)
{
    const int cpr = (C + vec - 1) / vec;
    int lgL = 0;
    while (lgL < 6 && (1 << lgL) < cpr) ++lgL;
    const int64_t rows_per_block = (int64_t)kWavesPerBlock * (64 >> lgL);
    return {lgL, (unsigned)((cpr + 63) / 64), (n + rows_per_block - 1) / rows_per_block};
}

int check_pair_sizes(int64_t E, int64_t U, int C, int64_t lda, int64_t need_a, const char* na, int64_t ldb,
                     int64_t need_b, const char* nb)
{
    if (E < 0 || E > INT32_MAX - 64 || U < 0 || U > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "E=%lld, U=%lld out of range [0, 2^31-64)", (long long)E, (long long)U);
    if (C < 0 || C > (1 << 20)) return srg_fail(SRG_ERR_INVALID, "C=%d out of range [0, 2^20]", C);
    if (lda < need_a || ldb < need_b)
        return srg_fail(SRG_ERR_INVALID, "leading dimensions (%s=%lld < %lld or %s=%lld < %lld)", na, (long long)lda,
                        (long long)need_a, nb, (long long)ldb, (long long)need_b);
    return SRG_OK;
}

}  // namespace

extern "C" {

int srg_pair_gather_add_f32(const float* P, int64_t ldp, int64_t U, const int64_t* q, const float* b, int64_t E,
                            int32_t C, float* out, int64_t ldo, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_pair_sizes(E, U, C, ldp, 2 * (int64_t)C, "ldp", ldo, C, "ldo");
    if (rc) return rc;
    if (E == 0 || C == 0) return srg_ok();
    if (!q || !out) return srg_fail(SRG_ERR_INVALID, "null q or out");
    if (U > 0 && !P) return srg_fail(SRG_ERR_INVALID, "null P with U=%lld", (long long)U);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the second half of a row of P starts C elements in, b has no rows: both are whole accesses with C % 4 == 0
    const bool v4 = rows_aligned(4, sizeof(float), C, {{P, ldp}, {out, ldo}, {b, 0}});
    const PairGrid pg = pair_grid(C, v4 ? 4 : 1, E);
    rc = launch_chunks_capped(pg.blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (v4)
            hipLaunchKernelGGL(k_pair_gather_add<4>, dim3(nb, pg.tiles), dim3(kBlock), 0, s, P, ldp, U, q, b, E, (int)C,
                               out, ldo, pg.lgL, (int)b0);
        else
            hipLaunchKernelGGL(k_pair_gather_add<1>, dim3(nb, pg.tiles), dim3(kBlock), 0, s, P, ldp, U, q, b, E, (int)C,
                               out, ldo, pg.lgL, (int)b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_pair_segment_sum_f32(const float* g, int64_t ldg, int64_t E, const int64_t* inc_ptr, const int64_t* inc_slot,
                             int64_t U, int32_t C, float* S, int64_t lds, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_pair_sizes(E, U, C, ldg, C, "ldg", lds, 2 * (int64_t)C, "lds");
    if (rc) return rc;
    if (U == 0 || C == 0) return srg_ok();
    if (!inc_ptr || !S) return srg_fail(SRG_ERR_INVALID, "null inc_ptr or S");
    if (E > 0 && (!g || !inc_slot)) return srg_fail(SRG_ERR_INVALID, "null g or inc_slot with E=%lld", (long long)E);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool v4 = rows_aligned(4, sizeof(float), C, {{g, ldg}, {S, lds}});
    const PairGrid pg = pair_grid(C, v4 ? 4 : 1, U);
    rc = launch_chunks_capped(pg.blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (v4)
            hipLaunchKernelGGL(k_pair_segment_sum<4>, dim3(nb, pg.tiles), dim3(kBlock), 0, s, g, ldg, E, inc_ptr, inc_slot,
                               U, (int)C, S, lds, pg.lgL, (int)b0);
        else
            hipLaunchKernelGGL(k_pair_segment_sum<1>, dim3(nb, pg.tiles), dim3(kBlock), 0, s, g, ldg, E, inc_ptr, inc_slot,
                               U, (int)C, S, lds, pg.lgL, (int)b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
