// srg_sample.hip -- neighbour sampling's row slice (srgnn.neighbor): rows nodes[b] of the
// operator with at most `fanout` entries each, the sampled analogue of the row slice of srg_csr_induced_f32.
//
// A row of len entries receives cnt = len entries if fanout < 0 or len <= fanout (a copy in stored order)
// and fanout otherwise: the positions p_t = walk(t), t < fanout, of the keyed bijection of [0, len)
// (FeistelWalk, srg_device.h), keyed by the node id, emitted in ascending position.  The count is closed
// form, so the caller forms ptr before the one launch; the kernel writes a row only where ptr[b + 1] - ptr[b]
// is its own cnt.  Column ids are copied and never used as addresses; a nodes[b] outside [0, n_rows) is an
// empty row.  Nothing is added atomically: the output is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// One wave per kSampleRowsPerWave = 4 consecutive batch rows, 16 lanes each, as k_csr_induced lays its rows
// out (lane l of group g holds entry beg + 16 t + l of row 4 w + g in step t): a copied row of at most
// kSampleShort = 64 entries is written by its group, all four steps' loads in flight at once.  The other rows
// go to the whole wave afterwards, one after the other:
//   a sampled row (len > fanout): lane t < fanout walks draw t; every lane ranks its position among the
//     row's draws with one v_readlane and one compare per draw (the draws are distinct, so the ranks are a
//     permutation of [0, fanout)), then gathers its entry and stores it at its rank.  fanout gathers,
//     whatever len is.  A walk that hit its bound (a bijection's never does) leaves the whole row unwritten;
//   a copied row longer than 64 entries (fanout < 0 only): 64 entries per step, kSampleWide steps in flight.
constexpr int kSampleRowsPerWave = 4;
constexpr int kSampleSteps = 4;
constexpr int64_t kSampleShort = 16 * kSampleSteps;
constexpr int kSampleWide = 4;
static_assert(SRG_SAMPLE_MAX_FANOUT == 64, "one wave holds a row's draws, one per lane");

__device__ __forceinline__ void sample_store(int64_t o, int64_t j, const int32_t* __restrict__ indices,
                                             const float* __restrict__ values, int32_t* __restrict__ out_idx,
                                             float* __restrict__ out_val, int64_t* __restrict__ out_eid)
{
    out_idx[o] = indices[j];
    if (out_val) out_val[o] = values[j];
    if (out_eid) out_eid[o] = j;
}

__global__ void __launch_bounds__(kBlock)
k_csr_sample(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
             const float* __restrict__ values, int64_t n_rows, const int64_t* __restrict__ nodes, int64_t B,
             int fanout, uint64_t seed, const int64_t* __restrict__ ptr, int32_t* __restrict__ out_idx,
             float* __restrict__ out_val, int64_t* __restrict__ out_eid, int block_base)
{
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, l = lane & 15;
    const int64_t b = (int64_t)wave_slot(block_base) * kSampleRowsPerWave + g;
    const bool valid = b < B;
    const int64_t r = valid ? nodes[b] : -1;
    const bool has_row = r >= 0 && r < n_rows;
    const int64_t beg = has_row ? indptr[r] : 0;
    const int64_t len = has_row ? indptr[r + 1] - beg : 0;
    const bool sampled = fanout > 0 && len > fanout;
    const int64_t cnt = sampled ? fanout : len;
    const int64_t row_out = valid ? ptr[b] : 0;
    // the caller's ptr is trusted only where it agrees with the count made here (a sampled row of 2^31 entries
    // or more is past the documented limit and is not written either)
    const bool ok = valid && cnt > 0 && ptr[b + 1] - row_out == cnt && !(sampled && len > INT32_MAX);
    const bool wide = ok && (sampled || len > kSampleShort);

    // ---- copied rows of at most 64 entries: the four groups side by side ----
    if (ok && !wide) {
#pragma unroll
        for (int t = 0; t < kSampleSteps; ++t) {
            const int64_t p = 16 * t + l;
            if (p < len) sample_store(row_out + p, beg + p, indices, values, out_idx, out_val, out_eid);
        }
    }

    // ---- sampled rows and long copies: the whole wave, one row after the other ----
    unsigned long long todo = __ballot(wide && l == 0);   // wave-uniform
    while (todo) {
        const int q = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t wb = bcast_lane(beg, q), wl = bcast_lane(len, q), wo = bcast_lane(row_out, q);
        const int64_t wr = bcast_lane(r, q);
        if (fanout > 0) {
            const FeistelWalk fw(sample_key(seed, (uint64_t)wr), (uint64_t)wl);
            const uint64_t x = lane < fanout ? fw.walk((uint64_t)lane) : 0;
            if (__ballot(lane < fanout && x >= (uint64_t)wl)) continue;   // kWalkFailed: the row stays empty
            const int p = (int)x;   // < len < 2^31
            int rank = 0;
            for (int s = 0; s < fanout; ++s) rank += __builtin_amdgcn_readlane(p, s) < p ? 1 : 0;
            if (lane < fanout) sample_store(wo + rank, wb + p, indices, values, out_idx, out_val, out_eid);
        } else {
            for (int64_t j0 = 0; j0 < wl; j0 += 64 * kSampleWide) {
#pragma unroll
                for (int u = 0; u < kSampleWide; ++u) {
                    const int64_t p = j0 + 64 * u + lane;
                    if (p < wl) sample_store(wo + p, wb + p, indices, values, out_idx, out_val, out_eid);
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int srg_csr_sample_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                       const int64_t* nodes, int64_t B, int32_t fanout, uint64_t seed, const int64_t* ptr,
                       int32_t* out_idx, float* out_val, int64_t* out_eid, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0 || B < 0)
        return srg_fail(SRG_ERR_INVALID, "negative size (n_rows=%lld, B=%lld)", (long long)n_rows, (long long)B);
    if (fanout == 0 || fanout > SRG_SAMPLE_MAX_FANOUT)
        return srg_fail(SRG_ERR_INVALID, "fanout=%d is neither in [1, %d] nor negative (every entry)", fanout,
                        SRG_SAMPLE_MAX_FANOUT);
    if (B > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "B=%lld >= 2^31", (long long)B);
    if (B == 0) return srg_ok();
    if (!nodes || !ptr || !out_idx) return srg_fail(SRG_ERR_INVALID, "null nodes, ptr or out_idx");
    if (n_rows > 0 && (!indptr || !indices)) return srg_fail(SRG_ERR_INVALID, "null indptr or indices");
    if (out_val && !values) return srg_fail(SRG_ERR_INVALID, "out_val without values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows_per_block = (int64_t)kWavesPerBlock * kSampleRowsPerWave;
    const int rc = launch_chunks_capped((B + rows_per_block - 1) / rows_per_block, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_csr_sample, dim3(nb), dim3(kBlock), 0, s, indptr, indices, values, n_rows, nodes, B,
                           (int)fanout, seed, ptr, out_idx, out_val, out_eid, (int)b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
