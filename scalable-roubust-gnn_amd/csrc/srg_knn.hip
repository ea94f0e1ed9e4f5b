// srg_knn.hip -- edge augmentation's per-node work for all low-degree nodes at once (edge_augument,
// SSRG/data_augument.py:73-103): the draw of every query row's candidates (srg_sample_distinct_i64) and
// the distance to each candidate plus the selection of the nearest (srg_knn_select_f32).
//
// The distance's summation order (restated by tests/edge_augment_ref.py), a function of d alone:
//   P = ceil(d / 4) pieces of 4 consecutive columns; G = the smallest power of two >= P, at most 64.
//   p_g, g < G: the pieces g, g + G, g + 2G, ... in that order, inside a piece the columns ascending, one
//   chain from +0 of the separately rounded squares of the separately rounded differences.
//   Halving tree: for h = G/2 .. 1: p_g = p_g + p_{g+h}, g < h.  dist = sqrt(p_0), correctly rounded.
// G lanes own one candidate row (lane g = p_g), so a wave reads 64 / G candidate rows per step and kU
// steps are in flight; the 16-byte and the 4-byte load path give a lane the same columns, so the bits do
// not depend on the path.  No atomics touch a result; the argument check's status word is the only one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

constexpr uint32_t kKeyInf = 0x7F800000u;       // +Inf: the largest key of a distance that is a number
constexpr uint32_t kKeyNaN = 0x7F800001u;       // every NaN distance, after +Inf
constexpr uint32_t kKeyOutside = 0x7F800002u;   // a candidate id outside [0, n), after every distance
constexpr uint32_t kKeyTaken = 0xFFFFFFFFu;     // selected in an earlier round
constexpr uint32_t kQuietNaN = 0x7FC00000u;
constexpr int kU = 4;                           // candidate rows in flight per lane group
// SRG_KNN_LAUNCH_ROWS (include/srgnn_hip.h) rows go out per launch whatever the workgroup's size; more rows
// go out in further launches (block_base).  Workgroups hold 1, 2 or 4 waves, so the division is exact.
static_assert(SRG_KNN_LAUNCH_ROWS % kWavesPerBlock == 0 && SRG_KNN_LAUNCH_ROWS <= kMaxLaunchBlocks,
              "a launch's rows fill whole workgroups and fit one grid");

constexpr unsigned kBadCandPtr = 1u, kBadOutPtr = 2u, kBadQuery = 4u, kBadCap = 8u;
constexpr unsigned kAnyResult = 0x100u;   // not an error: some row asks for a result

// Argument check of both entries: status[0] |= what is wrong, status[1] = the longest candidate list.
__global__ void __launch_bounds__(256)
k_knn_check(const int64_t* __restrict__ query, const int64_t* __restrict__ cand_ptr,
            const int64_t* __restrict__ out_ptr, int64_t n_query, int64_t n, int64_t cap,
            unsigned int* __restrict__ status)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int bad = 0, longest = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_query; r += stride) {
        const int64_t m = cand_ptr[r + 1] - cand_ptr[r];
        if (m < 0 || (r == 0 && cand_ptr[0] < 0)) bad |= kBadCandPtr;
        if (m > cap) bad |= kBadCap;
        if (out_ptr) {
            const int64_t k = out_ptr[r + 1] - out_ptr[r];
            if (k < 0 || k > m || (r == 0 && out_ptr[0] < 0)) bad |= kBadOutPtr;
            if (k > 0) bad |= kAnyResult;
        }
        const int64_t q = query[r];
        if (q < 0 || q >= n) bad |= kBadQuery;
        const unsigned int mm = m < 0 ? 0u : m > INT32_MAX ? (unsigned)INT32_MAX : (unsigned)m;
        longest = mm > longest ? mm : longest;
    }
    if (bad) atomicOr(status, bad);
    if (longest) atomicMax(status + 1, longest);
}

// one wave's LDS writes become visible to its own later reads (the LDS serves a wave's operations in order)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One wave per query row.  LDS per wave: the query row (q_stride floats, zero padded to a multiple of 4)
// and one key per candidate (key_stride of them).  The distance phase writes a key per candidate:
// the distance's bits (a non-negative float orders as its bits), kKeyNaN or kKeyOutside.  The selection
// phase runs k rounds of arg-min over (key, position): every lane scans positions lane, lane + 64, ...,
// the wave reduces the 64-bit (key << 32 | position) by a minimum, lane 0 writes the winner and marks it.
template <int G, bool V4>
__global__ void __launch_bounds__(kBlock)
k_knn_select(const float* __restrict__ X, int64_t ldx, int64_t n, int d, const int64_t* __restrict__ query,
             const int64_t* __restrict__ cand_ptr, const int64_t* __restrict__ cand,
             const int64_t* __restrict__ out_ptr, int64_t n_query, int64_t* __restrict__ sel,
             float* __restrict__ sel_dist, int key_stride, int q_stride, int64_t block_base)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    constexpr int CPS = 64 / G;   // candidate rows per wave step
    const int wpb = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* qrow = reinterpret_cast<float*>(knn_lds) + (int64_t)w * q_stride;
    uint32_t* keys = reinterpret_cast<uint32_t*>(knn_lds) + (int64_t)wpb * q_stride + (int64_t)w * key_stride;
    const int64_t r = (block_base + blockIdx.x) * wpb + w;
    if (r >= n_query) return;   // wave-uniform; the kernel has no workgroup barrier
    const int64_t q = query[r], cp = cand_ptr[r], op = out_ptr[r];
    const int M = (int)std::min<int64_t>(cand_ptr[r + 1] - cp, key_stride);
    const int k = (int)std::min<int64_t>(out_ptr[r + 1] - op, M);
    if (k <= 0) return;

    for (int j = lane; j < q_stride; j += 64) qrow[j] = j < d ? X[q * ldx + j] : 0.0f;
    wave_lds_sync();

    const int g = lane % G, grp = lane / G;
    const int full = d >> 2, rest = d & 3;   // pieces of 4 columns, columns of the partial last piece
    for (int base = 0; base < M; base += CPS * kU) {
        // an id outside [0, n) (and a position past the list) reads the query row instead: always an address
        // inside X and no branch around the loads; its key is kKeyOutside whatever that gives
        const float* row[kU];
        bool ok[kU];
        float acc[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int pos = base + u * CPS + grp;
            const int64_t id = pos < M ? cand[cp + pos] : -1;
            ok[u] = id >= 0 && id < n;
            row[u] = X + (ok[u] ? id : q) * ldx;
            acc[u] = 0.0f;
        }
        for (int piece = g; piece < full; piece += G) {
            const int j = piece * 4;
            const typename Vec<float, 4>::type qv = *reinterpret_cast<const typename Vec<float, 4>::type*>(qrow + j);
            typename Vec<float, 4>::type x[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if constexpr (V4) {
                    x[u] = gload<float, 4>(row[u] + j);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[u][e] = row[u][j + e];
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = __fsub_rn(qv[e], x[u][e]);
                    acc[u] = __fadd_rn(acc[u], __fmul_rn(t, t));
                }
            }
        }
        // the partial piece is the last piece of its lane's chain
        if (rest && g == full % G) {
            const int j = full * 4;
            float x[kU][3];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int e = 0; e < 3; ++e) x[u][e] = e < rest ? row[u][j + e] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if (e < rest) {
                        const float t = __fsub_rn(qrow[j + e], x[u][e]);
                        acc[u] = __fadd_rn(acc[u], __fmul_rn(t, t));
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
#pragma unroll
            for (int h = G / 2; h >= 1; h >>= 1) acc[u] = __fadd_rn(acc[u], __shfl_xor(acc[u], h, 64));
            const int pos = base + u * CPS + grp;
            if (g == 0 && pos < M) {
                const float dist = __builtin_sqrtf(acc[u]);   // llvm.sqrt.f32: the correctly rounded expansion
                keys[pos] = !ok[u] ? kKeyOutside : dist != dist ? kKeyNaN : __float_as_uint(dist);
            }
        }
    }
    wave_lds_sync();

    for (int i = 0; i < k; ++i) {
        unsigned long long best = ~0ull;
        for (int pos = lane; pos < M; pos += 64) {
            const unsigned long long c = ((unsigned long long)keys[pos] << 32) | (unsigned)pos;
            best = c < best ? c : best;
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
            const unsigned long long o = __shfl_xor(best, h, 64);
            best = o < best ? o : best;
        }
        const int pos = (int)(best & 0xFFFFFFFFull);
        const uint32_t key = (uint32_t)(best >> 32);
        if (lane == 0) {
            sel[op + i] = cand[cp + pos];
            if (sel_dist) sel_dist[op + i] = __uint_as_float(key <= kKeyInf ? key : kQuietNaN);
            keys[pos] = kKeyTaken;
        }
        wave_lds_sync();
    }
}

// One wave per row, a lane per draw: the keyed Feistel bijection of [0, 4^h) walked from t until it
// lands below m = n - 1 (FeistelWalk, srg_device.h; include/srgnn_hip.h states the arithmetic), then shifted
// past the query node.  A walk that hit its bound (a bijection's never does) writes -1, an id the selection
// treats as outside and never reads.
__global__ void __launch_bounds__(kBlock)
k_sample_distinct(const int64_t* __restrict__ query, const int64_t* __restrict__ cand_ptr, int64_t n_query,
                  int64_t n, uint64_t seed, int64_t* __restrict__ cand, int64_t block_base)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (block_base + blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (r >= n_query) return;   // wave-uniform
    const int64_t cp = cand_ptr[r], M = cand_ptr[r + 1] - cp;
    const uint64_t q = (uint64_t)query[r];
    const FeistelWalk fw(sample_key(seed, (uint64_t)r), (uint64_t)(n - 1));
    for (int64_t t = lane; t < M; t += 64) {
        const uint64_t x = fw.walk((uint64_t)t);
        cand[cp + t] = x == kWalkFailed ? -1 : (int64_t)(x + (x >= q ? 1 : 0));
    }
}

int check_into(unsigned int* d_status, const int64_t* query, const int64_t* cand_ptr, const int64_t* out_ptr,
               int64_t n_query, int64_t n, int64_t cap, hipStream_t s, unsigned int status[2])
{
    SRG_HIP_CHECK(hipMemsetAsync(d_status, 0, 2 * sizeof(unsigned int), s));
    const unsigned blocks = (unsigned)std::min<int64_t>((n_query + 255) / 256, launch_cap(8192));
    hipLaunchKernelGGL(k_knn_check, dim3(blocks), dim3(256), 0, s, query, cand_ptr, out_ptr, n_query, n, cap,
                       d_status);
    SRG_HIP_CHECK(hipGetLastError());
    SRG_HIP_CHECK(hipMemcpyAsync(status, d_status, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    return SRG_OK;
}

// Runs the check on `s` and waits for it: status[0] = the flags, status[1] = the longest list.  The status
// words are freed on every path; the wait for the copy to the host is why neither entry can be captured
// into a graph.
int run_check(const int64_t* query, const int64_t* cand_ptr, const int64_t* out_ptr, int64_t n_query, int64_t n,
              int64_t cap, hipStream_t s, unsigned int status[2])
{
    unsigned int* d_status = nullptr;
    SRG_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&d_status), 2 * sizeof(unsigned int), s));
    const int rc = check_into(d_status, query, cand_ptr, out_ptr, n_query, n, cap, s, status);
    const hipError_t freed = hipFreeAsync(d_status, s);
    if (rc) return rc;
    SRG_HIP_CHECK(freed);
    SRG_HIP_CHECK(hipStreamSynchronize(s));
    return SRG_OK;
}

int group_lanes(int d)
{
    const int pieces = (d + 3) / 4;
    int G = 1;
    while (G < pieces && G < 64) G *= 2;
    return G;
}

template <int G>
void launch_select(bool v4, dim3 grid, dim3 block, size_t lds, hipStream_t s, const float* X, int64_t ldx, int64_t n,
                   int d, const int64_t* query, const int64_t* cand_ptr, const int64_t* cand, const int64_t* out_ptr,
                   int64_t n_query, int64_t* sel, float* sel_dist, int key_stride, int q_stride, int64_t b0)
{
    if (v4)
        hipLaunchKernelGGL((k_knn_select<G, true>), grid, block, lds, s, X, ldx, n, d, query, cand_ptr, cand, out_ptr,
                           n_query, sel, sel_dist, key_stride, q_stride, b0);
    else
        hipLaunchKernelGGL((k_knn_select<G, false>), grid, block, lds, s, X, ldx, n, d, query, cand_ptr, cand,
                           out_ptr, n_query, sel, sel_dist, key_stride, q_stride, b0);
}

}  // namespace

extern "C" {

int srg_knn_select_f32(const float* X, int64_t ldx, int64_t n, int32_t d, const int64_t* query,
                       const int64_t* cand_ptr, const int64_t* cand, const int64_t* out_ptr, int64_t n_query,
                       int64_t* sel, float* sel_dist, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_query < 0 || n < 0) return srg_fail(SRG_ERR_INVALID, "n_query=%lld, n=%lld: negative size",
                                              (long long)n_query, (long long)n);
    if (d < 0 || d > SRG_KNN_MAX_D) return srg_fail(SRG_ERR_INVALID, "d=%d outside [0, %d]", d, SRG_KNN_MAX_D);
    if (ldx < d) return srg_fail(SRG_ERR_INVALID, "leading dimension ldx=%lld < d=%d", (long long)ldx, d);
    if (n_query == 0) return srg_ok();
    if (!query || !cand_ptr || !out_ptr) return srg_fail(SRG_ERR_INVALID, "null query, cand_ptr or out_ptr");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned int status[2] = {0, 0};
    int rc = run_check(query, cand_ptr, out_ptr, n_query, n, SRG_KNN_MAX_CAND, s, status);
    if (rc) return rc;
    if (status[0] & kBadCandPtr) return srg_fail(SRG_ERR_INVALID, "cand_ptr decreases or starts below 0");
    if (status[0] & kBadCap)
        return srg_fail(SRG_ERR_INVALID, "a row has more than SRG_KNN_MAX_CAND=%d candidates", SRG_KNN_MAX_CAND);
    if (status[0] & kBadOutPtr)
        return srg_fail(SRG_ERR_INVALID, "out_ptr decreases, starts below 0 or a row asks for more results than it has candidates (k > M)");
    if (status[0] & kBadQuery) return srg_fail(SRG_ERR_INVALID, "query id outside [0, %lld)", (long long)n);
    if (!(status[0] & kAnyResult)) return srg_ok();   // no row asks for a result: nothing to select
    if (!cand || !sel || (d > 0 && !X)) return srg_fail(SRG_ERR_INVALID, "null X, cand or sel");

    const int key_stride = (int)((status[1] + 63u) / 64u * 64u);
    const int q_stride = (d + 3) / 4 * 4;
    const size_t per_wave = (size_t)(key_stride + q_stride) * 4;   // <= (4096 + 8192) * 4 bytes
    int wpb = kWavesPerBlock;
    while (wpb > 1 && wpb * per_wave > 65536) wpb /= 2;
    const size_t lds = wpb * per_wave;
    const bool v4 = rows_aligned(4, sizeof(float), 0, {{X, ldx}});   // whatever d is: a row's tail is read by the element
    const int G = group_lanes(d);
    rc = launch_chunks_capped((n_query + wpb - 1) / wpb, SRG_KNN_LAUNCH_ROWS / wpb, [&](int64_t b0, unsigned nb) {
        const dim3 grid(nb), block(64 * wpb);
#define SRG_KNN_CASE(GG)                                                                                        \
    case GG:                                                                                                    \
        launch_select<GG>(v4, grid, block, lds, s, X, ldx, n, d, query, cand_ptr, cand, out_ptr, n_query, sel,   \
                          sel_dist, key_stride, q_stride, b0);                                                  \
        break
        switch (G) {
            SRG_KNN_CASE(1);
            SRG_KNN_CASE(2);
            SRG_KNN_CASE(4);
            SRG_KNN_CASE(8);
            SRG_KNN_CASE(16);
            SRG_KNN_CASE(32);
            default:
            SRG_KNN_CASE(64);
        }
#undef SRG_KNN_CASE
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_sample_distinct_i64(const int64_t* query, const int64_t* cand_ptr, int64_t n_query, int64_t n,
                            uint64_t seed, int64_t* cand, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_query < 0 || n < 0 || n > (int64_t(1) << 62))
        return srg_fail(SRG_ERR_INVALID, "n_query=%lld, n=%lld: negative size or n > 2^62", (long long)n_query,
                        (long long)n);
    if (n_query == 0) return srg_ok();
    if (!query || !cand_ptr) return srg_fail(SRG_ERR_INVALID, "null query or cand_ptr");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned int status[2] = {0, 0};
    int rc = run_check(query, cand_ptr, nullptr, n_query, n, n - 1, s, status);
    if (rc) return rc;
    if (status[0] & kBadCandPtr) return srg_fail(SRG_ERR_INVALID, "cand_ptr decreases or starts below 0");
    if (status[0] & kBadCap)
        return srg_fail(SRG_ERR_INVALID, "a row asks for more than n - 1 = %lld distinct candidates", (long long)n - 1);
    if (status[0] & kBadQuery) return srg_fail(SRG_ERR_INVALID, "query id outside [0, %lld)", (long long)n);
    if (status[1] == 0) return srg_ok();
    if (!cand) return srg_fail(SRG_ERR_INVALID, "null cand");
    const int64_t blocks = (n_query + kWavesPerBlock - 1) / kWavesPerBlock;
    rc = launch_chunks_capped(blocks, SRG_KNN_LAUNCH_ROWS / kWavesPerBlock, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_sample_distinct, dim3(nb), dim3(kBlock), 0, s, query, cand_ptr, n_query, n, seed, cand, b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
