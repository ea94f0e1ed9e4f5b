// srg_device.h -- device code that more than one kernel family uses: vector loads and stores, the chain
// link and the epilogue arithmetic, the row-wave gather, the filtered row walk, the rows-by-lanes layout of
// the streaming reductions, the samplers' keyed bijection (host and device), the launch constants; and
// the host checks that go with them, the vector-width check among them.  Everything is in the anonymous
// namespace: each translation unit that includes this header compiles its own copy into its own kernels.
// Not part of the C-ABI (include/srgnn_hip.h).
#ifndef SRG_DEVICE_H_
#define SRG_DEVICE_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "srgnn_hip.h"
#include "srg_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------
// vector helpers
// ------------------------------------------------------------------------------------------------
template <typename T, int VEC> struct Vec;
template <> struct Vec<float, 1> { typedef float type; };
template <> struct Vec<float, 2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Vec<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct Vec<double, 1> { typedef double type; };
template <> struct Vec<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };

// element i of a scalar-or-vector value
template <typename T> __device__ __forceinline__ T& elem(T& v, int) { return v; }
template <typename T> __device__ __forceinline__ const T& elem(const T& v, int) { return v; }
template <typename T, int N>
__device__ __forceinline__ T& elem(T __attribute__((ext_vector_type(N)))& v, int i) { return reinterpret_cast<T*>(&v)[i]; }
template <typename T, int N>
__device__ __forceinline__ const T& elem(const T __attribute__((ext_vector_type(N)))& v, int i) { return reinterpret_cast<const T*>(&v)[i]; }

template <typename T, int VEC>
__device__ __forceinline__ typename Vec<T, VEC>::type vload(const T* p)
{
    return *reinterpret_cast<const typename Vec<T, VEC>::type*>(p);
}
// Gather of one X row piece (plain loads: the gathered rows are re-read from L2 / Infinity Cache;
// non-temporal gathers measured 35 % slower on the products-shaped graph).
template <typename T, int VEC>
__device__ __forceinline__ typename Vec<T, VEC>::type gload(const T* p)
{
    return *reinterpret_cast<const typename Vec<T, VEC>::type*>(p);
}

template <typename T, int VEC>
__device__ __forceinline__ void vstore(T* p, typename Vec<T, VEC>::type v, bool nt)
{
    typedef typename Vec<T, VEC>::type V;
    if (nt)
        __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else
        *reinterpret_cast<V*>(p) = v;
}

// One link of the reference chain: acc = fma(a, x, acc) per component (fp32), or acc + a*x without
// contraction (fp64: scipy's csr_matvecs order, see srg_oracle.c).
__device__ __forceinline__ float link(float a, float x, float acc) { return __builtin_fmaf(a, x, acc); }
__device__ __forceinline__ double link(double a, double x, double acc)
{
    return __dadd_rn(acc, __dmul_rn(a, x));
}

// Epilogue arithmetic: fp64 follows numpy/scipy rounding exactly (no contraction into fma);
// fp32 leaves the compiler free (the fp32 Chebyshev path is tolerance-checked).
__device__ __forceinline__ double e_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double e_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double e_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double e_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float e_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float e_add(float a, float b) { return a + b; }
__device__ __forceinline__ float e_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float e_div(float a, float b) { return a / b; }

template <typename T, int VEC>
__device__ __forceinline__ void chain(typename Vec<T, VEC>::type& acc, T a,
                                      const typename Vec<T, VEC>::type& x)
{
    if constexpr (VEC == 1) {
        acc = link(a, x, acc);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = link(a, x[i], acc[i]);
    }
}

template <typename T, int VEC> __device__ __forceinline__ typename Vec<T, VEC>::type vzero()
{
    typename Vec<T, VEC>::type z;
    if constexpr (VEC == 1) {
        z = T(0);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) z[i] = T(0);
    }
    return z;
}

// Lane q's value in every lane (q wave-uniform): v_readlane, both halves of a 64-bit value.
template <typename T>
__device__ __forceinline__ T bcast_lane(T v, int q)
{
    if constexpr (sizeof(T) == 8) {
        const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)bits, q);
        const unsigned hi = __builtin_amdgcn_readlane((unsigned)(bits >> 32), q);
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    } else {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), q));
    }
}

// ------------------------------------------------------------------------------------------------
// the keyed bijection of the samplers (srg_sample_distinct_i64, srg_csr_sample_f32; include/srgnn_hip.h
// states the arithmetic): uint64 only and wrapping, the same on the host and on the device, so that a host
// program and a host restatement reproduce every draw bit for bit.
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the key of row (or node) r under `seed`
__host__ __device__ __forceinline__ uint64_t sample_key(uint64_t seed, uint64_t r)
{
    return mix64(seed + 0x9E3779B97F4A7C15ull * (r + 1));
}

constexpr uint64_t kWalkFailed = ~uint64_t(0);   // no draw: never below an m <= 2^62

// A four-round Feistel network over 2h bits, cycle-walked into [0, m): m <= 4^h, h the smallest h >= 1 for it.
struct FeistelWalk {
    uint64_t rk[4], mask, m;
    int h;
    __host__ __device__ __forceinline__ FeistelWalk(uint64_t key, uint64_t m_) : m(m_)
    {
        h = 1;
        while (h < 31 && (uint64_t(1) << (2 * h)) < m) ++h;   // m <= 2^62 = 4^31
        mask = (uint64_t(1) << h) - 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) rk[i] = key ^ (0xD6E8FEB86659FD93ull * (uint64_t)(i + 1));
    }
    // a bijection of [0, 4^h)
    __host__ __device__ __forceinline__ uint64_t perm(uint64_t x) const
    {
        uint64_t L = x >> h, R = x & mask;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t f = mix64(rk[i] ^ R) & mask;
            const uint64_t nr = L ^ f;
            L = R;
            R = nr;
        }
        return (L << h) | R;
    }
    // x = perm(t); while x >= m: x = perm(x).  t < m lies on a cycle of the permutation that returns to t, so
    // the walk lands below m within the cycle's length, at most 4^h applications.  The loop is bounded by
    // that: were perm not a bijection it still ends, with kWalkFailed, instead of spinning.
    __host__ __device__ __forceinline__ uint64_t walk(uint64_t t) const
    {
        const uint64_t bound = uint64_t(1) << (2 * h);
        uint64_t x = perm(t);
        for (uint64_t steps = 1; x >= m; ++steps) {
            if (steps >= bound) return kWalkFailed;
            x = perm(x);
        }
        return x;
    }
};

constexpr int kWavesPerBlock = 4;   // 256-thread workgroups
constexpr int kBlock = 64 * kWavesPerBlock;

// ------------------------------------------------------------------------------------------------
// the row-wave gather: acc (+)= A[row, :] * X[:, col .. col+VEC)
//
// The row's (column id, value) stream is read 64 entries at a time with one coalesced vector load
// (lane l holds entry jb + l), prefetched one block ahead, and broadcast to the whole wave with
// v_readlane (the lane index is wave-uniform).  Each entry's X row address is then a scalar base
// plus the lane's column offset.  U gathers are issued back to back, then consumed in CSR order.
// Entries past the end of the row repeat its last entry and are skipped by a wave-uniform predicate
// (never folded in as 0*x: that would flip -0.0 sums and turn inf/nan inputs into nan).
// FULL: every lane of the wave owns columns (d is a multiple of 64*VEC), so no lane predicates.
// ------------------------------------------------------------------------------------------------
// SPAN: the row's entries end at row_end[row] instead of indptr[row + 1] (kEpiSpan, srg_spmm_kernels.h).
template <typename T, int VEC, int U, bool FULL, typename IP, bool SPAN = false>
__device__ __forceinline__ void row_gather(typename Vec<T, VEC>::type& acc,
                                           const IP* __restrict__ indptr,
                                           const int32_t* __restrict__ indices,
                                           const T* __restrict__ vals, int row,
                                           const T* __restrict__ X, int64_t ldx, int col, bool act,
                                           const int64_t* __restrict__ row_end = nullptr)
{
    typedef typename Vec<T, VEC>::type V;
    const int lane = threadIdx.x & 63;
    const int64_t beg = indptr[row];
    int64_t end;
    if constexpr (SPAN)
        end = row_end[row];
    else
        end = indptr[row + 1];
    if (beg >= end) return;
    // entries past the row end are clamped to its last entry (always a valid id; skipped below)
    int64_t j0 = beg + lane;
    j0 = j0 < end ? j0 : end - 1;
    int c_nxt = indices[j0];
    T a_nxt = vals[j0];
    for (int64_t jb = beg; jb < end; jb += 64) {
        const int c_blk = c_nxt;
        const T a_blk = a_nxt;
        int64_t jn = jb + 64 + lane;   // prefetch the next block of the stream
        jn = jn < end ? jn : end - 1;
        c_nxt = indices[jn];
        a_nxt = vals[jn];
        const int nblk = (end - jb) < 64 ? (int)(end - jb) : 64;   // wave-uniform
        for (int s0 = 0; s0 < nblk; s0 += U) {
            V x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = __builtin_amdgcn_readlane(c_blk, s0 + u);
                const T* p = X + (int64_t)c * ldx + col;
                if (FULL || act)
                    x[u] = gload<T, VEC>(p);
                else
                    x[u] = vzero<T, VEC>();
            }
            const int n = (nblk - s0) < U ? (nblk - s0) : U;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                T a;
                if constexpr (sizeof(T) == 8) {   // v_readlane is 32-bit: broadcast both halves
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, a_blk);
                    const unsigned lo = __builtin_amdgcn_readlane((unsigned)bits, s0 + u);
                    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(bits >> 32), s0 + u);
                    a = __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
                } else {
                    a = __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a_blk), s0 + u));
                }
                if (u < n) chain<T, VEC>(acc, a, x[u]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the filtered row walk: the chain over the kept entries of indices[beg, end), in stored order
//
// Lanes across entries for the filter, lanes across columns for the chain.  The row's ids are read 64 at
// a time (lane l holds entry jb + l, -1 past the row's end), the next 64 while this block is walked.
// keep(id, j) is the lane's verdict on its entry j: a small struct with `kept` and whatever the lane
// derived from the entry.  It must reject every id outside its table's range before it or fetch uses one
// as an address.  One ballot collects the verdicts and is walked from its lowest set bit, so the chain
// keeps the stored order.  fetch(mine, q) broadcasts lane q's struct (v_readlane: q is wave-uniform) and
// issues that entry's loads into a Slot; U slots are in flight, then fold(slot) runs the chain links in
// order.  (fetch broadcasts what the lane itself loaded in keep before it issues a gather: the wait for
// that load would otherwise come to stand behind the slot's first gather.)  Slots past the last kept entry repeat it (always a valid address) and are skipped by a
// wave-uniform predicate; they, like the entries not kept, are never folded in as 0 * x: that would flip
// -0.0 sums and turn inf/nan inputs into nan.
// Cost of a long row: a row is one wave's serial chain.  A row of L entries of which M are kept costs
// L / 64 rounds of (ids -> verdicts -> ballot) plus M / U gather rounds, whatever the other waves do.
// ------------------------------------------------------------------------------------------------
template <typename Slot, int U, typename Keep, typename Fetch, typename Fold>
__device__ __forceinline__ void row_walk_kept(const int32_t* __restrict__ indices, int64_t beg, int64_t end,
                                              Keep keep, Fetch fetch, Fold fold)
{
    if (beg >= end) return;
    const int lane = threadIdx.x & 63;
    int64_t j0 = beg + lane;
    int id_nxt = j0 < end ? indices[j0] : -1;
    for (int64_t jb = beg; jb < end; jb += 64) {
        const int id = id_nxt;
        const int64_t jn = jb + 64 + lane;
        id_nxt = jn < end ? indices[jn] : -1;
        const auto mine = keep(id, jb + lane);
        unsigned long long mask = __ballot(mine.kept);
        while (mask) {
            const int live = __builtin_popcountll(mask);
            const int cnt = live < U ? live : U;   // wave-uniform
            Slot s[U];
            int q = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (mask) {
                    q = __builtin_ctzll(mask);
                    mask &= mask - 1;
                }
                s[u] = fetch(mine, q);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (u < cnt) fold(s[u]);
        }
    }
}

__device__ __forceinline__ int wave_slot(int block_base)
{
    // wave-uniform by construction; readfirstlane makes that provable to the compiler so that the
    // row's index stream goes through the scalar path.
    return __builtin_amdgcn_readfirstlane((int)((block_base + (int)blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6)));
}

// ------------------------------------------------------------------------------------------------
// rows by lanes: the layout of the streaming passes that reduce along a row (the hop attention's dot
// products, the NAFS step)
//
// S = 2^lgS lanes per row (the power of two >= the row's VEC-chunks, at most 64), R = 64 / S rows per wave
// step.  Lane c0 of row group g takes chunks c0, c0 + S, ... of row base + g, base = first, first + stride,
// ... (grid-stride over the wave steps); the S partials of a row are added in an xor butterfly, in which
// both partners add the same two values, so every lane of the row holds the same sum.  Every lane of the
// wave runs every step, for the butterfly reads its partners.  A row's bits depend on d and VEC only, never
// on the grid, the row count or the wave that got the row.
// ------------------------------------------------------------------------------------------------
struct RowLanes {
    int S, R, g, c0;
    int64_t first, stride;
    // block_dim: the kernel's blockDim.x, read there (read in here, behind a call boundary, it compiles to the
    // lookup that allows for a partial last workgroup, which HIP never launches)
    __device__ __forceinline__ RowLanes(int lgS, unsigned block_dim)
    {
        S = 1 << lgS, R = 64 >> lgS;
        const int lane = threadIdx.x & 63;
        g = lane >> lgS, c0 = lane & (S - 1);
        const int64_t wave = (int64_t)blockIdx.x * (block_dim >> 6) + (threadIdx.x >> 6);
        const int64_t waves = (int64_t)gridDim.x * (block_dim >> 6);
        first = wave * R, stride = waves * R;
    }
};

// the butterfly over S lanes, every add correctly rounded; several sums go through it side by side
template <typename... F>
__device__ __forceinline__ void butterfly_add(int S, F&... x)
{
    for (int m = S >> 1; m > 0; m >>= 1) ((x = __fadd_rn(x, __shfl_xor(x, m))), ...);
}

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
constexpr int kUnroll = 8;

// lgS of rows of cpr chunks and the RowLanes kernels' grid over n_rows rows: 256-thread workgroups, one
// wave step each wave, clipped to 256 * 64 workgroups (the kernels stride over the rest)
struct RowLanesGrid {
    int lgS;
    unsigned blocks;
};
RowLanesGrid row_lanes_grid(int cpr, int64_t n_rows)
{
    int lgS = 0;
    while (lgS < 6 && (1 << lgS) < cpr) ++lgS;
    const int64_t rows_per_block = (int64_t)(256 / 64) * (64 >> lgS);
    const int64_t blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    return {lgS, (unsigned)(blocks < 256 * 64 ? blocks : 256 * 64)};
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// May rows be read and written v elements of `elem` bytes at a time: d is whole accesses, and every row of
// every operand (base pointer, row stride in elements) starts on one.
struct Operand {
    const void* p;
    int64_t ld;
};
bool rows_aligned(int v, size_t elem, int d, std::initializer_list<Operand> ops)
{
    bool ok = d % v == 0;
    for (const Operand& o : ops) ok = ok && o.ld % v == 0 && aligned(o.p, v * elem);
    return ok;
}

int pick_vec(int d, int64_t ldx, int64_t ldy, const void* X, const void* Y, size_t elem)
{
    // widest per-lane access whose tiles line up with every row of X and Y
    if (elem == 4 && d >= 256 && rows_aligned(4, elem, d, {{X, ldx}, {Y, ldy}})) return 4;
    if (d >= 128 && rows_aligned(2, elem, d, {{X, ldx}, {Y, ldy}})) return 2;
    return 1;
}

int check_spmm_args(const void* indptr, const void* indices, const void* vals, int64_t n_rows,
                    const void* X, int64_t ldx, const void* Y, int64_t ldy, int d)
{
    if (n_rows < 0 || n_rows > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "n_rows=%lld out of range [0, 2^31-64)", (long long)n_rows);
    if (d < 0) return srg_fail(SRG_ERR_INVALID, "d=%d < 0", d);
    if (ldx < d || ldy < d)
        return srg_fail(SRG_ERR_INVALID, "leading dimensions (ldx=%lld, ldy=%lld) < d=%d",
                        (long long)ldx, (long long)ldy, d);
    if (n_rows > 0 && d > 0 && (!indptr || !Y))
        return srg_fail(SRG_ERR_INVALID, "null indptr or Y");
    (void)indices; (void)vals; (void)X;
    return SRG_OK;
}

}  // namespace

#endif  // SRG_DEVICE_H_
