// srg_spgemm.hip -- the sparse products of the wavelet model's preprocessing on MI355X (gfx950).
//
// SpectralModel.preprocess (SSRG/models/base_scalable/base_model.py:208-219) forms the product of
// the two sparsified wavelet matrices with torch_sparse.spspmm and multiplies it into the feature
// matrix with torch_sparse.spmm.  Both are CPU kernels in torch_sparse 0.6.x (spspmm_sum's CPU
// kernel; spmm = index_select, mul, scatter_add) with the arithmetic of scipy's csr_matmat:
//
//   C[i, j] = ((0 + A[i,k1]*B[k1,j]) + A[i,k2]*B[k2,j]) + ...   over row i of A in stored order,
//   every product rounded before it is added (no fma); entries that sum to 0 are dropped; the
//   columns of a row come out ascending.
//   Y[i, :] = ((0 + v1*X[c1, :]) + v2*X[c2, :]) + ...           (spmm: scatter_add in index order)
//
// SpGEMM design (Gustavson, one wave per output row, two passes: count, then fill):
//  * The row's running sums live in a dense accumulator over B's columns -- in LDS when B has at
//    most kLdsCols columns (the wavelet bases of the graphs the reference runs this on), else in a
//    per-workgroup slice of a caller-provided scratch buffer.  A bitmap marks the touched columns.
//  * A's entries are walked in stored order; the wave's 64 lanes take 64 entries of B's row at a
//    time (distinct columns, so no two lanes update one sum), and a barrier separates A's entries,
//    so every sum sees its products in A's order -- the CPU kernels' exact arithmetic.
//  * The touched words of the bitmap are scanned 64 at a time in ascending order; a wave prefix
//    sum over the lanes' nonzero counts places each kept entry, so the columns come out sorted.
//    The scan also resets what it read, leaving the accumulator zero for the workgroup's next row.
//
// The wavelet layers (wavelet/src/gwnn_layer.py) call spspmm with a learnable operand, so the product
// has an adjoint here too: k_spgemm_grad, one kernel for dL/dA and dL/dB, each output one sequential
// chain over a row of the other operand -- the forward's number of products, no fill-in.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "srg_device.h"
#include "srg_internal.h"
#include "srgnn_hip.h"

namespace {

// dense accumulator in LDS up to this many columns: 64 KiB of sums + 2 KiB of bitmap = 66 KiB, which
// fits only because gfx950 gives a workgroup up to 160 KiB of LDS (the 64 KiB of earlier CDNA parts
// would not hold it).  Cost model of the output scan below: it walks every bitmap word between the
// row's smallest and largest touched column, 64 words (2048 columns) per iteration, so a row costs
// O((hi - lo) / 2048) iterations however few entries it has -- on the scratch path (n_cols > 16384) a
// row touching columns 0 and n - 1 of an n = 2.4 M basis takes ~1.2 K iterations.  The wavelet bases
// the reference builds are dense-ish rows over N of a few thousand to ~10^5 columns (it is O(N^2) in
// memory), where the scan is a small part of the row; DESIGN.md §5.7.
constexpr int kLdsCols = 16384;
constexpr int kMaxGlobalSlots = 2048;    // workgroups of the scratch-accumulator path
constexpr int kWave = 64;

__device__ inline int64_t wave_excl_scan(int64_t v, int64_t* total)
{
    const int lane = threadIdx.x;
    int64_t x = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int64_t y = __shfl_up(x, o, kWave);
        if (lane >= o) x += y;
    }
    *total = __shfl(x, kWave - 1, kWave);
    return x - v;
}

// phase 0: cnt[r] = kept entries of C's row r;  phase 1: fills C's row r at cptr[r].
template <bool LDS>
__global__ __launch_bounds__(64) void k_spgemm(const int64_t* __restrict__ ap, const int32_t* __restrict__ ai,
                                               const float* __restrict__ av, int64_t m,
                                               const int64_t* __restrict__ bp, const int32_t* __restrict__ bi,
                                               const float* __restrict__ bv, int64_t ncols, int phase,
                                               int64_t* __restrict__ cnt, const int64_t* __restrict__ cptr,
                                               int32_t* __restrict__ ci, float* __restrict__ cv,
                                               float* __restrict__ g_acc, uint32_t* __restrict__ g_bits,
                                               int serial_b)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_lo, s_hi;
    const int lane = threadIdx.x;
    const int64_t nwords = (ncols + 31) >> 5;
    float* acc;
    uint32_t* bits;
    if (LDS) {
        acc = reinterpret_cast<float*>(smem);
        bits = reinterpret_cast<uint32_t*>(smem + 4 * ((ncols + 3) & ~int64_t(3)));
        for (int64_t i = lane; i < ncols; i += kWave) acc[i] = 0.0f;
        for (int64_t w = lane; w < nwords; w += kWave) bits[w] = 0u;
    } else {
        acc = g_acc + (int64_t)blockIdx.x * ncols;          // zero on entry (host memset), left zero
        bits = g_bits + (int64_t)blockIdx.x * nwords;
    }
    if (lane == 0) { s_lo = INT_MAX; s_hi = -1; }
    __syncthreads();
    for (int64_t r = blockIdx.x; r < m; r += gridDim.x) {
        const int64_t e1 = ap[r + 1];
        for (int64_t e = ap[r]; e < e1; ++e) {              // A's entries in stored order
            const int32_t k = ai[e];
            const float a = av[e];
            const int64_t b0 = bp[k], b1 = bp[k + 1];
            for (int64_t q = b0 + (serial_b ? 0 : lane); q < b1; q += (serial_b ? 1 : kWave)) {
                if (serial_b && lane != 0) break;           // repeated columns in a B row: one lane
                const int32_t j = bi[q];
                acc[j] = __fadd_rn(acc[j], __fmul_rn(a, bv[q]));
                const uint32_t bit = 1u << (j & 31);
                const uint32_t old = atomicOr(&bits[j >> 5], bit);
                if (!(old & bit)) {
                    atomicMin(&s_lo, j >> 5);
                    atomicMax(&s_hi, j >> 5);
                }
            }
            __syncthreads();                                // every sum sees its products in A's order
        }
        const int lo = s_lo, hi = s_hi;
        int64_t run = 0;
        const int64_t base = phase ? cptr[r] : 0;
        if (hi >= 0) {
            for (int64_t w0 = lo; w0 <= hi; w0 += kWave) {
                const int64_t w = w0 + lane;
                const uint32_t word = (w <= hi) ? bits[w] : 0u;
                uint32_t keep = 0;
                for (uint32_t t = word; t; t &= t - 1) {
                    const int b = __ffs(t) - 1;
                    if (acc[w * 32 + b] != 0.0f) keep |= 1u << b;
                }
                int64_t total = 0;
                int64_t pos = base + run + wave_excl_scan(__popc(keep), &total);
                for (uint32_t t = word; t; t &= t - 1) {
                    const int b = __ffs(t) - 1;
                    const int64_t j = w * 32 + b;
                    if (phase && ((keep >> b) & 1u)) {
                        ci[pos] = (int32_t)j;
                        cv[pos] = acc[j];
                        ++pos;
                    }
                    acc[j] = 0.0f;
                }
                if (word) bits[w] = 0u;
                run += total;
            }
        }
        if (!phase && lane == 0) cnt[r] = run;
        __syncthreads();
        if (lane == 0) { s_lo = INT_MAX; s_hi = -1; }
        __syncthreads();
    }
}

// The adjoint of C = A * B for either operand (srgnn_hip.h): for every entry e of a pattern row r,
//   out[e] = ((0 + D[r, j1] * R[k, j1]) + D[r, j2] * R[k, j2]) + ...   over row k = p_idx[e] of R in
// stored order, every product rounded before it is added; D[r, j] is +0 where row r of D has no entry.
// One workgroup per pattern row: row r of D is expanded into the dense accumulator the forward uses
// (LDS up to kLdsCols columns, else the workgroup's slice of the scratch; no bitmap: the row's own
// entries say what to reset), then each lane runs the whole chain of one pattern entry, so an output's
// order of additions never depends on the schedule, and no two lanes write one word.
constexpr int kGradThreads = 256;

template <bool LDS>
__global__ __launch_bounds__(kGradThreads) void k_spgemm_grad(
    const int64_t* __restrict__ pp, const int32_t* __restrict__ pi, int64_t m, const int64_t* __restrict__ dp,
    const int32_t* __restrict__ di, const float* __restrict__ dv, const int64_t* __restrict__ rp,
    const int32_t* __restrict__ ri, const float* __restrict__ rv, int64_t ncols, float* __restrict__ out,
    float* g_acc)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    float* acc;
    if (LDS) {
        acc = reinterpret_cast<float*>(smem);
        for (int64_t i = tid; i < ncols; i += kGradThreads) acc[i] = 0.0f;
    } else {
        acc = g_acc + (int64_t)blockIdx.x * ncols;          // zero on entry (host memset), left zero
    }
    __syncthreads();
    for (int64_t r = blockIdx.x; r < m; r += gridDim.x) {
        const int64_t d0 = dp[r], d1 = dp[r + 1];
        for (int64_t q = d0 + tid; q < d1; q += kGradThreads) acc[di[q]] = dv[q];
        __syncthreads();
        const int64_t e1 = pp[r + 1];
        for (int64_t e = pp[r] + tid; e < e1; e += kGradThreads) {
            const int32_t k = pi[e];
            const int64_t q1 = rp[k + 1];
            float s = 0.0f;
            for (int64_t q = rp[k]; q < q1; ++q) s = __fadd_rn(s, __fmul_rn(acc[ri[q]], rv[q]));
            out[e] = s;
        }
        __syncthreads();
        for (int64_t q = d0 + tid; q < d1; q += kGradThreads) acc[di[q]] = 0.0f;
        __syncthreads();
    }
}

// Y[r, :] = sum over row r's entries, in stored order, of (v * X[c, :]) -- each product rounded,
// then added, from +0: torch_sparse.spmm's index_select / mul / scatter_add arithmetic.
__global__ __launch_bounds__(256) void k_spmm_muladd(const int64_t* __restrict__ ip, const int32_t* __restrict__ ix,
                                                     const float* __restrict__ vv, int64_t n_rows,
                                                     const float* __restrict__ X, int64_t ldx,
                                                     float* __restrict__ Y, int64_t ldy, int d)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int64_t e0 = ip[r], e1 = ip[r + 1];
    for (int c0 = 0; c0 < d; c0 += kWave) {
        const int c = c0 + lane;
        float s = 0.0f;
        if (c < d)
            for (int64_t e = e0; e < e1; ++e) s = __fadd_rn(s, __fmul_rn(vv[e], X[(int64_t)ix[e] * ldx + c]));
        if (c < d) Y[r * ldy + c] = s;
    }
}

// The sampled dense-dense product (srgnn_hip.h: srg_sddmm_f32; spmm's value gradient): for entry
// e = (r, c), out[e] = ((+0 + G[r,0]*X[c,0]) + G[r,1]*X[c,1]) + ..., every product rounded before it is
// added, columns ascending.  One lane per entry -- a chain cannot be split across lanes without changing
// its order -- and one wave (= one workgroup) per 64 consecutive CSR entries, each lane finding its row by
// an upper-bound search over indptr, so long rows and short rows load the lanes alike.
//  * X's 64 gathered rows are staged kSdTile columns at a time into the wave's LDS tile with coalesced
//    loads (VEC: 16 bytes per lane, 8 lanes per row, 8 rows per instruction; otherwise 4 bytes per lane,
//    32 lanes per row), kSdLd = kSdTile + 4 dwords per row: lane l then reads its own row as 16-byte
//    pieces at dword l * 36 + j, 16-byte slot (9 l + j / 4) mod 16 -- distinct over each of
//    ds_read_b128's 16-lane groups (their lane ids are distinct mod 16 and 9 is odd): no bank conflict.
//  * The next tile's loads are issued into registers before the current tile's chain runs and stored to
//    LDS after it.
//  * G is read by each lane from its own row; lanes of one row read one address (one request).
//  * VEC needs 16-byte aligned bases and strides that are multiples of 4; it stages d & ~3 columns and
//    takes the last d & 3 columns straight from memory.  Either path runs the same chain: same bits.
typedef float f32x4 __attribute__((ext_vector_type(4)));    // stays in registers as an array element
constexpr int kSdTile = 32;
constexpr int kSdLd = kSdTile + 4;

template <bool VEC>
__global__ __launch_bounds__(kWave) void k_sddmm(const int64_t* __restrict__ ip, const int32_t* __restrict__ ix,
                                                 int64_t n_rows, int64_t e0, int64_t nnz,
                                                 const float* __restrict__ G, int64_t ldg,
                                                 const float* __restrict__ X, int64_t ldx, int d,
                                                 const int64_t* __restrict__ perm, float* __restrict__ out)
{
    __shared__ __align__(16) float tile[kWave * kSdLd];
    constexpr int kRegs = VEC ? kSdTile / 4 : kSdTile;      // staging registers: 8 float4 or 32 floats
    const int lane = threadIdx.x;
    const int64_t e = e0 + (int64_t)blockIdx.x * kWave + lane;
    const bool live = e < nnz;
    int64_t r = 0;
    int32_t c = 0;
    if (live && d > 0) {
        int64_t lo = 1, hi = n_rows;                        // the first i in [1, n_rows] with ip[i] > e
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ip[mid] > e) hi = mid; else lo = mid + 1;
        }
        r = lo - 1;
        c = ix[e];
    }
    r = live ? r : __shfl(r, 0, kWave);                     // lane 0 is live: idle lanes redo its entry
    c = live ? c : __shfl(c, 0, kWave);
    const float* g = G + r * ldg;
    const int dt = VEC ? (d & ~3) : d;                      // columns that go through the LDS tile
    using Piece = std::conditional_t<VEC, f32x4, float>;
    Piece v[kRegs];

    // the 64 rows' columns [c0, c0 + w) into the staging registers: coalesced along each row
    auto fetch = [&](int c0, int w) {
#pragma unroll
        for (int i = 0; i < kRegs; ++i) {
            const int row = VEC ? i * 8 + (lane >> 3) : i * 2 + (lane >> 5);
            const int col = VEC ? (lane & 7) * 4 : lane & 31;
            const int32_t cr = __shfl(c, row, kWave);
            // past the tile's width a lane loads its row's first piece again (every register is written)
            v[i] = *reinterpret_cast<const Piece*>(X + (int64_t)cr * ldx + c0 + (col < w ? col : 0));
        }
    };
    auto stage = [&](int w) {
#pragma unroll
        for (int i = 0; i < kRegs; ++i) {
            const int row = VEC ? i * 8 + (lane >> 3) : i * 2 + (lane >> 5);
            const int col = VEC ? (lane & 7) * 4 : lane & 31;
            if (col < w) *reinterpret_cast<Piece*>(&tile[row * kSdLd + col]) = v[i];
        }
    };

    float s = 0.0f;
    if (dt > 0) fetch(0, dt < kSdTile ? dt : kSdTile);
    for (int c0 = 0; c0 < dt; c0 += kSdTile) {
        const int w = dt - c0 < kSdTile ? dt - c0 : kSdTile;
        __syncthreads();                                    // the previous tile has been read
        stage(w);
        __syncthreads();
        const int c1 = c0 + kSdTile;
        if (c1 < dt) fetch(c1, dt - c1 < kSdTile ? dt - c1 : kSdTile);
        const float* mine = &tile[lane * kSdLd];
        for (int j = 0; j < w; j += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(mine + j);
            if (VEC) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(g + c0 + j);
                s = __fadd_rn(s, __fmul_rn(a.x, x.x));
                s = __fadd_rn(s, __fmul_rn(a.y, x.y));
                s = __fadd_rn(s, __fmul_rn(a.z, x.z));
                s = __fadd_rn(s, __fmul_rn(a.w, x.w));
            } else {
                const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j + k < w) s = __fadd_rn(s, __fmul_rn(g[c0 + j + k], xs[k]));
            }
        }
    }
    const float* x = X + (int64_t)c * ldx;
    for (int j = dt; j < d; ++j) s = __fadd_rn(s, __fmul_rn(g[j], x[j]));     // VEC: the last d & 3 columns
    if (live) out[perm ? perm[e] : e] = s;
}

}  // namespace

extern "C" {

int srg_spgemm_scratch_bytes(int64_t m, int64_t n_cols, int64_t* bytes)
{
    if (!bytes || m < 0 || n_cols < 0) return srg_fail(SRG_ERR_INVALID, "bad arguments");
    if (n_cols <= kLdsCols) {
        *bytes = 0;
        return srg_ok();
    }
    const int64_t per = 4 * n_cols + 4 * ((n_cols + 31) >> 5);
    const int64_t slots = m < kMaxGlobalSlots ? (m > 0 ? m : 1) : kMaxGlobalSlots;
    *bytes = slots * per;
    return srg_ok();
}

int srg_spgemm_f32(int phase, const int64_t* a_ptr, const int32_t* a_idx, const float* a_val, int64_t m,
                   const int64_t* b_ptr, const int32_t* b_idx, const float* b_val, int64_t n_cols,
                   int64_t* c_cnt, const int64_t* c_ptr, int32_t* c_idx, float* c_val, void* scratch,
                   int64_t scratch_bytes, uint32_t flags, void* stream)
{
    if (phase != 0 && phase != 1) return srg_fail(SRG_ERR_INVALID, "phase %d", phase);
    if (m < 0 || n_cols < 0 || n_cols > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "bad shape m=%lld n=%lld",
                                                                   (long long)m, (long long)n_cols);
    if (m == 0) return srg_ok();
    if (!a_ptr || !b_ptr || (phase == 0 && !c_cnt) || (phase == 1 && !c_ptr))
        return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int serial = (flags & SRG_SPGEMM_SERIAL_B) ? 1 : 0;
    if (n_cols <= kLdsCols) {
        const size_t lds = 4 * (size_t)((n_cols + 3) & ~int64_t(3)) + 4 * (size_t)((n_cols + 31) >> 5);
        if (lds > 48 * 1024)
            SRG_HIP_CHECK(hipFuncSetAttribute((const void*)k_spgemm<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
        const int64_t grid = m < 16384 ? m : 16384;
        hipLaunchKernelGGL(k_spgemm<true>, dim3((unsigned)grid), dim3(kWave), lds, s, a_ptr, a_idx, a_val, m,
                           b_ptr, b_idx, b_val, n_cols, phase, c_cnt, c_ptr, c_idx, c_val, (float*)nullptr,
                           (uint32_t*)nullptr, serial);
    } else {
        const int64_t per = 4 * n_cols + 4 * ((n_cols + 31) >> 5);
        const int64_t slots = scratch ? scratch_bytes / per : 0;
        if (slots < 1) return srg_fail(SRG_ERR_INVALID, "scratch of %lld bytes < one accumulator (%lld)",
                                       (long long)scratch_bytes, (long long)per);
        const int64_t grid = slots < m ? slots : m;
        float* acc = static_cast<float*>(scratch);
        uint32_t* bits = reinterpret_cast<uint32_t*>(acc + grid * n_cols);
        SRG_HIP_CHECK(hipMemsetAsync(scratch, 0, (size_t)(grid * per), s));
        hipLaunchKernelGGL(k_spgemm<false>, dim3((unsigned)grid), dim3(kWave), 0, s, a_ptr, a_idx, a_val, m,
                           b_ptr, b_idx, b_val, n_cols, phase, c_cnt, c_ptr, c_idx, c_val, acc, bits, serial);
    }
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_spgemm_grad_f32(const int64_t* p_ptr, const int32_t* p_idx, int64_t m, const int64_t* d_ptr,
                        const int32_t* d_idx, const float* d_val, const int64_t* r_ptr, const int32_t* r_idx,
                        const float* r_val, int64_t n_cols, float* out, void* scratch, int64_t scratch_bytes,
                        void* stream)
{
    if (m < 0 || n_cols < 0 || n_cols > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "bad shape m=%lld n=%lld",
                                                                   (long long)m, (long long)n_cols);
    if (m == 0) return srg_ok();
    if (!p_ptr || !d_ptr || !r_ptr) return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_cols <= kLdsCols) {
        const size_t lds = 4 * (size_t)((n_cols + 3) & ~int64_t(3));
        if (lds > 48 * 1024)
            SRG_HIP_CHECK(hipFuncSetAttribute((const void*)k_spgemm_grad<true>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const int64_t grid = m < kMaxGlobalSlots ? m : kMaxGlobalSlots;
        hipLaunchKernelGGL(k_spgemm_grad<true>, dim3((unsigned)grid), dim3(kGradThreads), lds, s, p_ptr, p_idx, m,
                           d_ptr, d_idx, d_val, r_ptr, r_idx, r_val, n_cols, out, (float*)nullptr);
    } else {
        const int64_t per = 4 * n_cols;
        int64_t slots = scratch ? scratch_bytes / per : 0;
        if (slots < 1) return srg_fail(SRG_ERR_INVALID, "scratch of %lld bytes < one accumulator (%lld)",
                                       (long long)scratch_bytes, (long long)per);
        if (slots > kMaxGlobalSlots) slots = kMaxGlobalSlots;
        const int64_t grid = slots < m ? slots : m;
        SRG_HIP_CHECK(hipMemsetAsync(scratch, 0, (size_t)(grid * per), s));
        hipLaunchKernelGGL(k_spgemm_grad<false>, dim3((unsigned)grid), dim3(kGradThreads), 0, s, p_ptr, p_idx, m,
                           d_ptr, d_idx, d_val, r_ptr, r_idx, r_val, n_cols, out, static_cast<float*>(scratch));
    }
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_spmm_muladd_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                        const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, void* stream)
{
    if (n_rows < 0 || d < 0 || ldx < d || ldy < d) return srg_fail(SRG_ERR_INVALID, "bad shape");
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!indptr || !Y) return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    const int rc = launch_chunks_capped((n_rows + 3) / 4, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        const int64_t r0 = b0 * 4;
        hipLaunchKernelGGL(k_spmm_muladd, dim3(nb), dim3(256), 0, static_cast<hipStream_t>(stream),
                           indptr + r0, indices, values, n_rows - r0, X, ldx, Y + r0 * ldy, ldy, d);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_sddmm_f32(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const float* G,
                  int64_t ldg, const float* X, int64_t ldx, int32_t d, const int64_t* perm, float* out,
                  void* stream)
{
    if (n_rows < 0 || nnz < 0 || d < 0)
        return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld nnz=%lld d=%d", (long long)n_rows, (long long)nnz,
                        (int)d);
    if (ldg < d || ldx < d)
        return srg_fail(SRG_ERR_INVALID, "row stride ldg=%lld or ldx=%lld < d=%d", (long long)ldg, (long long)ldx,
                        (int)d);
    if (n_rows == 0 || nnz == 0) return srg_ok();
    if (!out || (d > 0 && (!indptr || !indices || !G || !X))) return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    // (whatever d is: the kernel takes a row's last d % 4 columns by the element)
    const bool vec = rows_aligned(4, sizeof(float), 0, {{G, ldg}, {X, ldx}});
    const int rc = launch_chunks_capped((nnz + kWave - 1) / kWave, kMaxLaunchWaveBlocks, [&](int64_t b0, unsigned nb) {
        if (vec)
            hipLaunchKernelGGL(k_sddmm<true>, dim3(nb), dim3(kWave), 0, static_cast<hipStream_t>(stream),
                               indptr, indices, n_rows, b0 * kWave, nnz, G, ldg, X, ldx, d, perm, out);
        else
            hipLaunchKernelGGL(k_sddmm<false>, dim3(nb), dim3(kWave), 0, static_cast<hipStream_t>(stream),
                               indptr, indices, n_rows, b0 * kWave, nnz, G, ldg, X, ldx, d, perm, out);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
