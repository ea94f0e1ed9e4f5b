// srg_cheby.hip -- the Chebyshev (wavelet) steps: the fp32 and fp64 row kernels with the fused epilogue,
// the fp64 hub workgroups and the blocked fp64 step over a plan, the split fp32 epilogue, and the SpMM
// kernels of srg_spmm_kernels.h with the fused Chebyshev epilogue (srg_spmm_cheby_f32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_plan_internal.h"
#include "srg_spmm_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Chebyshev step with fused epilogue (wavelet basis)
// ------------------------------------------------------------------------------------------------
// The fused step's epilogue at VEC consecutive elements of row-offset `off`: acc = (A Tc) there becomes
// T_{k+1}, every scale's output updated -- k_cheby_epilogue's modes and operations:
//   INIT:       Tn = (acc - a2 Tc) / a1;  R_s = (c0_s/2) Tc + c1_s Tn
//   INIT_T:     Tn = (acc - a2 Tc) / a1   (R formed by the first step)
//   STEP_FIRST: Tn = acc - To (To = T0, Tc = T1);  R_s = ((c0_s/2) T0 + c1_s T1) + c2_s Tn
//   STEP:       Tn = acc - To;  R_s += ck_s Tn
// with SRG_CHEBY_NO_T leaving Tn unstored (the last order).  The lean sequence INIT_T, STEP_FIRST, ...,
// STEP | NO_T forms every R with the same operations in the same order as INIT, STEP, ..., STEP: the
// same bits with four panel passes less per order-3 filter.
template <typename T, int VEC>
__device__ __forceinline__ void cheby_epi_at(int mode, const typename Vec<T, VEC>::type& acc, const T* __restrict__ Tc,
                                             const T* __restrict__ To, T* __restrict__ Tn, T* __restrict__ R,
                                             int64_t off, int64_t r_stride, T a1, T a2, const ChebyCoef<T>& cf,
                                             int n_scales)
{
    typedef typename Vec<T, VEC>::type V;
    const int m = mode & 0xf;
    V tn;
    if (m == SRG_CHEBY_INIT || m == SRG_CHEBY_INIT_T) {
        const V tc = vload<T, VEC>(Tc + off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) elem(tn, i) = e_div(e_sub(elem(acc, i), e_mul(a2, elem(tc, i))), a1);
        if (m == SRG_CHEBY_INIT)
            for (int s = 0; s < n_scales; ++s) {
                V r;
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    elem(r, i) = e_add(e_mul(cf.prev[s], elem(tc, i)), e_mul(cf.cur[s], elem(tn, i)));
                vstore<T, VEC>(R + s * r_stride + off, r, false);
            }
    } else if (m == SRG_CHEBY_STEP_FIRST) {
        const V t0 = vload<T, VEC>(To + off), t1 = vload<T, VEC>(Tc + off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) elem(tn, i) = e_sub(elem(acc, i), elem(t0, i));
        for (int s = 0; s < n_scales; ++s) {
            V r;
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                elem(r, i) = e_add(e_add(e_mul(cf.prev[s], elem(t0, i)), e_mul(cf.mid[s], elem(t1, i))),
                                   e_mul(cf.cur[s], elem(tn, i)));
            vstore<T, VEC>(R + s * r_stride + off, r, false);
        }
    } else {
        const V to = vload<T, VEC>(To + off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) elem(tn, i) = e_sub(elem(acc, i), elem(to, i));
        for (int s = 0; s < n_scales; ++s) {
            T* rp = R + s * r_stride + off;
            V r = vload<T, VEC>(rp);
#pragma unroll
            for (int i = 0; i < VEC; ++i) elem(r, i) = e_add(elem(r, i), e_mul(cf.cur[s], elem(tn, i)));
            vstore<T, VEC>(rp, r, false);
        }
    }
    if (!(mode & SRG_CHEBY_NO_T)) vstore<T, VEC>(Tn + off, tn, false);
}

template <typename T, int VEC, int U>
__global__ void __launch_bounds__(kBlock)
k_cheby(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
        const T* __restrict__ vals, const int32_t* __restrict__ order, int n_rows,
        const T* __restrict__ Tc, const T* __restrict__ To, T* __restrict__ Tn, int64_t ld, int d,
        int mode, T a1, T a2, ChebyCoef<T> cf, int n_scales, T* __restrict__ R, int64_t r_stride,
        int block_base)
{
    typedef typename Vec<T, VEC>::type V;
    const int w = wave_slot(block_base);
    if (w >= n_rows) return;
    const int row = order ? order[w] : w;
    const int lane = threadIdx.x & 63;
    const int64_t roff = (int64_t)row * ld;
    for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
        const int col = c0 + lane * VEC;
        const bool act = col < d;
        V acc = vzero<T, VEC>();
        row_gather<T, VEC, U, false, int64_t>(acc, indptr, indices, vals, row, Tc, ld, col, act);
        if (!act) continue;
        cheby_epi_at<T, VEC>(mode, acc, Tc, To, Tn, R, roff + col, r_stride, a1, a2, cf, n_scales);
    }
}

// ------------------------------------------------------------------------------------------------
// fp64 Chebyshev step, hub rows: one workgroup per (hub row, 16-column slice)
//
// A row wave keeps U gathers of its row in flight, so a row of degree D costs ~D/U load latencies:
// in fp64 the products top row (155,868 entries) is one wave's chain beside the whole step.  As in
// k_spmm_hub, kHub64Producers waves gather windows of W entries into LDS (two tiles, one
// barrier per window; each window's gathers are issued two windows ahead) and one consumer wave
// runs the slice's 16 column chains out of LDS: link k of column c is acc = acc + a_k * x_k[c], the
// product and the sum rounded separately (scipy's csr_matvecs order, as row_gather), then k_cheby's
// epilogue for the row's 16 columns -- the same operations, so the same bits.
//   * producer lane (g, q) gathers the 16-byte chunk q (columns 2q, 2q + 1 of the slice) of entry g
//     of a group of 8: one dwordx4 instruction brings 8 entries' 128-byte slices;
//   * the tile is column-major, [16 columns][W + 4]: the consumer's lane c reads links k, k + 1
//     of its column with one ds_read_b128, their values with one broadcast ds_read_b128;
//   * the consumer keeps three 8-link register sets in flight (reads issued ~16 links ahead).
// ------------------------------------------------------------------------------------------------
constexpr int kHub64Cols = 16;
constexpr int kHub64Producers = 8;
constexpr int kHub64Threads = 64 * (kHub64Producers + 1);
constexpr int kHub64Slack = 32;                               // the ring's reads past the last window
// W entries per window: 512 (141 KB of LDS, one workgroup per CU) for a few hub rows beside the row waves,
// 256 (72 KB, two per CU) once a launch has more hub workgroups than CUs (as k_spmm_hub's kHubWideW)
template <int W>
struct Hub64Geom {
    static constexpr int UW = W / (kHub64Producers * 8);      // gathers per producer lane per window
    static constexpr int LD = W + 4;                          // doubles per tile column (16-byte rows)
    static constexpr int TILE = kHub64Cols * LD;
    static constexpr size_t LDS_BYTES = (size_t)(2 * TILE + 2 * W + kHub64Slack) * sizeof(double);
    static_assert(LDS_BYTES <= 160 * 1024, "k_cheby_hub64's LDS");
};

template <int W>
__global__ void __launch_bounds__(kHub64Threads)
k_cheby_hub64(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
              const double* __restrict__ vals, const int32_t* __restrict__ hub_rows, int n_slices,
              const double* __restrict__ Tc, const double* __restrict__ To, double* __restrict__ Tn, int64_t ld,
              int d, int mode, double a1, double a2, ChebyCoef<double> cf, int n_scales, double* __restrict__ R,
              int64_t r_stride)
{
    typedef typename Vec<double, 2>::type V2;
    constexpr int UW = Hub64Geom<W>::UW, LD = Hub64Geom<W>::LD, TILE = Hub64Geom<W>::TILE;
    extern __shared__ __attribute__((aligned(16))) double h64_lds[];
    double* aval_base = h64_lds + 2 * TILE;
    const int row = hub_rows[blockIdx.x / n_slices];
    const int slice = blockIdx.x % n_slices;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t beg = indptr[row];
    const int64_t end = indptr[row + 1];
    const int n_win = (int)((end - beg + W - 1) / W);

    if (wave == 0) {   // ---------------- consumer: 16 column chains ----------------
        const int c = lane & (kHub64Cols - 1);
        const int col = slice * kHub64Cols + c;
        const bool act = lane < kHub64Cols && col < d;
        double acc = 0.0;
        for (int h = 0; h < n_win; ++h) {
            __syncthreads();                      // window h is in tile h & 1
            if (lane < kHub64Cols) {
                const double* tcol = h64_lds + (h & 1) * TILE + c * LD;
                const double* av = aval_base + (h & 1) * W;
                const int64_t sb = beg + (int64_t)h * W;
                const int nb = (end - sb) < W ? (int)(end - sb) : W;
                const int nc = nb / 8;            // full 8-link sets
                V2 tA[4], aA[4], tB[4], aB[4], tC[4], aC[4];
                // set k: links 8k .. 8k + 7 (reads past nb stay inside the LDS block: kHub64Slack)
                auto ld = [&](int k, V2 (&t)[4], V2 (&a)[4]) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        t[i] = *reinterpret_cast<const V2*>(tcol + 8 * k + 2 * i);
                        a[i] = *reinterpret_cast<const V2*>(av + 8 * k + 2 * i);   // broadcast
                    }
                };
                auto run = [&](const V2 (&t)[4], const V2 (&a)[4]) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc = link(a[i][0], t[i][0], acc);
                        acc = link(a[i][1], t[i][1], acc);
                    }
                };
                ld(0, tA, aA);
                __builtin_amdgcn_sched_barrier(0);
                ld(1, tB, aB);
                __builtin_amdgcn_sched_barrier(0);
                int k = 0;
                for (; k + 3 <= nc; k += 3) {
                    ld(k + 2, tC, aC);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tA, aA);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(k + 3, tA, aA);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tB, aB);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(k + 4, tB, aB);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tC, aC);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // the loop leaves at most two full sets, k and k + 1 (already read), then < 8 links
                if (k < nc) run(tA, aA);
                if (k + 1 < nc) run(tB, aB);
                for (int q = nc * 8; q < nb; ++q) acc = link(av[q], tcol[q], acc);
            }
        }
        if (act) cheby_epi_at<double, 1>(mode, acc, Tc, To, Tn, R, (int64_t)row * ld + col, r_stride, a1, a2, cf, n_scales);
        return;
    }

    // ---------------- producers ----------------
    const int p = wave - 1;
    const int g = lane >> 3;          // entry within a gather's group of 8
    const int qq = lane & 7;          // 16-byte chunk: columns 2qq, 2qq + 1 of the slice
    const int qcol = slice * kHub64Cols + qq * 2;
    const bool gact = qcol < d;       // d even (the launch's condition): both columns or neither
    V2 x0[UW], x1[UW];
    double a0[UW], a1v[UW];
    int cn[UW];
    double an[UW];
    auto load_ids = [&](int w) {
        const int64_t sb = beg + (int64_t)w * W;
#pragma unroll
        for (int b = 0; b < UW; ++b) {
            int64_t jj = sb + (p * UW + b) * 8 + g;
            jj = jj < end ? jj : end - 1;
            cn[b] = indices[jj];
            an[b] = vals[jj];
        }
    };
    auto gather = [&](V2 (&x)[UW], double (&a)[UW]) {
#pragma unroll
        for (int b = 0; b < UW; ++b) {
            x[b] = gact ? gload<double, 2>(Tc + (int64_t)cn[b] * ld + qcol) : vzero<double, 2>();
            a[b] = an[b];
        }
    };
    auto put = [&](int w, const V2 (&x)[UW], const double (&a)[UW]) {
        double* tile = h64_lds + (w & 1) * TILE;
        double* av = aval_base + (w & 1) * W;
#pragma unroll
        for (int b = 0; b < UW; ++b) {
            const int nl = (p * UW + b) * 8 + g;   // entry within the window
            tile[(2 * qq) * LD + nl] = x[b][0];
            tile[(2 * qq + 1) * LD + nl] = x[b][1];
            if (qq == 0) av[nl] = a[b];
        }
    };
    // an empty row (any schedule may name one a hub row): the consumer passes no barrier, so the
    // producers, with nothing to gather, leave before their first
    if (n_win == 0) return;
    // prologue: windows 0 and 1 in flight, window 0 published, window 2 in flight
    if (n_win > 0) {
        load_ids(0);
        __builtin_amdgcn_sched_barrier(0);
        gather(x0, a0);
        if (n_win > 1) { load_ids(1); gather(x1, a1v); }
        if (n_win > 2) load_ids(2);
        put(0, x0, a0);
        if (n_win > 2) { gather(x0, a0); if (n_win > 3) load_ids(3); }
    }
    __syncthreads();                              // window 0 published
    for (int h = 0; h + 1 < n_win; h += 2) {
        put(h + 1, x1, a1v);
        if (h + 3 < n_win) { gather(x1, a1v); if (h + 4 < n_win) load_ids(h + 4); }
        __syncthreads();
        if (h + 2 >= n_win) break;
        put(h + 2, x0, a0);
        if (h + 4 < n_win) { gather(x0, a0); if (h + 5 < n_win) load_ids(h + 5); }
        __syncthreads();
    }
    // barrier count (n_win >= 1): 1 (prologue) + (n_win - 1) in the loop == the consumer's n_win
}

// the hub workgroups of n_items (row, slice) pairs on `s` (the window size by the launch's width)
void launch_hub64(int64_t n_items, hipStream_t s, const int64_t* indptr, const int32_t* indices, const double* vals,
                  const int32_t* rows, int n_slices, const double* Tc, const double* To, double* Tn, int64_t ld, int d,
                  int mode, double a1, double a2, const ChebyCoef<double>& cf, int n_scales, double* R, int64_t r_stride)
{
    if (n_items > kHubWideLaunch)
        hipLaunchKernelGGL(k_cheby_hub64<256>, dim3((unsigned)n_items), dim3(kHub64Threads), Hub64Geom<256>::LDS_BYTES, s,
                           indptr, indices, vals, rows, n_slices, Tc, To, Tn, ld, d, mode, a1, a2, cf, n_scales, R, r_stride);
    else
        hipLaunchKernelGGL(k_cheby_hub64<512>, dim3((unsigned)n_items), dim3(kHub64Threads), Hub64Geom<512>::LDS_BYTES, s,
                           indptr, indices, vals, rows, n_slices, Tc, To, Tn, ld, d, mode, a1, a2, cf, n_scales, R, r_stride);
}

// their dynamic-LDS limits on the current device, raised by the first fork of a step there (HubLds)
int hub64_attrs()
{
    SRG_HIP_CHECK(hipFuncSetAttribute((const void*)k_cheby_hub64<512>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)Hub64Geom<512>::LDS_BYTES));
    SRG_HIP_CHECK(hipFuncSetAttribute((const void*)k_cheby_hub64<256>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)Hub64Geom<256>::LDS_BYTES));
    return SRG_OK;
}
HubLds g_hub64_lds = {hub64_attrs, {}};

// ------------------------------------------------------------------------------------------------
// fp64 Chebyshev step over a column-blocked plan (srg_plan_cheby_step_f64): one launch per block of
// the plan, the row waves of k_cheby over the launch's schedule, row w's entries the span
// [slot_beg[w], slot_end[w]) of the caller's arrays.  A row's chain starts at 0 in block 0 (FIRST),
// continues from the fp64 partial sum the block before stored in Tn (exact: the stored value is the
// chain's value), and ends -- k_cheby's epilogue, the same operations -- in block 0 for the whole rows
// and in the last block for the cut rows (LAST).  So bitwise srg_cheby_step_f64, with each launch
// gathering from one column block of Tc (1/B of the panel: the L2 / Infinity Cache keep it).
// ------------------------------------------------------------------------------------------------
template <int VEC, int U, bool FIRST, bool LAST>
__global__ void __launch_bounds__(kBlock)
k_cheby_blk64(const int64_t* __restrict__ slot_beg, const int64_t* __restrict__ slot_end,
              const int32_t* __restrict__ order, int n_rows, const int32_t* __restrict__ indices,
              const double* __restrict__ vals, const double* __restrict__ Tc, const double* __restrict__ To,
              double* __restrict__ Tn, int64_t ld, int d, int mode, double a1, double a2, ChebyCoef<double> cf,
              int n_scales, double* __restrict__ R, int64_t r_stride, int block_base)
{
    typedef typename Vec<double, VEC>::type V;
    const int w = wave_slot(block_base);
    if (w >= n_rows) return;
    if constexpr (!FIRST && !LAST) {
        if (slot_beg[w] >= slot_end[w]) return;   // nothing in this block: the partial sum stays
    }
    const int row = order[w];
    const int lane = threadIdx.x & 63;
    const int64_t roff = (int64_t)row * ld;
    for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
        const int col = c0 + lane * VEC;
        const bool act = col < d;
        V acc = vzero<double, VEC>();
        if constexpr (!FIRST) {
            if (act) acc = vload<double, VEC>(Tn + roff + col);
        }
        row_gather<double, VEC, U, false, int64_t, true>(acc, slot_beg, indices, vals, w, Tc, ld, col, act, slot_end);
        if (!act) continue;
        if constexpr (!LAST)
            vstore<double, VEC>(Tn + roff + col, acc, false);
        else
            cheby_epi_at<double, VEC>(mode, acc, Tc, To, Tn, R, roff + col, r_stride, a1, a2, cf, n_scales);
    }
}

// Chebyshev epilogue after a load-balanced SpMM (fp32, large graphs): Tn holds acc = A*Tc (the
// same fma chain k_cheby forms, so results are bit-identical to the fused kernel) and becomes
// Tn; every panel has its own leading dimension, so column blocks of S and R need no copies.
// INIT_T / STEP_FIRST defer the INIT's scale outputs to the first step, which forms them from T0,
// T1 and T2 with the same operations in the same order (R = ((c0/2) T0 + c1 T1) + c2 T2), and
// SRG_CHEBY_NO_T leaves T_{k+1} unstored in the last order: 4 panel passes less per order-3 block.
__global__ void __launch_bounds__(256)
k_cheby_epilogue(float* __restrict__ Tn, int64_t ldn, const float* __restrict__ Tc, int64_t ldc,
                 const float* __restrict__ To, int64_t ldo, int64_t n_rows, int d, int mode, float a1,
                 float a2, ChebyCoef<float> cf, int n_scales, float* __restrict__ R, int64_t ldr,
                 int64_t r_stride)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool store_t = !(mode & SRG_CHEBY_NO_T);
    const int m = mode & 0xf;
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        float* tn = Tn + r * ldn;
        float* rr = R + r * ldr;
        for (int c = lane; c < d; c += 64) {
            const float acc = tn[c];
            float t;
            if (m == SRG_CHEBY_INIT || m == SRG_CHEBY_INIT_T) {
                const float tc = Tc[r * ldc + c];
                t = e_div(e_sub(acc, e_mul(a2, tc)), a1);
                if (m == SRG_CHEBY_INIT)
                    for (int s = 0; s < n_scales; ++s)
                        rr[s * r_stride + c] = e_add(e_mul(cf.prev[s], tc), e_mul(cf.cur[s], t));
            } else if (m == SRG_CHEBY_STEP_FIRST) {
                const float t0 = To[r * ldo + c], t1 = Tc[r * ldc + c];
                t = e_sub(acc, t0);
                for (int s = 0; s < n_scales; ++s)
                    rr[s * r_stride + c] = e_add(e_add(e_mul(cf.prev[s], t0), e_mul(cf.mid[s], t1)), e_mul(cf.cur[s], t));
            } else {
                t = e_sub(acc, To[r * ldo + c]);
                for (int s = 0; s < n_scales; ++s)
                    rr[s * r_stride + c] = e_add(rr[s * r_stride + c], e_mul(cf.cur[s], t));
            }
            if (store_t) tn[c] = t;
        }
    }
}

// The fused step's mode and coefficients (cheby_epi_at): coef_prev holds c0 per scale (INIT) or c0 then c1
// per scale (STEP_FIRST), coef c1 (INIT) or ck (STEP, STEP_FIRST); INIT_T takes neither; | SRG_CHEBY_NO_T.
template <typename T>
int cheby_coefs(int mode, const T* coef_prev, const T* coef, int n_scales, ChebyCoef<T>& cf)
{
    const int m = mode & ~SRG_CHEBY_NO_T;
    if (m != SRG_CHEBY_INIT && m != SRG_CHEBY_STEP && m != SRG_CHEBY_INIT_T && m != SRG_CHEBY_STEP_FIRST)
        return srg_fail(SRG_ERR_INVALID, "cheby mode %d", mode);
    if (n_scales < 1 || n_scales > 8) return srg_fail(SRG_ERR_INVALID, "n_scales=%d not in [1,8]", n_scales);
    const bool needs_r = m != SRG_CHEBY_INIT_T;
    if ((needs_r && !coef) || ((m == SRG_CHEBY_INIT || m == SRG_CHEBY_STEP_FIRST) && !coef_prev))
        return srg_fail(SRG_ERR_INVALID, "null coefficient array");
    for (int i = 0; i < 8; ++i) {
        const bool on = i < n_scales;
        cf.prev[i] = ((m == SRG_CHEBY_INIT || m == SRG_CHEBY_STEP_FIRST) && on) ? T(0.5) * coef_prev[i] : T(0);
        cf.mid[i] = (m == SRG_CHEBY_STEP_FIRST && on) ? coef_prev[n_scales + i] : T(0);
        cf.cur[i] = (needs_r && on) ? coef[i] : T(0);
    }
    return SRG_OK;
}

// cheby_coefs, and the To panel that a step reads
template <typename T>
int cheby_setup(int mode, const T* coef_prev, const T* coef, int n_scales, const void* To, ChebyCoef<T>& cf)
{
    if (int rc = cheby_coefs<T>(mode, coef_prev, coef, n_scales, cf)) return rc;
    const int m = mode & ~SRG_CHEBY_NO_T;
    if ((m == SRG_CHEBY_STEP || m == SRG_CHEBY_STEP_FIRST) && !To) return srg_fail(SRG_ERR_INVALID, "null To for a step");
    return SRG_OK;
}

// n_hub (fp64 only): the first n_hub rows of `order` run as k_cheby_hub64 workgroups on the hub side
// stream beside the row waves of the others (joined before the call returns to the stream's order;
// with SRG_CHEBY_HUB_NOJOIN in mode, left running for srg_hub_join: later launches on the stream run
// beside them)
template <typename T>
int launch_cheby(const int64_t* indptr, const int32_t* indices, const T* vals, int64_t n_rows,
                 const int32_t* order, const T* Tc, const T* To, T* Tn, int64_t ld, int d, int mode,
                 T a1, T a2, const T* coef_prev, const T* coef, int n_scales, T* R, int64_t r_stride,
                 hipStream_t s, int64_t n_hub = 0)
{
    bool nojoin = false;
    if constexpr (sizeof(T) == 8) {
        nojoin = (mode & SRG_CHEBY_HUB_NOJOIN) != 0;
        mode &= ~SRG_CHEBY_HUB_NOJOIN;
    }
    ChebyCoef<T> cf;
    int rc = cheby_setup<T>(mode, coef_prev, coef, n_scales, To, cf);
    if (rc) return rc;
    rc = check_spmm_args(indptr, indices, vals, n_rows, Tc, ld, Tn, ld, d);
    if (rc) return rc;
    if (r_stride < n_rows * ld && n_scales > 1)
        return srg_fail(SRG_ERR_INVALID, "r_stride too small for stacked scale panels");
    if (n_hub < 0 || n_hub > n_rows || (n_hub > 0 && !order))
        return srg_fail(SRG_ERR_INVALID, "n_hub=%lld needs a row_order and <= n_rows", (long long)n_hub);
    if (n_rows == 0 || d == 0) return srg_ok();
    // hub workgroups gather 16-byte pieces (two columns) of Tc's rows
    if (sizeof(T) != 8 || d % 2 || ld % 2 || !aligned(Tc, 16)) n_hub = 0;
    const int n_slices = (d + kHub64Cols - 1) / kHub64Cols;
    if (n_hub * n_slices > INT32_MAX - 64) return srg_fail(SRG_ERR_INVALID, "too many hub slices");
    HubFork hub(s, g_hub64_lds);
    if constexpr (sizeof(T) == 8) {
        if (n_hub > 0) {   // fork: the hub rows' workgroups beside the row waves
            if (int rc = hub.fork()) return rc;
            launch_hub64(n_hub * n_slices, hub.stream(), indptr, indices, vals, order, n_slices, Tc, To, Tn, ld, d, mode,
                         a1, a2, cf, n_scales, R, r_stride);
            SRG_HIP_CHECK(hipGetLastError());
            if (int rc = hub.record_join(nojoin)) return rc;
            if (int rc = hub.delay()) return rc;
        }
    }
    order = order ? order + n_hub : nullptr;
    n_rows -= n_hub;
    const int64_t blocks = (n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vec = pick_vec(d, ld, ld, Tc, Tn, sizeof(T)) >= 2 && aligned(R, 2 * sizeof(T)) &&
                            (r_stride % 2 == 0) && (To == nullptr || aligned(To, 2 * sizeof(T)))
                        ? 2
                        : 1;
    const int nr = (int)n_rows;
    rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (vec == 2)
            hipLaunchKernelGGL((k_cheby<T, 2, kUnroll>), dim3(nb), dim3(kBlock), 0, s, indptr, indices,
                               vals, order, nr, Tc, To, Tn, ld, d, mode, a1, a2, cf, n_scales, R,
                               r_stride, (int)b0);
        else
            hipLaunchKernelGGL((k_cheby<T, 1, kUnroll>), dim3(nb), dim3(kBlock), 0, s, indptr, indices,
                               vals, order, nr, Tc, To, Tn, ld, d, mode, a1, a2, cf, n_scales, R,
                               r_stride, (int)b0);
        return launch_status();
    });
    if (rc) return rc;
    if (!nojoin)
        if (int rc = hub.join()) return rc;
    return srg_ok();
}

}  // namespace

extern "C" {

int srg_spmm_cheby_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                       int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                       const float* Tc, int64_t ldc, float* Tn, int64_t ldn, int32_t d, uint32_t flags,
                       int mode, float a1, float a2, const float* To, int64_t ldo, const float* coef_prev,
                       const float* coef, int32_t n_scales, float* R, int64_t ldr, int64_t r_stride,
                       void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_spmm_args(indptr, indices, values, n_rows, Tc, ldc, Tn, ldn, d);
    if (rc) return rc;
    if (mode != SRG_CHEBY_INIT && mode != SRG_CHEBY_STEP) return srg_fail(SRG_ERR_INVALID, "cheby mode %d", mode);
    Epi e{};
    rc = cheby_coefs<float>(mode, coef_prev, coef, n_scales, e.cf);
    if (rc) return rc;
    if (flags & SRG_SPMM_ACCUMULATE) return srg_fail(SRG_ERR_INVALID, "the Chebyshev epilogue starts every chain from 0");
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!R || ldr < d) return srg_fail(SRG_ERR_INVALID, "R=%p ldr=%lld < d=%d", (void*)R, (long long)ldr, d);
    if (n_scales > 1 && r_stride < n_rows * ldr && r_stride > -n_rows * ldr)
        return srg_fail(SRG_ERR_INVALID, "r_stride overlaps the scale panels");
    if (mode == SRG_CHEBY_STEP && (!To || ldo < d))
        return srg_fail(SRG_ERR_INVALID, "step needs To with ldo >= d (To=%p ldo=%lld)", (const void*)To, (long long)ldo);
    if (Tn == Tc) return srg_fail(SRG_ERR_INVALID, "Tn must not alias Tc (its rows are gathered)");
    if (mode == SRG_CHEBY_STEP && To == Tn && ldo != ldn)
        return srg_fail(SRG_ERR_INVALID, "Tn may alias To only with the same leading dimension");
    if (R == Tn || R == Tc || (mode == SRG_CHEBY_STEP && R == To)) return srg_fail(SRG_ERR_INVALID, "R must not alias a T panel");
    e.cto = mode == SRG_CHEBY_STEP ? To : nullptr;
    e.ldo = mode == SRG_CHEBY_STEP ? ldo : 0;
    e.R = R;
    e.ldr = ldr;
    e.r_stride = r_stride;
    e.cmode = mode;
    e.ns = n_scales;
    e.a1 = a1;
    e.a2 = a2;
    rc = launch_spmm<int64_t, kEpiCheby>(indptr, indices, values, n_rows, row_order, n_hub, n_heavy, Tc, ldc, Tn, ldn,
                                         d, flags, static_cast<hipStream_t>(stream), e);
    return rc ? rc : srg_ok();
}

int srg_cheby_step_f64(const int64_t* indptr, const int32_t* indices, const double* values,
                       int64_t n_rows, const int32_t* row_order, const double* Tc,
                       const double* To, double* Tn, int64_t ld, int32_t d, int mode, double a1,
                       double a2, const double* coef_prev, const double* coef, int32_t n_scales,
                       double* R, int64_t r_stride, void* stream)
{
    if (mode & SRG_CHEBY_HUB_NOJOIN) return srg_fail(SRG_ERR_INVALID, "cheby mode %d: HUB_NOJOIN needs the hub entry", mode);
    SRG_DEVICE_GUARD(stream);
    return launch_cheby<double>(indptr, indices, values, n_rows, row_order, Tc, To, Tn, ld, d, mode,
                                a1, a2, coef_prev, coef, n_scales, R, r_stride,
                                static_cast<hipStream_t>(stream));
}

int srg_cheby_step_hub_f64(const int64_t* indptr, const int32_t* indices, const double* values,
                           int64_t n_rows, const int32_t* row_order, int64_t n_hub, const double* Tc,
                           const double* To, double* Tn, int64_t ld, int32_t d, int mode, double a1,
                           double a2, const double* coef_prev, const double* coef, int32_t n_scales,
                           double* R, int64_t r_stride, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    return launch_cheby<double>(indptr, indices, values, n_rows, row_order, Tc, To, Tn, ld, d, mode,
                                a1, a2, coef_prev, coef, n_scales, R, r_stride,
                                static_cast<hipStream_t>(stream), n_hub);
}

// Library-internal (srg_plan.hip's srg_plan_cheby_step_f64): one fp64 Chebyshev step over a plan's
// launches.  roles[i]: SRG_CHEBY64_FIRST / _LAST bits (the block where launch i's rows' chains start /
// end), or SRG_CHEBY64_HUBS (the whole hub rows: k_cheby_hub64 on the hub side stream, joined at the
// end of the step).  A launch without spans by slot is the one-launch plan's CSR launch: srg_cheby_
// step_hub_f64 over its schedule.  `values` are the fp64 values at the plan's entry positions.
__attribute__((visibility("hidden"))) int srg_run_plan_cheby_f64(const srg_hop_launch* launches, const uint8_t* roles, int32_t n_launch, const int64_t* indptr,
                           const int32_t* indices, const double* values, const double* Tc, const double* To,
                           double* Tn, int64_t ld, int32_t d, int mode, double a1, double a2, const double* coef_prev,
                           const double* coef, int32_t n_scales, double* R, int64_t r_stride, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    ChebyCoef<double> cf;
    int rc0 = cheby_setup<double>(mode, coef_prev, coef, n_scales, To, cf);
    if (rc0) return rc0;
    if (d < 0 || ld < d) return srg_fail(SRG_ERR_INVALID, "d=%d, ld=%lld", d, (long long)ld);
    if (n_launch == 1 && !launches[0].slot_beg) {
        const srg_hop_launch& L = launches[0];
        return launch_cheby<double>(indptr, indices, values, L.n_rows, L.row_order, Tc, To, Tn, ld, d, mode, a1, a2,
                                    coef_prev, coef, n_scales, R, r_stride, s, L.n_hub);
    }
    int64_t n_total = 0;
    for (int i = 0; i < n_launch; ++i) {
        const srg_hop_launch& L = launches[i];
        if (!L.slot_beg || !L.slot_end || (L.n_rows > 0 && !L.row_order))
            return srg_fail(SRG_ERR_INVALID, "launch %d: a blocked fp64 step reads spans by slot", i);
        if (roles[i] & (SRG_CHEBY64_LAST | SRG_CHEBY64_HUBS)) n_total += L.n_rows;
    }
    if (d == 0 || n_total == 0) return srg_ok();
    if (!Tc || !Tn || !R || !indices || !values) return srg_fail(SRG_ERR_INVALID, "null panel or entry array");
    if (r_stride < n_total * ld && n_scales > 1) return srg_fail(SRG_ERR_INVALID, "r_stride too small for stacked scale panels");
    const bool v2 = d % 2 == 0 && ld % 2 == 0 && aligned(Tc, 16) && aligned(Tn, 16) && aligned(R, 16) &&
                    r_stride % 2 == 0 && (To == nullptr || aligned(To, 16));
    const int n_slices = (d + kHub64Cols - 1) / kHub64Cols;
    HubFork hub(s, g_hub64_lds);
    for (int i = 0; i < n_launch; ++i) {
        const srg_hop_launch& L = launches[i];
        if (L.n_rows <= 0) continue;
        int role = roles[i];
        if (role == SRG_CHEBY64_HUBS) {
            if (v2 && L.n_rows * n_slices <= INT32_MAX - 64) {   // fork: the hub workgroups beside the blocks
                if (int rc = hub.fork()) return rc;
                launch_hub64(L.n_rows * n_slices, hub.stream(), indptr, indices, values, L.row_order, n_slices, Tc, To,
                             Tn, ld, d, mode, a1, a2, cf, n_scales, R, r_stride);
                SRG_HIP_CHECK(hipGetLastError());
                if (int rc = hub.record_join(false)) return rc;   // joined below, before the step returns
                if (int rc = hub.delay()) return rc;
                continue;
            }
            role = SRG_CHEBY64_FIRST | SRG_CHEBY64_LAST;   // row waves over their whole spans
        }
        const int64_t blocks = (L.n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
        const int nr = (int)L.n_rows;
        // (uncapped: 4 or 6 waves per SIMD measured 0.5-3 % slower, profiles/r06i_cheby64_plan_sweep.txt)
        const int rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
#define SRG_LAUNCH_BLK64(V, F, LA)                                                                                \
    hipLaunchKernelGGL((k_cheby_blk64<V, kUnroll, F, LA>), dim3(nb), dim3(kBlock), 0, s, L.slot_beg, L.slot_end, \
                       L.row_order, nr, indices, values, Tc, To, Tn, ld, d, mode, a1, a2, cf, n_scales, R, r_stride, \
                       (int)b0)
#define SRG_LAUNCH_BLK64_V(F, LA)                  \
    do {                                           \
        if (v2) SRG_LAUNCH_BLK64(2, F, LA);        \
        else SRG_LAUNCH_BLK64(1, F, LA);           \
    } while (0)
            switch (role & (SRG_CHEBY64_FIRST | SRG_CHEBY64_LAST)) {
            case SRG_CHEBY64_FIRST | SRG_CHEBY64_LAST: SRG_LAUNCH_BLK64_V(true, true); break;
            case SRG_CHEBY64_FIRST: SRG_LAUNCH_BLK64_V(true, false); break;
            case SRG_CHEBY64_LAST: SRG_LAUNCH_BLK64_V(false, true); break;
            default: SRG_LAUNCH_BLK64_V(false, false); break;
            }
#undef SRG_LAUNCH_BLK64_V
#undef SRG_LAUNCH_BLK64
            return launch_status();
        });
        if (rc) return rc;
    }
    if (int rc = hub.join()) return rc;
    return srg_ok();
}

int srg_cheby_step_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                       int64_t n_rows, const int32_t* row_order, const float* Tc, const float* To,
                       float* Tn, int64_t ld, int32_t d, int mode, float a1, float a2,
                       const float* coef_prev, const float* coef, int32_t n_scales, float* R,
                       int64_t r_stride, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    return launch_cheby<float>(indptr, indices, values, n_rows, row_order, Tc, To, Tn, ld, d, mode,
                               a1, a2, coef_prev, coef, n_scales, R, r_stride,
                               static_cast<hipStream_t>(stream));
}

int srg_cheby_epilogue_f32(float* Tn, int64_t ldn, const float* Tc, int64_t ldc, const float* To,
                           int64_t ldo, int64_t n_rows, int32_t d, int mode, float a1, float a2,
                           const float* coef_prev, const float* coef, int32_t n_scales, float* R,
                           int64_t ldr, int64_t r_stride, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    ChebyCoef<float> cf;
    int rc = cheby_coefs<float>(mode, coef_prev, coef, n_scales, cf);
    if (rc) return rc;
    const int m = mode & ~SRG_CHEBY_NO_T;
    const bool init = m == SRG_CHEBY_INIT || m == SRG_CHEBY_INIT_T;
    const bool needs_r = m != SRG_CHEBY_INIT_T;
    if (n_rows < 0 || d < 0 || ldn < d || (needs_r && ldr < d) || (init ? ldc < d : ldo < d) ||
        (m == SRG_CHEBY_STEP_FIRST && ldc < d))
        return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d", (long long)n_rows, d);
    if (needs_r && n_scales > 1 && r_stride < n_rows * ldr && r_stride > -n_rows * ldr)
        return srg_fail(SRG_ERR_INVALID, "r_stride overlaps the scale panels");
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!Tn || (needs_r && !R) || (init ? !Tc : !To) || (m == SRG_CHEBY_STEP_FIRST && !Tc))
        return srg_fail(SRG_ERR_INVALID, "null panel");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_rows + 3) / 4, launch_cap(256 * 16));
    hipLaunchKernelGGL(k_cheby_epilogue, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       Tn, ldn, Tc, ldc, To, ldo, n_rows, d, mode, a1, a2, cf, n_scales, R, ldr, r_stride);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

}  // extern "C"
