// srg_spmm_kernels.h -- CSR x dense-panel propagation kernels for MI355X (gfx950, CDNA4) and their
// launch ladder, as templates over the epilogue: a translation unit instantiates the epilogues it
// launches (srg_spmm.hip: plain and span; srg_cheby.hip: the fused Chebyshev step).
//
// The hot path of the reference is FloatCSRMulDenseOMP (SSRG/operators/csrc/matmul.c:23-40): per
// output row, for every stored nonzero in CSR order, answer[i,:] = fma(a_ij, X[j,:], answer[i,:]).
// It is HBM-bound (~0.48 flop/B at d = 128): the work is gathering 4*d-byte rows of X, one per
// nonzero.  The design here:
//
//  * One wavefront (64 lanes) owns one output row and a 64*VEC-column tile of it; each lane owns
//    VEC consecutive columns and keeps their running sums in registers.  Every output element is
//    therefore one sequential fp32 fma chain in CSR order -- bit-identical to the reference.
//  * The row's (column id, value) stream is wave-uniform, so it is read with scalar loads into
//    SGPRs (s_load_dwordx*), and each X row address is a scalar base + the lane's column offset:
//    one vector instruction (global_load_dwordx{1,2,4}) per nonzero gathers the whole 4*d-byte row.
//  * U nonzeros are processed per step: U independent gathers are issued back to back (U rows in
//    flight per wave, ~U*512 B at d = 128), then consumed in order by the fma chain.  The chain is
//    4 cycles per link; the gathers are what the wave waits on.
//  * Rows are scheduled through an optional permutation (host plan: decreasing length), so the
//    long power-law hub rows start first and overlap the bulk instead of forming the tail.
//  * No atomics, no inter-workgroup communication, no LDS: each row is owned by exactly one wave.
//
// The Chebyshev (wavelet) kernels reuse the same row-wave gather and add a fused epilogue that
// forms the next Chebyshev term and accumulates every scale's filter output in the same pass.
#ifndef SRG_SPMM_KERNELS_H_
#define SRG_SPMM_KERNELS_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// SpMM: Y = A * X  (or Y += A * X)
//
// One launch, two wave roles (wave-uniform, decided by blockIdx):
//  * blocks [0, nb_heavy): "slice" waves.  The first n_heavy rows of `order` are long rows; each is
//    cut into 32-column slices (128 B of every X row = one cache line) and every (row, slice) pair
//    is one wave.  Lane l gathers the 16-byte chunk (l & 7) of nonzero (l >> 3): one
//    global_load_dwordx4 instruction brings 8 nonzeros' slices (1 KiB); UH such instructions are in
//    flight per wave.  The 8x32 tile is transposed through a wave-private LDS slot so that lane c
//    (c < 32) runs the sequential fma chain of column c over the nonzeros in CSR order.  A row of
//    degree D is worked on by d/32 waves at once with UH*1 KiB in flight each, which keeps
//    power-law hubs (D > 10^5 on the products-shaped graph) off the critical path.
//  * blocks [nb_heavy, ...): "row" waves, one per remaining row (row_gather, srg_device.h).
// Both roles produce bit-identical results (one fma chain per output element, CSR order).
// ------------------------------------------------------------------------------------------------
constexpr int kSliceCols = 32;
// LDS tiles per slice wave (8 nonzeros x 32 columns, 1 KB each).  One suffices: a wave's LDS
// operations complete in issue order, so the next group's write cannot overtake this group's reads.
// Two (the round-1 layout) cost 8 KB per k_spmm block, which beside the hub group's 72 KB workgroups
// (halo exchange) left room for only two row blocks per CU.
constexpr int kSliceLdsBufs = 1;
// The slice waves' (column id, value) loads for the next group of entries are issued right after the
// current group's gathers, so their latency overlaps the gathers and the fma links instead of
// preceding the next gathers.  Products (one box, profiles/r04u_prefetch_ab.txt): none 6.02 ms per
// hop, slice waves 5.82.  It costs 2 UH registers (73 instead of 54-70: 6 waves per SIMD).  Same
// entries in the same order: same bits.  (The packed light rows stage their ids across their lanes
// instead, packed_rows; their round-4 per-group prefetch and LDS-staged entries measured slower,
// profiles/r04h_stage_entries_negative.txt.)
constexpr bool kPrefetchSliceIds = true;

// Epilogues of the SpMM kernels (every output element y a kernel stores may also go to):
//  * fused hop aggregation (srgnn.aggregate): with agg != nullptr it is folded into the accumulator
//    panel, agg = (init ? 0 : agg) + w*y, with separate multiply and add -- the same arithmetic as a
//    following srg_hop_accumulate_f32 step, without re-reading Y;
//  * fused Chebyshev step (srgnn.wavelet, srg_spmm_cheby_f32): y = A*T_k becomes T_{k+1} before it
//    is stored and every scale's output is updated, with k_cheby_epilogue's arithmetic --
//      INIT: T1 = (y - a2*T0) / a1,  R_s = (c0_s/2)*T0 + c1_s*T1   (T0 = X, the gathered panel)
//      STEP: T_{k+1} = y - T_{k-1},  R_s += ck_s*T_{k+1}
//    T0 / T_{k-1} is read before the chain (its latency hides under the gathers).  Y may alias
//    T_{k-1}: every element is read and then written by its one owner, and no wave gathers it, so
//    a step needs two work panels instead of three and one panel pass less than the split path.
template <typename T> struct ChebyCoef {
    T prev[8];   // c0_s / 2 (INIT, STEP_FIRST)
    T cur[8];    // c1_s (INIT) or ck_s (STEP, STEP_FIRST)
    T mid[8];    // c1_s (STEP_FIRST only)
};

struct Epi {
    float* agg;
    int64_t lda;
    float w;
    int init;
    // fused Chebyshev step (EX == kEpiCheby only)
    const float* cto;     // T_{k-1} (STEP)
    int64_t ldo;
    float* R;             // R_s = R + s * r_stride, rows ldr apart
    int64_t ldr, r_stride;
    int cmode, ns;
    float a1, a2;
    ChebyCoef<float> cf;
    // row spans (EX == kEpiSpan only): row r's entries are [indptr[r], row_end[r]) instead of
    // [indptr[r], indptr[r + 1]) -- a column block of a CSR whose rows hold sorted column ids is a
    // span of each row, so the block needs no copy of the ids and values (srg_spmm_span_f32)
    const int64_t* row_end;
    // kEpiSpan, optional: the spans by schedule slot (slot_beg[s] / slot_end[s] = the span of the row
    // in slot s of this launch's light-row schedule), read by the packed light rows instead of the
    // row-indexed arrays: consecutive slots, consecutive addresses (srg_propagate_plan_f32)
    const int64_t* slot_beg;
    const int64_t* slot_end;
};

// The aggregation epilogue's fields (agg = (init ? 0 : agg) + w * Y), everything else off.
inline Epi agg_epi(float* agg, int64_t lda, float w, int agg_init)
{
    Epi e{};
    e.agg = agg;
    e.lda = lda;
    e.w = w;
    e.init = agg_init ? 1 : 0;
    return e;
}

// Epilogue kinds (template parameter EX of the SpMM kernels).  Every call site sits under
// `if constexpr`: a runtime branch cost the plain kernels ~20 %, and even an empty inlined call
// (the reference-bound acc) changed the gather loop's schedule (+10 % per hop on products);
// guarded, the kEpiPlain kernels are instruction-for-instruction the plain ones.  kEpiSpan is the
// plain epilogue (aggregation included) over row spans.
// (round 5 removed the fused halo pack, kEpiSend, and the per-row accumulation of the medium-span
// probe, kEpiSpanRA: both measured slower)
constexpr int kEpiPlain = 0, kEpiCheby = 2, kEpiSpan = 3;
template <int EX> constexpr bool kIsSpan = EX == kEpiSpan;

// End of row `row`'s entries: the next row's start, or the span's end.
template <int EX, typename IP>
__device__ __forceinline__ int64_t row_stop(const IP* __restrict__ indptr, const Epi& e, int row)
{
    if constexpr (kIsSpan<EX>)
        return e.row_end[row];
    else
        return (int64_t)indptr[row + 1];
}


// Operands of the Chebyshev epilogue at (row, col), loaded before the chain so that their latency
// hides under the gathers (loaded after it, the R round trips were the end of every light row:
// +40 % per order on products): T0 = X (INIT) or T_{k-1} (STEP), and in a step the current
// outputs of the first kChebyPre scales (further scales are read after the chain).
constexpr int kChebyPre = 2;
template <int VEC> struct ChebyOps {
    typename Vec<float, VEC>::type pre, r[kChebyPre];
};

template <int VEC>
__device__ __forceinline__ void cheby_load(const Epi& e, int row, int col, const float* __restrict__ X, int64_t ldx,
                                           ChebyOps<VEC>& o)
{
    if (e.cmode == SRG_CHEBY_INIT) {
        o.pre = vload<float, VEC>(X + (int64_t)row * ldx + col);
    } else {
        o.pre = vload<float, VEC>(e.cto + (int64_t)row * e.ldo + col);
        const float* rr = e.R + (int64_t)row * e.ldr + col;
#pragma unroll
        for (int s = 0; s < kChebyPre; ++s)
            if (s < e.ns) o.r[s] = vload<float, VEC>(rr + s * e.r_stride);
    }
}

// acc = A*T_k at (row, col) becomes T_{k+1}; R_s updated (k_cheby_epilogue's operations, in order).
template <int VEC>
__device__ __forceinline__ void cheby_epi(const Epi& e, int row, int col, typename Vec<float, VEC>::type& acc,
                                          const ChebyOps<VEC>& o)
{
    typedef typename Vec<float, VEC>::type V;
    V t;
    float* rr = e.R + (int64_t)row * e.ldr + col;
    if (e.cmode == SRG_CHEBY_INIT) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) elem(t, i) = e_div(e_sub(elem(acc, i), e_mul(e.a2, elem(o.pre, i))), e.a1);
        for (int s = 0; s < e.ns; ++s) {
            V r;
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                elem(r, i) = e_add(e_mul(e.cf.prev[s], elem(o.pre, i)), e_mul(e.cf.cur[s], elem(t, i)));
            vstore<float, VEC>(rr + s * e.r_stride, r, false);
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) elem(t, i) = e_sub(elem(acc, i), elem(o.pre, i));
#pragma unroll
        for (int s = 0; s < kChebyPre; ++s) {
            if (s < e.ns) {
                V r = o.r[s];
#pragma unroll
                for (int i = 0; i < VEC; ++i) elem(r, i) = e_add(elem(r, i), e_mul(e.cf.cur[s], elem(t, i)));
                vstore<float, VEC>(rr + s * e.r_stride, r, false);
            }
        }
        for (int s = kChebyPre; s < e.ns; ++s) {
            V r = vload<float, VEC>(rr + s * e.r_stride);
#pragma unroll
            for (int i = 0; i < VEC; ++i) elem(r, i) = e_add(elem(r, i), e_mul(e.cf.cur[s], elem(t, i)));
            vstore<float, VEC>(rr + s * e.r_stride, r, false);
        }
    }
    acc = t;
}

template <int UH, bool SFULL, typename IP, int EX>
__device__ __forceinline__ void slice_wave(const IP* __restrict__ indptr,
                                           const int32_t* __restrict__ indices,
                                           const float* __restrict__ vals, int row, int slice,
                                           const float* __restrict__ X, int64_t ldx,
                                           float* __restrict__ Y, int64_t ldy, int d, int accumulate,
                                           int nt, float* __restrict__ lds, const Epi& epi)
{
    typedef typename Vec<float, 4>::type V4;
    const int lane = threadIdx.x & 63;
    const int g = lane >> 3;                 // nonzero within a group of 8
    const int qcol = slice * kSliceCols + (lane & 7) * 4;   // gather columns of this lane
    const bool gact = SFULL || qcol < d;
    const int ccol = slice * kSliceCols + lane;             // chain column of this lane
    const bool cact = lane < kSliceCols && (SFULL || ccol < d);
    float* __restrict__ yrow = Y + (int64_t)row * ldy;
    float acc = 0.0f;
    const int64_t beg = indptr[row];
    if (accumulate && cact) acc = yrow[ccol];
    const float aprev = (epi.agg && !epi.init && cact) ? epi.agg[(int64_t)row * epi.lda + ccol] : 0.0f;
    [[maybe_unused]] ChebyOps<1> cop;
    if constexpr (EX == kEpiCheby)
        if (cact) cheby_load<1>(epi, row, ccol, X, ldx, cop);
    const int64_t end = row_stop<EX>(indptr, epi, row);
    float av[UH];
    int cv[UH];
    auto load_ids = [&](int64_t j0, int* c, float* a) {   // clamped: no branches
#pragma unroll
        for (int b = 0; b < UH; ++b) {
            int64_t jj = j0 + b * 8 + g;
            jj = jj < end ? jj : end - 1;
            c[b] = indices[jj];
            a[b] = vals[jj];
        }
    };
    if (kPrefetchSliceIds && beg < end) load_ids(beg, cv, av);
    for (int64_t j = beg; j < end; j += 8 * UH) {
        V4 x[UH];
        if constexpr (!kPrefetchSliceIds) load_ids(j, cv, av);   // all index/value loads first ...
        __builtin_amdgcn_sched_barrier(0);   // keep every index load ahead of the first gather
#pragma unroll
        for (int b = 0; b < UH; ++b)     // ... then UH dependent gathers in flight
            x[b] = gact ? gload<float, 4>(X + (int64_t)cv[b] * ldx + qcol) : vzero<float, 4>();
        [[maybe_unused]] int ncv[UH];
        [[maybe_unused]] float nav[UH];
        if constexpr (kPrefetchSliceIds) {    // the next group's ids behind the gathers
            if (j + 8 * UH < end) load_ids(j + 8 * UH, ncv, nav);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int b = 0; b < UH; ++b) {
            const int64_t jb = j + b * 8;
            if (jb >= end) break;                               // wave-uniform
            const int nb = (end - jb) < 8 ? (int)(end - jb) : 8;
            float* slot = lds + (kSliceLdsBufs == 2 ? (b & 1) * 256 : 0);
            *reinterpret_cast<V4*>(slot + lane * 4) = x[b];     // tile [g][32 cols]
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = slot[q * kSliceCols + (lane & 31)];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, av[b]), q * 8));
                if (q < nb && cact) acc = __builtin_fmaf(a, t[q], acc);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if constexpr (kPrefetchSliceIds) {
#pragma unroll
            for (int b = 0; b < UH; ++b) {
                cv[b] = ncv[b];
                av[b] = nav[b];
            }
        }
    }
    if (cact) {
        if constexpr (EX == kEpiCheby) cheby_epi<1>(epi, row, ccol, acc, cop);
        if (nt)
            __builtin_nontemporal_store(acc, yrow + ccol);
        else
            yrow[ccol] = acc;
        if (epi.agg) epi.agg[(int64_t)row * epi.lda + ccol] = __fadd_rn(aprev, __fmul_rn(epi.w, acc));
    }
}

// Narrow panels (d <= 32): a row wave would leave 64 - d lanes idle, so here one wave runs
// R = 64 / S rows at once, S = the power of two >= d lanes per row (lane = sub-row g, column c).
// Each lane loads its own row's (column id, value) stream -- the S lanes of a row read the same
// address, one instruction for the whole wave -- then U gathers in flight, then U fma links.
// Rows come from the degree-sorted schedule, so the R rows of a wave have similar lengths.
// Still one sequential fma chain per output element, in CSR order.
template <int S, int U, typename IP, int EX>
__device__ __forceinline__ void narrow_rows(const IP* __restrict__ indptr, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, const int32_t* __restrict__ order,
                                            int n_rows, int first, const float* __restrict__ X, int64_t ldx,
                                            float* __restrict__ Y, int64_t ldy, int d, int accumulate, int nt,
                                            const Epi& epi)
{
    const int lane = threadIdx.x & 63;
    const int g = lane / S, c = lane % S;
    const int slot = first + g;
    const bool rv = slot < n_rows;
    const int row = rv ? (order ? order[slot] : slot) : 0;
    const bool act = rv && c < d;
    const int64_t beg = rv ? (int64_t)indptr[row] : 0;
    const int len = rv ? (int)(row_stop<EX>(indptr, epi, row) - beg) : 0;
    int maxlen = len;
#pragma unroll
    for (int off = S; off < 64; off <<= 1) {
        const int o = __shfl_xor(maxlen, off);
        maxlen = o > maxlen ? o : maxlen;
    }
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    float* __restrict__ yrow = Y + (int64_t)row * ldy;
    float acc = (accumulate && act) ? yrow[c] : 0.0f;
    const float aprev = (epi.agg && !epi.init && act) ? epi.agg[(int64_t)row * epi.lda + c] : 0.0f;
    [[maybe_unused]] ChebyOps<1> cop;
    if constexpr (EX == kEpiCheby)
        if (act) cheby_load<1>(epi, row, c, X, ldx, cop);
    for (int j = 0; j < maxlen; j += U) {
        int cv[U];
        float av[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool ok = j + u < len;
            const int64_t p = beg + (ok ? j + u : 0);
            cv[u] = ok ? indices[p] : 0;
            av[u] = ok ? vals[p] : 0.0f;
        }
        __builtin_amdgcn_sched_barrier(0);   // every id load ahead of the first gather
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            x[u] = (act && j + u < len) ? X[(int64_t)cv[u] * ldx + c] : 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (act && j + u < len) acc = __builtin_fmaf(av[u], x[u], acc);
    }
    if (act) {
        if constexpr (EX == kEpiCheby) cheby_epi<1>(epi, row, c, acc, cop);
        if (nt)
            __builtin_nontemporal_store(acc, yrow + c);
        else
            yrow[c] = acc;
        if (epi.agg) epi.agg[(int64_t)row * epi.lda + c] = __fadd_rn(aprev, __fmul_rn(epi.w, acc));
    }
}

// Light rows of wide panels (d = LQ * 4 * S, S = 64 / LR): one wave runs LR rows at once, S lanes
// per row, each lane LQ 16-byte column chunks (chunk q of lane l: columns q*4S + 4l .. +3, so the S
// lanes of a row read 16*S contiguous bytes per gather).  A one-row wave walks its row's short
// stream through a chain of dependent loads (schedule slot -> row pointers -> column ids -> X) and
// the phase is bound by how many rows are in flight, not by bytes; LR rows per wave multiply that.
// The S lanes of a row load S consecutive (column id, value) entries of it at once and hand them
// out by ds_bpermute, U gathers per row in flight, then the fma links in CSR order.  Entries past a
// row's end are skipped (never folded in as 0*x).  Still one sequential fma chain per output element.
template <int LR, int LQ, int U, typename IP, int EX>
__device__ __forceinline__ void packed_rows(const IP* __restrict__ indptr, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, const int32_t* __restrict__ order,
                                            int n_rows, int first, const float* __restrict__ X, int64_t ldx,
                                            float* __restrict__ Y, int64_t ldy, int accumulate, int nt,
                                            const Epi& epi)
{
    typedef typename Vec<float, 4>::type V4;
    constexpr int S = 64 / LR;
    static_assert(S % U == 0, "a row's id chunk holds whole groups of U entries");
    const int lane = threadIdx.x & 63;
    const int g = lane / S, l = lane % S;
    const int slot = first + g;
    const bool rv = slot < n_rows;
    const int row = rv ? (order ? order[slot] : slot) : 0;
    int64_t beg = 0;
    int len = 0;
    if (rv) {
        if constexpr (kIsSpan<EX>) {
            if (epi.slot_beg) {
                beg = epi.slot_beg[slot];
                len = (int)(epi.slot_end[slot] - beg);
            } else {
                beg = indptr[row];
                len = (int)(epi.row_end[row] - beg);
            }
        } else {
            beg = indptr[row];
            len = (int)(row_stop<EX>(indptr, epi, row) - beg);
        }
    }
    int maxlen = len;
#pragma unroll
    for (int off = S; off < 64; off <<= 1) {
        const int o = __shfl_xor(maxlen, off);
        maxlen = o > maxlen ? o : maxlen;
    }
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    float* __restrict__ yrow = Y + (int64_t)row * ldy;
    // the Chebyshev epilogue never aggregates nor accumulates (its entry rejects both): dropping
    // them statically keeps its registers (the prefetched operands) within 5 waves per SIMD
    float* __restrict__ arow = (EX != kEpiCheby && epi.agg) ? epi.agg + (int64_t)row * epi.lda : nullptr;
    V4 acc[LQ], aprev[LQ];
    [[maybe_unused]] ChebyOps<4> cop[LQ];
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
        const int col = q * 4 * S + 4 * l;
        acc[q] = (EX != kEpiCheby && accumulate && rv) ? vload<float, 4>(yrow + col) : vzero<float, 4>();
        aprev[q] = (arow && !epi.init && rv) ? vload<float, 4>(arow + col) : vzero<float, 4>();
        if constexpr (EX == kEpiCheby)
            if (rv) cheby_load<4>(epi, row, col, X, ldx, cop[q]);
    }
    // The row's entries S at a time: lane l of the row loads the (column id, value) of entry j0 + l, and
    // each group of U gathers takes its ids from the row's S lanes by ds_bpermute, so the dependent
    // chain per U entries is the gather alone (one id load per S entries instead of one per U); the
    // next S entries' ids load behind the current chunk's gathers.  Products 5.52 -> 5.33 ms per hop,
    // arxiv 0.157 -> 0.154 (round 5, profiles/r05ab_shfl_ids_ab.txt; before, every U entries began
    // with their id loads).  Entries past a row's end load nothing and are skipped.
    const int base = g * S;
    auto load_ids = [&](int j0, int& c, float& a) {
        const bool ok = j0 + l < len;
        const int64_t p = beg + (ok ? j0 + l : 0);
        c = ok ? indices[p] : 0;
        a = ok ? vals[p] : 0.0f;
    };
    if constexpr (U <= 2) {
    // U = 2 (the column blocks' launches): two chunks of ids (A: entries [ca, ca + S), B: the next S)
    // and two gather buffers, so step j + U's gathers are issued before step j's fma links -- 2U
    // gathers in flight across the steps.  Products 5.33 -> 5.27 ms per hop; with U = 4 (the one-launch
    // hop) the same pipeline costs arxiv 6 % (0.154 -> 0.163 ms: 8 gathers in flight per row, like
    // U = 8), so that keeps one U-group in flight (profiles/r05af_pipe_gathers_ab.txt)
    int ida = 0, idb = 0;
    float vaa = 0.0f, vab = 0.0f;
    int ca = 0;
    if (maxlen > 0) load_ids(0, ida, vaa);
    if (S < maxlen) load_ids(S, idb, vab);
    auto issue = [&](int j, V4 (&x)[U][LQ], float (&av)[U]) {
        const bool in_a = j < ca + S;            // wave-uniform
        const int off = base + (j & (S - 1));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = __shfl(in_a ? ida : idb, off + u);
            av[u] = __shfl(in_a ? vaa : vab, off + u);
#pragma unroll
            for (int q = 0; q < LQ; ++q)
                x[u][q] = (j + u < len) ? gload<float, 4>(X + (int64_t)c * ldx + q * 4 * S + 4 * l) : vzero<float, 4>();
        }
    };
    auto links = [&](int j, const V4 (&x)[U][LQ], const float (&av)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j + u < len)
#pragma unroll
                for (int q = 0; q < LQ; ++q) chain<float, 4>(acc[q], av[u], x[u][q]);
        if (j + U == ca + S) {                   // chunk A done: B becomes A, B loads the next S
            ida = idb;
            vaa = vab;
            ca += S;
            if (ca + S < maxlen) load_ids(ca + S, idb, vab);
        }
    };
    V4 xa[U][LQ], xb[U][LQ];
    float fa[U], fb[U];
    if (maxlen > 0) issue(0, xa, fa);
    for (int j = 0; j < maxlen; j += 2 * U) {
        if (j + U < maxlen) issue(j + U, xb, fb);
        links(j, xa, fa);
        if (j + U >= maxlen) break;
        if (j + 2 * U < maxlen) issue(j + 2 * U, xa, fa);
        links(j + U, xb, fb);
    }
    } else {
    int nid = 0;
    float nva = 0.0f;
    if (maxlen > 0) load_ids(0, nid, nva);
    for (int j0 = 0; j0 < maxlen; j0 += S) {
        const int cid = nid;
        const float cva = nva;
        if (j0 + S < maxlen) load_ids(j0 + S, nid, nva);
        const int nstep = (maxlen - j0) < S ? (maxlen - j0) : S;   // wave-uniform; S is a multiple of U
        for (int jj = 0; jj < nstep; jj += U) {
            int cv[U];
            float av[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cv[u] = __shfl(cid, base + jj + u);
                av[u] = __shfl(cva, base + jj + u);
            }
            const int j = j0 + jj;
            V4 x[U][LQ];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < LQ; ++q)
                    x[u][q] = (j + u < len) ? gload<float, 4>(X + (int64_t)cv[u] * ldx + q * 4 * S + 4 * l)
                                            : vzero<float, 4>();
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (j + u < len)
#pragma unroll
                    for (int q = 0; q < LQ; ++q) chain<float, 4>(acc[q], av[u], x[u][q]);
        }
    }
    }
    if (!rv) return;
#pragma unroll
    for (int q = 0; q < LQ; ++q) {
        const int col = q * 4 * S + 4 * l;
        if constexpr (EX == kEpiCheby) cheby_epi<4>(epi, row, col, acc[q], cop[q]);
        vstore<float, 4>(yrow + col, acc[q], nt != 0);
        if (arow) {
#pragma unroll
            for (int i = 0; i < 4; ++i) aprev[q][i] = __fadd_rn(aprev[q][i], __fmul_rn(epi.w, acc[q][i]));
            vstore<float, 4>(arow + col, aprev[q], false);
        }
    }
}

template <int VEC, int U, int UH, bool FULL, bool SFULL, typename IP, int NS = 0, int EX = kEpiPlain, int LR = 0, int LQ = 1,
          bool XH = false>
__global__ void __launch_bounds__(kBlock)
k_spmm(const IP* __restrict__ indptr, const int32_t* __restrict__ indices,
       const float* __restrict__ vals, const int32_t* __restrict__ order, int n_rows, int n_heavy,
       int n_slices, int nb_heavy, const float* __restrict__ X, int64_t ldx, float* __restrict__ Y,
       int64_t ldy, int d, int accumulate, int nt, int block_base, Epi epi)
{
    typedef typename Vec<float, VEC>::type V;
    const int bid = block_base + (int)blockIdx.x;
    // dynamic: at least kSpmmLdsBytes, more when the launch caps its blocks per CU (spmm_lds_bytes)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    if (bid < nb_heavy) {
        if constexpr (XH) {
            // XCD-aware slice waves: blocks are dealt round-robin over the 8 XCDs (b and b + 8 share
            // one), so block b takes slice (b % 8) % n_slices of 4 rows: an XCD's L2 then holds one
            // slice of the X rows these waves gather.  Groups of 8 blocks cover 8 / n_slices row
            // groups x every slice.
            const int per = 8 / n_slices, x = bid & 7;
            const int item = __builtin_amdgcn_readfirstlane(((bid >> 3) * per + x / n_slices) * kWavesPerBlock + wib);
            if (item >= n_heavy) return;
            slice_wave<UH, SFULL, IP, EX>(indptr, indices, vals, order[item], x % n_slices, X, ldx, Y, ldy, d,
                                            accumulate, nt, lds + wib * kSliceLdsBufs * 256, epi);
            return;
        }
        const int item = __builtin_amdgcn_readfirstlane(bid * kWavesPerBlock + wib);
        if (item >= n_heavy * n_slices) return;
        const int row = order[item / n_slices];
        slice_wave<UH, SFULL, IP, EX>(indptr, indices, vals, row, item % n_slices, X, ldx, Y, ldy, d,
                           accumulate, nt, lds + wib * kSliceLdsBufs * 256, epi);
        return;
    }
    if constexpr (LR > 0) {   // wide panel: LR light rows per wave
        const int first = __builtin_amdgcn_readfirstlane((bid - nb_heavy) * kWavesPerBlock + wib) * LR + n_heavy;
        if (first >= n_rows) return;
        packed_rows<LR, LQ, U, IP, EX>(indptr, indices, vals, order, n_rows, first, X, ldx, Y, ldy, accumulate, nt, epi);
        return;
    }
    if constexpr (NS > 0) {   // narrow panel: 64 / NS light rows per wave
        const int first = __builtin_amdgcn_readfirstlane((bid - nb_heavy) * kWavesPerBlock + wib) * (64 / NS) + n_heavy;
        if (first >= n_rows) return;
        narrow_rows<NS, U, IP, EX>(indptr, indices, vals, order, n_rows, first, X, ldx, Y, ldy, d, accumulate, nt, epi);
        return;
    }
    const int w = __builtin_amdgcn_readfirstlane((bid - nb_heavy) * kWavesPerBlock + wib) + n_heavy;
    if (w >= n_rows) return;
    const int row = order ? order[w] : w;
    float* __restrict__ yrow = Y + (int64_t)row * ldy;
    for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
        const int col = c0 + lane * VEC;
        const bool act = col < d;
        V acc = vzero<float, VEC>();
        if (EX != kEpiCheby && accumulate && (FULL || act)) acc = vload<float, VEC>(yrow + col);
        // the accumulator row is loaded before the chain, so its latency hides under the gathers
        V aprev = vzero<float, VEC>();
        float* arow = (EX != kEpiCheby && epi.agg) ? epi.agg + (int64_t)row * epi.lda : nullptr;
        if (arow && !epi.init && (FULL || act)) aprev = vload<float, VEC>(arow + col);
        [[maybe_unused]] ChebyOps<VEC> cop;
        if constexpr (EX == kEpiCheby)
            if (FULL || act) cheby_load<VEC>(epi, row, col, X, ldx, cop);
        row_gather<float, VEC, U, FULL, IP, kIsSpan<EX>>(acc, indptr, indices, vals, row, X, ldx, col, act,
                                                            epi.row_end);
        if (FULL || act) {
            if constexpr (EX == kEpiCheby) cheby_epi<VEC>(epi, row, col, acc, cop);
            vstore<float, VEC>(yrow + col, acc, nt != 0);
            if (arow) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) elem(aprev, i) = __fadd_rn(elem(aprev, i), __fmul_rn(epi.w, elem(acc, i)));
                vstore<float, VEC>(arow + col, aprev, false);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// hub rows: one workgroup per (row, 32-column slice), producer/consumer through LDS
//
// A slice wave keeps 8 KiB of gathers in flight, so a row of degree D costs ~D/64 load latencies
// (~6 ms for the 155,868-entry hub of the products-shaped graph): hidden at 1 GPU, the whole hop
// at 8.  Here the row's chain is fed from LDS by 8 producer waves:
//   * windows of kHubW = 512 nonzeros, double-buffered tiles: while the consumer runs window h
//     from one tile, the producers write window h+1 into the other (one barrier per window);
//   * each producer lane gathers W / 64 = 8 dwordx4 (8 nonzeros' 128-byte slices per wave
//     instruction) per window into one of two register sets, so a window's gathers are issued
//     two windows before they are written (~2 us of latency cover); the column ids / values of
//     the next window are loaded one window ahead;
//   * the tile is transposed, [32 columns][W + 16] with the 4-nonzero group index XOR-swizzled
//     per column group (conflict-free ds_write_b32 and ds_read_b128, see HubGeom);
//   * the consumer wave (lanes 0..31, one column each) runs the 32 chains, 4 links per
//     ds_read_b128, with a ring of three 16-link register sets so every LDS read is issued two
//     sets (~32 links) before its fmas.
// Still exactly one fma chain per output element, in CSR order.
// ------------------------------------------------------------------------------------------------
constexpr int kHubProducers = 8;
constexpr int kHubW = 512;                                   // nonzeros per window (the default)
constexpr int kHubThreads = 64 * (kHubProducers + 1);
// Window geometry for W nonzeros per window.  W = 512 (139 KB of LDS, one workgroup per CU) is the
// lowest-latency chain, for a few hub rows beside a big launch (one GPU).  W = 256 (72 KB) lets two
// workgroups share a CU, for launches with more hub workgroups than CUs (the halo exchange's hub
// group: hundreds of rows per rank), where the CUs' LDS, not one chain's latency, sets the time.
// Floats per tile column: W + 16 == 16 (mod 64).  With the 4-link group index XOR-ed by (c >> 2) & 7,
// both the producers' transposed ds_write_b32 (lanes: 4 nonzeros x 8 column chunks) and the
// consumer's ds_read_b128 (lanes: 32 columns, 16-lane groups) are bank-conflict-free (exhaustive
// check over all window offsets; the 4 (mod 64) stride of the first version made the reads 2-way)
template <int W, int NP = kHubProducers>
struct HubGeom {
    static constexpr int UW = W / (NP * 8);                  // gathers per producer lane per window
    static constexpr int LD = W + 16;
    static constexpr int TILE = kSliceCols * LD;             // floats per tile
    static constexpr size_t LDS_BYTES = (size_t)(2 * TILE + 2 * W) * sizeof(float);
};
constexpr int kHubWideLaunch = 256;   // more hub workgroups than this (the CU count) -> W = kHubWideW
constexpr int kHubWideW = 256;
__device__ __forceinline__ int hub_swz(int c) { return (c >> 2) & 7; }
// Full windows take their link values by DPP quad broadcast (hub_links16; the value-read-per-4-links
// loop it replaced in round 3 was removed in round 5)
constexpr int kHubDppL = 3;   // 16-link sets in flight (4 tile reads + 1 value read each)

// 16 links of one column chain: link 4i + j multiplies x = t[i][j] by the value that quad lane i
// holds in a[j] (quad_perm broadcast), acc = fma(value, x, acc) -- v_fmac_f32 with a DPP first
// operand, one instruction per link.  One asm block: the compiler's hazard pass would otherwise pad
// every link with an s_nop (it treats the chained accumulator like a DPP source; 0.95 vs 0.86 ms on
// the products hub row).  The DPP'd operands a[] normally come straight from LDS reads, but nothing
// stops the register allocator from producing one with a VALU copy (v_mov / v_accvgpr_read) right
// before the block, and gfx9 needs 2 wait states between a VALU write of a VGPR and a DPP read of
// it: the hazard pass cannot see inside the asm, so the block opens with its own `s_nop 1`.  This
// guard must stay (2 cycles per 16 links).
__device__ __forceinline__ void hub_links16(float& acc, const typename Vec<float, 4>::type& a,
                                            const typename Vec<float, 4>::type (&t)[4])
{
#define SRG_QP(I) " quad_perm:[" #I "," #I "," #I "," #I "] row_mask:0xf bank_mask:0xf\n"
    asm volatile(
        "s_nop 1\n"
        "v_fmac_f32_dpp %0, %1, %5" SRG_QP(0) "v_fmac_f32_dpp %0, %2, %6" SRG_QP(0)
        "v_fmac_f32_dpp %0, %3, %7" SRG_QP(0) "v_fmac_f32_dpp %0, %4, %8" SRG_QP(0)
        "v_fmac_f32_dpp %0, %1, %9" SRG_QP(1) "v_fmac_f32_dpp %0, %2, %10" SRG_QP(1)
        "v_fmac_f32_dpp %0, %3, %11" SRG_QP(1) "v_fmac_f32_dpp %0, %4, %12" SRG_QP(1)
        "v_fmac_f32_dpp %0, %1, %13" SRG_QP(2) "v_fmac_f32_dpp %0, %2, %14" SRG_QP(2)
        "v_fmac_f32_dpp %0, %3, %15" SRG_QP(2) "v_fmac_f32_dpp %0, %4, %16" SRG_QP(2)
        "v_fmac_f32_dpp %0, %1, %17" SRG_QP(3) "v_fmac_f32_dpp %0, %2, %18" SRG_QP(3)
        "v_fmac_f32_dpp %0, %3, %19" SRG_QP(3) "v_fmac_f32_dpp %0, %4, %20" SRG_QP(3)
        : "+v"(acc)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]),
          "v"(t[0][0]), "v"(t[0][1]), "v"(t[0][2]), "v"(t[0][3]), "v"(t[1][0]), "v"(t[1][1]), "v"(t[1][2]), "v"(t[1][3]),
          "v"(t[2][0]), "v"(t[2][1]), "v"(t[2][2]), "v"(t[2][3]), "v"(t[3][0]), "v"(t[3][1]), "v"(t[3][2]), "v"(t[3][3]));
#undef SRG_QP
}

// kHubProducers producer waves + the consumer (the round-1 ablations and the round-4 4-producer
// "lite" workgroup were removed in round 5: DESIGN.md §5.1, §7)
template <bool SFULL, typename IP, int EX = kEpiPlain, int W = kHubW>
__global__ void __launch_bounds__(kHubThreads)
k_spmm_hub(const IP* __restrict__ indptr, const int32_t* __restrict__ indices,
           const float* __restrict__ vals, const int32_t* __restrict__ hub_rows, int n_slices,
           const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int d,
           int accumulate, int nt, Epi epi)
{
    typedef typename Vec<float, 4>::type V4;
    extern __shared__ __attribute__((aligned(16))) float hub_lds[];
    // [2 tiles][32 columns][HubGeom<W>::LD] then [2][W] values
    float* aval_base = hub_lds + 2 * HubGeom<W>::TILE;
    const int item = blockIdx.x;
    const int row = hub_rows[item / n_slices];
    const int slice = item % n_slices;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t beg = indptr[row];
    const int64_t end = row_stop<EX>(indptr, epi, row);
    const int n_win = (int)((end - beg + W - 1) / W);

    if (wave == 0) {   // ---------------- consumer: 32 column chains ----------------
        const int c = lane & 31;
        const int ccol = slice * kSliceCols + c;
        const bool cact = lane < kSliceCols && (SFULL || ccol < d);
        float* __restrict__ yrow = Y + (int64_t)row * ldy;
        float acc = 0.0f;
        if (accumulate && cact) acc = yrow[ccol];
        const float aprev = (epi.agg && !epi.init && cact) ? epi.agg[(int64_t)row * epi.lda + ccol] : 0.0f;
        [[maybe_unused]] ChebyOps<1> cop;
        if constexpr (EX == kEpiCheby)
            if (cact) cheby_load<1>(epi, row, ccol, X, ldx, cop);
        const int sw = hub_swz(c);
        constexpr int G = 2;                      // groups of 4 links per register set (8 links)
        V4 tA[G], aA[G], tB[G], aB[G], tC[G], aC[G], tD[G], aD[G];
        for (int h = 0; h < n_win; ++h) {
            __syncthreads();                      // window h is in tile h & 1
            if (lane < kSliceCols) {
                const float* tcol = hub_lds + (h & 1) * HubGeom<W>::TILE + c * HubGeom<W>::LD;
                const float* av = aval_base + (h & 1) * W;
                const int64_t sb = beg + (int64_t)h * W;
                const int nb = (end - sb) < W ? (int)(end - sb) : W;
                const int nc = nb / (4 * G);      // full 8-link sets
                auto ld = [&](int set, V4 (&t)[G], V4 (&a)[G]) {
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        const int grp = set * G + i;
                        t[i] = *reinterpret_cast<const V4*>(tcol + ((grp ^ sw) << 2));
                        a[i] = *reinterpret_cast<const V4*>(av + (grp << 2));   // broadcast
                    }
                };
                auto run = [&](const V4 (&t)[G], const V4 (&a)[G]) {
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        acc = __builtin_fmaf(a[i][0], t[i][0], acc);
                        acc = __builtin_fmaf(a[i][1], t[i][1], acc);
                        acc = __builtin_fmaf(a[i][2], t[i][2], acc);
                        acc = __builtin_fmaf(a[i][3], t[i][3], acc);
                    }
                };
                if (nb == W) {
                    // full window, values by DPP: per 16 links one ds_read_b128 of values (lane l
                    // reads values 16k + 4 (l & 3) .. +3, so register j of quad lane i holds value
                    // 16k + 4i + j) and four tile reads (4 links each); link 4i + j is
                    //   v_fmac_f32_dpp acc, a[j], t_i[j] quad_perm:[i,i,i,i]
                    // (the quad broadcast of lane i's a[j] as the fma's first operand: the same
                    // fused multiply-add as v_fma_f32, so the chain keeps its bits).  The value
                    // reads drop from one per 4 links to one per 16.  Ring: kHubDppL 16-link sets
                    // in flight (5 LDS reads each, 5 * kHubDppL <= 15 = lgkmcnt's range).
                    constexpr int NK = W / 16;
                    const float* tb[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) tb[k] = hub_lds + (h & 1) * HubGeom<W>::TILE + c * HubGeom<W>::LD + ((k ^ sw) << 2);
                    const float* avl = av + 4 * (lane & 3);
                    auto rt = [&](int grp) { return *reinterpret_cast<const V4*>(tb[grp & 7] + (grp >> 3) * 32); };
                    auto rv = [&](int k) { return *reinterpret_cast<const V4*>(avl + 16 * k); };
                    V4 t[kHubDppL][4], a[kHubDppL];
#pragma unroll
                    for (int r = 0; r < kHubDppL; ++r) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) t[r][i] = rt(4 * r + i);
                        a[r] = rv(r);
                    }
#pragma unroll
                    for (int k0 = 0; k0 < NK; k0 += kHubDppL) {
#pragma unroll
                        for (int r = 0; r < kHubDppL; ++r) {
                            const int k = k0 + r;
                            if (k < NK) {
                                hub_links16(acc, a[r], t[r]);
                                if (k + kHubDppL < NK) {
#pragma unroll
                                    for (int i = 0; i < 4; ++i) t[r][i] = rt(4 * (k + kHubDppL) + i);
                                    a[r] = rv(k + kHubDppL);
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                    continue;
                }
                // unconditional: sets past nc read stale tile / value words, never used (and the
                // waitcnt pass then sees one issue order on every path into the loop)
                ld(0, tA, aA);
                __builtin_amdgcn_sched_barrier(0);
                ld(1, tB, aB);
                __builtin_amdgcn_sched_barrier(0);
                ld(2, tC, aC);
                __builtin_amdgcn_sched_barrier(0);
                int k = 0;
                // ring of four 8-link sets: every read is issued three sets (24 links) before its
                // fmas, with at most 12 LDS reads outstanding (lgkmcnt counts 15).  The loop's
                // loads are unconditional (k + 6 < nc) and the scheduling barriers keep the ring's
                // order; the last <= 6 sets run after it.
                for (; k + 7 <= nc; k += 4) {
                    ld(k + 3, tD, aD);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tA, aA);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(k + 4, tA, aA);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tB, aB);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(k + 5, tB, aB);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tC, aC);
                    __builtin_amdgcn_sched_barrier(0);
                    ld(k + 6, tC, aC);
                    __builtin_amdgcn_sched_barrier(0);
                    run(tD, aD);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (k < nc) run(tA, aA);
                if (k + 1 < nc) run(tB, aB);
                if (k + 2 < nc) run(tC, aC);
                for (int j = k + 3; j < nc; ++j) {
                    ld(j, tD, aD);
                    run(tD, aD);
                }
                for (int q = nc * 4 * G; q < nb; ++q)
                    acc = __builtin_fmaf(av[q], tcol[(((q >> 2) ^ sw) << 2) + (q & 3)], acc);
            }
        }
        if (cact) {
            if constexpr (EX == kEpiCheby) cheby_epi<1>(epi, row, ccol, acc, cop);
            if (nt)
                __builtin_nontemporal_store(acc, yrow + ccol);
            else
                yrow[ccol] = acc;
            if (epi.agg) epi.agg[(int64_t)row * epi.lda + ccol] = __fadd_rn(aprev, __fmul_rn(epi.w, acc));
            }
        return;
    }

    // ---------------- producers ----------------
    const int p = wave - 1;
    const int g = lane >> 3;          // nonzero within a gather's group of 8
    const int qq = lane & 7;          // 16-byte chunk = columns qq*4 .. qq*4+3 of the slice
    const int qcol = slice * kSliceCols + qq * 4;
    const bool gact = SFULL || qcol < d;
    V4 x0[HubGeom<W>::UW], x1[HubGeom<W>::UW];        // gathered windows, two register sets (even / odd windows)
    float a0[HubGeom<W>::UW], a1[HubGeom<W>::UW];
    int cn[HubGeom<W>::UW];                   // column ids / values of the next window to gather
    float an[HubGeom<W>::UW];
    auto load_ids = [&](int w) {
        const int64_t sb = beg + (int64_t)w * W;
#pragma unroll
        for (int b = 0; b < HubGeom<W>::UW; ++b) {
            int64_t jj = sb + (p * HubGeom<W>::UW + b) * 8 + g;
            jj = jj < end ? jj : end - 1;
            cn[b] = indices[jj];
            an[b] = vals[jj];
        }
    };
    auto gather = [&](V4 (&x)[HubGeom<W>::UW], float (&a)[HubGeom<W>::UW]) {
#pragma unroll
        for (int b = 0; b < HubGeom<W>::UW; ++b) {
            x[b] = gact ? gload<float, 4>(X + (int64_t)cn[b] * ldx + qcol) : vzero<float, 4>();
            a[b] = an[b];
        }
    };
    auto put = [&](int w, const V4 (&x)[HubGeom<W>::UW], const float (&a)[HubGeom<W>::UW]) {
        float* tile = hub_lds + (w & 1) * HubGeom<W>::TILE;
        float* av = aval_base + (w & 1) * W;
#pragma unroll
        for (int b = 0; b < HubGeom<W>::UW; ++b) {
            const int nl = (p * HubGeom<W>::UW + b) * 8 + g;   // nonzero within the window
#pragma unroll
            for (int i = 0; i < 4; ++i) {             // transposed, swizzled: conflict-free
                const int cc = qq * 4 + i;
                tile[cc * HubGeom<W>::LD + ((((nl >> 2) ^ hub_swz(cc)) << 2) | (nl & 3))] = x[b][i];
            }
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
        if (n_win > 1) { load_ids(1); gather(x1, a1); }
        if (n_win > 2) load_ids(2);
        put(0, x0, a0);
        if (n_win > 2) { gather(x0, a0); if (n_win > 3) load_ids(3); }
    }
    __syncthreads();                              // window 0 published
    for (int h = 0; h + 1 < n_win; h += 2) {
        // window h+1 (odd, set 1) -> tile 1 while the consumer runs window h; then gather h+3
        put(h + 1, x1, a1);
        if (h + 3 < n_win) { gather(x1, a1); if (h + 4 < n_win) load_ids(h + 4); }
        __syncthreads();
        if (h + 2 >= n_win) break;
        // window h+2 (even, set 0) -> tile 0 while the consumer runs window h+1; then gather h+4
        put(h + 2, x0, a0);
        if (h + 4 < n_win) { gather(x0, a0); if (h + 5 < n_win) load_ids(h + 5); }
        __syncthreads();
    }
    // barrier count (n_win >= 1): 1 (prologue) + (n_win - 1) in the loop == the consumer's n_win
}

constexpr size_t kHubLdsBytes = HubGeom<kHubW>::LDS_BYTES;

// slice-wave groups of 8 entries in flight.  Round 5, with the packed rows' id staging: for the
// 128- / 256-column packed launches 4 groups take the products hop from 5.26 to 5.22 ms (8 and 6
// measure the same, 2 is 4 % slower, 12 and 16 do not unroll: 9.9 / 11.7 ms; arxiv flat), but the
// RMAT-26 filter bank's 64-column blocks lose 3 % with 4 (1.243 against 1.202 s per step), so the
// 64-column packed launches and the other row paths keep 8 (profiles/r05bf_slice_unroll_ab.txt)
#ifndef SRG_UNROLL_HEAVY
#define SRG_UNROLL_HEAVY 8
#endif
constexpr int kUnrollHeavy = SRG_UNROLL_HEAVY;
constexpr int kUnrollHeavyWide = 4;           // the packed launches with 4 or 2 rows per wave (d = 128 / 256)

// Light rows per wave for wide panels (packed_rows): 512 / d rows, so that every lane holds two
// 16-byte column chunks (d = 64: 8 rows of 8 lanes, d = 128: 4 rows of 16 lanes, d = 256: 2 rows of 32
// lanes; measured best, profiles/r02_ab_d256.txt: 4 rows at d = 256 are 2 % slower than one row per
// wave; d = 32 packed measured even with the narrow path, profiles/r02_ab_d32.txt), 4 gathers per row in
// flight (2 with SRG_SPMM_PACKED_U2; 8 measured slower).  Results are identical for every setting.
constexpr int kPackedU = 4;
constexpr int packed_rows_for(int d) { return d == 64 ? 8 : d == 128 ? 4 : d == 256 ? 2 : 0; }
// LDS a k_spmm block needs (its waves' slice tiles), and what a launch reserves with
// SRG_SPMM_CAP_WAVES: ~160 KiB / (5 + 0.5) per 4-wave block, so at most 5 blocks -- 5 waves per SIMD --
// share a CU (gfx950's 160 KiB LDS; below the 64 KiB default dynamic-LDS limit).  Fewer waves gather
// from fewer rows at once and the L2 re-serves more of their lines: products 6.08 -> 5.96 ms per hop
// and 35.4 -> 31.3 GB of traffic at 5 waves without the slice waves' id prefetch, 5.84 -> 5.81 ms with
// it (whose registers already hold the kernel at 6 waves); 4 and 3 waves lose; arxiv (an 87 MB panel)
// is 3 % faster uncapped, the halo chunks flat (profiles/r04v_*, r04w_*, r04x_*).
constexpr int kSpmmLdsBytes = kWavesPerBlock * kSliceLdsBufs * 256 * (int)sizeof(float);
constexpr int kSpmmCapLdsBytes = (int)((160.0 * 1024.0) / 5.5) / 512 * 512;
static_assert(kSpmmCapLdsBytes > kSpmmLdsBytes && kSpmmCapLdsBytes <= 65536, "k_spmm's capped LDS reservation");
constexpr int spmm_lds_bytes(uint32_t flags) { return (flags & SRG_SPMM_CAP_WAVES) ? kSpmmCapLdsBytes : kSpmmLdsBytes; }

// Raises the dynamic-LDS limit of the hub kernels of epilogue EX on the current device, and the record of
// the devices where that is done (HubLds): launch_spmm<IP, EX> forks through it, so the kernels a
// translation unit instantiates are the ones it registers.
template <int EX>
int hub_attrs()
{
    for (const void* fn : {(const void*)k_spmm_hub<true, int, EX>, (const void*)k_spmm_hub<false, int, EX>,
                           (const void*)k_spmm_hub<true, int64_t, EX>, (const void*)k_spmm_hub<false, int64_t, EX>})
        SRG_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHubLdsBytes));
    for (const void* fn : {(const void*)k_spmm_hub<true, int, EX, kHubWideW>, (const void*)k_spmm_hub<false, int, EX, kHubWideW>,
                           (const void*)k_spmm_hub<true, int64_t, EX, kHubWideW>,
                           (const void*)k_spmm_hub<false, int64_t, EX, kHubWideW>})
        SRG_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HubGeom<kHubWideW>::LDS_BYTES));
    return SRG_OK;
}
template <int EX> HubLds g_hub_lds = {hub_attrs<EX>, {}};

// SRG_SPMM_FAST's hub rows on the fork `hub` (srg_spmm.hip); row_end: the rows' span ends (kEpiSpan)
template <typename IP, int EX>
int launch_fast_hubs(HubFork& hub, const IP* indptr, const int32_t* indices, const float* vals, const int32_t* order,
                     int64_t n_hub, const float* X, int64_t ldx, float* Y, int64_t ldy, int d, uint32_t flags,
                     const int64_t* row_end);

template <typename IP, int EX = kEpiPlain>
int launch_spmm(const IP* indptr, const int32_t* indices, const float* vals, int64_t n_rows,
                const int32_t* order, int64_t n_hub, int64_t n_heavy, const float* X, int64_t ldx,
                float* Y, int64_t ldy, int d, uint32_t flags, hipStream_t s,
                Epi epi = Epi{})
{
    if (n_rows <= 0 || d <= 0) return SRG_OK;
    if (n_hub < 0 || n_heavy < 0 || n_hub + n_heavy > n_rows || ((n_hub + n_heavy) > 0 && !order))
        return srg_fail(SRG_ERR_INVALID, "n_hub=%lld n_heavy=%lld need a row_order and <= n_rows",
                        (long long)n_hub, (long long)n_heavy);
    // slice waves and hub blocks gather 16-byte chunks: they need d % 4 == 0 and aligned rows;
    // otherwise every row takes the row-wave path (same results)
    const bool slice_ok = d % 4 == 0 && ldx % 4 == 0 && aligned(X, 16);
    if (!slice_ok) {
        n_heavy = 0;
        n_hub = 0;
    }
    const int n_slices = (d + kSliceCols - 1) / kSliceCols;
    if ((n_hub + n_heavy) * (int64_t)n_slices > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "too many heavy slices");
    const int acc = (flags & SRG_SPMM_ACCUMULATE) ? 1 : 0;
    const int nt = (flags & SRG_SPMM_NT_STORE) ? 1 : 0;
    const bool sfull = d % kSliceCols == 0;

    HubFork hub(s, g_hub_lds<EX>);
    const bool nojoin = (flags & SRG_SPMM_HUB_NOJOIN) != 0;
    bool fast = false;
    // constexpr: FAST runs its segments through the span kernels, which belong to the translation unit
    // of the plain and span epilogues
    if constexpr (EX == kEpiPlain || EX == kEpiSpan) {
        fast = n_hub > 0 && (flags & SRG_SPMM_FAST) && !epi.agg;
        if (fast)   // fork: the hub rows' segments, then their sums, beside the main launch
            if (int rc = launch_fast_hubs<IP, EX>(hub, indptr, indices, vals, order, n_hub, X, ldx, Y, ldy, d, flags,
                                                  epi.row_end))
                return rc;
    }
    if (n_hub > 0 && !fast) {   // fork: hub blocks run beside the main launch
        // CONTINUE after an unjoined fork: the hub rows are appended to the side stream, which is
        // already ordered after everything they read (the caller's guarantee), with no new fork
        // and no dispatch delay on the caller's stream
        if (int rc = hub.fork((flags & SRG_SPMM_HUB_CONTINUE) != 0)) return rc;
        const dim3 hgrid((unsigned)(n_hub * n_slices));
        // 256-nonzero windows (two workgroups per CU) once a launch has more hub workgroups than CUs
        const bool w256 = n_hub * n_slices > kHubWideLaunch || (flags & SRG_SPMM_HUB_W256);
#define SRG_LAUNCH_HUB(SF, WW)                                                                                      \
    hipLaunchKernelGGL((k_spmm_hub<SF, IP, EX, WW>), hgrid, dim3(kHubThreads), (HubGeom<WW>::LDS_BYTES), hub.stream(), \
                       indptr, indices, vals, order, n_slices, X, ldx, Y, ldy, d, acc, nt, epi)
        if (sfull) {
            if (w256) SRG_LAUNCH_HUB(true, kHubWideW);
            else SRG_LAUNCH_HUB(true, 512);
        } else {
            if (w256) SRG_LAUNCH_HUB(false, kHubWideW);
            else SRG_LAUNCH_HUB(false, 512);
        }
#undef SRG_LAUNCH_HUB
        SRG_HIP_CHECK(hipGetLastError());
        if (int rc = hub.record_join(nojoin)) return rc;
        if (!hub.continued())
            if (int rc = hub.delay()) return rc;
    }

    const int32_t* morder = order ? order + n_hub : nullptr;
    const int64_t m_rows = n_rows - n_hub;
    const int nb_heavy = (int)((n_heavy * n_slices + kWavesPerBlock - 1) / kWavesPerBlock);
    const int64_t n_light = m_rows - n_heavy;
    // light rows: LR rows per wave (packed_rows) when the column tiles line up; else, for d <= 32,
    // 64 / S rows per wave (narrow_rows); else one row per wave
    int lr = 0;
    if (!(flags & SRG_SPMM_WIDE_ROWS)) {
        const int cand = packed_rows_for(d);
        const int S = cand ? 64 / cand : 0;
        const int q = cand ? d / (4 * S) : 0;
        const bool ok = cand && d % (4 * S) == 0 && q == 2 && ldx % 4 == 0 &&
                        ldy % 4 == 0 && aligned(X, 16) && aligned(Y, 16) &&
                        (!epi.agg || (epi.lda % 4 == 0 && aligned(epi.agg, 16))) &&
                        (EX != kEpiCheby || (epi.ldo % 4 == 0 && aligned(epi.cto, 16) && epi.ldr % 4 == 0 &&
                                             epi.r_stride % 4 == 0 && aligned(epi.R, 16)));
        if (ok) lr = cand;
    }
    const int ns = (!lr && d <= 32 && !(flags & SRG_SPMM_WIDE_ROWS)) ? (d <= 1 ? 1 : d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : 32) : 0;
    const int64_t rows_per_block = (int64_t)kWavesPerBlock * (ns ? 64 / ns : lr ? lr : 1);
    // XCD-aware slice waves (k_spmm<..., XH>) with packed light rows, 2 / 4 / 8 slices
    const bool xh = lr && (n_slices == 2 || n_slices == 4 || n_slices == 8);
    int nb_heavy_launch = nb_heavy;
    if (xh) {
        const int64_t per = 8 / n_slices;
        const int64_t bh = ((n_heavy + kWavesPerBlock - 1) / kWavesPerBlock + per - 1) / per * 8;
        if (bh > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "grid too large");
        nb_heavy_launch = (int)bh;
    }
    const int64_t blocks = nb_heavy_launch + (n_light + rows_per_block - 1) / rows_per_block;
    if (blocks > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "grid too large");
    int vec = pick_vec(d, ldx, ldy, X, Y, sizeof(float));
    if (epi.agg) vec = std::min(vec, pick_vec(d, epi.lda, epi.lda, epi.agg, epi.agg, sizeof(float)));
    if (EX == kEpiCheby) {
        vec = std::min(vec, pick_vec(d, epi.ldo, epi.ldr, epi.cto, epi.R, sizeof(float)));
        while (vec > 1 && epi.r_stride % vec) vec /= 2;
    }
    const int nr = (int)m_rows, nh = (int)n_heavy;
    const int pu = (flags & SRG_SPMM_PACKED_U2) ? 2 : kPackedU;
    const unsigned shm = (unsigned)spmm_lds_bytes(flags);
    const int rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        const dim3 grid(nb);
        const int bb = (int)b0;
#define SRG_LAUNCH_SPMM(V, F, SF)                                                               \
    hipLaunchKernelGGL((k_spmm<V, kUnroll, kUnrollHeavy, F, SF, IP, 0, EX>), grid, dim3(kBlock), shm, s,   \
                       indptr, indices, vals, morder, nr, nh, n_slices, nb_heavy, X, ldx, Y, ldy, \
                       d, acc, nt, bb, epi)
        const bool full = d % (64 * vec) == 0;        // implies d % 32 == 0
#define SRG_LAUNCH_NARROW(NSV, SF)                                                                 \
    hipLaunchKernelGGL((k_spmm<1, kUnroll, kUnrollHeavy, false, SF, IP, NSV, EX>), grid, dim3(kBlock), shm, s, \
                       indptr, indices, vals, morder, nr, nh, n_slices, nb_heavy, X, ldx, Y, ldy,     \
                       d, acc, nt, bb, epi)
#define SRG_LAUNCH_PACKED(LRV, LQV, UV)                                                              \
    do {                                                                                              \
        if (xh)                                                                                       \
            hipLaunchKernelGGL((k_spmm<1, UV, (LRV < 8 ? kUnrollHeavyWide : kUnrollHeavy), false, true, IP, 0, EX, LRV, LQV, true>), grid, dim3(kBlock), \
                               shm, s, indptr, indices, vals, morder, nr, nh, n_slices, nb_heavy_launch, X, ldx, Y, ldy, \
                               d, acc, nt, bb, epi);                                                  \
        else                                                                                          \
            hipLaunchKernelGGL((k_spmm<1, UV, (LRV < 8 ? kUnrollHeavyWide : kUnrollHeavy), false, true, IP, 0, EX, LRV, LQV>), grid, dim3(kBlock), shm, s, \
                               indptr, indices, vals, morder, nr, nh, n_slices, nb_heavy, X, ldx, Y, ldy, \
                               d, acc, nt, bb, epi);                                                  \
    } while (0)
#define SRG_LAUNCH_PACKED_U(LRV, LQV)                                                                 \
    do {                                                                                              \
        if (pu == 2) SRG_LAUNCH_PACKED(LRV, LQV, 2);                                                  \
        else SRG_LAUNCH_PACKED(LRV, LQV, 4);                                                          \
    } while (0)
        // packed_rows_for gives two 16-byte chunks per lane (LQ = 2) at d = 64 / 128 / 256
        if (lr == 2) {
            SRG_LAUNCH_PACKED_U(2, 2);
        } else if (lr == 4) {
            SRG_LAUNCH_PACKED_U(4, 2);
        } else if (lr == 8) {
            SRG_LAUNCH_PACKED_U(8, 2);
        } else if (ns == 32) {
            if (sfull) SRG_LAUNCH_NARROW(32, true);
            else SRG_LAUNCH_NARROW(32, false);
        } else if (ns == 16) {
            SRG_LAUNCH_NARROW(16, false);
        } else if (ns == 8) {
            SRG_LAUNCH_NARROW(8, false);
        } else if (ns == 4) {
            SRG_LAUNCH_NARROW(4, false);
        } else if (ns == 2) {
            SRG_LAUNCH_NARROW(2, false);
        } else if (ns == 1) {
            SRG_LAUNCH_NARROW(1, false);
        } else if (vec == 4) {
            if (full) SRG_LAUNCH_SPMM(4, true, true);
            else if (sfull) SRG_LAUNCH_SPMM(4, false, true);
            else SRG_LAUNCH_SPMM(4, false, false);
        } else if (vec == 2) {
            if (full) SRG_LAUNCH_SPMM(2, true, true);
            else if (sfull) SRG_LAUNCH_SPMM(2, false, true);
            else SRG_LAUNCH_SPMM(2, false, false);
        } else {
            if (full) SRG_LAUNCH_SPMM(1, true, true);
            else if (sfull) SRG_LAUNCH_SPMM(1, false, true);
            else SRG_LAUNCH_SPMM(1, false, false);
        }
#undef SRG_LAUNCH_SPMM
#undef SRG_LAUNCH_NARROW
#undef SRG_LAUNCH_PACKED
#undef SRG_LAUNCH_PACKED_U
        return launch_status();
    });
    if (rc) return rc;
    return nojoin ? SRG_OK : hub.join();
}

}  // namespace

#endif  // SRG_SPMM_KERNELS_H_
