// srg_gat.hip -- the aggregation of a graph attention layer (GATConv; srgnn.gat): a sparse
// product whose values are computed per entry and per head and differentiated through.  A is a CSR over
// targets (row i holds the sources j of its incoming edges), Hf [n_src, H*C] the transformed features with
// the heads side by side, a_src [n_src, H] and a_dst [n_rows, H] the two halves of the score.
//
// Forward (srg_gat_attend_f32), per row i and head h over the row's entries e with source j_e:
//   s_e = a_src[j_e,h] + a_dst[i,h];  l_e = s_e > 0 ? s_e : slope * s_e;  m = max_e l_e;  p_e = expf(l_e - m)
//   z = sum_e p_e;  acc[c] = fmaf(p_e, Hf[j_e, h*C+c], acc[c]);  out[i, h*C+c] = acc[c] / z
// Backward (srg_gat_edge_grad_f32 over A, srg_gat_attend_adjoint_f32 over At and perm), with G = dL/dout and
// alpha_e = expf(l_e - M[i,h]) / Z[i,h] recomputed, never stored:
//   D[i,h] = sum_c G[i,h*C+c] out[i,h*C+c];  dalpha_e = sum_c G[i,h*C+c] Hf[j_e,h*C+c]
//   ds_e = (alpha_e * (dalpha_e - D[i,h])) * (s_e > 0 ? 1 : slope)
//   da_dst[i,h] = sum over row i of A of ds;  da_src[j,h] = sum over row j of At of ds[perm[t]]
//   dHf[j,h*C+c] = chain fmaf(alpha_t, G[i_t,h*C+c], .) over row j of At
//
// The order of every sum (none depends on H, on the load path, on the launch or on any other row):
//   * out's and dHf's chains: one fmaf chain per element from +0.0f over the row's entries in stored order
//     (A's for out, At's for dHf); an entry whose id is out of range is skipped, not folded in as 0 * x.
//   * m: a maximum (no rounding; a NaN score makes it NaN).
//   * z, da_dst, da_src (row sums of length L): lane l of 64 adds the terms at positions l, l + 64, l + 128, ...
//     of the row in that order from +0.0f; then the halving tree  p_l = p_l + p_{l+w}  for l < w,
//     w = 32, 16, 8, 4, 2, 1; the sum is p_0.  A function of the position in the row alone: a skipped entry
//     leaves its position out and moves no other term.
//   * D and dalpha (sums over a head's C columns): one fmaf chain from +0.0f, columns ascending.
//   * ds: the three products and the difference above, each rounded once, left to right as written.
// Nothing is contracted (the library is built with -ffp-contract=off; every fma here is written as one), the
// divides are IEEE correctly rounded, expf is the device library's (1 ulp).  No atomics, no allocation, no
// synchronisation: every result is run-to-run identical.
//
// Mapping.  srg_gat_attend_f32 is the row gather of the graph convolution (srg_gconv.hip): a wave owns one row
// and a tile of 64 * VEC consecutive columns of the H*C wide row (VEC 4: 16-byte loads, needs C % 4 == 0 so
// that a lane's four columns share a head; VEC 1: 4-byte loads; the same chain either way).  A lane takes its
// head from its column, reads that head's m and z once and a_src[j_e, h] per entry, and evaluates p_e itself:
// the lanes of one head compute the same expf from the same operands, so a tile may span several heads, or
// a head several tiles, without any exchange between lanes.  m and z come from a stats kernel that runs
// first (one wave per row, the lanes across the row's entries, the heads one after the other).
// srg_gat_attend_adjoint_f32 is the same gather over At with three [n, H] gathers (a_dst, M, Z) per entry.
// srg_gat_edge_grad_f32 lays a row's (entry, head) pairs over the lanes of its wave, each lane running the
// C-column chain of its pair (16-byte loads when C, the strides and the bases allow; the same order).
//
// The batch path (srg_gat_attend_rows_f32, srg_gat_edge_grad_rows_f32, srg_gat_attend_rows_adjoint_f32) is
// the same arithmetic in the same orders for the rows of a batch only: wave b of the stats, gather and edge
// kernels works on row rows[b] of A (a_dst is the full table, read at the row's id) and writes compact row b
// of out, M, Z, and the row's entries at eptr[b] .. of the compact dS.  Over At the batch is the position
// table pos: an entry whose target is no member (pos outside [0, B)) is skipped like an id out of range,
// in dHf's chain and in da_src's row sum, where it leaves its position out.  On finite operands every result
// has the bits the full path gives for G zero outside the batch.
//
// Cost of a long row: a row is one wave's serial work in every kernel here.  A row of L entries costs
// 2 H ceil(L / 64) score rounds in the stats kernel, L / 8 gather rounds (8 rows in flight) per column tile in
// the two gathers, and ceil(L H / 64) C-column chains in the edge kernel, whatever the other waves do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

constexpr int64_t kRowsPerLaunch = SRG_GAT_LAUNCH_ROWS;                    // rows (waves) of one launch
constexpr int64_t kBlocksPerLaunch = kRowsPerLaunch / kWavesPerBlock;
static_assert(kRowsPerLaunch % kBlock == 0 && kBlocksPerLaunch <= kMaxLaunchBlocks,
              "a launch's rows, or (row, head) items, fill whole workgroups and fit one grid");

__device__ __forceinline__ float leaky(float s, float slope) { return s > 0.0f ? s : __fmul_rn(slope, s); }

// p_0 of the halving tree in every lane (the adds commute, so every lane holds lane 0's bits)
__device__ __forceinline__ float wave_tree_sum(float p)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) p = __fadd_rn(p, __shfl_xor(p, w, 64));
    return p;
}

// the larger of two scores; a NaN wins
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// The row map of the stats, gather and edge kernels: wave slot b works on row `row` of A and writes compact
// row b.  The full path is the identity; the batch path reads rows[b], and an id outside [0, n_rows) gives
// -1 and is never an address.
template <bool ROWS>
__device__ __forceinline__ int mapped_row(int slot, const int64_t* __restrict__ rows, int64_t n_rows)
{
    if constexpr (!ROWS) {
        return slot;
    } else {
        const int64_t r = rows[slot];
        return r >= 0 && r < n_rows ? __builtin_amdgcn_readfirstlane((int)r) : -1;
    }
}

// M[i,h] and Z[i,h]: one wave per row, the lanes across its entries, the heads in turn.  A row without a
// valid entry, or a batch row whose id is out of range, gets M = 0, Z = 0.
template <bool ROWS>
__global__ void __launch_bounds__(kBlock)
k_gat_stats(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_src,
            const int64_t* __restrict__ rows, int64_t B, const float* __restrict__ a_src,
            const float* __restrict__ a_dst, float slope, int H, float* __restrict__ M, float* __restrict__ Z,
            int block_base)
{
    const int slot = wave_slot(block_base);
    if (slot >= (ROWS ? B : n_rows)) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int row = mapped_row<ROWS>(slot, rows, n_rows);
    if (ROWS && row < 0) {
        for (int h = lane; h < H; h += 64) M[(int64_t)slot * H + h] = 0.0f, Z[(int64_t)slot * H + h] = 0.0f;
        return;
    }
    const int64_t beg = indptr[row], end = indptr[row + 1];
    for (int h = 0; h < H; ++h) {
        const float ad = a_dst[(int64_t)row * H + h];
        float m = -INFINITY;
        bool seen = false;
        for (int64_t j = beg + lane; j < end; j += 64) {
            const int c = indices[j];
            if (c >= 0 && c < n_src) {
                m = nan_max(m, leaky(__fadd_rn(a_src[(int64_t)c * H + h], ad), slope));
                seen = true;
            }
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) m = nan_max(m, __shfl_xor(m, w, 64));
        float z = 0.0f;
        if (__any(seen)) {
            for (int64_t j = beg + lane; j < end; j += 64) {
                const int c = indices[j];
                if (c >= 0 && c < n_src)
                    z = __fadd_rn(z, expf(__fsub_rn(leaky(__fadd_rn(a_src[(int64_t)c * H + h], ad), slope), m)));
            }
            z = wave_tree_sum(z);
        } else {
            m = 0.0f;
        }
        if (lane == 0) {
            M[(int64_t)slot * H + h] = m;
            Z[(int64_t)slot * H + h] = z;
        }
    }
}

// a lane's verdict on its entry in both gathers: the id, kept when it is in range (so never an address otherwise)
struct KeptId {
    bool kept;
    int id;
};

// out[row, col ..]: the chain over the row's valid entries in stored order, divided by z: the filtered row
// walk (srg_device.h).  keep: the source id, kept when it lies in [0, n_src); fetch: that source's row of Hf
// and its a_src; fold: p_e and the chain link.
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(kBlock)
k_gat_attend(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_src,
             const int64_t* __restrict__ rows, int64_t B, const float* __restrict__ a_src,
             const float* __restrict__ a_dst, float slope, const float* __restrict__ Hf, int64_t ldh, int H, int C,
             const float* __restrict__ M, const float* __restrict__ Z, float* __restrict__ out, int64_t ldo,
             int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int slot = wave_slot(block_base);
    if (slot >= (ROWS ? B : n_rows)) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int col = ((int)blockIdx.y * 64 + lane) * VEC;
    const bool act = col < H * C;
    const int h = act ? col / C : 0;
    const int row = mapped_row<ROWS>(slot, rows, n_rows);
    if (ROWS && row < 0) {   // a batch id out of range: a row of +0
        if (act) vstore<float, VEC>(out + (int64_t)slot * ldo + col, vzero<float, VEC>(), false);
        return;
    }
    const float ad = a_dst[(int64_t)row * H + h];
    const float m = M[(int64_t)slot * H + h], z = Z[(int64_t)slot * H + h];
    V acc = vzero<float, VEC>();
    struct Slot { V x; float as; };
    row_walk_kept<Slot, kUnroll>(
        indices, indptr[row], indptr[row + 1],
        [&](int id, int64_t) { return KeptId{id >= 0 && id < n_src, id}; },
        [&](const KeptId& mine, int q) {
            const int c = __builtin_amdgcn_readlane(mine.id, q);
            if (!act) return Slot{vzero<float, VEC>(), 0.0f};
            return Slot{gload<float, VEC>(Hf + (int64_t)c * ldh + col), a_src[(int64_t)c * H + h]};
        },
        [&](const Slot& s) {
            const float p = expf(__fsub_rn(leaky(__fadd_rn(s.as, ad), slope), m));
            chain<float, VEC>(acc, p, s.x);
        });
    if (act) {
        V o;
        if constexpr (VEC == 1) {
            o = z == 0.0f ? 0.0f : __fdiv_rn(acc, z);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) o[i] = z == 0.0f ? 0.0f : __fdiv_rn(acc[i], z);
        }
        vstore<float, VEC>(out + (int64_t)slot * ldo + col, o, false);
    }
}

// dHf[row, col ..] over row `row` of At: the chain of alpha_t * G[i_t, col ..] over the valid entries in
// stored order, alpha_t recomputed from the target's a_dst, M and Z: the filtered row walk again.  keep: the
// target id, kept when it lies in [0, n_rows); fetch: that target's row of G, a_dst, M and Z; fold: alpha_t
// and the chain link.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_gat_adjoint(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_src,
              const float* __restrict__ a_src, const float* __restrict__ a_dst, float slope, int H, int C,
              const float* __restrict__ M, const float* __restrict__ Z, const float* __restrict__ G, int64_t ldg,
              float* __restrict__ dHf, int64_t ldd, int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int row = wave_slot(block_base);
    if (row >= n_src) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int col = ((int)blockIdx.y * 64 + lane) * VEC;
    const bool act = col < H * C;
    const int h = act ? col / C : 0;
    const float as = a_src[(int64_t)row * H + h];
    V acc = vzero<float, VEC>();
    struct Slot { V x; float ad, m, z; };
    row_walk_kept<Slot, kUnroll>(
        indices, indptr[row], indptr[row + 1],
        [&](int id, int64_t) { return KeptId{id >= 0 && id < n_rows, id}; },
        [&](const KeptId& mine, int q) {
            const int i = __builtin_amdgcn_readlane(mine.id, q);
            const int64_t ih = (int64_t)i * H + h;
            if (!act) return Slot{vzero<float, VEC>(), 0.0f, 0.0f, 1.0f};
            return Slot{gload<float, VEC>(G + (int64_t)i * ldg + col), a_dst[ih], M[ih], Z[ih]};
        },
        [&](const Slot& s) {
            const float p = expf(__fsub_rn(leaky(__fadd_rn(as, s.ad), slope), s.m));
            // Z == 0 marks a target without a valid entry (a forged id of At): it contributes nothing
            if (s.z != 0.0f) chain<float, VEC>(acc, __fdiv_rn(p, s.z), s.x);
        });
    if (act) vstore<float, VEC>(dHf + (int64_t)row * ldd + col, acc, false);
}

// dHf[row, col ..] of the batch path: the same chain over the member entries of row `row` of At only.  keep:
// the target id i, kept when it lies in [0, n_rows) and its position b = pos[i] (read after that check) in
// [0, B); fetch: row b of the compact G, M and Z, and the target's a_dst at its id; fold: as above.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_gat_adjoint_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
                   int64_t n_src, const int32_t* __restrict__ pos, int64_t B, const float* __restrict__ a_src,
                   const float* __restrict__ a_dst, float slope, int H, int C, const float* __restrict__ M,
                   const float* __restrict__ Z, const float* __restrict__ G, int64_t ldg, float* __restrict__ dHf,
                   int64_t ldd, int block_base)
{
    typedef typename Vec<float, VEC>::type V;
    const int row = wave_slot(block_base);
    if (row >= n_src) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int col = ((int)blockIdx.y * 64 + lane) * VEC;
    const bool act = col < H * C;
    const int h = act ? col / C : 0;
    const float as = a_src[(int64_t)row * H + h];
    V acc = vzero<float, VEC>();
    struct Member { bool kept; int id, p; };
    struct Slot { V x; float ad, m, z; };
    row_walk_kept<Slot, kUnroll>(
        indices, indptr[row], indptr[row + 1],
        [&](int id, int64_t) {
            int p = -1;
            if (id >= 0 && id < n_rows) p = pos[id];
            return Member{p >= 0 && p < B, id, p};
        },
        [&](const Member& mine, int q) {
            // (the position first: its readlane waits for the lane's load of pos[id], which must not come to
            // stand behind a gather that is already in flight)
            const int b = __builtin_amdgcn_readlane(mine.p, q);
            const int i = __builtin_amdgcn_readlane(mine.id, q);
            const int64_t bh = (int64_t)b * H + h;
            if (!act) return Slot{vzero<float, VEC>(), 0.0f, 0.0f, 1.0f};
            return Slot{gload<float, VEC>(G + (int64_t)b * ldg + col), a_dst[(int64_t)i * H + h], M[bh], Z[bh]};
        },
        [&](const Slot& s) {
            const float p = expf(__fsub_rn(leaky(__fadd_rn(as, s.ad), slope), s.m));
            if (s.z != 0.0f) chain<float, VEC>(acc, __fdiv_rn(p, s.z), s.x);   // Z == 0: an empty batch row
        });
    if (act) vstore<float, VEC>(dHf + (int64_t)row * ldd + col, acc, false);
}

// the C-column chain fmaf(a[c], b[c], .) from +0, columns ascending; V4: 16-byte loads, the same order
template <bool V4>
__device__ __forceinline__ float col_chain(const float* __restrict__ a, const float* __restrict__ b, int C)
{
    float acc = 0.0f;
    if constexpr (V4) {
        typedef typename Vec<float, 4>::type V;
        for (int c = 0; c < C; c += 4) {
            const V x = vload<float, 4>(a + c), y = vload<float, 4>(b + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_fmaf(x[i], y[i], acc);
        }
    } else {
        for (int c = 0; c < C; ++c) acc = __builtin_fmaf(a[c], b[c], acc);
    }
    return acc;
}

// D[i,h] = chain over c of G[i,h*C+c] * out[i,h*C+c]: one thread per (row, head)
template <bool V4>
__global__ void __launch_bounds__(kBlock)
k_gat_rowdot(int64_t total, int H, int C, const float* __restrict__ G, int64_t ldg, const float* __restrict__ O,
             int64_t ldo, float* __restrict__ D, int64_t base)
{
    const int64_t idx = base + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= total) return;
    const int64_t i = idx / H;
    const int h = (int)(idx - i * H);
    D[idx] = col_chain<V4>(G + i * ldg + (int64_t)h * C, O + i * ldo + (int64_t)h * C, C);
}

// The batch path: M, Z, G and D are compact (row b of the batch), dS holds nnz_out = nnzB entries and the
// row's entry k is written at eptr[b] + k while that lies below eptr[b + 1] and nnzB.
template <bool V4, bool ROWS>
__global__ void __launch_bounds__(kBlock)
k_gat_edge(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_src,
           int64_t nnz_out, const int64_t* __restrict__ rows, int64_t B, const int64_t* __restrict__ eptr,
           const float* __restrict__ a_src, const float* __restrict__ a_dst, float slope,
           const float* __restrict__ Hf, int64_t ldh, int H, int C, const float* __restrict__ M,
           const float* __restrict__ Z, const float* __restrict__ G, int64_t ldg, const float* __restrict__ D,
           float* __restrict__ dS, int block_base)
{
    const int slot = wave_slot(block_base);
    if (slot >= (ROWS ? B : n_rows)) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int row = mapped_row<ROWS>(slot, rows, n_rows);
    if (ROWS && row < 0) return;
    const int64_t beg = indptr[row];
    int64_t end = indptr[row + 1];
    int64_t obeg = beg;                    // where the row's first entry goes in dS
    if constexpr (ROWS) {
        obeg = eptr[slot];
        if (obeg < 0) return;
        int64_t oend = eptr[slot + 1];
        oend = oend < nnz_out ? oend : nnz_out;   // dS holds nnzB entries
        end = end - beg < oend - obeg ? end : beg + (oend - obeg);
    } else {
        end = end < nnz_out ? end : nnz_out;      // dS holds nnz entries
    }
    const int64_t pairs = (end - beg) * H;
    for (int64_t q = lane; q < pairs; q += 64) {
        const int64_t k = q / H;
        const int64_t e = beg + k;
        const int h = (int)(q % H);
        const int c = indices[e];
        float ds = 0.0f;
        const int64_t rh = (int64_t)slot * H + h;
        if (c >= 0 && c < n_src && Z[rh] != 0.0f) {   // Z == 0: M and Z are not this row's statistics
            const float s = __fadd_rn(a_src[(int64_t)c * H + h], a_dst[(int64_t)row * H + h]);
            const float alpha = __fdiv_rn(expf(__fsub_rn(leaky(s, slope), M[rh])), Z[rh]);
            const float da = col_chain<V4>(G + (int64_t)slot * ldg + (int64_t)h * C, Hf + (int64_t)c * ldh + (int64_t)h * C, C);
            ds = __fmul_rn(__fmul_rn(alpha, __fsub_rn(da, D[rh])), s > 0.0f ? 1.0f : slope);
        }
        dS[(obeg + k) * H + h] = ds;
    }
}

// out[r,h] = the row sum of dS[entry, h] over row r (entry j itself, or perm[j]): the lanes across the
// row's entries, the heads in turn; the order of the file header.
__global__ void __launch_bounds__(kBlock)
k_gat_rowsum(const int64_t* __restrict__ indptr, const int64_t* __restrict__ perm, int64_t n, int64_t nnz, int H,
             const float* __restrict__ dS, float* __restrict__ out, int block_base)
{
    const int row = wave_slot(block_base);
    if (row >= n) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int64_t beg = indptr[row], end = indptr[row + 1];
    for (int h = 0; h < H; ++h) {
        float acc = 0.0f;
        for (int64_t j = beg + lane; j < end; j += 64) {
            const int64_t e = perm ? perm[j] : j;
            if (e >= 0 && e < nnz) acc = __fadd_rn(acc, dS[e * H + h]);
        }
        acc = wave_tree_sum(acc);
        if (lane == 0) out[(int64_t)row * H + h] = acc;
    }
}

// da_src[r,h] of the batch path: the same row sum over row r of At with dS compact.  Entry t with target
// i = indices_t[t] is a term when i is in range, b = pos[i] is a member's position and the entry's place
// eptr[b] + (perm[t] - indptr[i]) lies in [eptr[b], eptr[b + 1]) and below nnzB; every other entry leaves
// its position out.  Each of i, b and perm[t] is range-checked before it is an address or an offset.  The
// heads go four at a time, so that an entry's place is worked out once for four of them.
__global__ void __launch_bounds__(kBlock)
k_gat_rowsum_rows(const int64_t* __restrict__ indptr_t, const int32_t* __restrict__ indices_t,
                  const int64_t* __restrict__ perm, int64_t n_src, int64_t n_rows, int64_t nnz,
                  const int32_t* __restrict__ pos, int64_t B, const int64_t* __restrict__ indptr,
                  const int64_t* __restrict__ eptr, int64_t nnzB, int H, const float* __restrict__ dS,
                  float* __restrict__ out, int block_base)
{
    const int row = wave_slot(block_base);
    if (row >= n_src) return;   // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int64_t beg = indptr_t[row], end = indptr_t[row + 1];
    for (int h0 = 0; h0 < H; h0 += 4) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t j = beg + lane; j < end; j += 64) {
            const int i = indices_t[j];
            if (i < 0 || i >= n_rows) continue;
            const int b = pos[i];
            if (b < 0 || b >= B) continue;
            const int64_t e = perm[j];
            if (e < 0 || e >= nnz) continue;
            const int64_t k = e - indptr[i], lo = eptr[b], hi = eptr[b + 1];
            const int64_t c = lo + k;
            if (k < 0 || lo < 0 || c >= hi || c >= nnzB) continue;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (h0 + u < H) acc[u] = __fadd_rn(acc[u], dS[c * H + h0 + u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float sum = wave_tree_sum(acc[u]);
            if (lane == 0 && h0 + u < H) out[(int64_t)row * H + h0 + u] = sum;
        }
    }
}

int check_shape(int64_t n_rows, int64_t n_src, int64_t nnz, int H, int C)
{
    if (n_rows < 0 || n_rows > INT32_MAX - 64 || n_src < 0 || n_src > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "n_rows=%lld, n_src=%lld out of range [0, 2^31-64)", (long long)n_rows,
                        (long long)n_src);
    if (nnz < 0) return srg_fail(SRG_ERR_INVALID, "nnz=%lld < 0", (long long)nnz);
    if (H < 1 || H > SRG_GAT_MAX_HEADS)
        return srg_fail(SRG_ERR_INVALID, "H=%d out of range [1, %d]", H, SRG_GAT_MAX_HEADS);
    if (C < 1 || (int64_t)H * C > SRG_GAT_MAX_WIDTH)
        return srg_fail(SRG_ERR_INVALID, "C=%d: H*C must lie in [H, %d]", C, SRG_GAT_MAX_WIDTH);
    return SRG_OK;
}

int check_ld(const char* name, int64_t ld, int W)
{
    if (ld < W) return srg_fail(SRG_ERR_INVALID, "leading dimension %s=%lld < H*C=%d", name, (long long)ld, W);
    return SRG_OK;
}

int check_batch(int64_t B, int64_t nnzB)
{
    if (B < 0 || B > INT32_MAX - 64)
        return srg_fail(SRG_ERR_INVALID, "B=%lld out of range [0, 2^31-64)", (long long)B);
    if (nnzB < 0) return srg_fail(SRG_ERR_INVALID, "nnzB=%lld < 0", (long long)nnzB);
    return SRG_OK;
}

// The stats and the gather over `count` wave slots: the rows of A (ROWS false: rows and B unused), or the rows
// of a batch.
template <bool ROWS>
int launch_attend(hipStream_t s, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_src,
                  const int64_t* rows, int64_t B, const float* a_src, const float* a_dst, float slope,
                  const float* Hf, int64_t ldh, int H, int C, float* out, int64_t ldo, float* M, float* Z)
{
    const int W = H * C;
    const bool v4 = rows_aligned(4, sizeof(float), C, {{Hf, ldh}, {out, ldo}});
    const int tile = v4 ? 256 : 64;
    const unsigned tiles = (unsigned)((W + tile - 1) / tile);
    const int64_t blocks = ((ROWS ? B : n_rows) + kWavesPerBlock - 1) / kWavesPerBlock;
    int rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_gat_stats<ROWS>, dim3(nb), dim3(kBlock), 0, s, indptr, indices, n_rows, n_src, rows, B,
                           a_src, a_dst, slope, H, M, Z, (int)b0);
        return launch_status();
    });
    if (rc) return rc;
    return launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
        if (v4)
            hipLaunchKernelGGL((k_gat_attend<4, ROWS>), dim3(nb, tiles), dim3(kBlock), 0, s, indptr, indices, n_rows,
                               n_src, rows, B, a_src, a_dst, slope, Hf, ldh, H, C, M, Z, out, ldo, (int)b0);
        else
            hipLaunchKernelGGL((k_gat_attend<1, ROWS>), dim3(nb, tiles), dim3(kBlock), 0, s, indptr, indices, n_rows,
                               n_src, rows, B, a_src, a_dst, slope, Hf, ldh, H, C, M, Z, out, ldo, (int)b0);
        return launch_status();
    });
}

// D, dS and da_dst over `count` wave slots.  ROWS false: dS holds nnz_out = nnz entries and da_dst sums over
// indptr; ROWS true: out, M, Z, G, D and da_dst are the batch's compact panels, dS holds nnz_out = nnzB
// entries and da_dst sums over eptr.
template <bool ROWS>
int launch_edge_grad(hipStream_t s, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_src,
                     int64_t nnz_out, const int64_t* rows, int64_t B, const int64_t* eptr, const float* a_src,
                     const float* a_dst, float slope, const float* Hf, int64_t ldh, int H, int C, const float* out,
                     int64_t ldo, const float* M, const float* Z, const float* G, int64_t ldg, float* D, float* dS,
                     float* da_dst)
{
    const int64_t count = ROWS ? B : n_rows;
    const int64_t total = count * H;   // one thread per item: kRowsPerLaunch items are whole blocks
    const bool v4d = rows_aligned(4, sizeof(float), C, {{G, ldg}, {out, ldo}});
    int rc = launch_chunks_capped((total + kBlock - 1) / kBlock, kRowsPerLaunch / kBlock, [&](int64_t b0, unsigned nb) {
        if (v4d)
            hipLaunchKernelGGL(k_gat_rowdot<true>, dim3(nb), dim3(kBlock), 0, s, total, H, C, G, ldg, out, ldo, D,
                               b0 * kBlock);
        else
            hipLaunchKernelGGL(k_gat_rowdot<false>, dim3(nb), dim3(kBlock), 0, s, total, H, C, G, ldg, out, ldo, D,
                               b0 * kBlock);
        return launch_status();
    });
    if (rc) return rc;
    const bool v4e = rows_aligned(4, sizeof(float), C, {{G, ldg}, {Hf, ldh}});
    const int64_t blocks = (count + kWavesPerBlock - 1) / kWavesPerBlock;
    rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
        if (v4e)
            hipLaunchKernelGGL((k_gat_edge<true, ROWS>), dim3(nb), dim3(kBlock), 0, s, indptr, indices, n_rows, n_src,
                               nnz_out, rows, B, eptr, a_src, a_dst, slope, Hf, ldh, H, C, M, Z, G, ldg, D, dS, (int)b0);
        else
            hipLaunchKernelGGL((k_gat_edge<false, ROWS>), dim3(nb), dim3(kBlock), 0, s, indptr, indices, n_rows, n_src,
                               nnz_out, rows, B, eptr, a_src, a_dst, slope, Hf, ldh, H, C, M, Z, G, ldg, D, dS, (int)b0);
        return launch_status();
    });
    if (rc) return rc;
    return launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_gat_rowsum, dim3(nb), dim3(kBlock), 0, s, ROWS ? eptr : indptr, (const int64_t*)nullptr,
                           count, nnz_out, H, dS, da_dst, (int)b0);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int srg_gat_attend_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                       const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh, int32_t H,
                       int32_t C, float* out, int64_t ldo, float* M, float* Z, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc) return rc;
    const int W = H * C;
    if ((rc = check_ld("ldh", ldh, W)) || (rc = check_ld("ldo", ldo, W))) return rc;
    if (n_rows == 0) return srg_ok();
    if (!out || !M || !Z) return srg_fail(SRG_ERR_INVALID, "null out, M or Z");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_src == 0) {   // every row is empty: out = +0, M = 0, Z = 0
        SRG_HIP_CHECK(hipMemset2DAsync(out, (size_t)ldo * sizeof(float), 0, (size_t)W * sizeof(float), (size_t)n_rows, s));
        SRG_HIP_CHECK(hipMemsetAsync(M, 0, (size_t)n_rows * H * sizeof(float), s));
        SRG_HIP_CHECK(hipMemsetAsync(Z, 0, (size_t)n_rows * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr || !indices || !a_src || !a_dst || !Hf)
        return srg_fail(SRG_ERR_INVALID, "null indptr, indices, a_src, a_dst or Hf");
    rc = launch_attend<false>(s, indptr, indices, n_rows, n_src, nullptr, 0, a_src, a_dst, slope, Hf, ldh, H, C, out,
                              ldo, M, Z);
    return rc ? rc : srg_ok();
}

int srg_gat_attend_rows_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                            const int64_t* rows, int64_t B, const float* a_src, const float* a_dst, float slope,
                            const float* Hf, int64_t ldh, int32_t H, int32_t C, float* out, int64_t ldo, float* M,
                            float* Z, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc || (rc = check_batch(B, 0))) return rc;
    const int W = H * C;
    if ((rc = check_ld("ldh", ldh, W)) || (rc = check_ld("ldo", ldo, W))) return rc;
    if (B == 0) return srg_ok();
    if (!out || !M || !Z) return srg_fail(SRG_ERR_INVALID, "null out, M or Z");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_src == 0 || n_rows == 0) {   // every row is empty: out = +0, M = 0, Z = 0
        SRG_HIP_CHECK(hipMemset2DAsync(out, (size_t)ldo * sizeof(float), 0, (size_t)W * sizeof(float), (size_t)B, s));
        SRG_HIP_CHECK(hipMemsetAsync(M, 0, (size_t)B * H * sizeof(float), s));
        SRG_HIP_CHECK(hipMemsetAsync(Z, 0, (size_t)B * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr || !indices || !rows || !a_src || !a_dst || !Hf)
        return srg_fail(SRG_ERR_INVALID, "null indptr, indices, rows, a_src, a_dst or Hf");
    rc = launch_attend<true>(s, indptr, indices, n_rows, n_src, rows, B, a_src, a_dst, slope, Hf, ldh, H, C, out, ldo,
                             M, Z);
    return rc ? rc : srg_ok();
}

int srg_gat_edge_grad_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows, int64_t n_src,
                          const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh,
                          int32_t H, int32_t C, const float* out, int64_t ldo, const float* M, const float* Z,
                          const float* G, int64_t ldg, float* D, float* dS, float* da_dst, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc) return rc;
    const int W = H * C;
    if ((rc = check_ld("ldh", ldh, W)) || (rc = check_ld("ldo", ldo, W)) || (rc = check_ld("ldg", ldg, W))) return rc;
    if (n_rows == 0) return srg_ok();
    if (!da_dst) return srg_fail(SRG_ERR_INVALID, "null da_dst");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_src == 0) {
        SRG_HIP_CHECK(hipMemsetAsync(da_dst, 0, (size_t)n_rows * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr || !indices || !a_src || !a_dst || !Hf || !out || !M || !Z || !G || !D || !dS)
        return srg_fail(SRG_ERR_INVALID, "null operand");
    rc = launch_edge_grad<false>(s, indptr, indices, n_rows, n_src, nnz, nullptr, 0, nullptr, a_src, a_dst, slope, Hf,
                                 ldh, H, C, out, ldo, M, Z, G, ldg, D, dS, da_dst);
    return rc ? rc : srg_ok();
}

int srg_gat_edge_grad_rows_f32(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows,
                               int64_t n_src, const int64_t* rows, int64_t B, const int64_t* eptr, int64_t nnzB,
                               const float* a_src, const float* a_dst, float slope, const float* Hf, int64_t ldh,
                               int32_t H, int32_t C, const float* out, int64_t ldo, const float* M, const float* Z,
                               const float* G, int64_t ldg, float* D, float* dS, float* da_dst, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc || (rc = check_batch(B, nnzB))) return rc;
    const int W = H * C;
    if ((rc = check_ld("ldh", ldh, W)) || (rc = check_ld("ldo", ldo, W)) || (rc = check_ld("ldg", ldg, W))) return rc;
    if (B == 0) return srg_ok();
    if (!da_dst) return srg_fail(SRG_ERR_INVALID, "null da_dst");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_src == 0 || n_rows == 0) {
        SRG_HIP_CHECK(hipMemsetAsync(da_dst, 0, (size_t)B * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr || !indices || !rows || !eptr || !a_src || !a_dst || !Hf || !out || !M || !Z || !G || !D ||
        (nnzB > 0 && !dS))
        return srg_fail(SRG_ERR_INVALID, "null operand");
    rc = launch_edge_grad<true>(s, indptr, indices, n_rows, n_src, nnzB, rows, B, eptr, a_src, a_dst, slope, Hf, ldh,
                                H, C, out, ldo, M, Z, G, ldg, D, dS, da_dst);
    return rc ? rc : srg_ok();
}

int srg_gat_attend_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const int64_t* perm, int64_t nnz,
                               int64_t n_rows, int64_t n_src, const float* a_src, const float* a_dst, float slope,
                               int32_t H, int32_t C, const float* M, const float* Z, const float* G, int64_t ldg,
                               const float* dS, float* dHf, int64_t ldd, float* da_src, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc) return rc;
    const int W = H * C;
    if (dHf && ((rc = check_ld("ldg", ldg, W)) || (rc = check_ld("ldd", ldd, W)))) return rc;
    if (n_src == 0 || (!dHf && !da_src)) return srg_ok();
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_rows == 0) {
        if (dHf)
            SRG_HIP_CHECK(hipMemset2DAsync(dHf, (size_t)ldd * sizeof(float), 0, (size_t)W * sizeof(float), (size_t)n_src, s));
        if (da_src) SRG_HIP_CHECK(hipMemsetAsync(da_src, 0, (size_t)n_src * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr_t || !indices_t) return srg_fail(SRG_ERR_INVALID, "null indptr_t or indices_t");
    if (dHf && (!a_src || !a_dst || !M || !Z || !G)) return srg_fail(SRG_ERR_INVALID, "null operand of dHf");
    if (da_src && (!perm || !dS)) return srg_fail(SRG_ERR_INVALID, "null perm or dS with da_src");
    const int64_t blocks = (n_src + kWavesPerBlock - 1) / kWavesPerBlock;
    if (dHf) {
        const bool v4 = rows_aligned(4, sizeof(float), C, {{G, ldg}, {dHf, ldd}});
        const int tile = v4 ? 256 : 64;
        const unsigned tiles = (unsigned)((W + tile - 1) / tile);
        rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
            if (v4)
                hipLaunchKernelGGL(k_gat_adjoint<4>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t, n_rows,
                                   n_src, a_src, a_dst, slope, (int)H, (int)C, M, Z, G, ldg, dHf, ldd, (int)b0);
            else
                hipLaunchKernelGGL(k_gat_adjoint<1>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t, n_rows,
                                   n_src, a_src, a_dst, slope, (int)H, (int)C, M, Z, G, ldg, dHf, ldd, (int)b0);
            return launch_status();
        });
        if (rc) return rc;
    }
    if (da_src)
        rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
            hipLaunchKernelGGL(k_gat_rowsum, dim3(nb), dim3(kBlock), 0, s, indptr_t, perm, n_src, nnz, (int)H, dS, da_src,
                               (int)b0);
            return launch_status();
        });
    return rc ? rc : srg_ok();
}

int srg_gat_attend_rows_adjoint_f32(const int64_t* indptr_t, const int32_t* indices_t, const int64_t* perm, int64_t nnz,
                                    int64_t n_rows, int64_t n_src, const int32_t* pos, int64_t B,
                                    const int64_t* indptr, const int64_t* eptr, int64_t nnzB, const float* a_src,
                                    const float* a_dst, float slope, int32_t H, int32_t C, const float* M,
                                    const float* Z, const float* G, int64_t ldg, const float* dS, float* dHf,
                                    int64_t ldd, float* da_src, void* stream)
{
    int rc = check_shape(n_rows, n_src, nnz, H, C);
    if (rc || (rc = check_batch(B, nnzB))) return rc;
    const int W = H * C;
    if (dHf && ((rc = check_ld("ldg", ldg, W)) || (rc = check_ld("ldd", ldd, W)))) return rc;
    if (n_src == 0 || (!dHf && !da_src)) return srg_ok();
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nnz == 0 || n_rows == 0 || B == 0) {   // no member entry anywhere
        if (dHf)
            SRG_HIP_CHECK(hipMemset2DAsync(dHf, (size_t)ldd * sizeof(float), 0, (size_t)W * sizeof(float), (size_t)n_src, s));
        if (da_src) SRG_HIP_CHECK(hipMemsetAsync(da_src, 0, (size_t)n_src * H * sizeof(float), s));
        return srg_ok();
    }
    if (!indptr_t || !indices_t || !pos) return srg_fail(SRG_ERR_INVALID, "null indptr_t, indices_t or pos");
    if (dHf && (!a_src || !a_dst || !M || !Z || !G)) return srg_fail(SRG_ERR_INVALID, "null operand of dHf");
    if (da_src && (!perm || !indptr || !eptr || (nnzB > 0 && !dS)))
        return srg_fail(SRG_ERR_INVALID, "null perm, indptr, eptr or dS with da_src");
    const int64_t blocks = (n_src + kWavesPerBlock - 1) / kWavesPerBlock;
    if (dHf) {
        const bool v4 = rows_aligned(4, sizeof(float), C, {{G, ldg}, {dHf, ldd}});
        const int tile = v4 ? 256 : 64;
        const unsigned tiles = (unsigned)((W + tile - 1) / tile);
        rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
            if (v4)
                hipLaunchKernelGGL(k_gat_adjoint_rows<4>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t, n_rows,
                                   n_src, pos, B, a_src, a_dst, slope, (int)H, (int)C, M, Z, G, ldg, dHf, ldd, (int)b0);
            else
                hipLaunchKernelGGL(k_gat_adjoint_rows<1>, dim3(nb, tiles), dim3(kBlock), 0, s, indptr_t, indices_t, n_rows,
                                   n_src, pos, B, a_src, a_dst, slope, (int)H, (int)C, M, Z, G, ldg, dHf, ldd, (int)b0);
            return launch_status();
        });
        if (rc) return rc;
    }
    if (da_src)
        rc = launch_chunks_capped(blocks, kBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
            hipLaunchKernelGGL(k_gat_rowsum_rows, dim3(nb), dim3(kBlock), 0, s, indptr_t, indices_t, perm, n_src, n_rows,
                               nnz, pos, B, indptr, eptr, nnzB, (int)H, dS, da_src, (int)b0);
            return launch_status();
        });
    return rc ? rc : srg_ok();
}

}  // extern "C"
