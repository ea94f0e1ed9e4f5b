// srg_hopattn.hip -- the learnable hop attention of GAMLP (SSRG/operators/message_operator/
// learnable_weighted_messahe_op.py, combination types gate / ori_ref / jk), forward and backward, without
// the [H*n, (T+1)*d] panel the reference's torch composition builds: scores, attend, attend gradient and
// the parameter gradient, each a streaming pass over the hop panels; and the recursive
// attention of iterate_learnable_weighted_message_op.py, the same four steps around a scalar recurrence per
// row (the srg_hop_recur_* entries).  Every kernel that reads a hop panel has a row-indexed
// form (ROWS = true, the srg_hop_*_rows_f32 entries): batch row r of panel t is panel row
// rows[r], everything else is indexed by r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// The hop list as a kernel argument: T device pointers and their row strides (elements).  Indexed with
// wave-uniform t only.
struct HopPanels {
    const float* p[SRG_HOP_MAX];
    int64_t ld[SRG_HOP_MAX];
};

// what panel t contributes to: the reference part of the score (jk: every panel; ori_ref: panel 0) and /
// or the hop part of the slice position t - start
__device__ __forceinline__ bool is_ref(int kind, int t) { return kind == SRG_HOP_JK || (kind == SRG_HOP_ORI_REF && t == 0); }
__host__ __device__ __forceinline__ int64_t pad4(int64_t x) { return (x + 3) / 4 * 4; }
__host__ __device__ __forceinline__ int ref_dim(int kind, int T, int d)
{
    return kind == SRG_HOP_JK ? T * d : kind == SRG_HOP_ORI_REF ? d : 0;
}

// The panel row behind batch row r.  ROWS = false: r itself, readable when the batch row is live.  ROWS = true:
// rows[r], one 8-byte load per batch row that serves every panel of the row's step; an index outside
// [0, n_src) is not readable and its row counts as +0.0f in every column (row 0's address stands in and is
// never dereferenced).
template <bool ROWS>
__device__ __forceinline__ int64_t panel_row(const int64_t* __restrict__ rows, int64_t n_src, int64_t r, bool live,
                                             bool& readable)
{
    if constexpr (ROWS) {
        const int64_t src = live ? rows[r] : -1;
        readable = (uint64_t)src < (uint64_t)n_src;
        return readable ? src : 0;
    } else {
        readable = live;
        return r;
    }
}
// VEC elements of a panel row, or zeros for a row that is not readable (ROWS = false: a plain load, the
// caller's loop runs for live rows only).
template <int VEC, bool ROWS>
__device__ __forceinline__ typename Vec<float, VEC>::type panel_load(const float* p, bool readable)
{
    if constexpr (ROWS) {
        if (!readable) return vzero<float, VEC>();
    }
    return vload<float, VEC>(p);
}

// One lane's share of the dot products of a panel row with N vectors: chunks rl.c0, rl.c0 + S, ... of the
// row at xr, one load of a chunk feeding N fma chains in chunk and element order, acc[k] = fma(v[k][e],
// x[e], acc[k]).  A chain starts from what the caller put into acc[k]; a vector with use[k] false is
// neither loaded nor folded (use is wave-uniform; constants fold away).
template <int VEC, bool ROWS, int N>
__device__ __forceinline__ void chunk_dots(const RowLanes& rl, const float* xr, bool live, bool readable, int cpr,
                                           const float* const (&v)[N], const bool (&use)[N], float (&acc)[N])
{
    typedef typename Vec<float, VEC>::type V;
    for (int c = rl.c0; live && c < cpr; c += rl.S) {
        const V xc = panel_load<VEC, ROWS>(xr + (int64_t)c * VEC, readable);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (!use[k]) continue;
            const V vc = vload<float, VEC>(v[k] + (int64_t)c * VEC);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[k] = __builtin_fmaf(elem(vc, j), elem(xc, j), acc[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// scores: zflat[h * n + i] = (ref(i) + hop(h, i)) + b   (gate: hop(h, i) + b)
//   ref(i)    = sum over the reference panels t ascending, columns in lane order, of w[t*d + c] * F_t[i, c]
//   hop(h, i) = sum over the columns of w[R + c] * F_{start+h}[i, c],  R = the reference part's length
// Rows by lanes (RowLanes, srg_device.h), the chunks folded by chunk_dots -- the reference part as ONE
// chain per lane that runs on through the panels t = 0, 1, ..., each hop part as a chain of its own from
// +0 -- and the S partials added by butterfly_add.  A panel row is loaded once and feeds both parts.  A hop
// part waits in zflat (written and read back by the same lane) until the last reference panel is folded
// in.  A row's bits depend on d, T, the slice and VEC only.  (Loading the rows of four panels ahead of the
// first fold measured slower, 0.49 against 0.30 ms at n = 200,000, T = 11, d = 128: 100 registers per lane
// instead of 30.)
// ------------------------------------------------------------------------------------------------
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_scores(HopPanels pl, int T, int start, int H, int kind, const float* __restrict__ w,
             const float* __restrict__ b, float* __restrict__ zflat, int64_t n, int d, int cpr, int lgS,
             const int64_t* __restrict__ rows, int64_t n_src)
{
    const RowLanes rl(lgS, blockDim.x);
    const int S = rl.S, c0 = rl.c0;
    const float* wh = w + ref_dim(kind, T, d);
    const float bias = b[0];
    // every lane of the wave runs every step (the butterfly reads its partners); rows past the end load nothing
    for (int64_t base = rl.first; base < n; base += rl.stride) {
        const int64_t r = base + rl.g;
        const bool live = r < n;
        bool readable;
        const int64_t pr = panel_row<ROWS>(rows, n_src, r, live, readable);
        float ref = 0.0f;
        for (int t = 0; t < T; ++t) {
            const int h = t - start;
            const bool hop = h >= 0 && h < H, rf = is_ref(kind, t);
            if (!hop && !rf) continue;
            const float* const v[2] = {w + (int64_t)t * d, wh};
            const bool use[2] = {rf, hop};
            float acc[2] = {ref, 0.0f};
            chunk_dots<VEC, ROWS>(rl, pl.p[t] + pr * pl.ld[t], live, readable, cpr, v, use, acc);
            ref = acc[0];
            if (hop) {
                butterfly_add(S, acc[1]);
                if (live && c0 == (h & (S - 1))) zflat[(int64_t)h * n + r] = acc[1];
            }
        }
        butterfly_add(S, ref);
        for (int h = c0; live && h < H; h += S) {
            float z = zflat[(int64_t)h * n + r];
            if (kind != SRG_HOP_GATE) z = __fadd_rn(ref, z);
            zflat[(int64_t)h * n + r] = __fadd_rn(z, bias);
        }
    }
}

// The score of node i at slice position h: the true transpose (gate) or the reference's .view(-1, H) of
// the hop-major vector (ori_ref, jk).
__device__ __forceinline__ int64_t paired(int flat, int64_t i, int h, int64_t n, int H)
{
    return flat ? i * H + h : (int64_t)h * n + i;
}

// P[i, h] = e_h / (e_0 + e_1 + ... + e_{H-1}), e_h = expf(a_h), a_h = 1 / (1 + expf(-S[i, h])): one thread
// per row, the sum left to right from e_0, every add and divide correctly rounded.  a is in (0, 1), so no
// maximum is subtracted.
__global__ void __launch_bounds__(256)
k_hop_softmax(const float* __restrict__ zflat, int flat, float* __restrict__ P, int64_t n, int H)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float* pr = P + i * H;
        float sum = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float s = zflat[paired(flat, i, h, n, H)];
            const float a = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-s)));
            const float e = expf(a);
            pr[h] = e;
            sum = h == 0 ? e : __fadd_rn(sum, e);
        }
        for (int h = 0; h < H; ++h) pr[h] = __fdiv_rn(pr[h], sum);
    }
}

// out[i, :] = P[i, 0] * F_0[i, :] + P[i, 1] * F_1[i, :] + ... in ascending h, separate multiply and add.
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_combine(HopPanels pl, int start, int H, const float* __restrict__ P, float* __restrict__ out, int64_t ldo,
              int64_t n, int cpr, int lgS, const int64_t* __restrict__ rows, int64_t n_src)
{
    typedef typename Vec<float, VEC>::type V;
    const RowLanes rl(lgS, blockDim.x);
    for (int64_t base = rl.first; base < n; base += rl.stride) {
        const int64_t r = base + rl.g;
        if (r >= n) continue;
        bool readable;
        const int64_t xr = panel_row<ROWS>(rows, n_src, r, true, readable);
        const float* pr = P + r * H;
        for (int c = rl.c0; c < cpr; c += rl.S) {
            V acc;
#pragma unroll 4
            for (int h = 0; h < H; ++h) {
                const V xc = panel_load<VEC, ROWS>(pl.p[start + h] + xr * pl.ld[start + h] + (int64_t)c * VEC, readable);
                const float ph = pr[h];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float t = __fmul_rn(ph, elem(xc, j));
                    elem(acc, j) = h == 0 ? t : __fadd_rn(elem(acc, j), t);
                }
            }
            vstore<float, VEC>(out + r * ldo + (int64_t)c * VEC, acc, false);
        }
    }
}

// dP[i, h] = G[i, :] . F_{start+h}[i, :]: rows by lanes, chunk_dots' one fma chain per lane from +0,
// butterfly_add.  HOP_MAJOR stores dP[h * n + i] (the recursive attention's per-row vectors).
template <int VEC, bool HOP_MAJOR, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_rowdots(HopPanels pl, int start, int H, const float* __restrict__ G, int64_t ldg, float* __restrict__ dP,
              int64_t n, int cpr, int lgS, const int64_t* __restrict__ rows, int64_t n_src)
{
    const RowLanes rl(lgS, blockDim.x);
    for (int64_t base = rl.first; base < n; base += rl.stride) {
        const int64_t r = base + rl.g;
        const bool live = r < n;
        bool readable;
        const int64_t pr = panel_row<ROWS>(rows, n_src, r, live, readable);
        const float* const v[1] = {G + r * ldg};
        for (int h = 0; h < H; ++h) {
            float dot[1] = {0.0f};
            chunk_dots<VEC, ROWS>(rl, pl.p[start + h] + pr * pl.ld[start + h], live, readable, cpr, v, {true}, dot);
            butterfly_add(rl.S, dot[0]);
            if (live && rl.c0 == (h & (rl.S - 1))) dP[HOP_MAJOR ? (int64_t)h * n + r : r * H + h] = dot[0];
        }
    }
}

// The softmax and sigmoid Jacobians of one row, one thread per row:
//   t = P_0 dP_0 + P_1 dP_1 + ... (left to right)      da_h = P_h * (dP_h - t)
//   dS_h = da_h * (a_h * (1 - a_h)),  a_h recomputed from the score as in the forward
// stored where the score came from (the inverse pairing).
__global__ void __launch_bounds__(256)
k_hop_jacobian(const float* __restrict__ zflat, int flat, const float* __restrict__ P, const float* __restrict__ dP,
               float* __restrict__ dzflat, int64_t n, int H)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float* pr = P + i * H;
        const float* dr = dP + i * H;
        float t = 0.0f;
        for (int h = 0; h < H; ++h) {
            const float m = __fmul_rn(pr[h], dr[h]);
            t = h == 0 ? m : __fadd_rn(t, m);
        }
        for (int h = 0; h < H; ++h) {
            const int64_t q = paired(flat, i, h, n, H);
            const float a = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-zflat[q])));
            const float da = __fmul_rn(pr[h], __fsub_rn(dr[h], t));
            dzflat[q] = __fmul_rn(da, __fmul_rn(a, __fsub_rn(1.0f, a)));
        }
    }
}

// s[i] = dz[0, i] + dz[1, i] + ... (left to right): the reference part's and the bias's per-node factor
__global__ void __launch_bounds__(256)
k_hop_dzsum(const float* __restrict__ dzflat, float* __restrict__ s, int64_t n, int H)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float t = dzflat[i];
        for (int h = 1; h < H; ++h) t = __fadd_rn(t, dzflat[(int64_t)h * n + i]);
        s[i] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// parameter gradient, both attentions: in_dim weights and the bias, summed over the rows in two stages.
// The scratch of the two stages, laid out in one place: s_floats floats of s (the per-row factor of the
// bias), then n_groups rows of ldq floats, row q the partial sums of group q = rows [q * rpg, (q + 1) *
// rpg): in_dim weight columns and the bias column, each row of either rounded up to 16 bytes.  The
// scratch queries, the hosts and both stages take it from here; the kernels get it by value.
// ------------------------------------------------------------------------------------------------
int64_t rows_per_group(int64_t n)   // a function of n alone (srgnn_hip.h)
{
    int64_t rpg = 32;
    while (rpg * 2048 < n) rpg *= 2;
    return rpg;
}
struct WgradLayout {
    int64_t rpg, n_groups, ldq, s_floats, in_dim;
    WgradLayout(int64_t n, int64_t in_dim)
        : rpg(rows_per_group(n)), n_groups((n + rpg - 1) / rpg), ldq(pad4(in_dim + 1)), s_floats(pad4(n)),
          in_dim(in_dim) {}
    int64_t bytes() const { return (s_floats + n_groups * ldq) * (int64_t)sizeof(float); }
};

// ------------------------------------------------------------------------------------------------
// stage 1.  CT = 2^lgCT threads of a workgroup serve one group (256 / CT groups per workgroup), thread c0
// owning the VEC columns of chunk c = tile * CT + c0 (blockIdx.y = tile: wide rows take more tiles, not more
// registers).  Per panel, rows ascending, two fma chains per column from one load of the panel
// row, chain a on the rows' factor a[i] and chain b on b[i]:
//   learnable   a = s, for a reference panel t                 -> partials[q, t*d + c]
//               b = dz[h, :], h = t - start in the slice        totalled over h -> partials[q, R + c]
//   recursive   a = dzp[h, :]                                   totalled over h -> partials[q, c]
//               b = dzq[h, :]                                   totalled over h -> partials[q, d + c]
// a total adds the panels' chains in ascending h, the first as it is.  The group's bias part s[i0] +
// s[i0+1] + ... goes to partials[q, in_dim].
// ------------------------------------------------------------------------------------------------

// The row loop of stage 1 under an index: fold(i, F[rows[i], chunk]) for i = i0 .. i1-1 ascending, ROWS_STEP
// rows a step.  The step is 16 rows where the identity loop unrolls 4: a group is one chain per column, the
// launch is a few waves per CU, and a row at a random address takes longer to arrive than the next row of a
// stream, so what sets the rate is how many row loads a thread has in flight (measured in DESIGN.md §5.4.4).
// A row's load waits for its index (index -> address -> row), so the next step's indices are fetched ahead:
// queued right behind this step's row loads -- loads return in order, so they hold no row up -- and back
// before the step's folds are done.  No branch stands between the loads of a step: an index that is out of
// range loads row 0 (there is one: n_src > 0) and its value is replaced by zeros; positions past i1 repeat the
// group's last row and are never folded.  The rows' two factors a[i], b[i] (s and dz, or dzp and dzq) are loaded
// with the step's rows, not one pair per fold: each fold would otherwise wait out a load of its own.  x points at
// the thread's chunk of panel row 0; fold(a[i], b[i], row).
constexpr int ROWS_STEP = 16;
template <int VEC, typename Fold>
__device__ __forceinline__ void indexed_rows(const float* x, int64_t ldx, const int64_t* __restrict__ rows,
                                             int64_t n_src, int64_t i0, int64_t i1, const float* __restrict__ a,
                                             const float* __restrict__ b, Fold fold)
{
    typedef typename Vec<float, VEC>::type V;
    if (n_src <= 0) {   // no panel row to stand in: every row reads as zeros
        for (int64_t i = i0; i < i1; ++i) fold(a[i], b[i], vzero<float, VEC>());
        return;
    }
    int64_t idx[ROWS_STEP];
#pragma unroll
    for (int u = 0; u < ROWS_STEP; ++u) idx[u] = rows[i0 + u < i1 ? i0 + u : i1 - 1];
    for (int64_t i = i0; i < i1; i += ROWS_STEP) {
        V xc[ROWS_STEP];
        float av[ROWS_STEP], bv[ROWS_STEP];
        bool readable[ROWS_STEP];
#pragma unroll
        for (int u = 0; u < ROWS_STEP; ++u) {
            readable[u] = (uint64_t)idx[u] < (uint64_t)n_src;
            xc[u] = vload<float, VEC>(x + (readable[u] ? idx[u] : 0) * ldx);
        }
#pragma unroll
        for (int u = 0; u < ROWS_STEP; ++u) {
            const int64_t j = i + u < i1 ? i + u : i1 - 1;
            av[u] = a[j];
            bv[u] = b[j];
        }
#pragma unroll
        for (int u = 0; u < ROWS_STEP; ++u) {
            const int64_t j = i + ROWS_STEP + u;
            idx[u] = rows[j < i1 ? j : i1 - 1];
        }
#pragma unroll
        for (int u = 0; u < ROWS_STEP; ++u)
            if (i + u < i1) fold(av[u], bv[u], readable[u] ? xc[u] : vzero<float, VEC>());
    }
}

// The learnable attention's stage 1.  The two stage-1 kernels share the layout and the host and keep their
// prologue, row loops and totals as written, on purpose: each shared form of them measured slower.
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_wgrad_partial(HopPanels pl, int T, int start, int H, int kind, const float* __restrict__ dzflat,
                    const float* __restrict__ s, float* __restrict__ partials, int64_t n, int d,
                    int cpr, int lgCT, WgradLayout L, int want_w, const int64_t* __restrict__ rows, int64_t n_src)
{
    typedef typename Vec<float, VEC>::type V;
    const int CT = 1 << lgCT;
    const int c0 = threadIdx.x & (CT - 1);
    const int64_t q = (int64_t)blockIdx.x * (256 >> lgCT) + (threadIdx.x >> lgCT);
    if (q >= L.n_groups) return;
    const int c = blockIdx.y * CT + c0;
    float* out = partials + q * L.ldq;
    const int64_t i0 = q * L.rpg, i1 = i0 + L.rpg < n ? i0 + L.rpg : n;
    if (c == 0) {
        float t = s[i0];
        for (int64_t i = i0 + 1; i < i1; ++i) t = __fadd_rn(t, s[i]);
        out[L.in_dim] = t;
    }
    if (!want_w || c >= cpr) return;
    V tot;
    for (int t = 0; t < T; ++t) {
        const int h = t - start;
        const bool hop = h >= 0 && h < H, rf = is_ref(kind, t);
        if (!hop && !rf) continue;
        const float* x = pl.p[t] + (int64_t)c * VEC;
        const int64_t ldx = pl.ld[t];
        const float* dz = dzflat + (int64_t)(hop ? h : 0) * n;
        V ra = vzero<float, VEC>(), ha = vzero<float, VEC>();
        if constexpr (ROWS) {
            indexed_rows<VEC>(x, ldx, rows, n_src, i0, i1, s, dz, [&](float si, float di, const V& xc) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (rf) elem(ra, j) = __builtin_fmaf(si, elem(xc, j), elem(ra, j));
                    if (hop) elem(ha, j) = __builtin_fmaf(di, elem(xc, j), elem(ha, j));
                }
            });
        } else {
#pragma unroll 4
            for (int64_t i = i0; i < i1; ++i) {
                const V xc = vload<float, VEC>(x + i * ldx);
                const float si = s[i], di = dz[i];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (rf) elem(ra, j) = __builtin_fmaf(si, elem(xc, j), elem(ra, j));
                    if (hop) elem(ha, j) = __builtin_fmaf(di, elem(xc, j), elem(ha, j));
                }
            }
        }
        if (rf) vstore<float, VEC>(out + (int64_t)t * d + (int64_t)c * VEC, ra, false);
        if (hop) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) elem(tot, j) = h == 0 ? elem(ha, j) : __fadd_rn(elem(tot, j), elem(ha, j));
        }
    }
    vstore<float, VEC>(out + (L.in_dim - d) + (int64_t)c * VEC, tot, false);
}

// The recursive attention's stage 1: every panel feeds both chains.
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_recur_wgrad_partial(HopPanels pl, int H, const float* __restrict__ dzp, const float* __restrict__ dzq,
                          const float* __restrict__ s, float* __restrict__ partials, int64_t n, int d,
                          int cpr, int lgCT, WgradLayout L, int want_w, const int64_t* __restrict__ rows, int64_t n_src)
{
    typedef typename Vec<float, VEC>::type V;
    const int CT = 1 << lgCT;
    const int c0 = threadIdx.x & (CT - 1);
    const int64_t q = (int64_t)blockIdx.x * (256 >> lgCT) + (threadIdx.x >> lgCT);
    if (q >= L.n_groups) return;
    const int c = blockIdx.y * CT + c0;
    float* out = partials + q * L.ldq;
    const int64_t i0 = q * L.rpg, i1 = i0 + L.rpg < n ? i0 + L.rpg : n;
    if (c == 0) {
        float t = s[i0];
        for (int64_t i = i0 + 1; i < i1; ++i) t = __fadd_rn(t, s[i]);
        out[L.in_dim] = t;
    }
    if (!want_w || c >= cpr) return;
    V toth, totc;
    for (int h = 0; h < H; ++h) {
        const float* x = pl.p[h] + (int64_t)c * VEC;
        const int64_t ldx = pl.ld[h];
        const float* dp = dzp + (int64_t)h * n;
        const float* dq = dzq + (int64_t)h * n;
        V ha = vzero<float, VEC>(), ca = vzero<float, VEC>();
        if constexpr (ROWS) {
            indexed_rows<VEC>(x, ldx, rows, n_src, i0, i1, dp, dq, [&](float pi, float qi, const V& xc) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    elem(ha, j) = __builtin_fmaf(pi, elem(xc, j), elem(ha, j));
                    elem(ca, j) = __builtin_fmaf(qi, elem(xc, j), elem(ca, j));
                }
            });
        } else {
#pragma unroll 4
            for (int64_t i = i0; i < i1; ++i) {
                const V xc = vload<float, VEC>(x + i * ldx);
                const float pi = dp[i], qi = dq[i];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    elem(ha, j) = __builtin_fmaf(pi, elem(xc, j), elem(ha, j));
                    elem(ca, j) = __builtin_fmaf(qi, elem(xc, j), elem(ca, j));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            elem(toth, j) = h == 0 ? elem(ha, j) : __fadd_rn(elem(toth, j), elem(ha, j));
            elem(totc, j) = h == 0 ? elem(ca, j) : __fadd_rn(elem(totc, j), elem(ca, j));
        }
    }
    vstore<float, VEC>(out + (int64_t)c * VEC, toth, false);
    vstore<float, VEC>(out + d + (int64_t)c * VEC, totc, false);
}

// stage 2: column j of the partials folded in group order, the first as it is
__global__ void __launch_bounds__(256)
k_hop_wgrad_fold(const float* __restrict__ partials, WgradLayout L, float* __restrict__ dw, float* __restrict__ db)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > L.in_dim) return;
    if (j < L.in_dim ? dw == nullptr : db == nullptr) return;
    float t = partials[j];
#pragma unroll 32
    for (int64_t q = 1; q < L.n_groups; ++q) t = __fadd_rn(t, partials[q * L.ldq + j]);
    if (j < L.in_dim) dw[j] = t; else db[0] = t;
}

// ------------------------------------------------------------------------------------------------
// The recursive hop attention (IterateLearnableWeightedMessageOp).  w = [w_h | w_c] is the
// row of Linear(2d, 1); w_c . (sum_j W_j F_j[i, :]) = sum_j W_j (w_c . F_j[i, :]), so between the panels and
// the final weighted sum the operator is a scalar recurrence per row on the 2H dot products below.
//
// zp[h * n + i] = w_h . F_h[i, :], zq[h * n + i] = w_c . F_h[i, :]: rows by lanes, chunk_dots' two fma chains
// per lane from +0 from one load of the panel row, both through one butterfly_add.
// ------------------------------------------------------------------------------------------------
template <int VEC, bool ROWS>
__global__ void __launch_bounds__(256)
k_hop_recur_scores(HopPanels pl, int H, const float* __restrict__ w, float* __restrict__ zp, float* __restrict__ zq,
                   int64_t n, int d, int cpr, int lgS, const int64_t* __restrict__ rows, int64_t n_src)
{
    const RowLanes rl(lgS, blockDim.x);
    const float* const v[2] = {w, w + d};
    for (int64_t base = rl.first; base < n; base += rl.stride) {
        const int64_t r = base + rl.g;
        const bool live = r < n;
        bool readable;
        const int64_t pr = panel_row<ROWS>(rows, n_src, r, live, readable);
        for (int h = 0; h < H; ++h) {
            float z[2] = {0.0f, 0.0f};
            chunk_dots<VEC, ROWS>(rl, pl.p[h] + pr * pl.ld[h], live, readable, cpr, v, {true, true}, z);
            butterfly_add(rl.S, z[0], z[1]);
            if (live && rl.c0 == (h & (rl.S - 1))) {
                zp[(int64_t)h * n + r] = z[0];
                zq[(int64_t)h * n + r] = z[1];
            }
        }
    }
}

// The work buffer of the recurrence, (H (H + 1) / 2 + H) vectors of n floats: vector tri(i) + j holds
// W(i)_j, the weights after step i (j <= i), vector H (H + 1) / 2 + i holds g_i.  A thread owns a row and
// walks the vectors at stride n, so a wave's accesses are 64 consecutive floats.  While a row is worked on
// its H-vectors live in LDS, a column of RECUR_BLOCK-strided floats per thread (no two threads share a
// word, so no barrier): a private array under a runtime index would go to scratch, and walking the
// recurrence through the global buffer alone made every step wait for its own stores and loads
// (k_hop_recur_forward 77 -> 31 us, k_hop_recur_backward 97 -> 70 us at n = 200,000, H = 11).
__host__ __device__ __forceinline__ int64_t tri(int i) { return (int64_t)i * (i + 1) / 2; }
constexpr int RECUR_BLOCK = 64;
constexpr int RECUR_FWD_VECTORS = 3;   // p, q, W
constexpr int RECUR_BWD_VECTORS = 5;   // q, dW, dq, W(i), W(i-1)

// count floats src[j * n] -> dst[j * RECUR_BLOCK] (a thread's column of an LDS vector), eight loads in flight at a
// time: a loop of single loads would wait out one memory latency per element.  The tail batch reads the last
// element again instead of branching.
__device__ __forceinline__ void recur_fetch(float* dst, const float* __restrict__ src, int64_t n, int count)
{
    for (int j0 = 0; j0 < count; j0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(j0 + u < count ? j0 + u : count - 1) * n];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u < count) dst[(j0 + u) * RECUR_BLOCK] = v[u];
    }
}

// One thread per row.  W(0) = [1] (NaN where s_0 = (p_0 + q_0) + b is NaN); for i = 1 .. H-1, with W = W(i-1):
//   r = W_0 q_0 + W_1 q_1 + ... + W_{i-1} q_{i-1}   (left to right)       s = (p_i + r) + b
//   g_i = 1 / (1 + expf(-s))
//   e_j = expf(W_j) (j < i), e_i = expf(g_i),  W(i)_j = e_j / (e_0 + e_1 + ... + e_i)   (left to right)
// every add, multiply and divide correctly rounded; the arguments of expf lie in (0, 1], so no maximum is
// subtracted.  P[i, :] = W(H-1).  Dynamic LDS: RECUR_FWD_VECTORS * H * RECUR_BLOCK floats.
__global__ void __launch_bounds__(RECUR_BLOCK)
k_hop_recur_forward(const float* __restrict__ zp, const float* __restrict__ zq, const float* __restrict__ b,
                    float* __restrict__ work, float* __restrict__ P, int64_t n, int H)
{
    extern __shared__ float recur_lds[];
    float* sp = recur_lds + threadIdx.x;            // element j at [j * RECUR_BLOCK]
    float* sq = sp + H * RECUR_BLOCK;
    float* sw = sq + H * RECUR_BLOCK;
    const int64_t stride = (int64_t)gridDim.x * RECUR_BLOCK;
    const float bias = b[0];
    for (int64_t r = (int64_t)blockIdx.x * RECUR_BLOCK + threadIdx.x; r < n; r += stride) {
        float* wr = work + r;
        float* gs = wr + (tri(H - 1) + H) * n;
        recur_fetch(sp, zp + r, n, H);
        recur_fetch(sq, zq + r, n, H);
        // W(0) = softmax([g_0]) is 1 whatever g_0 is -- except NaN: the reference's one-column softmax of a NaN
        // gate is NaN, so a row whose score s_0 = (p_0 + q_0) + b is NaN (a NaN cell of hop 0, or Inf cells
        // that meet with opposite signs) is NaN throughout, as there
        const float s0 = __fadd_rn(__fadd_rn(sp[0], sq[0]), bias);
        const float w0 = s0 != s0 ? s0 : 1.0f;
        sw[0] = w0;
        wr[0] = w0;
        gs[0] = 0.0f;   // g_0 itself is never read
        for (int i = 1; i < H; ++i) {
            float* cur = wr + tri(i) * n;
            float rs = 0.0f, sum = 0.0f;
            for (int j = 0; j < i; ++j) {
                const float wj = sw[j * RECUR_BLOCK];
                const float m = __fmul_rn(wj, sq[j * RECUR_BLOCK]);
                const float e = expf(wj);
                rs = j == 0 ? m : __fadd_rn(rs, m);
                sum = j == 0 ? e : __fadd_rn(sum, e);
                sw[j * RECUR_BLOCK] = e;
            }
            const float s = __fadd_rn(__fadd_rn(sp[i * RECUR_BLOCK], rs), bias);
            const float gi = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-s)));
            const float eg = expf(gi);
            sum = __fadd_rn(sum, eg);
            gs[(int64_t)i * n] = gi;
            sw[i * RECUR_BLOCK] = eg;
            for (int j = 0; j <= i; ++j) {
                const float wj = __fdiv_rn(sw[j * RECUR_BLOCK], sum);
                sw[j * RECUR_BLOCK] = wj;
                cur[(int64_t)j * n] = wj;
            }
        }
        for (int j = 0; j < H; ++j) P[r * H + j] = sw[j * RECUR_BLOCK];
    }
}

// The reverse recurrence, one thread per row.  dzp holds dW(H-1)_j = G[i, :] . F_j[i, :] on entry (hop-major);
// for i = H-1 .. 1, with W = W(i), dW = dW(i):
//   t = W_0 dW_0 + ... + W_i dW_i (left to right)      dx_j = W_j (dW_j - t)
//   ds = dx_i * (g_i * (1 - g_i))                      dzp[i] = ds
//   dzq[j] (+)= ds * W(i-1)_j,  dW(i-1)_j = dx_j + ds * q_j   for j < i
// dzq[j]'s first term (i = H-1) is stored as it is and the later ones added in descending i; dzq[H-1] = 0,
// dzp[0] = 0.  Slot i of dW is dead after step i, which is where ds goes.  Dynamic LDS: RECUR_BWD_VECTORS * H *
// RECUR_BLOCK floats.
__global__ void __launch_bounds__(RECUR_BLOCK)
k_hop_recur_backward(const float* __restrict__ zq, const float* __restrict__ work, float* __restrict__ dzp,
                     float* __restrict__ dzq, int64_t n, int H)
{
    extern __shared__ float recur_lds[];
    float* sq = recur_lds + threadIdx.x;            // element j at [j * RECUR_BLOCK]
    float* sdw = sq + H * RECUR_BLOCK;
    float* sdq = sdw + H * RECUR_BLOCK;
    float* swc = sdq + H * RECUR_BLOCK;
    float* swp = swc + H * RECUR_BLOCK;
    const int64_t stride = (int64_t)gridDim.x * RECUR_BLOCK;
    for (int64_t r = (int64_t)blockIdx.x * RECUR_BLOCK + threadIdx.x; r < n; r += stride) {
        const float* wr = work + r;
        const float* gs = wr + (tri(H - 1) + H) * n;
        recur_fetch(sq, zq + r, n, H);
        recur_fetch(sdw, dzp + r, n, H);
        recur_fetch(swc, wr + tri(H - 1) * n, n, H);
        sdq[(H - 1) * RECUR_BLOCK] = 0.0f;
        for (int i = H - 1; i >= 1; --i) {
            // swc holds W(i): loaded above for i = H-1, the W(i-1) of the step before otherwise
            const float* prev = wr + tri(i - 1) * n;
            const float gi = gs[(int64_t)i * n];
            recur_fetch(swp, prev, n, i);
            float t = 0.0f;
            for (int j = 0; j <= i; ++j) {
                const float m = __fmul_rn(swc[j * RECUR_BLOCK], sdw[j * RECUR_BLOCK]);
                t = j == 0 ? m : __fadd_rn(t, m);
            }
            const float dxi = __fmul_rn(swc[i * RECUR_BLOCK], __fsub_rn(sdw[i * RECUR_BLOCK], t));
            const float ds = __fmul_rn(dxi, __fmul_rn(gi, __fsub_rn(1.0f, gi)));
            for (int j = 0; j < i; ++j) {
                const float dx = __fmul_rn(swc[j * RECUR_BLOCK], __fsub_rn(sdw[j * RECUR_BLOCK], t));
                const float m = __fmul_rn(ds, swp[j * RECUR_BLOCK]);
                sdq[j * RECUR_BLOCK] = i == H - 1 ? m : __fadd_rn(sdq[j * RECUR_BLOCK], m);
                sdw[j * RECUR_BLOCK] = __fadd_rn(dx, __fmul_rn(ds, sq[j * RECUR_BLOCK]));
            }
            sdw[i * RECUR_BLOCK] = ds;
            float* x = swc; swc = swp; swp = x;
        }
        sdw[0] = 0.0f;
        for (int j = 0; j < H; ++j) {
            dzp[(int64_t)j * n + r] = sdw[j * RECUR_BLOCK];
            dzq[(int64_t)j * n + r] = sdq[j * RECUR_BLOCK];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct HopShape {
    HopPanels pl;
    int vec, cpr, lgS;
    bool empty;               // n == 0: nothing to launch, and nothing else here is set
    unsigned row_blocks;      // the row-streaming kernels' grid (row_lanes_grid)
    unsigned thread_blocks;   // the one-thread-per-row kernels' grid
};

// The head of every *_rows_* entry after its own flag checks: the row index (NULL is the identity, n_src is
// not looked at), the hop list and the slice; then the access width every row of every panel and of `wide` is
// aligned for, and the grids.  wide: the one operand besides the panels that the entry reads or writes in
// chunks (NULL: none), ld_name its row stride's name in the error text (NULL for a vector, ld = 0).
int hop_shape(const int64_t* rows, int64_t n_src, const float* const* panels, const int64_t* ldp, int T, int start,
              int end, int64_t n, int d, const Operand* wide, const char* ld_name, HopShape& hs)
{
    if (rows && n_src < 0) return srg_fail(SRG_ERR_INVALID, "n_src=%lld panel rows", (long long)n_src);
    if (ld_name && wide->ld < d) return srg_fail(SRG_ERR_INVALID, "%s=%lld < d=%d", ld_name, (long long)wide->ld, d);
    if (T < 1 || T > SRG_HOP_MAX) return srg_fail(SRG_ERR_INVALID, "T=%d hop panels: 1 .. %d", T, SRG_HOP_MAX);
    if (start < 0 || end <= start || end > T)
        return srg_fail(SRG_ERR_INVALID, "hop slice [%d, %d) of %d panels", start, end, T);
    if (n < 0 || d < 1) return srg_fail(SRG_ERR_INVALID, "bad shape n=%lld d=%d", (long long)n, d);
    if ((int64_t)T * d + d + 1 > INT32_MAX) return srg_fail(SRG_ERR_INVALID, "T*d = %d*%d too wide", T, d);
    hs.empty = n == 0;
    if (hs.empty) return SRG_OK;
    if (!panels || !ldp) return srg_fail(SRG_ERR_INVALID, "null panel list");
    for (int t = 0; t < T; ++t) {
        if (!panels[t] || ldp[t] < d)
            return srg_fail(SRG_ERR_INVALID, "panel %d: pointer %p, leading dimension %lld < d=%d", t,
                            (const void*)panels[t], (long long)ldp[t], d);
        hs.pl.p[t] = panels[t];
        hs.pl.ld[t] = ldp[t];
    }
    for (int t = T; t < SRG_HOP_MAX; ++t) { hs.pl.p[t] = nullptr; hs.pl.ld[t] = 0; }
    if (wide && !wide->p) return srg_fail(SRG_ERR_INVALID, "null pointer");
    hs.vec = 1;
    for (int v = 4; v > 1 && hs.vec == 1; v >>= 1) {
        bool ok = !wide || rows_aligned(v, sizeof(float), d, {{wide->p, wide->ld}});
        for (int t = 0; ok && t < T; ++t) ok = rows_aligned(v, sizeof(float), d, {{panels[t], ldp[t]}});
        if (ok) hs.vec = v;
    }
    hs.cpr = d / hs.vec;
    const RowLanesGrid rg = row_lanes_grid(hs.cpr, n);
    hs.lgS = rg.lgS;
    hs.row_blocks = rg.blocks;
    hs.thread_blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 16);
    return SRG_OK;
}

// the recurrence kernels' grid: one wave per block, grid-stride over the rows
unsigned recur_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + RECUR_BLOCK - 1) / RECUR_BLOCK, 256 * 64); }

int check_kind(int kind)
{
    if (kind != SRG_HOP_GATE && kind != SRG_HOP_ORI_REF && kind != SRG_HOP_JK)
        return srg_fail(SRG_ERR_INVALID, "hop attention kind %d", kind);
    return SRG_OK;
}

int check_pairing(int pairing)
{
    if (pairing != SRG_HOP_PAIR_TRANSPOSE && pairing != SRG_HOP_PAIR_FLAT)
        return srg_fail(SRG_ERR_INVALID, "hop attention pairing %d", pairing);
    return SRG_OK;
}

// launch(VEC, ROWS), both std::integral_constants, under the panels' access width; ROWS = true with an index,
// the identity kernels without
template <typename Launch>
void by_vec_rows(int vec, bool rows, Launch launch)
{
    auto by_rows = [&](auto V) {
        if (rows) launch(V, std::true_type{}); else launch(V, std::false_type{});
    };
    if (vec == 4) by_rows(std::integral_constant<int, 4>{});
    else if (vec == 2) by_rows(std::integral_constant<int, 2>{});
    else by_rows(std::integral_constant<int, 1>{});
}

// The parameter gradient of either attention once the entry has its shape: k_hop_dzsum over the H vectors at
// dz, the entry's stage 1, stage 2.  No rows: the sums are empty.  bad: what is wrong with the entry's other
// arguments (NULL: nothing), reported once there are rows.  stage1(grid, lgCT, s, partials, L) launches the
// entry's own stage-1 kernel.
template <typename Stage1>
int launch_wgrad(const HopShape& hs, const float* dz, int H, int64_t in_dim, float* dw, float* db, void* scratch,
                 const char* bad, int64_t n, hipStream_t st, Stage1 stage1)
{
    if (!dw && !db) return srg_ok();
    if (hs.empty) {
        if (dw) SRG_HIP_CHECK(hipMemsetAsync(dw, 0, (size_t)in_dim * sizeof(float), st));
        if (db) SRG_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float), st));
        return srg_ok();
    }
    if (bad) return srg_fail(SRG_ERR_INVALID, "%s", bad);
    const WgradLayout L(n, in_dim);
    int lgCT = 0;
    while (lgCT < 8 && (1 << lgCT) < hs.cpr) ++lgCT;
    float* s = static_cast<float*>(scratch);
    float* partials = s + L.s_floats;
    const int groups_per_block = 256 >> lgCT;
    const dim3 grid((unsigned)((L.n_groups + groups_per_block - 1) / groups_per_block),
                    (unsigned)((hs.cpr + (1 << lgCT) - 1) >> lgCT));
    hipLaunchKernelGGL(k_hop_dzsum, dim3(hs.thread_blocks), dim3(256), 0, st, dz, s, n, H);
    stage1(grid, lgCT, s, partials, L);
    hipLaunchKernelGGL(k_hop_wgrad_fold, dim3((unsigned)((in_dim + 1 + 255) / 256)), dim3(256), 0, st, partials, L, dw,
                       db);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

}  // namespace

extern "C" {

int srg_hop_scores_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                            int32_t T, int32_t start, int32_t end, int kind, const float* w, const float* b,
                            float* zflat, int64_t n, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (int rc = check_kind(kind)) return rc;
    HopShape hs;
    const Operand wide = {w, 0};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, start, end, n, d, &wide, nullptr, hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!b || !zflat) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const int H = end - start;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_scores<V, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, T, start, H, kind, w, b,
                           zflat, n, d, hs.cpr, hs.lgS, rows, n_src);
    });
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_scores_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                       int kind, const float* w, const float* b, float* zflat, int64_t n, int32_t d, void* stream)
{
    return srg_hop_scores_rows_f32(panels, ldp, nullptr, 0, T, start, end, kind, w, b, zflat, n, d, stream);
}

int srg_hop_attend_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                            int32_t T, int32_t start, int32_t end, const float* zflat, int pairing, float* P,
                            float* out, int64_t ldo, int64_t n, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (int rc = check_pairing(pairing)) return rc;
    HopShape hs;
    const Operand wide = {out, ldo};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, start, end, n, d, &wide, "ldo", hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!zflat || !P) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const int H = end - start;
    for (int t = start; t < end; ++t)
        if (out == panels[t]) return srg_fail(SRG_ERR_INVALID, "out must not alias a hop panel");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_hop_softmax, dim3(hs.thread_blocks), dim3(256), 0, st, zflat, pairing, P, n, H);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_combine<V, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, start, H, P, out, ldo,
                           n, hs.cpr, hs.lgS, rows, n_src);
    });
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_attend_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                       const float* zflat, int pairing, float* P, float* out, int64_t ldo, int64_t n, int32_t d,
                       void* stream)
{
    return srg_hop_attend_rows_f32(panels, ldp, nullptr, 0, T, start, end, zflat, pairing, P, out, ldo, n, d, stream);
}

int srg_hop_attend_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                 int32_t T, int32_t start, int32_t end, const float* G, int64_t ldg,
                                 const float* zflat, const float* P, int pairing, float* dP, float* dzflat, int64_t n,
                                 int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (int rc = check_pairing(pairing)) return rc;
    HopShape hs;
    const Operand wide = {G, ldg};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, start, end, n, d, &wide, "ldg", hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!zflat || !P || !dP || !dzflat) return srg_fail(SRG_ERR_INVALID, "null pointer");
    if (dzflat == zflat || dP == P) return srg_fail(SRG_ERR_INVALID, "dzflat / dP must not alias zflat / P");
    const int H = end - start;
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_rowdots<V, false, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, start, H, G, ldg,
                           dP, n, hs.cpr, hs.lgS, rows, n_src);
    });
    hipLaunchKernelGGL(k_hop_jacobian, dim3(hs.thread_blocks), dim3(256), 0, st, zflat, pairing, P, dP, dzflat, n, H);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_attend_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                            const float* G, int64_t ldg, const float* zflat, const float* P, int pairing,
                            float* dP, float* dzflat, int64_t n, int32_t d, void* stream)
{
    return srg_hop_attend_grad_rows_f32(panels, ldp, nullptr, 0, T, start, end, G, ldg, zflat, P, pairing, dP, dzflat,
                                        n, d, stream);
}

int srg_hop_scores_grad_scratch_bytes(int64_t n, int32_t d, int32_t T, int32_t H, int kind, int64_t* bytes)
{
    if (int rc = check_kind(kind)) return rc;
    if (!bytes) return srg_fail(SRG_ERR_INVALID, "null pointer");
    if (n < 0 || d < 1 || T < 1 || T > SRG_HOP_MAX || H < 1 || H > T)
        return srg_fail(SRG_ERR_INVALID, "bad shape n=%lld d=%d T=%d H=%d", (long long)n, d, T, H);
    *bytes = WgradLayout(n, (int64_t)ref_dim(kind, T, d) + d).bytes();
    return srg_ok();
}

int srg_hop_scores_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                 int32_t T, int32_t start, int32_t end, int kind, const float* dzflat, float* dw,
                                 float* db, void* scratch, int64_t n, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (int rc = check_kind(kind)) return rc;
    HopShape hs;
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, start, end, n, d, nullptr, nullptr, hs)) return rc;
    const int H = end - start;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char* bad = !dzflat || !scratch || !aligned(scratch, 16)
                          ? "dzflat or scratch null, or scratch not 16-byte aligned" : nullptr;
    return launch_wgrad(hs, dzflat, H, (int64_t)ref_dim(kind, T, d) + d, dw, db, scratch, bad, n, st,
                        [&](dim3 grid, int lgCT, const float* s, float* partials, const WgradLayout& L) {
        by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
            hipLaunchKernelGGL((k_hop_wgrad_partial<V, R>), grid, dim3(256), 0, st, hs.pl, T, start, H, kind, dzflat, s,
                               partials, n, d, hs.cpr, lgCT, L, dw != nullptr, rows, n_src);
        });
    });
}

int srg_hop_scores_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t start, int32_t end,
                            int kind, const float* dzflat, float* dw, float* db, void* scratch, int64_t n,
                            int32_t d, void* stream)
{
    return srg_hop_scores_grad_rows_f32(panels, ldp, nullptr, 0, T, start, end, kind, dzflat, dw, db, scratch, n, d,
                                        stream);
}

// ---- the recursive attention (start == 0: the reference works with no other) ----

int srg_hop_recur_scores_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                  int32_t T, int32_t end, const float* w, float* zp, float* zq, int64_t n, int32_t d,
                                  void* stream)
{
    SRG_DEVICE_GUARD(stream);
    HopShape hs;
    const Operand wide = {w, 0};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, 0, end, n, d, &wide, nullptr, hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!zp || !zq || zp == zq) return srg_fail(SRG_ERR_INVALID, "zp / zq null or the same");
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_recur_scores<V, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, end, w, zp, zq, n,
                           d, hs.cpr, hs.lgS, rows, n_src);
    });
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_recur_scores_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end, const float* w,
                             float* zp, float* zq, int64_t n, int32_t d, void* stream)
{
    return srg_hop_recur_scores_rows_f32(panels, ldp, nullptr, 0, T, end, w, zp, zq, n, d, stream);
}

int srg_hop_recur_attend_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows, int64_t n_src,
                                  int32_t T, int32_t end, const float* zp, const float* zq, const float* b,
                                  float* work, float* P, float* out, int64_t ldo, int64_t n, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    HopShape hs;
    const Operand wide = {out, ldo};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, 0, end, n, d, &wide, "ldo", hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!zp || !zq || !b || !work || !P) return srg_fail(SRG_ERR_INVALID, "null pointer");
    for (int t = 0; t < end; ++t)
        if (out == panels[t]) return srg_fail(SRG_ERR_INVALID, "out must not alias a hop panel");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_hop_recur_forward, dim3(recur_blocks(n)), dim3(RECUR_BLOCK),
                       (size_t)RECUR_FWD_VECTORS * end * RECUR_BLOCK * sizeof(float), st, zp, zq, b, work, P, n, end);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_combine<V, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, 0, end, P, out, ldo, n,
                           hs.cpr, hs.lgS, rows, n_src);
    });
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_recur_attend_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end, const float* zp,
                             const float* zq, const float* b, float* work, float* P, float* out, int64_t ldo,
                             int64_t n, int32_t d, void* stream)
{
    return srg_hop_recur_attend_rows_f32(panels, ldp, nullptr, 0, T, end, zp, zq, b, work, P, out, ldo, n, d, stream);
}

int srg_hop_recur_attend_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows,
                                       int64_t n_src, int32_t T, int32_t end, const float* G, int64_t ldg,
                                       const float* zq, const float* work, float* dzp, float* dzq, int64_t n,
                                       int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    HopShape hs;
    const Operand wide = {G, ldg};
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, 0, end, n, d, &wide, "ldg", hs)) return rc;
    if (hs.empty) return srg_ok();
    if (!zq || !work || !dzp || !dzq) return srg_fail(SRG_ERR_INVALID, "null pointer");
    if (dzp == dzq || dzp == zq || dzq == zq) return srg_fail(SRG_ERR_INVALID, "dzp, dzq and zq must not alias");
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
        hipLaunchKernelGGL((k_hop_rowdots<V, true, R>), dim3(hs.row_blocks), dim3(256), 0, st, hs.pl, 0, end, G, ldg,
                           dzp, n, hs.cpr, hs.lgS, rows, n_src);
    });
    hipLaunchKernelGGL(k_hop_recur_backward, dim3(recur_blocks(n)), dim3(RECUR_BLOCK),
                       (size_t)RECUR_BWD_VECTORS * end * RECUR_BLOCK * sizeof(float), st, zq, work, dzp, dzq, n, end);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_recur_attend_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end,
                                  const float* G, int64_t ldg, const float* zq, const float* work, float* dzp,
                                  float* dzq, int64_t n, int32_t d, void* stream)
{
    return srg_hop_recur_attend_grad_rows_f32(panels, ldp, nullptr, 0, T, end, G, ldg, zq, work, dzp, dzq, n, d, stream);
}

int srg_hop_recur_scores_grad_scratch_bytes(int64_t n, int32_t d, int32_t H, int64_t* bytes)
{
    if (!bytes) return srg_fail(SRG_ERR_INVALID, "null pointer");
    if (n < 0 || d < 1 || H < 1 || H > SRG_HOP_MAX || 2 * (int64_t)d + 1 > INT32_MAX)
        return srg_fail(SRG_ERR_INVALID, "bad shape n=%lld d=%d H=%d", (long long)n, d, H);
    *bytes = WgradLayout(n, 2 * (int64_t)d).bytes();
    return srg_ok();
}

int srg_hop_recur_scores_grad_rows_f32(const float* const* panels, const int64_t* ldp, const int64_t* rows,
                                       int64_t n_src, int32_t T, int32_t end, const float* dzp, const float* dzq,
                                       float* dw, float* db, void* scratch, int64_t n, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    HopShape hs;
    if (int rc = hop_shape(rows, n_src, panels, ldp, T, 0, end, n, d, nullptr, nullptr, hs)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char* bad = !dzp || !dzq || !scratch || !aligned(scratch, 16)
                          ? "dzp, dzq or scratch null, or scratch not 16-byte aligned" : nullptr;
    return launch_wgrad(hs, dzp, end, 2 * (int64_t)d, dw, db, scratch, bad, n, st,
                        [&](dim3 grid, int lgCT, const float* s, float* partials, const WgradLayout& L) {
        by_vec_rows(hs.vec, rows != nullptr, [&](auto V, auto R) {
            hipLaunchKernelGGL((k_hop_recur_wgrad_partial<V, R>), grid, dim3(256), 0, st, hs.pl, end, dzp, dzq, s,
                               partials, n, d, hs.cpr, lgCT, L, dw != nullptr, rows, n_src);
        });
    });
}

int srg_hop_recur_scores_grad_f32(const float* const* panels, const int64_t* ldp, int32_t T, int32_t end,
                                  const float* dzp, const float* dzq, float* dw, float* db, void* scratch, int64_t n,
                                  int32_t d, void* stream)
{
    return srg_hop_recur_scores_grad_rows_f32(panels, ldp, nullptr, 0, T, end, dzp, dzq, dw, db, scratch, n, d, stream);
}

}  // extern "C"
