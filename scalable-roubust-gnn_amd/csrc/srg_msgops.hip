// srg_msgops.hip -- the message operators over the hop panels, element-wise on the device: the hop
// accumulation and selection steps, the NAFS similarity weights, the row divide, torch's order for the
// tail of a weighted sum, and the row gather.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// hop aggregation (fused SGC / SSGC / GBP precompute: MessageOp.combine without the K+1 panels)
//
// The reference combines the hop list on the host (SSRG/operators/message_operator/{sum,mean,
// simple_weighted}_message_op.py, operators/utils.py:426-437).  Python's sum() is a left-to-right
// accumulation from +0; one_dim_weighted_add is torch's CPU dim-0 sum of rounded products, whose
// order (ATen cascade_sum) the host plans as a sequence of the element-wise steps below:
//   INIT: agg = 0 + w*y      ADD: agg = agg + w*y      DIV: agg = agg / w
// with separate multiply / add / correctly rounded divide (no contraction).  The last < 32 flat
// elements of a weighted sum take torch's scalar row_sum order instead (k_tail_*).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_hop_accumulate(float* __restrict__ agg, int64_t lda, const float* __restrict__ y, int64_t ldy,
                 int64_t n_rows, int d, float w, int mode)
{
    // one wave per row (grid-stride over rows), lanes stride the columns: no index division
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        float* a = agg + r * lda;
        const float* yr = y + r * ldy;
        for (int c = lane; c < d; c += 64) {
            if (mode == SRG_ACC_DIV) {
                a[c] = __fdiv_rn(a[c], w);
            } else {
                const float p = __fmul_rn(w, yr[c]);
                a[c] = __fadd_rn(mode == SRG_ACC_INIT ? 0.0f : a[c], p);
            }
        }
    }
}

// The selecting modes (SSRG/operators/message_operator/{min,max,concat}_message_op.py):
//   COPY: agg = y, bit for bit (concat's hop 0; the first hop of a min / max slice)
//   MIN:  if (!isnan(agg) && !(y >= agg)) agg = y        MAX: ... !(y <= agg) ...
// -- torch's CPU min / max over the stacked hops: the first NaN wins and sticks, a tie (-0 against
// +0 included) keeps the earlier hop.  Values move as their 32 bits, so NaN payloads survive.
__global__ void __launch_bounds__(256)
k_hop_select(float* __restrict__ agg, int64_t lda, const float* __restrict__ y, int64_t ldy, int64_t n_rows,
             int d, int mode)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        uint32_t* a = reinterpret_cast<uint32_t*>(agg + r * lda);
        const uint32_t* yr = reinterpret_cast<const uint32_t*>(y + r * ldy);
        for (int c = lane; c < d; c += 64) {
            const uint32_t yb = yr[c];
            if (mode == SRG_ACC_COPY) {
                a[c] = yb;
            } else {
                const float av = __uint_as_float(a[c]), yv = __uint_as_float(yb);
                const bool keep = mode == SRG_ACC_MIN ? yv >= av : yv <= av;
                if (av == av && !keep) a[c] = yb;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// NAFS step (SSRG/operators/message_operator/over_smooth_distance_op.py, OverSmoothDistanceWeightedOp):
// per row, hop y is weighted by exp of its cosine similarity to hop 0,
//   s = ((x0.y) / (sqrt(sum y^2) + 1e-10f)) / n0     e = expf(s)
//   acc = (init ? 0 : acc) + e * y     z = (init ? 0 : z) + e     e_out = e
// and k_row_divide's acc / z after the last hop makes the weights the softmax over the hops (|s| <= 1,
// so no maximum is subtracted and no hop waits for the others).  With hop0, y is hop 0 itself: x0 is
// not read (x0.y is sum y^2, the same fmas) and n0 = sqrt(sum y^2) + 1e-10f is written.
//
// S = 2^lgS lanes per row (the power of two >= the row's VEC-chunks, at most 64), 64 / S rows per
// wave step; lane c0 of a row takes chunks c0, c0 + S, ...  Each lane folds its elements into the
// two dot products in that order with fmas, the S partials are added in an xor butterfly (both
// partners add the same two values, so every lane holds the same sum): a row's bits depend on d
// and VEC only, never on the grid, n_rows or the wave that got the row.  HOLD: the row fits
// kSimChunks chunks per lane (d <= 256 * VEC), so y, x0 and acc stay in registers between the
// reduction and the accumulate -- 4 panel passes.  Wider rows (!HOLD) read y a second time.
// ------------------------------------------------------------------------------------------------
constexpr int kSimChunks = 4;

template <int VEC, bool HOLD>
__global__ void __launch_bounds__(256)
k_hop_simweight(const float* __restrict__ x0, int64_t ldx0, const float* __restrict__ y, int64_t ldy,
                float* __restrict__ n0, float* __restrict__ acc, int64_t lda, float* __restrict__ z,
                float* __restrict__ e_out, int64_t lde, int64_t n_rows, int cpr, int lgS, bool init, bool hop0)
{
    typedef typename Vec<float, VEC>::type V;
    constexpr int C = kSimChunks;
    const RowLanes rl(lgS, blockDim.x);
    const int S = rl.S, c0 = rl.c0;
    // every lane of the wave runs every step (the butterfly reads its partners); rows past the end load nothing
    for (int64_t base = rl.first; base < n_rows; base += rl.stride) {
        const int64_t r = base + rl.g;
        const bool live = r < n_rows;
        const float* yr = y + r * ldy;
        const float* xr = hop0 ? yr : x0 + r * ldx0;
        float* ar = acc + r * lda;
        V yv[C], xv[C], av[C];
        float dot = 0.0f, ny = 0.0f;
        if constexpr (HOLD) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int c = c0 + i * S;
                if (live && c < cpr) {
                    yv[i] = vload<float, VEC>(yr + (int64_t)c * VEC);
                    if (!hop0) xv[i] = vload<float, VEC>(xr + (int64_t)c * VEC);
                    if (!init) av[i] = vload<float, VEC>(ar + (int64_t)c * VEC);
                }
            }
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int c = c0 + i * S;
                if (live && c < cpr) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float yj = elem(yv[i], j);
                        ny = __builtin_fmaf(yj, yj, ny);
                        if (!hop0) dot = __builtin_fmaf(elem(xv[i], j), yj, dot);
                    }
                }
            }
        } else {
            for (int c = c0; live && c < cpr; c += S) {
                const V yc = vload<float, VEC>(yr + (int64_t)c * VEC);
                V xc = yc;
                if (!hop0) xc = vload<float, VEC>(xr + (int64_t)c * VEC);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float yj = elem(yc, j);
                    ny = __builtin_fmaf(yj, yj, ny);
                    if (!hop0) dot = __builtin_fmaf(elem(xc, j), yj, dot);
                }
            }
        }
        butterfly_add(S, ny, dot);
        if (hop0) dot = ny;
        const float norm = __fadd_rn(__fsqrt_rn(ny), 1e-10f);
        const float nr = hop0 ? norm : (live ? n0[r] : 1.0f);
        const float e = expf(__fdiv_rn(__fdiv_rn(dot, norm), nr));
        if (live && c0 == 0) {
            if (hop0) n0[r] = norm;
            z[r] = init ? e : __fadd_rn(z[r], e);
            if (e_out) e_out[r * lde] = e;
        }
        if constexpr (HOLD) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int c = c0 + i * S;
                if (live && c < cpr) {
                    V o;
#pragma unroll
                    for (int j = 0; j < VEC; ++j)
                        elem(o, j) = __fadd_rn(init ? 0.0f : elem(av[i], j), __fmul_rn(e, elem(yv[i], j)));
                    vstore<float, VEC>(ar + (int64_t)c * VEC, o, false);
                }
            }
        } else {
            for (int c = c0; live && c < cpr; c += S) {
                const V yc = vload<float, VEC>(yr + (int64_t)c * VEC);
                V o;
                if (!init) o = vload<float, VEC>(ar + (int64_t)c * VEC);
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    elem(o, j) = __fadd_rn(init ? 0.0f : elem(o, j), __fmul_rn(e, elem(yc, j)));
                vstore<float, VEC>(ar + (int64_t)c * VEC, o, false);
            }
        }
    }
}

// acc[r, :] = acc[r, :] / z[r] (correctly rounded): the NAFS weights' softmax denominator
__global__ void __launch_bounds__(256)
k_row_divide(float* __restrict__ acc, int64_t lda, const float* __restrict__ z, int64_t n_rows, int d)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_rows; r += waves) {
        float* a = acc + r * lda;
        const float zr = z[r];
        for (int c = lane; c < d; c += 64) a[c] = __fdiv_rn(a[c], zr);
    }
}

// Row gather (the send-side pack of the halo exchange, srgnn.dist): dst[i, :] = src[idx[i], :].
// S lanes per row (the power of two >= the row's VEC-chunks, at most 64), 64 / S rows per wave
// step and U = 4 steps in flight: 16-byte loads at d = 128 are 2 rows per wave-instruction, 8 rows
// per wave in flight.  Indices outside [0, n_src) leave their dst row unwritten (never a fault).
template <int VEC, int S>
__global__ void __launch_bounds__(256)
k_gather_rows(const float* __restrict__ src, int64_t lds, int64_t n_src, const int64_t* __restrict__ idx,
              int64_t n_idx, float* __restrict__ dst, int64_t ldd, int cpr)
{
    typedef typename Vec<float, VEC>::type V;
    constexpr int R = 64 / S, U = 4;
    const int lane = threadIdx.x & 63;
    const int g = lane / S, c0 = lane % S;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = wave * (R * U); base < n_idx; base += waves * (R * U)) {
        int64_t sr[U], dr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            dr[u] = base + u * R + g;
            sr[u] = dr[u] < n_idx ? idx[dr[u]] : -1;
            if (sr[u] >= n_src) sr[u] = -1;
        }
        for (int c = c0; c < cpr; c += S) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (sr[u] >= 0) v[u] = vload<float, VEC>(src + sr[u] * lds + (int64_t)c * VEC);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (sr[u] >= 0) vstore<float, VEC>(dst + dr[u] * ldd + (int64_t)c * VEC, v[u], false);
        }
    }
}

// torch's multi_row_sum (ATen/native/cpu/SumKernel.cpp) for one element over `count` rows of the
// tail history, rows start, start + stride, ...: 16-row blocks folded into 4 levels.
__device__ float torch_multi_row_sum(const float* hist, int start, int stride, int count, int e)
{
    int clog2 = 1;
    if (count > 2) clog2 = 32 - __clz(count - 1);
    const int lp = clog2 / 4 > 4 ? clog2 / 4 : 4;
    const int step = 1 << lp, mask = step - 1;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int i = 0;
    while (i + step <= count) {
        for (int j = 0; j < step; ++j, ++i)
            acc[0] = __fadd_rn(acc[0], hist[(int64_t)(start + i * stride) * SRG_TAIL_MAX + e]);
        for (int j = 1; j < 4; ++j) {
            acc[j] = __fadd_rn(acc[j], acc[j - 1]);
            acc[j - 1] = 0.0f;
            if ((i & (mask << (j * lp))) != 0) break;
        }
    }
    for (; i < count; ++i) acc[0] = __fadd_rn(acc[0], hist[(int64_t)(start + i * stride) * SRG_TAIL_MAX + e]);
    for (int j = 1; j < 4; ++j) acc[0] = __fadd_rn(acc[0], acc[j]);
    return acc[0];
}

// hist[term][e] = w * y[flat_start + e] (the rounded products of one hop's tail elements)
__global__ void k_tail_record(float* __restrict__ hist, const float* __restrict__ y, int64_t ldy, int d,
                              int64_t flat_start, int len, float w)
{
    const int e = threadIdx.x;
    if (e >= len) return;
    const int64_t f = flat_start + e;
    hist[e] = __fmul_rn(w, y[(f / d) * ldy + f % d]);
}

// torch's row_sum (4 interleaved partial sums, remainder into the first, then folded) over the
// recorded terms, stored as out = 0 + sum
__global__ void k_tail_rowsum(float* __restrict__ agg, int64_t lda, int d, int64_t flat_start, int len,
                              const float* __restrict__ hist, int n_terms)
{
    const int e = threadIdx.x;
    if (e >= len) return;
    const int n4 = n_terms / 4;
    float p[4];
    for (int c = 0; c < 4; ++c) p[c] = torch_multi_row_sum(hist, c, 4, n4, e);
    for (int i = 4 * n4; i < n_terms; ++i) p[0] = __fadd_rn(p[0], hist[(int64_t)i * SRG_TAIL_MAX + e]);
    for (int c = 1; c < 4; ++c) p[0] = __fadd_rn(p[0], p[c]);
    const int64_t f = flat_start + e;
    agg[(f / d) * lda + f % d] = __fadd_rn(0.0f, p[0]);
}

}  // namespace

extern "C" {

int srg_hop_accumulate_f32(float* agg, int64_t lda, const float* y, int64_t ldy, int64_t n_rows,
                           int32_t d, float w, int mode, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    const bool select = mode == SRG_ACC_COPY || mode == SRG_ACC_MIN || mode == SRG_ACC_MAX;
    if (mode != SRG_ACC_INIT && mode != SRG_ACC_ADD && mode != SRG_ACC_DIV && !select)
        return srg_fail(SRG_ERR_INVALID, "accumulate mode %d", mode);
    if (n_rows < 0 || d < 0 || lda < d || (mode != SRG_ACC_DIV && ldy < d))
        return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d lda=%lld ldy=%lld", (long long)n_rows, d,
                        (long long)lda, (long long)ldy);
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!agg || (mode != SRG_ACC_DIV && !y)) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 256 * 16);
    if (select)
        hipLaunchKernelGGL(k_hop_select, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                           agg, lda, y, ldy, n_rows, d, mode);
    else
        hipLaunchKernelGGL(k_hop_accumulate, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                           agg, lda, y, ldy, n_rows, d, w, mode);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_hop_simweight_f32(const float* x0, int64_t ldx0, const float* y, int64_t ldy, float* n0, float* acc,
                          int64_t lda, float* z, float* e_out, int64_t lde, int64_t n_rows, int32_t d,
                          uint32_t flags, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (flags & ~(uint32_t)(SRG_SIM_INIT | SRG_SIM_HOP0))
        return srg_fail(SRG_ERR_INVALID, "simweight flags 0x%x", flags);
    const bool init = (flags & SRG_SIM_INIT) != 0, hop0 = (flags & SRG_SIM_HOP0) != 0;
    if (n_rows < 0 || d < 0 || ldy < d || lda < d || (!hop0 && ldx0 < d) || (e_out && lde < 1))
        return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d ldx0=%lld ldy=%lld lda=%lld lde=%lld",
                        (long long)n_rows, d, (long long)ldx0, (long long)ldy, (long long)lda, (long long)lde);
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!y || !n0 || !acc || !z || (!hop0 && !x0)) return srg_fail(SRG_ERR_INVALID, "null pointer");
    if (acc == y || (!hop0 && acc == x0)) return srg_fail(SRG_ERR_INVALID, "acc must not alias a hop panel");
    // the widest access every row of every panel is aligned for (pick_vec's d thresholds are the
    // SpMM's tile widths; a streaming pass takes 16 bytes per lane from d = 4)
    int vec = 1;
    for (int v = 4; v > 1 && vec == 1; v >>= 1)   // x0 is not read at hop 0
        if (rows_aligned(v, sizeof(float), d, {{y, ldy}, {acc, lda}}) &&
            (hop0 || rows_aligned(v, sizeof(float), d, {{x0, ldx0}})))
            vec = v;
    const int cpr = d / vec;
    const auto [lgS, blocks] = row_lanes_grid(cpr, n_rows);
    const bool hold = cpr <= (kSimChunks << lgS);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SRG_SIMWEIGHT(V, H) hipLaunchKernelGGL((k_hop_simweight<V, H>), dim3(blocks), dim3(256), 0, st, x0, ldx0, y, \
                                               ldy, n0, acc, lda, z, e_out, lde, n_rows, cpr, lgS, init, hop0)
    if (vec == 4) {
        if (hold) SRG_SIMWEIGHT(4, true); else SRG_SIMWEIGHT(4, false);
    } else if (vec == 2) {
        if (hold) SRG_SIMWEIGHT(2, true); else SRG_SIMWEIGHT(2, false);
    } else {
        if (hold) SRG_SIMWEIGHT(1, true); else SRG_SIMWEIGHT(1, false);
    }
#undef SRG_SIMWEIGHT
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_row_divide_f32(float* acc, int64_t lda, const float* z, int64_t n_rows, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0 || d < 0 || lda < d)
        return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d lda=%lld", (long long)n_rows, d, (long long)lda);
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!acc || !z) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 256 * 16);
    hipLaunchKernelGGL(k_row_divide, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), acc, lda, z,
                       n_rows, d);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_tail_record_f32(float* hist, const float* y, int64_t ldy, int32_t d, int64_t flat_start,
                        int32_t len, float w, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (d <= 0 || ldy < d || flat_start < 0 || len < 0 || len > SRG_TAIL_MAX)
        return srg_fail(SRG_ERR_INVALID, "bad tail d=%d ldy=%lld flat_start=%lld len=%d", d, (long long)ldy,
                        (long long)flat_start, len);
    if (len == 0) return srg_ok();
    if (!hist || !y) return srg_fail(SRG_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL(k_tail_record, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                       hist, y, ldy, d, flat_start, len, w);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_tail_rowsum_f32(float* agg, int64_t lda, int32_t d, int64_t flat_start, int32_t len,
                        const float* hist, int32_t n_terms, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (d <= 0 || lda < d || flat_start < 0 || len < 0 || len > SRG_TAIL_MAX || n_terms < 0)
        return srg_fail(SRG_ERR_INVALID, "bad tail d=%d lda=%lld flat_start=%lld len=%d n_terms=%d", d,
                        (long long)lda, (long long)flat_start, len, n_terms);
    if (len == 0) return srg_ok();
    if (!agg || (n_terms > 0 && !hist)) return srg_fail(SRG_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL(k_tail_rowsum, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                       agg, lda, d, flat_start, len, hist, n_terms);
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

int srg_gather_rows_f32(const float* src, int64_t lds, int64_t n_src, const int64_t* idx, int64_t n_idx,
                        float* dst, int64_t ldd, int32_t d, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_idx < 0 || n_src < 0 || d < 0 || (d > 0 && (lds < d || ldd < d)))
        return srg_fail(SRG_ERR_INVALID, "bad gather shape n_idx=%lld n_src=%lld d=%d lds=%lld ldd=%lld",
                        (long long)n_idx, (long long)n_src, d, (long long)lds, (long long)ldd);
    if (n_idx == 0 || d == 0) return srg_ok();
    if (!src || !idx || !dst) return srg_fail(SRG_ERR_INVALID, "null pointer");
    const int vec = pick_vec(d, lds, ldd, src, dst, sizeof(float));
    const int cpr = d / vec;
    const int S = cpr >= 64 ? 64 : cpr > 16 ? 32 : cpr > 8 ? 16 : cpr > 4 ? 8 : 4;
    const int64_t rows_per_block = (int64_t)(256 / 64) * (64 / S) * 4;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_idx + rows_per_block - 1) / rows_per_block, 256 * 64);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SRG_GATHER(V, SS) hipLaunchKernelGGL((k_gather_rows<V, SS>), dim3(blocks), dim3(256), 0, st, src, lds, n_src, \
                                             idx, n_idx, dst, ldd, cpr)
#define SRG_GATHER_S(V)                          \
    if (S == 64) SRG_GATHER(V, 64);              \
    else if (S == 32) SRG_GATHER(V, 32);         \
    else if (S == 16) SRG_GATHER(V, 16);         \
    else if (S == 8) SRG_GATHER(V, 8);           \
    else SRG_GATHER(V, 4);
    if (vec == 4) {
        SRG_GATHER_S(4)
    } else if (vec == 2) {
        SRG_GATHER_S(2)
    } else {
        SRG_GATHER_S(1)
    }
#undef SRG_GATHER_S
#undef SRG_GATHER
    SRG_HIP_CHECK(hipGetLastError());
    return srg_ok();
}

}  // extern "C"
