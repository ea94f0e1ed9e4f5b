// srg_wavconv.hip -- the graph-wavelet filter Y = phi * (theta (.) (phi^-1 * Z)) and its adjoints on
// MI355X (gfx950), without ever forming phi * diag(theta) * phi^-1.
//
// The reference's wavelet layers (wavelet/src/gwnn_layer.py) build that n x n product with two spspmm
// calls per forward and multiply it into an [n, d] panel with spmm; it is close to dense whatever the
// sparsity of phi.  Re-associated, the layer is two sparse-times-dense products over the bases' own
// entries and its backward three more, all on narrow panels (d = hidden 16, classes 7):
//
//   srg_spmm_scaled_f32     Y[r, j] = chain over row r, stored order, of fl(fl(v * scale) * X[c, j])
//   srg_sddmm_rowsum_f32    out[k]  = chain over row k, stored order, of fl(v * s_e),
//                           s_e = chain over j ascending of fl(G[c, j] * P[k, j])
//
// Every chain starts from +0, every product is rounded before it is added (the library is built with
// -ffp-contract=off and the kernels spell __fmul_rn / __fadd_rn), one output element is one sequential
// chain owned by one lane, and nothing is added atomically: run-to-run identical.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "srg_internal.h"
#include "srgnn_hip.h"

namespace {

constexpr int kWave = 64;
// entries of a row that its lane group loads at once (id, value and, per column, the scale)
constexpr int kChunk = 16;

// One row per group of W lanes (W = the power of two >= d, at most 64), 64 / W rows per wave, lane l of
// a group owning column c0 + l: at d = 16 a wave runs four rows and every lane works, where a wave per
// row (k_spmm_muladd) leaves 48 lanes idle; a gather of one entry reads 4 * W contiguous bytes.
//  * The group's first min(W, 16) lanes load the next 16 entries' (id, value) at once -- 16 / W entries
//    per lane when the group is narrower than 16 -- and hand them out by ds_bpermute, so the only
//    dependent load per entry is the gather itself (k_spmm_muladd: id -> X, one entry at a time).
//  * The next 16 entries load behind the current 16 gathers; with a column scale, scale[id] is issued
//    after those gathers and the rescale fl(v * scale) is done once per entry by the lane that loaded
//    it, when the chunk becomes current.
//  * The 16 gathers of a chunk are issued together, then the 16 links of the chain run in stored
//    order; entries past the row's end load nothing and are skipped (never folded in as 0 * x).
//  * d > 64: one wave per row, the row walked once per 64-column piece.
// A row holds fewer than 2^31 entries.
template <int W>
__global__ __launch_bounds__(256) void k_spmm_scaled(const int64_t* __restrict__ ip, const int32_t* __restrict__ ix,
                                                     const float* __restrict__ vv, const float* __restrict__ scale,
                                                     int axis, int64_t n_rows, const float* __restrict__ X,
                                                     int64_t ldx, float* __restrict__ Y, int64_t ldy, int d)
{
    constexpr int RPW = kWave / W;                          // rows per wave
    constexpr int CW = W < kChunk ? W : kChunk;             // lanes of a group that load entries
    constexpr int K = kChunk / CW;                          // entries each of them loads
    const int lane = threadIdx.x & 63;
    const int g0 = lane & ~(W - 1), l = lane & (W - 1);
    const int64_t r = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / W;
    const bool rv = r < n_rows;
    int64_t beg = 0;
    int len = 0;
    if (rv) {
        beg = ip[r];
        len = (int)(ip[r + 1] - beg);
    }
    int maxlen = len;
#pragma unroll
    for (int off = W; off < kWave; off <<= 1) {
        const int o = __shfl_xor(maxlen, off, kWave);
        maxlen = o > maxlen ? o : maxlen;
    }
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    const bool col_scale = scale && axis == 0;
    const float row_scale = (scale && axis == 1 && rv) ? scale[r] : 0.0f;

    auto load = [&](int j0, int (&id)[K], float (&a)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = j0 + k * CW + l;
            const bool ok = l < CW && e < len;
            const int64_t p = beg + (ok ? e : 0);
            id[k] = ok ? ix[p] : 0;
            a[k] = ok ? vv[p] : 0.0f;
        }
    };
    auto load_scale = [&](int j0, const int (&id)[K], float (&sc)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool ok = l < CW && j0 + k * CW + l < len;
            sc[k] = col_scale ? (ok ? scale[id[k]] : 0.0f) : row_scale;
        }
    };

    for (int c0 = 0; c0 < d; c0 += kWave) {                 // one piece unless d > 64
        const int c = c0 + l;
        const bool cv = c < d;
        float s = 0.0f;
        int id[K], nid[K];
        float a[K], na[K], nsc[K];
        if (maxlen > 0) {
            load(0, nid, na);
            if (scale) load_scale(0, nid, nsc);
        }
        for (int j0 = 0; j0 < maxlen; j0 += kChunk) {
#pragma unroll
            for (int k = 0; k < K; ++k) {                   // the loaded chunk becomes the current one
                id[k] = nid[k];
                a[k] = scale ? __fmul_rn(na[k], nsc[k]) : na[k];
            }
            const bool more = j0 + kChunk < maxlen;
            if (more) load(j0 + kChunk, nid, na);
            float x[kChunk], av[kChunk];
#pragma unroll
            for (int t = 0; t < kChunk; ++t) {
                const int cc = W == 1 ? id[t / CW] : __shfl(id[t / CW], g0 + t % CW, kWave);
                av[t] = W == 1 ? a[t / CW] : __shfl(a[t / CW], g0 + t % CW, kWave);
                x[t] = (cv && j0 + t < len) ? X[(int64_t)cc * ldx + c] : 0.0f;
            }
            if (more && scale) load_scale(j0 + kChunk, nid, nsc);
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (j0 + t < len) s = __fadd_rn(s, __fmul_rn(av[t], x[t]));
        }
        if (rv && cv) Y[r * ldy + c] = s;
    }
}

// out[k] for one row k per wave: the lanes take 64 of the row's entries at a time, each lane running the
// whole column chain s_e of its entry, then the row's ordered sum of fl(v_e * s_e) is taken in entry
// order by reading the 64 products back from LDS, and carried across the row's tiles.
//  * G's gathered rows are staged kRsTile columns at a time into the wave's LDS tile: the staging loop
//    walks (row, column) pairs with the tile's width rounded up to a power of two, so consecutive lanes
//    read consecutive columns of a row (64-byte runs at d = 16) however narrow the panel is; a lane then
//    reads its own row at stride kRsLd = 33 dwords: the 32 lanes of each ds_read_b32 group hit 32
//    different banks.
//  * P's row is shared by every lane of the row: staged once per tile, read as an LDS broadcast.
constexpr int kRsTile = 32;
constexpr int kRsLd = kRsTile + 1;

__global__ __launch_bounds__(kWave) void k_sddmm_rowsum(const int64_t* __restrict__ ip, const int32_t* __restrict__ ix,
                                                        const float* __restrict__ vv, const float* __restrict__ G,
                                                        int64_t ldg, const float* __restrict__ P, int64_t ldp,
                                                        int d, float* __restrict__ out)
{
    __shared__ float tile[kWave * kRsLd];
    __shared__ float prow[kRsTile];
    __shared__ float prod[kWave];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    const int64_t e0 = ip[k], e1 = ip[k + 1];
    const float* __restrict__ p = P + k * ldp;
    float acc = 0.0f;                                       // the same in every lane
    for (int64_t b = e0; b < e1; b += kWave) {
        const int cnt = e1 - b < kWave ? (int)(e1 - b) : kWave;
        const bool live = lane < cnt;
        const int32_t c = live ? ix[b + lane] : 0;
        const float v = live ? vv[b + lane] : 0.0f;
        float s = 0.0f;
        for (int c0 = 0; c0 < d; c0 += kRsTile) {
            const int w = d - c0 < kRsTile ? d - c0 : kRsTile;
            const int sh = w > 1 ? 32 - __builtin_clz(w - 1) : 0;      // the tile's width as 2^sh >= w
            const int cells = cnt << sh;
            __syncthreads();                                // the previous tile has been read
            for (int base = 0; base < cells; base += kWave) {           // wave-uniform trip count
                const int idx = base + lane;
                const int row = idx >> sh, col = idx & ((1 << sh) - 1);  // row < 64
                const int32_t cr = __shfl(c, row, kWave);
                if (idx < cells && col < w) tile[row * kRsLd + col] = G[(int64_t)cr * ldg + c0 + col];
            }
            if (lane < w) prow[lane] = p[c0 + lane];
            __syncthreads();
            if (live) {
                const float* mine = &tile[lane * kRsLd];
                for (int j = 0; j < w; ++j) s = __fadd_rn(s, __fmul_rn(mine[j], prow[j]));
            }
        }
        __syncthreads();                                    // the previous tile's products have been read
        prod[lane] = __fmul_rn(v, s);
        __syncthreads();
        for (int i = 0; i < cnt; ++i) acc = __fadd_rn(acc, prod[i]);
    }
    if (lane == 0) out[k] = acc;
}

template <int W>
int launch_scaled(int64_t n_rows, hipStream_t s, const int64_t* ip, const int32_t* ix, const float* vv,
                  const float* scale, int axis, const float* X, int64_t ldx, float* Y, int64_t ldy, int d)
{
    constexpr int kRows = 4 * (kWave / W);                  // rows per 256-lane workgroup
    return launch_chunks_capped((n_rows + kRows - 1) / kRows, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        const int64_t r0 = b0 * kRows;
        hipLaunchKernelGGL(k_spmm_scaled<W>, dim3(nb), dim3(256), 0, s, ip + r0, ix, vv,
                           (scale && axis == 1) ? scale + r0 : scale, axis, n_rows - r0, X, ldx, Y + r0 * ldy, ldy,
                           d);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int srg_spmm_scaled_f32(const int64_t* indptr, const int32_t* indices, const float* values, const float* scale,
                        int32_t scale_axis, int64_t n_rows, const float* X, int64_t ldx, float* Y, int64_t ldy,
                        int32_t d, void* stream)
{
    if (n_rows < 0 || d < 0) return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d", (long long)n_rows, (int)d);
    if (ldx < d || ldy < d)
        return srg_fail(SRG_ERR_INVALID, "row stride ldx=%lld or ldy=%lld < d=%d", (long long)ldx, (long long)ldy,
                        (int)d);
    if (scale_axis != 0 && scale_axis != 1) return srg_fail(SRG_ERR_INVALID, "scale_axis %d", (int)scale_axis);
    if (n_rows == 0 || d == 0) return srg_ok();
    if (!indptr || !Y) return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define SRG_SCALED(W) launch_scaled<W>(n_rows, s, indptr, indices, values, scale, scale_axis, X, ldx, Y, ldy, d)
    int rc;
    if (d <= 1) rc = SRG_SCALED(1);
    else if (d <= 2) rc = SRG_SCALED(2);
    else if (d <= 4) rc = SRG_SCALED(4);
    else if (d <= 8) rc = SRG_SCALED(8);
    else if (d <= 16) rc = SRG_SCALED(16);
    else if (d <= 32) rc = SRG_SCALED(32);
    else rc = SRG_SCALED(64);
#undef SRG_SCALED
    return rc ? rc : srg_ok();
}

int srg_sddmm_rowsum_f32(const int64_t* indptr, const int32_t* indices, const float* values, int64_t n_rows,
                         const float* G, int64_t ldg, const float* P, int64_t ldp, int32_t d, float* out,
                         void* stream)
{
    if (n_rows < 0 || d < 0) return srg_fail(SRG_ERR_INVALID, "bad shape n_rows=%lld d=%d", (long long)n_rows, (int)d);
    if (ldg < d || ldp < d)
        return srg_fail(SRG_ERR_INVALID, "row stride ldg=%lld or ldp=%lld < d=%d", (long long)ldg, (long long)ldp,
                        (int)d);
    if (n_rows == 0) return srg_ok();
    if (!out || (d > 0 && (!indptr || !P))) return srg_fail(SRG_ERR_INVALID, "null pointer");
    SRG_DEVICE_GUARD(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d == 0) {                                           // every s_e is +0 and so is every row's sum
        SRG_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_rows * sizeof(float), s));
        return srg_ok();
    }
    const int rc = launch_chunks_capped(n_rows, kMaxLaunchWaveBlocks, [&](int64_t r0, unsigned nb) {   // a row per block
        hipLaunchKernelGGL(k_sddmm_rowsum, dim3(nb), dim3(kWave), 0, s, indptr + r0, indices, values, G, ldg,
                           P + r0 * ldp, ldp, d, out + r0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
