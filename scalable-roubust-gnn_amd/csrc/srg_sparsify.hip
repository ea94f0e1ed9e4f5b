// srg_sparsify.hip -- the wavelet basis built on the device: a dense fp64 filter block thresholded and
// compacted into CSR rows (count / fill), the blocks' rows appended into the final arrays (scipy's
// hstack(...).tocsr()) and sklearn's L1 row normalisation in place.  No atomics: every row has one
// owner wave (or lane group), so the results are the same bits run after run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// threshold + compact (SpectralModel.calculate_wavelet: sub[sub < tol] = 0; csr_matrix(sub.astype(float32)))
// ------------------------------------------------------------------------------------------------
// An entry survives iff it is not below the tolerance (a negated <, so a NaN entry or a NaN tolerance
// keeps it, as numpy's mask does) and its fp32 rounding is not zero (-0, and fp64 values that round to
// fp32 zero, are not stored by scipy; values that round to an fp32 subnormal are).
__device__ __forceinline__ bool survives(double v, double tol, float& f)
{
    f = (float)v;   // round to nearest even
    return !(v < tol) && f != 0.0f;
}

// One wave per row, VEC columns per lane and step: lane l holds columns c0 + VEC*l .. c0 + VEC*l + VEC-1
// of the step that starts at c0.  A survivor's slot in the row is the row's running count plus the
// survivors of the lanes below (two 64-lane ballots, first columns and second columns) plus, for a
// lane's second column, its own first: lane l's pair comes before lane l+1's, a lane's first column
// before its second -- columns ascending.  VEC = 2 reads 16 bytes per lane (row base and ldr even
// multiples of 8 bytes); a row's odd last column is read alone, never past the row.  FILL = false
// writes cnt[row], FILL = true the entries from ptr[row] on.
template <int VEC, bool FILL>
__global__ void __launch_bounds__(kBlock)
k_dense_sparsify(const double* __restrict__ R, int64_t ldr, int64_t n_rows, int w, double tol, int col0,
                 int64_t* __restrict__ cnt, const int64_t* __restrict__ ptr, int32_t* __restrict__ idx,
                 float* __restrict__ val, int64_t block_base)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (block_base + blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;   // wave-uniform
    const double* __restrict__ p = R + row * ldr;
    const unsigned long long below = (1ull << lane) - 1ull;
    int64_t base = 0;
    if constexpr (FILL) base = ptr[row];
    int64_t run = 0;
    for (int c0 = 0; c0 < w; c0 += 64 * VEC) {
        const int c = c0 + VEC * lane;
        double v0 = 0.0, v1 = 0.0;
        bool in0 = c < w, in1 = false;
        if constexpr (VEC == 2) {
            in1 = c + 1 < w;
            if (in1) {
                const typename Vec<double, 2>::type v = vload<double, 2>(p + c);
                v0 = v[0];
                v1 = v[1];
            } else if (in0) {
                v0 = p[c];
            }
        } else {
            if (in0) v0 = p[c];
        }
        float f0, f1 = 0.0f;
        const bool k0 = survives(v0, tol, f0) && in0;
        const unsigned long long m0 = __ballot(k0);
        int before = __popcll(m0 & below);
        int total = __popcll(m0);
        bool k1 = false;
        if constexpr (VEC == 2) {
            k1 = survives(v1, tol, f1) && in1;
            const unsigned long long m1 = __ballot(k1);
            before += __popcll(m1 & below);
            total += __popcll(m1);
        }
        if constexpr (FILL) {
            const int64_t o = base + run + before;
            if (k0) {
                idx[o] = col0 + c;
                val[o] = f0;
            }
            if (k1) {
                idx[o + (k0 ? 1 : 0)] = col0 + c + 1;
                val[o + (k0 ? 1 : 0)] = f1;
            }
        }
        run += total;
    }
    if constexpr (!FILL) {
        if (lane == 0) cnt[row] = run;
    }
}

// ------------------------------------------------------------------------------------------------
// append (sp.hstack(blocks).tocsr(): a row's entries follow block order)
// ------------------------------------------------------------------------------------------------
// Packed rows: a wave takes 4 consecutive rows, 16 lanes each (basis rows hold one to a few dozen
// entries per block: Cora 1 / 4.9 per row over three blocks); a row of more than kAppendShort entries
// is then copied by the whole wave, 64 entries per step.  The row's lanes read cursor[r] before its
// first lane advances it (one wave, program order); no other wave touches the row.
constexpr int64_t kAppendShort = 64;

__global__ void __launch_bounds__(kBlock)
k_csr_append_rows(const int64_t* __restrict__ src_ptr, const int32_t* __restrict__ src_idx,
                  const float* __restrict__ src_val, int64_t n_rows, int64_t* cursor,
                  int32_t* __restrict__ dst_idx, float* __restrict__ dst_val, int64_t block_base)
{
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t wave = (block_base + blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t r = wave * 4 + (lane >> 4);
    const bool valid = r < n_rows;
    const int64_t b = valid ? src_ptr[r] : 0;
    const int64_t len = valid ? src_ptr[r + 1] - b : 0;
    const int64_t pos = valid ? cursor[r] : 0;
    const bool wide = len > kAppendShort;
    if (!wide) {
        for (int64_t k = sub; k < len; k += 16) {
            dst_idx[pos + k] = src_idx[b + k];
            dst_val[pos + k] = src_val[b + k];
        }
    }
    unsigned long long todo = __ballot(wide && sub == 0);   // wave-uniform
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t wb = bcast_lane(b, l), wlen = bcast_lane(len, l), wpos = bcast_lane(pos, l);
        for (int64_t k = lane; k < wlen; k += 64) {
            dst_idx[wpos + k] = src_idx[wb + k];
            dst_val[wpos + k] = src_val[wb + k];
        }
    }
    if (valid && sub == 0) cursor[r] = pos + len;
}

// ------------------------------------------------------------------------------------------------
// L1 row normalisation (sklearn's _inplace_csr_row_normalize_l1)
// ------------------------------------------------------------------------------------------------
// One wave per 64 consecutive rows, as k_segment_sum (srg_csr.hip).  A row of at most kNormShort
// entries belongs to its lane: the fp64 sum of |x| left to right from +0, then x / sum in fp64
// rounded to fp32, skipped when the sum is 0 (a NaN sum is != 0: the row becomes NaN).  A longer row
// is taken by the whole wave: the values are read 64 at a time, the one sequential chain runs over
// them through v_readlane (every lane carries the same sum), and the divide runs 64 entries per step.
constexpr int64_t kNormShort = 64;

__global__ void __launch_bounds__(kBlock)
k_csr_row_normalize_l1(const int64_t* __restrict__ indptr, float* values, int64_t n_rows, int64_t block_base)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (block_base + blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (wave * 64 >= n_rows) return;   // wave-uniform
    const int64_t r = wave * 64 + lane;
    const bool valid = r < n_rows;
    const int64_t beg = valid ? indptr[r] : 0;
    const int64_t end = valid ? indptr[r + 1] : 0;
    const bool wide = end - beg > kNormShort;
    if (!wide) {
        double acc = 0.0;
        for (int64_t j = beg; j < end; ++j) acc = e_add(acc, __builtin_fabs((double)values[j]));
        if (acc != 0.0)
            for (int64_t j = beg; j < end; ++j) values[j] = (float)e_div((double)values[j], acc);
    }
    unsigned long long todo = __ballot(wide);   // wave-uniform
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t b = bcast_lane(beg, l), e = bcast_lane(end, l);
        double acc = 0.0;
        for (int64_t jb = b; jb < e; jb += 64) {
            const int64_t j = jb + lane;
            const double a = j < e ? __builtin_fabs((double)values[j]) : 0.0;
            const int nb = (e - jb) < 64 ? (int)(e - jb) : 64;   // wave-uniform
            for (int q = 0; q < nb; ++q) acc = e_add(acc, bcast_lane(a, q));
        }
        if (acc != 0.0)   // wave-uniform
            for (int64_t j = b + lane; j < e; j += 64) values[j] = (float)e_div((double)values[j], acc);
    }
}

template <int VEC>
void launch_sparsify(int phase, dim3 grid, hipStream_t s, const double* R, int64_t ldr, int64_t n_rows, int w,
                     double tol, int col0, int64_t* cnt, const int64_t* ptr, int32_t* idx, float* val, int64_t b0)
{
    if (phase == 0)
        hipLaunchKernelGGL((k_dense_sparsify<VEC, false>), grid, dim3(kBlock), 0, s, R, ldr, n_rows, w, tol, col0,
                           cnt, ptr, idx, val, b0);
    else
        hipLaunchKernelGGL((k_dense_sparsify<VEC, true>), grid, dim3(kBlock), 0, s, R, ldr, n_rows, w, tol, col0,
                           cnt, ptr, idx, val, b0);
}

}  // namespace

extern "C" {

int srg_dense_sparsify_f64(int phase, const double* R, int64_t ldr, int64_t n_rows, int32_t w, double tolerance,
                           int32_t col0, int64_t* cnt, const int64_t* ptr, int32_t* idx, float* val, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (phase != 0 && phase != 1) return srg_fail(SRG_ERR_INVALID, "phase=%d not 0 (count) or 1 (fill)", phase);
    if (n_rows < 0 || w < 0) return srg_fail(SRG_ERR_INVALID, "n_rows=%lld, w=%d: negative size", (long long)n_rows, w);
    if (ldr < w) return srg_fail(SRG_ERR_INVALID, "leading dimension ldr=%lld < w=%d", (long long)ldr, w);
    if (col0 < 0 || (int64_t)col0 + w > INT32_MAX)
        return srg_fail(SRG_ERR_INVALID, "column ids col0=%d .. col0+w=%lld outside int32", col0, (long long)col0 + w);
    if (n_rows == 0 || w == 0) return srg_ok();
    if (!R || (phase == 0 ? !cnt : !ptr)) return srg_fail(SRG_ERR_INVALID, "null R, cnt (phase 0) or ptr (phase 1)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 16-byte loads where every row starts on 16 bytes; else 8-byte loads, the same bits
    // (whatever w is: the kernel takes a row's odd last column by itself)
    const bool vec2 = rows_aligned(2, sizeof(double), 0, {{R, ldr}});
    const int64_t blocks = (n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
    const int rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        if (vec2)
            launch_sparsify<2>(phase, dim3(nb), s, R, ldr, n_rows, w, tolerance, col0, cnt, ptr, idx, val, b0);
        else
            launch_sparsify<1>(phase, dim3(nb), s, R, ldr, n_rows, w, tolerance, col0, cnt, ptr, idx, val, b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_csr_append_rows_f32(const int64_t* src_ptr, const int32_t* src_idx, const float* src_val, int64_t n_rows,
                            int64_t* cursor, int32_t* dst_idx, float* dst_val, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0) return srg_fail(SRG_ERR_INVALID, "n_rows=%lld < 0", (long long)n_rows);
    if (n_rows == 0) return srg_ok();
    if (!src_ptr || !cursor) return srg_fail(SRG_ERR_INVALID, "null src_ptr or cursor");
    const int64_t rows_per_block = 4 * kWavesPerBlock;
    const int64_t blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    const int rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_csr_append_rows, dim3(nb), dim3(kBlock), 0, static_cast<hipStream_t>(stream), src_ptr,
                           src_idx, src_val, n_rows, cursor, dst_idx, dst_val, b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

int srg_csr_row_normalize_l1_f32(const int64_t* indptr, float* values, int64_t n_rows, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_rows < 0) return srg_fail(SRG_ERR_INVALID, "n_rows=%lld < 0", (long long)n_rows);
    if (n_rows == 0) return srg_ok();
    if (!indptr) return srg_fail(SRG_ERR_INVALID, "null indptr");
    const int64_t rows_per_block = 64 * kWavesPerBlock;
    const int64_t blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    const int rc = launch_chunks_capped(blocks, kMaxLaunchBlocks, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(k_csr_row_normalize_l1, dim3(nb), dim3(kBlock), 0, static_cast<hipStream_t>(stream), indptr,
                           values, n_rows, b0);
        return launch_status();
    });
    return rc ? rc : srg_ok();
}

}  // extern "C"
