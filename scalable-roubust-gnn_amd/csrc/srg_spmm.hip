// srg_spmm.hip -- the fp32 product's entry points: the SpMM kernels of srg_spmm_kernels.h with the
// plain and span epilogues (the fused hop aggregation included), SRG_SPMM_FAST's hub segments, the
// K-hop loops over a schedule or a plan's launches, and the host-buffer product behind the reference's
// FloatCSRMulDenseOMP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "srgnn_hip.h"
#include "srg_internal.h"
#include "srg_plan_internal.h"
#include "srg_spmm_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------
// SRG_SPMM_FAST: the hub rows as kFastSegs segments each.  Segment s of hub row h (row order[h]) is
// entries [b + len*s/S, b + len*(s+1)/S) of the row -- a row span -- computed as an exact fma
// chain by the slice waves of the span kernel into a scratch panel; the S partial sums of a row are
// then added in segment order.  Tolerance mode (the reference's single chain is re-associated into
// S pieces, deterministically); the longest row's latency drops ~S-fold.
// ------------------------------------------------------------------------------------------------
constexpr int kFastSegs = 64;

template <typename IP, bool SPAN>
__global__ __launch_bounds__(256) void k_fast_segments(const IP* __restrict__ indptr, const int64_t* __restrict__ row_end,
                                                       const int32_t* __restrict__ order, int64_t n_hub,
                                                       int64_t* __restrict__ seg_beg, int64_t* __restrict__ seg_end,
                                                       int32_t* __restrict__ seg_order)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hub * kFastSegs) return;
    const int64_t h = i / kFastSegs, sg = i % kFastSegs;
    const int r = order[h];
    const int64_t b = (int64_t)indptr[r];
    const int64_t e = SPAN ? row_end[r] : (int64_t)indptr[r + 1];
    const int64_t len = e - b;
    seg_beg[i] = b + len * sg / kFastSegs;
    seg_end[i] = b + len * (sg + 1) / kFastSegs;
    seg_order[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_fast_reduce(const int32_t* __restrict__ order, int64_t n_hub,
                                                     const float* __restrict__ part, int64_t ldp,
                                                     float* __restrict__ Y, int64_t ldy, int d, int acc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t h = i / d;
    const int c = (int)(i % d);
    if (h >= n_hub) return;
    float* y = Y + (int64_t)order[h] * ldy + c;
    float v = acc ? *y : 0.0f;
    const float* p = part + h * kFastSegs * ldp + c;
    for (int sg = 0; sg < kFastSegs; ++sg) v = __fadd_rn(v, p[sg * ldp]);
    *y = v;
}

template <typename IP, int EX>
int launch_fast_hubs(HubFork& hub, const IP* indptr, const int32_t* indices, const float* vals, const int32_t* order,
                     int64_t n_hub, const float* X, int64_t ldx, float* Y, int64_t ldy, int d, uint32_t flags,
                     const int64_t* row_end)
{
    if (int rc = hub.fork()) return rc;
    const int64_t T = n_hub * kFastSegs;
    const int64_t ldp = (d + 3) & ~3;
    const size_t idx_bytes = ((size_t)T * (2 * sizeof(int64_t) + sizeof(int32_t)) + 255) & ~(size_t)255;
    void* buf = nullptr;
    SRG_HIP_CHECK(hipMallocAsync(&buf, idx_bytes + (size_t)T * ldp * sizeof(float), hub.stream()));
    int64_t* seg_beg = static_cast<int64_t*>(buf);
    int64_t* seg_end = seg_beg + T;
    int32_t* seg_order = reinterpret_cast<int32_t*>(seg_end + T);
    float* part = reinterpret_cast<float*>(static_cast<char*>(buf) + idx_bytes);
    const unsigned gs = (unsigned)((T + 255) / 256);
    if (EX == kEpiSpan)
        hipLaunchKernelGGL((k_fast_segments<IP, true>), dim3(gs), dim3(256), 0, hub.stream(), indptr, row_end,
                           order, n_hub, seg_beg, seg_end, seg_order);
    else
        hipLaunchKernelGGL((k_fast_segments<IP, false>), dim3(gs), dim3(256), 0, hub.stream(), indptr, nullptr,
                           order, n_hub, seg_beg, seg_end, seg_order);
    SRG_HIP_CHECK(hipGetLastError());
    Epi se{};
    se.row_end = seg_end;
    // every segment a slice-wave row (exact chain over its span), no hubs (so no fork of its own), no
    // accumulation
    if (int rc = launch_spmm<int64_t, kEpiSpan>(seg_beg, indices, vals, T, seg_order, 0, T, X, ldx, part, ldp, d,
                                                flags & SRG_SPMM_PACKED_U2, hub.stream(), se))
        return rc;
    const unsigned gr = (unsigned)((n_hub * d + 255) / 256);
    hipLaunchKernelGGL(k_fast_reduce, dim3(gr), dim3(256), 0, hub.stream(), order, n_hub, part, ldp, Y, ldy, d,
                       (flags & SRG_SPMM_ACCUMULATE) ? 1 : 0);
    SRG_HIP_CHECK(hipGetLastError());
    SRG_HIP_CHECK(hipFreeAsync(buf, hub.stream()));
    return hub.record_join((flags & SRG_SPMM_HUB_NOJOIN) != 0);
}

// ------------------------------------------------------------------------------------------------
// host-compat staging: grow-only device buffers reused across calls (the reference calls the
// product once per hop from Python, utils.py:45)
// ------------------------------------------------------------------------------------------------
struct Staging {
    std::mutex mu;
    void* buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[5] = {0, 0, 0, 0, 0};
    int device[5] = {-1, -1, -1, -1, -1};
    hipStream_t stream = nullptr;
    int stream_device = -1;
};
Staging g_stage;

int stage_reserve(int slot, size_t bytes, int dev)
{
    if (g_stage.cap[slot] >= bytes && g_stage.device[slot] == dev) return SRG_OK;
    if (g_stage.buf[slot]) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(g_stage.device[slot]);
        (void)hipFree(g_stage.buf[slot]);
        (void)hipSetDevice(cur);
        g_stage.buf[slot] = nullptr;
        g_stage.cap[slot] = 0;
    }
    size_t want = std::max<size_t>(bytes, 256);
    if (hipMalloc(&g_stage.buf[slot], want) != hipSuccess) {
        g_stage.buf[slot] = nullptr;
        (void)hipGetLastError();
        return srg_fail(SRG_ERR_ALLOC, "hipMalloc(%zu) failed", want);
    }
    g_stage.cap[slot] = want;
    g_stage.device[slot] = dev;
    return SRG_OK;
}

// answer (+)= A * mat on the GPU with host buffers.  overwrite: cuSPARSE beta = 0 semantics.
int host_compat_spmm(float* answer, const float* data, const int* indices, const int* indptr,
                     const float* mat, int mat_row, int mat_col, bool overwrite, int64_t nnz_hint)
{
    if (mat_row < 0 || mat_col < 0)
        return srg_fail(SRG_ERR_INVALID, "mat_row=%d mat_col=%d", mat_row, mat_col);
    if (mat_row == 0 || mat_col == 0) return srg_ok();
    if (!answer || !indptr || !mat) return srg_fail(SRG_ERR_INVALID, "null host pointer");
    const int64_t nnz = indptr[mat_row];
    if (indptr[0] != 0 || nnz < 0) return srg_fail(SRG_ERR_INVALID, "indptr[0]=%d indptr[n]=%lld", indptr[0], (long long)nnz);
    if (nnz_hint >= 0 && nnz_hint != nnz)
        return srg_fail(SRG_ERR_INVALID, "data_nnz=%lld != indptr[mat_row]=%lld", (long long)nnz_hint, (long long)nnz);
    for (int i = 0; i < mat_row; ++i)
        if (indptr[i + 1] < indptr[i]) return srg_fail(SRG_ERR_INVALID, "indptr decreases at row %d", i);
    if (nnz > 0 && (!indices || !data)) return srg_fail(SRG_ERR_INVALID, "null indices/data");
    for (int64_t j = 0; j < nnz; ++j)
        if (indices[j] < 0 || indices[j] >= mat_row)
            return srg_fail(SRG_ERR_INVALID, "column id %d at %lld outside [0, %d)", indices[j], (long long)j, mat_row);

    std::lock_guard<std::mutex> lock(g_stage.mu);
    int dev = 0;
    SRG_HIP_CHECK(hipGetDevice(&dev));
    if (!g_stage.stream || g_stage.stream_device != dev) {
        SRG_HIP_CHECK(hipStreamCreateWithFlags(&g_stage.stream, hipStreamNonBlocking));
        g_stage.stream_device = dev;
    }
    hipStream_t s = g_stage.stream;
    const size_t panel = (size_t)mat_row * (size_t)mat_col * sizeof(float);
    int rc;
    if ((rc = stage_reserve(0, (size_t)(mat_row + 1) * sizeof(int), dev))) return rc;
    if ((rc = stage_reserve(1, (size_t)nnz * sizeof(int), dev))) return rc;
    if ((rc = stage_reserve(2, (size_t)nnz * sizeof(float), dev))) return rc;
    if ((rc = stage_reserve(3, panel, dev))) return rc;
    if ((rc = stage_reserve(4, panel, dev))) return rc;
    int* d_ptr = static_cast<int*>(g_stage.buf[0]);
    int* d_idx = static_cast<int*>(g_stage.buf[1]);
    float* d_val = static_cast<float*>(g_stage.buf[2]);
    float* d_x = static_cast<float*>(g_stage.buf[3]);
    float* d_y = static_cast<float*>(g_stage.buf[4]);
    SRG_HIP_CHECK(hipMemcpyAsync(d_ptr, indptr, (size_t)(mat_row + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        SRG_HIP_CHECK(hipMemcpyAsync(d_idx, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        SRG_HIP_CHECK(hipMemcpyAsync(d_val, data, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, s));
    }
    SRG_HIP_CHECK(hipMemcpyAsync(d_x, mat, panel, hipMemcpyHostToDevice, s));
    uint32_t flags = 0;
    if (!overwrite) {
        SRG_HIP_CHECK(hipMemcpyAsync(d_y, answer, panel, hipMemcpyHostToDevice, s));
        flags |= SRG_SPMM_ACCUMULATE;
    }
    rc = launch_spmm<int>(d_ptr, d_idx, d_val, mat_row, nullptr, 0, 0, d_x, mat_col, d_y, mat_col, mat_col, flags, s);
    if (rc) return rc;
    SRG_HIP_CHECK(hipMemcpyAsync(answer, d_y, panel, hipMemcpyDeviceToHost, s));
    SRG_HIP_CHECK(hipStreamSynchronize(s));
    return srg_ok();
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

void FloatCSRMulDenseOMP(float answer[], float data[], int indices[], int indptr[], float mat[],
                         int mat_row, int mat_col)
{
    (void)host_compat_spmm(answer, data, indices, indptr, mat, mat_row, mat_col, false, -1);
}

int FloatCSRMulDense(float answer[], int data_nnz, float data[], int indices[], int indptr[],
                     float mat[], int mat_row, int mat_col)
{
    return host_compat_spmm(answer, data, indices, indptr, mat, mat_row, mat_col, true, data_nnz) == SRG_OK ? 0 : 1;
}

int srg_spmm_csr_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                     int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                     const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, uint32_t flags,
                     void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_spmm_args(indptr, indices, values, n_rows, X, ldx, Y, ldy, d);
    if (rc) return rc;
    rc = launch_spmm<int64_t>(indptr, indices, values, n_rows, row_order, n_hub, n_heavy, X, ldx, Y, ldy, d, flags,
                              static_cast<hipStream_t>(stream));
    return rc ? rc : srg_ok();
}

int srg_spmm_agg_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                     int64_t n_rows, const int32_t* row_order, int64_t n_hub, int64_t n_heavy,
                     const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, uint32_t flags,
                     float* agg, int64_t lda, float w, int agg_init, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_spmm_args(indptr, indices, values, n_rows, X, ldx, Y, ldy, d);
    if (rc) return rc;
    if (n_rows > 0 && d > 0 && (!agg || lda < d))
        return srg_fail(SRG_ERR_INVALID, "aggregation panel: agg=%p lda=%lld < d=%d", (void*)agg, (long long)lda, d);
    if (agg && agg == Y) return srg_fail(SRG_ERR_INVALID, "agg must not alias Y");
    rc = launch_spmm<int64_t>(indptr, indices, values, n_rows, row_order, n_hub, n_heavy, X, ldx, Y, ldy, d, flags,
                              static_cast<hipStream_t>(stream), agg_epi(agg, lda, w, agg_init));
    return rc ? rc : srg_ok();
}

int srg_spmm_span_f32(const int64_t* row_beg, const int64_t* row_end, const int32_t* indices,
                      const float* values, int64_t n_rows, const int32_t* row_order, int64_t n_hub,
                      int64_t n_heavy, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                      uint32_t flags, float* agg, int64_t lda, float w, int agg_init, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    int rc = check_spmm_args(row_beg, indices, values, n_rows, X, ldx, Y, ldy, d);
    if (rc) return rc;
    if (n_rows > 0 && d > 0 && !row_end) return srg_fail(SRG_ERR_INVALID, "null row_end");
    if (agg && (lda < d || agg == Y))
        return srg_fail(SRG_ERR_INVALID, "aggregation panel: lda=%lld < d=%d or agg aliases Y", (long long)lda, d);
    Epi e = agg_epi(agg, lda, w, agg_init);
    e.row_end = row_end;
    rc = launch_spmm<int64_t, kEpiSpan>(row_beg, indices, values, n_rows, row_order, n_hub, n_heavy, X, ldx, Y, ldy,
                                        d, flags, static_cast<hipStream_t>(stream), e);
    return rc ? rc : srg_ok();
}

int srg_propagate_khop_f32(const int64_t* indptr, const int32_t* indices, const float* values,
                           int64_t n_rows, const int32_t* row_order, int64_t n_hub,
                           int64_t n_heavy, float* const* panels,
                           int64_t ld, int32_t d, int32_t K, uint32_t flags, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (K < 0) return srg_fail(SRG_ERR_INVALID, "K=%d < 0", K);
    if (K > 0 && !panels) return srg_fail(SRG_ERR_INVALID, "null panels");
    for (int k = 0; k <= K; ++k)
        if (!panels[k] && n_rows > 0 && d > 0) return srg_fail(SRG_ERR_INVALID, "panels[%d] is null", k);
    int rc = check_spmm_args(indptr, indices, values, n_rows, panels ? panels[0] : nullptr, ld,
                             panels ? panels[0] : nullptr, ld, d);
    if (rc) return rc;
    const uint32_t f = flags & ~SRG_SPMM_ACCUMULATE;
    if (!row_order && n_hub == 0 && n_heavy == 0 && K > 0 && n_rows > 0 && d > 0 &&
        !(f & ~(SRG_SPMM_NT_STORE | SRG_SPMM_FAST))) {
        // no schedule: the hops run through a plan made for them (srg_plan.hip), freed after them.  Without
        // a schedule there were never hub rows here, so FAST (which only re-associates hub rows) changed
        // nothing: the implicit plan then has no hub rows either, and the bits stay exact
        srg_plan* P = nullptr;
        const int64_t hub_t = (f & SRG_SPMM_FAST) ? SRG_PLAN_NONE : SRG_PLAN_AUTO;
        rc = srg_plan_build(indptr, indices, values, n_rows, d, K, 0, hub_t, SRG_PLAN_AUTO, 0, stream, &P);
        if (rc) return rc;
        rc = srg_plan_propagate_f32(P, panels, ld, d, K, f, stream);
        const int rc2 = srg_plan_destroy(P, stream);
        return rc ? rc : rc2;
    }
    for (int k = 1; k <= K; ++k) {
        rc = launch_spmm<int64_t>(indptr, indices, values, n_rows, row_order, n_hub, n_heavy, panels[k - 1], ld,
                                  panels[k], ld, d, f, static_cast<hipStream_t>(stream));
        if (rc) return rc;
    }
    return srg_ok();
}

// one hop of a launch list: X (ldx) -> Y (ldy); launch i carries the aggregation epilogue (agg = (init ?
// 0 : agg) + w * Y, at the end of each of its rows' chains) when agg && agg_on[i]; with join_hub the
// hub side stream is joined into `s` after the hop
static int run_hop_launches(const srg_hop_launch* launches, int32_t n_launch, bool join_hub, const float* X,
                            int64_t ldx, float* Y, int64_t ldy, int32_t d, const uint8_t* agg_on, float* agg,
                            int64_t lda, float w, int agg_init, hipStream_t s, int dev)
{
    for (int i = 0; i < n_launch; ++i) {
        const srg_hop_launch& L = launches[i];
        Epi e = (agg && agg_on && agg_on[i]) ? agg_epi(agg, lda, w, agg_init) : Epi{};
        int rc;
        if (L.row_end) {
            e.row_end = L.row_end;
            // the light rows' slots count from the first non-hub row of the schedule
            e.slot_beg = L.slot_beg ? L.slot_beg + L.n_hub : nullptr;
            e.slot_end = L.slot_beg ? L.slot_end + L.n_hub : nullptr;
            rc = launch_spmm<int64_t, kEpiSpan>(L.row_beg, L.indices, L.values, L.n_rows, L.row_order, L.n_hub,
                                                L.n_heavy, X, ldx, Y, ldy, d, L.flags, s, e);
        } else {
            rc = launch_spmm<int64_t>(L.row_beg, L.indices, L.values, L.n_rows, L.row_order, L.n_hub, L.n_heavy,
                                      X, ldx, Y, ldy, d, L.flags, s, e);
        }
        if (rc) return rc;
    }
    return join_hub ? join_side_stream(dev, s, true) : SRG_OK;
}

static int check_launches(const srg_hop_launch* launches, int32_t n_launch, const float* X, int64_t ldx,
                          const float* Y, int64_t ldy, int32_t d)
{
    for (int i = 0; i < n_launch; ++i) {
        const srg_hop_launch& L = launches[i];
        int rc = check_spmm_args(L.row_beg, L.indices, L.values, L.n_rows, X, ldx, Y, ldy, d);
        if (rc) return rc;
        if (L.n_rows > 0 && L.n_hub + L.n_heavy > 0 && !L.row_order)
            return srg_fail(SRG_ERR_INVALID, "launch %d: hub / heavy rows need a row_order", i);
        if ((L.slot_beg != nullptr) != (L.slot_end != nullptr) || (L.slot_beg && !L.row_end))
            return srg_fail(SRG_ERR_INVALID, "launch %d: slot_beg / slot_end come together, with row_end", i);
    }
    return SRG_OK;
}

int srg_propagate_plan_f32(const srg_hop_launch* launches, int32_t n_launch, int32_t join_hub,
                           float* const* panels, int64_t ld, int32_t d, int32_t K, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (K < 0 || n_launch < 0) return srg_fail(SRG_ERR_INVALID, "K=%d / n_launch=%d < 0", K, n_launch);
    if (K == 0 || n_launch == 0) return srg_ok();
    if (!launches || !panels) return srg_fail(SRG_ERR_INVALID, "null launches or panels");
    for (int k = 0; k <= K; ++k)
        if (!panels[k] && d > 0) return srg_fail(SRG_ERR_INVALID, "panels[%d] is null", k);
    int rc = check_launches(launches, n_launch, panels[0], ld, panels[0], ld, d);
    if (rc) return rc;
    for (int i = 0; i < n_launch; ++i) {
        // without the per-hop join, hop k's hub rows would still run on the side stream while hop
        // k+1's launches on `stream` read panels[k]: a data race
        const srg_hop_launch& L = launches[i];
        if (!join_hub && K > 1 && L.n_hub > 0 && (L.flags & SRG_SPMM_HUB_NOJOIN))
            return srg_fail(SRG_ERR_INVALID, "launch %d: HUB_NOJOIN hub rows over K=%d hops need join_hub", i, K);
    }
    const hipStream_t s = static_cast<hipStream_t>(stream);
    for (int k = 1; k <= K; ++k) {
        rc = run_hop_launches(launches, n_launch, join_hub != 0, panels[k - 1], ld, panels[k], ld, d, nullptr, nullptr,
                              0, 0.0f, 0, s, guard_.dev);
        if (rc) return rc;
    }
    return srg_ok();
}

// srg_plan.hip's single hop (srg_plan_hop_f32): the launches of one hop between panels of their own
// leading dimensions, the aggregation epilogue on the launches agg_on names (checked here)
__attribute__((visibility("hidden"))) int srg_run_plan_hop(const srg_hop_launch* launches, int32_t n_launch,
                                                           int32_t join_hub, const float* X, int64_t ldx, float* Y,
                                                           int64_t ldy, int32_t d, const uint8_t* agg_on, float* agg,
                                                           int64_t lda, float w, int32_t agg_init, void* stream)
{
    SRG_DEVICE_GUARD(stream);
    if (n_launch <= 0) return srg_ok();
    int rc = check_launches(launches, n_launch, X, ldx, Y, ldy, d);
    if (rc) return rc;
    if (X == Y) return srg_fail(SRG_ERR_INVALID, "Y must not alias X (its rows are gathered)");
    if (agg && (lda < d || agg == Y || agg == X))
        return srg_fail(SRG_ERR_INVALID, "aggregation panel: lda=%lld < d=%d or agg aliases X / Y", (long long)lda, d);
    rc = run_hop_launches(launches, n_launch, join_hub != 0, X, ldx, Y, ldy, d, agg_on, agg, lda, w, agg_init,
                          static_cast<hipStream_t>(stream), guard_.dev);
    return rc ? rc : srg_ok();
}

}  // extern "C"
