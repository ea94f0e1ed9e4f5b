// srg_runtime.hip -- what every entry point of the library shares (srg_internal.h): the calling
// thread's error state, the device guard, and the hub side streams with HubFork.  Its one kernel is the
// dispatch delay after a fork; the kernels that run on the side streams belong to their families.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <utility>

#include "srgnn_hip.h"
#include "srg_internal.h"

#ifndef SRG_GIT_REV
#define SRG_GIT_REV "dev"
#endif

// ------------------------------------------------------------------------------------------------
// error handling and the device guard (srg_internal.h): the library's one definition of each
// ------------------------------------------------------------------------------------------------
namespace {
thread_local char g_err_msg[512] = "";
thread_local int g_err_code = SRG_OK;
}  // namespace

int srg_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err_msg, sizeof(g_err_msg), fmt, ap);
    va_end(ap);
    g_err_code = code;
    return code;
}

int srg_ok()
{
    g_err_code = SRG_OK;
    g_err_msg[0] = '\0';
    return SRG_OK;
}

DeviceGuard::DeviceGuard(hipStream_t s)
{
    // no usable device: leave it to the entry point (argument checks and empty problems
    // need none; its first HIP call reports the error)
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) { (void)hipGetLastError(); prev = -1; return; }
    dev = prev;
    if (s) {
        hipDevice_t d = 0;
        e = hipStreamGetDevice(s, &d);
        if (e != hipSuccess) { rc = srg_fail(SRG_ERR_HIP, "hipStreamGetDevice failed: %s", hipGetErrorString(e)); return; }
        dev = (int)d;
    }
    if (dev != prev) {
        e = hipSetDevice(dev);
        if (e != hipSuccess) { rc = srg_fail(SRG_ERR_HIP, "hipSetDevice(%d) failed: %s", dev, hipGetErrorString(e)); dev = prev; }
    }
}

DeviceGuard::~DeviceGuard()
{
    if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
}

// ------------------------------------------------------------------------------------------------
// hub side streams
// ------------------------------------------------------------------------------------------------
// One per (device, caller stream), created on first use, each with its own
// fork / join events: callers on different streams never share events.  The whole fork sequence
// of a launch (record fork, side-stream wait, hub launch, record join, main launch, join wait)
// runs under g_side_mu, so host threads sharing one caller stream cannot interleave their records
// either.  SRG_SPMM_HUB_NOJOIN leaves the join to srg_hub_join(stream), which waits on the same
// (device, stream) entry's join event.  At most kMaxSideStreams entries live per device: a caller
// that makes a new stream per call evicts the least recently used entry without an outstanding
// NOJOIN fork (its stream is destroyed asynchronously: queued hub work still completes).
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    uint64_t last_use = 0;
    bool pending = false;      // a NOJOIN fork not yet joined by srg_hub_join
};

namespace {

// One wave that sleeps ~`us` microseconds (s_memrealtime ticks at 100 MHz).  Enqueued on the main
// stream right after the hub workgroups are forked onto the side stream, so they are dispatched
// onto free CUs before the main launch's blocks fill every CU (a hub workgroup needs 9 waves and
// ~136 KB of LDS on one CU; behind a full-chip launch it could start milliseconds late and become
// the hop's tail).
__global__ void k_dispatch_delay(int us)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long ticks = 100ull * (unsigned long long)us;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}

// the single-wave delay after a hub fork (10 us: 0 and 5 stay bimodal, 20 is 1-3 % slower,
// profiles/r01_dispatch_delay_sweep.txt)
constexpr int kHubDelayUs = 10;

constexpr int kMaxSideStreams = 8;
std::mutex g_side_mu;
std::map<std::pair<int, hipStream_t>, SideStream> g_side;   // guarded by g_side_mu
uint64_t g_side_tick = 0;                                     // guarded by g_side_mu

// The side stream of (dev, caller), dev the current device; the caller holds g_side_mu.
int side_stream_locked(int dev, hipStream_t caller, SideStream** out)
{
    const auto key = std::make_pair(dev, caller);
    if (g_side.find(key) == g_side.end()) {
        int live = 0;
        auto lru = g_side.end();
        for (auto it = g_side.begin(); it != g_side.end(); ++it) {
            if (it->first.first != dev) continue;
            ++live;
            if (!it->second.pending && (lru == g_side.end() || it->second.last_use < lru->second.last_use)) lru = it;
        }
        if (live >= kMaxSideStreams && lru != g_side.end()) {
            (void)hipEventDestroy(lru->second.fork);
            (void)hipEventDestroy(lru->second.join);
            (void)hipStreamDestroy(lru->second.stream);
            g_side.erase(lru);
        }
    }
    // (insert, not operator[]: that one left std::piecewise_construct among the library's dynamic symbols)
    SideStream& ss = g_side.insert({key, SideStream{}}).first->second;
    ss.last_use = ++g_side_tick;
    if (!ss.stream) {
        // highest queue priority: the hub workgroups (9 waves, ~136 KB LDS each) must get CUs
        // before the main launch's many small blocks occupy them all (normal priority measured the
        // same or slower: DESIGN.md §7, round 4)
        int least = 0, greatest = 0;
        SRG_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        SRG_HIP_CHECK(hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, greatest));
        SRG_HIP_CHECK(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
        SRG_HIP_CHECK(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
    }
    *out = &ss;
    return SRG_OK;
}

}  // namespace

HubFork::HubFork(hipStream_t caller, HubLds& lds) : s_(caller), lds_(lds), lock_(g_side_mu, std::defer_lock) {}

int HubFork::fork(bool may_continue)
{
    if (!lock_.owns_lock()) lock_.lock();
    if (!ss_) {
        int dev = 0;
        SRG_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return srg_fail(SRG_ERR_HIP, "device id %d", dev);
        if (!lds_.done[dev]) {   // before the family's first hub launch on this device
            if (int rc = lds_.raise()) return rc;
            lds_.done[dev] = true;
        }
        if (int rc = side_stream_locked(dev, s_, &ss_)) return rc;
    }
    continued_ = may_continue && ss_->pending;
    if (continued_) return SRG_OK;
    SRG_HIP_CHECK(hipEventRecord(ss_->fork, s_));
    SRG_HIP_CHECK(hipStreamWaitEvent(ss_->stream, ss_->fork, 0));
    return SRG_OK;
}

hipStream_t HubFork::stream() const { return ss_->stream; }

int HubFork::record_join(bool pending)
{
    SRG_HIP_CHECK(hipEventRecord(ss_->join, ss_->stream));
    ss_->pending = pending;
    return SRG_OK;
}

int HubFork::delay()
{
    hipLaunchKernelGGL(k_dispatch_delay, dim3(1), dim3(64), 0, s_, kHubDelayUs);
    SRG_HIP_CHECK(hipGetLastError());
    return SRG_OK;
}

int HubFork::join()
{
    if (ss_) SRG_HIP_CHECK(hipStreamWaitEvent(s_, ss_->join, 0));
    return SRG_OK;
}

int join_side_stream(int dev, hipStream_t s, bool only_pending)
{
    std::lock_guard<std::mutex> lock(g_side_mu);
    auto it = g_side.find(std::make_pair(dev, s));
    if (it == g_side.end() || !(only_pending ? it->second.pending : it->second.join != nullptr)) return SRG_OK;
    SRG_HIP_CHECK(hipStreamWaitEvent(s, it->second.join, 0));
    it->second.pending = false;
    return SRG_OK;
}

extern "C" {

int srg_hub_side_streams(void)
{
    std::lock_guard<std::mutex> lock(g_side_mu);
    return (int)g_side.size();
}

int srg_hub_join(void* stream)
{
    SRG_DEVICE_GUARD(stream);
    const int rc = join_side_stream(guard_.dev, static_cast<hipStream_t>(stream), false);
    return rc ? rc : srg_ok();
}

const char* srg_last_error(void) { return g_err_msg; }
int srg_last_error_code(void) { return g_err_code; }
void srg_clear_error(void) { (void)srg_ok(); }
const char* srg_version(void) { return "srgnn_hip " SRG_GIT_REV " gfx950"; }

int64_t srg_debug_launch_cap(int64_t blocks)
{
    return g_launch_cap_override.exchange(blocks > 0 ? blocks : 0, std::memory_order_relaxed);
}

int64_t srg_debug_chunk_launches(void) { return g_chunk_launches.load(std::memory_order_relaxed); }

}  // extern "C"
