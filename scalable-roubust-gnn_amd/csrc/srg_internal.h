// srg_internal.h -- host plumbing shared by every translation unit of the library: the thread-local
// status behind srg_last_error, the HIP status check, the walk of a grid in launch-sized chunks, the device
// guard of the entry points and the fork of hub work onto a side stream.  Defined once, in srg_runtime.hip
// (the chunk walk here).  Not part of the C-ABI (include/srgnn_hip.h).
#ifndef SRG_INTERNAL_H_
#define SRG_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>

#include "srgnn_hip.h"

#pragma GCC visibility push(hidden)

// Records `code` and the formatted message as the calling thread's srg_last_error; returns `code`.
int srg_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Clears the calling thread's status; returns SRG_OK.
int srg_ok();

#define SRG_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return srg_fail(SRG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
    } while (0)

// SRG_HIP_CHECK(hipGetLastError()) as a function: what a callable of launch_chunks returns after its launch.
inline int launch_status()
{
    SRG_HIP_CHECK(hipGetLastError());
    return SRG_OK;
}

// A dispatch holds < 2^32 work-items per dimension: launches of more rows than that (111 M rows of the
// papers100M-shaped graph = 7.1e9 lanes) go out in chunks, the kernel adding the chunk's block_base to
// blockIdx.x or being handed pointers shifted by the chunk.  Both caps are the same 2^31-lane bound:
// 2^23 blocks of 256 lanes, 2^24 blocks of one 64-lane wave.
constexpr int64_t kMaxLaunchBlocks = int64_t(1) << 23;
constexpr int64_t kMaxLaunchWaveBlocks = int64_t(1) << 24;

// Walks [0, blocks) in ascending chunks of at most per_launch blocks: launch(b0, nb) launches blocks
// [b0, b0 + nb) and returns its status (launch_status()); the first non-zero status ends the walk and is
// returned.  Calls no HIP API itself.
template <typename Launch>
int launch_chunks(int64_t blocks, int64_t per_launch, Launch launch)
{
    for (int64_t b0 = 0; b0 < blocks; b0 += per_launch)
        if (int rc = launch(b0, (unsigned)std::min<int64_t>(per_launch, blocks - b0))) return rc;
    return SRG_OK;
}

// The test seam behind srg_debug_launch_cap / srg_debug_chunk_launches (include/srgnn_hip.h): a process-wide
// bound on the blocks of one launch (0: none) and a count of the launches the capped walk has issued.
// Header-inline, so every translation unit, and the stand-alone host program of the tests, shares one of each.
inline std::atomic<int64_t> g_launch_cap_override{0};
inline std::atomic<int64_t> g_chunk_launches{0};

// The blocks of one launch at a site whose own cap is dflt: min(dflt, override) under an override (never
// below one block), dflt without one.  One relaxed load.
inline int64_t launch_cap(int64_t dflt)
{
    const int64_t o = g_launch_cap_override.load(std::memory_order_relaxed);
    return o > 0 ? std::max<int64_t>(1, std::min(dflt, o)) : dflt;
}

// launch_chunks under launch_cap(dflt), counting one chunk launch per call of `launch`.
template <typename Launch>
int launch_chunks_capped(int64_t blocks, int64_t dflt, Launch launch)
{
    return launch_chunks(blocks, launch_cap(dflt), [&](int64_t b0, unsigned nb) {
        g_chunk_launches.fetch_add(1, std::memory_order_relaxed);
        return launch(b0, nb);
    });
}

// Makes the device of `s` current for the lifetime of the guard (the null stream means the
// current device), so every launch, event and side stream of an entry point belongs to the
// device the caller's stream lives on.
struct DeviceGuard {
    int prev = -1, dev = -1, rc = SRG_OK;
    explicit DeviceGuard(hipStream_t s);
    ~DeviceGuard();
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define SRG_DEVICE_GUARD(stream)                                   \
    DeviceGuard guard_(static_cast<hipStream_t>(stream));          \
    if (guard_.rc) return guard_.rc

// The dynamic-LDS limits of one kernel family's hub kernels.  Kernel attributes are per device and the
// kernels belong to the family's translation unit, so the family states how to raise them (`raise`, on
// the current device) and HubFork::fork does so once per device, before the family's first hub launch
// there, under the side-stream registry's lock (which also guards `done`).
constexpr int kMaxDevices = 64;
struct HubLds {
    int (*raise)();
    bool done[kMaxDevices];
};

struct SideStream;   // srg_runtime.hip: a (device, caller stream) entry of the registry

// One launch's fork of hub work onto the side stream of (current device, caller stream), step by step:
// fork, the hub launches on stream(), record_join, delay, the main launches, join.  Holds the registry's
// lock from the first fork until it goes out of scope (the end of the launch: see SideStream), and makes
// no HIP call when it does, so an error return only releases the lock.  A launch without hub rows never
// forks and never takes the lock.
class HubFork {
public:
    HubFork(hipStream_t caller, HubLds& lds);
    // Orders the side stream after the caller's stream.  may_continue: when the entry has an unjoined
    // fork, no new one is made (continued()): the hub work is appended to the side stream as it is.
    // Forking again on one object forks again under the lock it already holds.
    int fork(bool may_continue = false);
    bool continued() const { return continued_; }
    hipStream_t stream() const;
    // After the hub launches; pending: the join is left to srg_hub_join.
    int record_join(bool pending);
    // The single-wave delay on the caller's stream (k_dispatch_delay)
    int delay();
    // The caller's stream waits for the recorded join (nothing to wait for without a fork).
    int join();

private:
    hipStream_t s_;
    HubLds& lds_;
    std::unique_lock<std::mutex> lock_;
    SideStream* ss_ = nullptr;
    bool continued_ = false;
};

// Joins the side stream of (dev, s) into `s`: waits on the entry's join event -- only_pending: only after
// an unjoined fork; otherwise whenever the entry has one -- and marks it joined.
int join_side_stream(int dev, hipStream_t s, bool only_pending);

#pragma GCC visibility pop

#endif  // SRG_INTERNAL_H_
