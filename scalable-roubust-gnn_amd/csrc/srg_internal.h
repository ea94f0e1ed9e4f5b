// srg_internal.h -- host plumbing shared by every translation unit of the library: the thread-local
// status behind srg_last_error, the HIP status check and the device guard of the entry points.  Defined
// once, in srg_spmm.hip.  Not part of the C-ABI (include/srgnn_hip.h).
#ifndef SRG_INTERNAL_H_
#define SRG_INTERNAL_H_

#include <hip/hip_runtime.h>

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

#pragma GCC visibility pop

#endif  // SRG_INTERNAL_H_
