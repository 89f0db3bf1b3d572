// side_call.hpp -- the frame of an entry point of a side library (chain_diag.hip, posterior.hip, evidence.hip,
// predictive.hip, loo.hip, relabel.hip, fisher.hip): the error slot, buffers and the caller's device released on every
// exit path, device selection, the dynamic-LDS limit, staging of host chains, result copies.  DESIGN.md "The call frame
// of the side libraries".
//
// Host code only.  Each library is one translation unit built with -fvisibility=hidden, so each holds its own copy
// of the state below (the error slot, the record of raised limits).  The argument checks, their messages and
// *_version / *_last_error stay in the .hip files.
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

namespace vamp {
namespace side {

inline thread_local std::string g_err;     // what *_last_error returns

inline int fail(const std::string& msg) {
    g_err = msg;
    return -1;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            (void)hipGetLastError();                                                                    \
            return ::vamp::side::fail(std::string(#expr) + ": " + hipGetErrorString(e_));               \
        }                                                                                               \
    } while (0)

struct DevBuf {                    // released on every exit path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct DeviceRestore {             // the caller's current device, put back on every exit path
    int dev = -1;
    ~DeviceRestore() { if (dev >= 0) (void)hipSetDevice(dev); }
};

template <class T>
int upload(DevBuf& buf, const std::vector<T>& v, hipStream_t st) {
    if (v.empty()) return 0;
    HIP_TRY(hipMalloc(&buf.p, v.size() * sizeof(T)));
    HIP_TRY(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}

// makes `device` current and remembers the caller's in `restore`; `fn` ("name: ") opens the message
inline int set_device(const std::string& fn, int device, DeviceRestore& restore) {
    int ndev = 0, prev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(fn + "no HIP device " + std::to_string(device));
    HIP_TRY(hipGetDevice(&prev));
    restore.dev = prev;
    HIP_TRY(hipSetDevice(device));
    return 0;
}

struct LdsAsk {                    // a kernel and the most dynamic LDS a launch of it may ask for
    const void* kernel;
    size_t bytes;
};

// Kernels that may ask for more dynamic LDS than a launch gets by default: the limit is raised once per process and
// device, and a refusal is reported as what it is.  A library calls this from one place, with all such kernels: the
// record of what is done is per library, not per kernel.
inline int raise_lds_limit(const std::string& fn, int device, std::initializer_list<LdsAsk> asks) {
    constexpr int kMaxDevices = 64;
    static std::mutex mu;
    static bool done[kMaxDevices] = {};
    std::lock_guard<std::mutex> lock(mu);
    if (device < kMaxDevices && done[device]) return 0;
    size_t most = 0;
    hipError_t e = hipSuccess;
    for (const LdsAsk& a : asks) {
        most = a.bytes > most ? a.bytes : most;
        if (e == hipSuccess) e = hipFuncSetAttribute(a.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.bytes);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(fn + "this device does not grant a workgroup " + std::to_string(most / 1024) +
                    " KiB of dynamic LDS (hipFuncSetAttribute(MaxDynamicSharedMemorySize): " + hipGetErrorString(e) +
                    "); the kernels are built for gfx950's 160 KiB");
    }
    if (device < kMaxDevices) done[device] = true;
    return 0;
}

// doubles from the first kept sample of a chain to the end of its last: n_keep rows of walkers * ndim, ld apart
inline long long chain_span(int n_keep, long long ld, int walkers, int ndim) {
    return (long long)(n_keep - 1) * ld + (long long)walkers * ndim;
}

// Host chains to the device: len[g] doubles from base[g], one group after the other in one buffer; dbase[g] is the
// group's device view.  A length of zero means "not staged": nothing is copied and the view is NULL.
inline int stage_chains(const std::vector<long long>& len, const double* const* base, hipStream_t st, DevBuf& staging,
                        std::vector<const double*>& dbase) {
    long long total = 0;
    for (long long n : len) total += n;
    dbase.assign(len.size(), nullptr);
    if (total == 0) return 0;
    HIP_TRY(hipMalloc(&staging.p, total * sizeof(double)));
    long long off = 0;
    for (size_t g = 0; g < len.size(); ++g) {
        if (len[g] == 0) continue;
        HIP_TRY(hipMemcpyAsync(staging.as<double>() + off, base[g], len[g] * sizeof(double), hipMemcpyHostToDevice, st));
        dbase[g] = staging.as<double>() + off;
        off += len[g];
    }
    return 0;
}

// a result back to the caller; an output the caller did not ask for (NULL) or an empty one is skipped
inline int fetch(void* dst, const void* src, long long bytes, hipStream_t st) {
    if (!dst || bytes == 0) return 0;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

// the end of a call: the device's {n_used, n_bad} pair of every group back, the stream drained (the fetches queued
// before are then done too), the pairs fanned into the caller's arrays (either may be NULL)
inline int fetch_counts(const DevBuf& d_counts, int n_groups, int32_t* n_used, int32_t* n_bad, hipStream_t st) {
    std::vector<int32_t> counts((size_t)n_groups * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < n_groups; ++g) {
        if (n_used) n_used[g] = counts[2 * g];
        if (n_bad) n_bad[g] = counts[2 * g + 1];
    }
    return 0;
}

}  // namespace side
}  // namespace vamp
