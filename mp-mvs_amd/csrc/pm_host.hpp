// pm_host.hpp -- what the host side of every family of the C ABI shares (definitions: mpmvs_host.hip): entering a device, the
// pooled device and page-locked buffers, the scoped scratch and stateless-call helpers, the checked kernel launch, the pass clock, the
// guard of a call's malloc'd results, the camera conversion, the error channel of the calls without a PatchMatch context, and the one
// question the fusion asks a context.  (The host side of the scan is pm_scan_host.hpp: it names kernels, which a unit that never
// scans should not get into its code object.)  Declarations and small inline classes only; everything here is hidden: the library's
// dynamic symbol table is include/mpmvs.h and the kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_device.hpp"

#pragma GCC visibility push(hidden)

// hipGetLastError() reports the last error of ANY earlier runtime call of this thread (e.g. another caller's failed
// hipSetDevice).  Every entry point drops such a stale error first, so that the checks after its own kernel launches only
// see its own failures.
hipError_t enter_device(int device);

// Device-buffer pool (mpmvs_host.hip): released buffers are kept per (device, size) and handed out again.  Callers synchronise the
// owning stream before they release a buffer, so a pooled buffer is never still in use.
hipError_t pool_malloc_bytes(void** p, size_t bytes);
hipError_t pool_free(void* p);
template <typename T>
inline hipError_t pool_malloc(T** p, size_t bytes) {
    return pool_malloc_bytes((void**)p, bytes);
}

// The error text of the calls without a context, per host thread: what mpmvs_last_error(NULL) returns.  A failed mpmvs_create
// leaves its reason here, and so does every handle-free or handle-based call of the other families (call_fail).
std::string& call_error();
int call_fail(int code, const std::string& text);
#define CALLCHK(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) return call_fail(-100, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The finished Run() a context holds, as the fusion reads it: -2 unless the context is w x h, has planes whose .w mirrors the depth
// map and no pipelined Run() in flight; else 0 with the context's device, its stream (not synchronised here) and the planes
// (mpmvs_api.hip, the only file that sees struct mpmvs_ctx).
int ctx_resident_planes(const mpmvs_ctx* c, int w, int h, int* device, hipStream_t* stream, const float4** planes);

// page-locked scratch of one call: back to its pool on every return path
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() {
        if (p) mpmvs_free_pinned(p);
    }
};

// Pooled scratch buffer of one call on a stream that outlives it (a context's, the sky network's): on every return path the
// stream is synchronised first, then the buffer goes back to the pool -- nothing returns to the pool while the stream may use it.
struct Scratch {
    hipStream_t st;
    void* p = nullptr;
    explicit Scratch(hipStream_t stream) : st(stream) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        (void)pool_free(p);
    }
    hipError_t alloc(size_t bytes) { return pool_malloc_bytes(&p, bytes ? bytes : 4); }
    template <typename T>
    T* as() const { return (T*)p; }
};

// One stateless call on a device (fusion, sky mask, view selection, undistortion, the probes): a non-blocking stream of its own --
// the PatchMatch contexts other host threads drive on this device keep running -- and the pooled buffers of the call.  The
// destructor synchronises the stream, THEN gives the buffers back and destroys the events and the stream, on every return path.
class DeviceCall {
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<void*> bufs;
    bool entered_ = false, own_stream = false;

   public:
    explicit DeviceCall(int device) : entered_(enter_device(device) == hipSuccess) {
        own_stream = entered_ && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    }
    // a probe without a device argument: the current device and its null stream
    DeviceCall() : entered_(true) { (void)hipGetLastError(); }  // drop a stale error of an earlier call (see enter_device)
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;
    ~DeviceCall() {
        if (!entered_) return;
        (void)hipStreamSynchronize(st);
        for (void* p : bufs) (void)pool_free(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(st);
    }
    bool entered() const { return entered_; }         // the device could be selected
    bool ok() const { return own_stream; }            // ... and the stream exists
    hipStream_t stream() const { return st; }
    // nullptr: no memory.  Zero-sized arrays still get a (4-byte) buffer, so that no kernel argument is null.
    template <typename T>
    T* alloc(size_t bytes) {
        void* p = nullptr;
        if (pool_malloc_bytes(&p, bytes ? bytes : 4) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return (T*)p;
    }
    // the same for `count` elements of T
    template <typename T>
    T* alloc_n(size_t count) {
        return alloc<T>(count * sizeof(T));
    }
    // begin() ... end() around the kernels; once the stream is synchronised, elapsed() is their device time
    bool begin() { return hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess && hipEventRecord(ev[0], st) == hipSuccess; }
    bool end() { return hipEventRecord(ev[1], st) == hipSuccess; }
    bool elapsed(float* ms) const { return hipEventElapsedTime(ms, ev[0], ev[1]) == hipSuccess; }
};

// One kernel launch without dynamic LDS, and what it left: CALLCHK(launch(k_name, grid, block, stream, args...)).  Every argument is
// cast to the kernel's parameter type, so a plain nullptr serves where a kernel takes an optional typed pointer.
template <typename... K, typename... A>
inline hipError_t launch(void (*kernel)(K...), dim3 grid, dim3 block, hipStream_t stream, A&&... args) {
    static_assert(sizeof...(K) == sizeof...(A), "one argument per kernel parameter");
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<K>(args)...);
    return hipGetLastError();
}

// The pass borders of a call or a handle: N events, all created by the first mark (so that none is created between two launches of a
// timed sequence, where the wait for the host would count as device time) and destroyed with the clock.  Whoever owns a clock lets it
// die only after the stream it recorded on has been waited for (a handle's release function; a call declares its clock before the
// objects that synchronise the stream when they go).
template <int N>
struct PassClock {
    hipEvent_t e[N] = {};
    PassClock() = default;
    PassClock(const PassClock&) = delete;
    PassClock& operator=(const PassClock&) = delete;
    ~PassClock() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t mark(int k, hipStream_t stream) {
        for (hipEvent_t& x : e) {
            const hipError_t rc = x ? hipSuccess : hipEventCreate(&x);
            if (rc != hipSuccess) return rc;
        }
        return hipEventRecord(e[k], stream);
    }
    // the device time between two marks, once the stream is idle
    hipError_t ms(int a, int b, float* t) const { return hipEventElapsedTime(t, e[a], e[b]); }
};

// The malloc'd host buffers of a call's result: released unless the call succeeds and keep()s them for its caller.
class HostOut {
    std::vector<void*> bufs;
    bool kept = false;

   public:
    HostOut() = default;
    HostOut(const HostOut&) = delete;
    HostOut& operator=(const HostOut&) = delete;
    ~HostOut() {
        if (!kept)
            for (void* p : bufs) std::free(p);
    }
    // nullptr: no memory
    template <typename T>
    T* take(size_t count) {
        void* p = std::malloc(count * sizeof(T));
        if (p) bufs.push_back(p);
        return (T*)p;
    }
    void keep() { kept = true; }
};

inline void cam_to_dev(const mpmvs_camera& s, pm::CamDev& d) {
    std::memcpy(d.K, s.K, sizeof(d.K));
    std::memcpy(d.R, s.R, sizeof(d.R));
    std::memcpy(d.t, s.t, sizeof(d.t));
    std::memcpy(d.C, s.C, sizeof(d.C));
}

#pragma GCC visibility pop
