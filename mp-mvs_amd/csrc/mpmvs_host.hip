// mpmvs_host.hip -- the single definition of what pm_host.hpp declares across the translation units of the library: the
// device-buffer pool, the page-locked pool and the per-thread error text of the calls without a context; and the entry points of
// include/mpmvs.h that are nothing but those (buffers, device count, peer links).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"

hipError_t enter_device(int device) {
    (void)hipGetLastError();
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

std::string& call_error() {
    static thread_local std::string text;
    return text;
}
int call_fail(int code, const std::string& text) {
    call_error() = text;
    return code;
}

// ---------------------------------------------------------------------------
// Device-buffer pool.  A context is created and destroyed per ProcessProblem call in the reference's flow (three times
// per Problem with the shipped schedule) and always asks for the same two dozen buffer sizes; hipMalloc/hipFree cost
// ~0.1-0.3 ms each and hipFree synchronises the device.  Released buffers are therefore kept per (device, size) and handed
// out again; at most MPMVS_POOL_MB (default 4096, 0 = off) megabytes are held.  Callers synchronise the owning stream
// before they release a buffer, so a pooled buffer is never still in use.
// ---------------------------------------------------------------------------
namespace {
struct BufPool {
    std::mutex mu;
    std::unordered_map<void*, std::pair<int, size_t>> owner;
    std::map<std::pair<int, size_t>, std::vector<void*>> cached;
    size_t cached_bytes = 0;
    size_t cap = 4096ull << 20;
    BufPool() {
        if (const char* e = std::getenv("MPMVS_POOL_MB")) cap = (size_t)std::strtoull(e, nullptr, 10) << 20;
    }
    void trim_locked() {
        for (auto& kv : cached)
            for (void* p : kv.second) {
                owner.erase(p);
                (void)hipFree(p);
            }
        cached.clear();
        cached_bytes = 0;
    }
};
BufPool g_pool;
}  // namespace

hipError_t pool_malloc_bytes(void** p, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        auto it = g_pool.cached.find({dev, bytes});
        if (it != g_pool.cached.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            g_pool.cached_bytes -= bytes;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {  // out of memory with buffers parked in the pool: give them back and retry once
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(g_pool.mu);
        g_pool.trim_locked();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        g_pool.owner[*p] = {dev, bytes};
    }
    return e;
}
hipError_t pool_free(void* p) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        auto it = g_pool.owner.find(p);
        if (it != g_pool.owner.end()) {
            const size_t bytes = it->second.second;
            if (g_pool.cached_bytes + bytes <= g_pool.cap) {
                g_pool.cached[it->second].push_back(p);
                g_pool.cached_bytes += bytes;
                return hipSuccess;
            }
            g_pool.owner.erase(it);
        }
    }
    return hipFree(p);
}

// Pinned host buffers for the host arrays of the wrapper (hostPlaneHypotheses ...): hipHostMalloc takes milliseconds, the
// wrapper allocates the same few sizes for every Problem and pass, so released buffers are kept per size (at most
// MPMVS_PINNED_POOL_MB, default 1024).
namespace {
struct PinnedPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> owner;
    std::map<size_t, std::vector<void*>> cached;
    size_t cached_bytes = 0;
    size_t cap = 1024ull << 20;
    PinnedPool() {
        if (const char* e = std::getenv("MPMVS_PINNED_POOL_MB")) cap = (size_t)std::strtoull(e, nullptr, 10) << 20;
    }
};
PinnedPool g_pinned;
}  // namespace

extern "C" {

int mpmvs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mpmvs_free(void* p) { std::free(p); }

void* mpmvs_device_alloc(int device, size_t bytes) {
    if (bytes == 0 || enter_device(device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (pool_malloc_bytes(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void mpmvs_device_free(int device, void* p) {
    if (!p || enter_device(device) != hipSuccess) return;
    (void)pool_free(p);
}

void* mpmvs_alloc_pinned(size_t bytes) {
    if (bytes == 0) bytes = 4;
    static const bool trace = std::getenv("MPMVS_TRACE_PINNED") != nullptr;  // debugging aid: pool hits and misses on stderr
    {
        std::lock_guard<std::mutex> lk(g_pinned.mu);
        auto it = g_pinned.cached.find(bytes);
        if (it != g_pinned.cached.end() && !it->second.empty()) {
            void* p = it->second.back();
            it->second.pop_back();
            g_pinned.cached_bytes -= bytes;
            if (trace) std::fprintf(stderr, "[mpmvs] pinned %zu B: from the pool\n", bytes);
            return p;
        }
    }
    void* p = nullptr;
    (void)hipGetLastError();
    if (trace) std::fprintf(stderr, "[mpmvs] pinned %zu B: hipHostMalloc\n", bytes);
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_pinned.mu);
    g_pinned.owner[p] = bytes;
    return p;
}

void mpmvs_free_pinned(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pinned.mu);
        auto it = g_pinned.owner.find(p);
        if (it == g_pinned.owner.end()) return;  // not ours
        if (g_pinned.cached_bytes + it->second <= g_pinned.cap) {
            g_pinned.cached[it->second].push_back(p);
            g_pinned.cached_bytes += it->second;
            return;
        }
        g_pinned.owner.erase(it);
    }
    (void)hipHostFree(p);
}

// How `device` reaches `peer` (the path hipMemcpyPeerAsync of mpmvs_set_src_depths_mixed / mpmvs_fuse_*_ctx takes, and RCCL between
// the ranks of a node): *can_access = hipDeviceCanAccessPeer, *link_type / *hops = hipExtGetLinkTypeAndHopCount (link type 4 = xGMI,
// 2 = PCIe; -1 where the runtime does not say).  The reference has one device and no such question (src/PatchMatch.cpp:509).
int mpmvs_peer_info(int device, int peer, int* can_access, int* link_type, int* hops) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || peer < 0 || device >= n || peer >= n) return -1;
    int can = device == peer ? 1 : 0;
    if (device != peer && hipDeviceCanAccessPeer(&can, device, peer) != hipSuccess) {
        (void)hipGetLastError();
        can = -1;
    }
    uint32_t lt = 0, hc = 0;
    int ilt = -1, ihc = -1;
    if (device != peer && hipExtGetLinkTypeAndHopCount(device, peer, &lt, &hc) == hipSuccess) {
        ilt = (int)lt;
        ihc = (int)hc;
    } else {
        (void)hipGetLastError();
        if (device == peer) ihc = 0;
    }
    if (can_access) *can_access = can;
    if (link_type) *link_type = ilt;
    if (hops) *hops = ihc;
    return 0;
}

}  // extern "C"
