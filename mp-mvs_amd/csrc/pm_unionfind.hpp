// pm_unionfind.hpp -- the lock-free union-find that the connected components of a point cloud (pm_components.hpp) and of a triangle
// mesh (pm_mesh.hpp) share: the parent array, find with path halving, the compare-and-swap hook, and the three passes that follow
// the hook pass of either user (flatten, sizes, gather).  What each function does and why stale reads do no harm is written out in
// pm_components.hpp and DESIGN.md section 20; nothing here knows where the edges come from.
//   parent[]   an int per element: its own index at the start, -1 for an element that does not take part (never read again).
//              Invariant: parent[x] <= x.  A root has parent[x] == x.
// Several translation units include this header, so its kernels are `inline` (see pm_scan.hpp).
// The per-thread bodies are host and device code, so that tools/components_check.cpp and tools/mesh_clean_check.cpp can replay them
// thread by thread and edge by edge under the sanitizers; there the atomics are plain reads and writes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pm {

__host__ __device__ inline int cc_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
__host__ __device__ inline void cc_store(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
__host__ __device__ inline int cc_cas(int* p, int expect, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const int old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
__host__ __device__ inline void cc_add(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// the root of x's tree; halves the path it walks.  x takes part (parent[x] >= 0).
__host__ __device__ inline int cc_find(int* __restrict__ parent, int x) {
    int curr = cc_load(&parent[x]);
    if (curr != x) {
        int prev = x, next;
        while (curr > (next = cc_load(&parent[curr]))) {   // parent[curr] < curr: curr is no root
            cc_store(&parent[prev], next);                 // prev is no root either; next lies further down its tree
            prev = curr;
            curr = next;
        }
    }
    return curr;
}

// unites the trees of ra and rb, two roots that may have been hooked since they were found; returns the root of the united tree
// as of the hook
__host__ __device__ inline int cc_link(int* __restrict__ parent, int ra, int rb) {
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = cc_cas(&parent[hi], hi, lo);
        if (old == hi) return lo;          // hi was a root and hangs under lo now
        ra = cc_find(parent, old);         // hi had been hooked: old < hi is on its tree; max(ra, rb) falls with every retry
        rb = lo;
    }
    return ra;
}

__host__ __device__ inline int cc_union(int* __restrict__ parent, int a, int b) {
    return cc_link(parent, cc_find(parent, a), cc_find(parent, b));
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
// ---- flatten ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void cc_flatten_one(size_t i, int* __restrict__ parent, int32_t* __restrict__ label) {
    label[i] = cc_load(&parent[i]) < 0 ? -1 : cc_find(parent, (int)i);
}
inline __global__ __launch_bounds__(256) void k_cc_flatten(int n, int* __restrict__ parent, int32_t* __restrict__ label) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cc_flatten_one(i, parent, label);
}

// ---- sizes: cnt[] is zero at the start ---------------------------------------------------------------------------------------------
// one element with the label l (< 0: none) adds 1 to cnt[l]
__host__ __device__ inline void cc_count_label(int l, int* __restrict__ cnt) {
    if (l >= 0) cc_add(&cnt[l], 1);
}
__host__ __device__ inline void cc_count_one(size_t i, const int32_t* __restrict__ label, int* __restrict__ cnt) { cc_count_label(label[i], cnt); }
// the same sums with one add per distinct label of a wave: the lanes that share the label of the first lane still waiting are
// counted by a ballot, that lane adds their number, and they leave; a wave makes at most as many rounds as it holds labels.  Every
// lane of the wave must call it (l < 0: a lane with nothing to add).
__device__ __forceinline__ void cc_count_wave(int l, int* __restrict__ cnt) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = (int)(threadIdx.x & 63);
    bool waiting = l >= 0;
    unsigned long long todo = __ballot(waiting);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int ll = __shfl(l, lead, 64);
        const unsigned long long same = __ballot(waiting && l == ll);
        if (lane == lead) atomicAdd(&cnt[ll], (int)__popcll(same));
        waiting = waiting && l != ll;
        todo &= ~same;
    }
#endif
}
inline __global__ __launch_bounds__(256) void k_cc_count(int n, const int32_t* __restrict__ label, int* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    cc_count_wave(i < (size_t)n ? label[i] : -1, cnt);
}

__host__ __device__ inline void cc_gather_one(size_t i, const int32_t* __restrict__ label, const int* __restrict__ cnt, int32_t* __restrict__ size) {
    const int l = label[i];
    size[i] = l >= 0 ? cnt[l] : 0;
}
inline __global__ __launch_bounds__(256) void k_cc_gather(int n, const int32_t* __restrict__ label, const int* __restrict__ cnt, int32_t* __restrict__ size) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cc_gather_one(i, label, cnt, size);
}
#pragma clang diagnostic pop

}  // namespace pm
