// pm_knn.hpp -- exact capped k nearest neighbours on the grids of pm_cloud.hpp (mpmvs_cloud_knn, mpmvs_cloud_outliers; contract:
// DESIGN.md section 17 and include/mpmvs.h).  Per query the min(k, candidates) lexicographically smallest pairs (d2 bits, index)
// over the candidates of mpmvs_cloud_nearest -- finite targets with d2 = (dx*dx + dy*dy) + dz*dz <= r2 in fp32, no contraction --
// in ascending order, and the number of all candidates.  A query that is target `self` of the same cloud skips that one index
// (the exclusion is by index, not by distance: an exact duplicate stays a neighbour at d2 = +0).  Bit for bit the brute-force
// statement; independent of scheduling, because the order in which a cell's run is walked never shows in a sorted list of
// distinct keys.
//
// One thread per query, binned by k_cloud_qbin / k_cloud_qorder (pm_cloud.hpp), its candidates handed over by cloud_walk (there:
// why 27 cells hold them all).  The list is K sorted 64-bit keys, cloud_cand's (d2 bits << 32) | index; ~0 marks a free entry and is above every key
// (d2 <= r2 is finite).  A candidate below the worst key replaces it and sinks through one fully unrolled chain of K - 1
// compare-exchanges: every index is a constant, so the list stays in registers.  K is a template parameter of 4, 8, 16 or 32, the
// caller's k rounded up; only the first k entries are reported.
// Two store variants:
//   k_knn_list    writes the rows (d2, index) of k entries, +inf / -1 beyond the candidates, and the candidate count;
//   k_knn_reduce  writes only the mean of the k square roots (fp64 sum in ascending list order, IEEE sqrt and quotient, rounded to
//                 fp32 once; +inf below k candidates) and the candidate count: what mpmvs_cloud_outliers needs, so that no list
//                 reaches HBM.
// The per-thread bodies are host and device code, so that tools/knn_check.cpp can replay them thread by thread under the
// sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"

namespace pm {

constexpr int kKnnMaxK = 32;
constexpr unsigned kKnnNoSelf = ~0u;   // no target has this index: a cloud holds at most 2^31 - 1 points

// the list size that serves k: 4, 8, 16 or 32
__host__ __device__ inline int knn_list_size(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32)); }

template <int K>
struct KnnList {
    unsigned long long key[K];   // ascending; ~0 = free
};

template <int K>
__host__ __device__ __attribute__((always_inline)) inline void knn_clear(KnnList<K>& l) {
#pragma unroll
    for (int j = 0; j < K; ++j) l.key[j] = ~0ull;
}

// keeps the K smallest keys seen: the keys of one query are distinct (the index is part of the key)
template <int K>
__host__ __device__ __attribute__((always_inline)) inline void knn_push(KnnList<K>& l, unsigned long long cand) {
    if (cand < l.key[K - 1]) {
        l.key[K - 1] = cand;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const unsigned long long lo = l.key[j - 1], hi = l.key[j];
            const bool swap = hi < lo;
            l.key[j - 1] = swap ? hi : lo;
            l.key[j] = swap ? lo : hi;
        }
    }
}

// cloud_walk (pm_cloud.hpp) with a list as its visitor; returns the number of candidates
template <int K>
__host__ __device__ __attribute__((always_inline)) inline int knn_search(float x, float y, float z, int cx, int cy, int cz, const CloudGrid& g, unsigned self,
                                                                         KnnList<K>& l) {
    int within = 0;
    cloud_walk<1>(cx, cy, cz, g, [&](const uint4& t) {
        const float d2 = cloud_d2(x, y, z, t);
        if (d2 <= g.r2 && t.w != self) {
            ++within;
            knn_push(l, cloud_cand(d2, t));
        }
    });
    return within;
}

// the list of query i of q; self_base >= 0: query i is target self_base + i of the cloud, and skips it
template <int K>
__host__ __device__ __attribute__((always_inline)) inline int knn_query_list(const float* __restrict__ q, size_t i, const CloudGrid& g, long long self_base,
                                                                             KnnList<K>& l) {
    float x, y, z;
    int cx, cy, cz;
    knn_clear(l);
    if (!cloud_query_cell(q, i, g, x, y, z, cx, cy, cz)) return 0;
    return knn_search(x, y, z, cx, cy, cz, g, self_base >= 0 ? (unsigned)(self_base + (long long)i) : kKnnNoSelf, l);
}

// ---- the list variant: thread j serves query order[j] (order may be null: j itself); rows of k entries ---------------------
template <int K>
__host__ __device__ inline void knn_list_one(size_t j, const float* __restrict__ q, const int* __restrict__ order, const CloudGrid& g, long long self_base, int k,
                                             float* __restrict__ out_d2, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_within) {
    const size_t i = order ? (size_t)order[j] : j;
    KnnList<K> l;
    const int within = knn_query_list(q, i, g, self_base, l);
    float* d2 = out_d2 + i * (size_t)k;
    int32_t* idx = out_idx ? out_idx + i * (size_t)k : nullptr;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        if (e < k) {
            const unsigned long long key = l.key[e];
            const bool found = key != ~0ull;
            d2[e] = found ? cloud_float((uint32_t)(key >> 32)) : cloud_float(0x7f800000u);
            if (idx) idx[e] = found ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
        }
    }
    if (out_within) out_within[i] = within;
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_list(const float* __restrict__ q, int nq, const int* __restrict__ order, CloudGrid g, long long self_base, int k,
                                                  float* __restrict__ out_d2, int32_t* __restrict__ out_idx, int32_t* __restrict__ out_within) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)nq) knn_list_one<K>(j, q, order, g, self_base, k, out_d2, out_idx, out_within);
}

// ---- the reducing variant: the mean distance to the k nearest and the candidate count ------------------------------------------
template <int K>
__host__ __device__ inline void knn_reduce_one(size_t j, const float* __restrict__ q, const int* __restrict__ order, const CloudGrid& g, long long self_base, int k,
                                               float* __restrict__ out_mean, int32_t* __restrict__ out_within) {
    const size_t i = order ? (size_t)order[j] : j;
    KnnList<K> l;
    const int within = knn_query_list(q, i, g, self_base, l);
    float mean = cloud_float(0x7f800000u);
    if (within >= k) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < K; ++e)
            if (e < k) {
                const double d = sqrt((double)cloud_float((uint32_t)(l.key[e] >> 32)));
                s = e == 0 ? d : s + d;
            }
        mean = (float)(s / (double)k);
    }
    out_mean[i] = mean;
    out_within[i] = within;
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_reduce(const float* __restrict__ q, int nq, const int* __restrict__ order, CloudGrid g, long long self_base, int k,
                                                    float* __restrict__ out_mean, int32_t* __restrict__ out_within) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)nq) knn_reduce_one<K>(j, q, order, g, self_base, k, out_mean, out_within);
}

}  // namespace pm
