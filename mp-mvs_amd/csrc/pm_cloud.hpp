// pm_cloud.hpp -- exact capped nearest neighbour between two point clouds (mpmvs_cloud_*; contract: DESIGN.md section 13 and
// include/mpmvs.h).  Per query q the lexicographic minimum of (d2, index) over the finite targets p with
//   dx = qx - px, dy, dz in fp32;  d2 = (dx*dx + dy*dy) + dz*dz in fp32 (no contraction);  d2 <= r2 = radius * radius (fp32)
// or (+inf, -1) when there is none.  Bit for bit the brute-force statement; independent of scheduling.
//
// Structure: a sparse uniform grid of cell edge `edge` > radius addressed through an open-addressing hash table; no sort and no
// dense cell array.  Cell coordinate per axis: floor(((double)x - min) / edge) with min the finite bounding-box minimum, three
// coordinates of 21 bits packed into a u64 key.  edge = max(radius, 2^-60) * (1 + 2^-10), so that the 3 x 3 x 3 cells around a
// query's cell hold every candidate: the argument stands at cloud_walk below, the one walk over them that every search of the
// library (nearest, align, kNN, normals, components) goes through.
//
// Passes of a grid build (integer bookkeeping only; what depends on scheduling -- the slot a key lands in, the order inside a
// cell -- never reaches a result, because a query takes the minimum of (d2, index) over whole cells):
//   1. k_cloud_insert   per finite target: key -> slot by linear probing with a 64-bit compare-and-swap (a probe never waits:
//                       it claims the slot, finds its own key, or moves on; slots >= 2 x finite points, so the table cannot
//                       fill and a probe sequence is bounded by the table size), count per slot with an integer atomic.
//   2. k_cloud_stats    occupied slots and the fullest cell.
//   3. scan             slot counts -> offsets: k_scan_tiles, k_scan_totals<Sum> and k_vs_scan_add (pm_scan.hpp).
//   4. k_cloud_scatter  (x, y, z, original index) of every target into its cell's run: one 16-byte record per candidate.
// Passes of a query call:
//   5. k_cloud_qbin / scan / k_cloud_qorder   the queries binned by the hash of their own cell, so that the 64 queries of a
//                       wave sit in few cells and read the same target runs out of L1 / L2 (MPMVS_CLOUD_BIN=0: caller order).
//   6. k_cloud_query    one thread per query: cloud_walk with the minimum of (d2, index) as its visitor, results in caller order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_scan.hpp"

namespace pm {

constexpr int kCloudAxisBits = 21;
constexpr int kCloudAxisCells = 1 << kCloudAxisBits;
constexpr unsigned long long kCloudEmpty = ~0ull;   // no key: a key uses 63 bits
constexpr int kCloudMaxSlotsLog2 = 30;              // the scans and the slot indices are ints

// ---- key, packing and probing arithmetic, and the per-thread body of every kernel but the stats: host and device, so that a
// host program (tools/cloud_table_check.cpp) can replay the passes thread by thread, under the sanitizers ------------------
__host__ __device__ inline double cloud_edge(float radius) {
    const double r = (double)radius < 0x1p-60 ? 0x1p-60 : (double)radius;
    return r * (1.0 + 0x1p-10);
}
__host__ __device__ inline uint32_t cloud_bits(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return b.u;
}
__host__ __device__ inline float cloud_float(uint32_t u) {
    union { float f; uint32_t u; } b;
    b.u = u;
    return b.f;
}
__host__ __device__ inline bool cloud_finite(float v) { return (cloud_bits(v) & 0x7f800000u) != 0x7f800000u; }
// the atomics of the passes; the host replay runs one thread at a time
__host__ __device__ inline unsigned long long cloud_cas(unsigned long long* p, unsigned long long expect, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const unsigned long long old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
__host__ __device__ inline int cloud_fetch_add(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const int old = *p;
    *p = old + v;
    return old;
#endif
}
// cell coordinate of a finite x, clamped to [-2, cells + 1]: a clamped query has no neighbour cell inside [0, cells)
__host__ __device__ inline int cloud_cell(float x, double mn, double edge) {
    double t = floor(((double)x - mn) / edge);
    t = t < -2.0 ? -2.0 : t;
    t = t > (double)(kCloudAxisCells + 1) ? (double)(kCloudAxisCells + 1) : t;
    return (int)t;
}
__host__ __device__ inline bool cloud_cell_ok(int c) { return (unsigned)c < (unsigned)kCloudAxisCells; }
__host__ __device__ inline unsigned long long cloud_key(int cx, int cy, int cz) {
    return (unsigned long long)cx | ((unsigned long long)cy << kCloudAxisBits) | ((unsigned long long)cz << (2 * kCloudAxisBits));
}
__host__ __device__ inline unsigned long long cloud_mix(unsigned long long k) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}
// smallest power of two >= max(2 n, 256), as an exponent; > kCloudMaxSlotsLog2 means "too many"
__host__ __device__ inline int cloud_slots_log2(long long n_finite) {
    int b = 8;
    while (b <= kCloudMaxSlotsLog2 && (1ll << b) < 2 * n_finite) ++b;
    return b;
}

// The kernels below are `inline`: two translation units of the library include this header (the clouds and, for its clustering, the
// mesh simplification), as pm_scan.hpp says of its own.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"

// host only -- the pass over the coordinates that every entry point which builds a grid makes: the number of points with three finite
// coordinates and their bounding box (mn, mx untouched when there is none)
inline long long cloud_bbox(long long n, const float* xyz, float mn[3], float mx[3]) {
    long long n_fin = 0;
    for (long long i = 0; i < n; ++i) {
        const float* p = xyz + 3 * i;
        if (!(cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]))) continue;
        for (int a = 0; a < 3; ++a) {
            mn[a] = n_fin ? (p[a] < mn[a] ? p[a] : mn[a]) : p[a];
            mx[a] = n_fin ? (p[a] > mx[a] ? p[a] : mx[a]) : p[a];
        }
        ++n_fin;
    }
    return n_fin;
}

struct CloudGrid {
    double mn[3];
    double edge;
    float r2;
    unsigned mask;                        // slots - 1
    const unsigned long long* keys;       // [slots]
    const int* off;                       // [slots + 1]
    const uint4* pts;                     // [finite targets]: x, y, z bits and the original index, cell by cell
};

// ---- build -----------------------------------------------------------------------------------------------------------
__host__ __device__ inline void cloud_insert_one(size_t i, const float* __restrict__ xyz, double mnx, double mny, double mnz, double edge, unsigned mask,
                                                 unsigned long long* __restrict__ keys, int* __restrict__ cnt, int* __restrict__ slot_of) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    int s = -1;
    if (cloud_finite(x) && cloud_finite(y) && cloud_finite(z)) {
        int cx = cloud_cell(x, mnx, edge), cy = cloud_cell(y, mny, edge), cz = cloud_cell(z, mnz, edge);
        cx = cx < 0 ? 0 : (cx > kCloudAxisCells - 1 ? kCloudAxisCells - 1 : cx);
        cy = cy < 0 ? 0 : (cy > kCloudAxisCells - 1 ? kCloudAxisCells - 1 : cy);
        cz = cz < 0 ? 0 : (cz > kCloudAxisCells - 1 ? kCloudAxisCells - 1 : cz);
        const unsigned long long key = cloud_key(cx, cy, cz);
        unsigned h = (unsigned)cloud_mix(key) & mask;
        for (unsigned probe = 0; probe <= mask; ++probe) {
            // a slot changes once, from empty to its key: a key read here is final, an "empty" may be stale and is settled by the swap
            unsigned long long cur = keys[h];
            if (cur == kCloudEmpty) {
                cur = cloud_cas(&keys[h], kCloudEmpty, key);
                if (cur == kCloudEmpty) cur = key;
            }
            if (cur == key) {
                s = (int)h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (s >= 0) cloud_fetch_add(&cnt[s], 1);
    }
    slot_of[i] = s;
}

inline __global__ __launch_bounds__(256) void k_cloud_insert(const float* __restrict__ xyz, int n, double mnx, double mny, double mnz, double edge, unsigned mask,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ cnt, int* __restrict__ slot_of) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cloud_insert_one(i, xyz, mnx, mny, mnz, edge, mask, keys, cnt, slot_of);
}

// st[0] += occupied slots, st[1] = max(count)
inline __global__ __launch_bounds__(256) void k_cloud_stats(const int* __restrict__ cnt, unsigned slots, int* __restrict__ st) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int c = k < slots ? cnt[k] : 0;
    int occ = c > 0 ? 1 : 0, mx = c;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        occ += __shfl_xor(occ, d, 64);
        mx = max(mx, __shfl_xor(mx, d, 64));
    }
    if ((threadIdx.x & 63) == 0 && occ > 0) {
        atomicAdd(&st[0], occ);
        atomicMax(&st[1], mx);
    }
}

// cnt counts down to 0 while the runs fill
__host__ __device__ inline void cloud_scatter_one(size_t i, const float* __restrict__ xyz, const int* __restrict__ slot_of, const int* __restrict__ off,
                                                  int* __restrict__ cnt, uint4* __restrict__ pts) {
    const int s = slot_of[i];
    if (s < 0) return;
    const int pos = off[s] + cloud_fetch_add(&cnt[s], -1) - 1;
    uint4 rec;
    rec.x = cloud_bits(xyz[3 * i]), rec.y = cloud_bits(xyz[3 * i + 1]), rec.z = cloud_bits(xyz[3 * i + 2]), rec.w = (unsigned)i;
    pts[pos] = rec;
}

inline __global__ __launch_bounds__(256) void k_cloud_scatter(const float* __restrict__ xyz, int n, const int* __restrict__ slot_of, const int* __restrict__ off,
                                                       int* __restrict__ cnt, uint4* __restrict__ pts) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cloud_scatter_one(i, xyz, slot_of, off, cnt, pts);
}

// ---- query -----------------------------------------------------------------------------------------------------------
// the (clamped) cell of a query point; false, and no cell, if a coordinate is not finite
__host__ __device__ inline bool cloud_point_cell(float x, float y, float z, const CloudGrid& g, int& cx, int& cy, int& cz) {
    if (!(cloud_finite(x) && cloud_finite(y) && cloud_finite(z))) return false;
    cx = cloud_cell(x, g.mn[0], g.edge), cy = cloud_cell(y, g.mn[1], g.edge), cz = cloud_cell(z, g.mn[2], g.edge);
    return true;
}
__host__ __device__ inline bool cloud_query_cell(const float* __restrict__ q, size_t i, const CloudGrid& g, float& x, float& y, float& z, int& cx, int& cy,
                                                 int& cz) {
    x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    return cloud_point_cell(x, y, z, g, cx, cy, cz);
}

// bin of a query: the hash of its own (clamped) cell; a query without a cell goes to bin 0
__host__ __device__ inline int cloud_cell_bin(int cx, int cy, int cz, unsigned bin_mask) {
    return (int)((unsigned)cloud_mix(((unsigned long long)(cx + 2) | ((unsigned long long)(cy + 2) << 22)) ^ cloud_mix((unsigned long long)(cz + 2))) & bin_mask);
}
__host__ __device__ inline void cloud_qbin_one(size_t i, const float* __restrict__ q, const CloudGrid& g, unsigned bin_mask, int* __restrict__ qcnt,
                                               int* __restrict__ qbin) {
    float x, y, z;
    int cx, cy, cz, b = 0;
    if (cloud_query_cell(q, i, g, x, y, z, cx, cy, cz)) b = cloud_cell_bin(cx, cy, cz, bin_mask);
    qbin[i] = b;
    cloud_fetch_add(&qcnt[b], 1);
}

inline __global__ __launch_bounds__(256) void k_cloud_qbin(const float* __restrict__ q, int nq, CloudGrid g, unsigned bin_mask, int* __restrict__ qcnt,
                                                    int* __restrict__ qbin) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)nq) cloud_qbin_one(i, q, g, bin_mask, qcnt, qbin);
}

__host__ __device__ inline void cloud_qorder_one(size_t i, const int* __restrict__ qbin, const int* __restrict__ qoff, int* __restrict__ qcnt,
                                                 int* __restrict__ order) {
    const int b = qbin[i];
    order[qoff[b] + cloud_fetch_add(&qcnt[b], -1) - 1] = (int)i;
}

inline __global__ __launch_bounds__(256) void k_cloud_qorder(int nq, const int* __restrict__ qbin, const int* __restrict__ qoff, int* __restrict__ qcnt,
                                                      int* __restrict__ order) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)nq) cloud_qorder_one(i, qbin, qoff, qcnt, order);
}

// the slot that holds `key`, -1 if the table has none: the probe walks from the key's hash to the key or to the first empty slot
// (an insert never leaves a gap before its key), and the table is never full, so it ends within the table's size
__host__ __device__ inline int cloud_lookup(unsigned long long key, const CloudGrid& g) {
    unsigned h = (unsigned)cloud_mix(key) & g.mask;
    int s = -1;
    for (unsigned probe = 0; probe <= g.mask; ++probe) {
        const unsigned long long cur = g.keys[h];
        if (cur == key) s = (int)h;
        if (cur == key || cur == kCloudEmpty) break;
        h = (h + 1) & g.mask;
    }
    return s;
}

// THE CANDIDATE WALK, the only one: the 3 x 3 x 3 cells around the query's cell (cx, cy, cz), less those outside [0, cells); each
// one looked up, and every record t of a found cell's run (x, y, z bits and the caller's index in t.w) handed to visit(t).
// Why 27 cells suffice: a candidate is at most radius * (1 + 4 * 2^-24) away along an axis (one rounding in the difference, one
// in the square, two in the sums), the fp64 cell coordinate carries an error below 2^21 * 2^-51, and edge = max(radius, 2^-60) *
// (1 + 2^-10), so the coordinates of a query and of a candidate differ by less than (1 + 2.4e-7) / (1 + 9.77e-4) + 1e-9 < 1
// before the floor: by at most one after it.  (The 2^-60 floor keeps the bound where radius * radius underflows in fp32.)
// The visitor decides what a candidate is and in which order it tests: the walk computes no distance.  Always inlined, host and
// device: a visitor's state stays in the caller's registers.
// kUnroll is the unroll count of the dy and dx loops, so that what the code looks like does not hang on the compiler's size
// threshold: 3 writes the nine cells of a layer out (the nearest search: its kernels always were compiled so), 1 keeps them
// rolled (the list kernels, 22 and 50 registers lighter at K = 4 and 8 than with nine copies; the hook pass: never unrolled).
// Figures: DESIGN.md section 13.8.
template <int kUnroll, typename Visit>
__host__ __device__ __attribute__((always_inline)) inline void cloud_walk(int cx, int cy, int cz, const CloudGrid& g, Visit&& visit) {
    for (int dz = -1; dz <= 1; ++dz) {
        if (!cloud_cell_ok(cz + dz)) continue;
#pragma unroll kUnroll
        for (int dy = -1; dy <= 1; ++dy) {
            if (!cloud_cell_ok(cy + dy)) continue;
#pragma unroll kUnroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!cloud_cell_ok(cx + dx)) continue;
                const int s = cloud_lookup(cloud_key(cx + dx, cy + dy, cz + dz), g);
                if (s < 0) continue;
                const int e = g.off[s + 1];
                for (int p = g.off[s]; p < e; ++p) {
                    const uint4 t = g.pts[p];   // a copy: one 16-byte load, whatever fields the visitor reads
                    visit(t);
                }
            }
        }
    }
}

// the squared distance of the query (x, y, z) to the record t, in fp32: the one expression every result is stated in
__host__ __device__ inline float cloud_d2(float x, float y, float z, const uint4& t) {
    const float ddx = x - cloud_float(t.x), ddy = y - cloud_float(t.y), ddz = z - cloud_float(t.z);
    return (ddx * ddx + ddy * ddy) + ddz * ddz;
}
// the key of a candidate: (d2 bits << 32) | index; d2 >= +0, so its bits order as integers
__host__ __device__ inline unsigned long long cloud_cand(float d2, const uint4& t) { return ((unsigned long long)cloud_bits(d2) << 32) | t.w; }

// the search for the query (x, y, z) of cell (cx, cy, cz): the minimum key over the candidates, ~0 if there is none.  Shared by
// k_cloud_query and k_align_pass (pm_align.hpp).
__host__ __device__ inline unsigned long long cloud_search(float x, float y, float z, int cx, int cy, int cz, const CloudGrid& g) {
    unsigned long long best = ~0ull;
    cloud_walk<3>(cx, cy, cz, g, [&](const uint4& t) {
        // no branch (& and a select): the index is then needed whatever d2 is, and the record stays one 16-byte load; behind a
        // branch the compiler fetches the index in a second, dependent load per candidate (query time + 35 %)
        const float d2 = cloud_d2(x, y, z, t);
        const unsigned long long cand = cloud_cand(d2, t);
        best = ((d2 <= g.r2) & (cand < best)) ? cand : best;
    });
    return best;
}

// the query thread j serves is order[j] (order may be null: j itself)
__host__ __device__ inline void cloud_query_one(size_t j, const float* __restrict__ q, const int* __restrict__ order, const CloudGrid& g,
                                                float* __restrict__ out_d2, int32_t* __restrict__ out_idx) {
    const size_t i = order ? (size_t)order[j] : j;
    float x, y, z;
    int cx, cy, cz;
    unsigned long long best = ~0ull;
    if (cloud_query_cell(q, i, g, x, y, z, cx, cy, cz)) best = cloud_search(x, y, z, cx, cy, cz, g);
    const bool found = best != ~0ull;
    out_d2[i] = found ? cloud_float((uint32_t)(best >> 32)) : cloud_float(0x7f800000u);
    if (out_idx) out_idx[i] = found ? (int32_t)(uint32_t)(best & 0xffffffffull) : -1;
}

// one thread per query
inline __global__ __launch_bounds__(256) void k_cloud_query(const float* __restrict__ q, int nq, const int* __restrict__ order, CloudGrid g, float* __restrict__ out_d2,
                                                     int32_t* __restrict__ out_idx) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)nq) cloud_query_one(j, q, order, g, out_d2, out_idx);
}
#pragma clang diagnostic pop

}  // namespace pm
