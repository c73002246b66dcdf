// pm_simplify.hpp -- simplification of an indexed triangle mesh by vertex clustering (mpmvs_simplify_mesh; contract: include/mpmvs.h,
// statement 4, and DESIGN.md section 25).  The clusters are the voxels of mpmvs_cloud_voxel_downsample on the mesh's vertices, found
// by the passes of pm_cloud.hpp and pm_voxel.hpp as they are (k_cloud_insert, k_voxel_first / flag / number / accumulate / finish and
// the scan); this header adds the triangle side and the placement of the representative.  Bit for bit the plain-loop statement and
// independent of scheduling: whatever is added up is an integer, and everything after the sums is a fixed sequence of fp64
// operations (no contraction; + - * / sqrt floor fabs, comparisons and llrint only).
//   k_simp_quadric   one thread per triangle with three finite vertices: the unit normal nh = C / L of the normals statement's cross
//                    product, and per corner the plane through that vertex in its cell's coordinates (the cell centre is 0, the
//                    cell edge 1): fix(nh_i * nh_j), i <= j, fix(nh_i * delta) and 1 go to the ten int64 sums of the corner's
//                    cluster (voxel_add / voxel_fix as they are; a term that is 0 is skipped; corners that share a cluster are summed
//                    in the thread and add once): 10 atomic adds for a triangle inside one cell, up to 30 otherwise.
//   k_simp_place     one thread per cluster: A = Q / 2^30, r = R / 2^30, eight cyclic Jacobi sweeps on A (normal_rotate of
//                    pm_normals.hpp, the state in named scalars: a runtime-indexed array would live in scratch), the pseudo-inverse
//                    about the cell mean x0 with the eigenvalues above 1e-3 of the largest, and the result only if it stays in the
//                    cell; placed = 0 (no plane), 1 (placed by the quadric) or 2 (fell back to the mean).  k_voxel_finish has
//                    written the mean (and the colour) before: a cluster that is not placed keeps those bits.
//   k_simp_classify  one thread per triangle: its class (alive, a non-finite vertex, collapsed) and its key, the three cluster
//                    numbers ascending; the classes are counted per wave.
//   k_simp_insert    the duplicate filter without a sort: an open-addressing table of uint32 triangle indices ("owners"), a power
//                    of two >= 2 x alive slots, all ones for empty.  A thread probes from a hash of its key: an empty slot is
//                    claimed with a compare-and-swap; a taken slot whose owner has the same key receives an atomic min of the
//                    thread's index; any other slot sends the probe on.  Why this is right: DESIGN.md section 25 (the key a slot
//                    stands for never changes once it is taken, the table is at most half full, the owner at the end is the
//                    smallest index of its key).
//   k_simp_owner     one thread per slot: kept[owner] = 1.  Then k_scan_tiles / k_scan_totals<Sum> over the kept flags.
//   k_simp_emit      kept triangles in their order, with the cluster numbers in the original corner order; tri_src[new] = old.
// Every per-thread body is host and device code, so that tools/mesh_simplify_check.cpp can replay it thread by thread under the host
// sanitizers; there the atomics are plain reads and writes.  The insert is written as a step function -- one access to the table per
// step -- so that the replay can interleave the probes of all threads at random.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pm_mesh.hpp"
#include "pm_normals.hpp"
#include "pm_voxel.hpp"

namespace pm {

constexpr uint32_t kSimpEmpty = 0xffffffffu;
constexpr int kSimpSums = 10;   // per cluster: Q00 Q01 Q02 Q11 Q12 Q22, R0 R1 R2, T
enum : unsigned char { kSimpAlive = 0, kSimpNonFinite = 1, kSimpCollapsed = 2 };

__host__ __device__ inline uint32_t simp_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
__host__ __device__ inline void simp_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
// smallest power of two >= max(2 * alive, 256), as an exponent (alive <= 2^30: at most 31)
__host__ __device__ inline int simp_slots_log2(long long alive) {
    int b = 8;
    while ((1ll << b) < 2 * alive) ++b;
    return b;
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void simp_quadric_one(size_t t, const float* __restrict__ xyz, const int32_t* __restrict__ tri, const VoxelGrid& g,
                                                 const int32_t* __restrict__ cluster_of, unsigned long long* __restrict__ QRT) {
    const size_t v[3] = {(size_t)tri[3 * t], (size_t)tri[3 * t + 1], (size_t)tri[3 * t + 2]};
    if (!(mesh_finite3(xyz, v[0]) && mesh_finite3(xyz, v[1]) && mesh_finite3(xyz, v[2]))) return;
    const double ax = (double)xyz[3 * v[0]], ay = (double)xyz[3 * v[0] + 1], az = (double)xyz[3 * v[0] + 2];
    const double ux = (double)xyz[3 * v[1]] - ax, uy = (double)xyz[3 * v[1] + 1] - ay, uz = (double)xyz[3 * v[1] + 2] - az;
    const double wx = (double)xyz[3 * v[2]] - ax, wy = (double)xyz[3 * v[2] + 1] - ay, wz = (double)xyz[3 * v[2] + 2] - az;
    const double Cx = uy * wz - uz * wy, Cy = uz * wx - ux * wz, Cz = ux * wy - uy * wx;
    const double L = sqrt((Cx * Cx + Cy * Cy) + Cz * Cz);
    if (!(L > 0.0) || !__builtin_isfinite(L)) return;
    const double nx = Cx / L, ny = Cy / L, nz = Cz / L;
    const long long q[6] = {voxel_fix(nx * nx), voxel_fix(nx * ny), voxel_fix(nx * nz), voxel_fix(ny * ny), voxel_fix(ny * nz), voxel_fix(nz * nz)};
    // per corner: its cluster and its three R terms
    int32_t cl[3];
    long long r[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = xyz + 3 * v[c];
        const double tx = ((double)p[0] - g.o[0]) / g.e, ty = ((double)p[1] - g.o[1]) / g.e, tz = ((double)p[2] - g.o[2]) / g.e;
        const double qx = (tx - floor(tx)) - 0.5, qy = (ty - floor(ty)) - 0.5, qz = (tz - floor(tz)) - 0.5;
        const double delta = (nx * qx + ny * qy) + nz * qz;
        cl[c] = cluster_of[v[c]];
        r[c][0] = voxel_fix(nx * delta), r[c][1] = voxel_fix(ny * delta), r[c][2] = voxel_fix(nz * delta);
    }
    // corners that share a cluster add once, with their terms summed here: the same integers reach the sums with a third of the
    // atomics wherever a triangle lies inside one cell, which is most triangles
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if ((c > 0 && cl[c] == cl[0]) || (c > 1 && cl[c] == cl[1])) continue;   // went with an earlier corner
        long long mult = 1, rs[3] = {r[c][0], r[c][1], r[c][2]};
#pragma unroll
        for (int j = c + 1; j < 3; ++j)
            if (cl[j] == cl[c]) {
                ++mult;
                rs[0] += r[j][0], rs[1] += r[j][1], rs[2] += r[j][2];
            }
        unsigned long long* s = QRT + (size_t)kSimpSums * (size_t)cl[c];
        for (int k = 0; k < 6; ++k)
            if (q[k] != 0) voxel_add(&s[k], q[k] * mult);
        for (int k = 0; k < 3; ++k)
            if (rs[k] != 0) voxel_add(&s[6 + k], rs[k]);
        voxel_add(&s[9], mult);
    }
}

// ---- placement ---------------------------------------------------------------------------------------------------------------------
// out_xyz[k] holds the mean (k_voxel_finish); it is overwritten only where placed = 1
__host__ __device__ inline void simp_place_one(size_t k, const float* __restrict__ xyz, const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                               const VoxelGrid& g, const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ QRT,
                                               float* __restrict__ out_xyz, unsigned char* __restrict__ placed) {
    const unsigned long long* s = QRT + (size_t)kSimpSums * k;
    if ((long long)s[9] == 0) {
        placed[k] = 0;
        return;
    }
    const double A00 = (double)(long long)s[0] / 0x1p30, A01 = (double)(long long)s[1] / 0x1p30, A02 = (double)(long long)s[2] / 0x1p30;
    const double A11 = (double)(long long)s[3] / 0x1p30, A12 = (double)(long long)s[4] / 0x1p30, A22 = (double)(long long)s[5] / 0x1p30;
    const double r0 = (double)(long long)s[6] / 0x1p30, r1 = (double)(long long)s[7] / 0x1p30, r2 = (double)(long long)s[8] / 0x1p30;
    double a00 = A00, a01 = A01, a02 = A02, a11 = A11, a12 = A12, a22 = A22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kNormalSweeps; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;   // cannot show: every further rotation would be skipped
        normal_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
        normal_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
        normal_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
    }
    double lmax = a00;
    lmax = a11 > lmax ? a11 : lmax;
    lmax = a22 > lmax ? a22 : lmax;
    if (!(lmax > 0.0)) {
        placed[k] = 2;
        return;
    }
    const double den = (double)(long long)count[k] * 0x1p30;
    const double x00 = (double)(long long)S[3 * k] / den - 0.5, x01 = (double)(long long)S[3 * k + 1] / den - 0.5, x02 = (double)(long long)S[3 * k + 2] / den - 0.5;
    const double g0 = r0 - ((A00 * x00 + A01 * x01) + A02 * x02);
    const double g1 = r1 - ((A01 * x00 + A11 * x01) + A12 * x02);
    const double g2 = r2 - ((A02 * x00 + A12 * x01) + A22 * x02);
    const double cut = 1e-3 * lmax;
    const double y0 = a00 > cut ? ((v00 * g0 + v10 * g1) + v20 * g2) / a00 : 0.0;
    const double y1 = a11 > cut ? ((v01 * g0 + v11 * g1) + v21 * g2) / a11 : 0.0;
    const double y2 = a22 > cut ? ((v02 * g0 + v12 * g1) + v22 * g2) / a22 : 0.0;
    const double x0 = x00 + ((v00 * y0 + v01 * y1) + v02 * y2);
    const double x1 = x01 + ((v10 * y0 + v11 * y1) + v12 * y2);
    const double x2 = x02 + ((v20 * y0 + v21 * y1) + v22 * y2);
    if (!(fabs(x0) <= 0.5 && fabs(x1) <= 0.5 && fabs(x2) <= 0.5)) {   // false for a NaN: the representative stays in its cell
        placed[k] = 2;
        return;
    }
    placed[k] = 1;
    const float* lead = xyz + 3 * (size_t)first[k];
    const double x[3] = {x0, x1, x2};
    for (int a = 0; a < 3; ++a) {
        const double c = floor(((double)lead[a] - g.o[a]) / g.e);
        out_xyz[3 * k + a] = (float)(g.o[a] + (c + (0.5 + x[a])) * g.e);
    }
}

// ---- triangles -----------------------------------------------------------------------------------------------------------------------
// the class of triangle t and, for an alive one, its key; returns the class
__host__ __device__ inline int simp_classify_one(size_t t, const int32_t* __restrict__ tri, const int32_t* __restrict__ cluster_of, unsigned char* __restrict__ cls,
                                                 int32_t* __restrict__ key) {
    const int32_t A = cluster_of[tri[3 * t]], B = cluster_of[tri[3 * t + 1]], C = cluster_of[tri[3 * t + 2]];
    int c = kSimpAlive;
    if (A < 0 || B < 0 || C < 0) c = kSimpNonFinite;
    else if (A == B || B == C || A == C) c = kSimpCollapsed;
    cls[t] = (unsigned char)c;
    if (c == kSimpAlive) {
        const int32_t lo = A < B ? (A < C ? A : C) : (B < C ? B : C);
        const int32_t hi = A > B ? (A > C ? A : C) : (B > C ? B : C);
        key[3 * t] = lo;
        key[3 * t + 1] = (int32_t)(((long long)A + B + C) - lo - hi);
        key[3 * t + 2] = hi;
    }
    return c;
}
__host__ __device__ inline uint32_t simp_hash(const int32_t* __restrict__ key) {
    const unsigned long long k = cloud_mix((unsigned long long)(uint32_t)key[0] | ((unsigned long long)(uint32_t)key[1] << 32));
    return (uint32_t)cloud_mix(k ^ ((unsigned long long)(uint32_t)key[2] * 0x9e3779b97f4a7c15ull));
}
__host__ __device__ inline bool simp_same_key(const int32_t* __restrict__ key, size_t a, size_t b) {
    return key[3 * a] == key[3 * b] && key[3 * a + 1] == key[3 * b + 1] && key[3 * a + 2] == key[3 * b + 2];
}

// the probe of one alive triangle: h = the slot it looks at next, cur = the owner it found there (kSimpEmpty: none yet)
struct SimpProbe {
    uint32_t h, cur;
};
__host__ __device__ inline SimpProbe simp_probe_begin(size_t t, const int32_t* __restrict__ key, uint32_t mask) { return SimpProbe{simp_hash(key + 3 * t) & mask, kSimpEmpty}; }
// one step = one access to the table; true when the thread is done.
//   step A (cur == empty): read the slot; an empty one is claimed by compare-and-swap (a stale "empty" is settled by the swap).  Claimed:
//                          done.  Otherwise cur = the owner seen: it may be replaced later, but only by a triangle of the same key.
//   step B (cur == owner): the same key: atomic min of t into the slot, done; another key: on to the next slot.
__host__ __device__ inline bool simp_insert_step(size_t t, SimpProbe& p, const int32_t* __restrict__ key, uint32_t mask, uint32_t* __restrict__ table) {
    if (p.cur == kSimpEmpty) {
        uint32_t cur = table[p.h];
        if (cur == kSimpEmpty) {
            cur = simp_cas(&table[p.h], kSimpEmpty, (uint32_t)t);
            if (cur == kSimpEmpty) return true;
        }
        p.cur = cur;
        return false;
    }
    if (simp_same_key(key, t, (size_t)p.cur)) {
        simp_min(&table[p.h], (uint32_t)t);
        return true;
    }
    p.h = (p.h + 1) & mask;
    p.cur = kSimpEmpty;
    return false;
}
// the table holds at least twice as many slots as there are alive triangles, so an empty slot ends every probe within `mask` steps
__host__ __device__ inline void simp_insert_one(size_t t, const unsigned char* __restrict__ cls, const int32_t* __restrict__ key, uint32_t mask,
                                                uint32_t* __restrict__ table) {
    if (cls[t] != kSimpAlive) return;
    SimpProbe p = simp_probe_begin(t, key, mask);
    for (unsigned long long step = 0; step < 2ull * mask + 2ull; ++step)
        if (simp_insert_step(t, p, key, mask, table)) return;
}
__host__ __device__ inline void simp_owner_one(size_t s, const uint32_t* __restrict__ table, int* __restrict__ kept) {
    const uint32_t o = table[s];
    if (o != kSimpEmpty) kept[o] = 1;
}
__host__ __device__ inline void simp_emit_one(size_t t, const int32_t* __restrict__ tri, const int32_t* __restrict__ cluster_of, const int* __restrict__ kept,
                                              const int* __restrict__ excl, const int* __restrict__ tile, int32_t* __restrict__ out_tri, int32_t* __restrict__ out_src) {
    if (!kept[t]) return;
    const size_t j = (size_t)mesh_new_index(t, excl, tile);
    for (int k = 0; k < 3; ++k) out_tri[3 * j + k] = cluster_of[tri[3 * t + k]];
    out_src[j] = (int32_t)t;
}

__global__ __launch_bounds__(256) void k_simp_quadric(int m, const float* __restrict__ xyz, const int32_t* __restrict__ tri, VoxelGrid g,
                                                      const int32_t* __restrict__ cluster_of, unsigned long long* __restrict__ QRT) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) simp_quadric_one(t, xyz, tri, g, cluster_of, QRT);
}
__global__ __launch_bounds__(256) void k_simp_place(int nc, const float* __restrict__ xyz, const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                    VoxelGrid g, const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ QRT,
                                                    float* __restrict__ out_xyz, unsigned char* __restrict__ placed) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < (size_t)nc) simp_place_one(k, xyz, first, count, g, S, QRT, out_xyz, placed);
}
// class_count[c] += the triangles of class c, one add per class and wave
__global__ __launch_bounds__(256) void k_simp_classify(int m, const int32_t* __restrict__ tri, const int32_t* __restrict__ cluster_of, unsigned char* __restrict__ cls,
                                                       int32_t* __restrict__ key, int* __restrict__ class_count) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    cc_count_wave(t < (size_t)m ? simp_classify_one(t, tri, cluster_of, cls, key) : -1, class_count);
}
__global__ __launch_bounds__(256) void k_simp_insert(int m, const unsigned char* __restrict__ cls, const int32_t* __restrict__ key, uint32_t mask,
                                                     uint32_t* __restrict__ table) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) simp_insert_one(t, cls, key, mask, table);
}
__global__ __launch_bounds__(256) void k_simp_owner(uint32_t slots, const uint32_t* __restrict__ table, int* __restrict__ kept) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s < (size_t)slots) simp_owner_one(s, table, kept);
}
__global__ __launch_bounds__(256) void k_simp_emit(int m, const int32_t* __restrict__ tri, const int32_t* __restrict__ cluster_of, const int* __restrict__ kept,
                                                   const int* __restrict__ excl, const int* __restrict__ tile, int32_t* __restrict__ out_tri,
                                                   int32_t* __restrict__ out_src) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) simp_emit_one(t, tri, cluster_of, kept, excl, tile, out_tri, out_src);
}

}  // namespace pm
