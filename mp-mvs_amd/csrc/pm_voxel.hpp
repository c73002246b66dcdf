// pm_voxel.hpp -- voxel-grid downsampling of a point cloud (mpmvs_cloud_voxel_downsample; contract: DESIGN.md section 16 and
// include/mpmvs.h).  Every occupied cell of a uniform grid of edge e = (double)voxel gives one output point: the mean position,
// the normalised sum of the normals and the rounded mean colour of its members.  Bit for bit the plain-loop statement and
// independent of scheduling, because everything that is added up is an integer:
//   o[a] = (double)mn[a] - 0.5 * e;  t_a = ((double)x_a - o[a]) / e;  c_a = floor(t_a)   (fp64, no contraction; the lowest point
//   sits at a cell centre, and o <= mn makes every c_a >= 0);  fix(x) = llrint(x * 2^30), round to nearest even;
//   S[v][a] += fix(t_a - c_a);  N[v][a] += fix(clamp((double)n_a, -1, 1)) for a normal without a non-finite component;
//   C[v][k] += the colour byte.  Each position or normal term is at most 2^30 in magnitude and a voxel has at most 2^31 - 1
//   members, so every |sum| < 2^61.
// The voxels are numbered by their smallest member index ("first appearance").
//
// Structure: the hashed sparse grid of pm_cloud.hpp (one table slot per occupied cell; which slot a cell lands in depends on
// scheduling and never reaches a result) and the block scan of pm_scan.hpp.  Passes:
//   1. k_cloud_insert     (pm_cloud.hpp, with (o, e) for (mn, edge); the host's span check keeps its clamps from firing):
//                         slot_of per point, member count per slot.
//   2. k_voxel_first      per point: unsigned atomic min of its index into first[slot].
//   3. k_voxel_flag       per point: 1 iff it is its slot's first member (the voxel's LEADER); then the exclusive scan of the
//      + scan             flags over the points -- k_scan_tiles, k_scan_totals<Sum>, k_vs_scan_add -- numbers the voxels, and
//                         its grand total is m.  The host reads m here and sizes everything below by it.
//   4. k_voxel_number     per leader: vox_of_slot[slot] = v, out_first[v] = i, out_count[v] = the slot's count.
//   5. k_voxel_accumulate per point: 64-bit integer atomic adds into S, N, C of its voxel; out_voxel_of.
//   6. k_voxel_finish     per voxel: the fp64 arithmetic of the contract (the cell is recomputed from the leader's coordinates).
// The per-thread body of passes 2-6 is host and device code, so that tools/voxel_check.cpp can replay them thread by thread
// under the sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"

namespace pm {

struct VoxelGrid {
    double o[3];   // (double)mn - 0.5 * e
    double e;      // (double)voxel
};

__host__ __device__ inline void voxel_origin(const float mn[3], float voxel, VoxelGrid& g) {
    g.e = (double)voxel;
    for (int a = 0; a < 3; ++a) g.o[a] = (double)mn[a] - 0.5 * g.e;
}

// the atomics of the passes; the host replay runs one thread at a time
__host__ __device__ inline void voxel_min(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
__host__ __device__ inline void voxel_add(unsigned long long* p, long long v) {   // two's complement: the unsigned add is the signed one
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, (unsigned long long)v);
#else
    *p += (unsigned long long)v;
#endif
}
__host__ __device__ inline long long voxel_fix(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(x * 0x1p30);
#else
    return llrint(x * 0x1p30);   // the default rounding mode: to nearest even
#endif
}

// host only -- the cell-span limit of the grid over the finite bounding box: the first axis whose highest point lies in cell 2^21 or
// beyond (the cells are monotonic in x), with that cell in *top; -1 if every axis fits
inline int voxel_span_axis(const float mx[3], const VoxelGrid& g, double* top) {
    for (int a = 0; a < 3; ++a) {
        *top = floor(((double)mx[a] - g.o[a]) / g.e);
        if (!(*top < (double)kCloudAxisCells)) return a;
    }
    return -1;
}

// the kernels are `inline`: the clouds and the mesh simplification include this header from two translation units
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
// ---- pass 2 ------------------------------------------------------------------------------------------------------------
// first[] starts as all ones: above every index
__host__ __device__ inline void voxel_first_one(size_t i, const int* __restrict__ slot_of, unsigned* __restrict__ first) {
    const int s = slot_of[i];
    if (s >= 0) voxel_min(&first[s], (unsigned)i);
}
inline __global__ __launch_bounds__(256) void k_voxel_first(int n, const int* __restrict__ slot_of, unsigned* __restrict__ first) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) voxel_first_one(i, slot_of, first);
}

// ---- pass 3 (the scan itself is pm_scan.hpp's) ---------------------------------------------------------------------------
__host__ __device__ inline void voxel_flag_one(size_t i, const int* __restrict__ slot_of, const unsigned* __restrict__ first, int* __restrict__ flag) {
    const int s = slot_of[i];
    flag[i] = (s >= 0 && first[s] == (unsigned)i) ? 1 : 0;
}
inline __global__ __launch_bounds__(256) void k_voxel_flag(int n, const int* __restrict__ slot_of, const unsigned* __restrict__ first, int* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) voxel_flag_one(i, slot_of, first, flag);
}

// ---- pass 4 ------------------------------------------------------------------------------------------------------------
// num[i] = the leaders before i: a leader's voxel number
__host__ __device__ inline void voxel_number_one(size_t i, const int* __restrict__ flag, const int* __restrict__ num, const int* __restrict__ slot_of,
                                                 const int* __restrict__ cnt, int* __restrict__ vox_of_slot, int32_t* __restrict__ out_first,
                                                 int32_t* __restrict__ out_count) {
    if (!flag[i]) return;
    const int s = slot_of[i], v = num[i];
    vox_of_slot[s] = v;
    out_first[v] = (int32_t)i;
    out_count[v] = cnt[s];
}
inline __global__ __launch_bounds__(256) void k_voxel_number(int n, const int* __restrict__ flag, const int* __restrict__ num, const int* __restrict__ slot_of,
                                                      const int* __restrict__ cnt, int* __restrict__ vox_of_slot, int32_t* __restrict__ out_first,
                                                      int32_t* __restrict__ out_count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) voxel_number_one(i, flag, num, slot_of, cnt, vox_of_slot, out_first, out_count);
}

// ---- pass 5 ------------------------------------------------------------------------------------------------------------
// the three terms a finite point adds to S
__host__ __device__ inline void voxel_pos_terms(const float* __restrict__ p, const VoxelGrid& g, long long term[3]) {
    for (int a = 0; a < 3; ++a) {
        const double t = ((double)p[a] - g.o[a]) / g.e;
        term[a] = voxel_fix(t - floor(t));
    }
}
// normals, rgb, N, C, voxel_of: null = not wanted
__host__ __device__ inline void voxel_accumulate_one(size_t i, const float* __restrict__ xyz, const float* __restrict__ normals,
                                                     const unsigned char* __restrict__ rgb, const VoxelGrid& g, const int* __restrict__ slot_of,
                                                     const int* __restrict__ vox_of_slot, unsigned long long* __restrict__ S,
                                                     unsigned long long* __restrict__ N, unsigned long long* __restrict__ C, int32_t* __restrict__ voxel_of) {
    const int s = slot_of[i];
    if (s < 0) {
        if (voxel_of) voxel_of[i] = -1;
        return;
    }
    const size_t v = (size_t)vox_of_slot[s];
    if (voxel_of) voxel_of[i] = (int32_t)v;
    long long term[3];
    voxel_pos_terms(xyz + 3 * i, g, term);
    for (int a = 0; a < 3; ++a) voxel_add(&S[3 * v + a], term[a]);
    if (normals) {
        const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
        if (cloud_finite(nx) && cloud_finite(ny) && cloud_finite(nz)) {
            const float nn[3] = {nx, ny, nz};
            for (int a = 0; a < 3; ++a) {
                double d = (double)nn[a];
                d = d > 1.0 ? 1.0 : d;
                d = d < -1.0 ? -1.0 : d;
                const long long f = voxel_fix(d);
                if (f != 0) voxel_add(&N[3 * v + a], f);
            }
        }
    }
    if (rgb)
        for (int k = 0; k < 3; ++k) {
            const unsigned char b = rgb[3 * i + k];
            if (b) voxel_add(&C[3 * v + k], (long long)b);
        }
}
inline __global__ __launch_bounds__(256) void k_voxel_accumulate(int n, const float* __restrict__ xyz, const float* __restrict__ normals,
                                                          const unsigned char* __restrict__ rgb, VoxelGrid g, const int* __restrict__ slot_of,
                                                          const int* __restrict__ vox_of_slot, unsigned long long* __restrict__ S,
                                                          unsigned long long* __restrict__ N, unsigned long long* __restrict__ C,
                                                          int32_t* __restrict__ voxel_of) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) voxel_accumulate_one(i, xyz, normals, rgb, g, slot_of, vox_of_slot, S, N, C, voxel_of);
}

// ---- pass 6 ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void voxel_finish_one(size_t v, const float* __restrict__ xyz, const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                 const VoxelGrid& g, const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ N,
                                                 const unsigned long long* __restrict__ C, float* __restrict__ out_xyz, float* __restrict__ out_normals,
                                                 unsigned char* __restrict__ out_rgb) {
    const float* lead = xyz + 3 * (size_t)first[v];
    const long long cn = (long long)count[v];
    const double den = (double)cn * 0x1p30;   // exact: 31 bits times a power of two
    for (int a = 0; a < 3; ++a) {
        const double c = floor(((double)lead[a] - g.o[a]) / g.e);
        const double mean = (double)(long long)S[3 * v + a] / den;
        out_xyz[3 * v + a] = (float)(g.o[a] + (c + mean) * g.e);
    }
    if (out_normals) {
        const double n0 = (double)(long long)N[3 * v], n1 = (double)(long long)N[3 * v + 1], n2 = (double)(long long)N[3 * v + 2];
        const double L = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        out_normals[3 * v] = L == 0.0 ? 0.0f : (float)(n0 / L);
        out_normals[3 * v + 1] = L == 0.0 ? 0.0f : (float)(n1 / L);
        out_normals[3 * v + 2] = L == 0.0 ? 0.0f : (float)(n2 / L);
    }
    if (out_rgb)
        for (int k = 0; k < 3; ++k) out_rgb[3 * v + k] = (unsigned char)((2 * (long long)C[3 * v + k] + cn) / (2 * cn));   // round half up
}
inline __global__ __launch_bounds__(256) void k_voxel_finish(int m, const float* __restrict__ xyz, const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                      VoxelGrid g, const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ N,
                                                      const unsigned long long* __restrict__ C, float* __restrict__ out_xyz, float* __restrict__ out_normals,
                                                      unsigned char* __restrict__ out_rgb) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)m) voxel_finish_one(v, xyz, first, count, g, S, N, C, out_xyz, out_normals, out_rgb);
}
#pragma clang diagnostic pop

}  // namespace pm
