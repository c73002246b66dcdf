// pm_mesh.hpp -- an indexed triangle mesh on the device (mpmvs_mesh_*; contract: include/mpmvs.h and DESIGN.md section 24): its
// connected components, its area-weighted vertex normals and the compaction under a vertex mask.  n vertices (xyz fp32, optional
// rgb bytes), m triangles of three int32 indices in [0, n), checked by mpmvs_mesh_create.  Every output is a pure function of the
// arrays, bit for bit, independent of scheduling.
//
// COMPONENTS.  Two vertices are joined iff some triangle names both; connectivity is by index, never by position.  The union-find
// of pm_unionfind.hpp in one pass over the triangles:
//   k_mesh_cc_init    parent[v] = v: every vertex takes part.
//   k_mesh_cc_hook    one thread per triangle (a, b, c): root = cc_find(a), then the roots of b and c are linked to it.  Every value
//                     stored into parent[x] is a vertex index below x, as in the cloud's hook pass: the invariant parent[x] <= x and
//                     the argument of DESIGN.md section 20 do not ask where an edge comes from.
//   k_cc_flatten, k_cc_count, k_cc_gather   as they are: label[v], the vertex count of v's component.
//   k_mesh_tri_count  cnt[label[tri[3t]]] += 1 with the wave-merged add of k_cc_count: a triangle belongs to the component of its
//                     first index.
//
// NORMALS, all in fp64 with no contraction, only + - * / sqrt, comparisons and one llrint, each correctly rounded (the discipline of
// pm_normals.hpp).  The host passes `scale`, a power of two (mesh_scale below).
//   k_mesh_nrm_accum  one thread per triangle whose three vertices are finite: u = P_b - P_a, w = P_c - P_a from the floats converted
//                     to double, C = u x w, F_k = llrint(C_k * scale) (to nearest even), then S[a] += F, S[b] += F, S[c] += F: nine
//                     64-bit integer atomic adds.  Integer addition commutes, so the order of the triangles never shows.
//   k_mesh_nrm_finish one thread per vertex: x, y, z = (double)S_k, len = sqrt((x*x + y*y) + z*z); len == 0 gives (0, 0, 0), else
//                     ((float)(x/len), (float)(y/len), (float)(z/len)); the vertices with len > 0 are counted (wave-merged).
//   WHY NO SUM OVERFLOWS.  ext = the largest per-axis (double)max - (double)min over the finite vertices.  An edge component is the
//   rounded difference of two coordinates whose exact difference is at most the exact max - min; rounding is monotone, so it is at most
//   ext.  A product of two is at most fl(ext*ext), a difference of two products at most 2*fl(ext*ext) = B (doubling is exact, and B
//   is a double, so rounding cannot lift the difference above it).  With 2^(e-1) <= B < 2^e (frexp) and b the least integer with
//   max(m, 1) <= 2^b, scale = 2^(61-b-e): |C_k * scale| < 2^(61-b) exactly (a power of two scales without rounding), and so is its
//   llrint.  A triangle that names a vertex twice has C = 0 exactly (u = 0, w = 0 or u = w), so although it adds to that vertex twice,
//   a vertex receives at most m non-zero terms: |S_k| < 2^b * 2^(61-b) = 2^61 < 2^62.  The coordinates are floats: ext <= 2^129, B <=
//   2^259, no product overflows or underflows to a denormal that matters (the smallest non-zero product is 2^-298), and 61-b-e stays
//   far inside ldexp's range.
//
// SELECT.  keep[v] != 0 keeps a vertex; a triangle is kept iff its three vertices are; with drop_unreferenced a vertex also needs a
// kept triangle that names it.
//   k_mesh_sel_verts  vflag[v] = drop_unreferenced ? 0 : keep[v] != 0
//   k_mesh_sel_tris   tflag[t]; with drop_unreferenced a kept triangle stores 1 into the flags of its three vertices: plain stores of
//                     identical values
//   k_scan_tiles, k_scan_totals<Sum> (pm_scan.hpp) over both flag arrays; the tile offsets are added where they are used
//   k_mesh_emit_verts, k_mesh_emit_tris   kept vertices and triangles in their order, the triangles with the new numbers
// The per-thread bodies are host and device code, so that tools/mesh_clean_check.cpp can replay them thread by thread under the
// host sanitizers; there the atomics are plain reads and writes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pm_scan.hpp"
#include "pm_unionfind.hpp"

namespace pm {

__host__ __device__ inline bool mesh_finite(float v) { return __builtin_isfinite(v); }
__host__ __device__ inline bool mesh_finite3(const float* __restrict__ xyz, size_t v) {
    return mesh_finite(xyz[3 * v]) && mesh_finite(xyz[3 * v + 1]) && mesh_finite(xyz[3 * v + 2]);
}
__host__ __device__ inline void mesh_add64(long long* p, long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long*)p, (unsigned long long)v);   // two's complement: the unsigned add is the signed one
#else
    *p += v;
#endif
}

// host only: 0 if every normal is (0, 0, 0) (no finite vertex, ext == 0 or m == 0), else the power of two of the statement
inline double mesh_scale(const float* xyz, long long n, long long m, int* e_out = nullptr, int* b_out = nullptr) {
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    bool any = false;
    for (long long v = 0; v < n; ++v) {
        if (!mesh_finite3(xyz, (size_t)v)) continue;
        for (int a = 0; a < 3; ++a) {
            const double x = (double)xyz[3 * v + a];
            mn[a] = any ? (x < mn[a] ? x : mn[a]) : x;
            mx[a] = any ? (x > mx[a] ? x : mx[a]) : x;
        }
        any = true;
    }
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = mx[a] - mn[a] > ext ? mx[a] - mn[a] : ext;
    if (!any || ext == 0.0 || m == 0) return 0.0;
    const double B = 2.0 * (ext * ext);
    int e = 0, b = 0;
    (void)std::frexp(B, &e);
    while ((1ll << b) < m) ++b;
    if (e_out) *e_out = e;
    if (b_out) *b_out = b;
    return std::ldexp(1.0, 61 - b - e);
}

// ---- components ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void mesh_cc_hook_one(size_t t, const int32_t* __restrict__ tri, int* __restrict__ parent) {
    int root = cc_find(parent, tri[3 * t]);
    for (int k = 1; k < 3; ++k) {
        const int other = cc_find(parent, tri[3 * t + k]);
        if (other != root) root = cc_link(parent, root, other);
    }
}
__global__ __launch_bounds__(256) void k_mesh_cc_init(int n, int* __restrict__ parent) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)n) parent[v] = (int)v;
}
__global__ __launch_bounds__(256) void k_mesh_cc_hook(int m, const int32_t* __restrict__ tri, int* __restrict__ parent) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) mesh_cc_hook_one(t, tri, parent);
}
__host__ __device__ inline void mesh_tri_count_one(size_t t, const int32_t* __restrict__ tri, const int32_t* __restrict__ label, int* __restrict__ cnt) {
    cc_count_label(label[tri[3 * t]], cnt);
}
__global__ __launch_bounds__(256) void k_mesh_tri_count(int m, const int32_t* __restrict__ tri, const int32_t* __restrict__ label, int* __restrict__ cnt) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    cc_count_wave(t < (size_t)m ? label[tri[3 * t]] : -1, cnt);
}

// ---- normals ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void mesh_nrm_accum_one(size_t t, const float* __restrict__ xyz, const int32_t* __restrict__ tri, double scale, long long* __restrict__ S) {
    const size_t a = (size_t)tri[3 * t], b = (size_t)tri[3 * t + 1], c = (size_t)tri[3 * t + 2];
    if (!(mesh_finite3(xyz, a) && mesh_finite3(xyz, b) && mesh_finite3(xyz, c))) return;
    const double ax = (double)xyz[3 * a], ay = (double)xyz[3 * a + 1], az = (double)xyz[3 * a + 2];
    const double ux = (double)xyz[3 * b] - ax, uy = (double)xyz[3 * b + 1] - ay, uz = (double)xyz[3 * b + 2] - az;
    const double wx = (double)xyz[3 * c] - ax, wy = (double)xyz[3 * c + 1] - ay, wz = (double)xyz[3 * c + 2] - az;
    const double C[3] = {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
    for (int k = 0; k < 3; ++k) {
        const long long F = llrint(C[k] * scale);
        if (F == 0) continue;   // adding 0 changes nothing
        mesh_add64(&S[3 * a + k], F);
        mesh_add64(&S[3 * b + k], F);
        mesh_add64(&S[3 * c + k], F);
    }
}
__global__ __launch_bounds__(256) void k_mesh_nrm_accum(int m, const float* __restrict__ xyz, const int32_t* __restrict__ tri, double scale, long long* __restrict__ S) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) mesh_nrm_accum_one(t, xyz, tri, scale, S);
}
// true iff the normal is defined
__host__ __device__ inline bool mesh_nrm_finish_one(size_t v, const long long* __restrict__ S, float* __restrict__ out) {
    const double x = (double)S[3 * v], y = (double)S[3 * v + 1], z = (double)S[3 * v + 2];
    const double len = sqrt((x * x + y * y) + z * z);
    const bool defined = len > 0.0;
    out[3 * v] = defined ? (float)(x / len) : 0.0f;
    out[3 * v + 1] = defined ? (float)(y / len) : 0.0f;
    out[3 * v + 2] = defined ? (float)(z / len) : 0.0f;
    return defined;
}
// n_defined[0] += the defined normals, one add per wave
__global__ __launch_bounds__(256) void k_mesh_nrm_finish(int n, const long long* __restrict__ S, float* __restrict__ out, int* __restrict__ n_defined) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool defined = v < (size_t)n && mesh_nrm_finish_one(v, S, out);
    cc_count_wave(defined ? 0 : -1, n_defined);
}

// ---- select ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void mesh_sel_vert_one(size_t v, const unsigned char* __restrict__ keep, int drop_unreferenced, int* __restrict__ vflag) {
    vflag[v] = !drop_unreferenced && keep[v] != 0;
}
__global__ __launch_bounds__(256) void k_mesh_sel_verts(int n, const unsigned char* __restrict__ keep, int drop_unreferenced, int* __restrict__ vflag) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)n) mesh_sel_vert_one(v, keep, drop_unreferenced, vflag);
}
__host__ __device__ inline void mesh_sel_tri_one(size_t t, const int32_t* __restrict__ tri, const unsigned char* __restrict__ keep, int drop_unreferenced,
                                                 int* __restrict__ tflag, int* __restrict__ vflag) {
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const bool kept = keep[a] != 0 && keep[b] != 0 && keep[c] != 0;
    tflag[t] = kept;
    if (kept && drop_unreferenced) vflag[a] = vflag[b] = vflag[c] = 1;
}
__global__ __launch_bounds__(256) void k_mesh_sel_tris(int m, const int32_t* __restrict__ tri, const unsigned char* __restrict__ keep, int drop_unreferenced,
                                                       int* __restrict__ tflag, int* __restrict__ vflag) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) mesh_sel_tri_one(t, tri, keep, drop_unreferenced, tflag, vflag);
}
// the new number of a kept element k: its place in its tile plus the tile's offset
__host__ __device__ inline int mesh_new_index(size_t k, const int* __restrict__ excl, const int* __restrict__ tile) { return excl[k] + tile[k / kScanBlock]; }
__host__ __device__ inline void mesh_emit_vert_one(size_t v, const float* __restrict__ xyz, const unsigned char* __restrict__ rgb, const int* __restrict__ vflag,
                                                   const int* __restrict__ vexcl, const int* __restrict__ vtile, float* __restrict__ out_xyz,
                                                   unsigned char* __restrict__ out_rgb, int32_t* __restrict__ out_src) {
    if (!vflag[v]) return;
    const size_t j = (size_t)mesh_new_index(v, vexcl, vtile);
    for (int k = 0; k < 3; ++k) out_xyz[3 * j + k] = xyz[3 * v + k];
    if (rgb)
        for (int k = 0; k < 3; ++k) out_rgb[3 * j + k] = rgb[3 * v + k];
    out_src[j] = (int32_t)v;
}
__global__ __launch_bounds__(256) void k_mesh_emit_verts(int n, const float* __restrict__ xyz, const unsigned char* __restrict__ rgb, const int* __restrict__ vflag,
                                                         const int* __restrict__ vexcl, const int* __restrict__ vtile, float* __restrict__ out_xyz,
                                                         unsigned char* __restrict__ out_rgb, int32_t* __restrict__ out_src) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < (size_t)n) mesh_emit_vert_one(v, xyz, rgb, vflag, vexcl, vtile, out_xyz, out_rgb, out_src);
}
__host__ __device__ inline void mesh_emit_tri_one(size_t t, const int32_t* __restrict__ tri, const int* __restrict__ tflag, const int* __restrict__ texcl,
                                                  const int* __restrict__ ttile, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                  int32_t* __restrict__ out_tri) {
    if (!tflag[t]) return;
    const size_t j = (size_t)mesh_new_index(t, texcl, ttile);
    for (int k = 0; k < 3; ++k) out_tri[3 * j + k] = mesh_new_index((size_t)tri[3 * t + k], vexcl, vtile);   // a kept triangle's vertices are kept
}
__global__ __launch_bounds__(256) void k_mesh_emit_tris(int m, const int32_t* __restrict__ tri, const int* __restrict__ tflag, const int* __restrict__ texcl,
                                                        const int* __restrict__ ttile, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                        int32_t* __restrict__ out_tri) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) mesh_emit_tri_one(t, tri, tflag, texcl, ttile, vexcl, vtile, out_tri);
}

}  // namespace pm
