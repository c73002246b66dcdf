// pm_surface.hpp -- a mesh measured as a surface (mpmvs_surface_*; contract: include/mpmvs.h, statements 5 and 6 of the mesh section;
// DESIGN.md section 26).
//
// DISTANCE: per point of a cloud the lexicographic minimum of (D, triangle index) over the triangles within the radius, D the squared
// distance to the closest point of the triangle (Ericson's region cascade in fp64, one conversion to fp32).  Triangle-major scatter
// onto the cloud's own grid (pm_cloud.hpp), no second search structure:
//   1. k_surface_init     every point's key = (bits(+inf) << 32) | 0xffffffff.
//   2. k_surface_scatter  one thread per triangle: the cells of its bounding box, widened by one cell on every side and clipped to the
//                         grid; a triangle with more than `large` cells goes to a list instead.  Per cell: looked up, rejected where
//                         the triangle's plane is too far from the cell's centre, else one evaluation per point of the cell and one
//                         64-bit atomic minimum of (bits(D) << 32) | t where that improves the key just read.
//      k_surface_large    the listed triangles, one block each (grid-stride over the list): the cells dealt to the 256 threads.
//   3. k_surface_finish   keys -> out_d2, out_tri and the number of points with a candidate.
// All that threads share are integer minima and one list whose order never reaches a result.
//
// SAMPLE: the centroids of the regular s-subdivision of every triangle, s = ceil(longest edge / spacing).
//   1. k_surface_count    per triangle s * s (0 for a non-finite one), the total, and the first triangle beyond the limit of 4096.
//   2. scan_offsets       (pm_scan.hpp) counts -> offsets.
//   3. k_surface_emit     one thread per sample: its triangle by a binary search of the offsets, so that one huge triangle among many
//                         tiny ones is spread over as many threads as it has samples.
// The per-thread bodies are host and device, so that tools/mesh_distance_check.cpp can replay the passes thread by thread.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"

namespace pm {

constexpr double kSurfaceMaxRatio = 4096.0;         // longest edge / spacing of a sampled triangle
constexpr long long kSurfaceMaxSamples = 1ll << 30;
constexpr int kSurfaceLargeDefault = 125;           // cells of a triangle's range above which a block walks them: measured, DESIGN.md 26.4
constexpr unsigned long long kSurfaceNone = 0x7f800000ffffffffull;   // (bits(+inf) << 32) | 0xffffffff

// the cloud's grid as the scatter sees it
struct SurfaceGrid {
    CloudGrid g;
    int hi[3];         // the last cell of the grid per axis: the cell of the bounding box's maximum
    double reach;      // (radius + half a cell's diagonal) * (1 + 2^-8): how far from a cell's centre a candidate's triangle can be
    double gmax;       // the largest magnitude of a coordinate inside the grid
    int large;         // a triangle with more cells than this is dealt to a block
};

// the shared minimum and counters; the host replay runs one thread at a time
__host__ __device__ inline void surface_min(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
__host__ __device__ inline unsigned long long surface_add(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const unsigned long long old = *p;
    *p = old + v;
    return old;
#endif
}
__host__ __device__ inline void surface_min32(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// the corners of triangle t as doubles, A then B then C; false if a coordinate is not finite (the triangle takes no part)
__host__ __device__ inline bool surface_corners(const float* __restrict__ xyz, const int32_t* __restrict__ tri, size_t t, double P[9]) {
    bool fin = true;
    for (int c = 0; c < 3; ++c) {
        const size_t v = (size_t)tri[3 * t + c];
        for (int a = 0; a < 3; ++a) {
            const float x = xyz[3 * v + a];
            fin = fin && cloud_finite(x);
            P[3 * c + a] = (double)x;
        }
    }
    return fin;
}

__host__ __device__ inline double surface_dot(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// THE STATEMENT: D of the point q against the triangle P, rule by rule as include/mpmvs.h writes them.  A comparison with a NaN is false.
__host__ __device__ inline float surface_d2(const double P[9], const double q[3]) {
    const double *A = P, *B = P + 3, *Cc = P + 6;
    double ab[3], ac[3], ap[3], bp[3], cp[3], X[3];
    for (int k = 0; k < 3; ++k) {
        ab[k] = B[k] - A[k];
        ac[k] = Cc[k] - A[k];
        ap[k] = q[k] - A[k];
        bp[k] = q[k] - B[k];
        cp[k] = q[k] - Cc[k];
    }
    const double s1 = surface_dot(ab, ap), s2 = surface_dot(ac, ap), s3 = surface_dot(ab, bp), s4 = surface_dot(ac, bp), s5 = surface_dot(ab, cp),
                 s6 = surface_dot(ac, cp);
    const double vc = s1 * s4 - s3 * s2, vb = s5 * s2 - s1 * s6, va = s3 * s6 - s5 * s4;
    if (s1 <= 0.0 && s2 <= 0.0) {
        for (int k = 0; k < 3; ++k) X[k] = A[k];
    } else if (s3 >= 0.0 && s4 <= s3) {
        for (int k = 0; k < 3; ++k) X[k] = B[k];
    } else if (vc <= 0.0 && s1 >= 0.0 && s3 <= 0.0) {
        const double v = s1 / (s1 - s3);
        for (int k = 0; k < 3; ++k) X[k] = A[k] + v * ab[k];
    } else if (s6 >= 0.0 && s5 <= s6) {
        for (int k = 0; k < 3; ++k) X[k] = Cc[k];
    } else if (vb <= 0.0 && s2 >= 0.0 && s6 <= 0.0) {
        const double w = s2 / (s2 - s6);
        for (int k = 0; k < 3; ++k) X[k] = A[k] + w * ac[k];
    } else if (va <= 0.0 && (s4 - s3) >= 0.0 && (s5 - s6) >= 0.0) {
        const double w = (s4 - s3) / ((s4 - s3) + (s5 - s6));
        for (int k = 0; k < 3; ++k) X[k] = B[k] + w * (Cc[k] - B[k]);
    } else {
        const double den = (va + vb) + vc, v = vb / den, w = vc / den;
        for (int k = 0; k < 3; ++k) X[k] = (A[k] + v * ab[k]) + w * ac[k];
    }
    const double e[3] = {q[0] - X[0], q[1] - X[1], q[2] - X[2]};
    return (float)((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

__host__ __device__ inline double surface_abs(double x) { return x < 0.0 ? -x : x; }

// A participating triangle against the grid: the cell range of its box and what the cell rejection needs.
// WHY THE RANGE IS EXHAUSTIVE.  A candidate point p has D <= r2, so along every axis |p_a - X_a| <= radius * (1 + 4 * 2^-24), as for a
// point target (pm_cloud.hpp, cloud_walk).  The closest point X is a convex combination of the corners, computed in fp64: it lies in
// the corners' box [lo_a, hi_a] but for the rounding of at most a handful of operations on numbers no larger than twice the largest
// corner magnitude M_a of that axis.  The box is therefore widened by pad_a = 2^-48 * M_a before its cells are taken (16 units in
// the last place of 2 * M_a; an axis along which the triangle is flat has X_a exact and needs none, and gets it anyway).  Then p_a lies
// within radius * (1 + 2.4e-7) of [lo_a - pad_a, hi_a + pad_a], the cell coordinate is monotone in x, and edge = max(radius, 2^-60) *
// (1 + 2^-10): the coordinate of p exceeds that of the widened box's end by less than 1 before the floor, hence the cell of p lies in
// [cell(lo_a - pad_a) - 1, cell(hi_a + pad_a) + 1].  The range is clipped to [0, S.hi[a]], where every cell of the grid lies.
struct SurfaceTri {
    double P[9];
    double n[3], nlen;     // the plane's normal, not normalised, and its length; nlen = 0 switches the rejection off
    double slack;          // what the rounding of the plane distance can hide: 2^-40 * the largest magnitude involved
    int lo[3], ext[3];     // first cell and number of cells per axis; an empty range has ext[0] = 0
    unsigned long long cells;   // at most 2^63: three axes of 2^21 cells
};
__host__ __device__ inline void surface_range(SurfaceTri& T, const SurfaceGrid& S) {
    const double* P = T.P;
    double big = S.gmax;
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        double lo = P[a], hi = P[a], m = surface_abs(P[a]);
        for (int c = 1; c < 3; ++c) {
            const double x = P[3 * c + a];
            lo = x < lo ? x : lo;
            hi = x > hi ? x : hi;
            m = surface_abs(x) > m ? surface_abs(x) : m;
        }
        big = m > big ? m : big;
        const double pad = m * 0x1p-48;
        // cloud_cell clamps to [-2, cells + 1] and takes a float; the same floor on the padded doubles here
        double t0 = floor(((lo - pad) - S.g.mn[a]) / S.g.edge) - 1.0, t1 = floor(((hi + pad) - S.g.mn[a]) / S.g.edge) + 1.0;
        t0 = t0 < 0.0 ? 0.0 : t0;
        t1 = t1 > (double)S.hi[a] ? (double)S.hi[a] : t1;
        if (!(t0 <= t1)) empty = true;   // also a NaN, which finite corners cannot give
        T.lo[a] = empty ? 0 : (int)t0;
        T.ext[a] = empty ? 0 : (int)t1 - (int)t0 + 1;
    }
    if (empty) T.ext[0] = T.ext[1] = T.ext[2] = 0;
    T.cells = (unsigned long long)T.ext[0] * (unsigned long long)T.ext[1] * (unsigned long long)T.ext[2];
    const double u[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, w[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    T.n[0] = u[1] * w[2] - u[2] * w[1];
    T.n[1] = u[2] * w[0] - u[0] * w[2];
    T.n[2] = u[0] * w[1] - u[1] * w[0];
    const double l = sqrt(surface_dot(T.n, T.n));
    T.nlen = (l >= 1e-100 && l <= 1e100) ? l : 0.0;   // outside: squares underflow or overflow, the plane is not to be trusted
    T.slack = big * 0x1p-40;
}

// One cell of triangle t's range: the lookup, the rejection, the points.  The rejection only skips work: every point of the cell lies
// within half the cell's diagonal of its centre c, so a candidate's triangle has a point within radius * (1 + 2.4e-7) + half the
// diagonal of c, and its plane is no farther; S.reach carries 2^-8 of margin over that and T.slack the rounding of the distance.
__host__ __device__ inline void surface_cell(const SurfaceTri& T, uint32_t t, int cx, int cy, int cz, const SurfaceGrid& S, unsigned long long* __restrict__ keys) {
    const int s = cloud_lookup(cloud_key(cx, cy, cz), S.g);
    if (s < 0) return;
    if (T.nlen > 0.0) {
        const double c[3] = {(S.g.mn[0] + ((double)cx + 0.5) * S.g.edge) - T.P[0], (S.g.mn[1] + ((double)cy + 0.5) * S.g.edge) - T.P[1],
                             (S.g.mn[2] + ((double)cz + 0.5) * S.g.edge) - T.P[2]};
        if (surface_abs(surface_dot(T.n, c)) > (S.reach + T.slack) * T.nlen) return;
    }
    const int e = S.g.off[s + 1];
    for (int p = S.g.off[s]; p < e; ++p) {
        const uint4 rec = S.g.pts[p];
        const double q[3] = {(double)cloud_float(rec.x), (double)cloud_float(rec.y), (double)cloud_float(rec.z)};
        const float D = surface_d2(T.P, q);
        if (!(D <= S.g.r2)) continue;
        const unsigned long long cand = ((unsigned long long)cloud_bits(D) << 32) | t;
        // a key only ever falls: what is read here is no smaller than the key is by now, so skipping on it loses nothing
        if (cand < keys[rec.w]) surface_min(&keys[rec.w], cand);
    }
}

__host__ __device__ inline void surface_init_one(size_t i, unsigned long long* __restrict__ keys) { keys[i] = kSurfaceNone; }

// thread t of the scatter: the triangle's cells, or its place in the list of the large ones
__host__ __device__ inline void surface_scatter_one(size_t t, const float* __restrict__ xyz, const int32_t* __restrict__ tri, const SurfaceGrid& S,
                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ list, unsigned long long* __restrict__ n_list) {
    SurfaceTri T;
    if (!surface_corners(xyz, tri, t, T.P)) return;
    surface_range(T, S);
    if (T.cells == 0) return;
    if (T.cells > (unsigned long long)S.large) {
        list[surface_add(n_list, 1ull)] = (int32_t)t;
        return;
    }
    for (int z = 0; z < T.ext[2]; ++z)
        for (int y = 0; y < T.ext[1]; ++y)
            for (int x = 0; x < T.ext[0]; ++x) surface_cell(T, (uint32_t)t, T.lo[0] + x, T.lo[1] + y, T.lo[2] + z, S, keys);
}

// lane `lane` of the `lanes` that share the listed triangle k: every lanes-th cell of its range
__host__ __device__ inline void surface_large_lane(size_t k, int lane, int lanes, const float* __restrict__ xyz, const int32_t* __restrict__ tri, const SurfaceGrid& S,
                                                   unsigned long long* __restrict__ keys, const int32_t* __restrict__ list) {
    const size_t t = (size_t)list[k];
    SurfaceTri T;
    if (!surface_corners(xyz, tri, t, T.P)) return;
    surface_range(T, S);
    const unsigned long long row = (unsigned long long)T.ext[0], layer = row * (unsigned long long)T.ext[1];
    for (unsigned long long c = (unsigned long long)lane; c < T.cells; c += (unsigned long long)lanes) {
        const int z = (int)(c / layer), y = (int)((c - (unsigned long long)z * layer) / row), x = (int)(c - (unsigned long long)z * layer - (unsigned long long)y * row);
        surface_cell(T, (uint32_t)t, T.lo[0] + x, T.lo[1] + y, T.lo[2] + z, S, keys);
    }
}

// thread i of the finish: true if the point has a candidate
__host__ __device__ inline bool surface_finish_one(size_t i, const unsigned long long* __restrict__ keys, float* __restrict__ out_d2, int32_t* __restrict__ out_tri) {
    const unsigned long long k = keys[i];
    out_d2[i] = cloud_float((uint32_t)(k >> 32));
    if (out_tri) out_tri[i] = (int32_t)(uint32_t)(k & 0xffffffffull);   // 0xffffffff: -1
    return k != kSurfaceNone;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------------
// s of a participating triangle, or 0 where !(ratio <= 4096)
__host__ __device__ inline long long surface_subdiv(const double P[9], double h_s) {
    double l2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double* U = P + 3 * c;
        const double* V = P + 3 * ((c + 1) % 3);
        const double dx = V[0] - U[0], dy = V[1] - U[1], dz = V[2] - U[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        l2 = d > l2 ? d : l2;
    }
    const double ratio = sqrt(l2) / h_s;
    if (!(ratio <= kSurfaceMaxRatio)) return 0;
    const long long s = (long long)ceil(ratio);
    return s < 1 ? 1 : s;
}

// thread t of the count: cnt[t] = s * s, which it returns; a triangle beyond the limit lowers *first_bad to its index and counts 0
__host__ __device__ inline int surface_count_one(size_t t, const float* __restrict__ xyz, const int32_t* __restrict__ tri, double h_s, int* __restrict__ cnt,
                                                 uint32_t* __restrict__ first_bad) {
    double P[9];
    int c = 0;
    if (surface_corners(xyz, tri, t, P)) {
        const long long s = surface_subdiv(P, h_s);
        if (s == 0) surface_min32(first_bad, (uint32_t)t);
        c = (int)(s * s);   // at most 2^24
    }
    cnt[t] = c;
    return c;
}

// the triangle of sample j: the last t with off[t] <= j (off: the exclusive scan of the counts; j < the total, so that t has samples)
__host__ __device__ inline int surface_owner(const int* __restrict__ off, int m, int j) {
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// thread j of the emit
__host__ __device__ inline void surface_emit_one(size_t j, const float* __restrict__ xyz, const unsigned char* __restrict__ rgb, const int32_t* __restrict__ tri, int m,
                                                 double h_s, const int* __restrict__ off, float* __restrict__ out_xyz, int32_t* __restrict__ out_tri_of,
                                                 unsigned char* __restrict__ out_rgb, float* __restrict__ out_normals) {
    const int t = surface_owner(off, m, (int)j);
    double P[9];
    (void)surface_corners(xyz, tri, (size_t)t, P);
    const long long s = surface_subdiv(P, h_s), k = (long long)j - off[t];
    const long long u = s * s - 1 - k;
    long long g = (long long)sqrt((double)u);
    while (g * g > u) --g;
    while ((g + 1) * (g + 1) <= u) ++g;
    const long long i = s - 1 - g, l = k - (2 * s * i - i * i), jj = l >> 1;
    const long long na = (l & 1) ? 3 * i + 2 : 3 * i + 1, nb = (l & 1) ? 3 * jj + 2 : 3 * jj + 1, nc = 3 * s - na - nb;
    const double den = (double)(3 * s);
    for (int a = 0; a < 3; ++a) out_xyz[3 * j + a] = (float)((((double)na * P[a] + (double)nb * P[3 + a]) + (double)nc * P[6 + a]) / den);
    out_tri_of[j] = t;
    if (out_rgb) {
        const unsigned char *ca = rgb + 3 * (size_t)tri[3 * t], *cb = rgb + 3 * (size_t)tri[3 * t + 1], *cc = rgb + 3 * (size_t)tri[3 * t + 2];
        for (int a = 0; a < 3; ++a) out_rgb[3 * j + a] = (unsigned char)((2 * (na * ca[a] + nb * cb[a] + nc * cc[a]) + 3 * s) / (2 * 3 * s));
    }
    if (out_normals) {
        const double uu[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, w[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
        const double C[3] = {uu[1] * w[2] - uu[2] * w[1], uu[2] * w[0] - uu[0] * w[2], uu[0] * w[1] - uu[1] * w[0]};
        const double L = sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2]);
        const bool ok = L > 0.0 && L <= 1.7976931348623157e308;
        for (int a = 0; a < 3; ++a) out_normals[3 * j + a] = ok ? (float)(C[a] / L) : 0.0f;
    }
}

// ---- kernels: `inline`, as pm_cloud.hpp says of its own ------------------------------------------------------------------------------
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(256) void k_surface_init(int n, unsigned long long* __restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) surface_init_one(i, keys);
}

inline __global__ __launch_bounds__(256) void k_surface_scatter(int m, const float* __restrict__ xyz, const int32_t* __restrict__ tri, SurfaceGrid S,
                                                         unsigned long long* __restrict__ keys, int32_t* __restrict__ list, unsigned long long* __restrict__ n_list) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)m) surface_scatter_one(t, xyz, tri, S, keys, list, n_list);
}

// a block per listed triangle, the blocks striding over the list: its length is read here, so that the host need not wait for it
inline __global__ __launch_bounds__(256) void k_surface_large(const float* __restrict__ xyz, const int32_t* __restrict__ tri, SurfaceGrid S,
                                                       unsigned long long* __restrict__ keys, const int32_t* __restrict__ list,
                                                       const unsigned long long* __restrict__ n_list) {
    const size_t n = (size_t)*n_list;
    for (size_t k = blockIdx.x; k < n; k += gridDim.x) surface_large_lane(k, (int)threadIdx.x, 256, xyz, tri, S, keys, list);
}

inline __global__ __launch_bounds__(256) void k_surface_finish(int n, const unsigned long long* __restrict__ keys, float* __restrict__ out_d2, int32_t* __restrict__ out_tri,
                                                        unsigned long long* __restrict__ n_found) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int found = (i < (size_t)n && surface_finish_one(i, keys, out_d2, out_tri)) ? 1 : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) found += __shfl_xor(found, d, 64);
    if ((threadIdx.x & 63) == 0 && found > 0) atomicAdd(n_found, (unsigned long long)found);
}

inline __global__ __launch_bounds__(256) void k_surface_count(int m, const float* __restrict__ xyz, const int32_t* __restrict__ tri, double h_s, int* __restrict__ cnt,
                                                       unsigned long long* __restrict__ total, uint32_t* __restrict__ first_bad) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    long long c = t < (size_t)m ? surface_count_one(t, xyz, tri, h_s, cnt, first_bad) : 0;   // a wave's sum: at most 2^30
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(total, (unsigned long long)c);
}

inline __global__ __launch_bounds__(256) void k_surface_emit(int n_samples, const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                      const int32_t* __restrict__ tri, int m, double h_s, const int* __restrict__ off, float* __restrict__ out_xyz,
                                                      int32_t* __restrict__ out_tri_of, unsigned char* __restrict__ out_rgb, float* __restrict__ out_normals) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)n_samples) surface_emit_one(j, xyz, rgb, tri, m, h_s, off, out_xyz, out_tri_of, out_rgb, out_normals);
}
#pragma clang diagnostic pop

}  // namespace pm
