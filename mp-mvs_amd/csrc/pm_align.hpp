// pm_align.hpp -- one pass of point-to-point ICP on the device (mpmvs_align_*; contract: DESIGN.md section 15 and include/mpmvs.h):
// the moving cloud stays in HBM, is transformed by M (12 doubles, row-major 3 x 4) on the device, every transformed point takes
// its exact capped nearest neighbour in the target's grid (cloud_search of pm_cloud.hpp, the search of mpmvs_cloud_nearest), and
// the matched pairs are reduced to the 18 integers a similarity transform needs.  Bit for bit the plain-loop statement:
//   y_k = (float)(((A[k][0]*sx + A[k][1]*sy) + A[k][2]*sz) + t[k])   in fp64, no contraction; a source with a non-finite
//   coordinate is skipped, and so is one whose y has no candidate within the radius;
//   a = ((double)y - o) * iu,  b = ((double)p_j - o) * iu   with (o, u) the frame of the target's bounding box and iu = 1 / u;
//   fix(x) = llrint(x * 2^30), round to nearest even;
//   sums[0] += 1; sums[1..3] += fix(a_k); sums[4..6] += fix(b_k); sums[7 + 3 i + j] += fix(a_i * b_j);
//   sums[16] += fix((a_x*a_x + a_y*a_y) + a_z*a_z); sums[17] += fix((double)d2 * (iu * iu)).
// THE FRAME: o = the centre of the finite bounding box, h = half its largest extent + 2 radius, u = the smallest power of two
// >= h.  A matched y lies within radius * (1 + 4 * 2^-24) of a target along every axis, a target lies within half the extent
// of o, so |y - o| < h <= u along every axis: every component of a and of b is at most 1 in magnitude.
// OVERFLOW: hence |a_k|, |b_k|, |a_i * b_j| <= 1, the squared norm <= 3 and d2 / u^2 <= 3; every |fix(term)| <= 3 * 2^30.
// At most 2^31 - 1 sources contribute, so every |sum| < 3 * 2^30 * 2^31 = 3 * 2^61 < 2^63: an int64 cannot overflow.
// GRANULARITY: the grain is 2^-30 u.  An fp32 coordinate of magnitude up to u has a grain of 2^-24 u at worst, 64 times coarser.
// ORDER: integer addition is associative and commutative: the order of the lanes, waves, blocks and atomics never shows.
//
// Passes of a call (mpmvs_cloud.hip: align_pass):
//   1. k_align_qbin / scan / k_cloud_qorder   the sources binned by the cell of their TRANSFORMED point (MPMVS_CLOUD_BIN=0: caller order)
//   2. k_align_pass   one thread per source: transform, search, the pair in the normalised frame; then term by term: the wave
//                     adds it with __shfl_xor (a 64-bit value crosses lanes as two dwords and is put together again BEFORE the
//                     64-bit add, so carry and sign are the add's own; ds_bpermute, no LDS traffic) and parks it in LDS, where
//                     the four waves meet; threads 0..17 add the block's totals to the device buffer with one 64-bit integer
//                     atomic each.
#pragma once

#include "pm_cloud.hpp"

namespace pm {

constexpr int kAlignTerms = 18;

struct AlignXf {
    double m[12];   // row-major 3 x 4
    double o[3];
    double iu;      // 1 / u, a power of two
};

// frame[0..2] = o, frame[3] = u from the finite bounding box and the radius (host: the frame is computed once per call)
inline void align_frame(const float mn[3], const float mx[3], float radius, double frame[4]) {
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        frame[a] = 0.5 * ((double)mn[a] + (double)mx[a]);
        const double e = (double)mx[a] - (double)mn[a];
        ext = e > ext ? e : ext;
    }
    const double h = 0.5 * ext + 2.0 * (double)radius;
    int e = 0;
    const double m = frexp(h, &e);   // h = m * 2^e, m in [0.5, 1)
    frame[3] = m == 0.5 ? h : ldexp(1.0, e);
}

__host__ __device__ inline long long align_fix(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(x * 0x1p30);
#else
    return llrint(x * 0x1p30);   // the default rounding mode: to nearest even
#endif
}

__host__ __device__ inline float align_xform(const AlignXf& f, int k, float sx, float sy, float sz) {
    return (float)(((f.m[4 * k] * (double)sx + f.m[4 * k + 1] * (double)sy) + f.m[4 * k + 2] * (double)sz) + f.m[4 * k + 3]);
}

// the transformed point of source i and its cell; false if the source or its image is not finite
__host__ __device__ inline bool align_point(size_t i, const float* __restrict__ src, const AlignXf& f, const CloudGrid& g, float& x, float& y, float& z,
                                            int& cx, int& cy, int& cz) {
    const float sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
    if (!(cloud_finite(sx) && cloud_finite(sy) && cloud_finite(sz))) return false;
    x = align_xform(f, 0, sx, sy, sz), y = align_xform(f, 1, sx, sy, sz), z = align_xform(f, 2, sx, sy, sz);
    return cloud_point_cell(x, y, z, g, cx, cy, cz);
}

__host__ __device__ inline void align_qbin_one(size_t i, const float* __restrict__ src, const AlignXf& f, const CloudGrid& g, unsigned bin_mask,
                                               int* __restrict__ qcnt, int* __restrict__ qbin) {
    float x, y, z;
    int cx, cy, cz, b = 0;
    if (align_point(i, src, f, g, x, y, z, cx, cy, cz)) b = cloud_cell_bin(cx, cy, cz, bin_mask);
    qbin[i] = b;
    cloud_fetch_add(&qcnt[b], 1);
}

__global__ __launch_bounds__(256) void k_align_qbin(const float* __restrict__ src, int n, AlignXf f, CloudGrid g, unsigned bin_mask, int* __restrict__ qcnt,
                                                    int* __restrict__ qbin) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) align_qbin_one(i, src, f, g, bin_mask, qcnt, qbin);
}

// the matched pair of the source thread j serves (order[j], or j itself when order is null) in the normalised frame: a, b and
// dn = d2 / u^2; false for a skipped source.  txyz: the target's points in caller order (the index the search returns addresses them);
// t: that index (the point-to-plane pass of pm_align_plane.hpp gathers the target's normal with it).
__host__ __device__ inline bool align_match_one(size_t j, const float* __restrict__ src, const int* __restrict__ order, const AlignXf& f, const CloudGrid& g,
                                                const float* __restrict__ txyz, double a[3], double b[3], double& dn, size_t& t) {
    const size_t i = order ? (size_t)order[j] : j;
    float x, y, z;
    int cx, cy, cz;
    if (!align_point(i, src, f, g, x, y, z, cx, cy, cz)) return false;
    const unsigned long long best = cloud_search(x, y, z, cx, cy, cz, g);
    if (best == ~0ull) return false;
    const float d2 = cloud_float((uint32_t)(best >> 32));
    t = (size_t)(uint32_t)(best & 0xffffffffull);
    a[0] = ((double)x - f.o[0]) * f.iu, a[1] = ((double)y - f.o[1]) * f.iu, a[2] = ((double)z - f.o[2]) * f.iu;
    b[0] = ((double)txyz[3 * t] - f.o[0]) * f.iu, b[1] = ((double)txyz[3 * t + 1] - f.o[1]) * f.iu, b[2] = ((double)txyz[3 * t + 2] - f.o[2]) * f.iu;
    dn = (double)d2 * (f.iu * f.iu);
    return true;
}
__host__ __device__ inline bool align_pair_one(size_t j, const float* __restrict__ src, const int* __restrict__ order, const AlignXf& f, const CloudGrid& g,
                                               const float* __restrict__ txyz, double a[3], double b[3], double& dn) {
    size_t t;
    return align_match_one(j, src, order, f, g, txyz, a, b, dn, t);
}

// term k of a matched pair
__host__ __device__ inline long long align_term(int k, const double a[3], const double b[3], double dn) {
    if (k == 0) return 1;
    if (k < 4) return align_fix(a[k - 1]);
    if (k < 7) return align_fix(b[k - 4]);
    if (k < 16) return align_fix(a[(k - 7) / 3] * b[(k - 7) % 3]);
    if (k == 16) return align_fix((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    return align_fix(dn);
}

// a 64-bit value across lanes: two dwords travel, the halves are joined again, and only then does the 64-bit add run
__device__ inline long long align_shfl_xor(long long v, int d) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v & 0xffffffffull), d, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), d, 64);
    return (long long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

// one thread per source; sums[18] must be zero before the launch.  Term by term: formed, added across the wave, parked in LDS --
// a thread never holds more than one 64-bit term, so the kernel keeps the occupancy of the search.
__global__ __launch_bounds__(256) void k_align_pass(const float* __restrict__ src, int n, const int* __restrict__ order, AlignXf f, CloudGrid g,
                                                    const float* __restrict__ txyz, unsigned long long* __restrict__ sums) {
    __shared__ long long part[4][kAlignTerms];
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, dn = 0.0;
    const bool matched = j < (size_t)n && align_pair_one(j, src, order, f, g, txyz, a, b, dn);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kAlignTerms; ++k) {
        long long v = matched ? align_term(k, a, b, dn) : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += align_shfl_xor(v, d);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kAlignTerms) {
        const long long s = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (s != 0) atomicAdd(&sums[threadIdx.x], (unsigned long long)s);   // two's complement: the unsigned add is the signed one
    }
}

}  // namespace pm
