// pm_align_plane.hpp -- one pass of point-to-plane ICP on the device (mpmvs_align_plane_*; contract: DESIGN.md section 19 and
// include/mpmvs.h).  The pass of pm_align.hpp with one more input, a normal per target resident on the align handle, and other
// sums: the matched pair (a, b) of align_match_one, the normal n of the matched target j, and 38 integers instead of 18.
// Bit for bit the plain-loop statement (fp64, no contraction, only + - * / sqrt):
//   n = (double)nrm_j,  q = (n0*n0 + n1*n1) + n2*n2;  the source is skipped when q is not finite or q == 0;
//   nh_k = n_k / sqrt(q);  e = a - b;  r = (e0*nh0 + e1*nh1) + e2*nh2;
//   c = a x nh:  c0 = a1*nh2 - a2*nh1,  c1 = a2*nh0 - a0*nh2,  c2 = a0*nh1 - a1*nh0;  g = (a0*nh0 + a1*nh1) + a2*nh2;
//   J = (c0, c1, c2, nh0, nh1, nh2, g): the derivative of r by a small rotation, a translation and a scale change of the source;
//   sums[0] += 1; sums[1..28] += fix(J_i * J_j) for i <= j, row by row; sums[29 + i] += fix(J_i * r); sums[36] += fix(r * r);
//   sums[37] += fix((double)d2 * (iu * iu)).
// OVERFLOW: |a_k| <= 1 (pm_align.hpp) and |nh_k| <= 1 (q >= n_k^2 as computed, the square root and the quotient are correctly
// rounded and monotone), so |c_k| <= sqrt 2 and |g| <= sqrt 3 by Cauchy-Schwarz.  A matched y lies within radius (1 + 4 * 2^-24)
// of its target along every axis and u >= 2 radius, so |e_k| <= (1 + 4 * 2^-24) / 2 and |r| <= |e| < 0.87.  The largest product
// is g * g <= 3 up to rounding: every |term| < 4, every |fix(term)| < 2^32, and with at most 2^31 - 1 sources every
// |sum| <= 2^32 (2^31 - 1) < 2^63.
// SIGN: -n gives -nh, hence -c, -g and -r, each exactly (a negated product is the product negated, a difference of two negated
// products is the difference negated): J and r change sign together and every product of two of them keeps every bit.
//
// Passes of a call (mpmvs_cloud.hip: align_pass): the binning of pm_align.hpp as it is, then k_align_plane_pass instead of
// k_align_pass: one thread per source; the matched thread gathers the 12 bytes of its target's normal and forms J, r and dn
// once -- nine doubles in named scalars -- and then goes term by term as k_align_pass does: one term formed, added across the
// wave (align_shfl_xor), parked in LDS (4 x 38 x 8 = 1 216 bytes); threads 0..37 add the block's totals with one 64-bit
// integer atomic each.
#pragma once

#include "pm_align.hpp"

namespace pm {

constexpr int kAlignPlaneTerms = 38;

struct AlignPlanePair {
    double c0, c1, c2, n0, n1, n2, g;   // J
    double r, dn;
};

// J, r and dn of the source thread j serves; false for a source that align_match_one skips or whose target has no usable
// normal.  nrm: one normal per target in caller order (any sign, any length).
__host__ __device__ inline bool align_plane_pair_one(size_t j, const float* __restrict__ src, const int* __restrict__ order, const AlignXf& f,
                                                     const CloudGrid& g, const float* __restrict__ txyz, const float* __restrict__ nrm, AlignPlanePair& p) {
    double a[3], b[3];
    size_t t;
    if (!align_match_one(j, src, order, f, g, txyz, a, b, p.dn, t)) return false;
    const double n0 = (double)nrm[3 * t], n1 = (double)nrm[3 * t + 1], n2 = (double)nrm[3 * t + 2];
    const double q = (n0 * n0 + n1 * n1) + n2 * n2;
    if (!(q > 0.0 && q < (double)INFINITY)) return false;   // zero, +inf or NaN (q is never negative)
    const double len = sqrt(q);
    p.n0 = n0 / len, p.n1 = n1 / len, p.n2 = n2 / len;
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    p.r = (e0 * p.n0 + e1 * p.n1) + e2 * p.n2;
    p.c0 = a[1] * p.n2 - a[2] * p.n1;
    p.c1 = a[2] * p.n0 - a[0] * p.n2;
    p.c2 = a[0] * p.n1 - a[1] * p.n0;
    p.g = (a[0] * p.n0 + a[1] * p.n1) + a[2] * p.n2;
    return true;
}

// J_i by selection: under the kernel's full unrolling i is a constant and the chain folds to one register
__host__ __device__ inline double align_plane_j(const AlignPlanePair& p, int i) {
    return i == 0 ? p.c0 : i == 1 ? p.c1 : i == 2 ? p.c2 : i == 3 ? p.n0 : i == 4 ? p.n1 : i == 5 ? p.n2 : p.g;
}

// term k of a matched pair
__host__ __device__ inline long long align_plane_term(int k, const AlignPlanePair& p) {
    if (k == 0) return 1;
    if (k < 29) {   // the upper triangle of J J^T row by row: row i begins at 1 + 7 i - i (i - 1) / 2 and holds 7 - i products
        int i = 0, first = 1;
        while (k >= first + (7 - i)) first += 7 - i, ++i;
        return align_fix(align_plane_j(p, i) * align_plane_j(p, i + (k - first)));
    }
    if (k < 36) return align_fix(align_plane_j(p, k - 29) * p.r);
    if (k == 36) return align_fix(p.r * p.r);
    return align_fix(p.dn);
}

// one thread per source; sums[38] must be zero before the launch.  A thread holds the nine doubles of its pair and one 64-bit term.
__global__ __launch_bounds__(256) void k_align_plane_pass(const float* __restrict__ src, int n, const int* __restrict__ order, AlignXf f, CloudGrid g,
                                                          const float* __restrict__ txyz, const float* __restrict__ nrm, unsigned long long* __restrict__ sums) {
    __shared__ long long part[4][kAlignPlaneTerms];
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    AlignPlanePair p = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool matched = j < (size_t)n && align_plane_pair_one(j, src, order, f, g, txyz, nrm, p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kAlignPlaneTerms; ++k) {
        long long v = matched ? align_plane_term(k, p) : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += align_shfl_xor(v, d);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kAlignPlaneTerms) {
        const long long s = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (s != 0) atomicAdd(&sums[threadIdx.x], (unsigned long long)s);   // two's complement: the unsigned add is the signed one
    }
}

}  // namespace pm
