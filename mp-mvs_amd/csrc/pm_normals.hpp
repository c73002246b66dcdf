// pm_normals.hpp -- a surface normal per point of a cloud, fitted to its k nearest neighbours (mpmvs_cloud_normals; contract:
// DESIGN.md section 18 and include/mpmvs.h).  Per point the self-excluded list of pm_knn.hpp, the 3 x 3 scatter matrix of the
// min(k, candidates) neighbours and the point itself written about the point, its eigenvectors by eight cyclic Jacobi sweeps, the
// eigenvector of the smallest eigenvalue as the normal, the "surface variation" as the curvature, and a sign: canonical, towards a
// viewpoint, or by a reference normal.  fp64 throughout, no contraction, only + - * / sqrt fabs and comparisons, every one of them
// IEEE-correct on gfx950 and on the host: bit for bit the plain loop of the header, and independent of scheduling, because the list
// is (pm_knn.hpp) and everything after it is a fixed sequence of operations on that list.
//
// k_knn_normal<K> is the third store variant of the list search, next to k_knn_list and k_knn_reduce: one thread per point in binned
// order, the list of K 64-bit keys in registers, never in HBM.  The neighbours' coordinates are gathered by index from the handle's
// resident xyz (12 bytes each, as k_align_pass reads p_j) in one fully unrolled loop over K with an e < m predicate; after that loop
// the list is dead, so the Jacobi phase -- six matrix entries and nine of V, all named scalars: a runtime-indexed array would live
// in scratch -- does not add to the peak register count.  At most 20 bytes are written per point.
// The per-thread body is host and device code, so that tools/normals_check.cpp can replay it thread by thread under the sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_knn.hpp"

namespace pm {

constexpr int kNormalSweeps = 8;

// max(x, 0) of the contract: +0 for a negative, a zero of either sign, or a NaN
__host__ __device__ inline double normal_pos(double x) { return x > 0.0 ? x : 0.0; }

// one Jacobi rotation of the pair (p, q), r the third index: annihilates a_pq; every new value from the old ones
__host__ __device__ __attribute__((always_inline)) inline void normal_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                                                             double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp, arq = rq;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p, v0q = n0q, v1p = n1p, v1q = n1q, v2p = n2p, v2q = n2q;
}

// thread j serves point order[j] (order may be null: j itself) of the cloud xyz, the grid's own targets
template <int K>
__host__ __device__ inline void normal_one(size_t j, const float* __restrict__ xyz, const int* __restrict__ order, const CloudGrid& g, int k, int orient, double vx,
                                           double vy, double vz, const float* __restrict__ ref, float* __restrict__ out_n, float* __restrict__ out_curv,
                                           int32_t* __restrict__ out_within) {
    const size_t i = order ? (size_t)order[j] : j;
    KnnList<K> l;
    const int within = knn_query_list(xyz, i, g, 0, l);
    const int m = within < k ? within : k;
    const double px = (double)xyz[3 * i], py = (double)xyz[3 * i + 1], pz = (double)xyz[3 * i + 2];

    // the nine sums over the m neighbours in ascending list order; the first term initialises
    double sx = 0.0, sy = 0.0, sz = 0.0, qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        if (e < m) {
            const size_t t = (size_t)(uint32_t)(l.key[e] & 0xffffffffull);
            const double ex = (double)xyz[3 * t] - px, ey = (double)xyz[3 * t + 1] - py, ez = (double)xyz[3 * t + 2] - pz;
            sx = e == 0 ? ex : sx + ex;
            sy = e == 0 ? ey : sy + ey;
            sz = e == 0 ? ez : sz + ez;
            qxx = e == 0 ? ex * ex : qxx + ex * ex;
            qxy = e == 0 ? ex * ey : qxy + ex * ey;
            qxz = e == 0 ? ex * ez : qxz + ex * ez;
            qyy = e == 0 ? ey * ey : qyy + ey * ey;
            qyz = e == 0 ? ey * ez : qyz + ey * ez;
            qzz = e == 0 ? ez * ez : qzz + ez * ez;
        }
    }

    float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = cloud_float(0x7f800000u);
    if (m >= 2) {
        const double w = (double)(m + 1);
        double a00 = qxx - (sx * sx) / w, a01 = qxy - (sx * sy) / w, a02 = qxz - (sx * sz) / w;
        double a11 = qyy - (sy * sy) / w, a12 = qyz - (sy * sz) / w, a22 = qzz - (sz * sz) / w;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
        for (int sweep = 0; sweep < kNormalSweeps; ++sweep) {
            if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;   // cannot show: every further rotation would be skipped
            normal_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
            normal_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
            normal_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
        }
        // the smallest of the diagonal (ties: the lowest index) and the smaller of the other two
        const int i0 = a00 <= a11 ? (a00 <= a22 ? 0 : 2) : (a11 <= a22 ? 1 : 2);
        const double d0 = i0 == 0 ? a00 : (i0 == 1 ? a11 : a22);
        const double o1 = i0 == 0 ? a11 : a00, o2 = i0 == 2 ? a11 : a22;
        const double dmid = o1 < o2 ? o1 : o2;
        if (dmid > 0.0) {
            const double tr = (normal_pos(a00) + normal_pos(a11)) + normal_pos(a22);
            double n0 = i0 == 0 ? v00 : (i0 == 1 ? v01 : v02);
            double n1 = i0 == 0 ? v10 : (i0 == 1 ? v11 : v12);
            double n2 = i0 == 0 ? v20 : (i0 == 1 ? v21 : v22);
            // canonical sign: the component of the largest magnitude (ties: the lowest index) is positive
            const double f0 = fabs(n0), f1 = fabs(n1), f2 = fabs(n2);
            const double lead = f0 >= f1 ? (f0 >= f2 ? n0 : n2) : (f1 >= f2 ? n1 : n2);
            bool flip = lead < 0.0;
            if (orient != 0) {
                if (flip) n0 = -n0, n1 = -n1, n2 = -n2;
                double w0, w1, w2;
                if (orient == 1) {
                    w0 = vx - px, w1 = vy - py, w2 = vz - pz;
                } else {
                    w0 = (double)ref[3 * i], w1 = (double)ref[3 * i + 1], w2 = (double)ref[3 * i + 2];
                }
                const double dot = (n0 * w0 + n1 * w1) + n2 * w2;
                flip = dot < 0.0;   // a NaN or a zero keeps the canonical sign
            }
            if (flip) n0 = -n0, n1 = -n1, n2 = -n2;
            nx = (float)n0, ny = (float)n1, nz = (float)n2;
            curv = (float)(normal_pos(d0) / tr);
        }
    }
    out_n[3 * i] = nx, out_n[3 * i + 1] = ny, out_n[3 * i + 2] = nz;
    if (out_curv) out_curv[i] = curv;
    if (out_within) out_within[i] = within;
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_normal(const float* __restrict__ xyz, int n, const int* __restrict__ order, CloudGrid g, int k, int orient, double vx,
                                                    double vy, double vz, const float* __restrict__ ref, float* __restrict__ out_n, float* __restrict__ out_curv,
                                                    int32_t* __restrict__ out_within) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)n) normal_one<K>(j, xyz, order, g, k, orient, vx, vy, vz, ref, out_n, out_curv, out_within);
}

}  // namespace pm
