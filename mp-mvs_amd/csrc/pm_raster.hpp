// pm_raster.hpp -- a triangle mesh rasterised into pinhole cameras: per pixel the depth of the nearest surface along its ray and the
// triangle it shows (mpmvs_surface_render_depth; contract: include/mpmvs.h, statement 7 of the mesh section).
// Homogeneous rasterisation: the edge functions are the rows of the adjugate of the 3 x 3 matrix of image vertices, the depth is a
// quotient of determinants; no inverse of K, no clipping.  Bit for bit the plain-loop statement and independent of scheduling: all
// that threads share are 64-bit integer minima, counters and one list whose order never reaches a result.
//
// Passes (the key buffers of a chunk of views lie behind one another, 8 bytes per pixel):
//   1. k_raster_init     every key = (bits(+inf) << 32) | 0xffffffff.
//   2. k_raster_small    one thread per triangle, the views of the chunk in a loop (the cameras are kernel arguments, indexed
//                        uniformly): q, the three normals and det once per (triangle, view), then the pixel box.  A box of at most
//                        `large` pixels is walked by the thread (an empty box counts as one pixel); a larger one goes to a list as
//                        (view, triangle): a box of at most kRasterSplit pixels from the front of the list, a larger one from its back.
//   3. k_raster_large    launched twice; the lists' lengths are read on the device.  First the boxes of the front, a wave each
//                        (four per block and round); then those of the back, each dealt to the lanes of kRasterSlices blocks, so
//                        that one triangle that fills the image is no single block's work.  The pair's setup is done once, by the
//                        first lane of the wave or block, and shared through LDS.
//   4. k_raster_resolve  one thread per pixel: key -> depth and triangle, and the number of covered pixels, one atomic per block.
// Per candidate pixel: the key is read first; a key only falls, so a candidate that is not below what was read is dropped without an
// atomic, and one whose triangle's nearest corner is not below it without the division.
// The per-thread bodies are host and device code, so that tools/mesh_render_check.cpp replays the passes thread by thread under the
// sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"    // cloud_bits, cloud_float, cloud_finite

namespace pm {

constexpr int kRasterChunk = 8;              // views per launch of the triangle passes, as kRenderChunk of pm_render.hpp
constexpr int kRasterLargeDefault = 128;      // pixels of a box above which the pair goes to the list: measured, DESIGN.md 27.5
constexpr uint32_t kRasterSplit = 8192;       // pixels of a listed box above which kRasterSlices blocks share it; up to it: a wave
constexpr int kRasterSlices = 32;
constexpr unsigned long long kRasterNone = 0x7f800000ffffffffull;   // (bits(+inf) << 32) | 0xffffffff

struct RasterView {
    float K[9], R[9], t[3];
    int w, h;
    unsigned long long* keys;   // [h * w]
};
struct RasterChunkArgs {
    int n;
    int large;   // a box with more pixels than this goes to the list
    RasterView v[kRasterChunk];
};

// the shared minimum and counter; the host replay runs one thread at a time
__host__ __device__ inline void raster_min(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
__host__ __device__ inline unsigned long long raster_add(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const unsigned long long old = *p;
    *p = old + v;
    return old;
#endif
}

__host__ __device__ inline bool raster_finite(double x) { return x - x == 0.0; }   // false for an infinity and a NaN
__host__ __device__ inline double raster_abs(double x) { return x < 0.0 ? -x : x; }
__host__ __device__ inline double raster_min3(double a, double b, double c) {
    const double m = b < a ? b : a;
    return c < m ? c : m;
}
__host__ __device__ inline double raster_max3(double a, double b, double c) {
    const double m = b > a ? b : a;
    return c > m ? c : m;
}

// one (triangle, view) pair: what every pixel of it needs, and the box of pixels outside of which none is a candidate
struct RasterTri {
    double n[3][3];     // nbc, nca, nab
    double det, zlo, zhi;
    uint32_t zlo_bits;  // bits((float)zlo) where that is positive, else 0: no key of this pair is below (zlo_bits << 32)
    int x0, y0, bw, bh; // the box: first pixel, width and height; bw = 0: empty
};

// u x v, each component two products and one difference: swapping u and v negates every bit of it
__host__ __device__ inline void raster_cross(const double u[3], const double v[3], double out[3]) {
    out[0] = u[1] * v[2] - u[2] * v[1];
    out[1] = u[2] * v[0] - u[0] * v[2];
    out[2] = u[0] * v[1] - u[1] * v[0];
}
// the same with every term's magnitude: what bounds the rounding of the cross product
__host__ __device__ inline void raster_cross_abs(const double u[3], const double v[3], double out[3]) {
    out[0] = raster_abs(u[1] * v[2]) + raster_abs(u[2] * v[1]);
    out[1] = raster_abs(u[2] * v[0]) + raster_abs(u[0] * v[2]);
    out[2] = raster_abs(u[0] * v[1]) + raster_abs(u[1] * v[0]);
}

// THE BOX.  Only where all three q.z > 0; else, and wherever a number below leaves its range, the box is the whole image.  The box
// only skips work, so it must hold every candidate pixel of the image; DESIGN.md 27.2 has the argument in full.  In short: with a, b,
// c the image points q.xy / q.z and lambda the barycentric coordinates of a pixel p in them, lambda_a = E0 * qa.z / det exactly.  A
// computed edge function differs from the exact one by at most d_k = 2^-49 * ((w-1) * A.x + (h-1) * A.y + A.z) + 2^-1000, A the cross
// product with every term's magnitude (five roundings of 2^-53 each, taken as sixteen).  A candidate has three computed E of one sign,
// so with eps_k = d_k * q_k.z / |det| either every lambda_k >= -eps_k, and then p lies within (eps_0 + eps_1 + eps_2) * the box's
// larger side of the triangle, or every lambda_k <= eps_k, which the sum of 1 forbids while eps_0 + eps_1 + eps_2 < 1/4.  |det| is
// taken smaller by the rounding of its own three products.  The box is widened by that margin, by 2^-40 of the largest coordinate for
// the three divisions, and by one pixel, and clipped to the image.
__host__ __device__ inline void raster_box(RasterTri& T, const double q[3][3], int w, int h) {
    T.x0 = 0, T.y0 = 0, T.bw = w, T.bh = h;
    if (!(q[0][2] > 0.0 && q[1][2] > 0.0 && q[2][2] > 0.0)) return;
    double big = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (!(q[c][2] >= 0x1p-200)) return;
        for (int a = 0; a < 3; ++a) big = raster_abs(q[c][a]) > big ? raster_abs(q[c][a]) : big;
    }
    if (!(big <= 0x1p200)) return;
    double A[3][3];
    raster_cross_abs(q[1], q[2], A[0]);
    raster_cross_abs(q[2], q[0], A[1]);
    raster_cross_abs(q[0], q[1], A[2]);
    const double ddet = 0x1p-49 * ((raster_abs(q[0][0]) * A[0][0] + raster_abs(q[0][1]) * A[0][1]) + raster_abs(q[0][2]) * A[0][2]) + 0x1p-1000;
    const double adet = raster_abs(T.det) - ddet;
    if (!(adet > 0.0)) return;
    double eps = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double d = 0x1p-49 * (((double)(w - 1) * A[k][0] + (double)(h - 1) * A[k][1]) + A[k][2]) + 0x1p-1000;
        eps += d * q[k][2] / adet;
    }
    if (!(eps < 0.25)) return;
    const double ua = q[0][0] / q[0][2], ub = q[1][0] / q[1][2], uc = q[2][0] / q[2][2];
    const double va = q[0][1] / q[0][2], vb = q[1][1] / q[1][2], vc = q[2][1] / q[2][2];
    const double ulo = raster_min3(ua, ub, uc), uhi = raster_max3(ua, ub, uc), vlo = raster_min3(va, vb, vc), vhi = raster_max3(va, vb, vc);
    const double side = (uhi - ulo) > (vhi - vlo) ? (uhi - ulo) : (vhi - vlo);
    const double reach = raster_max3(raster_abs(ulo) > raster_abs(uhi) ? raster_abs(ulo) : raster_abs(uhi), raster_abs(vlo), raster_abs(vhi));
    const double margin = (eps * side * 1.0625 + reach * 0x1p-40) + 1.0;
    if (!raster_finite(margin)) return;
    double x0 = floor(ulo - margin), x1 = ceil(uhi + margin), y0 = floor(vlo - margin), y1 = ceil(vhi + margin);
    x0 = x0 < 0.0 ? 0.0 : x0;
    y0 = y0 < 0.0 ? 0.0 : y0;
    x1 = x1 > (double)(w - 1) ? (double)(w - 1) : x1;
    y1 = y1 > (double)(h - 1) ? (double)(h - 1) : y1;
    if (!(x0 <= x1 && y0 <= y1)) {   // outside the image
        T.bw = T.bh = 0;
        return;
    }
    T.x0 = (int)x0, T.y0 = (int)y0;
    T.bw = (int)x1 - (int)x0 + 1, T.bh = (int)y1 - (int)y0 + 1;
}

// triangle t in view V; false: it takes no part
__host__ __device__ inline bool raster_setup(RasterTri& T, const float* __restrict__ xyz, const int32_t* __restrict__ tri, size_t t, const RasterView& V) {
    double q[3][3];
    bool fin = true;
    for (int c = 0; c < 3; ++c) {
        const size_t v = (size_t)tri[3 * t + c];
        const double p0 = (double)xyz[3 * v], p1 = (double)xyz[3 * v + 1], p2 = (double)xyz[3 * v + 2];
        double X[3];
        for (int j = 0; j < 3; ++j) X[j] = (((double)V.R[3 * j] * p0 + (double)V.R[3 * j + 1] * p1) + (double)V.R[3 * j + 2] * p2) + (double)V.t[j];
        for (int j = 0; j < 3; ++j) {
            q[c][j] = ((double)V.K[3 * j] * X[0] + (double)V.K[3 * j + 1] * X[1]) + (double)V.K[3 * j + 2] * X[2];
            fin = fin && raster_finite(q[c][j]);
        }
    }
    if (!fin) return false;
    T.zhi = raster_max3(q[0][2], q[1][2], q[2][2]);
    if (!(T.zhi > 0.0)) return false;
    T.zlo = raster_min3(q[0][2], q[1][2], q[2][2]);
    raster_cross(q[1], q[2], T.n[0]);
    raster_cross(q[2], q[0], T.n[1]);
    raster_cross(q[0], q[1], T.n[2]);
    T.det = (q[0][0] * T.n[0][0] + q[0][1] * T.n[0][1]) + q[0][2] * T.n[0][2];
    const float zl = (float)T.zlo;
    T.zlo_bits = (zl > 0.0f) ? cloud_bits(zl) : 0u;
    raster_box(T, q, V.w, V.h);
    return true;
}

// pixel (x, y) of the pair: the statement's rules from "per pixel" to the key; 1 if it issued the atomic minimum
__host__ __device__ inline int raster_pixel(const RasterTri& T, uint32_t t, int x, int y, int w, unsigned long long* __restrict__ keys) {
    const double xd = (double)x, yd = (double)y;
    const double E0 = (xd * T.n[0][0] + yd * T.n[0][1]) + T.n[0][2];
    const double E1 = (xd * T.n[1][0] + yd * T.n[1][1]) + T.n[1][2];
    const double E2 = (xd * T.n[2][0] + yd * T.n[2][1]) + T.n[2][2];
    if (!((E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0) || (E0 <= 0.0 && E1 <= 0.0 && E2 <= 0.0))) return 0;
    const double S = (E0 + E1) + E2;
    if (!(S != 0.0)) return 0;
    unsigned long long* const slot = keys + ((size_t)y * (size_t)w + (size_t)x);
    // a key only ever falls: what is read here is no smaller than the key is by now, so skipping on it loses nothing.  The depth is
    // clamped to zlo from below and the conversion is monotone: no key of this pair is below (zlo_bits << 32) | t.
    const unsigned long long seen = *slot;
    if ((((unsigned long long)T.zlo_bits << 32) | t) >= seen) return 0;
    double z = T.det / S;
    z = z < T.zlo ? T.zlo : z;
    z = z > T.zhi ? T.zhi : z;
    const float zf = (float)z;
    if (!(cloud_finite(zf) && zf > 0.0f)) return 0;
    const unsigned long long key = ((unsigned long long)cloud_bits(zf) << 32) | t;
    if (!(key < seen)) return 0;
    raster_min(slot, key);
    return 1;
}

__host__ __device__ inline void raster_init_one(size_t i, unsigned long long* __restrict__ keys) { keys[i] = kRasterNone; }

// what a thread of the small pass adds to the call's counters
struct RasterTally {
    unsigned long long part, tested, atomics;   // pairs taking part; pixels of their boxes, listed or walked; atomic minima issued
};

// thread t of the small pass.  list has `cap` entries ((view << 32) | triangle): the pairs up to kRasterSplit pixels fill it from the
// front (n_list[0] counts them), the larger ones from the back (n_list[1]); every pair is listed at most once, so cap = m * A.n holds both.
__host__ __device__ inline void raster_small_one(size_t t, const float* __restrict__ xyz, const int32_t* __restrict__ tri, const RasterChunkArgs& A,
                                                 unsigned long long* __restrict__ list, size_t cap, unsigned long long* __restrict__ n_list, RasterTally& tally) {
    for (int k = 0; k < A.n; ++k) {
        const RasterView& V = A.v[k];
        RasterTri T;
        if (!raster_setup(T, xyz, tri, t, V)) continue;
        ++tally.part;
        const uint32_t pixels = (uint32_t)T.bw * (uint32_t)T.bh;   // a view has at most 2^31 - 1 pixels
        tally.tested += pixels;
        // an empty box counts as one pixel: with large = 0 every pair that takes part is listed
        if ((pixels > 0u ? pixels : 1u) > (uint32_t)A.large) {
            const unsigned long long e = ((unsigned long long)(uint32_t)k << 32) | (unsigned long long)(uint32_t)t;
            if (pixels > kRasterSplit) list[cap - 1 - (size_t)raster_add(&n_list[1], 1ull)] = e;
            else list[raster_add(&n_list[0], 1ull)] = e;
            continue;
        }
        for (int y = 0; y < T.bh; ++y)
            for (int x = 0; x < T.bw; ++x) tally.atomics += (unsigned long long)raster_pixel(T, (uint32_t)t, T.x0 + x, T.y0 + y, V.w, V.keys);
    }
}

// the setup of a listed pair, done once for the lanes that share it; false: nothing to do
__host__ __device__ inline bool raster_large_setup(RasterTri& T, unsigned long long e, const float* __restrict__ xyz, const int32_t* __restrict__ tri,
                                                   const RasterChunkArgs& A) {
    return raster_setup(T, xyz, tri, (size_t)(e & 0xffffffffull), A.v[(int)(e >> 32)]) && T.bw > 0;
}

// one lane of a listed pair: the pixels first, first + step, ... of its box; returns the atomic minima it issued
__host__ __device__ inline int raster_large_lane(const RasterTri& T, unsigned long long e, const RasterChunkArgs& A, uint32_t first, uint32_t step) {
    const RasterView& V = A.v[(int)(e >> 32)];
    const uint32_t pixels = (uint32_t)T.bw * (uint32_t)T.bh, bw = (uint32_t)T.bw;
    int atomics = 0;
    for (uint32_t j = first; j < pixels; j += step) {   // pixels < 2^31 and step <= 2^13: j cannot wrap
        const uint32_t y = j / bw, x = j - y * bw;
        atomics += raster_pixel(T, (uint32_t)(e & 0xffffffffull), T.x0 + (int)x, T.y0 + (int)y, V.w, V.keys);
    }
    return atomics;
}

// thread i of the resolve, over the pixels of the whole chunk: true if the pixel is covered.  No branch on "none": the bits of +inf
// are masked to those of 0.0f and 0xffffffff is -1.
__host__ __device__ inline bool raster_resolve_one(size_t i, const unsigned long long* __restrict__ keys, float* __restrict__ depth, int32_t* __restrict__ out_tri) {
    const unsigned long long k = keys[i];
    const bool covered = k != kRasterNone;
    depth[i] = cloud_float((uint32_t)(k >> 32) & (covered ? 0xffffffffu : 0u));
    if (out_tri) out_tri[i] = (int32_t)(uint32_t)(k & 0xffffffffull);
    return covered;
}

// ---- kernels: `inline`, as pm_cloud.hpp says of its own ------------------------------------------------------------------------------
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
#if defined(__HIPCC__)
// the sum of v over a wave, in every lane
__device__ inline unsigned long long raster_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
#endif

inline __global__ __launch_bounds__(256) void k_raster_init(size_t n, unsigned long long* __restrict__ keys) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) raster_init_one(i, keys);
}

// counters: [0] pairs taking part, [1] pixels of their boxes, [2] atomic minima issued
inline __global__ __launch_bounds__(256) void k_raster_small(int m, const float* __restrict__ xyz, const int32_t* __restrict__ tri, RasterChunkArgs A,
                                                      unsigned long long* __restrict__ list, size_t cap, unsigned long long* __restrict__ n_list,
                                                      unsigned long long* __restrict__ counters) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    RasterTally tally = {0ull, 0ull, 0ull};
    if (t < (size_t)m) raster_small_one(t, xyz, tri, A, list, cap, n_list, tally);
    const unsigned long long part = raster_wave_sum(tally.part), tested = raster_wave_sum(tally.tested), atomics = raster_wave_sum(tally.atomics);
    if ((threadIdx.x & 63) == 0) {
        if (part > 0) atomicAdd(&counters[0], part);
        if (tested > 0) atomicAdd(&counters[1], tested);
        if (atomics > 0) atomicAdd(&counters[2], atomics);
    }
}

// split == 0: the front of the list, a wave per pair, four pairs per block and round.  split != 0: the back of the list, a block per
// (pair, slice).  Every wave of a block runs the same number of rounds, so the two barriers of a round are met by all of them.
inline __global__ __launch_bounds__(256) void k_raster_large(const float* __restrict__ xyz, const int32_t* __restrict__ tri, RasterChunkArgs A,
                                                      const unsigned long long* __restrict__ list, size_t cap, const unsigned long long* __restrict__ n_list,
                                                      int split, unsigned long long* __restrict__ n_atomics) {
    __shared__ RasterTri shared_tri[4];
    __shared__ int shared_ok[4];
    const int tid = (int)threadIdx.x, g = split ? 0 : tid >> 6, lane = split ? tid : (tid & 63);
    const size_t per = split ? 1 : 4;
    const size_t n = split ? (size_t)n_list[1] * kRasterSlices : (size_t)n_list[0];
    unsigned long long atomics = 0;
    for (size_t base = (size_t)blockIdx.x * per; base < n; base += (size_t)gridDim.x * per) {
        const size_t item = base + (size_t)g;
        const bool live = item < n;
        unsigned long long e = 0;
        uint32_t slice = 0;
        if (live) {
            e = split ? list[cap - 1 - item / kRasterSlices] : list[item];
            slice = split ? (uint32_t)(item % kRasterSlices) : 0u;
        }
        if (live && lane == 0) shared_ok[g] = raster_large_setup(shared_tri[g], e, xyz, tri, A) ? 1 : 0;
        __syncthreads();
        if (live && shared_ok[g]) {
            const RasterTri T = shared_tri[g];
            atomics += (unsigned long long)raster_large_lane(T, e, A, split ? slice * 256u + (uint32_t)lane : (uint32_t)lane, split ? (uint32_t)kRasterSlices * 256u : 64u);
        }
        __syncthreads();
    }
    atomics = raster_wave_sum(atomics);
    if ((tid & 63) == 0 && atomics > 0) atomicAdd(n_atomics, atomics);
}

inline __global__ __launch_bounds__(256) void k_raster_resolve(size_t n, const unsigned long long* __restrict__ keys, float* __restrict__ depth,
                                                        int32_t* __restrict__ out_tri, unsigned long long* __restrict__ n_covered) {
    __shared__ unsigned long long wave_sum[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long covered = raster_wave_sum((i < n && raster_resolve_one(i, keys, depth, out_tri)) ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = covered;
    __syncthreads();
    if (threadIdx.x == 0) {   // one atomic per block
        const unsigned long long sum = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        if (sum > 0) atomicAdd(n_covered, sum);
    }
}
#pragma clang diagnostic pop

}  // namespace pm
