// pm_observe.hpp -- the space a terrestrial scanner observed, as a range cube map per scanner position, and the classification of
// query points against it (mpmvs_observer_*; contract: DESIGN.md section 21 and include/mpmvs.h).  Per scanner j at S and point p,
// everything in fp32 without contraction and with correctly rounded quotients:
//   d = p - S, A = |d|, m = the lowest axis that attains max(A), z = A_m; the point TAKES PART iff its coordinates are finite, z is
//   finite and z > 0;  face = 2 m + (d_m < 0), b = (m + 1) % 3, c = (m + 2) % 3, h = (float)R * 0.5f,
//   x = h * (d_b / z) + h, y = h * (d_c / z) + h  (0 <= x, y <= R),  px = x >= (float)R ? R - 1 : (int)x, py alike.
//   Zc = the smallest z of the scan points of the pixel (+inf: none);  Zn = the smallest Zc of the (2 w + 1)^2 window inside the face;
//   a query is COVERED iff it takes part and Zn at its pixel is finite, FREE iff covered and z + abs < Zn * (1.0f - rel).
// Bit for bit the plain-loop statement and independent of scheduling: all that threads share are integer minima and an integer count.
//
// Passes (the maps of the scanners of a chunk lie behind one another, 6 R^2 entries each; Zc starts as +inf bits):
//   1. k_observe_zmin      one thread per scan point, the scanners of the chunk in a loop (their positions are a kernel argument,
//                          indexed uniformly) or, with an owner per point, the one scanner: the point read once, per (point, scanner)
//                          that takes part one 32-bit atomicMin on the bits of z -- z > 0, so the bits order as the values.
//   2. k_observe_near      one thread per pixel of the chunk: the window minimum in a direct loop clipped to the face (min is
//                          associative, so any order gives the same bits), stored as a float into the resident Zn; the pixels with
//                          a finite Zn are counted per block and added once.
//   3. k_observe_classify  one thread per query, all scanners in a loop: the query read once, one 4-byte gather from Zn per (query,
//                          scanner), the two counts in registers and one store each at the end.
// The per-thread bodies are host and device code, so that tools/observe_check.cpp replays the passes thread by thread under the
// sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"    // cloud_bits, cloud_float, cloud_finite
#include "pm_render.hpp"   // render_min, kRenderInfBits

namespace pm {

constexpr int kObserveMaxScanners = 64;
constexpr int kObserveMaxFace = 4096;
constexpr int kObserveMaxWindow = 8;
constexpr int kObserveChunk = 8;   // scanners per launch of the scan passes: Zc exists for so many at a time
constexpr size_t kObserveChunkPixels = (size_t)1 << 27;   // ... and for fewer when their maps would pass this many pixels (one scanner always fits)
static_assert(kObserveChunkPixels < ((size_t)1 << 32) && (size_t)6 * kObserveMaxFace * kObserveMaxFace < ((size_t)1 << 32), "a chunk's pixel index fits 32 bits");

// scanners [j0, j0 + n) of the handle, whose maps lie behind one another from the map pointer a pass is given
struct ObserveScanners {
    int n, j0;
    float s[kObserveMaxScanners][3];
};

// face-major pixel index inside one scanner's 6 R^2 map, and z, of a point with finite coordinates; false: it takes no part
__host__ __device__ inline bool observe_locate(const float* S, int R, float p0, float p1, float p2, size_t& pix, float& z) {
    const float d0 = p0 - S[0], d1 = p1 - S[1], d2 = p2 - S[2];
    const float a0 = fabsf(d0), a1 = fabsf(d1), a2 = fabsf(d2);
    int m = 0;
    float dm = d0, db = d1, dc = d2;
    z = a0;
    if (a1 > z) m = 1, z = a1, dm = d1, db = d2, dc = d0;
    if (a2 > z) m = 2, z = a2, dm = d2, db = d0, dc = d1;
    if (!(cloud_finite(z) && z > 0.0f)) return false;   // a difference that overflowed, or the scanner's own position
    const float h = (float)R * 0.5f;
    const float x = h * (db / z) + h, y = h * (dc / z) + h;   // |db|, |dc| <= z: both lie in [0, R]
    const int px = x >= (float)R ? R - 1 : (int)x, py = y >= (float)R ? R - 1 : (int)y;
    const int f = 2 * m + (dm < 0.0f ? 1 : 0);
    pix = ((size_t)f * (size_t)R + (size_t)py) * (size_t)R + (size_t)px;
    return true;
}

// scan point i into the maps zc of the chunk's scanners; owner: null, or the scanner of every point (-1: none)
__host__ __device__ inline void observe_point_one(size_t i, const float* __restrict__ xyz, const int* __restrict__ owner, const ObserveScanners& A, int R,
                                                  uint32_t* __restrict__ zc) {
    const float p0 = xyz[3 * i], p1 = xyz[3 * i + 1], p2 = xyz[3 * i + 2];
    if (!(cloud_finite(p0) && cloud_finite(p1) && cloud_finite(p2))) return;
    const size_t face = (size_t)R * (size_t)R;
    int k0 = 0, k1 = A.n;
    if (owner) {
        k0 = owner[i] - A.j0, k1 = k0 + 1;
        if (k0 < 0 || k0 >= A.n) return;
    }
    for (int k = k0; k < k1; ++k) {
        size_t pix;
        float z;
        if (observe_locate(A.s[A.j0 + k], R, p0, p1, p2, pix, z)) render_min(&zc[(size_t)k * 6 * face + pix], cloud_bits(z));
    }
}

__global__ __launch_bounds__(256) void k_observe_zmin(const float* __restrict__ xyz, int n, const int* __restrict__ owner, ObserveScanners A, int R,
                                                      uint32_t* __restrict__ zc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) observe_point_one(i, xyz, owner, A, R, zc);
}

// pixel `pix` of the chunk's maps (a multiple of 6 R^2 entries): the window minimum inside its face; true: it is finite
__host__ __device__ inline bool observe_near_one(size_t pix, const uint32_t* __restrict__ zc, int R, int w, float* __restrict__ zn) {
    const uint32_t face = (uint32_t)R * (uint32_t)R;   // the maps of a chunk hold fewer than 2^32 pixels (kObserveChunkPixels): 32-bit quotients
    const uint32_t base = (uint32_t)pix / face * face, in = (uint32_t)pix - base;
    const int y = (int)(in / (uint32_t)R), x = (int)(in - (uint32_t)y * (uint32_t)R);
    const int x0 = x - w < 0 ? 0 : x - w, x1 = x + w > R - 1 ? R - 1 : x + w;
    const int y0 = y - w < 0 ? 0 : y - w, y1 = y + w > R - 1 ? R - 1 : y + w;
    uint32_t z1 = kRenderInfBits;
    for (int yy = y0; yy <= y1; ++yy) {
        const uint32_t* row = zc + base + (size_t)yy * (size_t)R;
        for (int xx = x0; xx <= x1; ++xx) {
            const uint32_t t = row[xx];
            z1 = t < z1 ? t : z1;
        }
    }
    zn[pix] = cloud_float(z1);
    return z1 != kRenderInfBits;
}

// one thread per pixel; n_pix = scanners of the chunk x 6 R^2
__global__ __launch_bounds__(256) void k_observe_near(const uint32_t* __restrict__ zc, size_t n_pix, int R, int w, float* __restrict__ zn,
                                                      unsigned long long* __restrict__ covered) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool fin = pix < n_pix && observe_near_one(pix, zc, R, w, zn);
    const int c = __syncthreads_count(fin);
    if (threadIdx.x == 0 && c) atomicAdd(covered, (unsigned long long)c);
}

// query q against the maps zn of all scanners of A (A.j0 == 0); m1 = 1.0f - rel
__host__ __device__ inline void observe_classify_one(size_t q, const float* __restrict__ xyz, const ObserveScanners& A, int R, const float* __restrict__ zn, float m1,
                                                     float abs_margin, int* __restrict__ out_free, int* __restrict__ out_covered) {
    const float p0 = xyz[3 * q], p1 = xyz[3 * q + 1], p2 = xyz[3 * q + 2];
    int n_free = 0, n_cov = 0;
    if (cloud_finite(p0) && cloud_finite(p1) && cloud_finite(p2)) {
        const size_t map = (size_t)6 * (size_t)R * (size_t)R;
        for (int j = 0; j < A.n; ++j) {
            size_t pix;
            float z;
            if (!observe_locate(A.s[j], R, p0, p1, p2, pix, z)) continue;
            const float near = zn[(size_t)j * map + pix];
            if (cloud_bits(near) == kRenderInfBits) continue;   // Zn is a positive finite number or +inf
            ++n_cov;
            n_free += z + abs_margin < near * m1 ? 1 : 0;
        }
    }
    out_free[q] = n_free;
    if (out_covered) out_covered[q] = n_cov;
}

__global__ __launch_bounds__(256) void k_observe_classify(const float* __restrict__ xyz, int n, ObserveScanners A, int R, const float* __restrict__ zn, float m1,
                                                          float abs_margin, int* __restrict__ out_free, int* __restrict__ out_covered) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < (size_t)n) observe_classify_one(q, xyz, A, R, zn, m1, abs_margin, out_free, out_covered);
}

}  // namespace pm
