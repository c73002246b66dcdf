// pm_viewsel.hpp -- view selection of a COLMAP sparse model (the pair scores of the reference's
// colmap2mvsnet_acm.py: calc_score and the argsort that follows it), point-major on the device.
// Contract: for images i < j, shared(i,j) counts the entries of i's point3D_ids
// (with their multiplicity, -1 skipped) whose point j also observes; small(i,j) counts those with a
// triangulation angle below 1 degree; score = 0 if shared == 0 or small >= floor(3 shared / 4) + 1,
// else shared.  Each row lists num_view images by (score desc, index desc).
//
// Passes (all integer bookkeeping; the results do not depend on scheduling):
//   1. k_vs_count / scan / k_vs_scatter: per-image observations -> point-major tracks (the image of
//      every observation, in scatter order).  The scan of the per-point counts into track offsets is
//      the shared one of pm_scan.hpp (k_scan_tiles, k_scan_totals<Sum>, k_vs_scan_add).
//   2. k_vs_mult: per track slot, whether it is the first slot of its image in the track (scanning
//      the track) and, if so, the image's multiplicity in it; other slots get 0.  "First" depends on
//      scatter order, the multiplicity it carries does not, so no per-track sort is needed.
//   3. k_vs_pairs: one thread per first slot (image a, multiplicity m) walks its track; for every
//      first slot of an image b > a it evaluates the angle in fp64 and adds (m << 32) | (m * [theta < 1])
//      to acc[a][b] with one u64 atomic.  Integer atomics commute: bit-reproducible.  A long track is
//      spread over as many threads as it has slots (one wave per 64), so no point serialises a wave.
//   4. k_vs_score: acc upper triangle -> symmetric u32 score matrix (diagonal 0).
//   5. k_vs_select: one block per row, num_view rounds of a block-wide max of the key
//      (score << 32) | k below the previous round's key: score desc, then index desc.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_scan.hpp"

namespace pm {

constexpr int kVsMaxImages = 32768;   // dense N x N accumulators: 12 N^2 bytes (12.9 GB at the cap)

// one block per image: count the observations of every point
__global__ __launch_bounds__(256) void k_vs_count(const int64_t* __restrict__ obs_off, const int32_t* __restrict__ obs_pt, int* __restrict__ cnt) {
    const int64_t b = obs_off[blockIdx.x], e = obs_off[blockIdx.x + 1];
    for (int64_t k = b + threadIdx.x; k < e; k += 256) {
        const int p = obs_pt[k];
        if (p >= 0) atomicAdd(&cnt[p], 1);
    }
}

// one block per image: every observation goes to the next free slot of its point's track
__global__ __launch_bounds__(256) void k_vs_scatter(const int64_t* __restrict__ obs_off, const int32_t* __restrict__ obs_pt, const int* __restrict__ pt_off,
                                                    int* __restrict__ fill, int* __restrict__ trk_img, int* __restrict__ trk_pt) {
    const int img = blockIdx.x;
    const int64_t b = obs_off[img], e = obs_off[img + 1];
    for (int64_t k = b + threadIdx.x; k < e; k += 256) {
        const int p = obs_pt[k];
        if (p < 0) continue;
        const int s = pt_off[p] + atomicAdd(&fill[p], 1);
        trk_img[s] = img;
        trk_pt[s] = p;
    }
}

// per track slot: multiplicity of its image in the track if the slot is that image's first, else 0
__global__ __launch_bounds__(256) void k_vs_mult(int nslots, const int* __restrict__ trk_img, const int* __restrict__ trk_pt, const int* __restrict__ pt_off,
                                                 int* __restrict__ trk_mult) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    const int img = trk_img[s], p = trk_pt[s];
    const int b = pt_off[p], e = pt_off[p + 1];
    int m = 0;
    bool first = true;
    for (int y = b; y < e; ++y) {
        const bool same = trk_img[y] == img;
        m += same ? 1 : 0;
        first = first && !(same && y < s);
    }
    trk_mult[s] = first ? m : 0;
}

__device__ inline double vs_dot(double x0, double x1, double x2, double y0, double y1, double y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

__global__ __launch_bounds__(256) void k_vs_pairs(int nslots, const int* __restrict__ trk_img, const int* __restrict__ trk_pt, const int* __restrict__ trk_mult,
                                                  const int* __restrict__ pt_off, const double* __restrict__ centers, const double* __restrict__ xyz,
                                                  unsigned long long* __restrict__ acc, int n_images) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    const int m = trk_mult[s];
    if (m == 0) return;
    const int a = trk_img[s], p = trk_pt[s];
    const double px = xyz[3 * (size_t)p], py = xyz[3 * (size_t)p + 1], pz = xyz[3 * (size_t)p + 2];
    const double ax = centers[3 * a] - px, ay = centers[3 * a + 1] - py, az = centers[3 * a + 2] - pz;
    const double na = sqrt(vs_dot(ax, ay, az, ax, ay, az));
    const unsigned long long hi = (unsigned long long)m << 32;
    unsigned long long* row = acc + (size_t)a * n_images;
    const int b = pt_off[p], e = pt_off[p + 1];
    for (int y = b; y < e; ++y) {
        const int img = trk_img[y];
        if (img <= a || trk_mult[y] == 0) continue;
        const double bx = centers[3 * img] - px, by = centers[3 * img + 1] - py, bz = centers[3 * img + 2] - pz;
        const double nb = sqrt(vs_dot(bx, by, bz, bx, by, bz));
        const double c = vs_dot(ax, ay, az, bx, by, bz) / na / nb;
        const double theta = (180.0 / M_PI) * acos(c);   // NaN compares false: not small
        atomicAdd(row + img, hi | (theta < 1.0 ? (unsigned long long)m : 0ull));
    }
}

// thread (i, j), j fastest; the upper-triangle accumulator of i < j scores both (i, j) and (j, i)
__global__ __launch_bounds__(256) void k_vs_score(const unsigned long long* __restrict__ acc, int n, unsigned* __restrict__ score) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n || j < i) return;
    if (j == i) {
        score[(size_t)i * n + i] = 0u;
        return;
    }
    const unsigned long long v = acc[(size_t)i * n + j];
    const unsigned long long shared = v >> 32, small = v & 0xffffffffull;
    const unsigned sc = (shared == 0 || small >= (3 * shared) / 4 + 1) ? 0u : (unsigned)shared;
    score[(size_t)i * n + j] = sc;
    score[(size_t)j * n + i] = sc;
}

__device__ inline unsigned long long vs_max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// one block per row: num_view rounds, each the largest key (score << 32 | k) below the previous round's
__global__ __launch_bounds__(256) void k_vs_select(const unsigned* __restrict__ score, int n, int num_view, int32_t* __restrict__ out_ids,
                                                   int32_t* __restrict__ out_scores) {
    __shared__ unsigned long long wbest[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned* row = score + (size_t)i * n;
    unsigned long long thr = ~0ull;
    for (int r = 0; r < num_view; ++r) {
        unsigned long long best = 0;   // a row always has a key left below thr (num_view <= n)
        for (int k = threadIdx.x; k < n; k += 256) {
            const unsigned long long key = ((unsigned long long)row[k] << 32) | (unsigned)k;
            if (key < thr) best = vs_max_u64(best, key);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) best = vs_max_u64(best, __shfl_xor(best, d, 64));
        if (lane == 0) wbest[w] = best;
        __syncthreads();
        thr = vs_max_u64(vs_max_u64(wbest[0], wbest[1]), vs_max_u64(wbest[2], wbest[3]));
        __syncthreads();
        if (threadIdx.x == 0) {
            out_ids[(size_t)i * num_view + r] = (int32_t)(thr & 0xffffffffull);
            out_scores[(size_t)i * num_view + r] = (int32_t)(thr >> 32);
        }
    }
}

}  // namespace pm
