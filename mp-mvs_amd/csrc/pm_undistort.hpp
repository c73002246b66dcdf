// pm_undistort.hpp -- the undistortion warp (mpmvs_undistort_u8): the byte image of a distorted COLMAP camera resampled to the
// PINHOLE camera of mpmvs_undistort_camera.  DEFINED by the host statement mpmvs_host_undistort_u8 (host/undistort.cpp): both
// take the source position and the blend from und_tap() / und_blend() of pm_undistort_model.hpp, fp64 without contraction, so
// the bytes and the validity mask are the host's bit for bit.  Contract and measurements: DESIGN.md section 12.
//
// The output is dense (rows W' * C bytes, no pitch), so the kernel walks it as ONE array of W' * H' pixels: a block owns
// kUndThreads consecutive pixels, i.e. kUndThreads * C consecutive bytes that start on a dword boundary whatever W' is.  A thread
// forms the coordinate chain of its pixel once, gathers its 4 * C source bytes straight from global memory (the map is close to
// the identity: the 256 pixels of a block read from a few source rows), and puts its C result bytes into LDS; after the barrier
// the block stores its stretch as whole dwords, a wave 256 contiguous bytes per instruction.  The caller rounds the output
// allocations up to a dword, so the last dword of the image is stored whole as well.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_undistort_model.hpp"

constexpr int kUndThreads = 256;

struct UndPinhole {
    double p[4];   // fx fy cx cy
};

template <int C>
__global__ __launch_bounds__(kUndThreads) void k_undistort(UndModel m, UndPinhole dst, const unsigned char* __restrict__ src, unsigned pitch,
                                                           int W, int H, int dw, unsigned n_pix, unsigned* __restrict__ out,
                                                           unsigned* __restrict__ out_valid) {
    static_assert(C == 1 || C == 3, "1 or 3 interleaved channels");
    __shared__ unsigned px32[kUndThreads * C / 4];
    __shared__ unsigned ok32[kUndThreads / 4];
    unsigned char* px = (unsigned char*)px32;
    unsigned char* ok = (unsigned char*)ok32;
    const unsigned t = threadIdx.x, base = blockIdx.x * kUndThreads, p = base + t;
    unsigned char v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    bool valid = false;
    if (p < n_pix) {
        const int Y = (int)(p / (unsigned)dw), X = (int)(p - (unsigned)Y * (unsigned)dw);
        const UndTap tap = und_tap(m, dst.p, X, Y, W, H);
        valid = tap.valid;
        if (valid) {
            const unsigned char* r0 = src + (size_t)tap.y0 * pitch;
            const unsigned char* r1 = src + (size_t)tap.y1 * pitch;
            unsigned char s00[C], s10[C], s01[C], s11[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {   // all 4 * C loads first: one memory round trip, not C
                s00[c] = r0[tap.x0 * C + c];
                s10[c] = r0[tap.x1 * C + c];
                s01[c] = r1[tap.x0 * C + c];
                s11[c] = r1[tap.x1 * C + c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = und_blend(tap, (double)s00[c], (double)s10[c], (double)s01[c], (double)s11[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) px[t * C + c] = v[c];
    ok[t] = valid ? 1 : 0;
    __syncthreads();
    // dword d of the block's stretch covers bytes base * C + 4 d ...: stored while it begins inside the image
    const size_t n_bytes = (size_t)n_pix * C;
    if (t < kUndThreads * C / 4 && (size_t)base * C + 4 * (size_t)t < n_bytes) out[(size_t)base * C / 4 + t] = px32[t];
    if (out_valid && t < kUndThreads / 4 && base + 4 * t < n_pix) out_valid[base / 4 + t] = ok32[t];
}
