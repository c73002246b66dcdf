// pm_ingest.hpp -- 8-bit image entry (mpmvs_set_views_u8, mpmvs_resize_u8): the views arrive as the bytes the files decoded
// to, at the files' size, and are shrunk to the size the Problem runs at on the device.  The reference does both on the host
// (imread(GRAYSCALE) + convertTo(CV_32F), src/PatchMatch.cpp:877-882; cv::resize(INTER_LINEAR), :893-925).
//
// The resampled image is DEFINED by the host statement ResizeLinear (host/PatchMatchHost.cpp): fp32, no contraction, sample
// position (x + 0.5f) * (src / dst) - 0.5f, the two clamp rules, top + ay * (bot - top).  Every kernel here takes its pixel
// values from the one function ingest_sample() (ingest_value() = the same from pixel coordinates), so the texels, the padded
// reference image and the probe cannot drift apart; the library is built with -ffp-contract=off and without fast-math, which
// makes the results bit-identical to the host's.  Measurements: profiles/EXPERIMENTS.md (57).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// Source geometry of one view: bytes at their own size, rows `pitch` bytes apart; sx = (float)src_w / dst_w and
// sy = (float)src_h / dst_h are formed on the host exactly as ResizeLinear forms them.
struct IngestSrc {
    const unsigned char* __restrict__ p;
    int w, h;
    unsigned pitch;   // < 2^32: a source image stays below 4 GB (checked by the caller)
    float sx, sy;
};

// one axis of ResizeLinear: the two source indices and the weight of the second for destination index d.  RESAMPLE = false: the image
// already has its size, index d stands for itself (what the formula gives for scale 1, without the arithmetic).
struct IngestAxis {
    int i0, i1;
    float a;
};
template <bool RESAMPLE>
__device__ __forceinline__ IngestAxis ingest_axis(int d, float scale, int n) {
    if (!RESAMPLE) return {d, d, 0.0f};
    const float f = ((float)d + 0.5f) * scale - 0.5f;
    int i0 = (int)floorf(f);
    float a = f - (float)i0;
    if (i0 < 0) { i0 = 0; a = 0.0f; }
    if (i0 >= n - 1) { i0 = n - 1; a = 0.0f; }
    const int i1 = i0 + 1 > n - 1 ? n - 1 : i0 + 1;
    return {i0, i1, a};
}

// THE resampling function: the pixel of the fp32 image that the byte image stands for, from its column and row terms (the column
// terms depend on x only, the row terms on y only: a caller that walks a column or a row forms them once).
template <bool RESAMPLE>
__device__ __forceinline__ float ingest_sample(const IngestSrc& s, const IngestAxis& cx, const IngestAxis& cy) {
    const unsigned char* r0 = s.p + (size_t)cy.i0 * s.pitch;
    if (!RESAMPLE) return (float)r0[cx.i0];
    const unsigned char* r1 = s.p + (size_t)cy.i1 * s.pitch;
    const float s00 = (float)r0[cx.i0], s10 = (float)r0[cx.i1], s01 = (float)r1[cx.i0], s11 = (float)r1[cx.i1];
    const float top = s00 + cx.a * (s10 - s00);
    const float bot = s01 + cx.a * (s11 - s01);
    return top + cy.a * (bot - top);
}
template <bool RESAMPLE>
__device__ __forceinline__ float ingest_value(const IngestSrc& s, int x, int y) {
    return ingest_sample<RESAMPLE>(s, ingest_axis<RESAMPLE>(x, s.sx, s.w), ingest_axis<RESAMPLE>(y, s.sy, s.h));
}

// bytes -> fp32 quad-difference texture (SrcTex): w x h float4 texels (t00, t10 - t00, t01 - t00, (t11 - t01) - (t10 - t00)) of
// the resampled image, the neighbours clamped at the DESTINATION edge as k_pack_quads_f32 clamps them.  A block makes
// kIngestTW x kIngestTH texels: every pixel value of the (TW + 1) x (TH + 1) tile is computed once into LDS (a texel needs four
// of them, each from four source bytes), then every thread stores whole texels, a wave a 1 KB row segment at a time.
// The tile is filled in five fully unrolled slots per thread, so that the byte loads of all of them are in flight together (one
// slot after the other, a block waits five memory round trips in a row): slots 0..3 are rows wy + 4 k of the thread's own
// column, whose terms are formed once; slot 4 is the last row and, on the second wave, the extra column.
constexpr int kIngestTW = 64, kIngestTH = 16, kIngestThreads = 256;
template <bool RESAMPLE>
__global__ __launch_bounds__(kIngestThreads) void k_ingest_quads(IngestSrc s, int w, int h, float4* __restrict__ dst) {
    static_assert(kIngestThreads == 4 * kIngestTW && kIngestTH == 16, "the slot scheme below is written for a 64 x 16 tile and 4 waves");
    __shared__ float tile[kIngestTH + 1][kIngestTW + 1];
    const int bx = blockIdx.x * kIngestTW, by = blockIdx.y * kIngestTH;
    const int lx = threadIdx.x % kIngestTW, wy = threadIdx.x / kIngestTW;
    auto col = [&](int l) { return ingest_axis<RESAMPLE>(bx + l > w - 1 ? w - 1 : bx + l, s.sx, s.w); };
    auto row = [&](int l) { return ingest_axis<RESAMPLE>(by + l > h - 1 ? h - 1 : by + l, s.sy, s.h); };
    const IngestAxis cx = col(lx);
    float v[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ingest_sample<RESAMPLE>(s, cx, row(wy + 4 * k));
    // slot 4: wave 0 the last row, the first TH + 1 threads of wave 1 the extra column (the others repeat a pixel and drop it)
    const bool extra = wy == 1 && lx <= kIngestTH;
    const int ex = extra ? kIngestTW : lx, ey = extra ? lx : kIngestTH;
    v[4] = ingest_sample<RESAMPLE>(s, extra ? col(kIngestTW) : cx, row(ey));
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[wy + 4 * k][lx] = v[k];
    if (wy == 0 || extra) tile[ey][ex] = v[4];
    __syncthreads();
    const int x = bx + lx;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = wy + 4 * k, y = by + ly;
        if (y >= h) return;
        const float t00 = tile[ly][lx], t10 = tile[ly][lx + 1], t01 = tile[ly + 1][lx], t11 = tile[ly + 1][lx + 1];
        dst[(size_t)y * w + x] = make_float4(t00, t10 - t00, t01 - t00, (t11 - t01) - (t10 - t00));
    }
}

// bytes -> replicate-padded fp32 image of (w + 2 apron) x (h + 2 apron) pixels: the reference image (apron = kRefApron) and,
// with apron 0, the dense output of the probe.  Every pixel value is needed once (the apron aside), so there is nothing to share.
__global__ void k_ingest_pad(IngestSrc s, int w, int h, float* __restrict__ dst, int apron) {
    const int pw = w + 2 * apron, ph = h + 2 * apron;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pw || y >= ph) return;
    int dx = x - apron, dy = y - apron;
    dx = dx < 0 ? 0 : (dx > w - 1 ? w - 1 : dx);
    dy = dy < 0 ? 0 : (dy > h - 1 ? h - 1 : dy);
    dst[(size_t)y * pw + x] = ingest_value<true>(s, dx, dy);
}
