// pm_skyseg.hpp -- inference kernels of the sky-segmentation network: the U^2-Net the reference runs
// through ncnn on the CPU (SkySegment::maskExtractor, SkySegment/src/SkyRegionDetect.cpp:541-561) and the preprocessing in front of
// it (pyrDown loop of GenerateSkyRegionMask, src/PatchMatch.cpp:16-18; from_pixels_resize + substract_mean_normalize).
//
// Activations are planar fp32 (NCHW as ncnn keeps them), one image.  A blob that a Concat produced is never materialised: a
// kernel takes the list of channel runs (SegSrcs) and walks it.
//
// Convolution 3x3 = implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 operands, fp32 accumulation: gfx950 has no xf32):
//   D[cout][pixel] += W[cout][k] * X[k][pixel],  k = (channel pair, tap, channel of the pair)
// A operand = weights, repacked once at load so that a wave reads the 64 values of one instruction as one 256-byte row;
// B operand = activations, gathered straight from global memory: the 32 pixels of a tile are 32 consecutive floats of one channel
// plane shifted by the tap offset (the image is walked as a flat index, so any size fills the tiles), a border tap loads nothing
// and contributes +0.  A wave owns kSegPT pixel tiles x MT tiles of 32 outputs; the operands of the next channel pair are loaded
// while the 9 * MT * kSegPT instructions of the current one issue.  The accumulator tile has the pixel on the lane, so the
// epilogue (bias, ReLU / sigmoid) stores 128-byte runs per output channel.  No atomics, a fixed summation order: the result is a
// function of the inputs alone.
// Convolutions with one output (the side outputs, the 1x1 fusion layer) and 1x1 kernels take the VALU kernel k_seg_conv_direct.
#pragma once

#include "pm_device.hpp"

namespace pm {

constexpr int kSegMaxSrc = 6;  // = MPMVS_SKYSEG_MAX_CONCAT
struct SegSrcs {
    const float* p[kSegMaxSrc];  // first channel plane of each run
    int c[kSegMaxSrc];           // channels of each run
    int n;
};

typedef float seg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSegPT = 2;          // pixel tiles (of 32) per wave
constexpr int kSegConvThreads = 256;

PM_DEV float seg_sigmoid(float x) {
    return 1.0f / (1.0f + d_exp(-x));  // own exp, IEEE divide; exp(-x) = inf gives 0
}

// plane of global channel c in the run list, nullptr beyond the last one (the zero half of an odd pair)
PM_DEV const float* seg_plane(const SegSrcs& s, int c, size_t hw) {
    const float* r = nullptr;
    int base = 0;
#pragma unroll
    for (int i = 0; i < kSegMaxSrc; ++i) {
        if (i < s.n) {
            const int lc = c - base;
            if (lc >= 0 && lc < s.c[i]) r = s.p[i] + (size_t)lc * hw;
            base += s.c[i];
        }
    }
    return r;
}

// wp: [pair][tap 9][mtile of the whole layer][lane 64] with lane = 32 * (channel of the pair) + (output % 32); zero where the
// channel or the output does not exist.  blockIdx.y selects MT consecutive output tiles.
template <int MT>
__global__ __launch_bounds__(kSegConvThreads) void k_seg_conv3_mfma(SegSrcs src, const float* __restrict__ wp, const float* __restrict__ bias,
                                                                     float* __restrict__ out, int H, int W, int n_pairs, int mtiles_total, int cout, int dil,
                                                                     int act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int hw = H * W;
    const int base = (blockIdx.x * (kSegConvThreads / 64) + wave) * (kSegPT * 32);
    if (base >= hw) return;  // whole wave
    const int mt0 = blockIdx.y * MT;

    int pix[kSegPT];
    unsigned mask[kSegPT];  // bit t: tap t lies inside the image for this lane's pixel
    int toff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) toff[t] = (t / 3 - 1) * dil * W + (t % 3 - 1) * dil;
#pragma unroll
    for (int pt = 0; pt < kSegPT; ++pt) {
        const int p = base + pt * 32 + col;
        pix[pt] = p;
        const int y = p / W, x = p - y * W;
        unsigned m = 0;
        if (p < hw) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + (t / 3 - 1) * dil, xx = x + (t % 3 - 1) * dil;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) m |= 1u << t;
            }
        }
        mask[pt] = m;
    }

    seg_f32x16 acc[MT][kSegPT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int pt = 0; pt < kSegPT; ++pt)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mt][pt][v] = 0.0f;

    float a_cur[9][MT], b_cur[9][kSegPT], a_nxt[9][MT], b_nxt[9][kSegPT];
    auto load = [&](int cp, float (&a)[9][MT], float (&b)[9][kSegPT]) {
        const float* plane = seg_plane(src, 2 * cp + half, (size_t)hw);
        const float* w = wp + ((size_t)cp * 9 * mtiles_total + mt0) * 64 + lane;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[t][mt] = w[((size_t)t * mtiles_total + mt) * 64];
#pragma unroll
            for (int pt = 0; pt < kSegPT; ++pt) {
                float v = 0.0f;
                if (plane != nullptr && ((mask[pt] >> t) & 1u)) v = plane[pix[pt] + toff[t]];
                b[t][pt] = v;
            }
        }
    };
    load(0, a_cur, b_cur);
    for (int cp = 0; cp < n_pairs; ++cp) {
        if (cp + 1 < n_pairs) load(cp + 1, a_nxt, b_nxt);
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int pt = 0; pt < kSegPT; ++pt) acc[mt][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[t][mt], b_cur[t][pt], acc[mt][pt], 0, 0, 0);
        if (cp + 1 < n_pairs) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) a_cur[t][mt] = a_nxt[t][mt];
#pragma unroll
                for (int pt = 0; pt < kSegPT; ++pt) b_cur[t][pt] = b_nxt[t][pt];
            }
        }
    }
    // D layout of the 32x32 tile: column (pixel) = lane & 31, row (output) = 8 * (v / 4) + 4 * (lane >> 5) + (v % 4)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = (mt0 + mt) * 32 + 8 * (v >> 2) + 4 * half + (v & 3);
            if (co >= cout) continue;
            const float bv = bias[co];
#pragma unroll
            for (int pt = 0; pt < kSegPT; ++pt) {
                if (pix[pt] >= hw) continue;
                float r = acc[mt][pt][v] + bv;
                if (act == 1) r = r > 0.0f ? r : 0.0f;
                else if (act == 4) r = seg_sigmoid(r);
                out[(size_t)co * hw + pix[pt]] = r;
            }
        }
}

// Convolution k x k (k = 1 or 3) on the vector ALU, one thread per output pixel, blockIdx.y = output channel.  w in ncnn order
// [cout][cin][ky][kx].  Sum order: channel, then tap (fma chain).
__global__ __launch_bounds__(256) void k_seg_conv_direct(SegSrcs src, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int H,
                                                         int W, int cin, int k, int dil, int act) {
    const int hw = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int co = blockIdx.y;
    const int y = p / W, x = p - y * W;
    const int kk = k * k, r = k / 2;
    const float* wc = w + (size_t)co * cin * kk;
    float acc = 0.0f;
    int cbase = 0;
    for (int s = 0; s < src.n; ++s) {
        for (int c = 0; c < src.c[s]; ++c) {
            const float* plane = src.p[s] + (size_t)c * hw;
            const float* wt = wc + (size_t)(cbase + c) * kk;
            for (int t = 0; t < kk; ++t) {
                const int yy = y + (t / k - r) * dil, xx = x + (t % k - r) * dil;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc = __builtin_fmaf(wt[t], plane[yy * W + xx], acc);
            }
        }
        cbase += src.c[s];
    }
    float v = acc + bias[co];
    if (act == 1) v = v > 0.0f ? v : 0.0f;
    else if (act == 4) v = seg_sigmoid(v);
    out[(size_t)co * hw + p] = v;
}

// Pooling max 2x2 stride 2, ceil mode: the last window of an odd size holds one row / column (ncnn pads the tail with -inf)
__global__ void k_seg_pool2(const float* __restrict__ in, float* __restrict__ out, int C, int H, int W, int OH, int OW) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * OH * OW) return;
    const int ox = i % OW, oy = (i / OW) % OH, c = i / (OW * OH);
    const float* pl = in + (size_t)c * H * W;
    const int y0 = 2 * oy, x0 = 2 * ox;
    const int y1 = y0 + 1 < H ? y0 + 1 : y0, x1 = x0 + 1 < W ? x0 + 1 : x0;
    const float a = pl[y0 * W + x0], b = pl[y0 * W + x1], cc = pl[y1 * W + x0], d = pl[y1 * W + x1];
    out[i] = fmaxf(fmaxf(a, b), fmaxf(cc, d));
}

// Interp bilinear to OH x OW, half-pixel centres, clamped at both ends (ncnn resize_type 2 without align_corner).  The sample
// position is formed in double (exact for every size that occurs), the two-step blend in fp32.
__global__ void k_seg_interp(const float* __restrict__ in, float* __restrict__ out, int C, int H, int W, int OH, int OW) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * OH * OW) return;
    const int ox = i % OW, oy = (i / OW) % OH, c = i / (OW * OH);
    double fy = ((double)oy + 0.5) * ((double)H / (double)OH) - 0.5, fx = ((double)ox + 0.5) * ((double)W / (double)OW) - 0.5;
    fy = fy < 0.0 ? 0.0 : fy;
    fx = fx < 0.0 ? 0.0 : fx;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > H - 1 ? H - 1 : y0;
    x0 = x0 > W - 1 ? W - 1 : x0;
    const int y1 = y0 + 1 < H ? y0 + 1 : y0, x1 = x0 + 1 < W ? x0 + 1 : x0;
    const float ay = y1 == y0 ? 0.0f : (float)(fy - (double)y0), ax = x1 == x0 ? 0.0f : (float)(fx - (double)x0);
    const float* pl = in + (size_t)c * H * W;
    const float s00 = pl[y0 * W + x0], s10 = pl[y0 * W + x1], s01 = pl[y1 * W + x0], s11 = pl[y1 * W + x1];
    const float top = s00 + ax * (s10 - s00), bot = s01 + ax * (s11 - s01);
    out[i] = top + ay * (bot - top);
}

__global__ void k_seg_add(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

__global__ void k_seg_sigmoid(const float* __restrict__ a, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = seg_sigmoid(a[i]);
}

// ---- preprocessing of maskExtractor / GenerateSkyRegionMask ---------------------------------------------------------------
PM_DEV int seg_reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// cv::pyrDown of an 8-bit image with `ch` interleaved channels: 5x5 binomial [1 4 6 4 1]^2 / 256 around source pixel (2x, 2y),
// reflect-101 border, output size given by the caller (the reference asks for (w / 2, h / 2)), rounded (s + 128) >> 8.  Integer arithmetic.
__global__ void k_seg_pyrdown(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int w, int h, int ow, int oh, int ch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ow * oh * ch) return;
    const int c = i % ch, ox = (i / ch) % ow, oy = i / (ch * ow);
    const int kw[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int yy = seg_reflect101(2 * oy + j - 2, h);
        int row = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) row += kw[k] * (int)in[((size_t)yy * w + seg_reflect101(2 * ox + k - 2, w)) * ch + c];
        s += kw[j] * row;
    }
    out[i] = (unsigned char)((s + 128) >> 8);
}

// B,G,R bytes (h x w x 3) -> R,G,B planes of net_h x net_w: the project's ResizeLinear geometry (pm_ingest.hpp) per channel, the
// result rounded to 8 bits (half to even, as the bytes ncnn resizes stay bytes), then (v - mean) * norm in fp32.
struct SegNorm {
    float mean[3], norm[3];  // in R, G, B order
};
__global__ void k_seg_resize_norm(const unsigned char* __restrict__ bgr, int w, int h, float* __restrict__ out, int net_w, int net_h, float sx, float sy,
                                  SegNorm nm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * net_w * net_h) return;
    const int x = i % net_w, y = (i / net_w) % net_h, c = i / (net_w * net_h);  // c: 0 = R
    float fx = ((float)x + 0.5f) * sx - 0.5f, fy = ((float)y + 0.5f) * sy - 0.5f;
    int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    float ax = fx - (float)x0, ay = fy - (float)y0;
    if (x0 < 0) { x0 = 0; ax = 0.0f; }
    if (x0 >= w - 1) { x0 = w - 1; ax = 0.0f; }
    if (y0 < 0) { y0 = 0; ay = 0.0f; }
    if (y0 >= h - 1) { y0 = h - 1; ay = 0.0f; }
    const int x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
    const int sc = 2 - c;  // byte of the B,G,R triple
    const float s00 = (float)bgr[((size_t)y0 * w + x0) * 3 + sc], s10 = (float)bgr[((size_t)y0 * w + x1) * 3 + sc];
    const float s01 = (float)bgr[((size_t)y1 * w + x0) * 3 + sc], s11 = (float)bgr[((size_t)y1 * w + x1) * 3 + sc];
    const float top = s00 + ax * (s10 - s00), bot = s01 + ax * (s11 - s01);
    const float v = __builtin_rintf(top + ay * (bot - top));  // within [0, 255]: a blend of bytes
    out[i] = (v - nm.mean[c]) * nm.norm[c];
}

}  // namespace pm
