// pm_device.hpp -- device-side building blocks of the PatchMatch hot path for
// gfx950 (MI355X): canonical deterministic fp32 math, Philox RNG, software
// bilinear "texture" fetch (CDNA has no sampler hardware), homography warp,
// bilateral NCC, geometric-consistency cost.
//
// Arithmetic follows DESIGN.md section 3 ("canonical arithmetic"): every fp32
// operation is a correctly rounded IEEE operation or an explicit fma, so this
// file must be compiled with -ffp-contract=off and without fast-math.  The
// reference functions each block restates are cited as "ref .cu:LINES"
// (reference src/PatchMatch.cu).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pm {

#define PM_DEV __device__ __forceinline__

constexpr int kMaxViews = 32;   // ref .cu:500 and the u32 view mask
constexpr int kRefApron = 20;   // widest NCC window radius (scale 2): ref .cu:342-346

// ---------------------------------------------------------------------------
// device-resident problem description (uniform across a launch -> scalar loads)
// ---------------------------------------------------------------------------
struct CamDev {
    float K[9];
    float R[9];
    float t[3];
    float C[3];
};

struct ViewDev {
    float A[9];        // K_s R_rel K_r^-1          (H = A - b m^T)
    float b[3];        // K_s t_rel
    float wf, hf;      // (float)width, (float)height
    float wm1, hm1;    // (float)(width-1), (float)(height-1)
    const float* img;  // fp32 format: w x h float4 quad texels (see SrcTex) or null
    int pitch;         // texels per row (= w)
    const uint32_t* img8;  // quad-packed u8 texture (see SrcTex8) or null
    int pitch8;            // dwords per row of the quad-packed texture (= w)
    int w, h;
    const float* depth;  // dense source depth map (geometric consistency) or null
    int dw, dh;
    float dwm1, dhm1;
    // geometric consistency (ref .cu:582-640) as two composed projective maps, evaluated on the host in double and rounded
    // once: reference pixel (x, y) at depth z -> source pixel  ~  z * Gf (x, y, 1)^T + gf,
    // source pixel (u, v) at depth d -> reference pixel  ~  d * Gb (u, v, 1)^T + gb
    float Gf[9], gf[3], Gb[9], gb[3];
};

struct ProblemDev {
    CamDev cam;          // reference camera
    float ifx, ify;      // 1/fx, 1/fy        (rounded from double)
    float cxfx, cyfy;    // cx/fx, cy/fy      (rounded from double)
    float fxfy;          // K[0] / K[4]       (fp32 division, as ref .cu:86 does per call)
    int W, H, V;
    const float* ref_img;  // texel (0,0) of the reference image, apron kRefApron
    int ref_pitch;
    ViewDev views[kMaxViews];
};

struct StateDev {
    float4* planes;
    float* costs;
    uint32_t* sel;
    float* geom;
    const float4* prior;
    const uint32_t* mask;
    float* depth;  // dense copy of planes[].w after GetDepthandNormal: what the median filter gathers (4 instead of 16 bytes per tap)
    // photometric cost of every pixel's stored plane against every view as InitializeScore evaluated it, view-major (own[v * W*H + idx],
    // V planes): the first update pass of either colour reads it back instead of evaluating the plane again (pm_kernels.hpp, update_body)
    float* own;
#ifdef PM_DBG_WAVETIME
    unsigned long long* wavetime;  // measurement builds: per-wave start / end stamps of the update launches (pm_kernels.hpp, WaveTimer)
#endif
};

// ---------------------------------------------------------------------------
// canonical math
// ---------------------------------------------------------------------------
// Reciprocal: the hardware seed (v_rcp_f32, 1 ulp) and two Newton steps in fma arithmetic.  tools/verify_rcp.hip checks all
// 2^32 inputs on the MI355X: for every z with z and 1 / z normal (|z| in [2^-126, 2^126]) the result is the correctly rounded
// IEEE quotient 1.0f / z bit for bit -- which is what the CPU oracle computes; 2^126 < |z| < inf gives a zero with the sign of
// z (the seed's denormal result is flushed); zero, denormal, infinite and NaN inputs give NaN.  Five instructions instead of the
// eleven of round 1's magic-constant seed + three Newton steps (3.22 -> 3.17 ms per update launch).
PM_DEV float d_rcp(float z) {
    float r = __builtin_amdgcn_rcpf(z);
    r = __builtin_fmaf(r, __builtin_fmaf(-z, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-z, r, 1.0f), r);
    return r;
}

// The six perspective divides of a window column share one reciprocal r of the PRODUCT of their depths.
// For near-degenerate planes (|n . view ray| ~ 1e-6, plane offset ~ 0) that product over- or underflows and the warp would
// silently collapse onto texel (0, 0).  d_rcp maps an infinite, NaN, zero or denormal product to NaN, so the SUM of the six
// column reciprocals is finite exactly when every column had a usable one (a product beyond 2^126 gives reciprocal 0: a
// finite, if useless, warp -- the same on both sides); an evaluation
// whose sum is not finite returns the sentinel cost 2.  Six full-rate adds and one v_cmp_class_f32 per evaluation
// (measured on the update kernel: 1.4 % of its time; a class test per column cost 1.8 %).
PM_DEV bool rcp_sum_not_finite(float racc) {
    return __builtin_amdgcn_class(racc, 0x207);  // sNaN qNaN -inf +inf
}

// d_exp for arguments known to lie in [-80, 80] (no NaN): the same value, without the range tests
PM_DEV float d_exp_inrange(float x) {
    const float n = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, r * r, r) + 1.0f;
    return __uint_as_float(__float_as_uint(y) + ((uint32_t)(int)n << 23));
}

// correctly rounded sqrt for x = 0 or normal x well inside the exponent range (no scaling, no inf/NaN
// handling): the hardware estimate is within 1 ulp; the residuals of its two neighbours decide
PM_DEV float d_sqrt_normal(float x) {
    float s;
    asm("v_sqrt_f32 %0, %1" : "=v"(s) : "v"(x));
    const float lo = __uint_as_float(__float_as_uint(s) - 1u), hi = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_lo = __builtin_fmaf(-lo, s, x), r_hi = __builtin_fmaf(-hi, s, x);
    s = r_lo <= 0.0f ? lo : s;
    s = r_hi > 0.0f ? hi : s;
    return s;
}

PM_DEV float d_exp(float x) {
    if (x < -80.0f) return 0.0f;
    if (x > 80.0f) return __uint_as_float(0x7f800000u);
    const float n = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, r * r, r) + 1.0f;
    if (!(x == x)) return y;
    const int ni = (int)n;
    return __uint_as_float(__float_as_uint(y) + ((uint32_t)ni << 23));
}

// d_exp without branches (the same value for every input): the window prologue calls it 36 times per pixel, and the three
// exec-mask branches of d_exp cost more there than the polynomial
PM_DEV float d_exp_select(float x) {
    const float n = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, r * r, r) + 1.0f;
    // n as an integer: only meaningful (and only used) for x in [-80, 80]; clamped first so that the conversion is defined
    const int ni = (int)__builtin_amdgcn_fmed3f(n, -128.0f, 128.0f);
    float e = __uint_as_float(__float_as_uint(y) + ((uint32_t)ni << 23));
    e = (x == x) ? e : y;  // NaN propagates through y
    e = (x > 80.0f) ? __uint_as_float(0x7f800000u) : e;
    e = (x < -80.0f) ? 0.0f : e;
    return e;
}

PM_DEV float d_sin(float a) {
    const float z = a * a;
    float p = -1.9515295891e-4f;
    p = __builtin_fmaf(p, z, 8.3321608736e-3f);
    p = __builtin_fmaf(p, z, -1.6666654611e-1f);
    return __builtin_fmaf(p * z, a, a);
}

PM_DEV float d_cos(float a) {
    const float z = a * a;
    float p = 2.443315711809948e-5f;
    p = __builtin_fmaf(p, z, -1.388731625493765e-3f);
    p = __builtin_fmaf(p, z, 4.166664568298827e-2f);
    return __builtin_fmaf(p * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
}

PM_DEV float d_asin_core(float x) {
    const float z = x * x;
    float p = 4.2163199048e-2f;
    p = __builtin_fmaf(p, z, 2.4181311049e-2f);
    p = __builtin_fmaf(p, z, 4.5470025998e-2f);
    p = __builtin_fmaf(p, z, 7.4953002686e-2f);
    p = __builtin_fmaf(p, z, 1.6666752422e-1f);
    return __builtin_fmaf(p * z, x, x);
}

PM_DEV float d_acos(float x) {
    if (!(x >= -1.0f && x <= 1.0f)) return __uint_as_float(0x7fc00000u);
    if (x > 0.5f) return 2.0f * d_asin_core(__builtin_sqrtf(0.5f * (1.0f - x)));
    if (x < -0.5f) return 3.14159265358979323846f - 2.0f * d_asin_core(__builtin_sqrtf(0.5f * (1.0f + x)));
    return 1.57079632679489661923f - d_asin_core(x);
}

// ---------------------------------------------------------------------------
// Philox4x32-10, counter = (pixel, launch, block, tag); replaces the 48-byte
// per-pixel cuRAND XORWOW state (ref .cu:546, include/PatchMatch.h:107): the
// stream position lives in a register, nothing is stored per pixel.
// ---------------------------------------------------------------------------
struct Rng {
    uint32_t key0, key1, pix, launch, k;
    uint32_t b0, b1, b2, b3;
};

PM_DEV void philox_refill(Rng& g) {
    uint32_t c0 = g.pix, c1 = g.launch, c2 = g.k >> 2, c3 = 0x4D504D56u;
    uint32_t k0 = g.key0, k1 = g.key1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0;
        const uint32_t n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    g.b0 = c0; g.b1 = c1; g.b2 = c2; g.b3 = c3;
}

PM_DEV Rng rng_make(uint64_t seed, uint32_t pix, uint32_t launch) {
    Rng g;
    g.key0 = (uint32_t)seed;
    g.key1 = (uint32_t)(seed >> 32);
    g.pix = pix;
    g.launch = launch;
    g.k = 0;
    g.b0 = g.b1 = g.b2 = g.b3 = 0;
    return g;
}

// uniform in (0, 1]: ((x >> 8) + 1) * 2^-24
PM_DEV float rng_uniform(Rng& g) {
    const uint32_t lane = g.k & 3u;
    if (lane == 0u) philox_refill(g);
    const uint32_t x = lane == 0u ? g.b0 : (lane == 1u ? g.b1 : (lane == 2u ? g.b2 : g.b3));
    g.k++;
    return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f;
}

// ---------------------------------------------------------------------------
// geometry helpers
// ---------------------------------------------------------------------------
// ref .cu:84-87
PM_DEV float depth_from_plane(const ProblemDev& P, const float4 pl, int px, int py) {
    const float den = ((float)px - P.cam.K[2]) * pl.x + (P.fxfy * ((float)py - P.cam.K[5])) * pl.y + P.cam.K[0] * pl.z;
    return (-pl.w * P.cam.K[0]) / den;
}
// same for an arbitrary camera (geometric consistency needs only the reference one)
// ref .cu:163-176
PM_DEV float plane_offset(const ProblemDev& P, int px, int py, float depth, const float4 n) {
    const float X0 = (depth * ((float)px - P.cam.K[2])) / P.cam.K[0];
    const float X1 = (depth * ((float)py - P.cam.K[5])) / P.cam.K[4];
    return -((n.x * X0 + n.y * X1) + n.z * depth);
}
// ref .cu:188-195
PM_DEV void normalize3(float4& n) {
    const float ns = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const float inv = 1.0f / __builtin_sqrtf(ns);
    n.x *= inv;
    n.y *= inv;
    n.z *= inv;
}
// ref .cu:197-219
PM_DEV float4 random_normal(const ProblemDev& P, int px, int py, Rng& g) {
    float q1, q2, s;
    do {
        q1 = 2.0f * rng_uniform(g) - 1.0f;
        q2 = 2.0f * rng_uniform(g) - 1.0f;
        s = q1 * q1 + q2 * q2;
    } while (s >= 1.0f);
    const float sq = __builtin_sqrtf(1.0f - s);
    float4 n;
    n.x = (2.0f * q1) * sq;
    n.y = (2.0f * q2) * sq;
    n.z = 1.0f - 2.0f * s;
    n.w = 0.0f;
    const float v0 = ((float)px - P.cam.K[2]) / P.cam.K[0];
    const float v1 = ((float)py - P.cam.K[5]) / P.cam.K[4];
    const float dp = (n.x * v0 + n.y * v1) + n.z * 1.0f;
    if (dp > 0.0f) {
        n.x = -n.x;
        n.y = -n.y;
        n.z = -n.z;
    }
    normalize3(n);
    return n;
}
// ref .cu:460-495
PM_DEV float4 perturbed_normal(const ProblemDev& P, int px, int py, const float4 normal, Rng& g, float perturbation) {
    const float v0 = ((float)px - P.cam.K[2]) / P.cam.K[0];
    const float v1 = ((float)py - P.cam.K[5]) / P.cam.K[4];
    const float a1 = (rng_uniform(g) - 0.5f) * perturbation;
    const float a2 = (rng_uniform(g) - 0.5f) * perturbation;
    const float a3 = (rng_uniform(g) - 0.5f) * perturbation;
    const float s1 = d_sin(a1), s2 = d_sin(a2), s3 = d_sin(a3);
    const float c1 = d_cos(a1), c2 = d_cos(a2), c3 = d_cos(a3);
    const float R0 = c2 * c3;
    const float R1 = (c3 * s1) * s2 - c1 * s3;
    const float R2 = s1 * s3 + (c1 * c3) * s2;
    const float R3 = c2 * s3;
    const float R4 = c1 * c3 + (s1 * s2) * s3;
    const float R5 = (c1 * s2) * s3 - c3 * s1;
    const float R6 = -s2;
    const float R7 = c2 * s1;
    const float R8 = c1 * c2;
    float4 np;
    np.x = (R0 * normal.x + R1 * normal.y) + R2 * normal.z;
    np.y = (R3 * normal.x + R4 * normal.y) + R5 * normal.z;
    np.z = (R6 * normal.x + R7 * normal.y) + R8 * normal.z;
    np.w = normal.w;
    const float dp = (np.x * v0 + np.y * v1) + np.z * 1.0f;
    if (dp >= 0.0f) return normal;
    normalize3(np);
    return np;
}

// ---------------------------------------------------------------------------
// Reference-window statistics (hypothesis independent; ref .cu:318-323 and the
// reference-image terms of :363-395).  The reference recomputes them for each of
// the 14*V evaluations of a pixel; here they are computed once per pixel and
// launch and parked in LDS:
//   * the block's reference-image tile + halo is staged once into LDS (coalesced rows, read back as the 36 window taps of
//     every pixel) as long as it leaves room for two blocks per CU;
//   * the 36 bilateral weights w and products w*r of a pixel live in a per-thread LDS column of 18 float4 ([tap pair][thread],
//     one conflict-free ds_read_b128 per tap pair), leaving the VGPRs to the gather pipeline of the NCC loop.
// LDS layout (one array): [18 * kBlockThreads float4][tile floats].
// Round 2 tried 4-byte records (w only, w*r recomputed from the tile in every evaluation) so that three blocks fit a CU, both
// for the whole update kernel (squeezed into 168 registers: slower) and for its phase A as a kernel of its own (fits easily:
// exactly as fast as with two waves per SIMD): the third wave buys this workload nothing (profiles/EXPERIMENTS.md, 14 and 22).
// ---------------------------------------------------------------------------
constexpr int kBlockThreads = 256;  // threads per block of the all-pixel NCC kernels (k_init, k_eval_ncc); the update kernel has its own (kUpdThreads)
extern __shared__ float pm_lds[];  // dynamic LDS of the NCC kernels
template <int NT>
constexpr int kLdsWeightFloatsOf = 2 * 36 * NT;  // 18 float4 weight records per thread of an NT-thread block
constexpr int kLdsWeightFloats = kLdsWeightFloatsOf<kBlockThreads>;

struct RefWin {
    // this thread's LDS column, one float4 per pair of vertically adjacent taps
    // (b = 2j, 2j+1 of window column a): (w_even, w_odd, w*r_even, w*r_odd)
    const float4* lw;  // lw[(a * 3 + j) * kBlockThreads]
    float inv_w, mean_r, var_r;
};

// Window geometry of a launch: the scale is a template parameter of the NCC kernels, so step and radius are constants.
// The reference tile (block + halo of the window radius) is staged in LDS only while two blocks still fit a CU's 160 KB next
// to their 72 KB of weight records, i.e. up to 2048 floats.  A larger tile would halve the occupancy of the whole kernel for
// the sake of its prologue (measured 5.96 vs 3.9 ms per launch at scale 2), so the window is then read from the L2-resident
// padded image instead.  With the 8 x 64 pixel blocks of the fp16 texture format that is the case from scale 1 on (28 x 84
// floats), with the 16 x 32 blocks of the fp32 format and the 16 x 16 dense blocks from scale 2 on.
template <int SCALE, int BW, int BH, int TILE_MAX = 2048>
struct Win {
    static constexpr int step = 2 << SCALE, radius = 5 * step / 2, pitch = BW + 2 * radius, rows = BH + 2 * radius;
    static constexpr bool tile_in_lds = pitch * rows <= TILE_MAX;
};

// cooperative load of the tile [x0-radius, x0+BW+radius) x [y0-radius, y0+BH+radius)
// of the apron-padded reference image; columns/rows beyond the apron (only ever
// addressed by threads whose pixel lies outside the image) are clamped
template <int NT>
PM_DEV void load_ref_tile(const ProblemDev& P, float* tile, int x0, int y0, int bw, int bh, int radius) {
    const int tw = bw + 2 * radius, th = bh + 2 * radius;
    const int xmin = -kRefApron, xmax = P.W + kRefApron - 1, ymin = -kRefApron, ymax = P.H + kRefApron - 1;
    for (int i = threadIdx.x; i < tw * th; i += NT) {
        const int ty = i / tw, tx = i - ty * tw;
        int gx = x0 - radius + tx, gy = y0 - radius + ty;
        gx = gx < xmin ? xmin : (gx > xmax ? xmax : gx);
        gy = gy < ymin ? ymin : (gy > ymax ? ymax : gy);
        tile[i] = P.ref_img[(long)gy * P.ref_pitch + gx];
    }
}

// The same tile in two halves, for the update kernel: all loads of a thread go out together and are stored afterwards, where the
// loop above pays one memory round trip per element of a thread (8 in a one-wave block).  N = ceil(tile / NT).
template <int NT, int BW, int BH, int RADIUS, int N>
PM_DEV void load_ref_tile_values(const ProblemDev& P, int x0, int y0, float (&v)[N]) {
    constexpr int tw = BW + 2 * RADIUS, th = BH + 2 * RADIUS;
    static_assert(N * NT >= tw * th, "every tile element has a thread");
    const int xmin = -kRefApron, xmax = P.W + kRefApron - 1, ymin = -kRefApron, ymax = P.H + kRefApron - 1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = min((int)threadIdx.x + k * NT, tw * th - 1);   // (the spare threads of the last round repeat the last element and drop it)
        const int ty = i / tw, tx = i - ty * tw;
        int gx = x0 - RADIUS + tx, gy = y0 - RADIUS + ty;
        gx = gx < xmin ? xmin : (gx > xmax ? xmax : gx);
        gy = gy < ymin ? ymin : (gy > ymax ? ymax : gy);
        v[k] = P.ref_img[(long)gy * P.ref_pitch + gx];
    }
}
template <int NT, int BW, int BH, int RADIUS, int N>
PM_DEV void store_ref_tile_values(float* tile, const float (&v)[N]) {
    constexpr int tw = BW + 2 * RADIUS, th = BH + 2 * RADIUS;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int i = (int)threadIdx.x + k * NT;
        if (i < tw * th) tile[i] = v[k];
    }
}

// weights of one pixel -> LDS column `lw`.  tap(dx, dy) reads the reference image at the pixel + (dx, dy): from the block's
// LDS tile, or from the apron-padded image in global memory (see Win).
template <int SCALE, int NT, class TAP>
PM_DEV void ref_window(float4* lw, TAP tap, const float (&spatial)[36], float two_sc, RefWin& rw) {
    constexpr int step = 2 << SCALE, radius = 5 * step / 2;
    // all 37 reference values first, in straight-line code: read inside the weight loop below, every tap waited for its own LDS /
    // memory round trip (14 separate waits at scale 2, where the window comes from global memory)
    const float rc = tap(0, 0);
    float rv[36];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) rv[a * 6 + b] = tap(a * step - radius, b * step - radius);
    float sw = 0.0f, swr = 0.0f, swrr = 0.0f;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        float pw = 0.0f, pwr = 0.0f, pwrr = 0.0f;
        float wv[6], wrv[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const float r = rv[a * 6 + b];
            const float e = spatial[a * 6 + b] - __builtin_fabsf(r - rc) / two_sc;  // ref .cu:318-323
            const float w = d_exp_select(e);
            const float wr = w * r;
            wv[b] = w;
            wrv[b] = wr;
            pw += w;
            pwr += wr;
            pwrr = __builtin_fmaf(wr, r, pwrr);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) lw[(a * 3 + j) * NT] = make_float4(wv[2 * j], wv[2 * j + 1], wrv[2 * j], wrv[2 * j + 1]);
        sw += pw;
        swr += pwr;
        swrr += pwrr;
    }
    rw.lw = lw;
    rw.inv_w = 1.0f / sw;
    rw.mean_r = swr * rw.inv_w;
    const float mrr = swrr * rw.inv_w;
    rw.var_r = __builtin_fmaf(-rw.mean_r, rw.mean_r, mrr);
}

// fills the pixel's weight column from the block's staged reference tile (Win::tile_in_lds: the tile is in LDS behind a barrier) or,
// where the tile is not staged, from the apron-padded image
template <int SCALE, int BW, int BH, int NT = kBlockThreads, int TILE_MAX = 2048>
PM_DEV void ref_window_at_pixel(const ProblemDev& P, int x, int y, int x0, int y0, const float (&spatial)[36], float two_sc, RefWin& rw) {
    typedef Win<SCALE, BW, BH, TILE_MAX> Wn;
    float4* lw = (float4*)pm_lds + threadIdx.x;
    if constexpr (Wn::tile_in_lds) {
        const int ctr = kLdsWeightFloatsOf<NT> + (y - y0 + Wn::radius) * Wn::pitch + (x - x0 + Wn::radius);
        ref_window<SCALE, NT>(lw, [&](int dx, int dy) { return pm_lds[ctr + dy * Wn::pitch + dx]; }, spatial, two_sc, rw);
    } else {
        const float* ctr = P.ref_img + (long)y * P.ref_pitch + x;
        const int pitch = P.ref_pitch;
        ref_window<SCALE, NT>(lw, [&](int dx, int dy) { return ctr[dy * pitch + dx]; }, spatial, two_sc, rw);
    }
}

// stages the block's reference tile if it is to live in LDS and fills the pixel's weight column
template <int SCALE, int BW, int BH, int NT = kBlockThreads, int TILE_MAX = 2048>
PM_DEV void ref_window_of_pixel(const ProblemDev& P, int x, int y, int x0, int y0, bool valid, const float (&spatial)[36], float two_sc, RefWin& rw) {
    typedef Win<SCALE, BW, BH, TILE_MAX> Wn;
    if constexpr (Wn::tile_in_lds) {
        load_ref_tile<NT>(P, pm_lds + kLdsWeightFloatsOf<NT>, x0, y0, BW, BH, Wn::radius);
        __syncthreads();
    }
    if (!valid) return;
    ref_window_at_pixel<SCALE, BW, BH, NT, TILE_MAX>(P, x, y, x0, y0, spatial, two_sc, rw);
}

// the tap-pair arithmetic is written on float2 vectors (v_pk_fma/mul_f32)
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Clamp a sample coordinate to [0, hi] (hi = size - 1); NaN -> 0 (v_med3_f32 returns
// min3 when an input is NaN).  The canonical rule is clamp addressing of the
// TEXELS: below 0 both texels of the pair are texel 0 and above
// hi both are texel hi, so the interpolated value does not depend on the fraction
// there and clamping the coordinate itself gives the same bits -- with no apron
// and non-negative texel indices.  (Without the clamp an update pass is 2.4 % faster; a proof that a window is interior and a
// second tap loop for the others would keep at best 1 % of that: profiles/EXPERIMENTS.md 42.)
PM_DEV float clamp_coord(float s, float hi) { return __builtin_amdgcn_fmed3f(s, 0.0f, hi); }

// floor + float->int in one instruction (hipcc only selects it under fast-math)
PM_DEV int floor_to_int(float c) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(c));
    return r;
}
// byte k of a packed dword as fp32 (kept as explicit instructions: left to itself hipcc subtracts the bytes as integers
// first, through slower SDWA forms); used by the sky kernel
template <int K>
PM_DEV float ubyte_to_float(uint32_t q) {
    float f;
    if constexpr (K == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(q));
    if constexpr (K == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(q));
    if constexpr (K == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(q));
    if constexpr (K == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(q));
    return f;
}

// index of texel (ix, iy) in its texture.  PM_DBG_ADDRMASK (measurement builds only, results are wrong): all gathers of a wave
// fall into a few cache lines, which takes the texture path (TA / L1 / TD) out of the picture while the instruction stream
// stays the same
template <class TEX>
PM_DEV int texel_index(const TEX& t, int iy, int ix) {
    unsigned idx = __umul24((unsigned)iy, (unsigned)t.pitch) + (unsigned)ix;  // v_mad_u32_u24
#ifdef PM_DBG_ADDRMASK
    idx &= (unsigned)(PM_DBG_ADDRMASK);
#endif
    return (int)idx;
}

// Source textures ("quad-difference" texels).  Texel (x, y) of a view packs the whole bilinear footprint of the image P
// (indices clamped to the image) as the coefficients of the bilinear polynomial t00 + ax dx + ay (dy + ax dxy):
//     t00 = P[y][x],  dx = P[y][x+1] - t00,  dy = P[y+1][x] - t00,  dxy = (P[y+1][x+1] - P[y+1][x]) - dx
// so that ONE gather serves a tap and the interpolation is three fmas with no unpacking
//     top = fma(ax, dx, t00);  ver = fma(ax, dxy, dy);  value = fma(ay, ver, top)
//   * fp32 format (any image): four floats, 16 bytes, one buffer_load_dwordx4.  The differences are the fp32 differences the
//     canonical arithmetic defines, rounded once when the texture is packed instead of once per tap.
//   * fp16 format (every pixel of every source image an integer in [0, 255]: always true for the reference's input unless
//     it rescales, imread(GRAYSCALE) -> convertTo(CV_32F), ref .cpp:877-882): four halfs, 8 bytes, one
//     buffer_load_dwordx2; dword 0 = (t00, dy), dword 1 = (dx, dxy).  Integers up to 255 and these differences (|.| <= 510)
//     are exact in fp16, v_fma_mix_f32 reads the half operands directly and rounds once in fp32: identical bits to the fp32 format.
// The 128-bit buffer resource is wave-uniform (built from scalar loads); the texel index is range checked by the hardware
// (an out-of-range index -- impossible, the coordinate is clamped first -- would read 0 instead of faulting).
// The gather addresses a texel by its INDEX (buffer_load ... idxen, the descriptor carries the texel size as its stride),
// so the address is one v_mad_u32_u24 instead of a 24-bit multiply and a shift-add (-1.2 % on k_update).  The descriptor is written out as four dwords because the indexed load is reached through
// its LLVM intrinsic (hipcc has no builtin for it); an index beyond `texels` reads 0 (cannot happen: clamped coordinates).
typedef int i32x4q __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2q __attribute__((ext_vector_type(2)));
typedef float f32x4q __attribute__((ext_vector_type(4)));
__device__ u32x2q pm_struct_load_b64(i32x4q rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.v2i32");
__device__ f32x4q pm_struct_load_f128(i32x4q rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.v4f32");
PM_DEV i32x4q make_indexed_rsrc(const void* base, int texel_bytes, int texels) {
    const unsigned long long a = (unsigned long long)base;
    return (i32x4q){(int)(unsigned)a, (int)(((unsigned)(a >> 32) & 0xffffu) | ((unsigned)texel_bytes << 16)), texels, 0x00020000};
}

struct SrcTex {
    i32x4q irsrc;
    int pitch;  // texels per row (= w)
    float wm1, hm1;
};

PM_DEV SrcTex make_src_tex(const ViewDev& vw) {
    SrcTex t;
    t.pitch = vw.pitch;
    t.wm1 = vw.wm1;
    t.hm1 = vw.hm1;
    t.irsrc = make_indexed_rsrc(vw.img, 16, vw.pitch * vw.h);
    return t;
}

struct SrcTex8 {
    i32x4q irsrc;
    int pitch;  // texels per row (= w)
    float wm1, hm1;
};

PM_DEV SrcTex8 make_src_tex8(const ViewDev& vw) {
    SrcTex8 t;
    t.pitch = vw.pitch8;
    t.wm1 = vw.wm1;
    t.hm1 = vw.hm1;
    t.irsrc = make_indexed_rsrc(vw.img8, 8, vw.pitch8 * vw.h);
    return t;
}

// Opt-in build -DPM_TEX_Q8 (libmpmvs_hip_q8.so): the interpolation fractions are quantised to 8 bits the way CUDA's texture unit does
// it (frac = floor(a * 256 + 0.5) / 256; CUDA C Programming Guide, "Linear Filtering": 9-bit fixed point with 8 bits of fraction) --
// what the reference's tex2D fetches apply on its hardware (ref .cu:377).  The default build keeps exact fp32 fractions: against the
// reference's FORMULAS it is within north_star's 1e-3, against formulas + this quantisation the tail reaches 1.9e-3;
// the q8 build closes that last digit for +6 instructions per tap.
#ifdef PM_TEX_Q8
PM_DEV float tex_fraction(float a) { return __builtin_floorf(__builtin_fmaf(a, 256.0f, 0.5f)) * 0.00390625f; }
#else
PM_DEV float tex_fraction(float a) { return a; }
#endif

// Bilinear tap in two halves: issue() clamps the coordinate, computes the address and starts the load; value()
// interpolates (ref .cu:377: tex2D(t, x+0.5, y+0.5) with the linear filter, software here: SURVEY a-2).  Lets a whole
// window column be in flight at once.
template <bool U8>
struct BilinearTap;

template <>
struct BilinearTap<false> {
    float ax, ay;
    f32x4q q;  // (t00, dx, dy, dxy)
    template <class TEX>
    PM_DEV void issue(const TEX& t, float sx, float sy) {
        const float cx = clamp_coord(sx, t.wm1);
        const float cy = clamp_coord(sy, t.hm1);
        ax = tex_fraction(__builtin_amdgcn_fractf(cx));  // v_fract_f32: x - floor(x), kept below 1
        ay = tex_fraction(__builtin_amdgcn_fractf(cy));
        const int idx = texel_index(t, floor_to_int(cy), floor_to_int(cx));
#ifdef PM_DBG_NOLOAD  // measurement builds only (results are wrong): the instruction stream without its gathers
        q = (f32x4q){(float)idx, 1.0f, ax, ay};
#else
        q = pm_struct_load_f128(t.irsrc, idx, 0, 0, 0);
#endif
    }
    PM_DEV float value() const {
        const float top = __builtin_fmaf(ax, q.y, q.x);  // value on the upper row
        const float ver = __builtin_fmaf(ax, q.w, q.z);  // lower row minus upper row
        return __builtin_fmaf(ay, ver, top);
    }
};
template <>
struct BilinearTap<true> {
    float ax, ay;
    u32x2q q;  // halfs: (t00, dy), (dx, dxy)
    template <class TEX>
    PM_DEV void issue(const TEX& t, float sx, float sy) {
        const float cx = clamp_coord(sx, t.wm1);
        const float cy = clamp_coord(sy, t.hm1);
        ax = tex_fraction(__builtin_amdgcn_fractf(cx));
        ay = tex_fraction(__builtin_amdgcn_fractf(cy));
        [[maybe_unused]] const int idx = texel_index(t, floor_to_int(cy), floor_to_int(cx));
#ifdef PM_DBG_NOLOAD  // measurement builds only (results are wrong): the instruction stream without its gathers
        q = (u32x2q){(uint32_t)idx, (uint32_t)idx};
#elif defined(PM_DBG_LDSTEX)
        // measurement builds only (results are wrong): what a tile-resident texel would cost per tap -- tile-relative coordinates
        // (two subtractions), the out-of-tile accumulator (two ORs), a byte address (one multiply-add and one shift; the shift is an
        // SDWA form that also keeps the low byte only, so that the read stays inside the 2 KB it may touch without a mask instruction
        // the real tile path would not have) and an 8-byte LDS read.  The texels come from the exchange area of the one-wave update
        // block (PM_DBG_LDSTEX = its offset in floats: kLdsWeightFloatsOf<64>), 256 of them at a pitch of 17 (odd: rows spread over
        // the banks) -- no tile loads, no barriers, no fallback for taps outside the tile: a LOWER bound on the tile path's time.
        {
            const float rx = cx - 16.0f, ry = cy - 8.0f;
            int irx = floor_to_int(rx), iry = floor_to_int(ry);
            asm volatile("v_or_b32 %0, %0, %1\n\tv_or_b32 %1, %1, %0" : "+v"(irx), "+v"(iry));  // stands in for the two accumulator ORs
            const unsigned ti = __umul24((unsigned)iry, 17u) + (unsigned)irx;
            unsigned a;
            asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(a) : "s"(3), "v"(ti));
            q = *reinterpret_cast<const u32x2q*>(reinterpret_cast<const char*>(pm_lds + (PM_DBG_LDSTEX)) + a);
        }
#else
        q = pm_struct_load_b64(t.irsrc, idx, 0, 0, 0);
#endif
    }
    PM_DEV float value() const {
        // fma(ax, (float)d0, (float)t00) and the same on the high halves, the fp16 operands read in place (hipcc does not form
        // v_fma_mix_f32 from the fpext + fma pattern here)
        float top, ver;
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(top) : "v"(ax), "v"(q.y), "v"(q.x));
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,1] op_sel_hi:[0,1,1]" : "=v"(ver) : "v"(ax), "v"(q.y), "v"(q.x));
        return __builtin_fmaf(ay, ver, top);
    }
};

// plane -> m = (n^T K_r^-1) / d, shared by all views of one hypothesis
PM_DEV void plane_to_m(const ProblemDev& P, const float4 pl, float& m0, float& m1, float& m2) {
    const float inv_d = 1.0f / pl.w;
    m0 = (pl.x * P.ifx) * inv_d;
    m1 = (pl.y * P.ify) * inv_d;
    m2 = __builtin_fmaf(-pl.y, P.cyfy, __builtin_fmaf(-pl.x, P.cxfx, pl.z)) * inv_d;
}

// ref .cu:325-414 ComputeBilateralNCC for one (hypothesis, source view), given the homography H = A - b m^T of the
// pair, the texture handle of the view (wave-uniform SrcTex / SrcTex8) and the LDS weight records of the pixel
// (rw.lw[rec * LWSTRIDE]).
template <bool U8, int LWSTRIDE, int SCALE, bool DEEP, class TEX>
PM_DEV float ncc_core(const TEX& tex, float wf, float hf, float H0, float H1, float H2, float H3, float H4, float H5, float H6, float H7, float H8,
                      const RefWin& rw, int px, int py) {
    constexpr int step = 2 << SCALE, radius = 5 * step / 2;
    const float fpx = (float)px, fpy = (float)py;
    {
        const float X = __builtin_fmaf(H1, fpy, __builtin_fmaf(H0, fpx, H2));
        const float Y = __builtin_fmaf(H4, fpy, __builtin_fmaf(H3, fpx, H5));
        const float Z = __builtin_fmaf(H7, fpy, __builtin_fmaf(H6, fpx, H8));
        const float rz = d_rcp(Z);
        const float cx = X * rz, cy = Y * rz;
        if (!(cx >= 0.0f && cx < wf && cy >= 0.0f && cy < hf)) return 2.0f;  // ref .cu:351-353
    }
    float racc = 0.0f;  // sum of the six column reciprocals: not finite = some column had no usable reciprocal
    const f32x2 h1 = {H1, H1}, h4 = {H4, H4}, h7 = {H7, H7};

    // phase 1 of window column a: warp its 6 taps as 3 packed pairs, share ONE
    // reciprocal between the six perspective divides, compute the
    // addresses and issue all gathers of the column back to back
    auto issue_column = [&](int a, BilinearTap<U8>(&tap)[6]) {
        const float tx = (float)(px + a * step - radius);
        const float Cx = __builtin_fmaf(H0, tx, H2);
        const float Cy = __builtin_fmaf(H3, tx, H5);
        const float Cz = __builtin_fmaf(H6, tx, H8);
        const f32x2 cx2 = {Cx, Cx}, cy2 = {Cy, Cy}, cz2 = {Cz, Cz};
        f32x2 XP[3], YP[3], ZP[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const f32x2 ty = {(float)(py + (2 * j) * step - radius), (float)(py + (2 * j + 1) * step - radius)};
            XP[j] = __builtin_elementwise_fma(h1, ty, cx2);
            YP[j] = __builtin_elementwise_fma(h4, ty, cy2);
            ZP[j] = __builtin_elementwise_fma(h7, ty, cz2);
        }
        const float q0 = ZP[0].x * ZP[0].y, q1 = ZP[1].x * ZP[1].y, q2 = ZP[2].x * ZP[2].y;
        const float t = q0 * q1, u = q1 * q2, v = q0 * q2;
        const float r = d_rcp(t * q2);
        racc += r;
        const float iq[3] = {r * u, r * v, r * t};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const f32x2 zs = {ZP[j].y, ZP[j].x};
            const f32x2 inv = (f32x2){iq[j], iq[j]} * zs;
            const f32x2 sx = XP[j] * inv, sy = YP[j] * inv;
            tap[2 * j].issue(tex, sx.x, sy.x);
            tap[2 * j + 1].issue(tex, sx.y, sy.y);
        }
    };
    // phase 2: interpolate; the even taps (b = 0, 2, 4) and the odd taps of ALL columns accumulate in the two halves of packed
    // registers and meet once, at the end of the window
    f32x2 A1 = {0.0f, 0.0f}, A2 = {0.0f, 0.0f}, A3 = {0.0f, 0.0f};
    auto consume_column = [&](const float4 (&wq)[3], const BilinearTap<U8>(&tap)[6]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const f32x2 sv = {tap[2 * j].value(), tap[2 * j + 1].value()};
            const f32x2 w2 = {wq[j].x, wq[j].y}, wr2 = {wq[j].z, wq[j].w};
            const f32x2 ws = w2 * sv;
            A1 = __builtin_elementwise_fma(w2, sv, A1);
            A2 = __builtin_elementwise_fma(ws, sv, A2);
            A3 = __builtin_elementwise_fma(wr2, sv, A3);
        }
        // A3 is only consumed after the variance test at the end, so the compiler would SINK its whole accumulation behind that
        // branch: keep all 36 interpolated values alive in registers and re-read the weight records from LDS there.  Pin it
        // to the column it belongs to.
        asm volatile("" : "+v"(A3));
    };
    // software pipeline over the 6 columns: the gathers of column a+1 are in flight
    // while column a is interpolated, so a wave never drains its loads; the LDS
    // weight records of a column are fetched one column ahead for the same reason
    auto load_weights = [&](int a, float4(&wq)[3]) {
#pragma unroll
        for (int j = 0; j < 3; ++j) wq[j] = rw.lw[(a * 3 + j) * LWSTRIDE];
    };
    // DEEP: the gathers of TWO columns ahead are in flight (12 .. 18 loads; fp16 texels 3.26 -> 3.22 ms per update launch).  A
    // column of fp32 texels takes 24 registers, so the callers ask for it only where the kernel around it has them to spare.
    if constexpr (DEEP) {
        BilinearTap<U8> tapA[6], tapB[6], tapC[6];
        float4 wA[3], wB[3];
        load_weights(0, wA);
        issue_column(0, tapA);
        issue_column(1, tapB);
        issue_column(2, tapC);
        load_weights(1, wB);
        consume_column(wA, tapA);
        issue_column(3, tapA);
        load_weights(2, wA);
        consume_column(wB, tapB);
        issue_column(4, tapB);
        load_weights(3, wB);
        consume_column(wA, tapC);
        issue_column(5, tapC);
        load_weights(4, wA);
        consume_column(wB, tapA);
        load_weights(5, wB);
        consume_column(wA, tapB);
        consume_column(wB, tapC);
    } else {
        BilinearTap<U8> tapA[6], tapB[6];
        float4 wA[3], wB[3];
        load_weights(0, wA);
        issue_column(0, tapA);
#pragma unroll
        for (int a = 0; a < 6; a += 2) {
            issue_column(a + 1, tapB);
            load_weights(a + 1, wB);
            consume_column(wA, tapA);
            if (a + 2 < 6) {
                issue_column(a + 2, tapA);
                load_weights(a + 2, wA);
            }
            consume_column(wB, tapB);
        }
    }
    const float T1 = A1.x + A1.y, T2 = A2.x + A2.y, T3 = A3.x + A3.y;
    if (rcp_sum_not_finite(racc)) return 2.0f;  // no usable warp (plane through the camera centre)
    const float ms = T1 * rw.inv_w, mss = T2 * rw.inv_w, mrs = T3 * rw.inv_w;
    const float var_s = __builtin_fmaf(-ms, ms, mss);
    if (rw.var_r < 1e-5f || var_s < 1e-5f) return 2.0f;  // ref .cu:406-408
    const float cov = __builtin_fmaf(-rw.mean_r, ms, mrs);
    const float den = d_sqrt_normal(rw.var_r * var_s);  // both factors >= 1e-5: correctly rounded without the range handling of sqrtf
    float cost = 1.0f - cov / den;
    cost = (cost < 2.0f) ? cost : 2.0f;  // ref .cu:412
    cost = (cost > 0.0f) ? cost : 0.0f;
    return cost;
}

// one-thread-per-pixel kernels: wave-uniform source view (constants through the scalar cache)
template <bool U8, int SCALE, bool DEEP = U8, int NT = kBlockThreads>
PM_DEV float ncc_cost(const ViewDev& vw, const RefWin& rw, int px, int py, float m0, float m1, float m2) {
    const float H0 = __builtin_fmaf(-vw.b[0], m0, vw.A[0]);
    const float H1 = __builtin_fmaf(-vw.b[0], m1, vw.A[1]);
    const float H2 = __builtin_fmaf(-vw.b[0], m2, vw.A[2]);
    const float H3 = __builtin_fmaf(-vw.b[1], m0, vw.A[3]);
    const float H4 = __builtin_fmaf(-vw.b[1], m1, vw.A[4]);
    const float H5 = __builtin_fmaf(-vw.b[1], m2, vw.A[5]);
    const float H6 = __builtin_fmaf(-vw.b[2], m0, vw.A[6]);
    const float H7 = __builtin_fmaf(-vw.b[2], m1, vw.A[7]);
    const float H8 = __builtin_fmaf(-vw.b[2], m2, vw.A[8]);
    const auto tex = [&] {
        if constexpr (U8)
            return make_src_tex8(vw);
        else
            return make_src_tex(vw);
    }();
    return ncc_core<U8, NT, SCALE, DEEP>(tex, vw.wf, vw.hf, H0, H1, H2, H3, H4, H5, H6, H7, H8, rw, px, py);
}

// ---------------------------------------------------------------------------
// geometric consistency (ref .cu:582-640)
// ---------------------------------------------------------------------------
// BackProjectPoint2W / ProjectPoint in the reference's own operation order (ref .cu:582-615): used by depth-map fusion (pm_fusion.hpp)
PM_DEV void backproject(const CamDev& cam, float x, float y, float depth, float& o0, float& o1, float& o2) {
    const float X0 = (depth * (x - cam.K[2])) / cam.K[0];
    const float X1 = (depth * (y - cam.K[5])) / cam.K[4];
    const float X2 = depth;
    const float t0 = (cam.R[0] * X0 + cam.R[3] * X1) + cam.R[6] * X2;
    const float t1 = (cam.R[1] * X0 + cam.R[4] * X1) + cam.R[7] * X2;
    const float t2 = (cam.R[2] * X0 + cam.R[5] * X1) + cam.R[8] * X2;
    o0 = t0 + cam.C[0];
    o1 = t1 + cam.C[1];
    o2 = t2 + cam.C[2];
}
PM_DEV void project(const CamDev& cam, float p0, float p1, float p2, float& u, float& v) {
    const float t0 = ((cam.R[0] * p0 + cam.R[1] * p1) + cam.R[2] * p2) + cam.t[0];
    const float t1 = ((cam.R[3] * p0 + cam.R[4] * p1) + cam.R[5] * p2) + cam.t[1];
    const float t2 = ((cam.R[6] * p0 + cam.R[7] * p1) + cam.R[8] * p2) + cam.t[2];
    const float d = (cam.K[6] * t0 + cam.K[7] * t1) + cam.K[8] * t2;
    u = ((cam.K[0] * t0 + cam.K[1] * t1) + cam.K[2] * t2) / d;
    v = ((cam.K[3] * t0 + cam.K[4] * t1) + cam.K[5] * t2) / d;
}
// reference src/PatchMatch.cpp:251-261: the projection of the fusion (pm_fusion.hpp), of the depth render (pm_render.hpp) and of the
// observer.  Host code too: the render passes are replayed on the host through it.
__host__ PM_DEV void project_depth(const CamDev& cam, float p0, float p1, float p2, float& u, float& v, float& depth) {
    const float t0 = ((cam.R[0] * p0 + cam.R[1] * p1) + cam.R[2] * p2) + cam.t[0];
    const float t1 = ((cam.R[3] * p0 + cam.R[4] * p1) + cam.R[5] * p2) + cam.t[1];
    const float t2 = ((cam.R[6] * p0 + cam.R[7] * p1) + cam.R[8] * p2) + cam.t[2];
    depth = (cam.K[6] * t0 + cam.K[7] * t1) + cam.K[8] * t2;
    u = ((cam.K[0] * t0 + cam.K[1] * t1) + cam.K[2] * t2) / depth;
    v = ((cam.K[3] * t0 + cam.K[4] * t1) + cam.K[5] * t2) / depth;
}
// ComputeGeomConsistencyCost: forward-project the pixel at the hypothesis' depth into the source view, read the source depth
// there (nearest texel, clamp), back-project and re-project into the reference view, cost = min(3, reprojection distance).
// The reference walks through world coordinates with 9 divisions per check (BackProjectPoint2W, ProjectPoint twice each way);
// here each direction is ONE projective map with host-composed constants (ViewDev::Gf/gf/Gb/gb): 9 + 9 fmas, two shared
// reciprocals, no division -- ~60 instructions per check instead of ~290 (round 4; DESIGN.md 3.8 measures the distance of this
// canonical form from the literal formulas).  The depth of the hypothesis at the pixel is view independent: computed once per
// hypothesis by the caller (depth_from_plane).
// The check in two halves, so that callers can put other work (or the first halves of other checks) between the depth gather
// and its use: issue() projects forward and starts the load, finish() projects back.  A check issued and finished back to back
// exposes the full latency of its gather (one scattered 4-byte load): 86 of them per pixel and iteration were 10 % of a wave's
// lifetime.
struct GeomCheck {
    float su, sv, sd;
    PM_DEV void issue(const ViewDev& vw, float z, int px, int py) {
        const float fx = (float)px, fy = (float)py;
        const float q0 = __builtin_fmaf(vw.Gf[1], fy, __builtin_fmaf(vw.Gf[0], fx, vw.Gf[2]));
        const float q1 = __builtin_fmaf(vw.Gf[4], fy, __builtin_fmaf(vw.Gf[3], fx, vw.Gf[5]));
        const float q2 = __builtin_fmaf(vw.Gf[7], fy, __builtin_fmaf(vw.Gf[6], fx, vw.Gf[8]));
        const float h0 = __builtin_fmaf(z, q0, vw.gf[0]);
        const float h1 = __builtin_fmaf(z, q1, vw.gf[1]);
        const float h2 = __builtin_fmaf(z, q2, vw.gf[2]);
        const float rh = d_rcp(h2);
        su = h0 * rh;
        sv = h1 * rh;
        float qx = (su >= 0.0f) ? su : 0.0f;  // NaN -> 0
        qx = (qx <= vw.dwm1) ? qx : vw.dwm1;
        float qy = (sv >= 0.0f) ? sv : 0.0f;
        qy = (qy <= vw.dhm1) ? qy : vw.dhm1;
        sd = vw.depth[(long)(int)qy * vw.dw + (int)qx];  // nearest, ref .cu:626
    }
    PM_DEV float finish(const ViewDev& vw, int px, int py) const {
        if (sd == 0.0f) return 3.0f;
        const float fx = (float)px, fy = (float)py;
        const float p0 = __builtin_fmaf(vw.Gb[1], sv, __builtin_fmaf(vw.Gb[0], su, vw.Gb[2]));
        const float p1 = __builtin_fmaf(vw.Gb[4], sv, __builtin_fmaf(vw.Gb[3], su, vw.Gb[5]));
        const float p2 = __builtin_fmaf(vw.Gb[7], sv, __builtin_fmaf(vw.Gb[6], su, vw.Gb[8]));
        const float k0 = __builtin_fmaf(sd, p0, vw.gb[0]);
        const float k1 = __builtin_fmaf(sd, p1, vw.gb[1]);
        const float k2 = __builtin_fmaf(sd, p2, vw.gb[2]);
        const float rk = d_rcp(k2);
        const float dc = fx - k0 * rk, dr = fy - k1 * rk;
        const float e = __builtin_sqrtf(__builtin_fmaf(dr, dr, dc * dc));
        return (e < 3.0f) ? e : 3.0f;  // NaN -> 3
    }
};
PM_DEV float geom_cost_view_body(const ViewDev& vw, float z, int px, int py) {
    GeomCheck g;
    g.issue(vw, z, px, py);
    return g.finish(vw, px, py);
}
PM_DEV float geom_cost(const ProblemDev& P, const ViewDev& vw, const float4 pl, int px, int py) {
    return geom_cost_view_body(vw, depth_from_plane(P, pl, px, py), px, py);
}

}  // namespace pm
