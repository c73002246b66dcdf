// oracle/ref_shim/cuda_standin.h
//
// TEST INFRASTRUCTURE ONLY.  Host stand-ins for the pieces of CUDA, cuRAND and OpenCV that the reference's DEVICE code names,
// so that its kernels and device functions compile with a host C++ compiler and run one thread at a time (oracle/ref_driver.cpp,
// oracle/Makefile target `ref`).  Nothing here is taken from the reference or from CUDA's headers: the types are the obvious
// PODs, and the texture fetch is written from the definition in the CUDA C++ Programming Guide ("Texture Fetching": linear
// filtering, unnormalised coordinates, clamp addressing).
//
// What a stand-in decides, and why:
//   tex2D        linear filter of the four texels around xB = x - 0.5f, yB = y - 0.5f, formed on the coordinate AS PASSED (the
//                caller's `x + 0.5f` has already been rounded to fp32 when the texture unit sees it); texel indices clamp to the
//                image (the reference asks for wrap addressing, which CUDA honours only with normalised coordinates: DESIGN.md
//                3.4); the fractions optionally keep 8 bits (CUDA's 9-bit fixed point with 8 bits of fraction); the blend is
//                (1-a)(1-b) T00 + a (1-b) T10 + (1-a) b T01 + a b T11 in fp32, left to right.
//   curandState  a cursor into a caller-supplied table of uniforms (one row per pixel): the driver feeds the project's own
//                stream, so the reference's code and the oracle consume the same numbers in the same order.  A pixel that
//                runs past its row raises a flag that the driver turns into an error.
//   rsqrtf       1 / sqrtf (IEEE), min / max on floats = fminf / fmaxf (CUDA's meaning: a NaN operand loses).
//   <math.h>     is included, not only <cmath>: a bare exp(float) / sqrt(float) / acos(float) in the reference's code must pick
//                the float overload as it does under nvcc; the static_asserts below keep that true.
#ifndef MPMVS_REF_SHIM_CUDA_STANDIN_H_
#define MPMVS_REF_SHIM_CUDA_STANDIN_H_

#include <math.h>
#include <stdlib.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "../../include/mpmvs.h"

static_assert(std::is_same<decltype(exp(1.0f)), float>::value, "exp(float) must be the float function");
static_assert(std::is_same<decltype(sqrt(1.0f)), float>::value, "sqrt(float) must be the float function");
static_assert(std::is_same<decltype(acos(1.0f)), float>::value, "acos(float) must be the float function");
static_assert(std::is_same<decltype(sin(1.0f)), float>::value, "sin(float) must be the float function");
static_assert(std::is_same<decltype(cos(1.0f)), float>::value, "cos(float) must be the float function");
static_assert(std::is_same<decltype(fabs(1.0f)), float>::value, "fabs(float) must be the float function");

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline

typedef unsigned char uchar;

// the byte-compatible mirrors of the reference's PODs (include/mpmvs.h)
typedef mpmvs_camera Camera;
typedef mpmvs_params PatchMatchParams;
static_assert(sizeof(Camera) == 112, "Camera must match the reference layout");
static_assert(sizeof(PatchMatchParams) == 56, "PatchMatchParams must match the reference layout");

struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct uint3 { unsigned int x, y, z; };
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
// one host thread plays one CUDA thread at a time; the driver sets these before each call of a kernel body
extern thread_local uint3 blockIdx, threadIdx;
extern thread_local dim3 blockDim, gridDim;

inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }

// ---- texture objects: a handle to a host image --------------------------------------------------------------------------
struct RefTexture {
    const float* px;
    int w, h;
    int q8;  // keep 8 bits of the interpolation fractions
};
typedef const RefTexture* cudaTextureObject_t;

inline float ref_texel(const RefTexture& t, int x, int y) {
    x = x < 0 ? 0 : (x > t.w - 1 ? t.w - 1 : x);
    y = y < 0 ? 0 : (y > t.h - 1 ? t.h - 1 : y);
    return t.px[(size_t)y * t.w + x];
}
// floor of a texture coordinate as an index that can still be clamped: anything left of the image (NaN included) -> -1,
// anything right of it -> size (both neighbours then clamp to the same border texel)
inline int ref_tex_index(float f, int size) {
    if (!(f >= -1.0f)) return -1;
    if (f > (float)size) return size;
    return (int)f;
}
template <class T>
inline T tex2D(cudaTextureObject_t t, float x, float y) {
    static_assert(std::is_same<T, float>::value, "single-channel float textures only");
    const float xB = x - 0.5f, yB = y - 0.5f;
    const float fi = floorf(xB), fj = floorf(yB);
    float a = xB - fi, b = yB - fj;
    if (t->q8) {
        a = floorf(a * 256.0f + 0.5f) / 256.0f;
        b = floorf(b * 256.0f + 0.5f) / 256.0f;
    }
    const int i = ref_tex_index(fi, t->w), j = ref_tex_index(fj, t->h);
    const float t00 = ref_texel(*t, i, j), t10 = ref_texel(*t, i + 1, j), t01 = ref_texel(*t, i, j + 1), t11 = ref_texel(*t, i + 1, j + 1);
    return (1.0f - a) * (1.0f - b) * t00 + a * (1.0f - b) * t10 + (1.0f - a) * b * t01 + a * b * t11;
}

// ---- cuRAND: a cursor into the caller's table of uniforms ---------------------------------------------------------------
struct curandState {
    const float* row;
    int pos, cap;
};
extern int g_ref_draw_overflow;  // set when any pixel asked for more uniforms than its row holds
inline float curand_uniform(curandState* s) {
    if (s->pos >= s->cap) {
        g_ref_draw_overflow = 1;
        s->pos++;
        return 0.5f;  // ends every rejection loop; the driver reports the overflow as an error
    }
    return s->row[s->pos++];
}
inline long long clock64() { return 0; }
inline void curand_init(long long, int, int, curandState*) {}  // the driver positions the cursors itself

#endif
