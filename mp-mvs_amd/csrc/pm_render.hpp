// pm_render.hpp -- z-buffer render of a point cloud into pinhole cameras with a splat visibility test (mpmvs_cloud_render_depth;
// contract: DESIGN.md section 14 and include/mpmvs.h): the per-view ground-truth depth map of a scan.  Per view and pixel
//   Zc = the smallest z of the in-view points that land in the pixel (+inf: none), z, u, v by project_depth (pm_device.hpp),
//        pixel = ((int)(u + 0.5f), (int)(v + 0.5f));
//   Z1 = the smallest Zc of the (2 splat + 1)^2 window around the pixel, inside the image;
//   depth = Zc if it is finite and Zc <= Z1 * (1 + occl_rel) in fp32, else 0;  idx = the smallest index of a point of the pixel
//        whose z has the bits of Zc where depth != 0, else -1.
// Bit for bit the plain-loop statement and independent of scheduling: all that threads share are integer minima.
//
// Passes (the buffers of a chunk of views lie behind one another; Zc starts as +inf bits, idx as 0xffffffff):
//   1. k_render_zmin     one thread per point, the views of the chunk in a loop (the cameras are kernel arguments, indexed
//                        uniformly): the point read once, per in-view (point, view) one 32-bit atomicMin on the bits of z -- z > 0,
//                        so the bits order as the values.
//   2. k_render_index    only when an index map is wanted: the same projection again (the same code, hence the same bits); a
//                        point whose z bits equal Zc at its pixel does an unsigned atomicMin on its index.
//   3. k_render_resolve  one thread per pixel of one view: the window minimum in a direct loop over Zc (min is associative, so
//                        any order gives the same bits), the visibility test, the store of depth, and -1 into idx where depth is 0.
// The per-thread bodies are host and device code, so that tools/render_check.cpp replays the passes thread by thread under the
// sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"    // cloud_bits, cloud_float, cloud_finite
#include "pm_device.hpp"   // CamDev, project_depth

namespace pm {

constexpr int kRenderMaxSplat = 8;
constexpr int kRenderChunk = 8;                    // views per launch of the point passes
constexpr uint32_t kRenderInfBits = 0x7f800000u;   // Zc of a pixel without a point
constexpr uint32_t kRenderNoIdx = 0xffffffffu;     // idx of a pixel before the index pass: above every index

struct RenderView {
    CamDev cam;
    int w, h;
    uint32_t* zc;    // [h * w] bits of the nearest z
    uint32_t* idx;   // [h * w] or null: no index map wanted for this view
};
struct RenderChunkArgs {
    int n;
    RenderView v[kRenderChunk];
};

// the integer minimum the passes share; the host replay runs one thread at a time
__host__ __device__ inline void render_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// pixel and z of a point with finite coordinates in a view; false: not in view.  A comparison with a NaN is false.
__host__ __device__ inline bool render_project(const RenderView& V, float p0, float p1, float p2, size_t& pix, float& z) {
    float u, v;
    project_depth(V.cam, p0, p1, p2, u, v, z);
    if (!(cloud_finite(z) && z > 0.0f)) return false;
    const float fu = u + 0.5f, fv = v + 0.5f;
    if (!(fu >= 0.0f && fu < (float)V.w && fv >= 0.0f && fv < (float)V.h)) return false;
    pix = (size_t)(int)fv * (size_t)V.w + (size_t)(int)fu;   // 0 <= fu < w <= 2^24: the conversion is exact and in range
    return true;
}

template <bool INDEX>
__host__ __device__ inline void render_point_one(size_t i, const float* __restrict__ xyz, const RenderChunkArgs& A) {
    const float p0 = xyz[3 * i], p1 = xyz[3 * i + 1], p2 = xyz[3 * i + 2];
    if (!(cloud_finite(p0) && cloud_finite(p1) && cloud_finite(p2))) return;
    for (int k = 0; k < A.n; ++k) {
        const RenderView& V = A.v[k];
        if (INDEX && !V.idx) continue;
        size_t pix;
        float z;
        if (!render_project(V, p0, p1, p2, pix, z)) continue;
        if (!INDEX)
            render_min(&V.zc[pix], cloud_bits(z));
        else if (V.zc[pix] == cloud_bits(z))
            render_min(&V.idx[pix], (uint32_t)i);
    }
}

__global__ __launch_bounds__(256) void k_render_zmin(const float* __restrict__ xyz, int n, RenderChunkArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) render_point_one<false>(i, xyz, A);
}

__global__ __launch_bounds__(256) void k_render_index(const float* __restrict__ xyz, int n, RenderChunkArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) render_point_one<true>(i, xyz, A);
}

// pixel `pix` of a w x h view; m = 1.0f + occl_rel
__host__ __device__ inline void render_resolve_one(size_t pix, const uint32_t* __restrict__ zc, int w, int h, int splat, float m, float* __restrict__ depth,
                                                   uint32_t* __restrict__ idx) {
    const int y = (int)(pix / (size_t)w), x = (int)(pix - (size_t)y * (size_t)w);
    const uint32_t own = zc[pix];
    bool visible = false;
    if (own != kRenderInfBits) {
        const int x0 = x - splat < 0 ? 0 : x - splat, x1 = x + splat > w - 1 ? w - 1 : x + splat;
        const int y0 = y - splat < 0 ? 0 : y - splat, y1 = y + splat > h - 1 ? h - 1 : y + splat;
        uint32_t z1 = own;
        for (int yy = y0; yy <= y1; ++yy) {
            const uint32_t* row = zc + (size_t)yy * (size_t)w;
            for (int xx = x0; xx <= x1; ++xx) {
                const uint32_t t = row[xx];
                z1 = t < z1 ? t : z1;
            }
        }
        visible = cloud_float(own) <= cloud_float(z1) * m;
    }
    depth[pix] = visible ? cloud_float(own) : 0.0f;
    if (idx && !visible) idx[pix] = kRenderNoIdx;   // -1 as an int32
}

// one thread per pixel of one view
__global__ __launch_bounds__(256) void k_render_resolve(const uint32_t* __restrict__ zc, int w, int h, int splat, float m, float* __restrict__ depth,
                                                        uint32_t* __restrict__ idx) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix < (size_t)w * (size_t)h) render_resolve_one(pix, zc, w, h, splat, m, depth, idx);
}

}  // namespace pm
