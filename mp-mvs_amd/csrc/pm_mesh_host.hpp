// pm_mesh_host.hpp -- the mesh handle (mpmvs_mesh) and its first step onto the device, for the two translation units that see inside
// it: mpmvs_mesh.hip, which owns the handle and every operation on a mesh alone, and mpmvs_cloud.hip, whose mpmvs_surface_distance
// reads a mesh's resident vertices and triangles against a cloud's grid.  Hidden, like everything of the host side: the library's
// dynamic symbol table is include/mpmvs.h and the kernels.
#pragma once

#include <cstdint>
#include <vector>

#include "pm_host.hpp"

#pragma GCC visibility push(hidden)

extern "C" {
struct mpmvs_mesh {
    int device = 0;
    long long n = 0, m = 0;
    bool with_color = false, ready = false;
    double scale = 0.0;                  // of the normals (mesh_scale); 0: every normal is (0, 0, 0)
    std::vector<float> xyz;              // the copies of create, until the first operation on the device has uploaded them
    std::vector<unsigned char> rgb;
    std::vector<int32_t> tri;
    float* d_xyz = nullptr;
    unsigned char* d_rgb = nullptr;
    int32_t* d_tri = nullptr;
    hipStream_t stream = nullptr;
    PassClock<5> clock;
    float ms[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // for mpmvs_simplify_mesh: the finite vertices and their bounding box, taken at create while the host copy exists
    long long n_fin = 0;
    float mn[3] = {0.0f, 0.0f, 0.0f}, mx[3] = {0.0f, 0.0f, 0.0f};
    float simp_ms[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // for mpmvs_surface_distance: the triangles whose three vertices are finite, counted at create; the passes of its last call and
    // of the last mpmvs_surface_sample
    long long m_fin = 0;
    float dist_ms[3] = {0.0f, 0.0f, 0.0f}, sample_ms[3] = {0.0f, 0.0f, 0.0f};
    // the passes of the last mpmvs_surface_render_depth: init, small, large, resolve
    float render_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    long long render_work[2] = {0, 0};   // of the same call: the pixels of the pairs' boxes, the atomic minima issued
};
}

// the first operation that needs the device: the stream and the mesh itself
inline int mesh_ready(mpmvs_mesh* h) {
    CALLCHK(enter_device(h->device));
    if (h->ready) return 0;
    if (!h->stream) CALLCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (!h->d_xyz) CALLCHK(pool_malloc(&h->d_xyz, n * 12));
    if (h->with_color && !h->d_rgb) CALLCHK(pool_malloc(&h->d_rgb, n * 3));
    if (m > 0 && !h->d_tri) CALLCHK(pool_malloc(&h->d_tri, m * 12));
    CALLCHK(hipMemcpyAsync(h->d_xyz, h->xyz.data(), n * 12, hipMemcpyHostToDevice, h->stream));
    if (h->with_color) CALLCHK(hipMemcpyAsync(h->d_rgb, h->rgb.data(), n * 3, hipMemcpyHostToDevice, h->stream));
    if (m > 0) CALLCHK(hipMemcpyAsync(h->d_tri, h->tri.data(), m * 12, hipMemcpyHostToDevice, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    std::vector<float>().swap(h->xyz);
    std::vector<unsigned char>().swap(h->rgb);
    std::vector<int32_t>().swap(h->tri);
    h->ready = true;
    return 0;
}

#pragma GCC visibility pop
