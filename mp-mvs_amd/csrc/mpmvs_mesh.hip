// mpmvs_mesh.hip -- the surface family of the C ABI declared in include/mpmvs.h: the dense TSDF volume handle (mpmvs_tsdf), the
// integration of depth maps into it and the marching-tetrahedra mesh of its zero level set (kernels and per-thread bodies:
// pm_tsdf.hpp).  Errors are reported like those of mpmvs_cloud_*: through mpmvs_last_error(NULL), per host
// thread; everything but -100 is found before the device is touched.  A handle opens its device with the first call that needs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_tsdf.hpp"

using namespace pm;

extern "C" {

constexpr long long kTsdfMaxVoxels = 1ll << 30;
constexpr long long kTsdfMaxViews = 1ll << 23;          // 2^23 views x 255 < 2^31: the colour sums cannot overflow
constexpr size_t kTsdfChunkPixels = (size_t)1 << 26;    // pixels per launch of the integration: 256 MB of depth maps on the device

struct mpmvs_tsdf {
    int device = 0;
    TsdfVol V{};
    size_t n_vox = 0;
    bool with_color = false, ready = false;
    long long views = 0;   // integrated over the handle's life
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // mesh: mark, scan, [the host reads the counts] vertices, triangles; ev[0], ev[1]: an integration launch
    float* d_sum = nullptr;
    int32_t* d_weight = nullptr;
    uint4* d_color = nullptr;
    float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
};

// the first call that needs the device: the stream, the events and the volume, all zero
static int tsdf_ready(mpmvs_tsdf* h) {
    CALLCHK(enter_device(h->device));
    if (h->ready) return 0;
    if (!h->stream) CALLCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev)
        if (!e) CALLCHK(hipEventCreate(&e));
    if (!h->d_sum) CALLCHK(pool_malloc(&h->d_sum, h->n_vox * 4));
    if (!h->d_weight) CALLCHK(pool_malloc(&h->d_weight, h->n_vox * 4));
    if (h->with_color && !h->d_color) CALLCHK(pool_malloc(&h->d_color, h->n_vox * 16));
    CALLCHK(hipMemsetAsync(h->d_sum, 0, h->n_vox * 4, h->stream));
    CALLCHK(hipMemsetAsync(h->d_weight, 0, h->n_vox * 4, h->stream));
    if (h->with_color) CALLCHK(hipMemsetAsync(h->d_color, 0, h->n_vox * 16, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    h->ready = true;
    return 0;
}

int mpmvs_tsdf_create(int device, const float origin[3], float voxel, const int dims[3], float trunc, int with_color, mpmvs_tsdf** out) {
    if (!out || !origin || !dims) return call_fail(-2, "tsdf create: bad argument");
    if (device < 0) return call_fail(-2, "tsdf create: negative device");
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) return call_fail(-2, "tsdf create: the origin must be finite");
        if (dims[a] < 1) return call_fail(-2, "tsdf create: every dimension must be at least 1");
    }
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return call_fail(-2, "tsdf create: voxel must be finite and positive");
    if (!std::isfinite(trunc) || !(trunc > 0.0f)) return call_fail(-2, "tsdf create: trunc must be finite and positive");
    const long long n_vox = ((long long)dims[0] * (long long)dims[1] > kTsdfMaxVoxels) ? kTsdfMaxVoxels + 1 : (long long)dims[0] * (long long)dims[1] * (long long)dims[2];
    if (n_vox > kTsdfMaxVoxels) return call_fail(-3, "tsdf create: more than 2^30 voxels");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite((float)((double)origin[a] + (double)(dims[a] - 1) * (double)voxel))) return call_fail(-2, "tsdf create: the far corner of the volume is not finite in fp32");
    mpmvs_tsdf* h = new mpmvs_tsdf;
    h->device = device;
    h->V.nx = dims[0]; h->V.ny = dims[1]; h->V.nz = dims[2];
    h->V.trunc = trunc;
    for (int a = 0; a < 3; ++a) h->V.o[a] = (double)origin[a];
    h->V.voxel = (double)voxel;
    h->n_vox = (size_t)n_vox;
    h->with_color = with_color != 0;
    *out = h;
    return 0;
}

void mpmvs_tsdf_destroy(mpmvs_tsdf* h) {
    if (!h) return;
    if (h->stream || h->d_sum) {
        (void)enter_device(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void* p : {(void*)h->d_sum, (void*)h->d_weight, (void*)h->d_color})
            if (p) (void)pool_free(p);
        for (hipEvent_t e : h->ev)
            if (e) (void)hipEventDestroy(e);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

// views [v0, v1) of an integrate call: the images up, one launch, its time added to ms[0]
static int tsdf_integrate_chunk(mpmvs_tsdf* h, int v0, int v1, const mpmvs_camera* cams, const float* const* depths, const unsigned char* const* colors, int channels) {
    const hipStream_t st = h->stream;
    size_t pixels = 0;
    for (int v = v0; v < v1; ++v) pixels += (size_t)cams[v].width * (size_t)cams[v].height;
    Scratch d_depth(st), d_col(st);
    CALLCHK(d_depth.alloc(pixels * 4));
    if (colors) CALLCHK(d_col.alloc(pixels * (size_t)channels));
    // the block test of pm_tsdf.hpp needs numbers throughout: every |P| of the volume and every camera entry it reads at most 2^40
    float pmax = 0.0f;
    const int last[3] = {h->V.nx - 1, h->V.ny - 1, h->V.nz - 1};
    for (int a = 0; a < 3; ++a) pmax = std::max(pmax, std::max(std::fabs(tsdf_pos(h->V, a, 0)), std::fabs(tsdf_pos(h->V, a, last[a]))));
    TsdfChunkArgs A;
    std::memset(&A, 0, sizeof A);
    A.n = v1 - v0;
    A.channels = colors ? channels : 0;
    size_t at = 0;
    for (int v = v0; v < v1; ++v) {
        const mpmvs_camera& c = cams[v];
        TsdfView& W = A.v[v - v0];
        std::memcpy(W.R, c.R, sizeof W.R);
        std::memcpy(W.t, c.t, sizeof W.t);
        W.K0 = c.K[0]; W.K2 = c.K[2]; W.K4 = c.K[4]; W.K5 = c.K[5];
        W.w = c.width; W.h = c.height;
        W.cull = pmax <= kTsdfCullBound;
        for (float x : c.R) W.cull = W.cull && std::fabs(x) <= kTsdfCullBound;   // false for a NaN
        for (float x : {c.t[0], c.t[1], c.t[2], W.K0, W.K2, W.K4, W.K5}) W.cull = W.cull && std::fabs(x) <= kTsdfCullBound;
        const size_t npix = (size_t)c.width * (size_t)c.height;
        W.depth = d_depth.as<float>() + at;
        CALLCHK(hipMemcpyAsync(d_depth.as<float>() + at, depths[v], npix * 4, hipMemcpyHostToDevice, st));
        if (colors) {
            W.color = d_col.as<unsigned char>() + at * (size_t)channels;
            CALLCHK(hipMemcpyAsync(d_col.as<unsigned char>() + at * (size_t)channels, colors[v], npix * (size_t)channels, hipMemcpyHostToDevice, st));
        }
        at += npix;
    }
    const size_t tiles = (size_t)((h->V.nx + kTsdfTileX - 1) / kTsdfTileX) * (size_t)((h->V.ny + kTsdfTileY - 1) / kTsdfTileY) * (size_t)h->V.nz;
    CALLCHK(hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)tiles), dim3(256), 0, st, h->V, A, h->d_sum, h->d_weight, h->with_color ? h->d_color : (uint4*)nullptr);
    CALLCHK(hipGetLastError());
    CALLCHK(hipEventRecord(h->ev[1], st));
    CALLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    CALLCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[0] += ms;
    return 0;
}

int mpmvs_tsdf_integrate(mpmvs_tsdf* h, int n_views, const mpmvs_camera* cams, const float* const* depths, const unsigned char* const* colors, int color_channels) {
    if (!h || n_views < 0) return call_fail(-2, "tsdf integrate: bad argument");
    if (colors && !h->with_color) return call_fail(-2, "tsdf integrate: colours given to a volume without colour");
    if (!colors && h->with_color && n_views > 0) return call_fail(-2, "tsdf integrate: a volume with colour needs colours");
    if (colors && color_channels != 1 && color_channels != 3) return call_fail(-2, "tsdf integrate: color_channels must be 1 or 3");
    if (n_views == 0) return 0;
    if (!cams || !depths) return call_fail(-2, "tsdf integrate: bad argument");
    for (int v = 0; v < n_views; ++v) {
        if (!depths[v]) return call_fail(-2, "tsdf integrate: view " + std::to_string(v) + " has no depth map");
        if (colors && !colors[v]) return call_fail(-2, "tsdf integrate: view " + std::to_string(v) + " has no colour image");
        if (cams[v].width <= 0 || cams[v].height <= 0) return call_fail(-2, "tsdf integrate: view " + std::to_string(v) + " has a non-positive width or height");
    }
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].width > (1 << 24) || cams[v].height > (1 << 24)) return call_fail(-3, "tsdf integrate: view " + std::to_string(v) + " is wider or higher than 2^24");
        if ((long long)cams[v].width * (long long)cams[v].height > (long long)INT32_MAX)
            return call_fail(-3, "tsdf integrate: view " + std::to_string(v) + " has more than 2^31 - 1 pixels");
    }
    if (h->views + (long long)n_views > kTsdfMaxViews) return call_fail(-3, "tsdf integrate: more than 2^23 views over the life of the volume");
    const int rc = tsdf_ready(h);
    if (rc) return rc;
    h->ms[0] = 0.0f;
    for (int v0 = 0; v0 < n_views;) {
        int v1 = v0 + 1;
        size_t pixels = (size_t)cams[v0].width * (size_t)cams[v0].height;
        while (v1 < n_views && v1 - v0 < kTsdfChunk && pixels + (size_t)cams[v1].width * (size_t)cams[v1].height <= kTsdfChunkPixels) {
            pixels += (size_t)cams[v1].width * (size_t)cams[v1].height;
            ++v1;
        }
        const int rc2 = tsdf_integrate_chunk(h, v0, v1, cams, depths, colors, color_channels);
        if (rc2) return rc2;
        h->views += v1 - v0;
        v0 = v1;
    }
    return 0;
}

int mpmvs_tsdf_get(mpmvs_tsdf* h, float* sum, int32_t* weight, uint32_t* color4) {
    if (!h || !sum || !weight) return call_fail(-2, "tsdf get: bad argument");
    if (color4 && !h->with_color) return call_fail(-2, "tsdf get: the volume has no colour");
    const int rc = tsdf_ready(h);
    if (rc) return rc;
    CALLCHK(hipMemcpyAsync(sum, h->d_sum, h->n_vox * 4, hipMemcpyDeviceToHost, h->stream));
    CALLCHK(hipMemcpyAsync(weight, h->d_weight, h->n_vox * 4, hipMemcpyDeviceToHost, h->stream));
    if (color4) CALLCHK(hipMemcpyAsync(color4, h->d_color, h->n_vox * 16, hipMemcpyDeviceToHost, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int mpmvs_tsdf_set(mpmvs_tsdf* h, const float* sum, const int32_t* weight, const uint32_t* color4) {
    if (!h || !sum || !weight) return call_fail(-2, "tsdf set: bad argument");
    if (color4 && !h->with_color) return call_fail(-2, "tsdf set: the volume has no colour");
    const int rc = tsdf_ready(h);
    if (rc) return rc;
    CALLCHK(hipMemcpyAsync(h->d_sum, sum, h->n_vox * 4, hipMemcpyHostToDevice, h->stream));
    CALLCHK(hipMemcpyAsync(h->d_weight, weight, h->n_vox * 4, hipMemcpyHostToDevice, h->stream));
    if (color4) CALLCHK(hipMemcpyAsync(h->d_color, color4, h->n_vox * 16, hipMemcpyHostToDevice, h->stream));
    else if (h->with_color) CALLCHK(hipMemsetAsync(h->d_color, 0, h->n_vox * 16, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// the device half of mpmvs_tsdf_mesh; the host buffers are allocated once the counts are known and handed over on success only
static long long tsdf_mesh_device(mpmvs_tsdf* h, int min_weight, float** xyz, unsigned char** rgb, int32_t** tri, long long* n_tri) {
    const hipStream_t st = h->stream;
    const size_t n = h->n_vox;
    const int n_tiles = (int)((n + kScanBlock - 1) / kScanBlock);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    Scratch d_mask(st), d_vexcl(st), d_tcount(st), d_totals(st), d_grand(st);
    CALLCHK(d_mask.alloc(n * 4));
    CALLCHK(d_vexcl.alloc(n * 4));
    CALLCHK(d_tcount.alloc(n * 4));
    CALLCHK(d_totals.alloc((size_t)n_tiles * 8));
    CALLCHK(d_grand.alloc(16));
    int* vtile = d_totals.as<int>();
    int* ttile = vtile + n_tiles;
    CALLCHK(hipMemsetAsync(d_grand.p, 0, 16, st));
    CALLCHK(hipEventRecord(h->ev[0], st));
    CALLCHK(hipMemsetAsync(d_mask.p, 0, n * 4, st));
    hipLaunchKernelGGL(k_tsdf_mark, dim3(blocks), dim3(256), 0, st, h->V, n, h->d_sum, h->d_weight, min_weight, d_mask.as<uint32_t>(), d_tcount.as<int>());
    CALLCHK(hipGetLastError());
    CALLCHK(hipEventRecord(h->ev[1], st));
    hipLaunchKernelGGL(k_tsdf_scan_tiles, dim3((unsigned)n_tiles), dim3(kScanBlock), 0, st, d_mask.as<uint32_t>(), n, d_vexcl.as<int>(), d_tcount.as<int>(), vtile, n_tiles);
    CALLCHK(hipGetLastError());
    hipLaunchKernelGGL(k_tsdf_sum_totals, dim3((unsigned)((n_tiles + kScanBlock - 1) / kScanBlock), 2), dim3(kScanBlock), 0, st, vtile, n_tiles, d_grand.as<unsigned long long>());
    CALLCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(2), dim3(kScanBlock), 0, st, vtile, n_tiles, 0, (int*)nullptr);
    CALLCHK(hipGetLastError());
    CALLCHK(hipEventRecord(h->ev[2], st));
    unsigned long long grand[2] = {0, 0};
    CALLCHK(hipMemcpyAsync(grand, d_grand.p, 16, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    CALLCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[1] = ms;
    CALLCHK(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->ms[2] = ms;
    if (grand[0] > (unsigned long long)INT32_MAX || grand[1] > (unsigned long long)INT32_MAX)
        return call_fail(-3, "tsdf mesh: " + std::to_string(grand[0]) + " vertices and " + std::to_string(grand[1]) + " triangles: more than 2^31 - 1");
    const size_t nv = (size_t)grand[0], nt = (size_t)grand[1];
    if (nt == 0) return 0;   // then nv == 0 too: a vertex exists only on an edge some triangle uses
    Scratch d_xyz(st), d_rgb(st), d_tri(st);
    CALLCHK(d_xyz.alloc(nv * 12));
    if (h->with_color) CALLCHK(d_rgb.alloc(nv * 3));
    CALLCHK(d_tri.alloc(nt * 12));
    CALLCHK(hipEventRecord(h->ev[5], st));
    hipLaunchKernelGGL(k_tsdf_vertices, dim3(blocks), dim3(256), 0, st, h->V, n, h->d_sum, h->d_weight, h->with_color ? h->d_color : (const uint4*)nullptr,
                       d_mask.as<uint32_t>(), d_vexcl.as<int>(), vtile, d_xyz.as<float>(), h->with_color ? d_rgb.as<unsigned char>() : (unsigned char*)nullptr);
    CALLCHK(hipGetLastError());
    CALLCHK(hipEventRecord(h->ev[3], st));
    hipLaunchKernelGGL(k_tsdf_triangles, dim3(blocks), dim3(256), 0, st, h->V, n, h->d_sum, h->d_weight, min_weight, d_mask.as<uint32_t>(), d_vexcl.as<int>(), vtile,
                       d_tcount.as<int>(), ttile, d_tri.as<int32_t>());
    CALLCHK(hipGetLastError());
    CALLCHK(hipEventRecord(h->ev[4], st));
    float* hx = (float*)std::malloc(nv * 12);
    int32_t* ht = (int32_t*)std::malloc(nt * 12);
    unsigned char* hc = h->with_color ? (unsigned char*)std::malloc(nv * 3) : nullptr;
    struct Guard {
        void *a, *b, *c;
        ~Guard() { std::free(a); std::free(b); std::free(c); }
    } g{hx, ht, hc};
    if (!hx || !ht || (h->with_color && !hc)) return call_fail(-100, "tsdf mesh: out of host memory");
    CALLCHK(hipMemcpyAsync(hx, d_xyz.p, nv * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(ht, d_tri.p, nt * 12, hipMemcpyDeviceToHost, st));
    if (hc) CALLCHK(hipMemcpyAsync(hc, d_rgb.p, nv * 3, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(hipEventElapsedTime(&ms, h->ev[5], h->ev[3]));
    h->ms[3] = ms;
    CALLCHK(hipEventElapsedTime(&ms, h->ev[3], h->ev[4]));
    h->ms[4] = ms;
    g.a = g.b = g.c = nullptr;
    *xyz = hx;
    *tri = ht;
    *rgb = hc;
    *n_tri = (long long)nt;
    return (long long)nv;
}

long long mpmvs_tsdf_mesh(mpmvs_tsdf* h, int min_weight, float** out_xyz, unsigned char** out_rgb, int32_t** out_tri, long long* n_tri) {
    if (!h || !out_xyz || !out_tri || !n_tri) return call_fail(-2, "tsdf mesh: bad argument");
    if (min_weight < 1) return call_fail(-2, "tsdf mesh: min_weight must be at least 1");
    if (h->with_color && !out_rgb) return call_fail(-2, "tsdf mesh: a volume with colour needs out_rgb");
    if (!h->with_color && out_rgb) return call_fail(-2, "tsdf mesh: the volume has no colour");
    float* xyz = nullptr;
    unsigned char* rgb = nullptr;
    int32_t* tri = nullptr;
    long long nt = 0, nv = 0;
    h->ms[1] = h->ms[2] = h->ms[3] = h->ms[4] = 0.0f;
    if (h->V.nx > 1 && h->V.ny > 1 && h->V.nz > 1) {   // else there is no cell: nothing is launched
        const int rc = tsdf_ready(h);
        if (rc) return rc;
        nv = tsdf_mesh_device(h, min_weight, &xyz, &rgb, &tri, &nt);
        if (nv < 0) return nv;
    }
    *out_xyz = xyz;
    *out_tri = tri;
    if (out_rgb) *out_rgb = rgb;
    *n_tri = nt;
    return nv;
}

int mpmvs_tsdf_pass_ms(const mpmvs_tsdf* h, float ms[5]) {
    if (!h || !ms) return call_fail(-2, "tsdf pass_ms: bad argument");
    std::memcpy(ms, h->ms, sizeof h->ms);
    return 0;
}

}  // extern "C"
