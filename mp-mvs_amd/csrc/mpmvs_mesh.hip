// mpmvs_mesh.hip -- the surface family of the C ABI declared in include/mpmvs.h: the TSDF volume handle (mpmvs_tsdf), dense or
// brick-sparse, the integration of depth maps into it and the marching-tetrahedra mesh of its zero level set (kernels and per-thread
// bodies: pm_tsdf.hpp, pm_tsdf_sparse.hpp; DESIGN.md sections 22 and 23); and the indexed triangle mesh handle (mpmvs_mesh): its
// connected components, vertex normals and compaction (pm_mesh.hpp, pm_unionfind.hpp), and its simplification by
// vertex clustering (pm_simplify.hpp on the clustering passes of pm_cloud.hpp and pm_voxel.hpp), its samples
// (pm_surface.hpp; section 26) and its render into cameras (pm_raster.hpp; section 27).  Errors are
// reported like those of mpmvs_cloud_*: through mpmvs_last_error(NULL), per host thread; everything but -100 is found before the
// device is touched.  A handle opens its device with the first call that needs it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_scan_host.hpp"
#include "pm_cluster_host.hpp"
#include "pm_mesh.hpp"
#include "pm_mesh_host.hpp"
#include "pm_surface.hpp"
#include "pm_raster.hpp"
#include "pm_simplify.hpp"
#include "pm_tsdf.hpp"
#include "pm_tsdf_sparse.hpp"

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
    PassClock<6> clock;   // mesh: mark, scan, [the host reads the counts] vertices, triangles; marks 0 and 1: an integration launch
    float* d_sum = nullptr;
    int32_t* d_weight = nullptr;
    uint4* d_color = nullptr;
    float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // a brick-sparse handle (mpmvs_tsdf_create_sparse): d_sum, d_weight and d_color hold n_bricks * 512 entries in brick-major order
    bool sparse = false;
    TsdfAlloc alloc{};
    int bx = 0, by = 0, bz = 0;
    size_t n_grid = 0;
    long long max_bricks = 0, n_bricks = 0;
    int32_t* d_grid = nullptr;       // [n_grid]: rank or -1
    int32_t* d_list = nullptr;       // [n_bricks]: linear index per rank
    std::vector<int32_t> list;       // its host copy
    float alloc_ms[2] = {0.0f, 0.0f};
};

// the first call that needs the device: the stream; then a dense handle's volume, all zero, or a brick-sparse
// handle's brick grid, all -1
static int tsdf_ready(mpmvs_tsdf* h) {
    CALLCHK(enter_device(h->device));
    if (h->ready) return 0;
    if (!h->stream) CALLCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if (h->sparse) {
        if (!h->d_grid) CALLCHK(pool_malloc(&h->d_grid, h->n_grid * 4));
        CALLCHK(hipMemsetAsync(h->d_grid, 0xff, h->n_grid * 4, h->stream));
    } else {
        if (!h->d_sum) CALLCHK(pool_malloc(&h->d_sum, h->n_vox * 4));
        if (!h->d_weight) CALLCHK(pool_malloc(&h->d_weight, h->n_vox * 4));
        if (h->with_color && !h->d_color) CALLCHK(pool_malloc(&h->d_color, h->n_vox * 16));
        CALLCHK(hipMemsetAsync(h->d_sum, 0, h->n_vox * 4, h->stream));
        CALLCHK(hipMemsetAsync(h->d_weight, 0, h->n_vox * 4, h->stream));
        if (h->with_color) CALLCHK(hipMemsetAsync(h->d_color, 0, h->n_vox * 16, h->stream));
    }
    CALLCHK(hipStreamSynchronize(h->stream));
    h->ready = true;
    return 0;
}
static TsdfBricks tsdf_bricks(const mpmvs_tsdf* h) { return TsdfBricks{h->bx, h->by, h->bz, h->d_grid, h->d_list}; }

// the lattice arguments of both create calls (`name` is the call's, for the message): everything but the far corner, which each
// call asks for with tsdf_new_handle after the size checks of its own
static int tsdf_check_lattice(const std::string& name, int device, const float* origin, float voxel, const int* dims, float trunc, mpmvs_tsdf** out) {
    if (!out || !origin || !dims) return call_fail(-2, name + ": bad argument");
    if (device < 0) return call_fail(-2, name + ": negative device");
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) return call_fail(-2, name + ": the origin must be finite");
        if (dims[a] < 1) return call_fail(-2, name + ": every dimension must be at least 1");
    }
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return call_fail(-2, name + ": voxel must be finite and positive");
    if (!std::isfinite(trunc) || !(trunc > 0.0f)) return call_fail(-2, name + ": trunc must be finite and positive");
    return 0;
}
// the last check of the lattice, then the handle with the fields that both kinds of volume have
static int tsdf_new_handle(const std::string& name, int device, const float* origin, float voxel, const int* dims, float trunc, int with_color, mpmvs_tsdf** out) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite((float)((double)origin[a] + (double)(dims[a] - 1) * (double)voxel))) return call_fail(-2, name + ": the far corner of the volume is not finite in fp32");
    mpmvs_tsdf* h = new mpmvs_tsdf;
    h->device = device;
    h->V.nx = dims[0]; h->V.ny = dims[1]; h->V.nz = dims[2];
    h->V.trunc = trunc;
    for (int a = 0; a < 3; ++a) h->V.o[a] = (double)origin[a];
    h->V.voxel = (double)voxel;
    h->n_vox = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];   // of a brick-sparse volume: virtual
    h->with_color = with_color != 0;
    *out = h;
    return 0;
}

int mpmvs_tsdf_create(int device, const float origin[3], float voxel, const int dims[3], float trunc, int with_color, mpmvs_tsdf** out) {
    const int rc = tsdf_check_lattice("tsdf create", device, origin, voxel, dims, trunc, out);
    if (rc) return rc;
    if ((long long)dims[0] * (long long)dims[1] > kTsdfMaxVoxels || (long long)dims[0] * (long long)dims[1] * (long long)dims[2] > kTsdfMaxVoxels)
        return call_fail(-3, "tsdf create: more than 2^30 voxels");
    return tsdf_new_handle("tsdf create", device, origin, voxel, dims, trunc, with_color, out);
}

void mpmvs_tsdf_destroy(mpmvs_tsdf* h) {
    if (!h) return;
    if (h->stream || h->d_sum || h->d_grid) {
        (void)enter_device(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void* p : {(void*)h->d_sum, (void*)h->d_weight, (void*)h->d_color, (void*)h->d_grid, (void*)h->d_list})
            if (p) (void)pool_free(p);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;   // the clock goes here: the stream has been waited for
}

// the views of an integrate or allocate call (`name` is the call's, for the message): every -2 of every view before any -3
static int tsdf_check_views(const std::string& name, int n_views, const mpmvs_camera* cams, const float* const* depths, const unsigned char* const* colors) {
    if (!cams || !depths) return call_fail(-2, name + ": bad argument");
    for (int v = 0; v < n_views; ++v) {
        if (!depths[v]) return call_fail(-2, name + ": view " + std::to_string(v) + " has no depth map");
        if (colors && !colors[v]) return call_fail(-2, name + ": view " + std::to_string(v) + " has no colour image");
        if (cams[v].width <= 0 || cams[v].height <= 0) return call_fail(-2, name + ": view " + std::to_string(v) + " has a non-positive width or height");
    }
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].width > (1 << 24) || cams[v].height > (1 << 24)) return call_fail(-3, name + ": view " + std::to_string(v) + " is wider or higher than 2^24");
        if ((long long)cams[v].width * (long long)cams[v].height > (long long)INT32_MAX)
            return call_fail(-3, name + ": view " + std::to_string(v) + " has more than 2^31 - 1 pixels");
    }
    return 0;
}

// the views in call order, cut into chunks [v0, v1) of at most kTsdfChunk views and (beyond the first view) kTsdfChunkPixels pixels
static int tsdf_for_chunks(int n_views, const mpmvs_camera* cams, const std::function<int(int, int)>& chunk) {
    for (int v0 = 0; v0 < n_views;) {
        int v1 = v0 + 1;
        size_t pixels = (size_t)cams[v0].width * (size_t)cams[v0].height;
        while (v1 < n_views && v1 - v0 < kTsdfChunk && pixels + (size_t)cams[v1].width * (size_t)cams[v1].height <= kTsdfChunkPixels) {
            pixels += (size_t)cams[v1].width * (size_t)cams[v1].height;
            ++v1;
        }
        const int rc = chunk(v0, v1);
        if (rc) return rc;
        v0 = v1;
    }
    return 0;
}

// views [v0, v1) of a call as kernel arguments: their cameras in A, their depth maps and, if given, their colour images on the device
struct TsdfChunk {
    Scratch d_depth, d_col;
    TsdfChunkArgs A;
    explicit TsdfChunk(hipStream_t st) : d_depth(st), d_col(st) {}
    int upload(const mpmvs_tsdf* h, int v0, int v1, const mpmvs_camera* cams, const float* const* depths, const unsigned char* const* colors, int channels) {
        const hipStream_t st = h->stream;
        size_t pixels = 0;
        for (int v = v0; v < v1; ++v) pixels += (size_t)cams[v].width * (size_t)cams[v].height;
        CALLCHK(d_depth.alloc(pixels * 4));
        if (colors) CALLCHK(d_col.alloc(pixels * (size_t)channels));
        // the block test of pm_tsdf.hpp needs numbers throughout: every |P| of the volume and every camera entry it reads at most 2^40
        float pmax = 0.0f;
        const int last[3] = {h->V.nx - 1, h->V.ny - 1, h->V.nz - 1};
        for (int a = 0; a < 3; ++a) pmax = std::max(pmax, std::max(std::fabs(tsdf_pos(h->V, a, 0)), std::fabs(tsdf_pos(h->V, a, last[a]))));
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
        return 0;
    }
};

// one launch (run: 0 or its -100) between the marks 0 and 1 of the handle's clock, waited for; its time is added to *ms
static int tsdf_timed(mpmvs_tsdf* h, float* ms, const std::function<int()>& run) {
    CALLCHK(h->clock.mark(0, h->stream));
    const int rc = run();
    if (rc) return rc;
    CALLCHK(h->clock.mark(1, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    float t = 0.0f;
    CALLCHK(h->clock.ms(0, 1, &t));
    *ms += t;
    return 0;
}

int mpmvs_tsdf_integrate(mpmvs_tsdf* h, int n_views, const mpmvs_camera* cams, const float* const* depths, const unsigned char* const* colors, int color_channels) {
    if (!h || n_views < 0) return call_fail(-2, "tsdf integrate: bad argument");
    if (colors && !h->with_color) return call_fail(-2, "tsdf integrate: colours given to a volume without colour");
    if (!colors && h->with_color && n_views > 0) return call_fail(-2, "tsdf integrate: a volume with colour needs colours");
    if (colors && color_channels != 1 && color_channels != 3) return call_fail(-2, "tsdf integrate: color_channels must be 1 or 3");
    if (n_views == 0) return 0;
    const int rc = tsdf_check_views("tsdf integrate", n_views, cams, depths, colors);
    if (rc) return rc;
    if (h->views + (long long)n_views > kTsdfMaxViews) return call_fail(-3, "tsdf integrate: more than 2^23 views over the life of the volume");
    if (h->sparse && h->n_bricks == 0) {   // no voxel exists: nothing to add to
        h->ms[0] = 0.0f;
        h->views += n_views;
        return 0;
    }
    const int rc2 = tsdf_ready(h);
    if (rc2) return rc2;
    h->ms[0] = 0.0f;
    const hipStream_t st = h->stream;
    const size_t tiles = (size_t)((h->V.nx + kTsdfTileX - 1) / kTsdfTileX) * (size_t)((h->V.ny + kTsdfTileY - 1) / kTsdfTileY) * (size_t)h->V.nz;
    uint4* const d_color = h->with_color ? h->d_color : nullptr;
    // per chunk: the images up, one launch, its time added to ms[0]
    return tsdf_for_chunks(n_views, cams, [&](int v0, int v1) {
        TsdfChunk c(st);
        const int rc3 = c.upload(h, v0, v1, cams, depths, colors, color_channels);
        if (rc3) return rc3;
        const int rc4 = tsdf_timed(h, &h->ms[0], [&] {
            if (h->sparse) CALLCHK(launch(k_tsdf_sparse_integrate, dim3((unsigned)h->n_bricks), dim3(kBrickVox), st, h->V, tsdf_bricks(h), c.A, h->d_sum, h->d_weight, d_color));
            else CALLCHK(launch(k_tsdf_integrate, dim3((unsigned)tiles), dim3(256), st, h->V, c.A, h->d_sum, h->d_weight, d_color));
            return 0;
        });
        if (!rc4) h->views += v1 - v0;
        return rc4;
    });
}

int mpmvs_tsdf_get(mpmvs_tsdf* h, float* sum, int32_t* weight, uint32_t* color4) {
    if (!h || !sum || !weight) return call_fail(-2, "tsdf get: bad argument");
    if (color4 && !h->with_color) return call_fail(-2, "tsdf get: the volume has no colour");
    if (h->sparse) return call_fail(-2, "tsdf get: a brick-sparse volume is read with mpmvs_tsdf_bricks and mpmvs_tsdf_get_bricks");
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
    if (h->sparse) return call_fail(-2, "tsdf set: a brick-sparse volume is written with mpmvs_tsdf_set_bricks");
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
    const size_t n = h->sparse ? (size_t)h->n_bricks * kBrickVox : h->n_vox;   // sparse: the existing voxels in brick-major order
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
    // passes 1, 3 and 4: a thread per voxel of the lattice, or a block per brick; the brick-sparse kernels take the brick table where
    // the dense ones take the number of voxels, and the rest of the argument list is the same
    auto per_voxel = [&](auto dense, auto sparse, auto... args) {
        return h->sparse ? launch(sparse, dim3((unsigned)h->n_bricks), dim3(kBrickVox), st, h->V, tsdf_bricks(h), args...)
                         : launch(dense, dim3(blocks), dim3(256), st, h->V, n, args...);
    };
    const uint4* const d_color = h->with_color ? h->d_color : nullptr;
    CALLCHK(hipMemsetAsync(d_grand.p, 0, 16, st));
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(hipMemsetAsync(d_mask.p, 0, n * 4, st));
    CALLCHK(per_voxel(k_tsdf_mark, k_tsdf_sparse_mark, h->d_sum, h->d_weight, min_weight, d_mask.as<uint32_t>(), d_tcount.as<int>()));
    CALLCHK(h->clock.mark(1, st));
    // not scan_offsets: the tiles come from the masks' popcounts and the triangle counts at once, and the totals are 64-bit sums
    CALLCHK(launch(k_tsdf_scan_tiles, dim3((unsigned)n_tiles), dim3(kScanBlock), st, d_mask.as<uint32_t>(), n, d_vexcl.as<int>(), d_tcount.as<int>(), vtile, n_tiles));
    CALLCHK(launch(k_tsdf_sum_totals, dim3((unsigned)((n_tiles + kScanBlock - 1) / kScanBlock), 2), dim3(kScanBlock), st, vtile, n_tiles, d_grand.as<unsigned long long>()));
    CALLCHK(launch(k_scan_totals<Sum>, dim3(2), dim3(kScanBlock), st, vtile, n_tiles, 0, nullptr));
    CALLCHK(h->clock.mark(2, st));
    unsigned long long grand[2] = {0, 0};
    CALLCHK(hipMemcpyAsync(grand, d_grand.p, 16, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(h->clock.ms(0, 1, &h->ms[1]));
    CALLCHK(h->clock.ms(1, 2, &h->ms[2]));
    if (grand[0] > (unsigned long long)INT32_MAX || grand[1] > (unsigned long long)INT32_MAX)
        return call_fail(-3, "tsdf mesh: " + std::to_string(grand[0]) + " vertices and " + std::to_string(grand[1]) + " triangles: more than 2^31 - 1");
    const size_t nv = (size_t)grand[0], nt = (size_t)grand[1];
    if (nt == 0) return 0;   // then nv == 0 too: a vertex exists only on an edge some triangle uses
    Scratch d_xyz(st), d_rgb(st), d_tri(st);
    CALLCHK(d_xyz.alloc(nv * 12));
    if (h->with_color) CALLCHK(d_rgb.alloc(nv * 3));
    CALLCHK(d_tri.alloc(nt * 12));
    CALLCHK(h->clock.mark(5, st));
    CALLCHK(per_voxel(k_tsdf_vertices, k_tsdf_sparse_vertices, h->d_sum, h->d_weight, d_color, d_mask.as<uint32_t>(), d_vexcl.as<int>(), vtile, d_xyz.as<float>(),
                      d_rgb.as<unsigned char>()));   // rgb: null without colour
    CALLCHK(h->clock.mark(3, st));
    CALLCHK(per_voxel(k_tsdf_triangles, k_tsdf_sparse_triangles, h->d_sum, h->d_weight, min_weight, d_mask.as<uint32_t>(), d_vexcl.as<int>(), vtile, d_tcount.as<int>(),
                      ttile, d_tri.as<int32_t>()));
    CALLCHK(h->clock.mark(4, st));
    HostOut out;
    float* hx = out.take<float>(nv * 3);
    int32_t* ht = out.take<int32_t>(nt * 3);
    unsigned char* hc = h->with_color ? out.take<unsigned char>(nv * 3) : nullptr;
    if (!hx || !ht || (h->with_color && !hc)) return call_fail(-100, "tsdf mesh: out of host memory");
    CALLCHK(hipMemcpyAsync(hx, d_xyz.p, nv * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(ht, d_tri.p, nt * 12, hipMemcpyDeviceToHost, st));
    if (hc) CALLCHK(hipMemcpyAsync(hc, d_rgb.p, nv * 3, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(h->clock.ms(5, 3, &h->ms[3]));
    CALLCHK(h->clock.ms(3, 4, &h->ms[4]));
    out.keep();
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
    if (h->V.nx > 1 && h->V.ny > 1 && h->V.nz > 1 && !(h->sparse && h->n_bricks == 0)) {   // else there is no cell: nothing is launched
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

// ---- the brick-sparse volume (statements A and B of include/mpmvs.h) -------------------------------------
constexpr long long kTsdfMaxGrid = 1ll << 24, kTsdfMaxBricks = 1ll << 21, kTsdfMaxSamples = 1ll << 16;

int mpmvs_tsdf_create_sparse(int device, const float origin[3], float voxel, const int dims[3], float trunc, int with_color, float pad, long long max_bricks,
                             mpmvs_tsdf** out) {
    const int rc = tsdf_check_lattice("tsdf create_sparse", device, origin, voxel, dims, trunc, out);
    if (rc) return rc;
    if (!std::isfinite(pad) || !(pad >= 0.0f && pad <= 8.0f)) return call_fail(-2, "tsdf create_sparse: pad must be finite and in [0, 8] voxels");
    if (max_bricks < 1) return call_fail(-2, "tsdf create_sparse: max_bricks must be at least 1");
    if (max_bricks > kTsdfMaxBricks) return call_fail(-3, "tsdf create_sparse: max_bricks above 2^21");
    long long b[3], cells = 1;
    for (int a = 0; a < 3; ++a) {
        b[a] = ((long long)dims[a] + kBrick - 1) / kBrick;   // <= 2^28
        cells = cells > kTsdfMaxGrid ? cells : cells * b[a];
    }
    if (cells > kTsdfMaxGrid) return call_fail(-3, "tsdf create_sparse: more than 2^24 cells in the brick grid");
    const double ratio = std::ceil(4.0 * (double)trunc / (double)voxel);
    if (!(ratio <= (double)kTsdfMaxSamples)) return call_fail(-3, "tsdf create_sparse: trunc / voxel asks for more than 2^16 samples per ray");
    const int rc2 = tsdf_new_handle("tsdf create_sparse", device, origin, voxel, dims, trunc, with_color, out);
    if (rc2) return rc2;
    mpmvs_tsdf* h = *out;
    h->sparse = true;
    h->bx = (int)b[0]; h->by = (int)b[1]; h->bz = (int)b[2];
    h->n_grid = (size_t)cells;
    h->max_bricks = max_bricks;
    h->alloc.n_s = std::max(1, (int)ratio);
    h->alloc.step = (2.0 * (double)trunc) / (double)h->alloc.n_s;
    for (int a = 0; a < 3; ++a) h->alloc.origin[a] = origin[a];
    h->alloc.voxel = voxel;
    h->alloc.pad = pad;
    *out = h;
    return 0;
}

// the pool of a new brick set: n bricks, all zero, and its list
struct TsdfPool {
    Scratch sum, weight, color, list;
    explicit TsdfPool(hipStream_t st) : sum(st), weight(st), color(st), list(st) {}
    int alloc(const mpmvs_tsdf* h, size_t n) {
        CALLCHK(sum.alloc(n * kBrickVox * 4));
        CALLCHK(weight.alloc(n * kBrickVox * 4));
        if (h->with_color) CALLCHK(color.alloc(n * kBrickVox * 16));
        CALLCHK(list.alloc(n * 4));
        CALLCHK(hipMemsetAsync(sum.p, 0, n * kBrickVox * 4, h->stream));
        CALLCHK(hipMemsetAsync(weight.p, 0, n * kBrickVox * 4, h->stream));
        if (h->with_color) CALLCHK(hipMemsetAsync(color.p, 0, n * kBrickVox * 16, h->stream));
        return 0;
    }
    // the handle takes the new pool, this object the old one (released when it goes out of scope); the stream must be idle
    void swap_into(mpmvs_tsdf* h) {
        std::swap(*(void**)&h->d_sum, sum.p);
        std::swap(*(void**)&h->d_weight, weight.p);
        std::swap(*(void**)&h->d_color, color.p);
        std::swap(*(void**)&h->d_list, list.p);
    }
};

// the scan, the refusal and the commit of mpmvs_tsdf_allocate, after the marking
static int tsdf_commit(mpmvs_tsdf* h, const uint32_t* d_flags) {
    const hipStream_t st = h->stream;
    const int n_grid = (int)h->n_grid, n_tiles = (n_grid + kScanBlock - 1) / kScanBlock;
    Scratch d_excl(st), d_totals(st), d_grand(st);
    CALLCHK(d_excl.alloc((size_t)n_grid * 4));
    CALLCHK(d_totals.alloc((size_t)n_tiles * 4));
    CALLCHK(d_grand.alloc(4));
    CALLCHK(h->clock.mark(2, st));
    // not scan_offsets: the tiles are scanned by a kernel that forms the flags from the grid and the marks as it reads them
    CALLCHK(launch(k_tsdf_brick_scan, dim3((unsigned)n_tiles), dim3(kScanBlock), st, h->d_grid, d_flags, n_grid, d_excl.as<int>(), d_totals.as<int>()));
    CALLCHK(launch(k_scan_totals<Sum>, dim3(1), dim3(kScanBlock), st, d_totals.as<int>(), n_tiles, 0, d_grand.as<int>()));
    CALLCHK(h->clock.mark(3, st));
    int grand = 0;
    CALLCHK(hipMemcpyAsync(&grand, d_grand.p, 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    CALLCHK(h->clock.ms(2, 3, &ms));
    h->alloc_ms[1] = ms;
    const long long n_new = (long long)grand;   // at most 2^24 grid cells: the int cannot overflow, the comparison is in 64 bits
    if (n_new > h->max_bricks)
        return call_fail(-3, "tsdf allocate: " + std::to_string(n_new) + " bricks, max_bricks is " + std::to_string(h->max_bricks) + "; nothing was allocated");
    if (n_new == h->n_bricks) return 0;   // the set only grows: no new brick
    TsdfPool pool(st);
    const int rc = pool.alloc(h, (size_t)n_new);
    if (rc) return rc;
    CALLCHK(h->clock.mark(4, st));
    if (h->n_bricks > 0)   // the colours, old and new: null without colour
        CALLCHK(launch(k_tsdf_brick_move, dim3((unsigned)h->n_bricks), dim3(kBrickVox), st, h->d_list, h->d_grid, d_flags, d_excl.as<int>(), d_totals.as<int>(), h->d_sum,
                       h->d_weight, h->with_color ? h->d_color : nullptr, pool.sum.as<float>(), pool.weight.as<int32_t>(), pool.color.as<uint4>()));
    CALLCHK(launch(k_tsdf_brick_commit, dim3((unsigned)((n_grid + 255) / 256)), dim3(256), st, n_grid, h->d_grid, d_flags, d_excl.as<int>(), d_totals.as<int>(),
                   pool.list.as<int32_t>()));
    CALLCHK(h->clock.mark(5, st));
    std::vector<int32_t> list((size_t)n_new);
    CALLCHK(hipMemcpyAsync(list.data(), pool.list.p, (size_t)n_new * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(h->clock.ms(4, 5, &ms));
    h->alloc_ms[1] += ms;
    pool.swap_into(h);
    h->list.swap(list);
    h->n_bricks = n_new;
    return 0;
}

int mpmvs_tsdf_allocate(mpmvs_tsdf* h, int n_views, const mpmvs_camera* cams, const float* const* depths) {
    if (!h || n_views < 0) return call_fail(-2, "tsdf allocate: bad argument");
    if (!h->sparse) return call_fail(-2, "tsdf allocate: the volume is dense (mpmvs_tsdf_create_sparse makes a brick-sparse one)");
    if (n_views == 0) return 0;
    const int rc = tsdf_check_views("tsdf allocate", n_views, cams, depths, nullptr);
    if (rc) return rc;
    const int rc2 = tsdf_ready(h);
    if (rc2) return rc2;
    h->alloc_ms[0] = h->alloc_ms[1] = 0.0f;
    const hipStream_t st = h->stream;
    Scratch d_flags(st);
    CALLCHK(d_flags.alloc(h->n_grid * 4));
    CALLCHK(hipMemsetAsync(d_flags.p, 0, h->n_grid * 4, st));
    // per chunk: the depth maps up, one marking launch (blockIdx.y: the view), its time added to alloc_ms[0]
    const int rc3 = tsdf_for_chunks(n_views, cams, [&](int v0, int v1) {
        TsdfChunk c(st);
        const int rc4 = c.upload(h, v0, v1, cams, depths, nullptr, 0);
        if (rc4) return rc4;
        size_t most = 0;
        for (int v = 0; v < c.A.n; ++v) most = std::max(most, (size_t)c.A.v[v].w * (size_t)c.A.v[v].h);
        return tsdf_timed(h, &h->alloc_ms[0], [&] {
            CALLCHK(launch(k_tsdf_alloc_mark, dim3((unsigned)((most + 255) / 256), (unsigned)c.A.n), dim3(256), st, h->V, tsdf_bricks(h), h->alloc, c.A, d_flags.as<uint32_t>()));
            return 0;
        });
    });
    return rc3 ? rc3 : tsdf_commit(h, d_flags.as<uint32_t>());
}

long long mpmvs_tsdf_bricks(mpmvs_tsdf* h, int32_t** coords) {
    if (!h) return call_fail(-2, "tsdf bricks: bad argument");
    if (!h->sparse) return call_fail(-2, "tsdf bricks: the volume is dense");
    if (!coords) return h->n_bricks;
    int32_t* c = nullptr;
    if (h->n_bricks > 0) {
        c = (int32_t*)std::malloc((size_t)h->n_bricks * 12);
        if (!c) return call_fail(-100, "tsdf bricks: out of host memory");
        const TsdfBricks B = tsdf_bricks(h);
        for (long long r = 0; r < h->n_bricks; ++r) {
            int I, J, K;
            tsdf_brick_coords(B, h->list[(size_t)r], I, J, K);
            c[3 * r] = I; c[3 * r + 1] = J; c[3 * r + 2] = K;
        }
    }
    *coords = c;
    return h->n_bricks;
}

int mpmvs_tsdf_get_bricks(mpmvs_tsdf* h, float* sum, int32_t* weight, uint32_t* color4) {
    if (!h || !sum || !weight) return call_fail(-2, "tsdf get_bricks: bad argument");
    if (!h->sparse) return call_fail(-2, "tsdf get_bricks: the volume is dense (mpmvs_tsdf_get reads it)");
    if (color4 && !h->with_color) return call_fail(-2, "tsdf get_bricks: the volume has no colour");
    if (h->n_bricks == 0) return 0;
    const int rc = tsdf_ready(h);
    if (rc) return rc;
    const size_t n = (size_t)h->n_bricks * kBrickVox;
    CALLCHK(hipMemcpyAsync(sum, h->d_sum, n * 4, hipMemcpyDeviceToHost, h->stream));
    CALLCHK(hipMemcpyAsync(weight, h->d_weight, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (color4) CALLCHK(hipMemcpyAsync(color4, h->d_color, n * 16, hipMemcpyDeviceToHost, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int mpmvs_tsdf_set_bricks(mpmvs_tsdf* h, long long n, const int32_t* coords, const float* sum, const int32_t* weight, const uint32_t* color4) {
    if (!h || n < 0 || (n > 0 && (!coords || !sum || !weight))) return call_fail(-2, "tsdf set_bricks: bad argument");
    if (!h->sparse) return call_fail(-2, "tsdf set_bricks: the volume is dense (mpmvs_tsdf_set writes it)");
    if (color4 && !h->with_color) return call_fail(-2, "tsdf set_bricks: the volume has no colour");
    if (n > h->max_bricks) return call_fail(-3, "tsdf set_bricks: " + std::to_string(n) + " bricks, max_bricks is " + std::to_string(h->max_bricks));
    std::vector<int32_t> list((size_t)n);
    for (long long r = 0; r < n; ++r) {
        const int32_t I = coords[3 * r], J = coords[3 * r + 1], K = coords[3 * r + 2];
        if (I < 0 || I >= h->bx || J < 0 || J >= h->by || K < 0 || K >= h->bz) return call_fail(-2, "tsdf set_bricks: brick " + std::to_string(r) + " is outside the brick grid");
        list[(size_t)r] = (K * h->by + J) * h->bx + I;
        if (r > 0 && list[(size_t)r] <= list[(size_t)r - 1])
            return call_fail(-2, "tsdf set_bricks: the bricks must ascend strictly by linear index (brick " + std::to_string(r) + " does not)");
    }
    const int rc = tsdf_ready(h);
    if (rc) return rc;
    const hipStream_t st = h->stream;
    std::vector<int32_t> grid(h->n_grid, -1);
    for (long long r = 0; r < n; ++r) grid[(size_t)list[(size_t)r]] = (int32_t)r;
    CALLCHK(hipMemcpyAsync(h->d_grid, grid.data(), h->n_grid * 4, hipMemcpyHostToDevice, st));
    TsdfPool pool(st);
    if (n > 0) {
        const int rc2 = pool.alloc(h, (size_t)n);
        if (rc2) return rc2;
        const size_t e = (size_t)n * kBrickVox;
        CALLCHK(hipMemcpyAsync(pool.list.p, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        CALLCHK(hipMemcpyAsync(pool.sum.p, sum, e * 4, hipMemcpyHostToDevice, st));
        CALLCHK(hipMemcpyAsync(pool.weight.p, weight, e * 4, hipMemcpyHostToDevice, st));
        if (color4) CALLCHK(hipMemcpyAsync(pool.color.p, color4, e * 16, hipMemcpyHostToDevice, st));
        TsdfBricks B = tsdf_bricks(h);
        B.list = pool.list.as<int32_t>();
        CALLCHK(launch(k_tsdf_brick_clip, dim3((unsigned)n), dim3(kBrickVox), st, h->V, B, pool.sum.as<float>(), pool.weight.as<int32_t>(),
                       pool.color.as<uint4>()));   // null without colour
    }
    CALLCHK(hipStreamSynchronize(st));
    pool.swap_into(h);
    h->list.swap(list);
    h->n_bricks = n;
    return 0;
}

int mpmvs_tsdf_sparse_stats(const mpmvs_tsdf* h, long long info[4], float ms[2]) {
    if (!h || !info || !ms) return call_fail(-2, "tsdf sparse_stats: bad argument");
    if (!h->sparse) return call_fail(-2, "tsdf sparse_stats: the volume is dense");
    info[0] = h->n_bricks;
    info[1] = h->max_bricks;
    info[2] = (long long)h->n_grid;
    info[3] = (h->d_grid ? (long long)h->n_grid * 4 : 0) + h->n_bricks * (4 + (long long)kBrickVox * (h->with_color ? 24 : 8));
    ms[0] = h->alloc_ms[0];
    ms[1] = h->alloc_ms[1];
    return 0;
}

// ---- an indexed triangle mesh: components, vertex normals, select (statements 1 to 3 of include/mpmvs.h) ----
constexpr long long kMeshMax = 1ll << 30;

int mpmvs_mesh_create(int device, long long n, const float* xyz, const unsigned char* rgb, long long m, const int32_t* tri, mpmvs_mesh** out) {
    if (!out) return call_fail(-2, "mesh create: bad argument");
    if (n < 0 || m < 0) return call_fail(-2, "mesh create: a negative count");
    if ((n > 0 && !xyz) || (m > 0 && !tri)) return call_fail(-2, "mesh create: vertices or triangles missing");
    if (device < 0) return call_fail(-2, "mesh create: negative device");
    if (n > kMeshMax || m > kMeshMax) return call_fail(-3, "mesh create: more than 2^30 vertices or triangles");
    for (long long k = 0; k < 3 * m; ++k)
        if (tri[k] < 0 || (long long)tri[k] >= n)
            return call_fail(-2, "mesh create: triangle " + std::to_string(k / 3) + " names vertex " + std::to_string(tri[k]) + ", outside [0, " + std::to_string(n) + ")");
    mpmvs_mesh* h = new mpmvs_mesh;
    h->device = device;
    h->n = n;
    h->m = m;
    h->with_color = rgb != nullptr;
    if (n > 0) h->xyz.assign(xyz, xyz + 3 * n);
    if (n > 0 && rgb) h->rgb.assign(rgb, rgb + 3 * n);
    if (m > 0) h->tri.assign(tri, tri + 3 * m);
    h->scale = mesh_scale(h->xyz.data(), n, m);
    h->n_fin = cloud_bbox(n, h->xyz.data(), h->mn, h->mx);
    for (long long t = 0; t < m; ++t) {   // the triangles that take part in mpmvs_surface_distance
        double P[9];
        if (surface_corners(h->xyz.data(), h->tri.data(), (size_t)t, P)) ++h->m_fin;
    }
    *out = h;
    return 0;
}

void mpmvs_mesh_destroy(mpmvs_mesh* h) {
    if (!h) return;
    if (h->stream || h->d_xyz) {
        (void)enter_device(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void* p : {(void*)h->d_xyz, (void*)h->d_rgb, (void*)h->d_tri})
            if (p) (void)pool_free(p);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;   // the clock goes here: the stream has been waited for
}

static dim3 mesh_blocks(size_t count) { return dim3((unsigned)((count + 255) / 256)); }

int mpmvs_mesh_components(mpmvs_mesh* h, int32_t* out_label, int32_t* out_verts, int32_t* out_tris, long long counts[4]) {
    if (!h || (h->n > 0 && !out_label)) return call_fail(-2, "mesh components: bad argument");
    h->ms[0] = h->ms[1] = h->ms[2] = 0.0f;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (m == 0) {   // nothing is joined: answered here
        for (size_t v = 0; v < n; ++v) {
            out_label[v] = (int32_t)v;
            if (out_verts) out_verts[v] = 1;
            if (out_tris) out_tris[v] = 0;
        }
        if (counts) counts[0] = 0, counts[1] = h->n, counts[2] = 0, counts[3] = -1;
        return 0;
    }
    const int rc = mesh_ready(h);
    if (rc) return rc;
    const hipStream_t st = h->stream;
    const int ni = (int)h->n, mi = (int)h->m;
    Scratch d_parent(st), d_label(st), d_cnt(st), d_verts(st), d_tris(st);
    CALLCHK(d_parent.alloc(n * 4));
    CALLCHK(d_label.alloc(n * 4));
    CALLCHK(d_cnt.alloc(n * 8));    // the vertex counts, then the triangle counts
    CALLCHK(d_verts.alloc(n * 4));
    CALLCHK(d_tris.alloc(n * 4));
    int* const vcnt = d_cnt.as<int>();
    int* const tcnt = vcnt + n;
    const dim3 blk(256);
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(launch(k_mesh_cc_init, mesh_blocks(n), blk, st, ni, d_parent.as<int>()));
    CALLCHK(launch(k_mesh_cc_hook, mesh_blocks(m), blk, st, mi, h->d_tri, d_parent.as<int>()));
    CALLCHK(h->clock.mark(1, st));
    CALLCHK(launch(k_cc_flatten, mesh_blocks(n), blk, st, ni, d_parent.as<int>(), d_label.as<int32_t>()));
    CALLCHK(h->clock.mark(2, st));
    CALLCHK(hipMemsetAsync(d_cnt.p, 0, n * 8, st));
    CALLCHK(launch(k_cc_count, mesh_blocks(n), blk, st, ni, d_label.as<int32_t>(), vcnt));
    CALLCHK(launch(k_mesh_tri_count, mesh_blocks(m), blk, st, mi, h->d_tri, d_label.as<int32_t>(), tcnt));
    CALLCHK(launch(k_cc_gather, mesh_blocks(n), blk, st, ni, d_label.as<int32_t>(), vcnt, d_verts.as<int32_t>()));
    CALLCHK(launch(k_cc_gather, mesh_blocks(n), blk, st, ni, d_label.as<int32_t>(), tcnt, d_tris.as<int32_t>()));
    CALLCHK(h->clock.mark(3, st));
    std::vector<int32_t> tris_host;   // the counts need the triangle counts whether the caller wants them or not
    if (counts && !out_tris) tris_host.resize(n);
    int32_t* const tris = out_tris ? out_tris : tris_host.data();
    CALLCHK(hipMemcpyAsync(out_label, d_label.p, n * 4, hipMemcpyDeviceToHost, st));
    if (out_verts) CALLCHK(hipMemcpyAsync(out_verts, d_verts.p, n * 4, hipMemcpyDeviceToHost, st));
    if (out_tris || counts) CALLCHK(hipMemcpyAsync(tris, d_tris.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) CALLCHK(h->clock.ms(k, k + 1, &h->ms[k]));
    if (counts) {
        // a vertex that a triangle names lies in a component with that triangle; one that none names is alone with 0 triangles
        long long comps = 0, unnamed = 0, best = 0, best_label = -1;
        for (size_t v = 0; v < n; ++v) {
            if (tris[v] == 0) ++unnamed;
            if (out_label[v] != (int32_t)v || tris[v] == 0) continue;
            ++comps;
            if (tris[v] > best) best = tris[v], best_label = (long long)v;   // ascending labels: among equals the smallest stays
        }
        counts[0] = comps, counts[1] = unnamed, counts[2] = best, counts[3] = best_label;
    }
    return 0;
}

int mpmvs_mesh_normals(mpmvs_mesh* h, float* out_normals, long long* n_defined) {
    if (!h || (h->n > 0 && !out_normals)) return call_fail(-2, "mesh normals: bad argument");
    h->ms[3] = h->ms[4] = 0.0f;
    const size_t n = (size_t)h->n;
    if (n == 0 || h->scale == 0.0) {   // no triangle, no finite vertex or no extent: every normal is zero
        if (n > 0) std::memset(out_normals, 0, n * 12);
        if (n_defined) *n_defined = 0;
        return 0;
    }
    const int rc = mesh_ready(h);
    if (rc) return rc;
    const hipStream_t st = h->stream;
    Scratch d_sum(st), d_out(st), d_def(st);
    CALLCHK(d_sum.alloc(n * 24));
    CALLCHK(d_out.alloc(n * 12));
    CALLCHK(d_def.alloc(4));
    CALLCHK(hipMemsetAsync(d_def.p, 0, 4, st));
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(hipMemsetAsync(d_sum.p, 0, n * 24, st));
    CALLCHK(launch(k_mesh_nrm_accum, mesh_blocks((size_t)h->m), dim3(256), st, (int)h->m, h->d_xyz, h->d_tri, h->scale, d_sum.as<long long>()));
    CALLCHK(h->clock.mark(1, st));
    CALLCHK(launch(k_mesh_nrm_finish, mesh_blocks(n), dim3(256), st, (int)h->n, d_sum.as<long long>(), d_out.as<float>(), d_def.as<int>()));
    CALLCHK(h->clock.mark(2, st));
    int defined = 0;
    CALLCHK(hipMemcpyAsync(out_normals, d_out.p, n * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(&defined, d_def.p, 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) CALLCHK(h->clock.ms(k, k + 1, &h->ms[3 + k]));
    if (n_defined) *n_defined = defined;
    return 0;
}

// the device half of mpmvs_mesh_select; the host buffers are allocated once the counts are known and handed over on success only
static long long mesh_select_device(mpmvs_mesh* h, const unsigned char* keep, int drop, float** xyz, unsigned char** rgb, int32_t** tri, int32_t** src, long long* m_out) {
    const hipStream_t st = h->stream;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    const int ni = (int)h->n, mi = (int)h->m;
    const size_t v_tiles = (n + kScanBlock - 1) / kScanBlock, t_tiles = (m + kScanBlock - 1) / kScanBlock;
    Scratch d_keep(st), d_vflag(st), d_tflag(st), d_vexcl(st), d_texcl(st), d_tiles(st), d_grand(st);
    CALLCHK(d_keep.alloc(n));
    CALLCHK(d_vflag.alloc(n * 4));
    CALLCHK(d_tflag.alloc(m * 4));
    CALLCHK(d_vexcl.alloc(n * 4));
    CALLCHK(d_texcl.alloc(m * 4));
    CALLCHK(d_tiles.alloc((v_tiles + t_tiles) * 4));
    CALLCHK(d_grand.alloc(8));
    int* const vtile = d_tiles.as<int>();
    int* const ttile = vtile + v_tiles;
    int* const grand = d_grand.as<int>();
    CALLCHK(hipMemcpyAsync(d_keep.p, keep, n, hipMemcpyHostToDevice, st));
    CALLCHK(hipMemsetAsync(d_grand.p, 0, 8, st));
    const dim3 blk(256);
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(launch(k_mesh_sel_verts, mesh_blocks(n), blk, st, ni, d_keep.as<unsigned char>(), drop, d_vflag.as<int>()));
    if (m > 0) CALLCHK(launch(k_mesh_sel_tris, mesh_blocks(m), blk, st, mi, h->d_tri, d_keep.as<unsigned char>(), drop, d_tflag.as<int>(), d_vflag.as<int>()));
    CALLCHK(h->clock.mark(1, st));
    // the emit kernels add the tile offsets themselves
    CALLCHK(scan_offsets(st, d_vflag.as<int>(), ni, d_vexcl.as<int>(), vtile, grand, false));
    if (m > 0) CALLCHK(scan_offsets(st, d_tflag.as<int>(), mi, d_texcl.as<int>(), ttile, grand + 1, false));
    CALLCHK(h->clock.mark(2, st));
    int g[2] = {0, 0};
    CALLCHK(hipMemcpyAsync(g, d_grand.p, 8, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) CALLCHK(h->clock.ms(k, k + 1, &h->ms[5 + k]));
    const size_t nv = (size_t)g[0], nt = (size_t)g[1];
    if (nv == 0) return 0;   // then nt == 0 too: a kept triangle keeps its vertices
    Scratch d_xyz(st), d_rgb(st), d_tri(st), d_src(st);
    CALLCHK(d_xyz.alloc(nv * 12));
    if (h->with_color) CALLCHK(d_rgb.alloc(nv * 3));
    CALLCHK(d_tri.alloc(nt * 12));
    CALLCHK(d_src.alloc(nv * 4));
    CALLCHK(h->clock.mark(3, st));
    CALLCHK(launch(k_mesh_emit_verts, mesh_blocks(n), blk, st, ni, h->d_xyz, h->with_color ? h->d_rgb : nullptr, d_vflag.as<int>(), d_vexcl.as<int>(), vtile,
                   d_xyz.as<float>(), d_rgb.as<unsigned char>(), d_src.as<int32_t>()));
    if (nt > 0)
        CALLCHK(launch(k_mesh_emit_tris, mesh_blocks(m), blk, st, mi, h->d_tri, d_tflag.as<int>(), d_texcl.as<int>(), ttile, d_vexcl.as<int>(), vtile, d_tri.as<int32_t>()));
    CALLCHK(h->clock.mark(4, st));
    HostOut out;
    float* hx = out.take<float>(nv * 3);
    int32_t* ht = nt ? out.take<int32_t>(nt * 3) : nullptr;
    unsigned char* hc = h->with_color ? out.take<unsigned char>(nv * 3) : nullptr;
    int32_t* hs = src ? out.take<int32_t>(nv) : nullptr;
    if (!hx || (nt && !ht) || (h->with_color && !hc) || (src && !hs)) return call_fail(-100, "mesh select: out of host memory");
    CALLCHK(hipMemcpyAsync(hx, d_xyz.p, nv * 12, hipMemcpyDeviceToHost, st));
    if (ht) CALLCHK(hipMemcpyAsync(ht, d_tri.p, nt * 12, hipMemcpyDeviceToHost, st));
    if (hc) CALLCHK(hipMemcpyAsync(hc, d_rgb.p, nv * 3, hipMemcpyDeviceToHost, st));
    if (hs) CALLCHK(hipMemcpyAsync(hs, d_src.p, nv * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(h->clock.ms(3, 4, &h->ms[7]));
    out.keep();
    *xyz = hx;
    *tri = ht;
    *rgb = hc;
    if (src) *src = hs;
    *m_out = (long long)nt;
    return (long long)nv;
}

long long mpmvs_mesh_select(mpmvs_mesh* h, const unsigned char* keep, int drop_unreferenced, float** out_xyz, unsigned char** out_rgb, int32_t** out_tri,
                            int32_t** out_src, long long* m_out) {
    if (!h || !out_xyz || !out_tri || !m_out || (h->n > 0 && !keep)) return call_fail(-2, "mesh select: bad argument");
    if (h->with_color && !out_rgb) return call_fail(-2, "mesh select: a mesh with colour needs out_rgb");
    if (!h->with_color && out_rgb) return call_fail(-2, "mesh select: the mesh has no colour");
    float* xyz = nullptr;
    unsigned char* rgb = nullptr;
    int32_t *tri = nullptr, *src = nullptr;
    long long nt = 0, nv = 0;
    h->ms[5] = h->ms[6] = h->ms[7] = 0.0f;
    if (h->n > 0 && !(drop_unreferenced && h->m == 0)) {   // else nothing can be kept: nothing is launched
        const int rc = mesh_ready(h);
        if (rc) return rc;
        nv = mesh_select_device(h, keep, drop_unreferenced != 0, &xyz, &rgb, &tri, out_src ? &src : nullptr, &nt);
        if (nv < 0) return nv;
    }
    *out_xyz = xyz;
    *out_tri = tri;
    if (out_rgb) *out_rgb = rgb;
    if (out_src) *out_src = src;
    *m_out = nt;
    return nv;
}

int mpmvs_mesh_pass_ms(const mpmvs_mesh* h, float ms[8]) {
    if (!h || !ms) return call_fail(-2, "mesh pass_ms: bad argument");
    std::memcpy(ms, h->ms, sizeof h->ms);
    return 0;
}

// ---- simplification by vertex clustering (statement 4 of include/mpmvs.h) -------------------------------------
// the host buffers of the result, as the entry point hands them out
struct SimpOut {
    HostOut mem;
    float* xyz = nullptr;
    unsigned char *rgb = nullptr, *placed = nullptr;
    int32_t *tri = nullptr, *count = nullptr, *src = nullptr;
};
static const ClusterNames kSimpNames = {"mesh simplify", "vertices", "cell", "clusters"};

// the device half of mpmvs_simplify_mesh: n_fin > 0.  class_counts = {alive, non-finite, collapsed}
static long long mesh_simplify_device(mpmvs_mesh* h, const VoxelGrid& g, int slots_log2, int placement, SimpOut& out, int32_t* out_cluster_of, bool want_count,
                                      bool want_placed, bool want_src, long long* m_out, long long class_counts[3]) {
    const hipStream_t st = h->stream;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    const int mi = (int)h->m;
    const dim3 blk(256);
    float* const ms = h->simp_ms;

    // ---- clusters: the passes of mpmvs_cloud_voxel_downsample on the resident vertices, then the quadrics between accumulate and finish
    // Declared before every other buffer, so that its clock goes last, after the stream has been waited for.  The caller's marks on
    // it: 8 quadric end, 9 place end, 10 classify end, 11 / 12 insert begin / end, 13 owner + scan end, 14 / 15 emit begin / end
    Clusters cl(st, kSimpNames, false);
    auto& clock = cl.clock;
    if (cl.mark(h->d_xyz, (int)h->n, h->n_fin, slots_log2, g)) return -100;
    const int nci = cl.count;
    const size_t nc = (size_t)nci;
    Scratch d_qrt(st), d_placed(st);
    if (placement == 1) CALLCHK(d_qrt.alloc(nc * kSimpSums * 8));
    CALLCHK(d_placed.alloc(nc));
    CALLCHK(hipMemsetAsync(d_placed.p, 0, nc, st));
    if (cl.number_and_accumulate(nullptr, h->with_color ? h->d_rgb : nullptr, true)) return -100;
    const int32_t* const d_cluster_of = cl.cluster_of.as<int32_t>();
    if (placement == 1 && m > 0) {   // from mark 6, the end of accumulate
        CALLCHK(hipMemsetAsync(d_qrt.p, 0, nc * kSimpSums * 8, st));
        CALLCHK(launch(k_simp_quadric, mesh_blocks(m), blk, st, mi, h->d_xyz, h->d_tri, g, d_cluster_of, d_qrt.as<unsigned long long>()));
    }
    CALLCHK(clock.mark(8, st));
    if (cl.finish()) return -100;
    if (placement == 1 && m > 0)   // without a triangle no cluster has a plane: placed stays 0 everywhere
        CALLCHK(launch(k_simp_place, mesh_blocks(nc), blk, st, nci, h->d_xyz, cl.out_first.as<int32_t>(), cl.out_count.as<int32_t>(), g, cl.S,
                       d_qrt.as<unsigned long long>(), cl.out_xyz.as<float>(), d_placed.as<unsigned char>()));
    CALLCHK(clock.mark(9, st));

    // ---- triangles: classes and keys, the duplicate filter, the scan of the kept flags, the emit
    Scratch d_cls(st), d_key(st), d_class(st), d_table(st), d_kept(st), d_excl(st), d_ttile(st), d_grand(st), d_tri(st), d_src(st);
    int cc[3] = {0, 0, 0};
    size_t nt = 0;
    if (m > 0) {
        CALLCHK(d_cls.alloc(m));
        CALLCHK(d_key.alloc(m * 12));
        CALLCHK(d_class.alloc(12));
        CALLCHK(hipMemsetAsync(d_class.p, 0, 12, st));
        CALLCHK(launch(k_simp_classify, mesh_blocks(m), blk, st, mi, h->d_tri, d_cluster_of, d_cls.as<unsigned char>(), d_key.as<int32_t>(), d_class.as<int>()));
        CALLCHK(clock.mark(10, st));
        CALLCHK(hipMemcpyAsync(cc, d_class.p, 12, hipMemcpyDeviceToHost, st));
        CALLCHK(hipStreamSynchronize(st));
        if (cc[0] < 0 || cc[1] < 0 || cc[2] < 0 || (long long)cc[0] + cc[1] + cc[2] != h->m) return call_fail(-100, "mesh simplify: the classes do not add up to the triangles");
    }
    if (cc[0] > 0) {
        const int tl2 = simp_slots_log2(cc[0]);
        const size_t tslots = (size_t)1 << tl2;
        CALLCHK(d_table.alloc(tslots * 4));
        CALLCHK(d_kept.alloc(m * 4));
        CALLCHK(d_excl.alloc(m * 4));
        CALLCHK(d_ttile.alloc((m + kScanBlock - 1) / kScanBlock * 4));
        CALLCHK(d_grand.alloc(4));
        CALLCHK(clock.mark(11, st));
        CALLCHK(hipMemsetAsync(d_table.p, 0xff, tslots * 4, st));
        CALLCHK(launch(k_simp_insert, mesh_blocks(m), blk, st, mi, d_cls.as<unsigned char>(), d_key.as<int32_t>(), (uint32_t)(tslots - 1), d_table.as<uint32_t>()));
        CALLCHK(clock.mark(12, st));
        CALLCHK(hipMemsetAsync(d_kept.p, 0, m * 4, st));
        CALLCHK(launch(k_simp_owner, mesh_blocks(tslots), blk, st, (uint32_t)tslots, d_table.as<uint32_t>(), d_kept.as<int>()));
        CALLCHK(scan_offsets(st, d_kept.as<int>(), mi, d_excl.as<int>(), d_ttile.as<int>(), d_grand.as<int>(), false));   // k_simp_emit adds the tile offsets
        CALLCHK(clock.mark(13, st));
        int kept = 0;
        CALLCHK(hipMemcpyAsync(&kept, d_grand.p, 4, hipMemcpyDeviceToHost, st));
        CALLCHK(hipStreamSynchronize(st));
        if (kept <= 0 || kept > cc[0]) return call_fail(-100, "mesh simplify: the device kept " + std::to_string(kept) + " of " + std::to_string(cc[0]) + " alive triangles");
        nt = (size_t)kept;
        CALLCHK(d_tri.alloc(nt * 12));
        CALLCHK(d_src.alloc(nt * 4));
        CALLCHK(clock.mark(14, st));
        CALLCHK(launch(k_simp_emit, mesh_blocks(m), blk, st, mi, h->d_tri, d_cluster_of, d_kept.as<int>(), d_excl.as<int>(), d_ttile.as<int>(), d_tri.as<int32_t>(),
                       d_src.as<int32_t>()));
        CALLCHK(clock.mark(15, st));
    }

    out.xyz = out.mem.take<float>(nc * 3);
    if (h->with_color) out.rgb = out.mem.take<unsigned char>(nc * 3);
    if (want_count) out.count = out.mem.take<int32_t>(nc);
    if (want_placed) out.placed = out.mem.take<unsigned char>(nc);
    if (nt) out.tri = out.mem.take<int32_t>(nt * 3);
    if (nt && want_src) out.src = out.mem.take<int32_t>(nt);
    if (!out.xyz || (h->with_color && !out.rgb) || (want_count && !out.count) || (want_placed && !out.placed) || (nt && !out.tri) || (nt && want_src && !out.src))
        return call_fail(-100, "mesh simplify: out of host memory");
    CALLCHK(hipMemcpyAsync(out.xyz, cl.out_xyz.p, nc * 12, hipMemcpyDeviceToHost, st));
    if (out.rgb) CALLCHK(hipMemcpyAsync(out.rgb, cl.out_rgb.p, nc * 3, hipMemcpyDeviceToHost, st));
    if (out.count) CALLCHK(hipMemcpyAsync(out.count, cl.out_count.p, nc * 4, hipMemcpyDeviceToHost, st));
    if (out.placed) CALLCHK(hipMemcpyAsync(out.placed, d_placed.p, nc, hipMemcpyDeviceToHost, st));
    if (out.tri) CALLCHK(hipMemcpyAsync(out.tri, d_tri.p, nt * 12, hipMemcpyDeviceToHost, st));
    if (out.src) CALLCHK(hipMemcpyAsync(out.src, d_src.p, nt * 4, hipMemcpyDeviceToHost, st));
    if (out_cluster_of) CALLCHK(hipMemcpyAsync(out_cluster_of, d_cluster_of, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float a = 0.0f, b = 0.0f;
    CALLCHK(clock.ms(0, 3, &a));
    CALLCHK(clock.ms(4, 5, &b));
    ms[0] = a + b;   // the clustering passes up to the numbering
    CALLCHK(clock.ms(5, 6, &ms[1]));
    if (placement == 1 && m > 0) CALLCHK(clock.ms(6, 8, &ms[2]));
    CALLCHK(clock.ms(8, 9, &ms[3]));
    if (m > 0) CALLCHK(clock.ms(9, 10, &ms[4]));
    if (cc[0] > 0) {
        CALLCHK(clock.ms(11, 12, &a));
        ms[4] += a;
        CALLCHK(clock.ms(12, 13, &ms[5]));
        CALLCHK(clock.ms(14, 15, &ms[6]));
    }
    *m_out = (long long)nt;
    class_counts[0] = cc[0], class_counts[1] = cc[1], class_counts[2] = cc[2];
    return (long long)nc;
}

long long mpmvs_simplify_mesh(mpmvs_mesh* h, float cell, int placement, float** out_xyz, unsigned char** out_rgb, int32_t** out_tri, long long* m_out,
                              int32_t* out_cluster_of, int32_t** out_count, unsigned char** out_placed, int32_t** out_tri_src, long long counts[3]) {
    if (!h || !out_xyz || !out_tri || !m_out) return call_fail(-2, "mesh simplify: bad argument");
    if (!std::isfinite(cell) || !(cell > 0.0f)) return call_fail(-2, "mesh simplify: the cell size must be finite and positive");
    if (placement != 0 && placement != 1) return call_fail(-2, "mesh simplify: placement must be 0 (mean) or 1 (quadric)");
    if (h->with_color && !out_rgb) return call_fail(-2, "mesh simplify: a mesh with colour needs out_rgb");
    if (!h->with_color && out_rgb) return call_fail(-2, "mesh simplify: the mesh has no colour");
    int slots_log2 = 0;
    VoxelGrid g;
    if (cluster_refusal(kSimpNames, h->n_fin, h->mn, h->mx, cell, &slots_log2, &g)) return -3;
    SimpOut out;
    long long nc = 0, nt = 0, cc[3] = {0, h->m, 0};   // without a finite vertex every triangle names a non-finite one
    std::memset(h->simp_ms, 0, sizeof h->simp_ms);
    if (h->n_fin > 0) {
        const int rc = mesh_ready(h);
        if (rc) return rc;
        nc = mesh_simplify_device(h, g, slots_log2, placement, out, out_cluster_of, out_count != nullptr, out_placed != nullptr, out_tri_src != nullptr, &nt, cc);
        if (nc < 0) return nc;
    } else if (out_cluster_of) {
        for (long long v = 0; v < h->n; ++v) out_cluster_of[v] = -1;
    }
    *out_xyz = out.xyz;
    *out_tri = out.tri;
    if (out_rgb) *out_rgb = out.rgb;
    if (out_count) *out_count = out.count;
    if (out_placed) *out_placed = out.placed;
    if (out_tri_src) *out_tri_src = out.src;
    *m_out = nt;
    if (counts) counts[0] = cc[1], counts[1] = cc[2], counts[2] = cc[0] - nt;
    out.mem.keep();
    return nc;
}

int mpmvs_simplify_mesh_ms(const mpmvs_mesh* h, float ms[7]) {
    if (!h || !ms) return call_fail(-2, "mesh simplify_ms: bad argument");
    std::memcpy(ms, h->simp_ms, sizeof h->simp_ms);
    return 0;
}

// ---- sampling the surface (statement 6 of include/mpmvs.h; pm_surface.hpp) ------------------------------------
// the device half of mpmvs_surface_sample: m > 0.  The host copy of the mesh is gone after the first upload, so the two -3 refusals
// are found here, after the count pass.
static long long surface_sample_device(mpmvs_mesh* h, float spacing, bool want_normals, float** xyz, int32_t** tri_of, unsigned char** rgb, float** normals) {
    const hipStream_t st = h->stream;
    const size_t m = (size_t)h->m;
    const int mi = (int)h->m;
    const double h_s = (double)spacing;
    const dim3 blk(256);
    PassClock<4> clock;   // before the buffers: they wait for the stream when they go
    Scratch d_cnt(st), d_off(st), d_tsum(st), d_tot(st);
    CALLCHK(d_cnt.alloc(m * 4));
    CALLCHK(d_off.alloc(m * 4));
    CALLCHK(d_tsum.alloc((m + kScanBlock - 1) / kScanBlock * 4));
    CALLCHK(d_tot.alloc(16));   // the total (64 bits), the first triangle beyond the limit
    unsigned long long tot[2] = {0, ~0ull};
    CALLCHK(hipMemcpyAsync(d_tot.p, tot, 16, hipMemcpyHostToDevice, st));
    CALLCHK(clock.mark(0, st));
    CALLCHK(launch(k_surface_count, mesh_blocks(m), blk, st, mi, h->d_xyz, h->d_tri, h_s, d_cnt.as<int>(), d_tot.as<unsigned long long>(),
                   (uint32_t*)(d_tot.as<unsigned long long>() + 1)));
    CALLCHK(clock.mark(1, st));
    CALLCHK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(clock.ms(0, 1, &h->sample_ms[0]));
    const uint32_t first_bad = (uint32_t)(tot[1] & 0xffffffffull);
    if (first_bad != 0xffffffffu)
        return call_fail(-3, "surface sample: the longest edge of triangle " + std::to_string(first_bad) + " is more than 4096 times the spacing");
    if (tot[0] > (unsigned long long)kSurfaceMaxSamples) return call_fail(-3, "surface sample: " + std::to_string(tot[0]) + " samples, more than 2^30");
    const size_t K = (size_t)tot[0];
    if (K == 0) return 0;
    Scratch d_xyz(st), d_of(st), d_rgb(st), d_nrm(st);
    CALLCHK(d_xyz.alloc(K * 12));
    CALLCHK(d_of.alloc(K * 4));
    if (h->with_color) CALLCHK(d_rgb.alloc(K * 3));
    if (want_normals) CALLCHK(d_nrm.alloc(K * 12));
    CALLCHK(clock.mark(1, st));
    CALLCHK(scan_offsets(st, d_cnt.as<int>(), mi, d_off.as<int>(), d_tsum.as<int>(), nullptr, true));
    CALLCHK(clock.mark(2, st));
    CALLCHK(launch(k_surface_emit, mesh_blocks(K), blk, st, (int)K, h->d_xyz, h->with_color ? h->d_rgb : nullptr, h->d_tri, mi, h_s, d_off.as<int>(),
                   d_xyz.as<float>(), d_of.as<int32_t>(), d_rgb.as<unsigned char>(), d_nrm.as<float>()));
    CALLCHK(clock.mark(3, st));
    HostOut out;
    float* hx = out.take<float>(K * 3);
    int32_t* ho = out.take<int32_t>(K);
    unsigned char* hc = h->with_color ? out.take<unsigned char>(K * 3) : nullptr;
    float* hn = want_normals ? out.take<float>(K * 3) : nullptr;
    if (!hx || !ho || (h->with_color && !hc) || (want_normals && !hn)) return call_fail(-100, "surface sample: out of host memory");
    CALLCHK(hipMemcpyAsync(hx, d_xyz.p, K * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(ho, d_of.p, K * 4, hipMemcpyDeviceToHost, st));
    if (hc) CALLCHK(hipMemcpyAsync(hc, d_rgb.p, K * 3, hipMemcpyDeviceToHost, st));
    if (hn) CALLCHK(hipMemcpyAsync(hn, d_nrm.p, K * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(clock.ms(1, 2, &h->sample_ms[1]));
    CALLCHK(clock.ms(2, 3, &h->sample_ms[2]));
    out.keep();
    *xyz = hx, *tri_of = ho, *rgb = hc, *normals = hn;
    return (long long)K;
}

long long mpmvs_surface_sample(mpmvs_mesh* h, float spacing, float** out_xyz, int32_t** out_tri_of, unsigned char** out_rgb, float** out_normals) {
    if (!h || !out_xyz || !out_tri_of) return call_fail(-2, "surface sample: bad argument");
    if (!std::isfinite(spacing) || !(spacing > 0.0f)) return call_fail(-2, "surface sample: the spacing must be finite and positive");
    if (h->with_color && !out_rgb) return call_fail(-2, "surface sample: a mesh with colour needs out_rgb");
    if (!h->with_color && out_rgb) return call_fail(-2, "surface sample: the mesh has no colour");
    float *xyz = nullptr, *nrm = nullptr;
    int32_t* of = nullptr;
    unsigned char* rgb = nullptr;
    long long K = 0;
    h->sample_ms[0] = h->sample_ms[1] = h->sample_ms[2] = 0.0f;
    if (h->m_fin > 0) {   // else no triangle yields a sample: nothing is launched
        const int rc = mesh_ready(h);
        if (rc) return rc;
        K = surface_sample_device(h, spacing, out_normals != nullptr, &xyz, &of, &rgb, &nrm);
        if (K < 0) return K;
    }
    *out_xyz = xyz;
    *out_tri_of = of;
    if (out_rgb) *out_rgb = rgb;
    if (out_normals) *out_normals = nrm;
    return K;
}

float mpmvs_surface_sample_ms(const mpmvs_mesh* h, float pass_ms[3]) {
    if (!h) return 0.0f;
    if (pass_ms) std::memcpy(pass_ms, h->sample_ms, sizeof h->sample_ms);
    return (h->sample_ms[0] + h->sample_ms[1]) + h->sample_ms[2];
}

// ---- rendering the surface into cameras (statement 7 of include/mpmvs.h; pm_raster.hpp) ----------------------
constexpr size_t kRasterChunkPixels = (size_t)1 << 26;   // a chunk of views ends before its key buffers pass this many pixels (one view always fits)
constexpr unsigned kRasterLargeBlocks = 4096;            // blocks of the large pass; they stride over the list

// MPMVS_RASTER_LARGE=<pixels>: the size of a pair's pixel box above which it goes to the list; read at every call (tests force both
// paths through it)
static int raster_large_threshold() {
    const char* e = std::getenv("MPMVS_RASTER_LARGE");
    if (!e || !*e) return kRasterLargeDefault;
    const long long v = std::strtoll(e, nullptr, 10);
    return v < 0 ? 0 : (v > (1ll << 30) ? (1 << 30) : (int)v);
}

// views [v0, v1) in one launch of each pass (two of the large one); cnt: pairs taking part, covered pixels, listed pairs, pixels of the
// boxes, atomic minima issued, added to
static int surface_render_chunk(mpmvs_mesh* h, int v0, int v1, const mpmvs_camera* cams, int large, float* const* out_depth, int32_t* const* out_tri, long long cnt[5]) {
    const hipStream_t st = h->stream;
    const size_t m = (size_t)h->m;
    size_t total = 0;
    bool any_tri = false;
    for (int v = v0; v < v1; ++v) {
        total += (size_t)cams[v].width * (size_t)cams[v].height;
        any_tri = any_tri || (out_tri && out_tri[v]);
    }
    Scratch d_keys(st), d_depth(st), d_tri(st), d_list(st), d_cnt(st);
    CALLCHK(d_keys.alloc(total * 8));
    CALLCHK(d_depth.alloc(total * 4));
    if (any_tri) CALLCHK(d_tri.alloc(total * 4));
    const size_t cap = m * (size_t)(v1 - v0);            // every pair at most once
    CALLCHK(d_list.alloc(cap * 8));
    CALLCHK(d_cnt.alloc(48));   // listed pairs up to kRasterSplit pixels, above it; pairs taking part, box pixels, atomics; covered pixels
    RasterChunkArgs A;
    std::memset(&A, 0, sizeof A);
    A.n = v1 - v0;
    A.large = large;
    size_t at = 0;
    for (int v = v0; v < v1; ++v) {
        RasterView& V = A.v[v - v0];
        std::memcpy(V.K, cams[v].K, sizeof V.K);
        std::memcpy(V.R, cams[v].R, sizeof V.R);
        std::memcpy(V.t, cams[v].t, sizeof V.t);
        V.w = cams[v].width, V.h = cams[v].height;
        V.keys = d_keys.as<unsigned long long>() + at;
        at += (size_t)V.w * (size_t)V.h;
    }
    unsigned long long* const d_n = d_cnt.as<unsigned long long>();
    CALLCHK(hipMemsetAsync(d_cnt.p, 0, 48, st));
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(launch(k_raster_init, mesh_blocks(total), dim3(256), st, total, d_keys.as<unsigned long long>()));
    CALLCHK(h->clock.mark(1, st));
    CALLCHK(launch(k_raster_small, mesh_blocks(m), dim3(256), st, (int)h->m, h->d_xyz, h->d_tri, A, d_list.as<unsigned long long>(), cap, d_n, d_n + 2));
    CALLCHK(h->clock.mark(2, st));
    for (int split = 0; split < 2; ++split)
        CALLCHK(launch(k_raster_large, dim3(kRasterLargeBlocks), dim3(256), st, h->d_xyz, h->d_tri, A, d_list.as<unsigned long long>(), cap, d_n, split, d_n + 4));
    CALLCHK(h->clock.mark(3, st));
    CALLCHK(launch(k_raster_resolve, mesh_blocks(total), dim3(256), st, total, d_keys.as<unsigned long long>(), d_depth.as<float>(), d_tri.as<int32_t>(), d_n + 5));
    CALLCHK(h->clock.mark(4, st));
    at = 0;
    for (int v = v0; v < v1; ++v) {
        const size_t npix = (size_t)cams[v].width * (size_t)cams[v].height;
        CALLCHK(hipMemcpyAsync(out_depth[v], d_depth.as<float>() + at, npix * 4, hipMemcpyDeviceToHost, st));
        if (out_tri && out_tri[v]) CALLCHK(hipMemcpyAsync(out_tri[v], d_tri.as<int32_t>() + at, npix * 4, hipMemcpyDeviceToHost, st));
        at += npix;
    }
    unsigned long long n[6] = {0, 0, 0, 0, 0, 0};
    CALLCHK(hipMemcpyAsync(n, d_cnt.p, 48, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int p = 0; p < 4; ++p) {
        float ms = 0.0f;
        CALLCHK(h->clock.ms(p, p + 1, &ms));
        h->render_ms[p] += ms;
    }
    cnt[0] += (long long)n[2], cnt[1] += (long long)n[5], cnt[2] += (long long)(n[0] + n[1]), cnt[3] += (long long)n[3], cnt[4] += (long long)n[4];
    return 0;
}

int mpmvs_surface_render_depth(mpmvs_mesh* surface, int n_views, const mpmvs_camera* cams, float* const* out_depth, int32_t* const* out_tri, long long counts[3]) {
    mpmvs_mesh* const h = surface;
    if (!h || n_views < 0) return call_fail(-2, "surface render: bad argument");
    if (n_views == 0) return 0;
    if (!cams || !out_depth) return call_fail(-2, "surface render: bad argument");
    for (int v = 0; v < n_views; ++v) {
        if (!out_depth[v]) return call_fail(-2, "surface render: view " + std::to_string(v) + " has no depth buffer");
        if (cams[v].width <= 0 || cams[v].height <= 0) return call_fail(-2, "surface render: view " + std::to_string(v) + " has a non-positive width or height");
    }
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].width > (1 << 24) || cams[v].height > (1 << 24)) return call_fail(-3, "surface render: view " + std::to_string(v) + " is wider or higher than 2^24");
        if ((long long)cams[v].width * (long long)cams[v].height > (long long)INT32_MAX)
            return call_fail(-3, "surface render: view " + std::to_string(v) + " has more than 2^31 - 1 pixels");
    }
    std::memset(h->render_ms, 0, sizeof h->render_ms);
    h->render_work[0] = h->render_work[1] = 0;
    long long cnt[5] = {0, 0, 0, 0, 0};
    if (h->m_fin == 0) {   // no triangle takes part in any view: answered here
        for (int v = 0; v < n_views; ++v) {
            const size_t npix = (size_t)cams[v].width * (size_t)cams[v].height;
            std::fill(out_depth[v], out_depth[v] + npix, 0.0f);
            if (out_tri && out_tri[v]) std::fill(out_tri[v], out_tri[v] + npix, (int32_t)-1);
        }
    } else {
        const int rc = mesh_ready(h);
        if (rc) return rc;
        const int large = raster_large_threshold();
        for (int v0 = 0; v0 < n_views;) {
            int v1 = v0 + 1;
            size_t pixels = (size_t)cams[v0].width * (size_t)cams[v0].height;
            while (v1 < n_views && v1 - v0 < kRasterChunk && pixels + (size_t)cams[v1].width * (size_t)cams[v1].height <= kRasterChunkPixels) {
                pixels += (size_t)cams[v1].width * (size_t)cams[v1].height;
                ++v1;
            }
            const int rc2 = surface_render_chunk(h, v0, v1, cams, large, out_depth, out_tri, cnt);
            if (rc2) return rc2;
            v0 = v1;
        }
    }
    if (counts) counts[0] = cnt[0], counts[1] = cnt[1], counts[2] = cnt[2];
    h->render_work[0] = cnt[3], h->render_work[1] = cnt[4];
    return 0;
}

float mpmvs_surface_render_ms(const mpmvs_mesh* h, float pass_ms[4]) {
    if (!h) return 0.0f;
    if (pass_ms) std::memcpy(pass_ms, h->render_ms, sizeof h->render_ms);
    return ((h->render_ms[0] + h->render_ms[1]) + h->render_ms[2]) + h->render_ms[3];
}

int mpmvs_surface_render_work(const mpmvs_mesh* h, long long work[2]) {
    if (!h || !work) return call_fail(-2, "surface render_work: bad argument");
    work[0] = h->render_work[0], work[1] = h->render_work[1];
    return 0;
}

}  // extern "C"
