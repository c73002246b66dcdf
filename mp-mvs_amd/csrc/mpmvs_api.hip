// mpmvs_api.hip -- host side of the C ABI declared in include/mpmvs.h: context
// and HBM residency management, uploads (upload_views for both image entries; its host half, the staging
// plan and the row work, is pm_stage.hpp), the Run() launch schedule (reference src/PatchMatch.cu:1188-1254),
// the stateless calls (DeviceCall: fusion -- FuseRun, on the request and rules of pm_fusion_host.hpp --, sky mask, view selection, undistortion), the point-cloud search handle (mpmvs_cloud)
// and the probes used by the parity tests.
//
// HBM layout per context:
//   reference image   (W+40) x (H+40) fp32, replicated apron 20  (window radius <= 20)
//   source images     fp32 format: w x h float4, each packing the 2x2 bilinear footprint of one texel
//                     u8 format (all images 8-bit exact): w x h dwords, each packing the 2x2
//                     bilinear footprint of one texel (pm_device.hpp SrcTex8)
//   source depth maps dense w x h fp32 (geometric consistency only)
//   planes float4, costs f32, selected views u32, geometric costs f32 [H*W]
//   prior planes float4 + mask u32 [H*W] (planar prior only)
//   ProblemDev: cameras + per-view constants, read through the scalar cache
// There is no per-pixel RNG state (the reference keeps 48 B/pixel of cuRAND).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <atomic>
#include <thread>
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_fusion.hpp"
#include "pm_sky.hpp"
#include "pm_kernels.hpp"
#include "pm_prior.hpp"
#include "pm_viewsel.hpp"
#include "pm_cloud.hpp"
#include "pm_voxel.hpp"
#include "pm_knn.hpp"
#include "pm_normals.hpp"
#include "pm_components.hpp"
#include "pm_align.hpp"
#include "pm_align_plane.hpp"
#include "pm_align_host.hpp"
#include "pm_render.hpp"
#include "pm_observe.hpp"
#include "pm_ingest.hpp"
#include "pm_undistort.hpp"
#include "pm_skyseg.hpp"
#include "pm_skyseg_model.hpp"
#include "pm_stage.hpp"
#include "pm_tracks_host.hpp"
#include "pm_fusion_host.hpp"

using namespace pm;

static_assert(sizeof(mpmvs_camera) == 112, "Camera layout");
static_assert(sizeof(mpmvs_params) == 56, "PatchMatchParams layout");

struct mpmvs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // mpmvs_run_get: the cost maps go to the host while the median filter still runs
    hipEvent_t costs_final = nullptr;
    // mpmvs_run_get_async: results are staged on the device so that the next Run() may start while they travel to the host
    float4* stage_planes = nullptr;
    float* stage_costs = nullptr;
    float* stage_geom = nullptr;
    hipEvent_t staged = nullptr, staging_free = nullptr;
    int async_outstanding = 0;
    int n_img = 0, W = 0, H = 0;
    std::vector<mpmvs_camera> cams;
    ProblemDev hP;               // host mirror
    ProblemDev* dP = nullptr;    // device copy
    float* d_ref = nullptr;
    // the quad-packed source textures of all views live in ONE allocation; d_src / d_src8 point into it
    void* d_tex_all = nullptr;
    std::vector<float*> d_src;      // fp32 format: w x h float4 texels per view
    std::vector<uint32_t*> d_src8;  // u8 format (every image 8-bit exact): w x h dwords per view
    bool all_u8 = false;
    std::vector<float*> d_depth; // dense source depth maps
    StateDev S{};
    bool depth_plane_valid = false;  // S.depth mirrors planes[].w (true from GetDepthandNormal until planes are rewritten)
    // S.own (the per-view costs InitializeScore stored) describes the planes of colour k as long as own_scale[k] >= 0: the window scale
    // and the bilateral sigmas it was evaluated with (own_ss / own_sc).  Set by enqueuing k_init; an update pass of colour k may read
    // the buffer iff it runs with these, and enqueuing it clears k; every other writer of S.planes and every change of the views clears
    // both (own_invalidate).  Host-side and conservative: the kernels are only ever told what holds for the whole launch.
    int own_scale[2] = {-1, -1};
    float own_ss = 0.0f, own_sc = 0.0f;
    bool own_enabled = true;   // mpmvs_dbg_own_costs(0): every pass recomputes
    int own_served = 0;        // update passes enqueued with the buffer in use
    float4* d_prior = nullptr;
    uint32_t* d_mask = nullptr;
    bool have_prior = false, have_depths = false;
    bool profiling = false;
    bool force_f32 = false;  // keep the fp32 texture format even for 8-bit exact images
    float k_ms[6] = {0, 0, 0, 0, 0, 0};
    int k_cnt[6] = {0, 0, 0, 0, 0, 0};
    struct Timed {
        int kind;
        hipEvent_t e0, e1;
        int passes;  // update launches: passes chained into the launch (booked as that many launches, alternating colours)
    };
    std::vector<Timed> pending;
    int* h_sync_err = nullptr;  // page-locked: the error word comes back with the stream synchronisation that ends a Run()
    int* d_sync = nullptr;      // ticket / completion / error words of the chained update launches (pm_kernels.hpp, ChainArgs)
    int sync_blocks = 0;
    bool chain = true;          // Run() chains the passes of a scale into one launch (MPMVS_CHAIN=0: one launch per pass)
    int spin_limit = kSpinLimit;   // polls after which a waiting block of a chained launch gives up (mpmvs_dbg_chain_stall shortens it)
    int dbg_stall_pos = -1;        // fault injection: this block position never signals its first pass (mpmvs_dbg_chain_stall)
    bool sync_overflow = false;    // a chained launch needed more completion words than d_sync holds (refused, -100)
    bool chain_failed_check = false;  // per-pass launches because the device failed the self-check of the chained launch
    // the banded end of mpmvs_run_get (enqueue_band_tail): row-band counters that the last update pass raises (pm_kernels.hpp, ChainArgs)
    unsigned* d_band = nullptr;
    unsigned band_run = 0;        // banded Run()s since the counters were last zeroed (the targets of the next one: band_run + 1 times its waves)
    bool band_armed = false;      // the last update launch enqueued by this Run() raises the band counters
    bool can_wait_value = false;  // hipStreamWaitValue32 is available on the device
    std::vector<hipEvent_t> event_pool;
    // Staging buffers of an upload that is still in flight on `stream` (mpmvs_set_views returns once its work is ENQUEUED): page-locked
    // host memory and pooled device memory, given back by release_deferred() right after the next synchronisation of the stream
    std::vector<void*> deferred_pinned, deferred_dev;
    std::string err;
};

static thread_local std::string g_create_err;
#ifdef PM_DBG_WAVETIME
static size_t kWaveTimeBytes(int W, int H) { return (size_t)16 * ((size_t)(W / 16 + 2) * (H / 8 + 8)) * 4 * 8; }
#endif

#define HIPCHK(ctx, expr)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            return -100;                                                                            \
        }                                                                                           \
    } while (0)

// hipGetLastError() reports the last error of ANY earlier runtime call of this thread (e.g. another caller's failed
// hipSetDevice).  Every entry point drops such a stale error first, so that the checks after its own kernel launches only
// see its own failures.
static hipError_t enter_device(int device) {
    (void)hipGetLastError();
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

static int fail(mpmvs_ctx* c, int code, const char* msg) {
    c->err = msg;
    return code;
}

// Start of every entry point: select the context's device, and refuse to touch a context whose pipelined Run()s
// (mpmvs_run_get_async) are still in flight -- only further mpmvs_run_get_async calls and mpmvs_wait are allowed then.
#define ENTER(ctx)                                                                                          \
    do {                                                                                                    \
        HIPCHK(ctx, enter_device((ctx)->device));                                                           \
        if ((ctx)->async_outstanding) return fail(ctx, -8, "pipelined Run()s are in flight: call mpmvs_wait first"); \
    } while (0)

// ---------------------------------------------------------------------------
// Device-buffer pool.  A context is created and destroyed per ProcessProblem call in the reference's flow (three times
// per Problem with the shipped schedule) and always asks for the same two dozen buffer sizes; hipMalloc/hipFree cost
// ~0.1-0.3 ms each and hipFree synchronises the device.  Released buffers are therefore kept per (device, size) and handed
// out again; at most MPMVS_POOL_MB (default 4096, 0 = off) megabytes are held.  Callers synchronise the owning stream
// before they release a buffer, so a pooled buffer is never still in use.
// ---------------------------------------------------------------------------
namespace {
struct BufPool {
    std::mutex mu;
    std::unordered_map<void*, std::pair<int, size_t>> owner;
    std::map<std::pair<int, size_t>, std::vector<void*>> cached;
    size_t cached_bytes = 0;
    size_t cap = 4096ull << 20;
    BufPool() {
        if (const char* e = std::getenv("MPMVS_POOL_MB")) cap = (size_t)std::strtoull(e, nullptr, 10) << 20;
    }
    void trim_locked() {
        for (auto& kv : cached)
            for (void* p : kv.second) {
                owner.erase(p);
                (void)hipFree(p);
            }
        cached.clear();
        cached_bytes = 0;
    }
};
BufPool g_pool;
}  // namespace

static hipError_t pool_malloc_bytes(void** p, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        auto it = g_pool.cached.find({dev, bytes});
        if (it != g_pool.cached.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            g_pool.cached_bytes -= bytes;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {  // out of memory with buffers parked in the pool: give them back and retry once
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(g_pool.mu);
        g_pool.trim_locked();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        g_pool.owner[*p] = {dev, bytes};
    }
    return e;
}
template <typename T>
static hipError_t pool_malloc(T** p, size_t bytes) {
    return pool_malloc_bytes((void**)p, bytes);
}
static hipError_t pool_free(void* p) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        auto it = g_pool.owner.find(p);
        if (it != g_pool.owner.end()) {
            const size_t bytes = it->second.second;
            if (g_pool.cached_bytes + bytes <= g_pool.cap) {
                g_pool.cached[it->second].push_back(p);
                g_pool.cached_bytes += bytes;
                return hipSuccess;
            }
            g_pool.owner.erase(it);
        }
    }
    return hipFree(p);
}

// Pinned host buffers for the host arrays of the wrapper (hostPlaneHypotheses ...): hipHostMalloc takes milliseconds, the
// wrapper allocates the same few sizes for every Problem and pass, so released buffers are kept per size (at most
// MPMVS_PINNED_POOL_MB, default 1024).
namespace {
struct PinnedPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> owner;
    std::map<size_t, std::vector<void*>> cached;
    size_t cached_bytes = 0;
    size_t cap = 1024ull << 20;
    PinnedPool() {
        if (const char* e = std::getenv("MPMVS_PINNED_POOL_MB")) cap = (size_t)std::strtoull(e, nullptr, 10) << 20;
    }
};
PinnedPool g_pinned;
}  // namespace

// page-locked scratch of one call: back to its pool on every return path
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() {
        if (p) mpmvs_free_pinned(p);
    }
};

// Pooled scratch buffer of one call on a stream that outlives it (a context's, the sky network's): on every return path the
// stream is synchronised first, then the buffer goes back to the pool -- nothing returns to the pool while the stream may use it.
struct Scratch {
    hipStream_t st;
    void* p = nullptr;
    explicit Scratch(hipStream_t stream) : st(stream) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        (void)pool_free(p);
    }
    hipError_t alloc(size_t bytes) { return pool_malloc_bytes(&p, bytes ? bytes : 4); }
    template <typename T>
    T* as() const { return (T*)p; }
};

// One stateless call on a device (fusion, sky mask, view selection, undistortion, the probes): a non-blocking stream of its own --
// the PatchMatch contexts other host threads drive on this device keep running -- and the pooled buffers of the call.  The
// destructor synchronises the stream, THEN gives the buffers back and destroys the events and the stream, on every return path.
class DeviceCall {
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<void*> bufs;
    bool entered_ = false, own_stream = false;

   public:
    explicit DeviceCall(int device) : entered_(enter_device(device) == hipSuccess) {
        own_stream = entered_ && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    }
    // a probe without a device argument: the current device and its null stream
    DeviceCall() : entered_(true) { (void)hipGetLastError(); }  // drop a stale error of an earlier call (see enter_device)
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;
    ~DeviceCall() {
        if (!entered_) return;
        (void)hipStreamSynchronize(st);
        for (void* p : bufs) (void)pool_free(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(st);
    }
    bool entered() const { return entered_; }         // the device could be selected
    bool ok() const { return own_stream; }            // ... and the stream exists
    hipStream_t stream() const { return st; }
    // nullptr: no memory.  Zero-sized arrays still get a (4-byte) buffer, so that no kernel argument is null.
    template <typename T>
    T* alloc(size_t bytes) {
        void* p = nullptr;
        if (pool_malloc_bytes(&p, bytes ? bytes : 4) != hipSuccess) return nullptr;
        bufs.push_back(p);
        return (T*)p;
    }
    // the same for `count` elements of T
    template <typename T>
    T* alloc_n(size_t count) {
        return alloc<T>(count * sizeof(T));
    }
    // begin() ... end() around the kernels; once the stream is synchronised, elapsed() is their device time
    bool begin() { return hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess && hipEventRecord(ev[0], st) == hipSuccess; }
    bool end() { return hipEventRecord(ev[1], st) == hipSuccess; }
    bool elapsed(float* ms) const { return hipEventElapsedTime(ms, ev[0], ev[1]) == hipSuccess; }
};

// S.own no longer describes the planes (or the images, or the texture format they were evaluated in): called by whatever writes
// S.planes other than k_init and the update passes themselves, and by whatever changes the views
static void own_invalidate(mpmvs_ctx* c) { c->own_scale[0] = c->own_scale[1] = -1; }

// the device staging buffers of mpmvs_run_get_async: all three or none
static void free_run_stage(mpmvs_ctx* c) {
    if (c->stage_planes) (void)pool_free(c->stage_planes);
    if (c->stage_costs) (void)pool_free(c->stage_costs);
    if (c->stage_geom) (void)pool_free(c->stage_geom);
    c->stage_planes = nullptr;
    c->stage_costs = c->stage_geom = nullptr;
}

static void reset_kernel_times(mpmvs_ctx* c) {
    for (int k = 0; k < 6; ++k) {
        c->k_ms[k] = 0.0f;
        c->k_cnt[k] = 0;
    }
}

static void release_deferred(mpmvs_ctx* c);
static void free_views(mpmvs_ctx* c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);  // nothing may still use what goes back to the pool
    release_deferred(c);
    if (c->d_ref) (void)pool_free(c->d_ref);
    c->d_ref = nullptr;
    if (c->d_tex_all) (void)pool_free(c->d_tex_all);
    c->d_tex_all = nullptr;
    c->d_src.clear();
    c->d_src8.clear();
    c->all_u8 = false;
    for (float* p : c->d_depth) (void)pool_free(p);
    c->d_depth.clear();
    if (c->S.planes) (void)pool_free(c->S.planes);
    if (c->S.costs) (void)pool_free(c->S.costs);
    if (c->S.sel) (void)pool_free(c->S.sel);
    if (c->S.geom) (void)pool_free(c->S.geom);
    if (c->S.depth) (void)pool_free(c->S.depth);
    if (c->S.own) (void)pool_free(c->S.own);
    own_invalidate(c);
    if (c->d_sync) (void)pool_free(c->d_sync);
    c->d_sync = nullptr;
    if (c->d_band) (void)pool_free(c->d_band);
    c->d_band = nullptr;
    c->band_run = 0;
#ifdef PM_DBG_WAVETIME
    if (c->S.wavetime) (void)hipFree(c->S.wavetime);
#endif
    free_run_stage(c);
    if (c->d_prior) (void)pool_free(c->d_prior);
    if (c->d_mask) (void)pool_free(c->d_mask);
    c->S = StateDev{};
    c->d_prior = nullptr;
    c->d_mask = nullptr;
    c->have_prior = c->have_depths = false;
}

static void cam_to_dev(const mpmvs_camera& s, CamDev& d) {
    std::memcpy(d.K, s.K, sizeof(d.K));
    std::memcpy(d.R, s.R, sizeof(d.R));
    std::memcpy(d.t, s.t, sizeof(d.t));
    std::memcpy(d.C, s.C, sizeof(d.C));
}

// Geometric consistency (ref .cu:582-640) as one projective map per direction: a pixel (x, y) of camera `a` at
// depth z lands in camera `b` at  ~  z * G (x, y, 1)^T + g  with
//   G = K_b (R_b R_a^T) Kinv'_a,   g = K_b (R_b C_a + t_b)
// where Kinv'_a = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1] is what BackProjectPoint2W applies (ref .cu:587-589: no skew), R_a^T and
// C_a what it transforms with (:595-600), and R_b, t_b and the FULL K_b what ProjectPoint uses (:608-614).  Double, this fixed
// order, one rounding to fp32; the oracle evaluates the same expressions.
static void geom_maps(const mpmvs_camera& a, const mpmvs_camera& b, float G[9], float g[3]) {
    const double fx = a.K[0], fy = a.K[4], cx = a.K[2], cy = a.K[5];
    double Rba[9], M[9], tb[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rba[i * 3 + j] = ((double)b.R[i * 3] * (double)a.R[j * 3] + (double)b.R[i * 3 + 1] * (double)a.R[j * 3 + 1]) +
                             (double)b.R[i * 3 + 2] * (double)a.R[j * 3 + 2];
    for (int i = 0; i < 3; ++i) {
        M[i * 3 + 0] = Rba[i * 3 + 0] / fx;
        M[i * 3 + 1] = Rba[i * 3 + 1] / fy;
        M[i * 3 + 2] = (Rba[i * 3 + 2] - (Rba[i * 3 + 0] * cx) / fx) - (Rba[i * 3 + 1] * cy) / fy;
        tb[i] = (((double)b.R[i * 3] * (double)a.C[0] + (double)b.R[i * 3 + 1] * (double)a.C[1]) + (double)b.R[i * 3 + 2] * (double)a.C[2]) + (double)b.t[i];
    }
    for (int i = 0; i < 3; ++i) {
        const double k0 = b.K[i * 3], k1 = b.K[i * 3 + 1], k2 = b.K[i * 3 + 2];
        for (int j = 0; j < 3; ++j) G[i * 3 + j] = (float)((k0 * M[0 + j] + k1 * M[3 + j]) + k2 * M[6 + j]);
        g[i] = (float)((k0 * tb[0] + k1 * tb[1]) + k2 * tb[2]);
    }
}

// per-view constants of H = A - b m^T, evaluated in double in the fixed order
// of DESIGN.md section 3.3 and rounded once to fp32
static void precompute_views(mpmvs_ctx* c) {
    const mpmvs_camera& r = c->cams[0];
    ProblemDev& P = c->hP;
    cam_to_dev(r, P.cam);
    const double fx = r.K[0], fy = r.K[4], cx = r.K[2], cy = r.K[5];
    P.ifx = (float)(1.0 / fx);
    P.ify = (float)(1.0 / fy);
    P.cxfx = (float)(cx / fx);
    P.cyfy = (float)(cy / fy);
    P.fxfy = r.K[0] / r.K[4];
    P.W = r.width;
    P.H = r.height;
    P.V = c->n_img - 1;
    for (int v = 1; v < c->n_img; ++v) {
        const mpmvs_camera& s = c->cams[v];
        ViewDev& o = P.views[v - 1];
        double Rrel[9], Crel[3], trel[3], M[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Rrel[i * 3 + j] = ((double)s.R[i * 3] * (double)r.R[j * 3] + (double)s.R[i * 3 + 1] * (double)r.R[j * 3 + 1]) +
                                  (double)s.R[i * 3 + 2] * (double)r.R[j * 3 + 2];
        for (int k = 0; k < 3; ++k) Crel[k] = (double)r.C[k] - (double)s.C[k];
        for (int i = 0; i < 3; ++i)
            trel[i] = ((double)s.R[i * 3] * Crel[0] + (double)s.R[i * 3 + 1] * Crel[1]) + (double)s.R[i * 3 + 2] * Crel[2];
        for (int i = 0; i < 3; ++i) {
            M[i * 3 + 0] = Rrel[i * 3 + 0] / fx;
            M[i * 3 + 1] = Rrel[i * 3 + 1] / fy;
            M[i * 3 + 2] = (Rrel[i * 3 + 2] - (Rrel[i * 3 + 0] * cx) / fx) - (Rrel[i * 3 + 1] * cy) / fy;
        }
        const double k0 = s.K[0], k2 = s.K[2], k4 = s.K[4], k5 = s.K[5], k8 = s.K[8];
        for (int j = 0; j < 3; ++j) {
            o.A[0 + j] = (float)(k0 * M[0 + j] + k2 * M[6 + j]);
            o.A[3 + j] = (float)(k4 * M[3 + j] + k5 * M[6 + j]);
            o.A[6 + j] = (float)(k8 * M[6 + j]);
        }
        o.b[0] = (float)(k0 * trel[0] + k2 * trel[2]);
        o.b[1] = (float)(k4 * trel[1] + k5 * trel[2]);
        o.b[2] = (float)(k8 * trel[2]);
        o.w = s.width;
        o.h = s.height;
        o.wf = (float)s.width;
        o.hf = (float)s.height;
        o.wm1 = (float)(s.width - 1);
        o.hm1 = (float)(s.height - 1);
        geom_maps(r, s, o.Gf, o.gf);   // reference pixel at depth z -> source pixel
        geom_maps(s, r, o.Gb, o.gb);   // source pixel at depth d -> reference pixel
    }
}

// Call right after a synchronisation of c->stream: whatever an earlier call parked for its asynchronous transfers is free again.
static void release_deferred(mpmvs_ctx* c) {
    for (void* p : c->deferred_pinned) mpmvs_free_pinned(p);
    c->deferred_pinned.clear();
    for (void* p : c->deferred_dev) (void)pool_free(p);
    c->deferred_dev.clear();
}

// The device copy of the Problem description follows the host mirror.  The copy leaves from a page-locked snapshot of its own (a
// transfer out of pageable memory would make the call wait for everything ahead of it on the stream), so the caller may go on
// changing c->hP and nothing here waits for the GPU.
static int upload_problem_async(mpmvs_ctx* c) {
    void* snap = mpmvs_alloc_pinned(sizeof(ProblemDev));
    if (!snap) {   // no page-locked memory: the plain, synchronising form
        HIPCHK(c, hipMemcpyAsync(c->dP, &c->hP, sizeof(ProblemDev), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        release_deferred(c);
        return 0;
    }
    std::memcpy(snap, &c->hP, sizeof(ProblemDev));
    c->deferred_pinned.push_back(snap);
    HIPCHK(c, hipMemcpyAsync(c->dP, snap, sizeof(ProblemDev), hipMemcpyHostToDevice, c->stream));
    return 0;
}
static int upload_problem(mpmvs_ctx* c) {
    const int rc = upload_problem_async(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release_deferred(c);
    return 0;
}

// ---------------------------------------------------------------------------
// Self-check of the chained update launch (pm_kernels.hpp, k_update).  Its hand-over from pass to pass -- write-through stores, a
// counter, an agent-scope acquire -- is validated empirically on gfx942 / gfx950; a memory system that broke it would not crash, it
// would hand out stale planes.  So the first context created on a device runs one small Problem (512 x 384, 9 source views: the
// MAXV = 16 instantiations, which keeps these launches apart from the 8-view kernels in a profile of anything else; window scales 1 and 0:
// the 256- and the 64-thread form) chained and pass by pass with the same seed and compares every plane and cost bit for bit.  A
// mismatch switches every context of that device to per-pass launches.  ~10 ms, once per process and device; MPMVS_CHAIN_SELFCHECK=0 skips it.
// ---------------------------------------------------------------------------
namespace {
std::mutex g_chain_check_mu;
int g_chain_state[64] = {0};   // per device: 0 = not checked yet, 1 = passed (or skipped), -1 = failed
thread_local bool g_in_chain_check = false;
}  // namespace

static int run_chain_check(int device) {
    const int W = 512, H = 384, V = 9;
    std::vector<std::vector<float>> img(V + 1, std::vector<float>((size_t)W * H));
    std::vector<mpmvs_camera> cams(V + 1);
    std::vector<const float*> ptr(V + 1);
    for (int i = 0; i <= V; ++i) {
        mpmvs_camera& cm = cams[i];
        std::memset(&cm, 0, sizeof(cm));
        cm.K[0] = cm.K[4] = 400.0f, cm.K[2] = 0.5f * W, cm.K[5] = 0.5f * H, cm.K[8] = 1.0f;
        cm.R[0] = cm.R[4] = cm.R[8] = 1.0f;
        const int k = i - 1;   // sources on a 3 x 3 grid around the reference
        const float cx = i == 0 ? 0.0f : 0.12f * (float)(k % 3 - 1) + 0.01f * (float)k, cy = i == 0 ? 0.0f : 0.12f * (float)(k / 3 - 1);
        cm.C[0] = cx, cm.C[1] = cy, cm.C[2] = 0.0f;
        cm.t[0] = -cx, cm.t[1] = -cy, cm.t[2] = 0.0f;
        cm.height = H, cm.width = W;
        cm.depth_min = 2.0f, cm.depth_max = 6.0f;
        // a fronto-parallel textured plane at depth 4: view i sees the pattern shifted by its disparity
        const float sx = cx * 400.0f / 4.0f, sy = cy * 400.0f / 4.0f;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float u = (float)x + sx, v = (float)y + sy;
                const uint32_t ux = (uint32_t)(int)std::floor(u * 0.5f), vy = (uint32_t)(int)std::floor(v * 0.5f);
                uint32_t h = ux * 0x9E3779B1u ^ (vy * 0x85EBCA77u + 0x27D4EB2Fu);
                h ^= h >> 15, h *= 0x2C1B3C6Du, h ^= h >> 12;
                const float val = 128.0f + 50.0f * std::sin(0.21f * u + 0.13f * v) + 40.0f * std::sin(0.05f * u - 0.33f * v) + (float)(h & 31u) - 16.0f;
                img[i][(size_t)y * W + x] = std::floor(std::min(255.0f, std::max(0.0f, val)));
            }
        ptr[i] = img[i].data();
    }
    mpmvs_ctx* c = mpmvs_create(device);
    if (!c) return 0;
    mpmvs_params p;
    std::memset(&p, 0, sizeof(p));
    p.max_iterations = 3, p.num_images = V + 1, p.top_k = 4, p.sigma_spatial = 5.0f, p.sigma_color = 3.0f;
    p.depth_min = 2.0f, p.depth_max = 6.0f, p.max_scale = 1;
    const size_t wh = (size_t)W * H;
    // page-locked outputs: the chained Run() then ends in the banded tail (enqueue_band_tail) and is checked with it, against the
    // per-pass launches and the whole-image tail
    float* pl[2] = {static_cast<float*>(mpmvs_alloc_pinned(wh * 16)), static_cast<float*>(mpmvs_alloc_pinned(wh * 16))};
    float* co[2] = {static_cast<float*>(mpmvs_alloc_pinned(wh * 4)), static_cast<float*>(mpmvs_alloc_pinned(wh * 4))};
    int verdict = 0;
    if (pl[0] && pl[1] && co[0] && co[1] && mpmvs_set_views(c, V + 1, cams.data(), ptr.data(), nullptr) == 0) {
        int rc[2];
        for (int k = 0; k < 2; ++k) {
            c->chain = (k == 0);
            rc[k] = mpmvs_run_get(c, &p, 0x5EEDC4A1ull, pl[k], co[k], nullptr);
        }
        // a chained Run() that fails (-101: a block gave up waiting; -100) where the per-pass one runs is a failed check; only
        // when the per-pass Run() fails too could the check not run
        if (rc[1] == 0)
            verdict = (rc[0] == 0 && std::memcmp(pl[0], pl[1], wh * 16) == 0 && std::memcmp(co[0], co[1], wh * 4) == 0) ? 1 : -1;
    }
    mpmvs_destroy(c);
    for (int k = 0; k < 2; ++k) {
        if (pl[k]) mpmvs_free_pinned(pl[k]);
        if (co[k]) mpmvs_free_pinned(co[k]);
    }
    return verdict;
}

static bool chain_check_passed(int device) {
    if (g_in_chain_check || device < 0 || device >= 64) return true;   // the check's own context
    if (const char* e = std::getenv("MPMVS_CHAIN_SELFCHECK"))
        if (std::atoi(e) == 0) return true;
    std::lock_guard<std::mutex> lk(g_chain_check_mu);
    if (g_chain_state[device] == 0) {
        g_in_chain_check = true;
        const int v = run_chain_check(device);
        g_in_chain_check = false;
        if (v < 0) std::fprintf(stderr, "mpmvs: the chained update launch failed its self-check on device %d: launching one kernel per pass\n", device);
        g_chain_state[device] = v;   // 0 (the check itself could not run): try again with the next context
    }
    return g_chain_state[device] >= 0;
}

extern "C" {

int mpmvs_texture_filter_bits(void) {
#ifdef PM_TEX_Q8
    return 8;
#else
    return 0;
#endif
}

int mpmvs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

mpmvs_ctx* mpmvs_create(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_err = std::string("no HIP device available: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (device < 0 || device >= n) {
        g_create_err = "device index out of range";
        return nullptr;
    }
    if ((e = enter_device(device)) != hipSuccess) {
        g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    mpmvs_ctx* c = new mpmvs_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = pool_malloc(&c->dP, sizeof(ProblemDev))) != hipSuccess) {
        g_create_err = std::string("context setup: ") + hipGetErrorString(e);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        (void)hipGetLastError();
        delete c;
        return nullptr;
    }
    std::memset(&c->hP, 0, sizeof(ProblemDev));
    c->h_sync_err = static_cast<int*>(mpmvs_alloc_pinned(sizeof(int)));   // pooled page-locked memory (include/mpmvs.h)
    if (!c->h_sync_err) {   // without it a timed-out chained launch would go unreported
        g_create_err = "context setup: no page-locked memory for the error word of the update launches";
        (void)hipStreamDestroy(c->stream);
        (void)pool_free(c->dP);
        delete c;
        return nullptr;
    }
    *c->h_sync_err = 0;
    int wait_value = 0;
    if (hipDeviceGetAttribute(&wait_value, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess) (void)hipGetLastError();
    c->can_wait_value = wait_value != 0;
    if (const char* e = std::getenv("MPMVS_CHAIN")) c->chain = std::atoi(e) != 0;   // 0: one update launch per pass (measurements, bisecting)
    if (c->chain && !chain_check_passed(device)) {
        c->chain = false;
        c->chain_failed_check = true;
    }
    return c;
}

void mpmvs_destroy(mpmvs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);  // a pipelined Run() nobody waited for
    free_views(c);
    for (hipEvent_t ev : c->event_pool) (void)hipEventDestroy(ev);
    if (c->dP) (void)pool_free(c->dP);   // (hipFree would synchronise the whole device)
    if (c->costs_final) (void)hipEventDestroy(c->costs_final);
    if (c->staged) (void)hipEventDestroy(c->staged);
    if (c->staging_free) (void)hipEventDestroy(c->staging_free);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->h_sync_err) mpmvs_free_pinned(c->h_sync_err);
    delete c;
}

const char* mpmvs_last_error(const mpmvs_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// ---------------------------------------------------------------------------
// Image upload (CudaMemInit's image half, ref .cpp:999-1025).  The caller's images are pageable fp32 arrays; copied as they
// are, the runtime stages them through its own bounce buffers at a fraction of the PCIe rate and every copy is synchronous.
// Here the rows are converted (8-bit exact images: to bytes, which also quarters the traffic) or copied into ONE page-locked
// staging buffer by a few host threads, go to the device in asynchronous DMA transfers, and are unpacked there; the call
// does not synchronise (round 6): both staging buffers stay with the context until its stream is next synchronised (release_deferred).
// The host half -- slots, groups, the row work -- is pm_stage.hpp.
// ---------------------------------------------------------------------------
// an upload gives up: nothing of it stays in flight, the staging buffers go back
static int upload_failed(mpmvs_ctx* c, const char* what) {
    (void)hipStreamSynchronize(c->stream);
    release_deferred(c);
    c->err = what;
    return -100;
}

// Second half of an image upload: the per-pixel state of the Problem and its ProblemDev, enqueued behind the unpacking kernels
static int finish_views(mpmvs_ctx* c) {
    if (hipGetLastError() != hipSuccess) return upload_failed(c, "unpacking the images on the device failed");
    const size_t wh = (size_t)c->W * c->H;
    int rc = -100;
    if (pool_malloc(&c->S.planes, wh * 16) == hipSuccess && pool_malloc(&c->S.costs, wh * 4) == hipSuccess &&
        pool_malloc(&c->S.sel, wh * 4) == hipSuccess && pool_malloc(&c->S.geom, wh * 4) == hipSuccess && pool_malloc(&c->S.depth, wh * 4) == hipSuccess &&
        pool_malloc(&c->S.own, wh * 4 * (size_t)std::max(1, c->n_img - 1)) == hipSuccess &&   // one plane per source view of THIS Problem; written by k_init before any read
        hipMemsetAsync(c->S.planes, 0, wh * 16, c->stream) == hipSuccess && hipMemsetAsync(c->S.costs, 0, wh * 4, c->stream) == hipSuccess &&
        hipMemsetAsync(c->S.sel, 0, wh * 4, c->stream) == hipSuccess && hipMemsetAsync(c->S.geom, 0, wh * 4, c->stream) == hipSuccess)
        rc = 0;
    c->depth_plane_valid = false;
    if (!rc) {
        // one completion word per update block (the smallest block the kernel can be built with is 16 x 8 pixels), zeroed once: every
        // chained launch leaves them zeroed again
        c->sync_blocks = ((c->W + 15) / 16 + 1) * ((c->H + 7) / 8 + 4);
        const size_t bytes = (size_t)(kSyncHeader + c->sync_blocks) * sizeof(int);
        if (pool_malloc(&c->d_sync, bytes) != hipSuccess || hipMemsetAsync(c->d_sync, 0, bytes, c->stream) != hipSuccess) rc = -100;
        // one band counter per 8 image rows at most (bands are 32 rows and more), zeroed here and after a failed Run() only
        const size_t band_bytes = (size_t)((c->H + 7) / 8 + 4) * sizeof(unsigned);
        c->band_run = 0;
        if (!rc && (pool_malloc(&c->d_band, band_bytes) != hipSuccess || hipMemsetAsync(c->d_band, 0, band_bytes, c->stream) != hipSuccess)) rc = -100;
    }
#ifdef PM_DBG_WAVETIME
    // room for 16 launches of one wave per 64 pixels of a colour, 4 x u64 each (generous: blocks overhang the image border)
    if (!rc && (hipMalloc(&c->S.wavetime, kWaveTimeBytes(c->W, c->H)) != hipSuccess || hipMemsetAsync(c->S.wavetime, 0, kWaveTimeBytes(c->W, c->H), c->stream) != hipSuccess)) rc = -100;
#endif
    if (rc) return upload_failed(c, "allocation of the per-pixel state failed");
    // no synchronisation: everything later on this context follows on the same stream, and a transfer that fails is reported by the
    // next call that waits for the stream (mpmvs_run*, mpmvs_get, ...) as -100
    return upload_problem_async(c);
}

static IngestSrc ingest_src(const unsigned char* d_bytes, int src_w, int src_h, int dst_w, int dst_h) {
    // the two ratios exactly as ResizeLinear forms them (host/PatchMatchHost.cpp)
    return IngestSrc{d_bytes, src_w, src_h, (unsigned)src_w, (float)src_w / dst_w, (float)src_h / dst_h};
}

// What the two entries hand to the one upload (upload_views): the images as the caller holds them, and how their rows reach the stage.
struct ViewsInput {
    std::vector<pmstage::HostImage> im;   // per view the size it is staged at (the byte entry: its own, it may be shrunk on the device)
    size_t slot_px;                       // staging room per pixel, bytes
    // Whether the reference image / the sources are staged as bytes (else as fp32 rows), decided before the first group is staged:
    // the texture format of the sources must be known before the first of them is packed.  May stage group 0 on the way when
    // that is all there is, and says so (true).  Absent: everything is bytes.
    std::function<bool(const pmstage::StagePlan&, char* stage, bool& ref_bytes, bool& src_bytes)> formats;
    std::function<void(const pmstage::StagePlan&, int g, char* stage, bool ref_bytes, bool src_bytes)> stage_group;
};

// THE image upload, for both entries.  `in` says how the rows are staged; which kernel unpacks a view follows from what was staged:
//   reference   bytes, same size   k_pad_u8              source, fp16 texels   bytes, same size   k_pack_quads_u8
//               bytes, resampled   k_ingest_pad          source, fp32 texels   fp32               k_pack_quads_f32
//               fp32               k_pad                                       bytes              k_ingest_quads<resampled>
// The sources take the 8-byte fp16 texels iff they are staged as bytes (8-bit exact: the reference's imread path, ref .cpp:877-882),
// none of them is resampled (a resampled image is not made of integers) and fp32 is not forced; else the 16-byte fp32 ones.  One
// inexact source sends all sources to fp32; the reference image decides its own format.
static int upload_views(mpmvs_ctx* c, int n, const mpmvs_camera* cams, const ViewsInput& in) {
    c->n_img = n;
    c->cams.assign(cams, cams + n);
    c->W = cams[0].width;
    c->H = cams[0].height;
    std::memset(&c->hP, 0, sizeof(ProblemDev));
    precompute_views(c);
    const pmstage::HostImage* im = in.im.data();
    auto resampled = [&](int i) { return im[i].w != cams[i].width || im[i].h != cams[i].height; };
    // host staging (page-locked, pooled) and its device twin: a slot per image, 256-byte aligned, in groups under the staging limit
    const pmstage::StagePlan plan = pmstage::plan_stage(im, n, in.slot_px, pmstage::stage_limit_bytes());
    const int n_groups = plan.groups();
    const size_t stage_bytes = plan.stage_bytes;
    // Both staging buffers stay with the context until the stream has been synchronised the next time (release_deferred): the call
    // returns as soon as the transfers and the unpacking kernels are ENQUEUED, so that the upload of one Problem overlaps whatever else
    // the GPU and the host are doing -- the other contexts of a multi-Problem job, this context's own next call (ref src/main.cpp:20-41).
    char* const stage = (char*)mpmvs_alloc_pinned(stage_bytes);
    if (!stage) return fail(c, -100, "no page-locked staging memory for the images");
    c->deferred_pinned.push_back(stage);
    void* d_stage_p = nullptr;
    HIPCHK(c, pool_malloc_bytes(&d_stage_p, stage_bytes ? stage_bytes : 4));
    c->deferred_dev.push_back(d_stage_p);
    char* const d_stage = (char*)d_stage_p;
    bool ref_bytes = true, src_bytes = true;
    const bool staged = in.formats && in.formats(plan, stage, ref_bytes, src_bytes);
    bool src_u8 = src_bytes && !c->force_f32;
    for (int v = 1; v < n; ++v) src_u8 = src_u8 && !resampled(v);
    c->all_u8 = src_u8;
    // reference image (replicate-padded fp32) and one allocation for the textures of all views, each 256-byte aligned.  Every
    // view is addressed through its own buffer resource (base = the view's first texel, 32-bit offsets inside it), so only a
    // single view is limited to 4 GB (checked by the caller), not the allocation: 32 views of 3200 x 3200 fp32 texels are 5.2 GB.
    const int pw = c->W + 2 * kRefApron, ph = c->H + 2 * kRefApron;
    if (pool_malloc(&c->d_ref, (size_t)pw * ph * 4) != hipSuccess) return upload_failed(c, "allocation of the reference image failed");
    c->hP.ref_pitch = pw;
    c->hP.ref_img = c->d_ref + (size_t)kRefApron * pw + kRefApron;
    const size_t texel = src_u8 ? 8 : 16;
    std::vector<size_t> tex_off(n, 0);
    size_t tex_total = 0;
    for (int v = 1; v < n; ++v) {
        tex_off[v] = tex_total;
        tex_total += ((size_t)cams[v].width * cams[v].height * texel + 255) & ~(size_t)255;
    }
    if (pool_malloc(&c->d_tex_all, tex_total) != hipSuccess) return upload_failed(c, "allocation of the source textures failed");
    if (src_u8) c->d_src8.assign(n - 1, nullptr); else c->d_src.assign(n - 1, nullptr);
    for (int g = 0; g < n_groups; ++g) {
        const int first = plan.group_first[g], last = plan.group_first[g + 1];
        // (with one group nothing synchronises: g == 0)
        if (g > 0 && hipStreamSynchronize(c->stream) != hipSuccess) return upload_failed(c, "upload of the images failed");  // the staging buffers are free again
        if (!staged) in.stage_group(plan, g, stage, ref_bytes, src_bytes);
        for (int i = first; i < last; ++i) {
            const size_t off = plan.at(g, i);
            const size_t bytes = (size_t)im[i].w * im[i].h * ((i == 0 ? ref_bytes : src_bytes) ? 1 : 4);
            if (hipMemcpyAsync(d_stage + off, stage + off, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                return upload_failed(c, "upload of the images failed");
        }
        for (int v = first; v < last; ++v) {
            const char* src = d_stage + plan.at(g, v);
            const int w = cams[v].width, h = cams[v].height;
            const IngestSrc s = ingest_src((const unsigned char*)src, im[v].w, im[v].h, w, h);   // (read where the view is staged as bytes)
            if (v == 0) {
                const dim3 grid((pw + 255) / 256, ph);
                if (!ref_bytes)
                    hipLaunchKernelGGL(k_pad, grid, dim3(256), 0, c->stream, (const float*)src, w, h, c->d_ref, kRefApron);
                else if (resampled(0))
                    hipLaunchKernelGGL(k_ingest_pad, grid, dim3(256), 0, c->stream, s, w, h, c->d_ref, kRefApron);
                else
                    hipLaunchKernelGGL(k_pad_u8, grid, dim3(256), 0, c->stream, (const unsigned char*)src, w, h, c->d_ref, kRefApron);
                continue;
            }
            ViewDev& o = c->hP.views[v - 1];
            if (src_u8) {
                c->d_src8[v - 1] = (uint32_t*)((char*)c->d_tex_all + tex_off[v]);
                hipLaunchKernelGGL(k_pack_quads_u8, dim3((w + 255) / 256, h), dim3(256), 0, c->stream, (const unsigned char*)src, w, h, (uint2*)c->d_src8[v - 1]);
                o.pitch8 = w;
                o.img8 = c->d_src8[v - 1];
                continue;
            }
            c->d_src[v - 1] = (float*)((char*)c->d_tex_all + tex_off[v]);
            float4* const tex = (float4*)c->d_src[v - 1];
            const dim3 grid((w + kIngestTW - 1) / kIngestTW, (h + kIngestTH - 1) / kIngestTH);
            if (!src_bytes)
                hipLaunchKernelGGL(k_pack_quads_f32, dim3((w + 255) / 256, h), dim3(256), 0, c->stream, (const float*)src, w, h, tex);
            else if (resampled(v))
                hipLaunchKernelGGL(k_ingest_quads<true>, grid, dim3(kIngestThreads), 0, c->stream, s, w, h, tex);
            else
                hipLaunchKernelGGL(k_ingest_quads<false>, grid, dim3(kIngestThreads), 0, c->stream, s, w, h, tex);
            o.pitch = w;
            o.img = c->d_src[v - 1];
        }
    }
    return finish_views(c);
}

// What both entries check before they touch the context; the byte entry (src_w / src_h / pitch in bytes as it got them, any of
// them null) adds the checks of its source sizes
static int validate_views(mpmvs_ctx* c, int n, const mpmvs_camera* cams, const void* const* images, bool bytes, const int* src_w, const int* src_h,
                          const size_t* pitch_bytes) {
    if (n < 2 || n - 1 > MPMVS_MAX_SRC_VIEWS) return fail(c, -1, "need 2..33 views");
    if (bytes && (!cams || !images || (src_w == nullptr) != (src_h == nullptr))) return fail(c, -2, "null argument (source widths and heights come together)");
    for (int i = 0; i < n; ++i) {
        if (cams[i].width <= 0 || cams[i].height <= 0 || !images[i]) return fail(c, -2, "bad image size or null image");
        const int sw = src_w ? src_w[i] : cams[i].width, sh = src_h ? src_h[i] : cams[i].height;
        if (bytes) {
            if (sw <= 0 || sh <= 0) return fail(c, -2, "bad source image size");
            if (pitch_bytes && pitch_bytes[i] < (size_t)sw) return fail(c, -2, "row pitch smaller than the source width");
        }
        // texel indices are formed with a 24-bit multiply (texel_index, pm_device.hpp) and offsets inside a view are 32 bits
        if (cams[i].width >= (1 << 24) || cams[i].height >= (1 << 24) || (size_t)cams[i].width * cams[i].height * 16 >= (1ull << 32))
            return fail(c, -3, "image too large (a view's texture must stay below 4 GB)");
        if (bytes && (size_t)sw * sh >= (1ull << 32)) return fail(c, -3, "source image too large (it must stay below 4 GB)");
    }
    return 0;
}

// the views of the context are replaced by an upload -- or by nothing
static int replace_views(mpmvs_ctx* c, int n, const mpmvs_camera* cams, const ViewsInput& in) {
    free_views(c);
    const int rc = upload_views(c, n, cams, in);
    if (rc) {  // no half-built Problem is left behind: the context is as after mpmvs_create
        const std::string why = c->err;
        free_views(c);
        c->n_img = c->W = c->H = 0;
        c->cams.clear();
        std::memset(&c->hP, 0, sizeof(ProblemDev));
        c->err = why;
    }
    return rc;
}

int mpmvs_set_views(mpmvs_ctx* c, int n, const mpmvs_camera* cams, const float* const* images, const size_t* pitch_bytes) {
    if (!c) return -1;
    ENTER(c);
    const int bad = validate_views(c, n, cams, (const void* const*)images, false, nullptr, nullptr, nullptr);
    if (bad) return bad;
    ViewsInput in;
    in.slot_px = 4;   // room for w * h floats; an image that is 8-bit exact is staged as w * h BYTES at the start of its slot
    for (int i = 0; i < n; ++i)
        in.im.push_back({(const char*)images[i], cams[i].width, cams[i].height, pitch_bytes ? pitch_bytes[i] : (size_t)cams[i].width * 4});
    const pmstage::HostImage* im = in.im.data();
    const bool try_src_u8 = !c->force_f32;
    // ordinary inputs are one group: one pass over the images that decides the formats while it stages; several groups take a
    // first pass that only decides the formats
    in.formats = [=](const pmstage::StagePlan& plan, char* stage, bool& ref_u8, bool& src_u8) {
        if (plan.groups() == 1) {
            pmstage::stage_deciding(im, n, plan, try_src_u8, stage, ref_u8, src_u8);
            return true;
        }
        pmstage::exact_sweep<false>(im, n, try_src_u8, nullptr, nullptr, ref_u8, src_u8);
        return false;
    };
    in.stage_group = [=](const pmstage::StagePlan& plan, int g, char* stage, bool ref_u8, bool src_u8) {
        pmstage::stage_known(im, plan, g, stage, ref_u8, src_u8);
    };
    return replace_views(c, n, cams, in);
}

// 8-bit entry (pm_ingest.hpp): the views arrive as bytes at their own size.  Nothing is tested or converted on the host -- the formats
// follow from the sizes alone -- so the host work is one row-wise copy per image into the page-locked stage.
int mpmvs_set_views_u8(mpmvs_ctx* c, int n, const mpmvs_camera* cams, const unsigned char* const* images, const int* src_widths,
                       const int* src_heights, const size_t* pitch_bytes) {
    if (!c) return -1;
    ENTER(c);
    const int bad = validate_views(c, n, cams, (const void* const*)images, true, src_widths, src_heights, pitch_bytes);
    if (bad) return bad;
    ViewsInput in;
    in.slot_px = 1;
    for (int i = 0; i < n; ++i) {
        const int sw = src_widths ? src_widths[i] : cams[i].width, sh = src_heights ? src_heights[i] : cams[i].height;
        in.im.push_back({(const char*)images[i], sw, sh, pitch_bytes ? pitch_bytes[i] : (size_t)sw});
    }
    const pmstage::HostImage* im = in.im.data();
    in.stage_group = [=](const pmstage::StagePlan& plan, int g, char* stage, bool, bool) { pmstage::stage_byte_rows(im, plan, g, stage); };
    return replace_views(c, n, cams, in);
}

int mpmvs_resize_u8(int device, const unsigned char* src, int src_w, int src_h, size_t pitch_bytes, int dst_w, int dst_h, float* out) {
    if (!src || !out || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0) return -2;
    if (pitch_bytes == 0) pitch_bytes = (size_t)src_w;
    if (pitch_bytes < (size_t)src_w) return -2;
    if ((size_t)src_w * src_h >= (1ull << 32) || dst_w >= (1 << 24) || dst_h >= (1 << 24)) return -3;
    DeviceCall call(device);
    if (!call.ok()) return -100;
    const size_t out_bytes = (size_t)dst_w * dst_h * 4;
    unsigned char* d_src = call.alloc<unsigned char>((size_t)src_w * src_h);
    float* d_out = call.alloc<float>(out_bytes);
    if (!d_src || !d_out) return -100;
    if (hipMemcpy2DAsync(d_src, (size_t)src_w, src, pitch_bytes, (size_t)src_w, (size_t)src_h, hipMemcpyHostToDevice, call.stream()) != hipSuccess) return -100;
    hipLaunchKernelGGL(k_ingest_pad, dim3((dst_w + 255) / 256, dst_h), dim3(256), 0, call.stream(), ingest_src(d_src, src_w, src_h, dst_w, dst_h), dst_w, dst_h,
                       d_out, 0);
    if (hipGetLastError() != hipSuccess) return -100;
    if (hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, call.stream()) != hipSuccess || hipStreamSynchronize(call.stream()) != hipSuccess) return -100;
    return 0;
}

static int attach_depths(mpmvs_ctx* c, int n_src, const int* widths, const int* heights) {
    for (int i = 0; i < n_src; ++i) {
        ViewDev& o = c->hP.views[i];
        o.depth = c->d_depth[i];
        o.dw = widths[i];
        o.dh = heights[i];
        o.dwm1 = (float)(widths[i] - 1);
        o.dhm1 = (float)(heights[i] - 1);
    }
    c->have_depths = true;
    return upload_problem(c);
}

// (re)allocates the map of source i when its size changes; a kept map must have the size the caller states
static int depth_slot(mpmvs_ctx* c, int i, int w, int h, bool replace) {
    if (w <= 0 || h <= 0) return fail(c, -2, "bad depth map");
    const ViewDev& o = c->hP.views[i];
    if (c->d_depth[i] && o.dw == w && o.dh == h) return 0;
    if (!replace) return fail(c, -2, "no resident depth map of that size to keep");
    if (c->d_depth[i]) (void)pool_free(c->d_depth[i]);
    c->d_depth[i] = nullptr;
    HIPCHK(c, pool_malloc(&c->d_depth[i], (size_t)w * h * 4));
    return 0;
}

// A copy into a depth slot failed after depth_slot() may already have exchanged buffers: the device-side ProblemDev could still
// name a buffer that went back to the pool.  The context then holds NO usable depth maps (a geometric Run() is refused by
// check_ready until a later call succeeds) and nothing of this call is left in flight.
static int depth_upload_failed(mpmvs_ctx* c) {
    c->err = std::string("uploading a source depth map failed: ") + hipGetErrorString(hipGetLastError());
    c->have_depths = false;
    (void)hipStreamSynchronize(c->stream);
    return -100;
}

// the three public forms below: per source a device buffer (on src_devices[i], default the context's device), a host array, or
// neither (keep what an earlier call left there)
static int set_src_depths_impl(mpmvs_ctx* c, int n_src, const float* const* depths, const size_t* pitch_bytes, const float* const* d_depths,
                               const int* src_devices, const int* widths, const int* heights, bool null_is_error) {
    if (c->n_img < 2 || n_src != c->n_img - 1) return fail(c, -1, "n_src must equal the number of source views");
    (void)hipStreamSynchronize(c->stream);
    if ((int)c->d_depth.size() != n_src) {
        for (float* p : c->d_depth) (void)pool_free(p);
        c->d_depth.assign(n_src, nullptr);
        c->have_depths = false;
    }
    for (int i = 0; i < n_src; ++i) {
        const float* dev = d_depths ? d_depths[i] : nullptr;
        const float* host = depths ? depths[i] : nullptr;
        if (!dev && !host && null_is_error) return fail(c, -2, "bad depth map");
        int rc = depth_slot(c, i, widths[i], heights[i], dev != nullptr || host != nullptr);
        if (rc) {
            c->have_depths = false;
            return rc;
        }
        if (!dev && !host) continue;  // keep the map an earlier call uploaded
        ViewDev& o = c->hP.views[i];
        o.dw = widths[i], o.dh = heights[i];  // depth_slot compares against these
        const size_t bytes = (size_t)widths[i] * heights[i] * 4;
        hipError_t e;
        if (dev) {
            const int from = src_devices ? src_devices[i] : c->device;
            if (from == c->device)
                e = hipMemcpyAsync(c->d_depth[i], dev, bytes, hipMemcpyDeviceToDevice, c->stream);
            else
                e = hipMemcpyPeerAsync(c->d_depth[i], c->device, dev, from, bytes, c->stream);   // over xGMI between the GPUs of a node
        } else {
            const size_t pitch = pitch_bytes ? pitch_bytes[i] : (size_t)widths[i] * 4;
            e = hipMemcpy2DAsync(c->d_depth[i], (size_t)widths[i] * 4, host, pitch, (size_t)widths[i] * 4, heights[i], hipMemcpyHostToDevice, c->stream);
        }
        if (e != hipSuccess) return depth_upload_failed(c);
    }
    return attach_depths(c, n_src, widths, heights);
}

int mpmvs_set_src_depths(mpmvs_ctx* c, int n_src, const float* const* depths, const int* widths, const int* heights, const size_t* pitch_bytes) {
    if (!c) return -1;
    ENTER(c);
    return set_src_depths_impl(c, n_src, depths, pitch_bytes, nullptr, nullptr, widths, heights, false);
}

int mpmvs_set_src_depths_device(mpmvs_ctx* c, int n_src, const float* const* d_depths, const int* widths, const int* heights) {
    if (!c) return -1;
    ENTER(c);
    return set_src_depths_impl(c, n_src, nullptr, nullptr, d_depths, nullptr, widths, heights, true);
}

int mpmvs_set_src_depths_mixed(mpmvs_ctx* c, int n_src, const float* const* depths, const float* const* d_depths, const int* src_devices, const int* widths,
                               const int* heights) {
    if (!c) return -1;
    ENTER(c);
    return set_src_depths_impl(c, n_src, depths, nullptr, d_depths, src_devices, widths, heights, false);
}

int mpmvs_set_state(mpmvs_ctx* c, const void* planes4, const void* costs) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.planes) return fail(c, -1, "set_views first");
    const size_t wh = (size_t)c->W * c->H;
    own_invalidate(c);
    if (planes4) {
        c->depth_plane_valid = false;
        HIPCHK(c, hipMemcpyAsync(c->S.planes, planes4, wh * 16, hipMemcpyHostToDevice, c->stream));
    }
    if (costs) HIPCHK(c, hipMemcpyAsync(c->S.costs, costs, wh * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_set_selected_views(mpmvs_ctx* c, const void* sel) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.sel) return fail(c, -1, "set_views first");
    HIPCHK(c, hipMemcpyAsync(c->S.sel, sel, (size_t)c->W * c->H * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_set_geom_costs(mpmvs_ctx* c, const void* geom) {
    if (!c || !geom) return -1;
    ENTER(c);
    if (!c->S.geom) return fail(c, -1, "set_views first");
    HIPCHK(c, hipMemcpyAsync(c->S.geom, geom, (size_t)c->W * c->H * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_set_prior(mpmvs_ctx* c, const void* prior4, const void* mask) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.planes) return fail(c, -1, "set_views first");
    const size_t wh = (size_t)c->W * c->H;
    if (!c->d_prior) HIPCHK(c, pool_malloc(&c->d_prior, wh * 16));
    if (!c->d_mask) HIPCHK(c, pool_malloc(&c->d_mask, wh * 4));
    HIPCHK(c, hipMemcpyAsync(c->d_prior, prior4, wh * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_mask, mask, wh * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->S.prior = c->d_prior;
    c->S.mask = c->d_mask;
    c->have_prior = true;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
#ifdef PM_DBG_WAVETIME
// measurement builds: the per-wave records of the last <= 16 update launches ([launch % 16][wave][4] u64; pm_kernels.hpp, WaveTimer)
extern "C" long mpmvs_dbg_wavetime(mpmvs_ctx* c, void* out, size_t cap_bytes) {
    if (!c || !c->S.wavetime) return -1;
    if (enter_device(c->device) != hipSuccess) return -1;
    const size_t n = kWaveTimeBytes(c->W, c->H);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (out && hipMemcpy(out, c->S.wavetime, n < cap_bytes ? n : cap_bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long)n;
}
#endif

static int check_ready(mpmvs_ctx* c, const mpmvs_params* p) {
    if (c->n_img < 2) return fail(c, -1, "set_views not called (need >= 2 views)");
    if (p->num_images != c->n_img) return fail(c, -2, "params.num_images != number of views");
    if (p->max_scale < 0 || p->max_scale > 2) return fail(c, -3, "max_scale must be 0..2 (window radius <= 20)");
    if (p->geom_consistency && !c->have_depths) return fail(c, -4, "geom_consistency needs source depth maps");
    if (p->planar_prior && !c->have_prior) return fail(c, -5, "planar_prior needs set_prior");
    // The reference never runs both at once: ProcessProblem clears geom_consistency before the prior Run()
    // (ref src/PatchMatch.cpp:535), so that kernel variant is not built.
    if (p->geom_consistency && p->planar_prior) return fail(c, -7, "geom_consistency and planar_prior are mutually exclusive (ref PatchMatch.cpp:535)");
    return 0;
}

static hipEvent_t get_event(mpmvs_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// the row the reference's checkerboard grid reaches down to (ref .cu:1196), and the rows the checkerboard launches cover: that
// grid, at most the image
static int checker_ylimit(const mpmvs_ctx* c) { return 2 * 16 * (((c->H / 2) + 15) / 16); }
static int checker_rows(const mpmvs_ctx* c) { return std::min(c->H, checker_ylimit(c)); }

static dim3 checker_grid(const mpmvs_ctx* c) {
    const int rows = checker_rows(c);
    return dim3(((c->W + kChkBlockW - 1) / kChkBlockW) * ((rows + kChkBlockH<> - 1) / kChkBlockH<>));
}
// The kernel variant that serves a launch.  The NCC kernels are instantiated per bound MAXV on the number of source views, texel
// format (U8: fp16 texels) and window scale (a template parameter: pm_device.hpp, Win).  dispatch_variant calls
// launch(MAXV, U8, SCALE), as std::integral_constant values, for V views (the first of the BUCKETS that holds them; the last one
// takes the rest), the format `u8` and `scale` in 0..2 -- or scale 0 only where SCALE0_ONLY, and then no other scale is instantiated.
// The per-view arrays of the update kernel (8 x V candidate costs and four V-vectors, in scratch) are sized by MAXV: buckets of 8
// keep that scratch and the register pressure around it proportional to the Problem (the shipped configuration allows 20 views,
// reference config/config.yaml:19; the hard limit is 32, ref .cu:500).
template <bool SCALE0_ONLY, int BUCKET, int... BUCKETS, class F>
static void dispatch_variant(int V, bool u8, int scale, F&& launch) {
    if constexpr (sizeof...(BUCKETS) > 0) {
        if (V > BUCKET) return dispatch_variant<SCALE0_ONLY, BUCKETS...>(V, u8, scale, launch);
    }
    const auto with_format = [&](auto fmt) {
        using MaxV = std::integral_constant<int, BUCKET>;
        if (scale == 0) launch(MaxV{}, fmt, std::integral_constant<int, 0>{});
        if constexpr (!SCALE0_ONLY) {
            if (scale == 1) launch(MaxV{}, fmt, std::integral_constant<int, 1>{});
            if (scale == 2) launch(MaxV{}, fmt, std::integral_constant<int, 2>{});
        }
    };
    if (u8)
        with_format(std::true_type{});
    else
        with_format(std::false_type{});
}

template <bool GEOM, bool PRIOR, int MAXV, bool U8, int SCALE>
static void launch_update_chain(mpmvs_ctx* c, const LaunchArgs& a, const ChainArgs& ch0) {
    constexpr int NT = kUpdThreads<U8, SCALE>, BW = kChkBlockW, BH = kChkBlockH<NT>;
    const int rows = checker_rows(c);
    ChainArgs ch = ch0;
    ch.nbx = (c->W + BW - 1) / BW;
    ch.nby = (rows + BH - 1) / BH;
    ch.nb = ch.nbx * ch.nby;
    ch.sync = c->d_sync;
    ch.spin_limit = c->spin_limit;
    ch.stall_pos = c->dbg_stall_pos;
    if (ch.nb > c->sync_blocks) {   // (never write past the completion words, whatever the block shape)
        c->sync_overflow = true;
        return;
    }
    if (ch.band) c->band_armed = true;
    const dim3 grid((unsigned)(ch.n_pass * ch.nb));   // one block per work item (pass, position), handed out by ticket (k_update)
    const size_t lds = update_lds_bytes<NT>();
    const dim3 blk(NT);
    hipLaunchKernelGGL((k_update<GEOM, PRIOR, MAXV, U8, SCALE>), grid, blk, lds, c->stream, c->dP, c->S, a, ch);
}
// The photometric update exists at the scales 0..2 of the multi-scale schedule; the geometric and the prior update run at scale 0
// only, as Run() does (ref .cu:1188-1254: the scale loop belongs to the photometric branch).
template <bool GEOM, bool PRIOR>
static void launch_update(mpmvs_ctx* c, const LaunchArgs& a, const ChainArgs& ch) {
    dispatch_variant<GEOM || PRIOR, 8, 16, 24, kMaxViews>(c->hP.V, c->all_u8, a.scale, [&](auto maxv, auto u8, auto scale) {
        launch_update_chain<GEOM, PRIOR, maxv, u8, scale>(c, a, ch);
    });
}

// the spatial half of the bilateral weight exponent (ref .cu:318-323) of the 36 window taps at `scale`, [column][row]
static void fill_spatial_terms(LaunchArgs& a, int scale) {
    const int step = 2 << scale, radius = 5 * step / 2;
    for (int col = 0; col < 6; ++col)
        for (int row = 0; row < 6; ++row) {
            const int dx = col * step - radius, dy = row * step - radius;
            const float sd = std::sqrt((float)dx * (float)dx + (float)dy * (float)dy);
            a.spatial[col * 6 + row] = (-sd) / a.two_ss;
        }
}

// the canonical exp of pm_device.hpp (d_exp) on the host, for arguments <= 0: the same fma sequence, the same bits
static float host_exp_canonical(float x) {
    if (x < -80.0f) return 0.0f;
    const float n = std::rint(x * 1.44269504088896341f);
    float r = std::fma(n, -0.693359375f, x);
    r = std::fma(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = std::fma(p, r, 1.3981999507e-3f);
    p = std::fma(p, r, 8.3334519073e-3f);
    p = std::fma(p, r, 4.1665795894e-2f);
    p = std::fma(p, r, 1.6666665459e-1f);
    p = std::fma(p, r, 5.0000001201e-1f);
    const float y = std::fma(p, r * r, r) + 1.0f;
    uint32_t bits;
    memcpy(&bits, &y, 4);
    bits += (uint32_t)(int)n << 23;
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

static LaunchArgs make_args(const mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, int kind, int iter, int scale, uint32_t launch) {
    LaunchArgs a;
    a.seed = seed;
    a.launch = launch;
    a.iter = iter;
    a.scale = scale;
    a.parity = (kind == MPMVS_KIND_RED || kind == MPMVS_KIND_FILTER_RED) ? 1 : 0;
    a.ylimit = checker_ylimit(c);
    a.top_k = p->top_k;
    a.depth_min = p->depth_min;
    a.depth_max = p->depth_max;
    a.two_ss = (2.0f * p->sigma_spatial) * p->sigma_spatial;
    a.two_sc = (2.0f * p->sigma_color) * p->sigma_color;
    fill_spatial_terms(a, scale);
    // ref .cu:832: double product, one rounding to float
    a.cost_threshold = (float)(0.8 * (double)host_exp_canonical((float)(iter * iter) / (-90.0f)));
    a.init_random = (!p->geom_consistency && !p->planar_prior) ? 1 : 0;
    a.use_prior = p->planar_prior ? 1 : 0;
    return a;
}

// Height of a row band of the banded end of Run() (enqueue_band_tail): about H / kTailBands rows, a multiple of 32 -- the block
// height of the filter launches (kChkBlockH<256>), of two rows of k_depth_normal's blocks and of four 8-row groups of the band counters.
constexpr int kTailBands = 12;
static int band_rows(const mpmvs_ctx* c) {
    const int k = (c->H + 16 * kTailBands) / (32 * kTailBands);
    return 32 * (k > 1 ? k : 1);
}

// One launch.  For the update kinds `passes` > 1 chains that many passes into it -- alternating colours starting with `kind`, launch
// ids launch, launch + 1, ..., iterations iter, iter (+1 after every red pass): exactly the launches that many calls would make.
// signal_bands: the launch ends a banded Run() -- its last pass raises the band counters (enqueue_band_tail).
static int enqueue_step(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, int kind, int iter, int scale, uint32_t launch, int passes = 1,
                        bool signal_bands = false) {
    if (scale < 0 || scale > 2) return fail(c, -3, "scale must be 0..2");
    if (passes < 1 || (passes + 1) / 2 + 1 > kChainMaxIters) return fail(c, -6, "too many passes in one update launch");
    if ((kind == MPMVS_KIND_BLACK || kind == MPMVS_KIND_RED) && scale != 0 && (p->geom_consistency || p->planar_prior))
        return fail(c, -3, "geometric / planar-prior updates run at scale 0 only (as Run() does)");
    const LaunchArgs a = make_args(c, p, seed, kind, iter, scale, launch);
    ChainArgs ch{};
    ch.n_pass = passes;
    for (int j = 0; j < kChainMaxIters; ++j) ch.thr[j] = (float)(0.8 * (double)host_exp_canonical((float)((iter + j) * (iter + j)) / (-90.0f)));
    if (signal_bands && passes > 1 && c->d_band) {
        ch.band = c->d_band;
        ch.band_groups = band_rows(c) / kWaveRows;
        ch.n_groups = (checker_rows(c) + kWaveRows - 1) / kWaveRows;
        ch.band_run = c->band_run + 1;
    }

    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->profiling) {
        e0 = get_event(c);
        e1 = get_event(c);
        HIPCHK(c, hipEventRecord(e0, c->stream));
    }
    const dim3 blk(256);
    const dim3 grid_dense((c->W + 15) / 16, (c->H + 15) / 16);
    const dim3 grid_chk = checker_grid(c);  // k_filter (checker_pixel)
    int own_passes = 0;   // passes of this launch that read S.own
    switch (kind) {
        case MPMVS_KIND_INIT: {
            c->depth_plane_valid = false;
            const size_t lds = ncc_lds_bytes(16, 16, a.scale);
            dispatch_variant<false, 8, 16, 24, kMaxViews>(c->hP.V, c->all_u8, a.scale, [&](auto maxv, auto u8, auto scale) {
                hipLaunchKernelGGL((k_init<maxv, u8, scale>), grid_dense, blk, lds, c->stream, c->dP, c->S, a);
            });
            // S.own now holds the per-view costs of every pixel's plane, as evaluated with this window
            c->own_scale[0] = c->own_scale[1] = a.scale;
            c->own_ss = p->sigma_spatial;
            c->own_sc = p->sigma_color;
            break;
        }
        case MPMVS_KIND_BLACK:
        case MPMVS_KIND_RED:
            c->depth_plane_valid = false;
            // the first pass of a colour after k_init reads S.own; every pass rewrites the planes of its colour
            for (int k = 0; k < passes; ++k) {
                const int colour = (a.parity + k) & 1;
                if (k < 2 && c->own_enabled && c->own_scale[colour] == a.scale && c->own_ss == p->sigma_spatial && c->own_sc == p->sigma_color) {
                    ch.own_mask |= 1 << colour;
                    own_passes++;
                }
                c->own_scale[colour] = -1;
            }
            if (p->geom_consistency)
                launch_update<true, false>(c, a, ch);
            else if (p->planar_prior)
                launch_update<false, true>(c, a, ch);
            else
                launch_update<false, false>(c, a, ch);
            break;
        case MPMVS_KIND_DEPTH_NORMAL:
            hipLaunchKernelGGL(k_depth_normal, grid_dense, blk, 0, c->stream, c->dP, c->S, 0);
            c->depth_plane_valid = true;
            own_invalidate(c);   // the planes change form (world normal, depth)
            break;
        case MPMVS_KIND_FILTER_BLACK:
        case MPMVS_KIND_FILTER_RED:
            own_invalidate(c);   // the filter rewrites planes[].w
            if (!c->depth_plane_valid) {  // a filter step on a state that did not come from GetDepthandNormal (mpmvs_set_state + mpmvs_step)
                const int n = c->W * c->H;
                hipLaunchKernelGGL(k_export_depth, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S.planes, c->S.depth, n);
                c->depth_plane_valid = true;
            }
            hipLaunchKernelGGL(k_filter, grid_chk, blk, 0, c->stream, c->dP, c->S, a, 0);
            break;
        default:
            return fail(c, -6, "bad kernel kind");
    }
    HIPCHK(c, hipGetLastError());
    if (c->sync_overflow) {
        c->sync_overflow = false;
        if (c->profiling) {
            c->event_pool.push_back(e0);
            c->event_pool.push_back(e1);
        }
        return fail(c, -100, "the update launch has more block positions than completion words (d_sync)");
    }
    c->own_served += own_passes;
    if (c->profiling) {
        HIPCHK(c, hipEventRecord(e1, c->stream));
        c->pending.push_back({kind, e0, e1, passes});
    }
    return 0;
}

static int finish(mpmvs_ctx* c) {
    // the error word of the chained update launches: a block that gave up waiting for its neighbours (pm_kernels.hpp, kSpinLimit)
    const bool check = c->d_sync && c->h_sync_err;
    if (check) HIPCHK(c, hipMemcpyAsync(c->h_sync_err, c->d_sync + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release_deferred(c);
    for (auto& pe : c->pending) {
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, pe.e0, pe.e1);
        if (pe.passes > 1) {
            // a chained update launch: booked as its passes, alternating colours from pe.kind on, each with an equal share of the time
            const int other = pe.kind == MPMVS_KIND_BLACK ? MPMVS_KIND_RED : MPMVS_KIND_BLACK;
            const int n_first = (pe.passes + 1) / 2, n_other = pe.passes / 2;
            c->k_ms[pe.kind] += ms * (float)n_first / (float)pe.passes;
            c->k_ms[other] += ms * (float)n_other / (float)pe.passes;
            c->k_cnt[pe.kind] += n_first;
            c->k_cnt[other] += n_other;
        } else {
            c->k_ms[pe.kind] += ms;
            c->k_cnt[pe.kind] += 1;
        }
        c->event_pool.push_back(pe.e0);
        c->event_pool.push_back(pe.e1);
    }
    c->pending.clear();
    if (check && *c->h_sync_err) {
        (void)hipMemsetAsync(c->d_sync, 0, (size_t)(kSyncHeader + c->sync_blocks) * sizeof(int), c->stream);
        (void)hipStreamSynchronize(c->stream);
        return fail(c, -101, "an update launch timed out waiting for the blocks of its previous pass (results invalid)");
    }
    return 0;
}

extern "C" {

// Everything a failed Run() may have left behind: launches and copies into caller buffers still in flight on either stream
// (the caller may free its buffers once the call has returned), and profiling events that would otherwise be booked on the
// next call.  Returns `rc` unchanged.
static int abandon_run(mpmvs_ctx* c, int rc) {
    const std::string why = c->err;
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    release_deferred(c);
    for (auto& pe : c->pending) {
        c->event_pool.push_back(pe.e0);
        c->event_pool.push_back(pe.e1);
    }
    c->pending.clear();
    own_invalidate(c);   // whatever the failed launches left in the planes, S.own does not describe it
    if (c->d_sync) {  // a launch that did not finish leaves them dirty
        (void)hipMemsetAsync(c->d_sync, 0, (size_t)(kSyncHeader + c->sync_blocks) * sizeof(int), c->stream);
        (void)hipStreamSynchronize(c->stream);
    }
    // the band counters: a launch that gave up lifted them to their targets and its blocks then added to them -- start over from
    // zero, now that both streams are idle and no wait is armed
    c->band_armed = false;
    if (c->d_band) {
        (void)hipMemsetAsync(c->d_band, 0, (size_t)((c->H + 7) / 8 + 4) * sizeof(unsigned), c->stream);
        (void)hipStreamSynchronize(c->stream);
        c->band_run = 0;
    }
    (void)hipGetLastError();
    c->err = why;
    return rc;
}

// The launch schedule of Run() (ref .cu:1200-1244) in two halves, ONE copy of it for the blocking and the pipelined Run(): the
// random streams are keyed by the launch numbers, so the two entry points give the same bits only while they number alike.
// enqueue_updates: InitializeScore and every Black / RedPixelUpdate (costs and geometric costs are final afterwards);
// enqueue_finalize: GetDepthandNormal and the two median-filter launches.
// signal_bands: the last launch raises the band counters (enqueue_band_tail); c->band_armed tells whether it was enqueued.
static int enqueue_updates(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, uint32_t& launch, bool signal_bands = false) {
    int rc;
    if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_INIT, 0, p->max_scale, launch++))) return rc;
    // the black / red passes of one window scale: one launch per pass (the reference's schedule, ref .cu:1211-1236), or -- the
    // default -- chained into launches of up to 2 * (kChainMaxIters - 1) passes whose blocks wait for their neighbours of the pass
    // before (pm_kernels.hpp, k_update): same launch ids, same results, no tail between the passes
    auto scale_passes = [&](int s) -> int {
        int i = 0;
        while (i < p->max_iterations) {
            const int n = c->chain ? std::min(p->max_iterations - i, kChainMaxIters - 1) : 1;
            if (c->chain) {
                const bool last = s == 0 && i + n >= p->max_iterations;
                if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_BLACK, i, s, launch, 2 * n, signal_bands && last))) return rc;
                launch += 2 * n;
            } else {
                if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_BLACK, i, s, launch++))) return rc;
                if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_RED, i, s, launch++))) return rc;
            }
            i += n;
        }
        return 0;
    };
    if (p->geom_consistency || p->planar_prior) {
        if ((rc = scale_passes(0))) return rc;
    } else {
        for (int s = p->max_scale; s >= 0; --s)
            if ((rc = scale_passes(s))) return rc;
    }
    return 0;
}
static int enqueue_finalize(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, uint32_t& launch) {
    int rc;
    if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_DEPTH_NORMAL, 0, 0, launch++))) return rc;
    if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_FILTER_BLACK, 0, 0, launch++))) return rc;
    if ((rc = enqueue_step(c, p, seed, MPMVS_KIND_FILTER_RED, 0, 0, launch++))) return rc;
    return 0;
}

// A host buffer the banded copies may write into: page-locked (or registered) memory.  A copy into pageable memory is synchronous,
// which would serialise the bands with the host.
static bool host_pinned(const void* ptr) {
    if (!ptr) return true;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// The banded end of Run() (mpmvs_run_get on the chained path).  Rows of the image become final in raster order during the last
// update pass (its tickets are raster-ordered), so GetDepthandNormal, the two median-filter launches and the device-to-host copies
// run band by band on the copy stream while that pass still works further down, instead of after it.  Step s, for band s of rows:
//   * wait (hipStreamWaitValue32, >=) for the band counters that the last pass raises (pm_kernels.hpp, ChainArgs) until every
//     wave whose candidates reach into the band (23 rows, kDirs) has completed: k_depth_normal rewrites the planes that the pass
//     reads as candidates;
//   * copy the band's costs (and geometric costs): final with the update;
//   * k_depth_normal on the band: depths are done down to its end D;
//   * k_filter black down to FB = D - 32 (the filter reads the other colour's depths 5 rows on, in place: they must all exist);
//   * k_filter red down to FR = FB - 32 (it reads black depths filtered 5 rows on, while no black filter may still read the red
//     depths it rewrites);
//   * copy the planes down to FR: final.
// The step whose wait covers the whole image -- every band counter -- takes everything down to the image's end.  Every launch and
// copy keeps its arithmetic and its inputs, so the maps are the bits of the whole-image tail; the stream's launches follow one
// another, which orders the reads and writes above.
static int enqueue_band_tail(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, uint32_t launch, void* planes4, void* costs, void* geom) {
    hipStream_t fs = c->copy_stream;
    const int W = c->W, H = c->H, bh = band_rows(c), n_bands = (H + bh - 1) / bh;
    const int rows = checker_rows(c), n_groups = (rows + kWaveRows - 1) / kWaveRows, gpb = bh / kWaveRows;
    const unsigned per_group = (unsigned)((W + kChkBlockW - 1) / kChkBlockW);   // last-pass waves per 8-row group
    const int nbx_f = (W + kChkBlockW - 1) / kChkBlockW, bh_f = kChkBlockH<256>;
    static_assert(kChkBlockH<256> == 32, "the filter's lag behind the depths (32 rows) is one filter block row");
    const LaunchArgs fa[2] = {make_args(c, p, seed, MPMVS_KIND_FILTER_BLACK, 0, 0, launch + 1), make_args(c, p, seed, MPMVS_KIND_FILTER_RED, 0, 0, launch + 2)};
    const dim3 blk(256);
    // a launch on the copy stream, timed like enqueue_step's when profiling (booked as one launch of its kind per band)
    auto timed = [&](int kind, auto&& go) -> int {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (c->profiling) {
            e0 = get_event(c);
            e1 = get_event(c);
            HIPCHK(c, hipEventRecord(e0, fs));
        }
        go();
        HIPCHK(c, hipGetLastError());
        if (c->profiling) {
            HIPCHK(c, hipEventRecord(e1, fs));
            c->pending.push_back({kind, e0, e1, 1});
        }
        return 0;
    };
    // rows [r0, r1) of one colour (r0 a multiple of 32)
    auto filter = [&](int r0, int r1, int colour) -> int {
        r1 = std::min(r1, rows);   // rows below the reference's checkerboard grid are not filtered
        if (r1 <= r0) return 0;
        const int f0 = r0 / bh_f, f1 = (r1 + bh_f - 1) / bh_f;
        return timed(colour ? MPMVS_KIND_FILTER_RED : MPMVS_KIND_FILTER_BLACK, [&] {
            hipLaunchKernelGGL(k_filter, dim3((unsigned)(nbx_f * (f1 - f0))), blk, 0, fs, c->dP, c->S, fa[colour], f0 * nbx_f);
        });
    };
    int rc, waited = 0;          // band counters the stream waits for already
    int done_fb = 0, done_fr = 0; // rows filtered black / red so far
    for (int s = 0; s < n_bands; ++s) {
        const int r0 = s * bh;
        int r1 = std::min(H, r0 + bh);
        // the 8-row groups whose last-pass waves read rows of this band: 8 g - 23 < r1
        const int need = std::min(n_groups, (r1 + 22) / kWaveRows + 1);
        for (; waited * gpb < need; ++waited) {
            const int groups = std::min(n_groups, (waited + 1) * gpb) - waited * gpb;
            HIPCHK(c, hipStreamWaitValue32(fs, c->d_band + waited, c->band_run * per_group * (unsigned)groups, hipStreamWaitValueGte, 0xFFFFFFFFu));
        }
        const bool last = waited * gpb >= n_groups;   // the update has ended: this step takes the rest of the image
        if (last) r1 = H;
        const size_t off = (size_t)r0 * W, n = (size_t)(r1 - r0) * W;
        if (costs) HIPCHK(c, hipMemcpyAsync(static_cast<float*>(costs) + off, c->S.costs + off, n * 4, hipMemcpyDeviceToHost, fs));
        if (geom) HIPCHK(c, hipMemcpyAsync(static_cast<float*>(geom) + off, c->S.geom + off, n * 4, hipMemcpyDeviceToHost, fs));
        if ((rc = timed(MPMVS_KIND_DEPTH_NORMAL, [&] {
                 hipLaunchKernelGGL(k_depth_normal, dim3((unsigned)((W + 15) / 16), (unsigned)((r1 - r0 + 15) / 16)), blk, 0, fs, c->dP, c->S, r0 / 16);
             })))
            return rc;
        const int fb = last ? H : std::max(0, r1 - bh_f), fr = last ? H : std::max(0, fb - bh_f);
        if (fb > done_fb) {
            if ((rc = filter(done_fb, fb, 0))) return rc;
            done_fb = fb;
        }
        if (fr > done_fr) {
            if ((rc = filter(done_fr, fr, 1))) return rc;
            const size_t po = (size_t)done_fr * W, pn = (size_t)(fr - done_fr) * W;
            if (planes4) HIPCHK(c, hipMemcpyAsync(static_cast<float4*>(planes4) + po, c->S.planes + po, pn * 16, hipMemcpyDeviceToHost, fs));
            done_fr = fr;
        }
        if (last) break;
    }
    c->depth_plane_valid = true;
    own_invalidate(c);   // k_depth_normal and the filter have rewritten the planes
    return 0;
}

static int enqueue_run(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, void* planes4, void* costs, void* geom) {
    int rc;
    uint32_t launch = 0;
    // the banded end: chained launches, stream waits, an output, page-locked host buffers; otherwise the whole-image tail below
    const bool banded = c->chain && c->can_wait_value && c->d_band && (planes4 || costs || geom) && host_pinned(planes4) && host_pinned(costs) &&
                        host_pinned(geom);
    if (banded) {
        if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->costs_final) HIPCHK(c, hipEventCreateWithFlags(&c->costs_final, hipEventDisableTiming));
        // targets grow with every banded Run(); long before they could overflow, start over from zero (nothing waits between Run()s)
        if ((uint64_t)(c->band_run + 1) * (uint64_t)((c->W + kChkBlockW - 1) / kChkBlockW) * (uint64_t)(band_rows(c) / kWaveRows) > 0x7fffffffull) {
            HIPCHK(c, hipMemsetAsync(c->d_band, 0, (size_t)((c->H + 7) / 8 + 4) * sizeof(unsigned), c->stream));
            c->band_run = 0;
        }
        // the copy stream's waits come after everything enqueued on the context so far (the zeroing of the counters included)
        HIPCHK(c, hipEventRecord(c->costs_final, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->costs_final, 0));
    }
    if ((rc = enqueue_updates(c, p, seed, launch, banded))) return rc;
    if (c->band_armed) {
        c->band_armed = false;
        c->band_run++;
        if ((rc = enqueue_band_tail(c, p, seed, launch, planes4, costs, geom))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        return finish(c);
    }
    const size_t wh = (size_t)c->W * c->H;
    const bool early = costs || geom;
    if (early) {
        if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->costs_final) HIPCHK(c, hipEventCreateWithFlags(&c->costs_final, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->costs_final, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->costs_final, 0));
        if (costs) HIPCHK(c, hipMemcpyAsync(costs, c->S.costs, wh * 4, hipMemcpyDeviceToHost, c->copy_stream));
        if (geom) HIPCHK(c, hipMemcpyAsync(geom, c->S.geom, wh * 4, hipMemcpyDeviceToHost, c->copy_stream));
    }
    if ((rc = enqueue_finalize(c, p, seed, launch))) return rc;
    if (planes4) HIPCHK(c, hipMemcpyAsync(planes4, c->S.planes, wh * 16, hipMemcpyDeviceToHost, c->stream));
    if (early) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return finish(c);
}

// Run() (ref .cu:1188-1254).  With output pointers the device-to-host copies that end the reference's Run() (:1246-1251) are
// part of the call: costs (and geometric costs) are final after the last update launch, so they travel on a second stream
// while GetDepthandNormal and the median filter still run; the planes follow on the main stream.
static int run_impl(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, void* planes4, void* costs, void* geom) {
    if (!c || !p) return -1;
    ENTER(c);
    int rc = check_ready(c, p);
    if (rc) return rc;
    reset_kernel_times(c);
    rc = enqueue_run(c, p, seed, planes4, costs, geom);
    return rc ? abandon_run(c, rc) : 0;
}

int mpmvs_run(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed) { return run_impl(c, p, seed, nullptr, nullptr, nullptr); }

// The geometric-cost buffer follows the reference's rule (ref .cu:1248): Run() copies cudaGeomCosts whenever
// params.geomPlanarPrior is set, whatever the mode of THIS Run() -- the flag survives SetGeomConsistencyParams(false, true)
// (ref .cpp:655-665), so the planar-prior re-run of a geometric pass (ref .cpp:535,604) copies the map its geometric Run()
// left behind (the prior kernels do not write it).  Any Run() may therefore be given a buffer; it receives what the device
// holds (zeros before the first geometric Run() of the context).
int mpmvs_run_get(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, void* planes4, void* costs, void* geom) {
    return run_impl(c, p, seed, planes4, costs, geom);
}

// Pipelined Run(): the same launches, but the result maps are first copied into staging buffers on the device (46 MB, ~25 us) and
// travel to the host from there on the copy stream, so the call returns at once and the NEXT Run() of this context -- which
// overwrites the state with its InitializeScore -- may start while the previous result is still crossing PCIe (0.7 ms of a
// 17 ms cfg-1 step otherwise spent waiting).  The caller gives consecutive calls different host buffers and collects with
// mpmvs_wait(); in between the context accepts nothing but further mpmvs_run_get_async calls.  Same results as mpmvs_run_get.
int mpmvs_run_get_async(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, void* planes4, void* costs, void* geom) {
    if (!c || !p) return -1;
    HIPCHK(c, enter_device(c->device));
    int rc = check_ready(c, p);
    if (rc) return rc;
    const size_t wh = (size_t)c->W * c->H;
    if (!c->stage_planes || !c->stage_costs || !c->stage_geom) {
        // all three or none: a partial set left behind by a failed allocation would make the next call copy through a null pointer
        if ((!c->stage_planes && pool_malloc(&c->stage_planes, wh * 16) != hipSuccess) || (!c->stage_costs && pool_malloc(&c->stage_costs, wh * 4) != hipSuccess) ||
            (!c->stage_geom && pool_malloc(&c->stage_geom, wh * 4) != hipSuccess)) {
            free_run_stage(c);
            return fail(c, -100, "allocation of the staging buffers failed");
        }
    }
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->staged) HIPCHK(c, hipEventCreateWithFlags(&c->staged, hipEventDisableTiming));
    if (!c->staging_free) HIPCHK(c, hipEventCreateWithFlags(&c->staging_free, hipEventDisableTiming));
    if (!c->async_outstanding) reset_kernel_times(c);   // the kernel times of pipelined Run()s accumulate until mpmvs_wait
    c->async_outstanding++;
    uint32_t launch = 0;
    auto body = [&]() -> int {
        int r;
        if ((r = enqueue_updates(c, p, seed, launch)) || (r = enqueue_finalize(c, p, seed, launch))) return r;
        // the staging buffers are free once the previous call's copies have left them (a 0.7 ms copy against a whole Run())
        if (c->async_outstanding > 1) HIPCHK(c, hipStreamWaitEvent(c->stream, c->staging_free, 0));
        if (planes4) HIPCHK(c, hipMemcpyAsync(c->stage_planes, c->S.planes, wh * 16, hipMemcpyDeviceToDevice, c->stream));
        if (costs) HIPCHK(c, hipMemcpyAsync(c->stage_costs, c->S.costs, wh * 4, hipMemcpyDeviceToDevice, c->stream));
        if (geom) HIPCHK(c, hipMemcpyAsync(c->stage_geom, c->S.geom, wh * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->staged, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->staged, 0));
        if (planes4) HIPCHK(c, hipMemcpyAsync(planes4, c->stage_planes, wh * 16, hipMemcpyDeviceToHost, c->copy_stream));
        if (costs) HIPCHK(c, hipMemcpyAsync(costs, c->stage_costs, wh * 4, hipMemcpyDeviceToHost, c->copy_stream));
        if (geom) HIPCHK(c, hipMemcpyAsync(geom, c->stage_geom, wh * 4, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->staging_free, c->copy_stream));
        return 0;
    };
    rc = body();
    if (rc) {
        c->async_outstanding = 0;
        return abandon_run(c, rc);
    }
    return 0;
}

// Completes every pipelined Run() of the context: all result maps are in their host buffers when it returns.
int mpmvs_wait(mpmvs_ctx* c) {
    if (!c) return -1;
    HIPCHK(c, enter_device(c->device));
    c->async_outstanding = 0;
    if (c->copy_stream && hipStreamSynchronize(c->copy_stream) != hipSuccess) {
        c->err = "the device-to-host copies of a pipelined Run() failed";
        return abandon_run(c, -100);
    }
    const int rc = finish(c);
    return rc ? abandon_run(c, rc) : 0;
}

int mpmvs_step(mpmvs_ctx* c, const mpmvs_params* p, uint64_t seed, int kind, int iter, int scale, uint32_t launch_id) {
    if (!c || !p) return -1;
    ENTER(c);
    int rc = check_ready(c, p);
    if (rc) return rc;
    if ((rc = enqueue_step(c, p, seed, kind, iter, scale, launch_id)) || (rc = finish(c))) return abandon_run(c, rc);
    return 0;
}

int mpmvs_get(mpmvs_ctx* c, void* planes4, void* costs, void* geom) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.planes) return fail(c, -1, "set_views first");
    const size_t wh = (size_t)c->W * c->H;
    if (planes4) HIPCHK(c, hipMemcpyAsync(planes4, c->S.planes, wh * 16, hipMemcpyDeviceToHost, c->stream));
    if (costs) HIPCHK(c, hipMemcpyAsync(costs, c->S.costs, wh * 4, hipMemcpyDeviceToHost, c->stream));
    if (geom) HIPCHK(c, hipMemcpyAsync(geom, c->S.geom, wh * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_get_selected_views(mpmvs_ctx* c, void* sel) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.sel) return fail(c, -1, "set_views first");
    HIPCHK(c, hipMemcpyAsync(sel, c->S.sel, (size_t)c->W * c->H * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_export_depth_device(mpmvs_ctx* c, float* d_out) {
    if (!c) return -1;
    ENTER(c);
    if (!c->S.planes) return fail(c, -1, "set_views first");
    const int n = c->W * c->H;
    hipLaunchKernelGGL(k_export_depth, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S.planes, d_out, n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// mapping: 0 = one thread per pixel (k_eval_ncc); the cooperative lane-group mappings 1..4 of round 2 were measured, not
// adopted and removed again (profiles/EXPERIMENTS.md, 10)
static int eval_ncc_impl(mpmvs_ctx* c, const mpmvs_params* p, const void* planes_cam4, int nh, int scale, int mapping, void* out, float* kernel_ms) {
    if (!c || !p) return -1;
    ENTER(c);
    int rc = check_ready(c, p);
    if (rc) return rc;
    if (scale < 0 || scale > 2) return fail(c, -3, "scale must be 0..2");
    if (nh < 1 || mapping != 0) return fail(c, -3, "bad probe arguments (only mapping 0 exists)");
    const size_t wh = (size_t)c->W * c->H;
    const int V = c->hP.V;
    Scratch d_pl(c->stream), d_out(c->stream);
    HIPCHK(c, d_pl.alloc(wh * 16 * nh));
    HIPCHK(c, d_out.alloc(wh * 4 * V * nh));
    HIPCHK(c, hipMemcpyAsync(d_pl.p, planes_cam4, wh * 16 * nh, hipMemcpyHostToDevice, c->stream));
    LaunchArgs a{};
    a.scale = scale;
    a.two_ss = (2.0f * p->sigma_spatial) * p->sigma_spatial;
    a.two_sc = (2.0f * p->sigma_color) * p->sigma_color;
    fill_spatial_terms(a, scale);
    struct Lent {   // two events of the context, back in its pool on every return path
        mpmvs_ctx* c;
        hipEvent_t e0, e1;
        ~Lent() { c->event_pool.insert(c->event_pool.end(), {e0, e1}); }
    } lent{c, get_event(c), get_event(c)};
    const hipEvent_t e0 = lent.e0, e1 = lent.e1;
    HIPCHK(c, hipEventRecord(e0, c->stream));
    {
        const dim3 grid((c->W + 15) / 16, (c->H + 15) / 16);
        const size_t lds = ncc_lds_bytes(16, 16, scale);
        dispatch_variant<false, 8, kMaxViews>(V, c->all_u8, scale, [&](auto maxv, auto u8, auto sc) {
            hipLaunchKernelGGL((k_eval_ncc<maxv, u8, sc>), grid, dim3(256), lds, c->stream, c->dP, d_pl.as<float4>(), nh, d_out.as<float>(), a);
        });
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, wh * 4 * V * nh, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

int mpmvs_eval_ncc(mpmvs_ctx* c, const mpmvs_params* p, const void* planes_cam4, int scale, void* out) {
    return eval_ncc_impl(c, p, planes_cam4, 1, scale, 0, out, nullptr);
}

int mpmvs_eval_ncc_multi(mpmvs_ctx* c, const mpmvs_params* p, const void* planes_cam4, int nh, int scale, int mapping, void* out, float* kernel_ms) {
    return eval_ncc_impl(c, p, planes_cam4, nh, scale, mapping, out, kernel_ms);
}

int mpmvs_eval_geom(mpmvs_ctx* c, const mpmvs_params* p, const void* planes_cam4, void* out) {
    if (!c || !p) return -1;
    ENTER(c);
    if (c->n_img < 2) return fail(c, -1, "set_views first");
    if (!c->have_depths) return fail(c, -4, "need source depth maps");
    const size_t wh = (size_t)c->W * c->H;
    const int V = c->hP.V;
    Scratch d_pl(c->stream), d_out(c->stream);
    HIPCHK(c, d_pl.alloc(wh * 16));
    HIPCHK(c, d_out.alloc(wh * 4 * V));
    HIPCHK(c, hipMemcpyAsync(d_pl.p, planes_cam4, wh * 16, hipMemcpyHostToDevice, c->stream));
    const dim3 grid((c->W + 15) / 16, (c->H + 15) / 16);
    hipLaunchKernelGGL(k_eval_geom, grid, dim3(256), 0, c->stream, c->dP, d_pl.as<float4>(), d_out.as<float>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, wh * 4 * V, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_homography(mpmvs_ctx* c, const void* plane4, int v, void* H9) {
    if (!c) return -1;
    ENTER(c);
    if (c->n_img < 2 || v < 0 || v >= c->hP.V) return fail(c, -1, "bad source view");
    Scratch d_h(c->stream);
    HIPCHK(c, d_h.alloc(9 * 4));
    const float* pf = (const float*)plane4;
    hipLaunchKernelGGL(k_homography, dim3(1), dim3(64), 0, c->stream, c->dP, make_float4(pf[0], pf[1], pf[2], pf[3]), v, d_h.as<float>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(H9, d_h.p, 9 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------
// planar prior on the device (pm_prior.hpp)
// ---------------------------------------------------------------------------
int mpmvs_prior_vertices(mpmvs_ctx* c, int geom_rule, int* out_xy, int cap, int* n_out) {
    if (!c || !out_xy || cap < 0 || !n_out) return -1;
    ENTER(c);
    if (!c->S.costs) return fail(c, -1, "set_views first");
    const int W = c->W, H = c->H;
    const int ncx = (W + kPriorCell - 1) / kPriorCell, ncy = (H + kPriorCell - 1) / kPriorCell, ncells = ncx * ncy;
    const int nb = (ncells + 255) / 256;
    Scratch d_cnt(c->stream), d_pts(c->stream), d_sums(c->stream), d_xy(c->stream);
    int rc = 0, total = 0;
    if (d_cnt.alloc((size_t)ncells * 4) != hipSuccess || d_pts.alloc((size_t)ncells * 12) != hipSuccess || d_sums.alloc((size_t)(nb + 1) * 4) != hipSuccess ||
        d_xy.alloc((size_t)cap * 8) != hipSuccess)
        rc = -100;
    if (!rc) {
        hipLaunchKernelGGL(k_prior_cells, dim3(nb), dim3(256), 0, c->stream, c->S.costs, c->S.geom, W, H, geom_rule ? 1 : 0, ncx, ncells, d_cnt.as<int>(),
                           d_pts.as<uint32_t>());
        hipLaunchKernelGGL(k_scan_tiles, dim3(nb), dim3(256), 0, c->stream, d_cnt.as<int>(), ncells, (int*)nullptr, d_sums.as<int>());
        hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(256), 0, c->stream, d_sums.as<int>(), nb, 0, d_sums.as<int>() + nb);
        hipLaunchKernelGGL(k_prior_scatter, dim3(nb), dim3(256), 0, c->stream, d_cnt.as<int>(), d_pts.as<uint32_t>(), ncells, d_sums.as<int>(), cap, d_xy.as<int>());
        if (hipGetLastError() != hipSuccess) rc = -100;
    }
    if (!rc && hipMemcpyAsync(&total, d_sums.as<int>() + nb, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = -100;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = -100;
    if (!rc && total > 0 &&
        hipMemcpyAsync(out_xy, d_xy.p, (size_t)std::min(total, cap) * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = -100;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = -100;
    if (rc) return fail(c, rc, "prior vertices failed on the device");
    *n_out = total;
    return 0;
}

int mpmvs_prior_from_triangles(mpmvs_ctx* c, const mpmvs_params* p, const int* tri_xy, int n) {
    if (!c || !p || (n > 0 && !tri_xy) || n < 0) return -1;
    ENTER(c);
    if (!c->S.planes) return fail(c, -1, "set_views first");
    const int W = c->W, H = c->H;
    // vertex check and task table in one parallel sweep: 64 consecutive p-rows of one triangle per wave (pm_prior.hpp); a
    // triangle of longest edge L has at most floor(L) + 2 rows (the accumulated p passes 1 after L + 1 steps; the kernel's own
    // p < 1 test is what decides).  Chunks of triangles are counted, their task ranges follow by a prefix sum, then filled:
    // the table is the one the sequential loop would build.
    const size_t wh = (size_t)W * H;
    auto rows_of = [&](int t) {
        const int* v = tri_xy + 6 * (size_t)t;
        const long long e01 = (long long)(v[0] - v[2]) * (v[0] - v[2]) + (long long)(v[1] - v[3]) * (v[1] - v[3]);
        const long long e02 = (long long)(v[0] - v[4]) * (v[0] - v[4]) + (long long)(v[1] - v[5]) * (v[1] - v[5]);
        const long long e12 = (long long)(v[2] - v[4]) * (v[2] - v[4]) + (long long)(v[3] - v[5]) * (v[3] - v[5]);
        return (int)std::sqrt((double)std::max(e01, std::max(e02, e12))) + 3;
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const int nchunks = n >= 65536 ? (int)std::max(1u, std::min(8u, hw ? hw : 1u)) : 1;
    std::vector<size_t> chunk_tasks((size_t)nchunks + 1, 0);
    std::atomic<bool> inside(true);
    auto chunk_range = [&](int ch, int& t0, int& t1) {
        t0 = (int)((long long)n * ch / nchunks);
        t1 = (int)((long long)n * (ch + 1) / nchunks);
    };
    auto in_chunks = [&](auto&& fn) {
        std::vector<std::thread> pool;
        for (int ch = 1; ch < nchunks; ++ch) pool.emplace_back(fn, ch);
        fn(0);
        for (std::thread& t : pool) t.join();
    };
    in_chunks([&](int ch) {
        int t0, t1;
        chunk_range(ch, t0, t1);
        size_t k = 0;
        bool ok = true;
        for (int t = t0; t < t1; ++t) {
            const int* v = tri_xy + 6 * (size_t)t;
            for (int i = 0; i < 6; i += 2) ok &= v[i] >= 0 && v[i] < W && v[i + 1] >= 0 && v[i + 1] < H;
            k += (size_t)(rows_of(t) + 63) / 64;
        }
        chunk_tasks[(size_t)ch + 1] = k;
        if (!ok) inside = false;
    });
    if (!inside) return fail(c, -2, "triangle vertex outside the image");
    for (int k = 0; k < nchunks; ++k) chunk_tasks[(size_t)k + 1] += chunk_tasks[(size_t)k];
    if (chunk_tasks.back() > 0x7fffffffull) return fail(c, -2, "too many raster tasks");
    if (!c->d_prior) HIPCHK(c, pool_malloc(&c->d_prior, wh * 16));
    if (!c->d_mask) HIPCHK(c, pool_malloc(&c->d_mask, wh * 4));
    std::vector<int> task_tri(chunk_tasks.back()), task_row0(chunk_tasks.back());
    in_chunks([&](int ch) {
        int t0, t1;
        chunk_range(ch, t0, t1);
        size_t k = chunk_tasks[(size_t)ch];
        for (int t = t0; t < t1; ++t) {
            const int rows = rows_of(t);
            for (int r0 = 0; r0 < rows; r0 += 64) {
                task_tri[k] = t;
                task_row0[k++] = r0;
            }
        }
    });
    const int n_tasks = (int)task_tri.size();
    Scratch d_tri(c->stream), d_pl(c->stream), d_tt(c->stream), d_tr(c->stream);
    int rc = 0;
    if (d_tri.alloc((size_t)n * 24) != hipSuccess || d_pl.alloc((size_t)n * 16) != hipSuccess || d_tt.alloc((size_t)n_tasks * 4) != hipSuccess ||
        d_tr.alloc((size_t)n_tasks * 4) != hipSuccess)
        rc = -100;
    if (!rc && n > 0 &&
        (hipMemcpyAsync(d_tri.p, tri_xy, (size_t)n * 24, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
         hipMemcpyAsync(d_tt.p, task_tri.data(), (size_t)n_tasks * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
         hipMemcpyAsync(d_tr.p, task_row0.data(), (size_t)n_tasks * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess))
        rc = -100;
    if (!rc && hipMemsetAsync(c->d_mask, 0, wh * 4, c->stream) != hipSuccess) rc = -100;
    if (!rc) {
        if (n_tasks > 0)
            hipLaunchKernelGGL(k_prior_raster, dim3((n_tasks + 3) / 4), dim3(256), 0, c->stream, d_tri.as<int>(), n_tasks, d_tt.as<int>(), d_tr.as<int>(), c->dP,
                               c->S.planes, c->d_mask, d_pl.as<float4>());
        hipLaunchKernelGGL(k_prior_finish, dim3((unsigned)((wh + 255) / 256)), dim3(256), 0, c->stream, c->dP, d_pl.as<float4>(), p->depth_min, p->depth_max,
                           c->d_mask, c->d_prior);
        if (hipGetLastError() != hipSuccess) rc = -100;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = -100;
    if (rc) return fail(c, rc, "prior construction failed on the device");
    c->S.prior = c->d_prior;
    c->S.mask = c->d_mask;
    c->have_prior = true;
    return 0;
}

int mpmvs_get_prior(mpmvs_ctx* c, void* prior4, void* mask) {
    if (!c) return -1;
    ENTER(c);
    if (!c->have_prior) return fail(c, -5, "no prior installed");
    const size_t wh = (size_t)c->W * c->H;
    if (prior4) HIPCHK(c, hipMemcpyAsync(prior4, c->d_prior, wh * 16, hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpyAsync(mask, c->d_mask, wh * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mpmvs_math(int fn, const void* in, void* out, int n) {
    if (fn < 0 || fn > 6 || n <= 0) return -1;
    DeviceCall call;
    float *d_in = call.alloc<float>((size_t)n * 4), *d_out = call.alloc<float>((size_t)n * 4);
    if (!d_in || !d_out) return -100;
    if (hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) return -100;
    hipLaunchKernelGGL(k_math, dim3((n + 255) / 256), dim3(256), 0, call.stream(), fn, d_in, d_out, n);
    if (hipGetLastError() != hipSuccess) return -100;
    return hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}

int mpmvs_verify_rcp(unsigned long long counts[4]) {
    if (!counts) return -1;
    DeviceCall call;
    unsigned long long* d = call.alloc<unsigned long long>(32);
    if (!d || hipMemset(d, 0, 32) != hipSuccess) return -100;
    for (uint64_t base = 0; base < (1ULL << 32); base += (1ULL << 24)) {
        hipLaunchKernelGGL(k_verify_rcp, dim3(1 << 16), dim3(256), 0, call.stream(), (uint32_t)base, d);
        if (hipGetLastError() != hipSuccess) return -100;
    }
    return hipMemcpy(counts, d, 32, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}

int mpmvs_rng(uint64_t seed, uint32_t pix, uint32_t launch_id, int n, void* out) {
    if (n <= 0) return -1;
    DeviceCall call;
    float* d_out = call.alloc<float>((size_t)n * 4);
    if (!d_out) return -100;
    hipLaunchKernelGGL(k_rng, dim3(1), dim3(64), 0, call.stream(), seed, pix, launch_id, n, d_out);
    if (hipGetLastError() != hipSuccess) return -100;
    return hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}

static float g_fuse_kernel_ms = 0.0f;
static int g_fuse_passes_total = 0, g_fuse_passes_max = 0;
// device time of the kernels (and mask copies) of the last mpmvs_fuse call, HIP events
float mpmvs_fuse_kernel_ms(void) { return g_fuse_kernel_ms; }
// passes of the last MPMVS_FUSE_REFERENCE_ORDER call: *total over all images, *max for one image (either may be NULL)
void mpmvs_fuse_passes(int* total, int* max_per_image) {
    if (total) *total = g_fuse_passes_total;
    if (max_per_image) *max_per_image = g_fuse_passes_max;
}

// a failed HIP call ends a fusion call with -100 (no error text); FuseRun's DeviceCall synchronises and frees on the way out
#define FUSECHK(expr) do { if ((expr) != hipSuccess) return -100; } while (0)

extern "C++" {
namespace {
// depth-map fusion, snapshot formulation (pm_fusion.hpp); host buffers in and out (FuseRequest, pm_fusion_host.hpp).  With
// `records` the fused points are compacted on the device into PLY vertex records (reference PointCloud order) and only those cross PCIe.
// ctxs (nullable): per image the PatchMatch context whose device state holds its final maps -- (world normal, depth) per pixel, what
// Run() leaves in cudaPlaneHypotheses and the reference copies out (ref .cu:1246) and writes to depths.dmb / normals.dmb
// (src/PatchMatch.cpp:610-633) for RunFusion to read back (:334-336).  For such an image nothing is uploaded: the planes are split
// into the fusion's depth and normal arrays device to device (k_split_planes), or GPU to GPU when the context lives on another device.
// tracks (nullable, with `records` only): receives per fused point the (image, pixel) pairs that were averaged (pm_fusion.hpp,
// "Tracks").  The device holds one image's tracks at a time; they leave for the host at the image boundary.
// One call is one FuseRun: run() checks the request, stages the views and the tables, fuses image by image in index order
// (fuse_image) and downloads.  Every stage returns 0 or the code the call ends with.
class FuseRun {
    const FuseRequest& q;
    const bool exact;
    DeviceCall call;   // own stream: a fusion call must not stall the PatchMatch contexts other host threads drive on this device
    hipStream_t st = nullptr;
    std::vector<FuseView> hv;   // host mirror of d_views; .mask / .mask_next: the masks the next image sees, the marks of the one being fused
    std::vector<unsigned char*> d_valid;   // per image the per-pixel outputs
    std::vector<float*> d_out;
    size_t total_px = 0, max_blocks = 0, max_wh = 0;   // over the estimated images: pixels, 256-pixel blocks and pixels of the largest
    int max_ngb = 1;                                   // ... and the longest view list
    FuseView* d_views = nullptr;
    int* d_src = nullptr;
    // per source slot the consistent source pixel of every pixel (exact mode), with tracks one more row for the slot bits
    int* d_consq = nullptr;
    struct {   // compaction: per-block counts and their total, the running base, the records of all images
        int* blocks = nullptr;
        long long* base = nullptr;
        unsigned char* out = nullptr;
    } rec;
    struct {   // tracks: lengths, their in-tile scan and tile totals; one image's offsets and entries; the running entry base
        int *len = nullptr, *excl = nullptr, *tiles = nullptr, *ent_image = nullptr, *ent_pixel = nullptr;
        long long *ebase = nullptr, *point_off = nullptr;
    } trk;
    struct { int *carry = nullptr, *diff = nullptr; } ex;   // exact mode: the chunk carries of the scan, the counter of changed marking times
    size_t pixels(int i) const { return (size_t)hv[i].w * hv[i].h; }
    static int launched() { return hipGetLastError() == hipSuccess ? 0 : -100; }   // after the last launch of a stage
    // f(view, ns, blocks) for every source of image i (slots 1 .. num_ngb - 1 of its list; slot 0 is the image itself):
    // ns its pixels, blocks the grid of a one-thread-per-pixel kernel over them
    template <typename F>
    void each_source(int i, F&& f) {
        for (int k = q.src_off[i] + 1; k < q.src_off[i + 1]; ++k) {
            FuseView& v = hv[q.src_ids[k]];
            f(v, v.w * v.h, dim3((v.w * v.h + 255) / 256));
        }
    }
    // k_fuse<EXACT, TRACKS> over image i.  d_consq is null exactly for <false, false>, the one form that writes no row of it.
    void launch_fuse(int i) {
        const int b = q.src_off[i], num_ngb = q.src_off[i + 1] - b;   // 1 .. kMaxFuseNgb: fuse_check_request
        const dim3 grid((hv[i].w + 31) / 32, (hv[i].h + 7) / 8);
        auto launch = [&](auto ex_, auto tr_) {
            hipLaunchKernelGGL((k_fuse<decltype(ex_)::value, decltype(tr_)::value>), grid, dim3(256), 0, st, d_views, i, d_src + b, num_ngb,
                               q.flags & MPMVS_FUSE_DYNAMIC_CONSISTENCY, d_valid[i], d_out[i], d_consq);
        };
        if (!exact)
            q.tracks ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
        else
            q.tracks ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    }
    // Stage a view, the resident case: the maps of image i are in context cx, no upload
    int split_resident(int i, const mpmvs_ctx* cx, float* dd, float* dn) {
        const size_t wh = pixels(i);
        if (cx->W != hv[i].w || cx->H != hv[i].h || !cx->S.planes || !cx->depth_plane_valid || cx->async_outstanding) return -2;   // no finished Run() of that size behind it
        const float4* planes = cx->S.planes;
        if (cx->device == q.device) {
            FUSECHK(hipStreamSynchronize(cx->stream));
        } else {
            // another GPU of the node: its stream is drained there, the planes cross xGMI into a scratch buffer here
            float4* tmp = call.alloc_n<float4>(wh);
            if (!tmp || hipSetDevice(cx->device) != hipSuccess || hipStreamSynchronize(cx->stream) != hipSuccess || hipSetDevice(q.device) != hipSuccess ||
                hipMemcpyPeerAsync(tmp, q.device, cx->S.planes, cx->device, wh * 16, st) != hipSuccess) {
                (void)hipSetDevice(q.device);
                return -100;
            }
            planes = tmp;
        }
        hipLaunchKernelGGL(k_split_planes, dim3((unsigned)((wh + 255) / 256)), dim3(256), 0, st, planes, dd, dn, wh);
        return launched();
    }
    // Stage a view: the buffers of image i, its maps (uploaded, or split from resident planes), colours and sky mask; masks cleared.
    // With `records` the per-pixel outputs of an image are consumed (compacted) before the next image is fused: one buffer
    // of the largest size serves all images (the per-image form would be 37 B per pixel of the whole dataset)
    int stage_view(int i, unsigned char* shared_valid, float* shared_out) {
        FuseView& v = hv[i];
        cam_to_dev(q.cams[i], v.cam);
        v.w = q.cams[i].width, v.h = q.cams[i].height, v.cch = q.color_channels;
        const size_t wh = pixels(i);
        const bool has_sky = q.sky && q.sky[i];
        float *dd = call.alloc_n<float>(wh), *dn = call.alloc_n<float>(wh * 3);
        unsigned char* dg = call.alloc_n<unsigned char>(wh * q.color_channels);
        unsigned char* dsky = has_sky ? call.alloc_n<unsigned char>(wh) : nullptr;
        v.mask = call.alloc_n<unsigned char>(wh), v.mask_next = call.alloc_n<unsigned char>(wh);
        d_valid[i] = q.records ? shared_valid : call.alloc_n<unsigned char>(wh);
        d_out[i] = q.records ? shared_out : call.alloc_n<float>(wh * 9);
        v.tau = exact ? call.alloc_n<int>(wh) : nullptr, v.tau_new = exact ? call.alloc_n<int>(wh) : nullptr;
        if (!dd || !dn || !dg || (has_sky && !dsky) || !v.mask || !v.mask_next || !d_valid[i] || !d_out[i] || (exact && (!v.tau || !v.tau_new))) return -100;
        v.depth = dd, v.normal = dn, v.color = dg, v.sky = dsky;
        if (mpmvs_ctx* const cx = q.ctxs ? q.ctxs[i] : nullptr) {
            if (const int rc = split_resident(i, cx, dd, dn)) return rc;
        } else if (!q.depths || !q.normals || !q.depths[i] || !q.normals[i]) {
            return -2;
        } else {
            FUSECHK(hipMemcpyAsync(dd, q.depths[i], wh * 4, hipMemcpyHostToDevice, st));
            FUSECHK(hipMemcpyAsync(dn, q.normals[i], wh * 12, hipMemcpyHostToDevice, st));
        }
        FUSECHK(hipMemcpyAsync(dg, q.colors[i], wh * q.color_channels, hipMemcpyHostToDevice, st));
        if (dsky) FUSECHK(hipMemcpyAsync(dsky, q.sky[i], wh, hipMemcpyHostToDevice, st));
        FUSECHK(hipMemsetAsync(v.mask, 0, wh, st));
        FUSECHK(hipMemsetAsync(v.mask_next, 0, wh, st));
        if (!q.records) FUSECHK(hipMemsetAsync(d_valid[i], 0, wh, st));
        if (!q.records) FUSECHK(hipMemsetAsync(d_out[i], 0, wh * 36, st));
        return 0;
    }
    // Stage the tables: the views and the source ids, then the scratch of compaction, tracks and exact mode
    int stage_tables() {
        const int n = q.n, n_ids = q.src_off[n];
        d_views = call.alloc_n<FuseView>(n);
        d_src = call.alloc_n<int>(n_ids > 0 ? n_ids : 1);
        if (!d_views || !d_src) return -100;
        FUSECHK(hipMemcpyAsync(d_views, hv.data(), sizeof(FuseView) * n, hipMemcpyHostToDevice, st));
        FUSECHK(hipMemcpyAsync(d_src, q.src_ids, sizeof(int) * n_ids, hipMemcpyHostToDevice, st));
        if (q.records) {
            rec.blocks = call.alloc_n<int>(max_blocks + 1);
            rec.base = call.alloc_n<long long>(1);
            rec.out = call.alloc_n<unsigned char>(total_px * kPlyRecord);  // upper bound: every pixel a point
            if (!rec.blocks || !rec.base || !rec.out) return -100;
            FUSECHK(hipMemsetAsync(rec.base, 0, sizeof(long long), st));
        }
        // rows of max_wh: tracks read every slot's row and one of slot bits, exact mode alone the source slots', the plain snapshot none
        const size_t consq_rows = q.tracks ? (size_t)max_ngb : exact ? (size_t)std::max(max_ngb - 1, 1) : 0;
        if (consq_rows && !(d_consq = call.alloc_n<int>(consq_rows * max_wh))) return -100;
        if (q.tracks) {
            trk.len = call.alloc_n<int>(max_wh), trk.excl = call.alloc_n<int>(max_wh), trk.tiles = call.alloc_n<int>(max_blocks + 1);
            trk.ent_image = call.alloc_n<int>((size_t)max_ngb * max_wh), trk.ent_pixel = call.alloc_n<int>((size_t)max_ngb * max_wh);
            trk.point_off = call.alloc_n<long long>(max_wh), trk.ebase = call.alloc_n<long long>(1);
            if (!trk.len || !trk.excl || !trk.tiles || !trk.ent_image || !trk.ent_pixel || !trk.point_off || !trk.ebase) return -100;
            FUSECHK(hipMemsetAsync(trk.ebase, 0, sizeof(long long), st));
        }
        if (exact) {
            ex.carry = call.alloc_n<int>((size_t)std::max(max_ngb - 1, 1) * ((max_wh + 255) / 256));
            ex.diff = call.alloc_n<int>(1);
            if (!ex.carry || !ex.diff) return -100;
        }
        return 0;
    }
    // Fuse one image by snapshot: all its pixels read the masks as they were when the image started
    int fuse_snapshot(int i) {
        launch_fuse(i);
        FUSECHK(hipGetLastError());
        // the marks of image i become the masks the next image sees
        bool ok = true;
        each_source(i, [&](FuseView& v, int ns, dim3) { ok &= hipMemcpyAsync(v.mask, v.mask_next, (size_t)ns, hipMemcpyDeviceToDevice, st) == hipSuccess; });
        return ok ? 0 : -100;
    }
    // Fuse one image by fixpoint over tau (pm_fusion.hpp), the reference's sequential masking order: every pass re-evaluates all
    // pixels of the image against the marking times of the previous pass; ends when the marking times repeat.  A pass counts
    // for mpmvs_fuse_passes once it is started, also when it fails
    int fuse_fixpoint(int i) {
        const int b = q.src_off[i], num_ngb = q.src_off[i + 1] - b;
        const int npix = hv[i].w * hv[i].h, nchunks = (npix + 255) / 256;
        each_source(i, [&](FuseView& v, int ns, dim3 blocks) { hipLaunchKernelGGL(k_fuse_tau_init, blocks, dim3(256), 0, st, v.mask, ns, v.tau); });
        for (int passes = 1, changed = 1; changed; ++passes) {
            ++g_fuse_passes_total;
            g_fuse_passes_max = std::max(g_fuse_passes_max, passes);
            each_source(i, [&](FuseView& v, int ns, dim3 blocks) { hipLaunchKernelGGL(k_fuse_tau_init, blocks, dim3(256), 0, st, v.mask, ns, v.tau_new); });
            launch_fuse(i);
            if (num_ngb > 1) {
                hipLaunchKernelGGL(k_fuse_carry_local, dim3(nchunks, num_ngb - 1), dim3(256), 0, st, d_consq, npix, nchunks, ex.carry);
                hipLaunchKernelGGL(k_scan_totals<LastValid>, dim3(num_ngb - 1), dim3(256), 0, st, ex.carry, nchunks, -1, (int*)nullptr);
                hipLaunchKernelGGL(k_fuse_mark, dim3(nchunks), dim3(256), 0, st, d_views, d_src + b, num_ngb, d_valid[i], d_consq, ex.carry, npix, nchunks);
            }
            FUSECHK(hipMemsetAsync(ex.diff, 0, 4, st));
            each_source(i, [&](FuseView& v, int ns, dim3 blocks) { hipLaunchKernelGGL(k_fuse_tau_diff, blocks, dim3(256), 0, st, v.tau, v.tau_new, ns, ex.diff); });
            FUSECHK(hipGetLastError());
            FUSECHK(hipMemcpyAsync(&changed, ex.diff, 4, hipMemcpyDeviceToHost, st));
            FUSECHK(hipStreamSynchronize(st));
            each_source(i, [&](FuseView& v, int, dim3) { std::swap(v.tau, v.tau_new); });
            FUSECHK(hipMemcpyAsync(d_views, hv.data(), sizeof(FuseView) * q.n, hipMemcpyHostToDevice, st));
            // changed == 0: tau (now in .tau) reproduces itself, the sequential result.  Every pass fixes at least one more pixel; measured <= 7 per image
            if (changed && (passes > npix || passes > 4096)) return -3;
        }
        each_source(i, [&](FuseView& v, int ns, dim3 blocks) { hipLaunchKernelGGL(k_fuse_tau_to_mask, blocks, dim3(256), 0, st, v.tau, ns, v.mask); });
        return launched();
    }
    // Compact records: the valid pixels of image i, in raster order, behind those of the images before it
    int compact_records(int i) {
        const int wh = hv[i].w * hv[i].h, nb = (wh + 255) / 256;
        hipLaunchKernelGGL(k_fuse_count, dim3(nb), dim3(256), 0, st, d_valid[i], wh, rec.blocks);
        hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(256), 0, st, rec.blocks, nb, 0, rec.blocks + nb);
        hipLaunchKernelGGL(k_fuse_scatter, dim3(nb), dim3(256), 0, st, d_valid[i], d_out[i], wh, rec.blocks, rec.base, rec.out);
        hipLaunchKernelGGL(k_fuse_advance, dim3(1), dim3(1), 0, st, rec.base, rec.blocks + nb);
        return launched();
    }
    // Ship one image's tracks (after compact_records(i), whose block counts it reads): built on the device, appended to the host sink
    int ship_tracks(int i) {
        const int b = q.src_off[i], num_ngb = q.src_off[i + 1] - b;
        const int wh = hv[i].w * hv[i].h, nb = (wh + 255) / 256;
        hipLaunchKernelGGL(k_fuse_track_len, dim3(nb), dim3(256), 0, st, d_valid[i], d_consq + (size_t)(num_ngb - 1) * wh, wh, trk.len);
        hipLaunchKernelGGL(k_scan_tiles, dim3(nb), dim3(256), 0, st, trk.len, wh, trk.excl, trk.tiles);
        hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(256), 0, st, trk.tiles, nb, 0, trk.tiles + nb);
        hipLaunchKernelGGL(k_fuse_track_scatter, dim3(nb), dim3(256), 0, st, d_valid[i], d_consq, wh, i, d_src + b, num_ngb, rec.blocks, trk.tiles, trk.excl,
                           trk.ebase, trk.point_off, trk.ent_image, trk.ent_pixel);
        hipLaunchKernelGGL(k_fuse_advance, dim3(1), dim3(1), 0, st, trk.ebase, trk.tiles + nb);
        // the image's tracks leave before the next image reuses the buffers: its two counts first, then what they size
        int got[2] = {0, 0};
        FUSECHK(hipGetLastError());
        FUSECHK(hipMemcpyAsync(&got[0], rec.blocks + nb, 4, hipMemcpyDeviceToHost, st));
        FUSECHK(hipMemcpyAsync(&got[1], trk.tiles + nb, 4, hipMemcpyDeviceToHost, st));
        FUSECHK(hipStreamSynchronize(st));
        if (got[0] < 0 || got[0] > wh || got[1] < got[0] || (long long)got[1] > (long long)wh * num_ngb) return -100;
        TrackSink& sink = *q.tracks;
        if (!sink.reserve((size_t)got[0], (size_t)got[1])) return -101;
        if (got[0] > 0) {
            FUSECHK(hipMemcpyAsync(sink.off_tail(), trk.point_off, (size_t)got[0] * 8, hipMemcpyDeviceToHost, st));
            FUSECHK(hipMemcpyAsync(sink.image_tail(), trk.ent_image, (size_t)got[1] * 4, hipMemcpyDeviceToHost, st));
            FUSECHK(hipMemcpyAsync(sink.pixel_tail(), trk.ent_pixel, (size_t)got[1] * 4, hipMemcpyDeviceToHost, st));
            FUSECHK(hipStreamSynchronize(st));
        }
        return sink.commit((size_t)got[0], (size_t)got[1]) ? 0 : -100;
    }
    // one estimated image: fused, then (with `records`) compacted and its tracks shipped before the next image reuses the buffers
    int fuse_image(int i) {
        if (q.records) FUSECHK(hipMemsetAsync(d_valid[i], 0, pixels(i), st));
        if (const int rc = exact ? fuse_fixpoint(i) : fuse_snapshot(i)) return rc;
        if (!q.records) return 0;
        if (const int rc = compact_records(i)) return rc;
        return q.tracks ? ship_tracks(i) : 0;
    }
    // Download: the per-pixel outputs and masks that were asked for, then the records; handed over once all have arrived
    int download() {
        for (int i = 0; i < q.n; ++i) {
            const size_t wh = pixels(i);
            if (q.out_valid) FUSECHK(hipMemcpyAsync(q.out_valid[i], d_valid[i], wh, hipMemcpyDeviceToHost, st));
            if (q.out_points9) FUSECHK(hipMemcpyAsync(q.out_points9[i], d_out[i], wh * 36, hipMemcpyDeviceToHost, st));
            if (q.out_masks) FUSECHK(hipMemcpyAsync(q.out_masks[i], hv[i].mask, wh, hipMemcpyDeviceToHost, st));
        }
        std::unique_ptr<unsigned char, void (*)(void*)> host(nullptr, std::free);   // released unless the records are handed over
        long long count = 0;
        if (q.records) {
            FUSECHK(hipMemcpyAsync(&count, rec.base, sizeof(count), hipMemcpyDeviceToHost, st));
            FUSECHK(hipStreamSynchronize(st));
            host.reset((unsigned char*)std::malloc(count > 0 ? (size_t)count * kPlyRecord : 1));
            if (!host) return -101;
            if (count > 0) FUSECHK(hipMemcpyAsync(host.get(), rec.out, (size_t)count * kPlyRecord, hipMemcpyDeviceToHost, st));
            if (q.tracks && (long long)q.tracks->points() != count) return -100;
        }
        FUSECHK(hipStreamSynchronize(st));   // the outputs have arrived
        if (q.records) {
            *q.records = host.release();
            *q.n_records = count;
        }
        return 0;
    }
   public:
    explicit FuseRun(const FuseRequest& request) : q(request), exact((request.flags & MPMVS_FUSE_REFERENCE_ORDER) != 0), call(request.device) {}
    int run() {
        g_fuse_passes_total = g_fuse_passes_max = 0;
        if (const int rc = fuse_check_request(q, call.entered(), kMaxFuseNgb)) return rc;
        if (!call.ok()) return -100;
        st = call.stream();
        const int n = q.n;
        hv.resize(n), d_valid.assign(n, nullptr), d_out.assign(n, nullptr);
        for (int i = 0; i < n; ++i)
            if (q.estimate[i]) {
                const size_t wh = (size_t)q.cams[i].width * q.cams[i].height;
                total_px += wh, max_wh = std::max(max_wh, wh), max_blocks = std::max(max_blocks, (wh + 255) / 256);
                max_ngb = std::max(max_ngb, q.src_off[i + 1] - q.src_off[i]);
            }
        unsigned char* shared_valid = q.records ? call.alloc_n<unsigned char>(max_wh) : nullptr;
        float* shared_out = q.records ? call.alloc_n<float>(max_wh * 9) : nullptr;
        if (q.records && (!shared_valid || !shared_out)) return -100;
        for (int i = 0; i < n; ++i)
            if (const int rc = stage_view(i, shared_valid, shared_out)) return rc;
        if (const int rc = stage_tables()) return rc;
        (void)call.begin();
        for (int i = 0; i < n; ++i)
            if (q.estimate[i])
                if (const int rc = fuse_image(i)) return rc;
        (void)call.end();
        FUSECHK(hipStreamSynchronize(st));
        (void)call.elapsed(&g_fuse_kernel_ms);   // written on success only
        return download();
    }
};
}  // namespace
}  // extern "C++"

// the record forms: the count, or the code
static long long fuse_run_records(FuseRequest q, unsigned char** records, TrackSink* tracks = nullptr) {
    long long count = 0;
    q.records = records, q.n_records = &count, q.tracks = tracks;
    const int rc = FuseRun(q).run();
    return rc ? rc : count;
}

// The ctx forms take maps that are still resident in the PatchMatch contexts that estimated them (ctxs[i] != NULL: depths[i] /
// normals[i] are not read and may be NULL; depths / normals themselves may be NULL when every image has a context); ctxs NULL:
// host arrays only, which is what the forms without ctxs are.
int mpmvs_fuse_ctx(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs, const float* const* depths, const float* const* normals,
                   const unsigned char* const* colors, int color_channels, const unsigned char* const* sky, const int* src_off, const int* src_ids,
                   int use_dynamic, unsigned char* const* out_valid, float* const* out_points9, unsigned char* const* out_masks) {
    if (!out_valid || !out_points9 || !out_masks) return -1;
    return FuseRun({device, n, cams, estimate, ctxs, depths, normals, colors, color_channels, sky, src_off, src_ids, use_dynamic, out_valid, out_points9, out_masks}).run();
}

int mpmvs_fuse(int device, int n, const mpmvs_camera* cams, const int* estimate, const float* const* depths, const float* const* normals,
               const unsigned char* const* colors, int color_channels, const unsigned char* const* sky, const int* src_off, const int* src_ids,
               int use_dynamic, unsigned char* const* out_valid, float* const* out_points9, unsigned char* const* out_masks) {
    return mpmvs_fuse_ctx(device, n, cams, estimate, nullptr, depths, normals, colors, color_channels, sky, src_off, src_ids, use_dynamic, out_valid, out_points9,
                          out_masks);
}

long long mpmvs_fuse_ply_ctx(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs, const float* const* depths,
                             const float* const* normals, const unsigned char* const* colors, int color_channels, const unsigned char* const* sky,
                             const int* src_off, const int* src_ids, int use_dynamic, unsigned char** records, unsigned char* const* out_masks) {
    if (!records) return -1;
    return fuse_run_records({device, n, cams, estimate, ctxs, depths, normals, colors, color_channels, sky, src_off, src_ids, use_dynamic, nullptr, nullptr, out_masks},
                            records);
}

long long mpmvs_fuse_ply(int device, int n, const mpmvs_camera* cams, const int* estimate, const float* const* depths, const float* const* normals,
                         const unsigned char* const* colors, int color_channels, const unsigned char* const* sky, const int* src_off,
                         const int* src_ids, int use_dynamic, unsigned char** records, unsigned char* const* out_masks) {
    return mpmvs_fuse_ply_ctx(device, n, cams, estimate, nullptr, depths, normals, colors, color_channels, sky, src_off, src_ids, use_dynamic, records, out_masks);
}

// mpmvs_fuse_ply_ctx that also returns every point's track (include/mpmvs.h); ctxs may be NULL
long long mpmvs_fuse_ply_tracks(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs, const float* const* depths,
                                const float* const* normals, const unsigned char* const* colors, int color_channels, const unsigned char* const* sky,
                                const int* src_off, const int* src_ids, int use_dynamic, unsigned char** records, long long** track_off,
                                int32_t** track_image, int32_t** track_pixel, unsigned char* const* out_masks) {
    if (!records) return -1;
    if (!track_off || !track_image || !track_pixel) return -2;
    unsigned char* rec = nullptr;
    TrackSink sink;
    const long long count = fuse_run_records(
        {device, n, cams, estimate, ctxs, depths, normals, colors, color_channels, sky, src_off, src_ids, use_dynamic, nullptr, nullptr, out_masks}, &rec, &sink);
    if (count < 0) return count;   // nothing was handed over
    if (!sink.finish(track_off, track_image, track_pixel)) {
        std::free(rec);
        return -101;
    }
    *records = rec;
    return count;
}

void mpmvs_free(void* p) { std::free(p); }

static float g_sky_kernel_ms = 0.0f;
float mpmvs_sky_kernel_ms(void) { return g_sky_kernel_ms; }

// joint-bilateral sky-mask refinement (pm_sky.hpp); host buffers in and out
int mpmvs_sky_bilateral(int device, const unsigned char* bgr, const float* mask, float* out, int height, int width) {
    DeviceCall call(device);
    if (!bgr || !mask || !out || height <= 0 || width <= 0 || !call.entered()) return -1;
    if (!call.ok()) return -100;
    const hipStream_t st = call.stream();
    const size_t wh = (size_t)height * width;
    unsigned char* d_img = call.alloc<unsigned char>(wh * 3);
    float *d_mask = call.alloc<float>(wh * 4), *d_out = call.alloc<float>(wh * 4);
    if (!d_img || !d_mask || !d_out) return -100;
    if (hipMemcpyAsync(d_img, bgr, wh * 3, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(d_mask, mask, wh * 4, hipMemcpyHostToDevice, st) != hipSuccess)
        return -100;
    (void)call.begin();
    const dim3 grid((width + kSkyTW - 1) / kSkyTW, (height + kSkyTH - 1) / kSkyTH);
    hipLaunchKernelGGL(k_sky_bilateral, grid, dim3(256), 0, st, d_img, d_mask, d_out, height, width);
    if (hipGetLastError() != hipSuccess) return -100;
    (void)call.end();
    if (hipStreamSynchronize(st) != hipSuccess) return -100;
    (void)call.elapsed(&g_sky_kernel_ms);
    if (hipMemcpyAsync(out, d_out, wh * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -100;
    return 0;
}

static float g_viewsel_kernel_ms = 0.0f;
float mpmvs_view_select_kernel_ms(void) { return g_viewsel_kernel_ms; }

// view selection of a COLMAP model (pm_viewsel.hpp); host buffers in and out.  Every index the kernels follow is checked
// here first: obs_off ascends from 0, obs_pt lies in [-1, n_points), and the track slots fit an int.
int mpmvs_view_select(int device, int n_images, const double* centers, int n_points, const double* xyz, const int64_t* obs_off,
                      const int32_t* obs_pt, int num_view, int32_t* out_ids, int32_t* out_scores, uint32_t* shared, uint32_t* small) {
    if (n_images <= 0 || n_points < 0 || num_view < 0 || num_view > n_images || !centers || !obs_off || !out_ids || !out_scores ||
        (n_points > 0 && !xyz))
        return -1;
    if (n_images > kVsMaxImages) return -2;
    if (obs_off[0] != 0) return -1;
    for (int i = 0; i < n_images; ++i)
        if (obs_off[i + 1] < obs_off[i]) return -1;
    const int64_t n_obs = obs_off[n_images];
    if (n_obs > 0 && !obs_pt) return -1;
    int64_t n_slots = 0;
    for (int64_t k = 0; k < n_obs; ++k) {
        if (obs_pt[k] < -1 || obs_pt[k] >= n_points) return -1;
        n_slots += obs_pt[k] >= 0;
    }
    if (n_obs > INT32_MAX || n_slots > INT32_MAX - 256) return -1;
    DeviceCall call(device);
    if (!call.ok()) return -100;
    const hipStream_t st = call.stream();

    const size_t n = (size_t)n_images, nn = n * n;
    const int ntiles = (n_points + kScanBlock - 1) / kScanBlock;
    const int ns = (int)n_slots;
    double *d_centers = call.alloc<double>(n * 24), *d_xyz = call.alloc<double>((size_t)n_points * 24);
    int64_t* d_obs_off = call.alloc<int64_t>((n + 1) * 8);
    int32_t* d_obs_pt = call.alloc<int32_t>((size_t)n_obs * 4);
    int *d_cnt = call.alloc<int>((size_t)n_points * 4), *d_off = call.alloc<int>(((size_t)n_points + 1) * 4);
    int *d_tsum = call.alloc<int>((size_t)ntiles * 4), *d_fill = call.alloc<int>((size_t)n_points * 4);
    int *d_trk_img = call.alloc<int>((size_t)ns * 4), *d_trk_pt = call.alloc<int>((size_t)ns * 4), *d_trk_mult = call.alloc<int>((size_t)ns * 4);
    unsigned long long* d_acc = call.alloc<unsigned long long>(nn * 8);
    unsigned* d_score = call.alloc<unsigned>(nn * 4);
    int32_t *d_ids = call.alloc<int32_t>(n * num_view * 4), *d_scores = call.alloc<int32_t>(n * num_view * 4);
    if (!d_centers || !d_xyz || !d_obs_off || !d_obs_pt || !d_cnt || !d_off || !d_tsum || !d_fill || !d_trk_img || !d_trk_pt || !d_trk_mult || !d_acc ||
        !d_score || !d_ids || !d_scores)
        return -100;
    // (a zero-sized array has a 4-byte buffer: that much is cleared)
    auto bytes = [](size_t b) { return b ? b : (size_t)4; };
    if (hipMemcpyAsync(d_centers, centers, n * 24, hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_points > 0 && hipMemcpyAsync(d_xyz, xyz, (size_t)n_points * 24, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(d_obs_off, obs_off, (n + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_obs > 0 && hipMemcpyAsync(d_obs_pt, obs_pt, (size_t)n_obs * 4, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemsetAsync(d_cnt, 0, bytes((size_t)n_points * 4), st) != hipSuccess || hipMemsetAsync(d_off, 0, ((size_t)n_points + 1) * 4, st) != hipSuccess ||
        hipMemsetAsync(d_fill, 0, bytes((size_t)n_points * 4), st) != hipSuccess || hipMemsetAsync(d_acc, 0, nn * 8, st) != hipSuccess)
        return -100;
    (void)call.begin();
    if (n_slots > 0) {
        hipLaunchKernelGGL(k_vs_count, dim3(n_images), dim3(256), 0, st, d_obs_off, d_obs_pt, d_cnt);
        hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, st, d_cnt, n_points, d_off, d_tsum);
        hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(kScanBlock), 0, st, d_tsum, ntiles, 0, d_off + n_points);
        hipLaunchKernelGGL(k_vs_scan_add, dim3(ntiles), dim3(kScanBlock), 0, st, d_off, n_points, d_tsum);
        hipLaunchKernelGGL(k_vs_scatter, dim3(n_images), dim3(256), 0, st, d_obs_off, d_obs_pt, d_off, d_fill, d_trk_img, d_trk_pt);
        const dim3 gs((ns + 255) / 256);
        hipLaunchKernelGGL(k_vs_mult, gs, dim3(256), 0, st, ns, d_trk_img, d_trk_pt, d_off, d_trk_mult);
        hipLaunchKernelGGL(k_vs_pairs, gs, dim3(256), 0, st, ns, d_trk_img, d_trk_pt, d_trk_mult, d_off, d_centers, d_xyz, d_acc, n_images);
    }
    hipLaunchKernelGGL(k_vs_score, dim3((n_images + 255) / 256, n_images), dim3(256), 0, st, d_acc, n_images, d_score);
    if (num_view > 0) hipLaunchKernelGGL(k_vs_select, dim3(n_images), dim3(256), 0, st, d_score, n_images, num_view, d_ids, d_scores);
    if (hipGetLastError() != hipSuccess) return -100;
    (void)call.end();
    if (hipStreamSynchronize(st) != hipSuccess) return -100;
    (void)call.elapsed(&g_viewsel_kernel_ms);
    if (num_view > 0 && (hipMemcpyAsync(out_ids, d_ids, n * num_view * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(out_scores, d_scores, n * num_view * 4, hipMemcpyDeviceToHost, st) != hipSuccess))
        return -100;
    std::vector<unsigned long long> acc;
    if (shared || small) {
        acc.resize(nn);
        if (hipMemcpyAsync(acc.data(), d_acc, nn * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return -100;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return -100;
    for (size_t k = 0; k < acc.size(); ++k) {
        if (shared) shared[k] = (uint32_t)(acc[k] >> 32);
        if (small) small[k] = (uint32_t)(acc[k] & 0xffffffffull);
    }
    return 0;
}

// the output camera of the undistortion (pm_undistort_model.hpp: und_output_camera); host only, touches no device
int mpmvs_undistort_camera(int model_id, const double* params, int n_params, int width, int height, double blank_pixels, double min_scale,
                           double max_scale, double out_pinhole[4], int* out_width, int* out_height) {
    UndModel m;
    if (!out_pinhole || !out_width || !out_height || !und_model_init(m, model_id, params, n_params) ||
        !und_options_ok(width, height, blank_pixels, min_scale, max_scale))
        return -2;
    int w = 0, h = 0;
    double k[4];
    if (!und_output_camera(m, width, height, blank_pixels, min_scale, max_scale, k, w, h)) return -2;
    std::memcpy(out_pinhole, k, sizeof k);
    *out_width = w;
    *out_height = h;
    return 0;
}

static thread_local float g_undistort_kernel_ms = 0.0f;   // per calling thread: concurrent calls do not overwrite each other's reading
float mpmvs_undistort_kernel_ms(void) { return g_undistort_kernel_ms; }

// the undistortion warp (pm_undistort.hpp); host buffers in and out
int mpmvs_undistort_u8(int device, const unsigned char* src, int channels, int width, int height, size_t pitch_bytes, int model_id,
                       const double* params, int n_params, const double dst_pinhole[4], int dst_width, int dst_height, unsigned char* out,
                       unsigned char* out_valid) {
    UndModel m;
    if (!src || !out || !dst_pinhole || (channels != 1 && channels != 3) || width <= 0 || height <= 0 || dst_width <= 0 || dst_height <= 0 ||
        !und_model_init(m, model_id, params, n_params))
        return -2;
    const size_t row = (size_t)width * channels;
    if (pitch_bytes == 0) pitch_bytes = row;
    if (pitch_bytes < row) return -2;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(dst_pinhole[i])) return -2;
    if (!(dst_pinhole[0] > 0.0) || !(dst_pinhole[1] > 0.0)) return -2;
    const size_t n_pix = (size_t)dst_width * dst_height, out_bytes = n_pix * channels, src_bytes = row * height;
    if (out_bytes >= (1ull << 31) || row >= (1ull << 31) || src_bytes >= (1ull << 40)) return -3;
    PinnedBuf pinned;   // (outlives the call's stream work: destroyed after `call`)
    DeviceCall call(device);
    if (!call.ok()) return -100;
    const hipStream_t st = call.stream();
    // one page-locked stage for the three host arrays (each part starts on a 16-byte boundary; the outputs are rounded up to the
    // dword the kernel stores last)
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_out = up16(src_bytes), o_valid = o_out + up16(out_bytes), stage_bytes = o_valid + up16(n_pix);
    unsigned char* const stage = (unsigned char*)(pinned.p = mpmvs_alloc_pinned(stage_bytes));
    if (!stage) return -100;
    unsigned char *d_src = call.alloc<unsigned char>(up16(src_bytes)), *d_out = call.alloc<unsigned char>(up16(out_bytes));
    unsigned char* d_valid = out_valid ? call.alloc<unsigned char>(up16(n_pix)) : nullptr;
    if (!d_src || !d_out || (out_valid && !d_valid)) return -100;
    for (int y = 0; y < height; ++y) std::memcpy(stage + (size_t)y * row, src + (size_t)y * pitch_bytes, row);
    if (hipMemcpyAsync(d_src, stage, src_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -100;
    if (!call.begin()) return -100;
    UndPinhole dst;
    std::memcpy(dst.p, dst_pinhole, sizeof dst.p);
    const dim3 grid((unsigned)((n_pix + kUndThreads - 1) / kUndThreads));
    if (channels == 1)
        hipLaunchKernelGGL(k_undistort<1>, grid, dim3(kUndThreads), 0, st, m, dst, d_src, (unsigned)row, width, height, dst_width, (unsigned)n_pix,
                           (unsigned*)d_out, (unsigned*)d_valid);
    else
        hipLaunchKernelGGL(k_undistort<3>, grid, dim3(kUndThreads), 0, st, m, dst, d_src, (unsigned)row, width, height, dst_width, (unsigned)n_pix,
                           (unsigned*)d_out, (unsigned*)d_valid);
    if (hipGetLastError() != hipSuccess || !call.end()) return -100;
    if (hipMemcpyAsync(stage + o_out, d_out, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (out_valid && hipMemcpyAsync(stage + o_valid, d_valid, n_pix, hipMemcpyDeviceToHost, st) != hipSuccess))
        return -100;
    if (hipStreamSynchronize(st) != hipSuccess || !call.elapsed(&g_undistort_kernel_ms)) return -100;
    std::memcpy(out, stage + o_out, out_bytes);
    if (out_valid) std::memcpy(out_valid, stage + o_valid, n_pix);
    return 0;
}

void* mpmvs_device_alloc(int device, size_t bytes) {
    if (bytes == 0 || enter_device(device) != hipSuccess) return nullptr;
    void* p = nullptr;
    if (pool_malloc_bytes(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void mpmvs_device_free(int device, void* p) {
    if (!p || enter_device(device) != hipSuccess) return;
    (void)pool_free(p);
}

void* mpmvs_alloc_pinned(size_t bytes) {
    if (bytes == 0) bytes = 4;
    static const bool trace = std::getenv("MPMVS_TRACE_PINNED") != nullptr;  // debugging aid: pool hits and misses on stderr
    {
        std::lock_guard<std::mutex> lk(g_pinned.mu);
        auto it = g_pinned.cached.find(bytes);
        if (it != g_pinned.cached.end() && !it->second.empty()) {
            void* p = it->second.back();
            it->second.pop_back();
            g_pinned.cached_bytes -= bytes;
            if (trace) std::fprintf(stderr, "[mpmvs] pinned %zu B: from the pool\n", bytes);
            return p;
        }
    }
    void* p = nullptr;
    (void)hipGetLastError();
    if (trace) std::fprintf(stderr, "[mpmvs] pinned %zu B: hipHostMalloc\n", bytes);
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_pinned.mu);
    g_pinned.owner[p] = bytes;
    return p;
}

void mpmvs_free_pinned(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pinned.mu);
        auto it = g_pinned.owner.find(p);
        if (it == g_pinned.owner.end()) return;  // not ours
        if (g_pinned.cached_bytes + it->second <= g_pinned.cap) {
            g_pinned.cached[it->second].push_back(p);
            g_pinned.cached_bytes += it->second;
            return;
        }
        g_pinned.owner.erase(it);
    }
    (void)hipHostFree(p);
}

int mpmvs_set_texture_format(mpmvs_ctx* c, int force_fp32) {
    if (!c) return -1;
    c->force_f32 = force_fp32 != 0;
    own_invalidate(c);
    return 0;
}

int mpmvs_texture_format(mpmvs_ctx* c) {
    if (!c) return -1;
    return c->all_u8 ? 1 : 0;
}

int mpmvs_set_profiling(mpmvs_ctx* c, int enable) {
    if (!c) return -1;
    c->profiling = enable != 0;
    return 0;
}

// How `device` reaches `peer` (the path hipMemcpyPeerAsync of mpmvs_set_src_depths_mixed / mpmvs_fuse_*_ctx takes, and RCCL between
// the ranks of a node): *can_access = hipDeviceCanAccessPeer, *link_type / *hops = hipExtGetLinkTypeAndHopCount (link type 4 = xGMI,
// 2 = PCIe; -1 where the runtime does not say).  The reference has one device and no such question (src/PatchMatch.cpp:509).
int mpmvs_peer_info(int device, int peer, int* can_access, int* link_type, int* hops) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || peer < 0 || device >= n || peer >= n) return -1;
    int can = device == peer ? 1 : 0;
    if (device != peer && hipDeviceCanAccessPeer(&can, device, peer) != hipSuccess) {
        (void)hipGetLastError();
        can = -1;
    }
    uint32_t lt = 0, hc = 0;
    int ilt = -1, ihc = -1;
    if (device != peer && hipExtGetLinkTypeAndHopCount(device, peer, &lt, &hc) == hipSuccess) {
        ilt = (int)lt;
        ihc = (int)hc;
    } else {
        (void)hipGetLastError();
        if (device == peer) ihc = 0;
    }
    if (can_access) *can_access = can;
    if (link_type) *link_type = ilt;
    if (hops) *hops = ihc;
    return 0;
}

int mpmvs_chain_status(mpmvs_ctx* c) {
    if (!c) return 0;
    return c->chain ? 1 : (c->chain_failed_check ? -1 : 0);
}

int mpmvs_dbg_chain_stall(mpmvs_ctx* c, int block_pos, int spin_limit) {
    if (!c) return -1;
    c->dbg_stall_pos = block_pos < 0 ? -1 : block_pos;
    c->spin_limit = spin_limit > 0 ? spin_limit : kSpinLimit;
    return 0;
}

int mpmvs_dbg_own_costs(mpmvs_ctx* c, int enable, int* passes_served) {
    if (!c) return -1;
    if (enable >= 0) c->own_enabled = enable != 0;
    if (passes_served) *passes_served = c->own_served;
    return 0;
}

int mpmvs_get_kernel_times(mpmvs_ctx* c, float* ms6, int* count6) {
    if (!c) return -1;
    for (int k = 0; k < 6; ++k) {
        if (ms6) ms6[k] = c->k_ms[k];
        if (count6) count6[k] = c->k_cnt[k];
    }
    return 0;
}

// ---------------------------------------------------------------------------
// sky-segmentation network (pm_skyseg.hpp, pm_skyseg_model.hpp).  Errors of these entry points are
// reported through mpmvs_last_error(NULL) (per host thread, like a failed mpmvs_create).
// ---------------------------------------------------------------------------
struct mpmvs_skyseg {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    skyseg::Model m;
    float* d_arena = nullptr;
    float* d_const = nullptr;            // repacked / raw weights and the biases of every live convolution
    std::vector<size_t> w_at, b_at;      // per layer: float offsets into d_const
    std::vector<char> use_mfma;          // per layer
    int launches = 0;
    bool ran = false;
    float net_ms = 0.0f, pre_ms = 0.0f;
};

static int seg_fail(int code, const std::string& text) {
    g_create_err = text;
    return code;
}
#define SEGCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) return seg_fail(-100, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int mpmvs_skyseg_inspect(const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, long long counts[6]) {
    if (!counts) return seg_fail(-2, "skyseg: bad argument");
    skyseg::Model m;
    std::string err;
    const int rc = skyseg::load_model(param_path, bin_path, in_h, in_w, output_blob, m, err);
    if (rc) return seg_fail(rc, err);
    counts[0] = (long long)m.layers.size();
    counts[1] = m.n_blobs_declared;
    counts[2] = m.n_conv;
    counts[3] = m.n_live;
    counts[4] = m.weight_bytes;
    counts[5] = m.macs;
    return 0;
}

static void seg_release(mpmvs_skyseg* n) {
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    if (n->d_arena) (void)pool_free(n->d_arena);
    if (n->d_const) (void)pool_free(n->d_const);
    for (hipEvent_t e : n->ev)
        if (e) (void)hipEventDestroy(e);
    if (n->stream) (void)hipStreamDestroy(n->stream);
    delete n;
}

static int seg_load_device(mpmvs_skyseg* n) {
    skyseg::Model& m = n->m;
    SEGCHK(enter_device(n->device));
    SEGCHK(hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : n->ev) SEGCHK(hipEventCreate(&e));
    std::vector<float> host;
    n->w_at.assign(m.layers.size(), 0);
    n->b_at.assign(m.layers.size(), 0);
    n->use_mfma.assign(m.layers.size(), 0);
    for (int li : m.order) {
        const skyseg::Layer& L = m.layers[li];
        if (L.op != skyseg::OP_CONV) continue;
        const float* w = m.weights.data() + L.w_off;
        n->w_at[li] = host.size();
        if (L.k == 3 && L.cout > 1) {  // operand layout of k_seg_conv3_mfma
            n->use_mfma[li] = 1;
            const int pairs = (L.cin + 1) / 2;
            int mt = (L.cout + 31) / 32;
            if (mt > 1) mt = (mt + 1) / 2 * 2;
            host.resize(host.size() + (size_t)pairs * 9 * mt * 64, 0.0f);
            float* d = host.data() + n->w_at[li];
            for (int cp = 0; cp < pairs; ++cp)
                for (int t = 0; t < 9; ++t)
                    for (int j = 0; j < mt; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int c = 2 * cp + (lane >> 5), co = j * 32 + (lane & 31);
                            if (c < L.cin && co < L.cout) d[(((size_t)cp * 9 + t) * mt + j) * 64 + lane] = w[((size_t)co * L.cin + c) * 9 + t];
                        }
        } else {
            host.insert(host.end(), w, w + (size_t)L.cout * L.cin * L.k * L.k);
        }
        host.resize((host.size() + 63) / 64 * 64, 0.0f);
        n->b_at[li] = host.size();
        host.insert(host.end(), m.biases.begin() + L.b_off, m.biases.begin() + L.b_off + L.cout);
        host.resize((host.size() + 63) / 64 * 64, 0.0f);
    }
    if (host.empty()) host.resize(64, 0.0f);
    SEGCHK(pool_malloc(&n->d_const, host.size() * 4));
    SEGCHK(hipMemcpyAsync(n->d_const, host.data(), host.size() * 4, hipMemcpyHostToDevice, n->stream));
    SEGCHK(hipStreamSynchronize(n->stream));  // `host` goes away
    SEGCHK(pool_malloc(&n->d_arena, std::max<size_t>(m.arena_floats, 64) * 4));
    return 0;
}

int mpmvs_skyseg_load(int device, const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, mpmvs_skyseg** net) {
    if (!net) return seg_fail(-2, "skyseg: bad argument");
    *net = nullptr;
    mpmvs_skyseg* n = new mpmvs_skyseg;
    n->device = device;
    std::string err;
    int rc = skyseg::load_model(param_path, bin_path, in_h, in_w, output_blob, n->m, err);  // all of the checking: no device touched yet
    if (rc) {
        delete n;
        return seg_fail(rc, err);
    }
    rc = seg_load_device(n);
    if (rc) {
        seg_release(n);
        return rc;
    }
    *net = n;
    return 0;
}

void mpmvs_skyseg_destroy(mpmvs_skyseg* n) {
    if (!n) return;
    (void)enter_device(n->device);
    seg_release(n);
}

static float* seg_ptr(const mpmvs_skyseg* n, const skyseg::Seg& s) {
    const skyseg::Buf& b = n->m.bufs[s.buf];
    return n->d_arena + b.off + (size_t)s.coff * b.h * b.w;
}

// enqueues the kernels of the network on the net's stream (the input blob is already in place)
static int seg_enqueue(mpmvs_skyseg* n) {
    const skyseg::Model& m = n->m;
    int launches = 0;
    for (int li : m.order) {
        const skyseg::Layer& L = m.layers[li];
        const skyseg::Blob& in = m.blobs[L.in[0]];
        const skyseg::Blob& ob = m.blobs[L.out[0]];
        float* out = seg_ptr(n, ob.segs[0]);
        const int ohw = ob.h * ob.w;
        switch (L.op) {
            case skyseg::OP_CONV: {
                SegSrcs s{};
                s.n = (int)in.segs.size();
                for (int i = 0; i < s.n; ++i) {
                    s.p[i] = seg_ptr(n, in.segs[i]);
                    s.c[i] = in.segs[i].c;
                }
                const float *w = n->d_const + n->w_at[li], *b = n->d_const + n->b_at[li];
                if (n->use_mfma[li]) {
                    const int mt = (L.cout + 31) / 32, per_block = (kSegConvThreads / 64) * kSegPT * 32;
                    const dim3 grid((ohw + per_block - 1) / per_block, mt > 1 ? (mt + 1) / 2 : 1);
                    const int mt_total = mt > 1 ? (mt + 1) / 2 * 2 : 1;
                    if (mt > 1)
                        hipLaunchKernelGGL(k_seg_conv3_mfma<2>, grid, dim3(kSegConvThreads), 0, n->stream, s, w, b, out, ob.h, ob.w, (L.cin + 1) / 2, mt_total, L.cout, L.dil, L.act);
                    else
                        hipLaunchKernelGGL(k_seg_conv3_mfma<1>, grid, dim3(kSegConvThreads), 0, n->stream, s, w, b, out, ob.h, ob.w, (L.cin + 1) / 2, mt_total, L.cout, L.dil, L.act);
                } else {
                    hipLaunchKernelGGL(k_seg_conv_direct, dim3((ohw + 255) / 256, L.cout), dim3(256), 0, n->stream, s, w, b, out, ob.h, ob.w, L.cin, L.k, L.dil, L.act);
                }
                ++launches;
                break;
            }
            case skyseg::OP_POOL:
            case skyseg::OP_INTERP:
            case skyseg::OP_SIGMOID: {
                int cdone = 0;
                for (const skyseg::Seg& sg : in.segs) {  // a Concat result: one launch per part
                    const float* src = seg_ptr(n, sg);
                    float* dst = out + (size_t)cdone * ohw;
                    const int total = sg.c * ohw;
                    const dim3 grid((total + 255) / 256);
                    if (L.op == skyseg::OP_POOL) hipLaunchKernelGGL(k_seg_pool2, grid, dim3(256), 0, n->stream, src, dst, sg.c, in.h, in.w, ob.h, ob.w);
                    else if (L.op == skyseg::OP_INTERP) hipLaunchKernelGGL(k_seg_interp, grid, dim3(256), 0, n->stream, src, dst, sg.c, in.h, in.w, ob.h, ob.w);
                    else hipLaunchKernelGGL(k_seg_sigmoid, grid, dim3(256), 0, n->stream, src, dst, total);
                    cdone += sg.c;
                    ++launches;
                }
                break;
            }
            case skyseg::OP_ADD: {
                const int total = ob.c * ohw;
                hipLaunchKernelGGL(k_seg_add, dim3((total + 255) / 256), dim3(256), 0, n->stream, seg_ptr(n, in.segs[0]), seg_ptr(n, m.blobs[L.in[1]].segs[0]), out, total);
                ++launches;
                break;
            }
            default:
                return seg_fail(-100, "skyseg: layer " + L.name + " has no kernel");  // a missing kernel is an error
        }
    }
    SEGCHK(hipGetLastError());
    n->launches = launches;
    return 0;
}

static int seg_copy_out(mpmvs_skyseg* n, const skyseg::Blob& b, float* out) {
    size_t done = 0;
    for (const skyseg::Seg& s : b.segs) {
        const size_t fl = (size_t)s.c * b.h * b.w;
        SEGCHK(hipMemcpyAsync(out + done, seg_ptr(n, s), fl * 4, hipMemcpyDeviceToHost, n->stream));
        done += fl;
    }
    SEGCHK(hipStreamSynchronize(n->stream));
    return 0;
}

static int seg_run_tail(mpmvs_skyseg* n, float* out) {
    SEGCHK(hipEventRecord(n->ev[1], n->stream));
    int rc = seg_enqueue(n);
    if (rc) {
        (void)hipStreamSynchronize(n->stream);
        return rc;
    }
    SEGCHK(hipEventRecord(n->ev[2], n->stream));
    rc = seg_copy_out(n, n->m.blobs[n->m.output_blob], out);
    if (rc) return rc;
    (void)hipEventElapsedTime(&n->net_ms, n->ev[1], n->ev[2]);
    n->ran = true;
    return 0;
}

int mpmvs_skyseg_run(mpmvs_skyseg* n, const float* in, float* out) {
    if (!n || !in || !out) return seg_fail(-2, "skyseg: bad argument");
    SEGCHK(enter_device(n->device));
    const skyseg::Blob& ib = n->m.blobs[n->m.input_blob];
    SEGCHK(hipMemcpyAsync(seg_ptr(n, ib.segs[0]), in, (size_t)ib.c * ib.h * ib.w * 4, hipMemcpyHostToDevice, n->stream));
    n->pre_ms = 0.0f;
    return seg_run_tail(n, out);
}

// the preprocessing of mpmvs_skyseg_run_u8, enqueued: bytes -> pyrDown loop -> resize + normalise into the input blob
static int seg_preprocess(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch, Scratch& a, Scratch& b) {
    const skyseg::Blob& ib = n->m.blobs[n->m.input_blob];
    if (!bgr || h <= 0 || w <= 0 || h > 32768 || w > 32768) return seg_fail(-2, "skyseg: bad image size");
    if (ib.c != 3) return seg_fail(-2, "skyseg: the network does not take a 3-channel image");
    if (pitch == 0) pitch = (size_t)w * 3;
    if (pitch < (size_t)w * 3) return seg_fail(-2, "skyseg: pitch smaller than a row");
    SEGCHK(a.alloc((size_t)w * h * 3));
    SEGCHK(hipMemcpy2DAsync(a.p, (size_t)w * 3, bgr, pitch, (size_t)w * 3, (size_t)h, hipMemcpyHostToDevice, n->stream));
    SEGCHK(hipEventRecord(n->ev[0], n->stream));
    unsigned char *cur = a.as<unsigned char>(), *other = nullptr;
    if (h > 768 && w > 768) {
        SEGCHK(b.alloc((size_t)(w / 2) * (h / 2) * 3));
        other = b.as<unsigned char>();
    }
    while (h > 768 && w > 768) {  // src/PatchMatch.cpp:16-18
        const int ow = w / 2, oh = h / 2;
        const int total = ow * oh * 3;
        hipLaunchKernelGGL(k_seg_pyrdown, dim3((total + 255) / 256), dim3(256), 0, n->stream, cur, other, w, h, ow, oh, 3);
        std::swap(cur, other);  // the next level fits the first buffer: it is a quarter of it
        w = ow, h = oh;
    }
    SegNorm nm;
    nm.mean[0] = 0.485f * 255.f, nm.mean[1] = 0.456f * 255.f, nm.mean[2] = 0.406f * 255.f;  // SkyRegionDetect.cpp:628-629
    nm.norm[0] = 1 / 0.229f / 255.f, nm.norm[1] = 1 / 0.224f / 255.f, nm.norm[2] = 1 / 0.225f / 255.f;
    const int total = 3 * ib.h * ib.w;
    hipLaunchKernelGGL(k_seg_resize_norm, dim3((total + 255) / 256), dim3(256), 0, n->stream, cur, w, h, seg_ptr(n, ib.segs[0]), ib.w, ib.h, (float)w / ib.w,
                       (float)h / ib.h, nm);
    SEGCHK(hipGetLastError());
    return 0;
}

int mpmvs_skyseg_run_u8(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out) {
    if (!n || !out) return seg_fail(-2, "skyseg: bad argument");
    SEGCHK(enter_device(n->device));
    Scratch a(n->stream), b(n->stream);
    int rc = seg_preprocess(n, bgr, h, w, pitch_bytes, a, b);
    if (!rc) rc = seg_run_tail(n, out);   // (ends synchronised)
    if (!rc) (void)hipEventElapsedTime(&n->pre_ms, n->ev[0], n->ev[1]);
    return rc;
}

int mpmvs_skyseg_preprocess_u8(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out_chw) {
    if (!n || !out_chw) return seg_fail(-2, "skyseg: bad argument");
    SEGCHK(enter_device(n->device));
    Scratch a(n->stream), b(n->stream);
    int rc = seg_preprocess(n, bgr, h, w, pitch_bytes, a, b);
    if (!rc) rc = seg_copy_out(n, n->m.blobs[n->m.input_blob], out_chw);
    n->ran = false;  // the blobs of the last run are no longer all there
    return rc;
}

int mpmvs_skyseg_set_keep(mpmvs_skyseg* n, int keep) {
    if (!n) return seg_fail(-2, "skyseg: bad argument");
    if ((keep != 0) == n->m.keep) return 0;
    SEGCHK(enter_device(n->device));
    SEGCHK(hipStreamSynchronize(n->stream));
    const size_t before = n->m.arena_floats;
    skyseg::plan(n->m, keep != 0);
    n->ran = false;
    if (std::max<size_t>(n->m.arena_floats, 64) != std::max<size_t>(before, 64)) {
        (void)pool_free(n->d_arena);
        n->d_arena = nullptr;
        if (pool_malloc(&n->d_arena, std::max<size_t>(n->m.arena_floats, 64) * 4) != hipSuccess) {
            (void)hipGetLastError();
            skyseg::plan(n->m, !keep);  // back to the plan that fitted
            SEGCHK(pool_malloc(&n->d_arena, std::max<size_t>(n->m.arena_floats, 64) * 4));
            return seg_fail(-100, "skyseg: no memory for the arena of the keep mode");
        }
    }
    return 0;
}

int mpmvs_skyseg_blob(mpmvs_skyseg* n, const char* name, float* out, int dims[3]) {
    if (!n || !name || !dims) return seg_fail(-2, "skyseg: bad argument");
    const skyseg::Model& m = n->m;
    int id = -1;
    for (int i = 0; i < (int)m.blobs.size(); ++i)
        if (m.blobs[i].name == name) id = i;
    bool live = id >= 0;
    if (live)
        for (const skyseg::Seg& s : m.blobs[id].segs) live = live && m.bufs[s.buf].first >= 0;
    if (!live) return seg_fail(MPMVS_SKYSEG_E_NOBLOB, std::string("skyseg: no live blob named ") + name);
    dims[0] = m.blobs[id].c, dims[1] = m.blobs[id].h, dims[2] = m.blobs[id].w;
    if (!out) return 0;
    if (!m.keep || !n->ran) return seg_fail(MPMVS_SKYSEG_E_NOKEEP, "skyseg: blobs can be fetched after a run in keep mode only");
    SEGCHK(enter_device(n->device));
    return seg_copy_out(n, m.blobs[id], out);
}

int mpmvs_skyseg_dims(const mpmvs_skyseg* n, int dims[7]) {
    if (!n || !dims) return seg_fail(-2, "skyseg: bad argument");
    const skyseg::Blob &i = n->m.blobs[n->m.input_blob], &o = n->m.blobs[n->m.output_blob];
    dims[0] = i.c, dims[1] = i.h, dims[2] = i.w, dims[3] = o.c, dims[4] = o.h, dims[5] = o.w;
    int launches = 0;
    for (int li : n->m.order) {
        const skyseg::Layer& L = n->m.layers[li];
        launches += (L.op == skyseg::OP_POOL || L.op == skyseg::OP_INTERP || L.op == skyseg::OP_SIGMOID) ? (int)n->m.blobs[L.in[0]].segs.size() : 1;
    }
    dims[6] = launches;
    return 0;
}

float mpmvs_skyseg_ms(const mpmvs_skyseg* n, float* pre_ms) {
    if (!n) return 0.0f;
    if (pre_ms) *pre_ms = n->pre_ms;
    return n->net_ms;
}

// ---------------------------------------------------------------------------
// capped nearest neighbour between point clouds (pm_cloud.hpp).  Errors of these entry points are
// reported through mpmvs_last_error(NULL), per host thread.
// ---------------------------------------------------------------------------
// one grid of a cloud: the table and the cell runs for one radius
struct CloudGridBuf {
    float radius = 0.0f;
    unsigned long long* d_keys = nullptr;
    int* d_off = nullptr;
    uint4* d_pts = nullptr;
    long long occupied = 0, fullest = 0;
    unsigned long long last_use = 0;
};
constexpr size_t kCloudMaxGrids = 8;   // per handle; the least recently used one gives its buffers to a new radius

// device ms (HIP events) of an operation's last call on a handle: its own passes, and the grid build it needed (0 if reused)
struct CloudOpMs {
    float ms = 0.0f, build_ms = 0.0f;
};
static float cloud_op_ms(const CloudOpMs& t, float* build_ms) {
    if (build_ms) *build_ms = t.build_ms;
    return t.ms;
}

struct mpmvs_cloud {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // build begin / end, query begin / end; a render: the borders of its three passes
    long long n = 0, n_fin = 0;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};   // finite bounding box
    int slots_log2 = 0;
    float* d_xyz = nullptr;
    int *d_cnt = nullptr, *d_tsum = nullptr, *d_slot_of = nullptr, *d_st = nullptr;   // scratch of a build
    std::vector<CloudGridBuf> grids;   // every grid has the same sizes: they depend on the finite count only
    unsigned long long use_clock = 0;
    long long stats[4] = {0, 0, 0, 0};
    // the last nearest, knn, normals and components call (cloud_enter fills build_ms).  query.build_ms is also where cloud_grid
    // leaves the build time of the grid it was last asked for, whoever asked (0 = cached): mpmvs_cloud_kernel_ms reports an align
    // pass's build through it
    CloudOpMs query, knn, normals, cc;
    float render_pass_ms[3] = {0.0f, 0.0f, 0.0f};   // z-min, index, resolve of the last render call
    int* d_cc = nullptr;                            // n ints of mpmvs_cloud_components (parent, then the sizes): allocated by its first call
    float cc_pass_ms[3] = {0.0f, 0.0f, 0.0f};       // the components call's hook (with init and binning), flatten and size passes
};

static void cloud_free_grid(CloudGridBuf& g) {
    for (void* p : {(void*)g.d_keys, (void*)g.d_off, (void*)g.d_pts})
        if (p) (void)pool_free(p);
    g = CloudGridBuf();
}

static void cloud_release(mpmvs_cloud* c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (CloudGridBuf& g : c->grids) cloud_free_grid(g);
    for (void* p : {(void*)c->d_xyz, (void*)c->d_cnt, (void*)c->d_tsum, (void*)c->d_slot_of, (void*)c->d_st, (void*)c->d_cc})
        if (p) (void)pool_free(p);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static int cloud_create_device(mpmvs_cloud* c, const float* xyz) {
    SEGCHK(enter_device(c->device));
    SEGCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->ev) SEGCHK(hipEventCreate(&e));
    if (c->n_fin == 0) return 0;   // nothing to search: every call answers on the host
    const size_t n = (size_t)c->n, slots = (size_t)1 << c->slots_log2;
    SEGCHK(pool_malloc(&c->d_xyz, n * 12));
    SEGCHK(pool_malloc(&c->d_slot_of, n * 4));
    SEGCHK(pool_malloc(&c->d_cnt, slots * 4));
    SEGCHK(pool_malloc(&c->d_tsum, slots / kScanBlock * 4));
    SEGCHK(pool_malloc(&c->d_st, 8));
    SEGCHK(hipMemcpyAsync(c->d_xyz, xyz, n * 12, hipMemcpyHostToDevice, c->stream));
    SEGCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the host's pass over a cloud, shared by every entry point that builds a grid: the number of points with three finite
// coordinates and their bounding box (mn, mx untouched when there is none)
static long long cloud_bbox(long long n, const float* xyz, float mn[3], float mx[3]) {
    long long n_fin = 0;
    for (long long i = 0; i < n; ++i) {
        const float* p = xyz + 3 * i;
        if (!(cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]))) continue;
        for (int a = 0; a < 3; ++a) {
            mn[a] = n_fin ? std::min(mn[a], p[a]) : p[a];
            mx[a] = n_fin ? std::max(mx[a], p[a]) : p[a];
        }
        ++n_fin;
    }
    return n_fin;
}

// a handle on the host side only: the count, the bounding box and the table size of n points (n <= 2^31 - 1); nullptr, with the
// -3 text under the name `who`, beyond 2^29 finite points
static mpmvs_cloud* cloud_new(int device, long long n, const float* xyz, const char* who) {
    mpmvs_cloud* c = new mpmvs_cloud;
    c->device = device;
    c->n = n;
    c->n_fin = cloud_bbox(n, xyz, c->mn, c->mx);
    c->slots_log2 = cloud_slots_log2(c->n_fin);
    if (c->slots_log2 > kCloudMaxSlotsLog2) {
        delete c;
        (void)seg_fail(-3, std::string(who) + ": more than 2^29 finite points (the table would exceed 2^30 slots)");
        return nullptr;
    }
    return c;
}

int mpmvs_cloud_create(int device, long long n, const float* xyz, mpmvs_cloud** cloud) {
    if (!cloud) return seg_fail(-2, "cloud: bad argument");
    *cloud = nullptr;
    if (n < 0 || (n > 0 && !xyz)) return seg_fail(-2, "cloud: bad argument");
    if (n > INT32_MAX) return seg_fail(-3, "cloud: more than 2^31 - 1 points");
    mpmvs_cloud* c = cloud_new(device, n, xyz, "cloud");
    if (!c) return -3;
    const int rc = cloud_create_device(c, xyz);
    if (rc) {
        cloud_release(c);
        return rc;
    }
    *cloud = c;
    return 0;
}

void mpmvs_cloud_destroy(mpmvs_cloud* c) {
    if (!c) return;
    (void)enter_device(c->device);
    cloud_release(c);
}

// slot counts -> offsets (off[n] = the total): the library's scan plus the add pass
static void cloud_scan(hipStream_t st, const int* cnt, int n, int* off, int* tsum) {
    const int ntiles = (n + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(kScanBlock), 0, st, cnt, n, off, tsum);
    hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(kScanBlock), 0, st, tsum, ntiles, 0, off + n);
    hipLaunchKernelGGL(k_vs_scan_add, dim3(ntiles), dim3(kScanBlock), 0, st, off, n, tsum);
}

// builds the grid of `radius` into g, whose buffers exist
static int cloud_build(mpmvs_cloud* c, CloudGridBuf& g, float radius) {
    const hipStream_t st = c->stream;
    const size_t slots = (size_t)1 << c->slots_log2;
    const int n = (int)c->n;
    const double edge = cloud_edge(radius);
    SEGCHK(hipMemsetAsync(g.d_keys, 0xff, slots * 8, st));
    SEGCHK(hipMemsetAsync(c->d_cnt, 0, slots * 4, st));
    SEGCHK(hipMemsetAsync(c->d_st, 0, 8, st));
    SEGCHK(hipEventRecord(c->ev[0], st));
    const dim3 gp((n + 255) / 256), gs((unsigned)(slots / 256));
    hipLaunchKernelGGL(k_cloud_insert, gp, dim3(256), 0, st, c->d_xyz, n, (double)c->mn[0], (double)c->mn[1], (double)c->mn[2], edge, (unsigned)(slots - 1),
                       g.d_keys, c->d_cnt, c->d_slot_of);
    hipLaunchKernelGGL(k_cloud_stats, gs, dim3(256), 0, st, c->d_cnt, (unsigned)slots, c->d_st);
    cloud_scan(st, c->d_cnt, (int)slots, g.d_off, c->d_tsum);
    hipLaunchKernelGGL(k_cloud_scatter, gp, dim3(256), 0, st, c->d_xyz, n, c->d_slot_of, g.d_off, c->d_cnt, g.d_pts);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[1], st));
    int h_st[2] = {0, 0};
    SEGCHK(hipMemcpyAsync(h_st, c->d_st, 8, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    SEGCHK(hipEventElapsedTime(&c->query.build_ms, c->ev[0], c->ev[1]));
    g.occupied = h_st[0], g.fullest = h_st[1];
    g.radius = radius;
    return 0;
}

// the grid of `radius`: a cached one (build_ms = 0), or a new one in fresh buffers or in those of the least recently used grid
static int cloud_grid(mpmvs_cloud* c, float radius, CloudGridBuf** out) {
    CloudGridBuf* g = nullptr;
    for (CloudGridBuf& k : c->grids)
        if (std::memcmp(&k.radius, &radius, 4) == 0) g = &k;
    if (g) {
        c->query.build_ms = 0.0f;
    } else {
        if (c->grids.size() < kCloudMaxGrids) {
            const size_t slots = (size_t)1 << c->slots_log2;
            CloudGridBuf fresh;
            if (pool_malloc(&fresh.d_keys, slots * 8) != hipSuccess || pool_malloc(&fresh.d_off, (slots + 1) * 4) != hipSuccess ||
                pool_malloc(&fresh.d_pts, (size_t)c->n_fin * 16) != hipSuccess) {
                (void)hipGetLastError();
                cloud_free_grid(fresh);
                if (c->grids.empty()) return seg_fail(-100, "cloud: no device memory for the grid");
            } else {
                c->grids.push_back(fresh);
                g = &c->grids.back();
            }
        }
        if (!g) {
            g = &c->grids[0];
            for (CloudGridBuf& k : c->grids)
                if (k.last_use < g->last_use) g = &k;
        }
        const int rc = cloud_build(c, *g, radius);
        if (rc) {   // what the buffers hold is not a grid of any radius
            (void)hipStreamSynchronize(c->stream);
            cloud_free_grid(*g);
            c->grids.erase(c->grids.begin() + (g - c->grids.data()));
            return rc;
        }
    }
    g->last_use = ++c->use_clock;
    c->stats[0] = c->n_fin, c->stats[1] = g->occupied, c->stats[2] = g->fullest, c->stats[3] = 1ll << c->slots_log2;
    *out = g;
    return 0;
}

// MPMVS_CLOUD_BIN=0: the queries (and the sources of an align pass) are served in caller order; read once per process
static bool cloud_bin_queries() {
    static const bool bin = [] {
        const char* e = std::getenv("MPMVS_CLOUD_BIN");
        return !(e && e[0] == '0');
    }();
    return bin;
}

// the kernels' view of a built grid
static CloudGrid cloud_grid_args(const mpmvs_cloud* c, const CloudGridBuf& grid, float radius) {
    CloudGrid g;
    for (int a = 0; a < 3; ++a) g.mn[a] = (double)c->mn[a];
    g.edge = cloud_edge(radius);
    g.r2 = radius * radius;
    g.mask = (unsigned)(((size_t)1 << c->slots_log2) - 1);
    g.keys = grid.d_keys, g.off = grid.d_off, g.pts = grid.d_pts;
    return g;
}

// the binning of nq queries: a power of two of bins, at least 2^8 and at least nq
static int cloud_bins_log2(long long nq) {
    int lg = 8;
    while (lg < kCloudMaxSlotsLog2 && (1ll << lg) < nq) ++lg;
    return lg;
}

// the binning buffers of up to `cap` queries, on a stream that outlives them: those of one call, or of an aligner for all its passes
struct CloudBins {
    Scratch qbin, order, qcnt, qoff, qtsum;
    explicit CloudBins(hipStream_t st) : qbin(st), order(st), qcnt(st), qoff(st), qtsum(st) {}
    hipError_t alloc(size_t cap) {
        const size_t bins = (size_t)1 << cloud_bins_log2((long long)cap);
        hipError_t e;
        if ((e = qbin.alloc(cap * 4)) != hipSuccess || (e = order.alloc(cap * 4)) != hipSuccess || (e = qcnt.alloc(bins * 4)) != hipSuccess ||
            (e = qoff.alloc((bins + 1) * 4)) != hipSuccess || (e = qtsum.alloc(bins / kScanBlock * 4)) != hipSuccess)
            return e;
        return hipSuccess;
    }
};

extern "C++" {
// The one binning path: the serving order of nq <= cap queries into b.order.  The counts are cleared, `begin` (may be null) is
// recorded -- the callers whose timed interval opens after the memset pass their begin event -- and then count / scan / order run.
// count(grid, bin_mask, qcnt, qbin) launches the counting kernel, the only part that differs: k_cloud_qbin on raw queries,
// k_align_qbin on transformed sources.
template <typename Count>
static int cloud_bin(hipStream_t st, CloudBins& b, int nq, hipEvent_t begin, Count&& count) {
    const size_t bins = (size_t)1 << cloud_bins_log2(nq);   // <= what alloc sized
    const dim3 gq(((unsigned)nq + 255u) / 256u);            // unsigned: nq may be 2^31 - 1
    SEGCHK(hipMemsetAsync(b.qcnt.p, 0, bins * 4, st));
    if (begin) SEGCHK(hipEventRecord(begin, st));
    count(gq, (unsigned)(bins - 1), b.qcnt.as<int>(), b.qbin.as<int>());
    cloud_scan(st, b.qcnt.as<int>(), (int)bins, b.qoff.as<int>(), b.qtsum.as<int>());
    hipLaunchKernelGGL(k_cloud_qorder, gq, dim3(256), 0, st, nq, b.qbin.as<int>(), b.qoff.as<int>(), b.qcnt.as<int>(), b.order.as<int>());
    return 0;
}
// the counting launch of raw queries
static auto cloud_count_queries(hipStream_t st, const float* d_q, int nq, const CloudGrid& g) {
    return [=](dim3 gq, unsigned bin_mask, int* qcnt, int* qbin) { hipLaunchKernelGGL(k_cloud_qbin, gq, dim3(256), 0, st, d_q, nq, g, bin_mask, qcnt, qbin); };
}

// The one dispatch over the list sizes of the kNN family (pm_knn.hpp: knn_list_size): launch(std::integral_constant<int, K>) with
// the K of 4, 8, 16 or 32 that serves k
template <typename F>
static void knn_dispatch(int k, F&& launch) {
    switch (knn_list_size(k)) {
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        case 16: launch(std::integral_constant<int, 16>{}); break;
        default: launch(std::integral_constant<int, 32>{}); break;
    }
}
}  // extern "C++"

// the cell-span limit of a grid of `radius` over the handle's finite bounding box (-3), found on the host; `who` opens the text
static int cloud_span_check(const mpmvs_cloud* c, float radius, const char* who = "cloud: the targets") {
    const double edge = cloud_edge(radius);
    for (int a = 0; a < 3 && c->n_fin > 0; ++a) {
        const double cells = std::floor(((double)c->mx[a] - (double)c->mn[a]) / edge) + 1.0;
        if (cells > (double)kCloudAxisCells) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "%s span %.6g cells of edge %.6g along %c, more than 2^21 (extent / radius = %.6g)", who, cells, edge,
                          "xyz"[a], ((double)c->mx[a] - (double)c->mn[a]) / (double)radius);
            return seg_fail(-3, msg);
        }
    }
    return 0;
}

// what every entry point with a radius asks of it; each keeps the text of its own refusal
static bool cloud_radius_ok(float radius) { return std::isfinite(radius) && radius > 0.0f; }

// The device half of the prologue of every operation on a handle with finite points: the device, the grid of `radius` (cached or
// built now) and the kernels' view of it in g; the build time goes to t->build_ms and t->ms is cleared (t may be null: an align
// pass and the outlier filter read query.build_ms themselves).
static int cloud_open(mpmvs_cloud* c, float radius, CloudOpMs* t, CloudGrid& g) {
    SEGCHK(enter_device(c->device));
    CloudGridBuf* grid = nullptr;
    const int rc = cloud_grid(c, radius, &grid);
    if (rc) return rc;
    if (t) *t = CloudOpMs{0.0f, c->query.build_ms};
    g = cloud_grid_args(c, *grid, radius);
    return 0;
}
// The whole prologue, after the entry point's own argument checks: the span limit first (-3 before the device is touched).
static int cloud_enter(mpmvs_cloud* c, float radius, CloudOpMs* t, CloudGrid& g) {
    const int span = cloud_span_check(c, radius);
    return span ? span : cloud_open(c, radius, t, g);
}
// a handle without a finite point answers on the host: no grid, no time
static void cloud_answered_on_host(mpmvs_cloud* c, CloudOpMs& t) {
    c->stats[0] = c->stats[1] = c->stats[2] = c->stats[3] = 0;
    t = CloudOpMs();
}

int mpmvs_cloud_nearest(mpmvs_cloud* c, float radius, long long n_q, const float* q_xyz, float* out_d2, int32_t* out_idx) {
    if (!c || !out_d2 || n_q < 0 || (n_q > 0 && !q_xyz)) return seg_fail(-2, "cloud: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "cloud: the radius must be finite and positive");
    if (n_q > INT32_MAX) return seg_fail(-3, "cloud: more than 2^31 - 1 queries");
    if (n_q == 0) return 0;
    if (c->n_fin == 0) {   // no candidate anywhere
        for (long long i = 0; i < n_q; ++i) {
            out_d2[i] = INFINITY;
            if (out_idx) out_idx[i] = -1;
        }
        cloud_answered_on_host(c, c->query);
        return 0;
    }
    CloudGrid g;
    const int rc = cloud_enter(c, radius, &c->query, g);
    if (rc) return rc;
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries();
    const int nq = (int)n_q;
    const size_t q = (size_t)n_q;
    Scratch d_q(st), d_d2(st), d_idx(st);
    CloudBins bins(st);
    SEGCHK(d_q.alloc(q * 12));
    SEGCHK(d_d2.alloc(q * 4));
    if (out_idx) SEGCHK(d_idx.alloc(q * 4));
    if (bin) SEGCHK(bins.alloc(q));
    SEGCHK(hipMemcpyAsync(d_q.p, q_xyz, q * 12, hipMemcpyHostToDevice, st));
    if (bin) {
        const int brc = cloud_bin(st, bins, nq, c->ev[2], cloud_count_queries(st, d_q.as<float>(), nq, g));
        if (brc) return brc;
    } else {
        SEGCHK(hipEventRecord(c->ev[2], st));
    }
    hipLaunchKernelGGL(k_cloud_query, dim3(((unsigned)nq + 255u) / 256u), dim3(256), 0, st, d_q.as<float>(), nq, bin ? bins.order.as<int>() : (const int*)nullptr, g,
                       d_d2.as<float>(), out_idx ? d_idx.as<int32_t>() : (int32_t*)nullptr);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[3], st));
    SEGCHK(hipMemcpyAsync(out_d2, d_d2.p, q * 4, hipMemcpyDeviceToHost, st));
    if (out_idx) SEGCHK(hipMemcpyAsync(out_idx, d_idx.p, q * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    SEGCHK(hipEventElapsedTime(&c->query.ms, c->ev[2], c->ev[3]));
    return 0;
}

int mpmvs_cloud_stats(const mpmvs_cloud* c, long long stats[4]) {
    if (!c || !stats) return seg_fail(-2, "cloud: bad argument");
    std::memcpy(stats, c->stats, sizeof c->stats);
    return 0;
}

float mpmvs_cloud_kernel_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->query, build_ms) : 0.0f; }

// ---------------------------------------------------------------------------
// voxel-grid downsampling of a cloud (pm_voxel.hpp).  A stateless call: host buffers in and out, a stream
// of its own.  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
static thread_local float g_voxel_ms = 0.0f;   // per calling thread, as g_undistort_kernel_ms
static thread_local float g_voxel_pass_ms[6] = {0, 0, 0, 0, 0, 0};
float mpmvs_cloud_voxel_ms(void) { return g_voxel_ms; }
void mpmvs_cloud_voxel_pass_ms(float ms[6]) {
    if (ms) std::memcpy(ms, g_voxel_pass_ms, sizeof g_voxel_pass_ms);
}

namespace {
// the borders of the six passes; destroyed after the DeviceCall declared below them has synchronised its stream
struct VoxelEvents {
    hipEvent_t e[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~VoxelEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};
// the host buffers of the result: released unless the call succeeds
struct VoxelOut {
    void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool keep = false;
    ~VoxelOut() {
        if (!keep)
            for (void* x : p) std::free(x);
    }
};
}  // namespace

long long mpmvs_cloud_voxel_downsample(int device, long long n, const float* xyz, const float* normals, const unsigned char* rgb, float voxel, float** out_xyz,
                                       float** out_normals, unsigned char** out_rgb, int32_t** out_count, int32_t** out_first, int32_t* out_voxel_of) {
    if (n < 0 || (n > 0 && !xyz) || !out_xyz || !out_count || !out_first || (normals && !out_normals) || (rgb && !out_rgb))
        return seg_fail(-2, "voxel: bad argument");
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return seg_fail(-2, "voxel: the voxel size must be finite and positive");
    *out_xyz = nullptr, *out_count = nullptr, *out_first = nullptr;
    if (out_normals) *out_normals = nullptr;
    if (out_rgb) *out_rgb = nullptr;
    if (n > INT32_MAX) return seg_fail(-3, "voxel: more than 2^31 - 1 points");
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    const long long n_fin = cloud_bbox(n, xyz, mn, mx);
    const int slots_log2 = cloud_slots_log2(n_fin);
    if (slots_log2 > kCloudMaxSlotsLog2) return seg_fail(-3, "voxel: more than 2^29 finite points (the table would exceed 2^30 slots)");
    VoxelGrid g;
    voxel_origin(mn, voxel, g);
    if (n_fin > 0)
        for (int a = 0; a < 3; ++a) {
            const double top = std::floor(((double)mx[a] - g.o[a]) / g.e);   // the cell of the highest point: the cells are monotonic in x
            if (!(top < (double)kCloudAxisCells)) {
                char msg[200];
                std::snprintf(msg, sizeof msg, "voxel: the points span %.6g cells of edge %.6g along %c, more than 2^21 (extent / voxel = %.6g)", top + 1.0, g.e,
                              "xyz"[a], ((double)mx[a] - (double)mn[a]) / g.e);
                return seg_fail(-3, msg);
            }
        }
    if (n_fin == 0) {   // nothing occupies a voxel: answered on the host
        if (out_voxel_of)
            for (long long i = 0; i < n; ++i) out_voxel_of[i] = -1;
        g_voxel_ms = 0.0f;
        std::memset(g_voxel_pass_ms, 0, sizeof g_voxel_pass_ms);
        return 0;
    }

    VoxelEvents ev;
    VoxelOut out;
    DeviceCall call(device);
    if (!call.ok()) return seg_fail(-100, "voxel: the device could not be selected or gave no stream");
    const hipStream_t st = call.stream();
    for (hipEvent_t& e : ev.e) SEGCHK(hipEventCreate(&e));
    const size_t np = (size_t)n, slots = (size_t)1 << slots_log2;
    const int ni = (int)n, ntiles = (ni + kScanBlock - 1) / kScanBlock;
    float* d_xyz = call.alloc<float>(np * 12);
    int* d_slot_of = call.alloc<int>(np * 4);
    int* d_flag = call.alloc<int>(np * 4);
    int* d_num = call.alloc<int>(np * 4);
    int* d_tsum = call.alloc<int>((size_t)ntiles * 4);
    int* d_m = call.alloc<int>(4);
    unsigned long long* d_keys = call.alloc<unsigned long long>(slots * 8);
    int* d_cnt = call.alloc<int>(slots * 4);
    unsigned* d_first = call.alloc<unsigned>(slots * 4);
    int* d_vox_of_slot = call.alloc<int>(slots * 4);
    float* d_nrm = normals ? call.alloc<float>(np * 12) : nullptr;
    unsigned char* d_rgb = rgb ? call.alloc<unsigned char>(np * 3) : nullptr;
    int32_t* d_voxel_of = out_voxel_of ? call.alloc<int32_t>(np * 4) : nullptr;
    if (!d_xyz || !d_slot_of || !d_flag || !d_num || !d_tsum || !d_m || !d_keys || !d_cnt || !d_first || !d_vox_of_slot || (normals && !d_nrm) ||
        (rgb && !d_rgb) || (out_voxel_of && !d_voxel_of))
        return seg_fail(-100, "voxel: no device memory");
    SEGCHK(hipMemcpyAsync(d_xyz, xyz, np * 12, hipMemcpyHostToDevice, st));
    if (normals) SEGCHK(hipMemcpyAsync(d_nrm, normals, np * 12, hipMemcpyHostToDevice, st));
    if (rgb) SEGCHK(hipMemcpyAsync(d_rgb, rgb, np * 3, hipMemcpyHostToDevice, st));
    SEGCHK(hipMemsetAsync(d_keys, 0xff, slots * 8, st));
    SEGCHK(hipMemsetAsync(d_cnt, 0, slots * 4, st));
    SEGCHK(hipMemsetAsync(d_first, 0xff, slots * 4, st));
    const dim3 gp((unsigned)ntiles), blk(256);
    SEGCHK(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(k_cloud_insert, gp, blk, 0, st, d_xyz, ni, g.o[0], g.o[1], g.o[2], g.e, (unsigned)(slots - 1), d_keys, d_cnt, d_slot_of);
    SEGCHK(hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(k_voxel_first, gp, blk, 0, st, ni, d_slot_of, d_first);
    SEGCHK(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(k_voxel_flag, gp, blk, 0, st, ni, d_slot_of, d_first, d_flag);
    hipLaunchKernelGGL(k_scan_tiles, gp, dim3(kScanBlock), 0, st, d_flag, ni, d_num, d_tsum);
    hipLaunchKernelGGL(k_scan_totals<Sum>, dim3(1), dim3(kScanBlock), 0, st, d_tsum, ntiles, 0, d_m);
    hipLaunchKernelGGL(k_vs_scan_add, gp, dim3(kScanBlock), 0, st, d_num, ni, d_tsum);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(ev.e[3], st));
    int m = 0;
    SEGCHK(hipMemcpyAsync(&m, d_m, 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    if (m <= 0 || (long long)m > n_fin) return seg_fail(-100, "voxel: the device counted " + std::to_string(m) + " voxels for " + std::to_string(n_fin) + " finite points");

    const size_t mv = (size_t)m;
    int32_t* d_out_first = call.alloc<int32_t>(mv * 4);
    int32_t* d_out_count = call.alloc<int32_t>(mv * 4);
    float* d_out_xyz = call.alloc<float>(mv * 12);
    float* d_out_nrm = normals ? call.alloc<float>(mv * 12) : nullptr;
    unsigned char* d_out_rgb = rgb ? call.alloc<unsigned char>(mv * 3) : nullptr;
    // S, then N, then C: 3 x 64 bits per voxel each
    const size_t acc_parts = 1 + (normals ? 1 : 0) + (rgb ? 1 : 0);
    unsigned long long* d_acc = call.alloc<unsigned long long>(acc_parts * mv * 24);
    if (!d_out_first || !d_out_count || !d_out_xyz || (normals && !d_out_nrm) || (rgb && !d_out_rgb) || !d_acc) return seg_fail(-100, "voxel: no device memory");
    unsigned long long* d_S = d_acc;
    unsigned long long* d_N = normals ? d_acc + 3 * mv : nullptr;
    unsigned long long* d_C = rgb ? d_acc + 3 * mv * (normals ? 2 : 1) : nullptr;
    out.p[0] = std::malloc(mv * 12), out.p[1] = std::malloc(mv * 4), out.p[2] = std::malloc(mv * 4);
    if (normals) out.p[3] = std::malloc(mv * 12);
    if (rgb) out.p[4] = std::malloc(mv * 3);
    if (!out.p[0] || !out.p[1] || !out.p[2] || (normals && !out.p[3]) || (rgb && !out.p[4])) return seg_fail(-100, "voxel: no host memory for the result");
    SEGCHK(hipMemsetAsync(d_acc, 0, acc_parts * mv * 24, st));
    SEGCHK(hipEventRecord(ev.e[4], st));   // pass 4 begins here: the wait for m is not device time
    hipLaunchKernelGGL(k_voxel_number, gp, blk, 0, st, ni, d_flag, d_num, d_slot_of, d_cnt, d_vox_of_slot, d_out_first, d_out_count);
    SEGCHK(hipEventRecord(ev.e[5], st));
    hipLaunchKernelGGL(k_voxel_accumulate, gp, blk, 0, st, ni, d_xyz, d_nrm, d_rgb, g, d_slot_of, d_vox_of_slot, d_S, d_N, d_C, d_voxel_of);
    SEGCHK(hipEventRecord(ev.e[6], st));
    hipLaunchKernelGGL(k_voxel_finish, dim3((unsigned)((mv + 255) / 256)), blk, 0, st, m, d_xyz, d_out_first, d_out_count, g, d_S, d_N, d_C, d_out_xyz, d_out_nrm,
                       d_out_rgb);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(ev.e[7], st));
    SEGCHK(hipMemcpyAsync(out.p[0], d_out_xyz, mv * 12, hipMemcpyDeviceToHost, st));
    SEGCHK(hipMemcpyAsync(out.p[1], d_out_count, mv * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipMemcpyAsync(out.p[2], d_out_first, mv * 4, hipMemcpyDeviceToHost, st));
    if (normals) SEGCHK(hipMemcpyAsync(out.p[3], d_out_nrm, mv * 12, hipMemcpyDeviceToHost, st));
    if (rgb) SEGCHK(hipMemcpyAsync(out.p[4], d_out_rgb, mv * 3, hipMemcpyDeviceToHost, st));
    if (out_voxel_of) SEGCHK(hipMemcpyAsync(out_voxel_of, d_voxel_of, np * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    float ms[6] = {0, 0, 0, 0, 0, 0};
    SEGCHK(hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
    SEGCHK(hipEventElapsedTime(&ms[1], ev.e[1], ev.e[2]));
    SEGCHK(hipEventElapsedTime(&ms[2], ev.e[2], ev.e[3]));
    SEGCHK(hipEventElapsedTime(&ms[3], ev.e[4], ev.e[5]));
    SEGCHK(hipEventElapsedTime(&ms[4], ev.e[5], ev.e[6]));
    SEGCHK(hipEventElapsedTime(&ms[5], ev.e[6], ev.e[7]));
    std::memcpy(g_voxel_pass_ms, ms, sizeof ms);
    g_voxel_ms = ((ms[0] + ms[1]) + (ms[2] + ms[3])) + (ms[4] + ms[5]);
    *out_xyz = (float*)out.p[0], *out_count = (int32_t*)out.p[1], *out_first = (int32_t*)out.p[2];
    if (normals) *out_normals = (float*)out.p[3];
    if (rgb) *out_rgb = (unsigned char*)out.p[4];
    out.keep = true;
    return m;
}

// ---------------------------------------------------------------------------
// k nearest neighbours within a cloud handle, and the statistical / radius outlier filter on top of them (pm_knn.hpp; DESIGN.md
// section 17).  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
constexpr size_t kKnnChunkEntries = (size_t)1 << 23;   // list entries per launch of the list variant: 2^23 / k queries (2^18 at k = 32), whatever n_q

int mpmvs_cloud_knn(mpmvs_cloud* c, float radius, int k, long long n_q, const float* q_xyz, float* out_d2, int32_t* out_idx, int32_t* out_within) {
    if (!c || !out_d2 || n_q < 0) return seg_fail(-2, "cloud knn: bad argument");
    if (k < 1 || k > MPMVS_KNN_MAX_K) return seg_fail(-2, "cloud knn: k must lie in [1, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!q_xyz && n_q != c->n) return seg_fail(-2, "cloud knn: without query points n_q must be the cloud's own count");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "cloud knn: the radius must be finite and positive");
    if (n_q > INT32_MAX) return seg_fail(-3, "cloud knn: more than 2^31 - 1 queries");
    if (n_q == 0) return 0;
    const size_t nq = (size_t)n_q, kk = (size_t)k;
    if (c->n_fin == 0) {   // no candidate anywhere
        for (size_t e = 0; e < nq * kk; ++e) {
            out_d2[e] = INFINITY;
            if (out_idx) out_idx[e] = -1;
        }
        if (out_within) std::memset(out_within, 0, nq * 4);
        cloud_answered_on_host(c, c->knn);
        return 0;
    }
    CloudGrid g;
    const int rc = cloud_enter(c, radius, &c->knn, g);
    if (rc) return rc;
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries();
    const size_t chunk = std::min(nq, kKnnChunkEntries / kk);
    Scratch d_q(st), d_d2(st), d_idx(st), d_within(st);
    CloudBins bins(st);
    if (q_xyz) {
        SEGCHK(d_q.alloc(nq * 12));
        SEGCHK(hipMemcpyAsync(d_q.p, q_xyz, nq * 12, hipMemcpyHostToDevice, st));
    }
    SEGCHK(d_d2.alloc(chunk * kk * 4));
    if (out_idx) SEGCHK(d_idx.alloc(chunk * kk * 4));
    if (out_within) SEGCHK(d_within.alloc(chunk * 4));
    if (bin) SEGCHK(bins.alloc(chunk));
    const float* d_all = q_xyz ? d_q.as<float>() : c->d_xyz;
    for (size_t i0 = 0; i0 < nq; i0 += chunk) {
        const int cn = (int)std::min(chunk, nq - i0);
        const float* d_qc = d_all + 3 * i0;
        SEGCHK(hipEventRecord(c->ev[2], st));
        if (bin) {
            const int brc = cloud_bin(st, bins, cn, nullptr, cloud_count_queries(st, d_qc, cn, g));
            if (brc) return brc;
        }
        const int* order = bin ? bins.order.as<int>() : (const int*)nullptr;
        const long long self_base = q_xyz ? -1ll : (long long)i0;
        int32_t* di = out_idx ? d_idx.as<int32_t>() : (int32_t*)nullptr;
        int32_t* dw = out_within ? d_within.as<int32_t>() : (int32_t*)nullptr;
        knn_dispatch(k, [&](auto K) {
            hipLaunchKernelGGL(k_knn_list<K>, dim3((cn + 255) / 256), dim3(256), 0, st, d_qc, cn, order, g, self_base, k, d_d2.as<float>(), di, dw);
        });
        SEGCHK(hipGetLastError());
        SEGCHK(hipEventRecord(c->ev[3], st));
        SEGCHK(hipMemcpyAsync(out_d2 + i0 * kk, d_d2.p, (size_t)cn * kk * 4, hipMemcpyDeviceToHost, st));
        if (out_idx) SEGCHK(hipMemcpyAsync(out_idx + i0 * kk, d_idx.p, (size_t)cn * kk * 4, hipMemcpyDeviceToHost, st));
        if (out_within) SEGCHK(hipMemcpyAsync(out_within + i0, d_within.p, (size_t)cn * 4, hipMemcpyDeviceToHost, st));
        SEGCHK(hipStreamSynchronize(st));
        float ms = 0.0f;
        SEGCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        c->knn.ms += ms;
    }
    return 0;
}

float mpmvs_cloud_knn_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->knn, build_ms) : 0.0f; }

static thread_local float g_outliers_ms = 0.0f;   // per calling thread, as g_voxel_ms
float mpmvs_cloud_outliers_ms(void) { return g_outliers_ms; }

// the device half of mpmvs_cloud_outliers: a handle of the call's own (its stream, its grid), the reducing kernel over every point
static int outliers_device(mpmvs_cloud* c, const float* xyz, float radius, int k, float* mean, int32_t* within, float* ms) {
    int rc = cloud_create_device(c, xyz);
    if (rc) return rc;
    CloudGrid g;
    if ((rc = cloud_open(c, radius, nullptr, g)) != 0) return rc;   // the caller has checked the span
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries();
    const size_t n = (size_t)c->n;
    const int ni = (int)c->n;
    Scratch d_mean(st), d_within(st);
    CloudBins bins(st);
    SEGCHK(d_mean.alloc(n * 4));
    SEGCHK(d_within.alloc(n * 4));
    if (bin) SEGCHK(bins.alloc(n));
    SEGCHK(hipEventRecord(c->ev[2], st));
    if (bin && (rc = cloud_bin(st, bins, ni, nullptr, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    const int* order = bin ? bins.order.as<int>() : (const int*)nullptr;
    knn_dispatch(k, [&](auto K) {
        hipLaunchKernelGGL(k_knn_reduce<K>, dim3((ni + 255) / 256), dim3(256), 0, st, c->d_xyz, ni, order, g, 0ll, k, d_mean.as<float>(), d_within.as<int32_t>());
    });
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[3], st));
    SEGCHK(hipMemcpyAsync(mean, d_mean.p, n * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipMemcpyAsync(within, d_within.p, n * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    float q_ms = 0.0f;
    SEGCHK(hipEventElapsedTime(&q_ms, c->ev[2], c->ev[3]));
    *ms = c->query.build_ms + q_ms;
    return 0;
}

long long mpmvs_cloud_outliers(int device, long long n, const float* xyz, float radius, int k, double std_ratio, int min_within, unsigned char* out_keep,
                               float* out_mean, int32_t* out_within, long long counts[3], double stats[3]) {
    if (n < 0 || (n > 0 && (!xyz || !out_keep))) return seg_fail(-2, "outliers: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "outliers: the radius must be finite and positive");
    if (k < 1 || k > MPMVS_KNN_MAX_K) return seg_fail(-2, "outliers: k must lie in [1, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!(std_ratio >= 0.0)) return seg_fail(-2, "outliers: std_ratio must not be negative or NaN");
    if (min_within < 0) return seg_fail(-2, "outliers: min_within must not be negative");
    if (n > INT32_MAX) return seg_fail(-3, "outliers: more than 2^31 - 1 points");
    mpmvs_cloud* c = cloud_new(device, n, xyz, "outliers");   // the limits of mpmvs_cloud_create and of a grid, in their one place
    if (!c) return -3;
    const long long n_fin = c->n_fin;
    if (cloud_span_check(c, radius, "outliers: the points")) {
        delete c;
        return -3;
    }
    if (counts) counts[0] = n_fin, counts[1] = counts[2] = 0;
    if (stats) stats[0] = stats[1] = stats[2] = 0.0;
    if (n_fin == 0) {   // nothing to keep: answered on the host
        delete c;
        for (long long i = 0; i < n; ++i) {
            out_keep[i] = 0;
            if (out_mean) out_mean[i] = INFINITY;
            if (out_within) out_within[i] = 0;
        }
        g_outliers_ms = 0.0f;
        return 0;
    }
    const size_t np = (size_t)n;
    std::vector<float> mean_own;
    std::vector<int32_t> within_own;
    if (!out_mean) mean_own.resize(np);
    if (!out_within) within_own.resize(np);
    float* mean = out_mean ? out_mean : mean_own.data();
    int32_t* within = out_within ? out_within : within_own.data();
    float ms = 0.0f;
    const int rc = outliers_device(c, xyz, radius, k, mean, within, &ms);
    (void)enter_device(c->device);
    cloud_release(c);
    if (rc) return rc;

    // the statistics: integer sums, so their order never shows
    const double rd = (double)radius;
    long long cfin = 0, S1 = 0, S2 = 0;
    for (size_t i = 0; i < np; ++i) {
        if (!cloud_finite(mean[i])) continue;
        const double a = (double)mean[i] / rd;
        S1 += llrint(a * 0x1p30);
        S2 += llrint((a * a) * 0x1p30);
        ++cfin;
    }
    double mu = 0.0, sigma = 0.0, T = 0.0;
    if (cfin > 0) {
        const double den = (double)cfin * 0x1p30;
        mu = (double)S1 / den;
        const double var = (double)S2 / den - mu * mu;
        sigma = std::sqrt(var > 0.0 ? var : 0.0);
        T = std::isinf(std_ratio) ? (double)INFINITY : (mu + std_ratio * sigma) * rd;
    }
    long long kept = 0;
    for (size_t i = 0; i < np; ++i) {
        const bool keep = cloud_finite(mean[i]) && (double)mean[i] <= T && within[i] >= min_within;
        out_keep[i] = keep ? 1 : 0;
        kept += keep ? 1 : 0;
    }
    if (counts) counts[1] = cfin, counts[2] = kept;
    if (stats) stats[0] = mu * rd, stats[1] = sigma * rd, stats[2] = T;
    g_outliers_ms = ms;
    return kept;
}

// ---------------------------------------------------------------------------
// a normal per point from its k nearest neighbours (pm_normals.hpp): the reducing kernel k_knn_normal over
// every point of the handle, in one launch, as outliers_device launches k_knn_reduce.  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
int mpmvs_cloud_normals(mpmvs_cloud* c, float radius, int k, int orient, const double view[3], const float* ref_normals, float* out_normals, float* out_curvature,
                        int32_t* out_within) {
    if (!c || !out_normals) return seg_fail(-2, "cloud normals: bad argument");
    if (k < 2 || k > MPMVS_KNN_MAX_K) return seg_fail(-2, "cloud normals: k must lie in [2, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "cloud normals: the radius must be finite and positive");
    if (orient < 0 || orient > 2) return seg_fail(-2, "cloud normals: orient must be 0 (canonical), 1 (viewpoint) or 2 (reference normals)");
    if (orient == 1 && !(view && std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2])))
        return seg_fail(-2, "cloud normals: orient 1 needs a finite viewpoint");
    if (orient == 2 && !ref_normals) return seg_fail(-2, "cloud normals: orient 2 needs reference normals");
    if (c->n == 0) return 0;
    const size_t n = (size_t)c->n;
    if (c->n_fin == 0) {   // no candidate anywhere: every normal is undefined
        std::memset(out_normals, 0, n * 12);
        for (size_t i = 0; i < n && out_curvature; ++i) out_curvature[i] = INFINITY;
        if (out_within) std::memset(out_within, 0, n * 4);
        cloud_answered_on_host(c, c->normals);
        return 0;
    }
    CloudGrid g;
    int rc = cloud_enter(c, radius, &c->normals, g);
    if (rc) return rc;
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries();
    const int ni = (int)c->n;
    const double no_view[3] = {0.0, 0.0, 0.0};
    const double* v = orient == 1 ? view : no_view;
    Scratch d_n(st), d_curv(st), d_within(st), d_ref(st);
    CloudBins bins(st);
    SEGCHK(d_n.alloc(n * 12));
    if (out_curvature) SEGCHK(d_curv.alloc(n * 4));
    if (out_within) SEGCHK(d_within.alloc(n * 4));
    if (orient == 2) {
        SEGCHK(d_ref.alloc(n * 12));
        SEGCHK(hipMemcpyAsync(d_ref.p, ref_normals, n * 12, hipMemcpyHostToDevice, st));
    }
    if (bin) SEGCHK(bins.alloc(n));
    SEGCHK(hipEventRecord(c->ev[2], st));
    if (bin && (rc = cloud_bin(st, bins, ni, nullptr, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    const int* order = bin ? bins.order.as<int>() : (const int*)nullptr;
    const float* dr = orient == 2 ? d_ref.as<float>() : (const float*)nullptr;
    float* dc = out_curvature ? d_curv.as<float>() : (float*)nullptr;
    int32_t* dw = out_within ? d_within.as<int32_t>() : (int32_t*)nullptr;
    knn_dispatch(k, [&](auto K) {
        hipLaunchKernelGGL(k_knn_normal<K>, dim3((ni + 255) / 256), dim3(256), 0, st, c->d_xyz, ni, order, g, k, orient, v[0], v[1], v[2], dr, d_n.as<float>(), dc, dw);
    });
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[3], st));
    SEGCHK(hipMemcpyAsync(out_normals, d_n.p, n * 12, hipMemcpyDeviceToHost, st));
    if (out_curvature) SEGCHK(hipMemcpyAsync(out_curvature, d_curv.p, n * 4, hipMemcpyDeviceToHost, st));
    if (out_within) SEGCHK(hipMemcpyAsync(out_within, d_within.p, n * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    SEGCHK(hipEventElapsedTime(&c->normals.ms, c->ev[2], c->ev[3]));
    return 0;
}

float mpmvs_cloud_normals_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->normals, build_ms) : 0.0f; }

// ---------------------------------------------------------------------------
// the connected components of the handle's cloud under "within a radius" (pm_components.hpp): a lock-free
// union-find in one pass over the edges, a flatten pass and a size pass.  The four counts are taken on the host from the downloaded
// labels and sizes.  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
int mpmvs_cloud_components(mpmvs_cloud* c, float radius, int32_t* out_label, int32_t* out_size, long long counts[4]) {
    if (!c || (c->n > 0 && !out_label)) return seg_fail(-2, "cloud components: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "cloud components: the radius must be finite and positive");
    const size_t n = (size_t)c->n;
    if (c->n_fin == 0) {   // n == 0 included: nothing takes part
        for (size_t i = 0; i < n; ++i) {
            out_label[i] = -1;
            if (out_size) out_size[i] = 0;
        }
        if (counts) counts[0] = counts[1] = counts[2] = 0, counts[3] = -1;
        cloud_answered_on_host(c, c->cc);
        c->cc_pass_ms[0] = c->cc_pass_ms[1] = c->cc_pass_ms[2] = 0.0f;
        return 0;
    }
    CloudGrid g;
    int rc = cloud_enter(c, radius, &c->cc, g);
    if (rc) return rc;
    c->cc_pass_ms[0] = c->cc_pass_ms[1] = c->cc_pass_ms[2] = 0.0f;
    if (!c->d_cc) SEGCHK(pool_malloc(&c->d_cc, n * 4));
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries(), want_size = out_size || counts;
    const int ni = (int)c->n;
    const dim3 gp((ni + 255) / 256);
    Scratch d_label(st), d_size(st);
    CloudBins bins(st);
    SEGCHK(d_label.alloc(n * 4));
    if (want_size) SEGCHK(d_size.alloc(n * 4));
    if (bin) SEGCHK(bins.alloc(n));
    std::vector<int32_t> size_own;
    if (want_size && !out_size) size_own.resize(n);
    int32_t* size = out_size ? out_size : size_own.data();
    // the grid is built: its two events are free again, and the four borders of the three passes fit the handle's four
    SEGCHK(hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_cc_init, gp, dim3(256), 0, st, c->d_xyz, ni, c->d_cc);
    if (bin && (rc = cloud_bin(st, bins, ni, nullptr, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    hipLaunchKernelGGL(k_cc_hook, gp, dim3(256), 0, st, c->d_xyz, ni, bin ? bins.order.as<int>() : (const int*)nullptr, g, c->d_cc);
    SEGCHK(hipEventRecord(c->ev[1], st));
    hipLaunchKernelGGL(k_cc_flatten, gp, dim3(256), 0, st, ni, c->d_cc, d_label.as<int32_t>());
    SEGCHK(hipEventRecord(c->ev[2], st));
    if (want_size) {   // the parents have served: the same ints count the members of every label
        SEGCHK(hipMemsetAsync(c->d_cc, 0, n * 4, st));
        hipLaunchKernelGGL(k_cc_count, gp, dim3(256), 0, st, ni, d_label.as<int32_t>(), c->d_cc);
        hipLaunchKernelGGL(k_cc_gather, gp, dim3(256), 0, st, ni, d_label.as<int32_t>(), c->d_cc, d_size.as<int32_t>());
    }
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[3], st));
    SEGCHK(hipMemcpyAsync(out_label, d_label.p, n * 4, hipMemcpyDeviceToHost, st));
    if (want_size) SEGCHK(hipMemcpyAsync(size, d_size.p, n * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    for (int p = 0; p < 3; ++p) SEGCHK(hipEventElapsedTime(&c->cc_pass_ms[p], c->ev[p], c->ev[p + 1]));
    if (!want_size) c->cc_pass_ms[2] = 0.0f;   // two events with nothing between them
    c->cc.ms = (c->cc_pass_ms[0] + c->cc_pass_ms[1]) + c->cc_pass_ms[2];
    if (counts) {   // a component is counted at its label; the largest, ties to the smallest label
        long long comps = 0, best = 0, best_label = -1;
        for (size_t i = 0; i < n; ++i) {
            if (out_label[i] != (int32_t)i) continue;
            ++comps;
            if (size[i] > best) best = size[i], best_label = (long long)i;
        }
        counts[0] = c->n_fin, counts[1] = comps, counts[2] = best, counts[3] = best_label;
    }
    return 0;
}

float mpmvs_cloud_components_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->cc, build_ms) : 0.0f; }

int mpmvs_cloud_components_pass_ms(const mpmvs_cloud* c, float ms[3]) {
    if (!c || !ms) return seg_fail(-2, "cloud components: bad argument");
    std::memcpy(ms, c->cc_pass_ms, sizeof c->cc_pass_ms);
    return 0;
}

// ---------------------------------------------------------------------------
// registration of a moving cloud to a target handle: the ICP pass and its closed-form solve (pm_align.hpp, pm_align_host.hpp;
// DESIGN.md section 15), and the point-to-plane pass and its Gauss-Newton step beside them (pm_align_plane.hpp; section 19).
// Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
struct mpmvs_align {
    mpmvs_cloud* target;   // borrowed: its stream, grids and points serve every pass
    long long n = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float* d_src = nullptr;
    float* d_nrm = nullptr;   // a normal per target, caller order (mpmvs_align_set_normals); owned by this handle
    bool has_nrm = false;     // also true for normals of a target without points
    CloudBins bins;           // of the n sources, allocated once: a pass allocates nothing
    unsigned long long* d_sums = nullptr;
    float pass_ms = 0.0f;
    explicit mpmvs_align(mpmvs_cloud* t) : target(t), bins(t->stream) {}
};

static void align_release(mpmvs_align* h) {
    if (h->target->stream) (void)hipStreamSynchronize(h->target->stream);
    for (void* p : {(void*)h->d_src, (void*)h->d_nrm, (void*)h->d_sums})
        if (p) (void)pool_free(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;   // the bins go back to the pool here
}

static int align_create_device(mpmvs_align* h, const float* s_xyz) {
    const hipStream_t st = h->target->stream;
    SEGCHK(enter_device(h->target->device));
    for (hipEvent_t& e : h->ev) SEGCHK(hipEventCreate(&e));
    if (h->n == 0) return 0;
    const size_t n = (size_t)h->n;
    SEGCHK(pool_malloc(&h->d_src, n * 12));
    SEGCHK(h->bins.alloc(n));
    SEGCHK(pool_malloc(&h->d_sums, kAlignPlaneTerms * 8));   // the larger of the two passes' sums
    SEGCHK(hipMemcpyAsync(h->d_src, s_xyz, n * 12, hipMemcpyHostToDevice, st));
    SEGCHK(hipStreamSynchronize(st));
    return 0;
}

int mpmvs_align_create(mpmvs_cloud* target, long long n_s, const float* s_xyz, mpmvs_align** out) {
    if (!out) return seg_fail(-2, "align: bad argument");
    *out = nullptr;
    if (!target || n_s < 0 || (n_s > 0 && !s_xyz)) return seg_fail(-2, "align: bad argument");
    if (n_s > INT32_MAX) return seg_fail(-3, "align: more than 2^31 - 1 source points");
    mpmvs_align* h = new mpmvs_align(target);
    h->n = n_s;
    const int rc = align_create_device(h, s_xyz);
    if (rc) {
        align_release(h);
        return rc;
    }
    *out = h;
    return 0;
}

void mpmvs_align_destroy(mpmvs_align* h) {
    if (!h) return;
    (void)enter_device(h->target->device);
    align_release(h);
}

float mpmvs_align_ms(const mpmvs_align* h) { return h ? h->pass_ms : 0.0f; }

// the device half of a pass: the grid of `radius` (cached per radius in the target; the caller has checked the span), the binning,
// the kernel, 18 integers back (plane: the point-to-plane kernel, 38 integers)
static int align_pass(mpmvs_align* h, float radius, const AlignXf& f, bool plane, long long* sums) {
    mpmvs_cloud* c = h->target;
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries();
    CloudGrid g;
    const int rc = cloud_open(c, radius, nullptr, g);
    if (rc) return rc;
    const int n = (int)h->n;
    const size_t sums_bytes = (size_t)(plane ? kAlignPlaneTerms : kAlignTerms) * 8;
    SEGCHK(hipMemsetAsync(h->d_sums, 0, sums_bytes, st));
    if (bin) {   // by the cell of the transformed source
        const int brc = cloud_bin(st, h->bins, n, h->ev[0], [&](dim3 gq, unsigned bin_mask, int* qcnt, int* qbin) {
            hipLaunchKernelGGL(k_align_qbin, gq, dim3(256), 0, st, h->d_src, n, f, g, bin_mask, qcnt, qbin);
        });
        if (brc) return brc;
    } else {
        SEGCHK(hipEventRecord(h->ev[0], st));
    }
    const dim3 gq(((unsigned)n + 255u) / 256u);   // unsigned: n may be 2^31 - 1
    const int* order = bin ? h->bins.order.as<int>() : (const int*)nullptr;
    if (plane)
        hipLaunchKernelGGL(k_align_plane_pass, gq, dim3(256), 0, st, h->d_src, n, order, f, g, c->d_xyz, h->d_nrm, h->d_sums);
    else
        hipLaunchKernelGGL(k_align_pass, gq, dim3(256), 0, st, h->d_src, n, order, f, g, c->d_xyz, h->d_sums);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(h->ev[1], st));
    SEGCHK(hipMemcpyAsync(sums, h->d_sums, sums_bytes, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    SEGCHK(hipEventElapsedTime(&h->pass_ms, h->ev[0], h->ev[1]));
    return 0;
}

static bool align_finite12(const double M[12]) {
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(M[k])) return false;
    return true;
}

// a pass of either kind: the checks, the frame, and the cases that launch nothing
static int align_sums_any(mpmvs_align* h, float radius, const double M[12], bool plane, long long* sums, double frame[4]) {
    if (!h || !M || !sums || !frame) return seg_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return seg_fail(-2, "align: the transform must be finite");
    if (plane && !h->has_nrm) return seg_fail(-2, "align: a point-to-plane pass needs mpmvs_align_set_normals first");
    const mpmvs_cloud* c = h->target;
    for (int k = 0; k < (plane ? kAlignPlaneTerms : kAlignTerms); ++k) sums[k] = 0;
    for (int k = 0; k < 4; ++k) frame[k] = 0.0;
    h->pass_ms = 0.0f;
    if (c->n_fin == 0) return 0;   // no candidate anywhere, and no bounding box to take a frame from
    const int span = cloud_span_check(c, radius);
    if (span) return span;
    align_frame(c->mn, c->mx, radius, frame);
    if (h->n == 0) return 0;
    AlignXf f;
    for (int k = 0; k < 12; ++k) f.m[k] = M[k];
    for (int k = 0; k < 3; ++k) f.o[k] = frame[k];
    f.iu = 1.0 / frame[3];
    return align_pass(h, radius, f, plane, sums);
}

int mpmvs_align_sums(mpmvs_align* h, float radius, const double M[12], long long sums[18], double frame[4]) {
    return align_sums_any(h, radius, M, false, sums, frame);
}

int mpmvs_align_set_normals(mpmvs_align* h, const float* nrm) {
    if (!h) return seg_fail(-2, "align: bad argument");
    mpmvs_cloud* c = h->target;
    SEGCHK(enter_device(c->device));
    SEGCHK(hipStreamSynchronize(c->stream));   // no pass is reading the buffer that goes
    h->has_nrm = false;
    if (h->d_nrm) {
        SEGCHK(pool_free(h->d_nrm));
        h->d_nrm = nullptr;
    }
    if (!nrm) return 0;
    if (c->n > 0) {
        SEGCHK(pool_malloc(&h->d_nrm, (size_t)c->n * 12));
        SEGCHK(hipMemcpyAsync(h->d_nrm, nrm, (size_t)c->n * 12, hipMemcpyHostToDevice, c->stream));
        SEGCHK(hipStreamSynchronize(c->stream));
    }
    h->has_nrm = true;
    return 0;
}

int mpmvs_align_plane_sums(mpmvs_align* h, float radius, const double M[12], long long sums[38], double frame[4]) {
    return align_sums_any(h, radius, M, true, sums, frame);
}

int mpmvs_align_plane_solve(const long long sums[38], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse_plane,
                            double* rmse_point) {
    if (!sums || !frame || !M_in || !M_out) return seg_fail(-2, "align: bad argument");
    return align_plane_solve(sums, frame, with_scale, M_in, M_out, rmse_plane, rmse_point);
}

int mpmvs_align_plane_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M[12], long long* iters, long long* inliers,
                          double* rmse_plane, double* rmse_point) {
    if (!h || !M) return seg_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return seg_fail(-2, "align: the transform must be finite");
    if (max_iter < 1) return seg_fail(-2, "align: max_iter must be at least 1");
    if (!(eps >= 0.0)) return seg_fail(-2, "align: eps must not be negative");
    if (!h->has_nrm) return seg_fail(-2, "align: point-to-plane ICP needs mpmvs_align_set_normals first");
    long long n_pass = 0, sums[kAlignPlaneTerms] = {0};
    double frame[4], last_plane = 0.0, last_point = 0.0;
    for (int it = 0; it < max_iter; ++it) {
        const int rc = mpmvs_align_plane_sums(h, radius, M, sums, frame);
        if (rc < 0) return rc;
        ++n_pass;
        double D[12], next[12];
        if (align_plane_update(sums, frame, with_scale, D, &last_plane, &last_point)) break;
        align_compose(D, M, next);
        for (int k = 0; k < 12; ++k) M[k] = next[k];   // one that left the finite numbers is refused by the next pass, as in the caller's own loop
        if (align_move(D, frame) <= eps) break;
    }
    if (iters) *iters = n_pass;
    if (inliers) *inliers = sums[0];
    if (rmse_plane) *rmse_plane = last_plane;
    if (rmse_point) *rmse_point = last_point;
    return 0;
}

int mpmvs_align_solve(const long long sums[18], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse) {
    if (!sums || !frame || !M_in || !M_out) return seg_fail(-2, "align: bad argument");
    return align_solve(sums, frame, with_scale, M_in, M_out, rmse);
}

int mpmvs_align_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M[12], long long* iters, long long* inliers, double* rmse) {
    if (!h || !M) return seg_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return seg_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return seg_fail(-2, "align: the transform must be finite");
    if (max_iter < 1) return seg_fail(-2, "align: max_iter must be at least 1");
    if (!(eps >= 0.0)) return seg_fail(-2, "align: eps must not be negative");
    long long n_pass = 0, sums[18] = {0};
    double frame[4], last_rmse = 0.0;
    for (int it = 0; it < max_iter; ++it) {
        const int rc = mpmvs_align_sums(h, radius, M, sums, frame);
        if (rc < 0) return rc;
        ++n_pass;
        double D[12], next[12];
        if (align_update(sums, frame, with_scale, D, &last_rmse)) break;
        align_compose(D, M, next);
        for (int k = 0; k < 12; ++k) M[k] = next[k];   // one that left the finite numbers is refused by the next pass, as in the caller's own loop
        if (align_move(D, frame) <= eps) break;
    }
    if (iters) *iters = n_pass;
    if (inliers) *inliers = sums[0];
    if (rmse) *rmse = last_rmse;
    return 0;
}

// ---------------------------------------------------------------------------
// z-buffer render of the handle's cloud into cameras (pm_render.hpp).  The handle's grids are not touched.
// ---------------------------------------------------------------------------
static_assert(kRenderMaxSplat == MPMVS_RENDER_MAX_SPLAT, "splat bound");
constexpr size_t kRenderChunkPixels = (size_t)1 << 27;   // a chunk of views ends before its buffers pass this many pixels (one view always fits)

// views [v0, v1) in one launch of each point pass
static int cloud_render_chunk(mpmvs_cloud* c, int v0, int v1, const mpmvs_camera* cams, int splat, float m, float* const* out_depth, int32_t* const* out_idx) {
    const hipStream_t st = c->stream;
    size_t total = 0;
    bool any_idx = false;
    for (int v = v0; v < v1; ++v) {
        total += (size_t)cams[v].width * (size_t)cams[v].height;
        any_idx = any_idx || (out_idx && out_idx[v]);
    }
    Scratch d_zc(st), d_depth(st), d_idx(st);
    SEGCHK(d_zc.alloc(total * 4));
    SEGCHK(d_depth.alloc(total * 4));
    if (any_idx) SEGCHK(d_idx.alloc(total * 4));
    RenderChunkArgs A;
    std::memset(&A, 0, sizeof A);
    A.n = v1 - v0;
    size_t at = 0;
    for (int v = v0; v < v1; ++v) {
        RenderView& V = A.v[v - v0];
        cam_to_dev(cams[v], V.cam);
        V.w = cams[v].width, V.h = cams[v].height;
        V.zc = d_zc.as<uint32_t>() + at;
        V.idx = (out_idx && out_idx[v]) ? d_idx.as<uint32_t>() + at : nullptr;
        at += (size_t)V.w * (size_t)V.h;
    }
    SEGCHK(hipMemsetD32Async((hipDeviceptr_t)d_zc.p, (int)kRenderInfBits, total, st));
    if (any_idx) SEGCHK(hipMemsetAsync(d_idx.p, 0xff, total * 4, st));
    const int n = (int)c->n;
    const dim3 gp((n + 255) / 256);
    SEGCHK(hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_render_zmin, gp, dim3(256), 0, st, c->d_xyz, n, A);
    SEGCHK(hipEventRecord(c->ev[1], st));
    if (any_idx) hipLaunchKernelGGL(k_render_index, gp, dim3(256), 0, st, c->d_xyz, n, A);
    SEGCHK(hipEventRecord(c->ev[2], st));
    at = 0;
    for (int k = 0; k < A.n; ++k) {
        const RenderView& V = A.v[k];
        const size_t npix = (size_t)V.w * (size_t)V.h;
        hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, V.zc, V.w, V.h, splat, m, d_depth.as<float>() + at, V.idx);
        at += npix;
    }
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(c->ev[3], st));
    at = 0;
    for (int k = 0; k < A.n; ++k) {
        const RenderView& V = A.v[k];
        const size_t npix = (size_t)V.w * (size_t)V.h;
        SEGCHK(hipMemcpyAsync(out_depth[v0 + k], d_depth.as<float>() + at, npix * 4, hipMemcpyDeviceToHost, st));
        if (V.idx) SEGCHK(hipMemcpyAsync(out_idx[v0 + k], V.idx, npix * 4, hipMemcpyDeviceToHost, st));
        at += npix;
    }
    SEGCHK(hipStreamSynchronize(st));
    for (int p = 0; p < 3; ++p) {
        if (p == 1 && !any_idx) continue;   // no index pass: the gap between two event records is not its time
        float ms = 0.0f;
        SEGCHK(hipEventElapsedTime(&ms, c->ev[p], c->ev[p + 1]));
        c->render_pass_ms[p] += ms;
    }
    return 0;
}

int mpmvs_cloud_render_depth(mpmvs_cloud* c, int n_views, const mpmvs_camera* cams, int splat, float occl_rel, float* const* out_depth, int32_t* const* out_idx) {
    if (!c || n_views < 0) return seg_fail(-2, "cloud render: bad argument");
    if (splat < 0 || splat > MPMVS_RENDER_MAX_SPLAT) return seg_fail(-2, "cloud render: splat must lie in [0, " + std::to_string(MPMVS_RENDER_MAX_SPLAT) + "]");
    if (!std::isfinite(occl_rel) || !(occl_rel >= 0.0f)) return seg_fail(-2, "cloud render: occl_rel must be finite and not negative");
    if (n_views == 0) return 0;
    if (!cams || !out_depth) return seg_fail(-2, "cloud render: bad argument");
    for (int v = 0; v < n_views; ++v) {
        if (!out_depth[v]) return seg_fail(-2, "cloud render: view " + std::to_string(v) + " has no depth buffer");
        if (cams[v].width <= 0 || cams[v].height <= 0) return seg_fail(-2, "cloud render: view " + std::to_string(v) + " has a non-positive width or height");
    }
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].width > (1 << 24) || cams[v].height > (1 << 24)) return seg_fail(-3, "cloud render: view " + std::to_string(v) + " is wider or higher than 2^24");
        if ((long long)cams[v].width * (long long)cams[v].height > (long long)INT32_MAX)
            return seg_fail(-3, "cloud render: view " + std::to_string(v) + " has more than 2^31 - 1 pixels");
    }
    c->render_pass_ms[0] = c->render_pass_ms[1] = c->render_pass_ms[2] = 0.0f;
    if (c->n_fin == 0) {   // nothing lands anywhere
        for (int v = 0; v < n_views; ++v) {
            const size_t npix = (size_t)cams[v].width * (size_t)cams[v].height;
            std::fill(out_depth[v], out_depth[v] + npix, 0.0f);
            if (out_idx && out_idx[v]) std::fill(out_idx[v], out_idx[v] + npix, (int32_t)-1);
        }
        return 0;
    }
    SEGCHK(enter_device(c->device));
    const float m = 1.0f + occl_rel;
    for (int v0 = 0; v0 < n_views;) {
        int v1 = v0 + 1;
        size_t pixels = (size_t)cams[v0].width * (size_t)cams[v0].height;
        while (v1 < n_views && v1 - v0 < kRenderChunk && pixels + (size_t)cams[v1].width * (size_t)cams[v1].height <= kRenderChunkPixels) {
            pixels += (size_t)cams[v1].width * (size_t)cams[v1].height;
            ++v1;
        }
        const int rc = cloud_render_chunk(c, v0, v1, cams, splat, m, out_depth, out_idx);
        if (rc) return rc;
        v0 = v1;
    }
    return 0;
}

float mpmvs_cloud_render_ms(const mpmvs_cloud* c) { return c ? (c->render_pass_ms[0] + c->render_pass_ms[1]) + c->render_pass_ms[2] : 0.0f; }

int mpmvs_cloud_render_pass_ms(const mpmvs_cloud* c, float ms[3]) {
    if (!c || !ms) return seg_fail(-2, "cloud render: bad argument");
    std::memcpy(ms, c->render_pass_ms, sizeof c->render_pass_ms);
    return 0;
}

// ---------------------------------------------------------------------------
// the space the scanners of a scan observed: a resident range cube map per scanner position and the classification of query points
// against it (pm_observe.hpp).  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
static_assert(kObserveMaxScanners == MPMVS_OBSERVE_MAX_SCANNERS && kObserveMaxFace == MPMVS_OBSERVE_MAX_FACE && kObserveMaxWindow == MPMVS_OBSERVE_MAX_WINDOW,
              "observer bounds");
constexpr long long kObserveChunkQueries = 1ll << 24;       // queries per launch of the classify pass: 320 MB of device buffers at most

struct mpmvs_observer {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // the borders of the two passes of a chunk; ev[0], ev[1]: of a classify launch
    ObserveScanners sc;                               // all scanners, j0 = 0
    int R = 0, w = 0;
    float* d_zn = nullptr;                            // [n_scanners][6][R][R]
    long long stats[2] = {0, 0};
    float build_pass_ms[2] = {0.0f, 0.0f}, classify_ms = 0.0f;
};

static void observer_release(mpmvs_observer* h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_zn) (void)pool_free(h->d_zn);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// the device half of mpmvs_observer_create: Zc and Zn of one chunk of scanners after the other; the scan's points are read in place
static int observer_create_device(mpmvs_observer* h, const mpmvs_cloud* scan, const int* owner) {
    SEGCHK(enter_device(scan->device));
    SEGCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev) SEGCHK(hipEventCreate(&e));
    const hipStream_t st = h->stream;
    const size_t map = (size_t)6 * (size_t)h->R * (size_t)h->R, total = map * (size_t)h->sc.n;
    SEGCHK(pool_malloc(&h->d_zn, total * 4));
    if (scan->n_fin == 0) {   // nothing lands anywhere
        SEGCHK(hipMemsetD32Async((hipDeviceptr_t)h->d_zn, (int)kRenderInfBits, total, st));
        SEGCHK(hipStreamSynchronize(st));
        return 0;
    }
    const int per = (int)std::min<size_t>((size_t)kObserveChunk, std::max<size_t>(1, kObserveChunkPixels / map));
    const int n = (int)scan->n;
    Scratch d_zc(st), d_owner(st), d_cnt(st);
    SEGCHK(d_zc.alloc(map * (size_t)std::min(per, h->sc.n) * 4));
    SEGCHK(d_cnt.alloc(8));
    SEGCHK(hipMemsetAsync(d_cnt.p, 0, 8, st));
    if (owner) {
        SEGCHK(d_owner.alloc((size_t)n * 4));
        SEGCHK(hipMemcpyAsync(d_owner.p, owner, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    for (int j0 = 0; j0 < h->sc.n; j0 += per) {
        ObserveScanners A = h->sc;
        A.j0 = j0, A.n = std::min(per, h->sc.n - j0);
        const size_t n_pix = map * (size_t)A.n;
        SEGCHK(hipMemsetD32Async((hipDeviceptr_t)d_zc.p, (int)kRenderInfBits, n_pix, st));
        SEGCHK(hipEventRecord(h->ev[0], st));
        hipLaunchKernelGGL(k_observe_zmin, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, st, scan->d_xyz, n, owner ? d_owner.as<int>() : (const int*)nullptr, A,
                           h->R, d_zc.as<uint32_t>());
        SEGCHK(hipEventRecord(h->ev[1], st));
        hipLaunchKernelGGL(k_observe_near, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, d_zc.as<uint32_t>(), n_pix, h->R, h->w,
                           h->d_zn + map * (size_t)j0, d_cnt.as<unsigned long long>());
        SEGCHK(hipGetLastError());
        SEGCHK(hipEventRecord(h->ev[2], st));
        SEGCHK(hipStreamSynchronize(st));
        for (int p = 0; p < 2; ++p) {
            float ms = 0.0f;
            SEGCHK(hipEventElapsedTime(&ms, h->ev[p], h->ev[p + 1]));
            h->build_pass_ms[p] += ms;
        }
    }
    unsigned long long covered = 0;
    SEGCHK(hipMemcpyAsync(&covered, d_cnt.p, 8, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    h->stats[0] = (long long)covered;
    return 0;
}

int mpmvs_observer_create(mpmvs_cloud* scan, int n_scanners, const float* scanners_xyz, const int* owner, int face_size, int window, mpmvs_observer** out) {
    if (!out) return seg_fail(-2, "observer: bad argument");
    *out = nullptr;
    if (!scanners_xyz) return seg_fail(-2, "observer: bad argument");
    if (n_scanners < 1 || n_scanners > MPMVS_OBSERVE_MAX_SCANNERS)
        return seg_fail(-2, "observer: the number of scanners must lie in [1, " + std::to_string(MPMVS_OBSERVE_MAX_SCANNERS) + "]");
    for (int k = 0; k < 3 * n_scanners; ++k)
        if (!std::isfinite(scanners_xyz[k])) return seg_fail(-2, "observer: scanner " + std::to_string(k / 3) + " has a non-finite coordinate");
    if (face_size < 1 || face_size > MPMVS_OBSERVE_MAX_FACE) return seg_fail(-2, "observer: face_size must lie in [1, " + std::to_string(MPMVS_OBSERVE_MAX_FACE) + "]");
    if (window < 0 || window > MPMVS_OBSERVE_MAX_WINDOW) return seg_fail(-2, "observer: window must lie in [0, " + std::to_string(MPMVS_OBSERVE_MAX_WINDOW) + "]");
    if ((long long)n_scanners * 6 * face_size * face_size > (1ll << 31)) return seg_fail(-3, "observer: more than 2^31 pixels (scanners x 6 x face_size^2)");
    if (!scan) return seg_fail(-2, "observer: no scan");   // after the checks that need none
    for (long long i = 0; owner && i < scan->n; ++i)
        if (owner[i] < -1 || owner[i] >= n_scanners)
            return seg_fail(-2, "observer: owner[" + std::to_string(i) + "] = " + std::to_string(owner[i]) + " is neither -1 nor a scanner");
    mpmvs_observer* h = new mpmvs_observer;
    h->device = scan->device;
    std::memset(&h->sc, 0, sizeof h->sc);
    h->sc.n = n_scanners;
    std::memcpy(h->sc.s, scanners_xyz, (size_t)n_scanners * 12);
    h->R = face_size, h->w = window;
    h->stats[1] = (long long)n_scanners * 6 * face_size * face_size;
    const int rc = observer_create_device(h, scan, owner);
    if (rc) {
        observer_release(h);
        return rc;
    }
    *out = h;
    return 0;
}

void mpmvs_observer_destroy(mpmvs_observer* h) {
    if (!h) return;
    (void)enter_device(h->device);
    observer_release(h);
}

// queries [0, n) of one launch
static int observer_classify_chunk(mpmvs_observer* h, int n, const float* q_xyz, float m1, float abs_margin, int* out_free, int* out_covered) {
    const hipStream_t st = h->stream;
    Scratch d_q(st), d_free(st), d_cov(st);
    SEGCHK(d_q.alloc((size_t)n * 12));
    SEGCHK(d_free.alloc((size_t)n * 4));
    if (out_covered) SEGCHK(d_cov.alloc((size_t)n * 4));
    SEGCHK(hipMemcpyAsync(d_q.p, q_xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
    SEGCHK(hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(k_observe_classify, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, st, d_q.as<float>(), n, h->sc, h->R, h->d_zn, m1, abs_margin,
                       d_free.as<int>(), out_covered ? d_cov.as<int>() : (int*)nullptr);
    SEGCHK(hipGetLastError());
    SEGCHK(hipEventRecord(h->ev[1], st));
    SEGCHK(hipMemcpyAsync(out_free, d_free.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (out_covered) SEGCHK(hipMemcpyAsync(out_covered, d_cov.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    SEGCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    SEGCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->classify_ms += ms;
    return 0;
}

int mpmvs_observer_classify(mpmvs_observer* h, long long n_q, const float* q_xyz, float rel, float abs_margin, int* out_free, int* out_covered) {
    if (!std::isfinite(rel) || !(rel >= 0.0f && rel < 1.0f)) return seg_fail(-2, "observer: rel must lie in [0, 1)");
    if (!std::isfinite(abs_margin) || !(abs_margin >= 0.0f)) return seg_fail(-2, "observer: abs_margin must be finite and not negative");
    if (n_q < 0 || !out_free || (n_q > 0 && !q_xyz)) return seg_fail(-2, "observer: bad argument");
    if (n_q > INT32_MAX) return seg_fail(-3, "observer: more than 2^31 - 1 queries");
    if (!h) return seg_fail(-2, "observer: no handle");   // after the checks that need none
    h->classify_ms = 0.0f;
    if (n_q == 0) return 0;
    SEGCHK(enter_device(h->device));
    const float m1 = 1.0f - rel;
    for (long long q0 = 0; q0 < n_q; q0 += kObserveChunkQueries) {
        const int n = (int)std::min(kObserveChunkQueries, n_q - q0);
        const int rc = observer_classify_chunk(h, n, q_xyz + 3 * q0, m1, abs_margin, out_free + q0, out_covered ? out_covered + q0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpmvs_observer_maps(mpmvs_observer* h, int scanner, float* out_near) {
    if (!h || !out_near) return seg_fail(-2, "observer: bad argument");
    if (scanner < 0 || scanner >= h->sc.n) return seg_fail(-2, "observer: no scanner " + std::to_string(scanner));
    SEGCHK(enter_device(h->device));
    const size_t map = (size_t)6 * (size_t)h->R * (size_t)h->R;
    SEGCHK(hipMemcpyAsync(out_near, h->d_zn + map * (size_t)scanner, map * 4, hipMemcpyDeviceToHost, h->stream));
    SEGCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int mpmvs_observer_stats(mpmvs_observer* h, long long out[2]) {
    if (!h || !out) return seg_fail(-2, "observer: bad argument");
    out[0] = h->stats[0], out[1] = h->stats[1];
    return 0;
}

float mpmvs_observer_ms(mpmvs_observer* h, float build_ms[2]) {
    if (!h) return 0.0f;
    if (build_ms) build_ms[0] = h->build_pass_ms[0], build_ms[1] = h->build_pass_ms[1];
    return h->classify_ms;
}

}  // extern "C"
