// mpmvs_api.hip -- the PatchMatch context of the C ABI declared in include/mpmvs.h, and nothing else: context
// and HBM residency management, uploads (upload_views for both image entries; its host half, the staging
// plan and the row work, is pm_stage.hpp), the Run() launch schedule (reference src/PatchMatch.cu:1188-1254), the planar prior,
// the self-check of the chained launch and the probes used by the parity tests.  struct mpmvs_ctx is private to this file; the
// other families of the library are mpmvs_fusion.hip, mpmvs_image.hip, mpmvs_skyseg.hip and mpmvs_cloud.hip, and what all of
// them share is pm_host.hpp (mpmvs_host.hip).
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
#include "pm_host.hpp"
#include "pm_kernels.hpp"
#include "pm_prior.hpp"
#include "pm_ingest.hpp"
#include "pm_stage.hpp"

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

#ifdef PM_DBG_WAVETIME
static size_t kWaveTimeBytes(int W, int H) { return (size_t)16 * ((size_t)(W / 16 + 2) * (H / 8 + 8)) * pm::kWaveRecWords * 8; }
#endif

#define HIPCHK(ctx, expr)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            return -100;                                                                            \
        }                                                                                           \
    } while (0)

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

mpmvs_ctx* mpmvs_create(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        call_error() = std::string("no HIP device available: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (device < 0 || device >= n) {
        call_error() = "device index out of range";
        return nullptr;
    }
    if ((e = enter_device(device)) != hipSuccess) {
        call_error() = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    mpmvs_ctx* c = new mpmvs_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = pool_malloc(&c->dP, sizeof(ProblemDev))) != hipSuccess) {
        call_error() = std::string("context setup: ") + hipGetErrorString(e);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        (void)hipGetLastError();
        delete c;
        return nullptr;
    }
    std::memset(&c->hP, 0, sizeof(ProblemDev));
    c->h_sync_err = static_cast<int*>(mpmvs_alloc_pinned(sizeof(int)));   // pooled page-locked memory (include/mpmvs.h)
    if (!c->h_sync_err) {   // without it a timed-out chained launch would go unreported
        call_error() = "context setup: no page-locked memory for the error word of the update launches";
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

const char* mpmvs_last_error(const mpmvs_ctx* c) { return c ? c->err.c_str() : call_error().c_str(); }

}  // extern "C"

// what the fusion may know of a context (pm_host.hpp)
int ctx_resident_planes(const mpmvs_ctx* c, int w, int h, int* device, hipStream_t* stream, const float4** planes) {
    if (c->W != w || c->H != h || !c->S.planes || !c->depth_plane_valid || c->async_outstanding) return -2;   // no finished Run() of that size behind it
    *device = c->device;
    *stream = c->stream;
    *planes = c->S.planes;
    return 0;
}

extern "C" {

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
    // room for 16 launches of one wave per 64 pixels of a colour, kWaveRecWords x u64 each (generous: blocks overhang the image border)
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
    if (launch(k_ingest_pad, dim3((dst_w + 255) / 256, dst_h), dim3(256), call.stream(), ingest_src(d_src, src_w, src_h, dst_w, dst_h), dst_w, dst_h, d_out, 0) != hipSuccess)
        return -100;
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
// measurement builds: the per-wave records of the last <= 16 update launches ([launch % 16][wave][kWaveRecWords] u64; pm_kernels.hpp, WaveTimer)
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
    HIPCHK(c, launch(k_export_depth, dim3((n + 255) / 256), dim3(256), c->stream, c->S.planes, d_out, n));
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
    HIPCHK(c, launch(k_eval_geom, grid, dim3(256), c->stream, c->dP, d_pl.as<float4>(), d_out.as<float>()));
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
    HIPCHK(c, launch(k_homography, dim3(1), dim3(64), c->stream, c->dP, make_float4(pf[0], pf[1], pf[2], pf[3]), v, d_h.as<float>()));
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
    // the vertex picker packs (y << 16) | x and the row bound of the raster is stated up to that size (pm_prior.hpp)
    if (W > kPriorMaxSide || H > kPriorMaxSide) return fail(c, -3, "image side above 65535: no planar prior at this size");
    // vertex check and task table in one parallel sweep: 64 consecutive p-rows of one triangle per wave (pm_prior.hpp).  The
    // rows of a triangle are prior_rows() of its longest edge: at least as many as the reference's fp32 accumulation of p runs
    // (which is not floor(L) + 2: from L ~ 12 000 on the rounding of the accumulation adds whole rows), and less than one task
    // more; the kernel's own p < 1 test is what decides.  Chunks of triangles are counted, their task ranges follow by a
    // prefix sum, then filled: the table is the one the sequential loop would build.
    const size_t wh = (size_t)W * H;
    auto rows_of = [&](int t) { return prior_rows(prior_longest_edge_sq(tri_xy + 6 * (size_t)t)); };
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
            if (!ok) break;  // the call is refused: no rows are counted for coordinates that were not checked
            k += (size_t)(rows_of(t) + kPriorTaskRows - 1) / kPriorTaskRows;
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
            for (int r0 = 0; r0 < rows; r0 += kPriorTaskRows) {
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

int mpmvs_prior_rows(const long long* edge_sq, int n, int* rows) {
    if (n < 0 || (n > 0 && (!edge_sq || !rows))) return -1;
    for (int i = 0; i < n; ++i)
        if (edge_sq[i] < 0 || edge_sq[i] > kPriorMaxEdgeSq) return -1;
    // long edges cost O(L) each: interleaved over a few host threads
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = n >= 1024 ? (int)std::max(1u, std::min(16u, hw ? hw : 1u)) : 1;
    auto part = [&](int k) {
        for (int i = k; i < n; i += nthreads) rows[i] = prior_rows(edge_sq[i]);
    };
    std::vector<std::thread> pool;
    for (int k = 1; k < nthreads; ++k) pool.emplace_back(part, k);
    part(0);
    for (std::thread& t : pool) t.join();
    return 0;
}

int mpmvs_math(int fn, const void* in, void* out, int n) {
    if (fn < 0 || fn > 6 || n <= 0) return -1;
    DeviceCall call;
    float *d_in = call.alloc<float>((size_t)n * 4), *d_out = call.alloc<float>((size_t)n * 4);
    if (!d_in || !d_out) return -100;
    if (hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) return -100;
    if (launch(k_math, dim3((n + 255) / 256), dim3(256), call.stream(), fn, d_in, d_out, n) != hipSuccess) return -100;
    return hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}

int mpmvs_verify_rcp(unsigned long long counts[4]) {
    if (!counts) return -1;
    DeviceCall call;
    unsigned long long* d = call.alloc<unsigned long long>(32);
    if (!d || hipMemset(d, 0, 32) != hipSuccess) return -100;
    for (uint64_t base = 0; base < (1ULL << 32); base += (1ULL << 24)) {
        if (launch(k_verify_rcp, dim3(1 << 16), dim3(256), call.stream(), (uint32_t)base, d) != hipSuccess) return -100;
    }
    return hipMemcpy(counts, d, 32, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
}

int mpmvs_rng(uint64_t seed, uint32_t pix, uint32_t launch_id, int n, void* out) {
    if (n <= 0) return -1;
    DeviceCall call;
    float* d_out = call.alloc<float>((size_t)n * 4);
    if (!d_out) return -100;
    if (launch(k_rng, dim3(1), dim3(64), call.stream(), seed, pix, launch_id, n, d_out) != hipSuccess) return -100;
    return hipMemcpy(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -100;
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

}  // extern "C"
