// mpmvs_cloud.hip -- the point clouds of the C ABI declared in include/mpmvs.h: the search handle (mpmvs_cloud), its grid cache
// and the one prologue of every operation on it; nearest, voxel downsampling, kNN, outlier removal, normals and components; and
// the scoring calls that work on a handle's grid -- ICP in both forms (mpmvs_align), depth rendering and the observer.  The
// scoring calls stay in this file: they launch the binning kernels of pm_cloud.hpp through the cloud_bin template and read the
// handle's members, so a file of their own would need pm_cloud.hpp a second time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_scan_host.hpp"
#include "pm_cloud.hpp"
#include "pm_voxel.hpp"
#include "pm_cluster_host.hpp"
#include "pm_knn.hpp"
#include "pm_normals.hpp"
#include "pm_components.hpp"
#include "pm_align.hpp"
#include "pm_align_plane.hpp"
#include "pm_align_host.hpp"
#include "pm_render.hpp"
#include "pm_observe.hpp"
#include "pm_mesh_host.hpp"
#include "pm_surface.hpp"

using namespace pm;

extern "C" {

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
    PassClock<4> clock;   // build begin / end, query begin / end; a render: the borders of its three passes
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
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;   // the clock goes here: the stream has been waited for
}

static int cloud_create_device(mpmvs_cloud* c, const float* xyz) {
    CALLCHK(enter_device(c->device));
    CALLCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (c->n_fin == 0) return 0;   // nothing to search: every call answers on the host
    const size_t n = (size_t)c->n, slots = (size_t)1 << c->slots_log2;
    CALLCHK(pool_malloc(&c->d_xyz, n * 12));
    CALLCHK(pool_malloc(&c->d_slot_of, n * 4));
    CALLCHK(pool_malloc(&c->d_cnt, slots * 4));
    CALLCHK(pool_malloc(&c->d_tsum, slots / kScanBlock * 4));
    CALLCHK(pool_malloc(&c->d_st, 8));
    CALLCHK(hipMemcpyAsync(c->d_xyz, xyz, n * 12, hipMemcpyHostToDevice, c->stream));
    CALLCHK(hipStreamSynchronize(c->stream));
    return 0;
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
        (void)call_fail(-3, std::string(who) + ": more than 2^29 finite points (the table would exceed 2^30 slots)");
        return nullptr;
    }
    return c;
}

int mpmvs_cloud_create(int device, long long n, const float* xyz, mpmvs_cloud** cloud) {
    if (!cloud) return call_fail(-2, "cloud: bad argument");
    *cloud = nullptr;
    if (n < 0 || (n > 0 && !xyz)) return call_fail(-2, "cloud: bad argument");
    if (n > INT32_MAX) return call_fail(-3, "cloud: more than 2^31 - 1 points");
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

// builds the grid of `radius` into g, whose buffers exist
static int cloud_build(mpmvs_cloud* c, CloudGridBuf& g, float radius) {
    const hipStream_t st = c->stream;
    const size_t slots = (size_t)1 << c->slots_log2;
    const int n = (int)c->n;
    const double edge = cloud_edge(radius);
    CALLCHK(hipMemsetAsync(g.d_keys, 0xff, slots * 8, st));
    CALLCHK(hipMemsetAsync(c->d_cnt, 0, slots * 4, st));
    CALLCHK(hipMemsetAsync(c->d_st, 0, 8, st));
    CALLCHK(c->clock.mark(0, st));
    const dim3 gp((n + 255) / 256), gs((unsigned)(slots / 256));
    CALLCHK(launch(k_cloud_insert, gp, dim3(256), st, c->d_xyz, n, (double)c->mn[0], (double)c->mn[1], (double)c->mn[2], edge, (unsigned)(slots - 1), g.d_keys,
                   c->d_cnt, c->d_slot_of));
    CALLCHK(launch(k_cloud_stats, gs, dim3(256), st, c->d_cnt, (unsigned)slots, c->d_st));
    CALLCHK(scan_offsets(st, c->d_cnt, (int)slots, g.d_off, c->d_tsum, g.d_off + slots, true));   // slot counts -> offsets, off[slots] = the total
    CALLCHK(launch(k_cloud_scatter, gp, dim3(256), st, c->d_xyz, n, c->d_slot_of, g.d_off, c->d_cnt, g.d_pts));
    CALLCHK(c->clock.mark(1, st));
    int h_st[2] = {0, 0};
    CALLCHK(hipMemcpyAsync(h_st, c->d_st, 8, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(c->clock.ms(0, 1, &c->query.build_ms));
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
                if (c->grids.empty()) return call_fail(-100, "cloud: no device memory for the grid");
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
// The one binning path: the serving order of nq <= cap queries into b.order.  The counts are cleared, begin() marks the caller's
// clock -- the callers whose timed interval opens after the memset pass their mark, the others no_mark -- and then count / scan /
// order run.  count(grid, bin_mask, qcnt, qbin) launches the counting kernel, the only part that differs: k_cloud_qbin on raw
// queries, k_align_qbin on transformed sources.
template <typename Begin, typename Count>
static int cloud_bin(hipStream_t st, CloudBins& b, int nq, Begin&& begin, Count&& count) {
    const size_t bins = (size_t)1 << cloud_bins_log2(nq);   // <= what alloc sized
    const dim3 gq(((unsigned)nq + 255u) / 256u);            // unsigned: nq may be 2^31 - 1
    CALLCHK(hipMemsetAsync(b.qcnt.p, 0, bins * 4, st));
    CALLCHK(begin());
    CALLCHK(count(gq, (unsigned)(bins - 1), b.qcnt.as<int>(), b.qbin.as<int>()));
    CALLCHK(scan_offsets(st, b.qcnt.as<int>(), (int)bins, b.qoff.as<int>(), b.qtsum.as<int>(), b.qoff.as<int>() + bins, true));
    CALLCHK(launch(k_cloud_qorder, gq, dim3(256), st, nq, b.qbin.as<int>(), b.qoff.as<int>(), b.qcnt.as<int>(), b.order.as<int>()));
    return 0;
}
static hipError_t no_mark() { return hipSuccess; }
// the counting launch of raw queries
static auto cloud_count_queries(hipStream_t st, const float* d_q, int nq, const CloudGrid& g) {
    return [=](dim3 gq, unsigned bin_mask, int* qcnt, int* qbin) { return launch(k_cloud_qbin, gq, dim3(256), st, d_q, nq, g, bin_mask, qcnt, qbin); };
}

// The one dispatch over the list sizes of the kNN family (pm_knn.hpp: knn_list_size): run(std::integral_constant<int, K>) with
// the K of 4, 8, 16 or 32 that serves k; what run returns
template <typename F>
static int knn_dispatch(int k, F&& run) {
    switch (knn_list_size(k)) {
        case 4: return run(std::integral_constant<int, 4>{});
        case 8: return run(std::integral_constant<int, 8>{});
        case 16: return run(std::integral_constant<int, 16>{});
        default: return run(std::integral_constant<int, 32>{});
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
            return call_fail(-3, msg);
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
    CALLCHK(enter_device(c->device));
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
    if (!c || !out_d2 || n_q < 0 || (n_q > 0 && !q_xyz)) return call_fail(-2, "cloud: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "cloud: the radius must be finite and positive");
    if (n_q > INT32_MAX) return call_fail(-3, "cloud: more than 2^31 - 1 queries");
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
    CALLCHK(d_q.alloc(q * 12));
    CALLCHK(d_d2.alloc(q * 4));
    if (out_idx) CALLCHK(d_idx.alloc(q * 4));
    if (bin) CALLCHK(bins.alloc(q));
    CALLCHK(hipMemcpyAsync(d_q.p, q_xyz, q * 12, hipMemcpyHostToDevice, st));
    if (bin) {
        const int brc = cloud_bin(st, bins, nq, [&] { return c->clock.mark(2, st); }, cloud_count_queries(st, d_q.as<float>(), nq, g));
        if (brc) return brc;
    } else {
        CALLCHK(c->clock.mark(2, st));
    }
    CALLCHK(launch(k_cloud_query, dim3(((unsigned)nq + 255u) / 256u), dim3(256), st, d_q.as<float>(), nq, bins.order.as<int>(), g, d_d2.as<float>(),
                   d_idx.as<int32_t>()));
    CALLCHK(c->clock.mark(3, st));
    CALLCHK(hipMemcpyAsync(out_d2, d_d2.p, q * 4, hipMemcpyDeviceToHost, st));
    if (out_idx) CALLCHK(hipMemcpyAsync(out_idx, d_idx.p, q * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(c->clock.ms(2, 3, &c->query.ms));
    return 0;
}

int mpmvs_cloud_stats(const mpmvs_cloud* c, long long stats[4]) {
    if (!c || !stats) return call_fail(-2, "cloud: bad argument");
    std::memcpy(stats, c->stats, sizeof c->stats);
    return 0;
}

float mpmvs_cloud_kernel_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->query, build_ms) : 0.0f; }

// ---------------------------------------------------------------------------
// exact capped distance from a cloud's points to a mesh's surface (pm_surface.hpp; statement 5 of the mesh
// section of include/mpmvs.h).  It lives here because it walks the cloud's grid; of the mesh it reads the resident vertices and
// triangles (pm_mesh_host.hpp).  The launches go to the cloud's stream: the mesh's buffers are only read, and every call on either
// handle waits for its stream before it returns.
// ---------------------------------------------------------------------------
// MPMVS_SURFACE_LARGE=<cells>: the size of a triangle's cell range above which a block walks it; read at every call (tests force
// both paths through it)
static int surface_large_threshold() {
    const char* e = std::getenv("MPMVS_SURFACE_LARGE");
    if (!e || !*e) return kSurfaceLargeDefault;
    const long v = std::strtol(e, nullptr, 10);
    return v < 0 ? 0 : (v > (1l << 30) ? (1 << 30) : (int)v);
}

int mpmvs_surface_distance(mpmvs_mesh* surface, mpmvs_cloud* points, float radius, float* out_d2, int32_t* out_tri, long long counts[2]) {
    mpmvs_mesh* const h = surface;
    mpmvs_cloud* const c = points;
    if (!h || !c) return call_fail(-2, "surface distance: a NULL handle");
    if (c->n > 0 && !out_d2) return call_fail(-2, "surface distance: out_d2 missing");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "surface distance: the radius must be finite and positive");
    if (h->device != c->device) return call_fail(-2, "surface distance: the mesh is on device " + std::to_string(h->device) + ", the cloud on device " + std::to_string(c->device));
    const int span = cloud_span_check(c, radius, "surface distance: the points");
    if (span) return span;
    h->dist_ms[0] = h->dist_ms[1] = h->dist_ms[2] = 0.0f;
    if (c->n == 0) {
        if (counts) counts[0] = counts[1] = 0;
        return 0;
    }
    if (h->m_fin == 0 || c->n_fin == 0) {   // no triangle or no point takes part: answered here
        for (long long i = 0; i < c->n; ++i) {
            out_d2[i] = INFINITY;
            if (out_tri) out_tri[i] = -1;
        }
        if (counts) counts[0] = 0, counts[1] = c->n_fin;
        return 0;
    }
    const int rc = mesh_ready(h);
    if (rc) return rc;
    SurfaceGrid S;
    const int rc2 = cloud_open(c, radius, nullptr, S.g);   // the build time stays with the cloud's own report
    if (rc2) return rc2;
    S.gmax = 0.0;
    for (int a = 0; a < 3; ++a) {
        S.hi[a] = cloud_cell(c->mx[a], S.g.mn[a], S.g.edge);
        S.hi[a] = S.hi[a] < 0 ? 0 : (S.hi[a] > kCloudAxisCells - 1 ? kCloudAxisCells - 1 : S.hi[a]);   // as the insert clamps
        S.gmax = std::max(S.gmax, std::max(std::fabs((double)c->mn[a]), std::fabs((double)c->mx[a]) + S.g.edge));
    }
    S.reach = ((double)radius + 0.8660254037844387 * S.g.edge) * (1.0 + 0x1p-8);
    S.large = surface_large_threshold();
    const hipStream_t st = c->stream;
    const size_t n = (size_t)c->n, m = (size_t)h->m;
    PassClock<4> clock;   // before the buffers: they wait for the stream when they go
    Scratch d_keys(st), d_list(st), d_cnt(st), d_d2(st), d_tri(st);
    CALLCHK(d_keys.alloc(n * 8));
    CALLCHK(d_list.alloc(m * 4));
    CALLCHK(d_cnt.alloc(16));   // the length of the list, the points with a candidate
    CALLCHK(d_d2.alloc(n * 4));
    if (out_tri) CALLCHK(d_tri.alloc(n * 4));
    unsigned long long* const n_list = d_cnt.as<unsigned long long>();
    CALLCHK(hipMemsetAsync(d_cnt.p, 0, 16, st));
    const dim3 blk(256), gn((unsigned)((n + 255) / 256)), gm((unsigned)((m + 255) / 256));
    CALLCHK(clock.mark(0, st));
    CALLCHK(launch(k_surface_init, gn, blk, st, (int)c->n, d_keys.as<unsigned long long>()));
    CALLCHK(clock.mark(1, st));
    CALLCHK(launch(k_surface_scatter, gm, blk, st, (int)h->m, h->d_xyz, h->d_tri, S, d_keys.as<unsigned long long>(), d_list.as<int32_t>(), n_list));
    // the listed triangles: as many blocks as the device keeps busy, striding over a list whose length they read themselves
    CALLCHK(launch(k_surface_large, dim3((unsigned)std::min<size_t>(m, 2048)), blk, st, h->d_xyz, h->d_tri, S, d_keys.as<unsigned long long>(), d_list.as<int32_t>(),
                   n_list));
    CALLCHK(clock.mark(2, st));
    CALLCHK(launch(k_surface_finish, gn, blk, st, (int)c->n, d_keys.as<unsigned long long>(), d_d2.as<float>(), d_tri.as<int32_t>(), n_list + 1));
    CALLCHK(clock.mark(3, st));
    unsigned long long cnt[2] = {0, 0};
    CALLCHK(hipMemcpyAsync(out_d2, d_d2.p, n * 4, hipMemcpyDeviceToHost, st));
    if (out_tri) CALLCHK(hipMemcpyAsync(out_tri, d_tri.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(cnt, d_cnt.p, 16, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) CALLCHK(clock.ms(k, k + 1, &h->dist_ms[k]));
    if (counts) counts[0] = (long long)cnt[1], counts[1] = c->n_fin;
    return 0;
}

float mpmvs_surface_distance_ms(const mpmvs_mesh* surface, float pass_ms[3]) {
    if (!surface) return 0.0f;
    if (pass_ms) std::memcpy(pass_ms, surface->dist_ms, sizeof surface->dist_ms);
    return (surface->dist_ms[0] + surface->dist_ms[1]) + surface->dist_ms[2];
}

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

long long mpmvs_cloud_voxel_downsample(int device, long long n, const float* xyz, const float* normals, const unsigned char* rgb, float voxel, float** out_xyz,
                                       float** out_normals, unsigned char** out_rgb, int32_t** out_count, int32_t** out_first, int32_t* out_voxel_of) {
    if (n < 0 || (n > 0 && !xyz) || !out_xyz || !out_count || !out_first || (normals && !out_normals) || (rgb && !out_rgb))
        return call_fail(-2, "voxel: bad argument");
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return call_fail(-2, "voxel: the voxel size must be finite and positive");
    *out_xyz = nullptr, *out_count = nullptr, *out_first = nullptr;
    if (out_normals) *out_normals = nullptr;
    if (out_rgb) *out_rgb = nullptr;
    if (n > INT32_MAX) return call_fail(-3, "voxel: more than 2^31 - 1 points");
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    const long long n_fin = cloud_bbox(n, xyz, mn, mx);
    const ClusterNames names = {"voxel", "points", "voxel", "voxels"};
    int slots_log2 = 0;
    VoxelGrid g;
    if (cluster_refusal(names, n_fin, mn, mx, voxel, &slots_log2, &g)) return -3;
    if (n_fin == 0) {   // nothing occupies a voxel: answered on the host
        if (out_voxel_of)
            for (long long i = 0; i < n; ++i) out_voxel_of[i] = -1;
        g_voxel_ms = 0.0f;
        std::memset(g_voxel_pass_ms, 0, sizeof g_voxel_pass_ms);
        return 0;
    }

    HostOut out;
    DeviceCall call(device);
    if (!call.ok()) return call_fail(-100, "voxel: the device could not be selected or gave no stream");
    const hipStream_t st = call.stream();
    Clusters cl(st, names, true);   // after the call: its buffers and its clock go while the stream exists
    const size_t np = (size_t)n;
    float* d_xyz = call.alloc<float>(np * 12);
    float* d_nrm = normals ? call.alloc<float>(np * 12) : nullptr;
    unsigned char* d_rgb = rgb ? call.alloc<unsigned char>(np * 3) : nullptr;
    if (!d_xyz || (normals && !d_nrm) || (rgb && !d_rgb)) return call_fail(-100, "voxel: no device memory");
    CALLCHK(hipMemcpyAsync(d_xyz, xyz, np * 12, hipMemcpyHostToDevice, st));
    if (normals) CALLCHK(hipMemcpyAsync(d_nrm, normals, np * 12, hipMemcpyHostToDevice, st));
    if (rgb) CALLCHK(hipMemcpyAsync(d_rgb, rgb, np * 3, hipMemcpyHostToDevice, st));
    if (cl.mark(d_xyz, (int)n, n_fin, slots_log2, g)) return -100;
    const size_t mv = (size_t)cl.count;
    float* h_xyz = out.take<float>(mv * 3);
    int32_t* h_count = out.take<int32_t>(mv);
    int32_t* h_first = out.take<int32_t>(mv);
    float* h_nrm = normals ? out.take<float>(mv * 3) : nullptr;
    unsigned char* h_rgb = rgb ? out.take<unsigned char>(mv * 3) : nullptr;
    if (!h_xyz || !h_count || !h_first || (normals && !h_nrm) || (rgb && !h_rgb)) return call_fail(-100, "voxel: no host memory for the result");
    if (cl.number_and_accumulate(d_nrm, d_rgb, out_voxel_of != nullptr) || cl.finish()) return -100;
    CALLCHK(hipMemcpyAsync(h_xyz, cl.out_xyz.p, mv * 12, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(h_count, cl.out_count.p, mv * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(h_first, cl.out_first.p, mv * 4, hipMemcpyDeviceToHost, st));
    if (normals) CALLCHK(hipMemcpyAsync(h_nrm, cl.out_normals.p, mv * 12, hipMemcpyDeviceToHost, st));
    if (rgb) CALLCHK(hipMemcpyAsync(h_rgb, cl.out_rgb.p, mv * 3, hipMemcpyDeviceToHost, st));
    if (out_voxel_of) CALLCHK(hipMemcpyAsync(out_voxel_of, cl.cluster_of.p, np * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float ms[6] = {0, 0, 0, 0, 0, 0};
    if (cl.pass_ms(ms)) return -100;
    std::memcpy(g_voxel_pass_ms, ms, sizeof ms);
    g_voxel_ms = ((ms[0] + ms[1]) + (ms[2] + ms[3])) + (ms[4] + ms[5]);
    *out_xyz = h_xyz, *out_count = h_count, *out_first = h_first;
    if (normals) *out_normals = h_nrm;
    if (rgb) *out_rgb = h_rgb;
    out.keep();
    return cl.count;
}

// ---------------------------------------------------------------------------
// k nearest neighbours within a cloud handle, and the statistical / radius outlier filter on top of them (pm_knn.hpp; DESIGN.md
// section 17).  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
constexpr size_t kKnnChunkEntries = (size_t)1 << 23;   // list entries per launch of the list variant: 2^23 / k queries (2^18 at k = 32), whatever n_q

int mpmvs_cloud_knn(mpmvs_cloud* c, float radius, int k, long long n_q, const float* q_xyz, float* out_d2, int32_t* out_idx, int32_t* out_within) {
    if (!c || !out_d2 || n_q < 0) return call_fail(-2, "cloud knn: bad argument");
    if (k < 1 || k > MPMVS_KNN_MAX_K) return call_fail(-2, "cloud knn: k must lie in [1, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!q_xyz && n_q != c->n) return call_fail(-2, "cloud knn: without query points n_q must be the cloud's own count");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "cloud knn: the radius must be finite and positive");
    if (n_q > INT32_MAX) return call_fail(-3, "cloud knn: more than 2^31 - 1 queries");
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
        CALLCHK(d_q.alloc(nq * 12));
        CALLCHK(hipMemcpyAsync(d_q.p, q_xyz, nq * 12, hipMemcpyHostToDevice, st));
    }
    CALLCHK(d_d2.alloc(chunk * kk * 4));
    if (out_idx) CALLCHK(d_idx.alloc(chunk * kk * 4));
    if (out_within) CALLCHK(d_within.alloc(chunk * 4));
    if (bin) CALLCHK(bins.alloc(chunk));
    const float* d_all = q_xyz ? d_q.as<float>() : c->d_xyz;
    for (size_t i0 = 0; i0 < nq; i0 += chunk) {
        const int cn = (int)std::min(chunk, nq - i0);
        const float* d_qc = d_all + 3 * i0;
        CALLCHK(c->clock.mark(2, st));
        if (bin) {
            const int brc = cloud_bin(st, bins, cn, no_mark, cloud_count_queries(st, d_qc, cn, g));
            if (brc) return brc;
        }
        const long long self_base = q_xyz ? -1ll : (long long)i0;
        const int krc = knn_dispatch(k, [&](auto K) {   // order, idx and within: null where not allocated
            CALLCHK(launch(k_knn_list<K>, dim3((cn + 255) / 256), dim3(256), st, d_qc, cn, bins.order.as<int>(), g, self_base, k, d_d2.as<float>(),
                           d_idx.as<int32_t>(), d_within.as<int32_t>()));
            return 0;
        });
        if (krc) return krc;
        CALLCHK(c->clock.mark(3, st));
        CALLCHK(hipMemcpyAsync(out_d2 + i0 * kk, d_d2.p, (size_t)cn * kk * 4, hipMemcpyDeviceToHost, st));
        if (out_idx) CALLCHK(hipMemcpyAsync(out_idx + i0 * kk, d_idx.p, (size_t)cn * kk * 4, hipMemcpyDeviceToHost, st));
        if (out_within) CALLCHK(hipMemcpyAsync(out_within + i0, d_within.p, (size_t)cn * 4, hipMemcpyDeviceToHost, st));
        CALLCHK(hipStreamSynchronize(st));
        float ms = 0.0f;
        CALLCHK(c->clock.ms(2, 3, &ms));
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
    CALLCHK(d_mean.alloc(n * 4));
    CALLCHK(d_within.alloc(n * 4));
    if (bin) CALLCHK(bins.alloc(n));
    CALLCHK(c->clock.mark(2, st));
    if (bin && (rc = cloud_bin(st, bins, ni, no_mark, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    rc = knn_dispatch(k, [&](auto K) {   // order: null without binning
        CALLCHK(launch(k_knn_reduce<K>, dim3((ni + 255) / 256), dim3(256), st, c->d_xyz, ni, bins.order.as<int>(), g, 0ll, k, d_mean.as<float>(),
                       d_within.as<int32_t>()));
        return 0;
    });
    if (rc) return rc;
    CALLCHK(c->clock.mark(3, st));
    CALLCHK(hipMemcpyAsync(mean, d_mean.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipMemcpyAsync(within, d_within.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float q_ms = 0.0f;
    CALLCHK(c->clock.ms(2, 3, &q_ms));
    *ms = c->query.build_ms + q_ms;
    return 0;
}

long long mpmvs_cloud_outliers(int device, long long n, const float* xyz, float radius, int k, double std_ratio, int min_within, unsigned char* out_keep,
                               float* out_mean, int32_t* out_within, long long counts[3], double stats[3]) {
    if (n < 0 || (n > 0 && (!xyz || !out_keep))) return call_fail(-2, "outliers: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "outliers: the radius must be finite and positive");
    if (k < 1 || k > MPMVS_KNN_MAX_K) return call_fail(-2, "outliers: k must lie in [1, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!(std_ratio >= 0.0)) return call_fail(-2, "outliers: std_ratio must not be negative or NaN");
    if (min_within < 0) return call_fail(-2, "outliers: min_within must not be negative");
    if (n > INT32_MAX) return call_fail(-3, "outliers: more than 2^31 - 1 points");
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
    if (!c || !out_normals) return call_fail(-2, "cloud normals: bad argument");
    if (k < 2 || k > MPMVS_KNN_MAX_K) return call_fail(-2, "cloud normals: k must lie in [2, " + std::to_string(MPMVS_KNN_MAX_K) + "]");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "cloud normals: the radius must be finite and positive");
    if (orient < 0 || orient > 2) return call_fail(-2, "cloud normals: orient must be 0 (canonical), 1 (viewpoint) or 2 (reference normals)");
    if (orient == 1 && !(view && std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2])))
        return call_fail(-2, "cloud normals: orient 1 needs a finite viewpoint");
    if (orient == 2 && !ref_normals) return call_fail(-2, "cloud normals: orient 2 needs reference normals");
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
    CALLCHK(d_n.alloc(n * 12));
    if (out_curvature) CALLCHK(d_curv.alloc(n * 4));
    if (out_within) CALLCHK(d_within.alloc(n * 4));
    if (orient == 2) {
        CALLCHK(d_ref.alloc(n * 12));
        CALLCHK(hipMemcpyAsync(d_ref.p, ref_normals, n * 12, hipMemcpyHostToDevice, st));
    }
    if (bin) CALLCHK(bins.alloc(n));
    CALLCHK(c->clock.mark(2, st));
    if (bin && (rc = cloud_bin(st, bins, ni, no_mark, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    rc = knn_dispatch(k, [&](auto K) {   // order, reference normals, curvature and within: null where not allocated
        CALLCHK(launch(k_knn_normal<K>, dim3((ni + 255) / 256), dim3(256), st, c->d_xyz, ni, bins.order.as<int>(), g, k, orient, v[0], v[1], v[2], d_ref.as<float>(),
                       d_n.as<float>(), d_curv.as<float>(), d_within.as<int32_t>()));
        return 0;
    });
    if (rc) return rc;
    CALLCHK(c->clock.mark(3, st));
    CALLCHK(hipMemcpyAsync(out_normals, d_n.p, n * 12, hipMemcpyDeviceToHost, st));
    if (out_curvature) CALLCHK(hipMemcpyAsync(out_curvature, d_curv.p, n * 4, hipMemcpyDeviceToHost, st));
    if (out_within) CALLCHK(hipMemcpyAsync(out_within, d_within.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(c->clock.ms(2, 3, &c->normals.ms));
    return 0;
}

float mpmvs_cloud_normals_ms(const mpmvs_cloud* c, float* build_ms) { return c ? cloud_op_ms(c->normals, build_ms) : 0.0f; }

// ---------------------------------------------------------------------------
// the connected components of the handle's cloud under "within a radius" (pm_components.hpp): a lock-free
// union-find in one pass over the edges, a flatten pass and a size pass.  The four counts are taken on the host from the downloaded
// labels and sizes.  Errors are reported like those of mpmvs_cloud_*.
// ---------------------------------------------------------------------------
int mpmvs_cloud_components(mpmvs_cloud* c, float radius, int32_t* out_label, int32_t* out_size, long long counts[4]) {
    if (!c || (c->n > 0 && !out_label)) return call_fail(-2, "cloud components: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "cloud components: the radius must be finite and positive");
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
    if (!c->d_cc) CALLCHK(pool_malloc(&c->d_cc, n * 4));
    const hipStream_t st = c->stream;
    const bool bin = cloud_bin_queries(), want_size = out_size || counts;
    const int ni = (int)c->n;
    const dim3 gp((ni + 255) / 256);
    Scratch d_label(st), d_size(st);
    CloudBins bins(st);
    CALLCHK(d_label.alloc(n * 4));
    if (want_size) CALLCHK(d_size.alloc(n * 4));
    if (bin) CALLCHK(bins.alloc(n));
    std::vector<int32_t> size_own;
    if (want_size && !out_size) size_own.resize(n);
    int32_t* size = out_size ? out_size : size_own.data();
    // the grid is built: its two events are free again, and the four borders of the three passes fit the handle's four
    CALLCHK(c->clock.mark(0, st));
    CALLCHK(launch(k_cc_init, gp, dim3(256), st, c->d_xyz, ni, c->d_cc));
    if (bin && (rc = cloud_bin(st, bins, ni, no_mark, cloud_count_queries(st, c->d_xyz, ni, g))) != 0) return rc;
    CALLCHK(launch(k_cc_hook, gp, dim3(256), st, c->d_xyz, ni, bins.order.as<int>(), g, c->d_cc));   // order: null without binning
    CALLCHK(c->clock.mark(1, st));
    CALLCHK(launch(k_cc_flatten, gp, dim3(256), st, ni, c->d_cc, d_label.as<int32_t>()));
    CALLCHK(c->clock.mark(2, st));
    if (want_size) {   // the parents have served: the same ints count the members of every label
        CALLCHK(hipMemsetAsync(c->d_cc, 0, n * 4, st));
        CALLCHK(launch(k_cc_count, gp, dim3(256), st, ni, d_label.as<int32_t>(), c->d_cc));
        CALLCHK(launch(k_cc_gather, gp, dim3(256), st, ni, d_label.as<int32_t>(), c->d_cc, d_size.as<int32_t>()));
    }
    CALLCHK(c->clock.mark(3, st));
    CALLCHK(hipMemcpyAsync(out_label, d_label.p, n * 4, hipMemcpyDeviceToHost, st));
    if (want_size) CALLCHK(hipMemcpyAsync(size, d_size.p, n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    for (int p = 0; p < 3; ++p) CALLCHK(c->clock.ms(p, p + 1, &c->cc_pass_ms[p]));
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
    if (!c || !ms) return call_fail(-2, "cloud components: bad argument");
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
    PassClock<2> clock;   // the borders of a pass
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
    delete h;   // the bins go back to the pool here, and the clock goes
}

static int align_create_device(mpmvs_align* h, const float* s_xyz) {
    const hipStream_t st = h->target->stream;
    CALLCHK(enter_device(h->target->device));
    if (h->n == 0) return 0;
    const size_t n = (size_t)h->n;
    CALLCHK(pool_malloc(&h->d_src, n * 12));
    CALLCHK(h->bins.alloc(n));
    CALLCHK(pool_malloc(&h->d_sums, kAlignPlaneTerms * 8));   // the larger of the two passes' sums
    CALLCHK(hipMemcpyAsync(h->d_src, s_xyz, n * 12, hipMemcpyHostToDevice, st));
    CALLCHK(hipStreamSynchronize(st));
    return 0;
}

int mpmvs_align_create(mpmvs_cloud* target, long long n_s, const float* s_xyz, mpmvs_align** out) {
    if (!out) return call_fail(-2, "align: bad argument");
    *out = nullptr;
    if (!target || n_s < 0 || (n_s > 0 && !s_xyz)) return call_fail(-2, "align: bad argument");
    if (n_s > INT32_MAX) return call_fail(-3, "align: more than 2^31 - 1 source points");
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
    CALLCHK(hipMemsetAsync(h->d_sums, 0, sums_bytes, st));
    if (bin) {   // by the cell of the transformed source
        const int brc = cloud_bin(st, h->bins, n, [&] { return h->clock.mark(0, st); }, [&](dim3 gq, unsigned bin_mask, int* qcnt, int* qbin) {
            return launch(k_align_qbin, gq, dim3(256), st, h->d_src, n, f, g, bin_mask, qcnt, qbin);
        });
        if (brc) return brc;
    } else {
        CALLCHK(h->clock.mark(0, st));
    }
    const dim3 gq(((unsigned)n + 255u) / 256u);   // unsigned: n may be 2^31 - 1
    const int* order = bin ? h->bins.order.as<int>() : nullptr;   // the bins exist either way
    if (plane)
        CALLCHK(launch(k_align_plane_pass, gq, dim3(256), st, h->d_src, n, order, f, g, c->d_xyz, h->d_nrm, h->d_sums));
    else
        CALLCHK(launch(k_align_pass, gq, dim3(256), st, h->d_src, n, order, f, g, c->d_xyz, h->d_sums));
    CALLCHK(h->clock.mark(1, st));
    CALLCHK(hipMemcpyAsync(sums, h->d_sums, sums_bytes, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    CALLCHK(h->clock.ms(0, 1, &h->pass_ms));
    return 0;
}

static bool align_finite12(const double M[12]) {
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(M[k])) return false;
    return true;
}

// a pass of either kind: the checks, the frame, and the cases that launch nothing
static int align_sums_any(mpmvs_align* h, float radius, const double M[12], bool plane, long long* sums, double frame[4]) {
    if (!h || !M || !sums || !frame) return call_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return call_fail(-2, "align: the transform must be finite");
    if (plane && !h->has_nrm) return call_fail(-2, "align: a point-to-plane pass needs mpmvs_align_set_normals first");
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
    if (!h) return call_fail(-2, "align: bad argument");
    mpmvs_cloud* c = h->target;
    CALLCHK(enter_device(c->device));
    CALLCHK(hipStreamSynchronize(c->stream));   // no pass is reading the buffer that goes
    h->has_nrm = false;
    if (h->d_nrm) {
        CALLCHK(pool_free(h->d_nrm));
        h->d_nrm = nullptr;
    }
    if (!nrm) return 0;
    if (c->n > 0) {
        CALLCHK(pool_malloc(&h->d_nrm, (size_t)c->n * 12));
        CALLCHK(hipMemcpyAsync(h->d_nrm, nrm, (size_t)c->n * 12, hipMemcpyHostToDevice, c->stream));
        CALLCHK(hipStreamSynchronize(c->stream));
    }
    h->has_nrm = true;
    return 0;
}

int mpmvs_align_plane_sums(mpmvs_align* h, float radius, const double M[12], long long sums[38], double frame[4]) {
    return align_sums_any(h, radius, M, true, sums, frame);
}

int mpmvs_align_plane_solve(const long long sums[38], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse_plane,
                            double* rmse_point) {
    if (!sums || !frame || !M_in || !M_out) return call_fail(-2, "align: bad argument");
    return align_plane_solve(sums, frame, with_scale, M_in, M_out, rmse_plane, rmse_point);
}

int mpmvs_align_plane_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M[12], long long* iters, long long* inliers,
                          double* rmse_plane, double* rmse_point) {
    if (!h || !M) return call_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return call_fail(-2, "align: the transform must be finite");
    if (max_iter < 1) return call_fail(-2, "align: max_iter must be at least 1");
    if (!(eps >= 0.0)) return call_fail(-2, "align: eps must not be negative");
    if (!h->has_nrm) return call_fail(-2, "align: point-to-plane ICP needs mpmvs_align_set_normals first");
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
    if (!sums || !frame || !M_in || !M_out) return call_fail(-2, "align: bad argument");
    return align_solve(sums, frame, with_scale, M_in, M_out, rmse);
}

int mpmvs_align_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M[12], long long* iters, long long* inliers, double* rmse) {
    if (!h || !M) return call_fail(-2, "align: bad argument");
    if (!cloud_radius_ok(radius)) return call_fail(-2, "align: the radius must be finite and positive");
    if (!align_finite12(M)) return call_fail(-2, "align: the transform must be finite");
    if (max_iter < 1) return call_fail(-2, "align: max_iter must be at least 1");
    if (!(eps >= 0.0)) return call_fail(-2, "align: eps must not be negative");
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
    CALLCHK(d_zc.alloc(total * 4));
    CALLCHK(d_depth.alloc(total * 4));
    if (any_idx) CALLCHK(d_idx.alloc(total * 4));
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
    CALLCHK(hipMemsetD32Async((hipDeviceptr_t)d_zc.p, (int)kRenderInfBits, total, st));
    if (any_idx) CALLCHK(hipMemsetAsync(d_idx.p, 0xff, total * 4, st));
    const int n = (int)c->n;
    const dim3 gp((n + 255) / 256);
    CALLCHK(c->clock.mark(0, st));
    CALLCHK(launch(k_render_zmin, gp, dim3(256), st, c->d_xyz, n, A));
    CALLCHK(c->clock.mark(1, st));
    if (any_idx) CALLCHK(launch(k_render_index, gp, dim3(256), st, c->d_xyz, n, A));
    CALLCHK(c->clock.mark(2, st));
    at = 0;
    for (int k = 0; k < A.n; ++k) {
        const RenderView& V = A.v[k];
        const size_t npix = (size_t)V.w * (size_t)V.h;
        CALLCHK(launch(k_render_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), st, V.zc, V.w, V.h, splat, m, d_depth.as<float>() + at, V.idx));
        at += npix;
    }
    CALLCHK(c->clock.mark(3, st));
    at = 0;
    for (int k = 0; k < A.n; ++k) {
        const RenderView& V = A.v[k];
        const size_t npix = (size_t)V.w * (size_t)V.h;
        CALLCHK(hipMemcpyAsync(out_depth[v0 + k], d_depth.as<float>() + at, npix * 4, hipMemcpyDeviceToHost, st));
        if (V.idx) CALLCHK(hipMemcpyAsync(out_idx[v0 + k], V.idx, npix * 4, hipMemcpyDeviceToHost, st));
        at += npix;
    }
    CALLCHK(hipStreamSynchronize(st));
    for (int p = 0; p < 3; ++p) {
        if (p == 1 && !any_idx) continue;   // no index pass: the gap between two event records is not its time
        float ms = 0.0f;
        CALLCHK(c->clock.ms(p, p + 1, &ms));
        c->render_pass_ms[p] += ms;
    }
    return 0;
}

int mpmvs_cloud_render_depth(mpmvs_cloud* c, int n_views, const mpmvs_camera* cams, int splat, float occl_rel, float* const* out_depth, int32_t* const* out_idx) {
    if (!c || n_views < 0) return call_fail(-2, "cloud render: bad argument");
    if (splat < 0 || splat > MPMVS_RENDER_MAX_SPLAT) return call_fail(-2, "cloud render: splat must lie in [0, " + std::to_string(MPMVS_RENDER_MAX_SPLAT) + "]");
    if (!std::isfinite(occl_rel) || !(occl_rel >= 0.0f)) return call_fail(-2, "cloud render: occl_rel must be finite and not negative");
    if (n_views == 0) return 0;
    if (!cams || !out_depth) return call_fail(-2, "cloud render: bad argument");
    for (int v = 0; v < n_views; ++v) {
        if (!out_depth[v]) return call_fail(-2, "cloud render: view " + std::to_string(v) + " has no depth buffer");
        if (cams[v].width <= 0 || cams[v].height <= 0) return call_fail(-2, "cloud render: view " + std::to_string(v) + " has a non-positive width or height");
    }
    for (int v = 0; v < n_views; ++v) {
        if (cams[v].width > (1 << 24) || cams[v].height > (1 << 24)) return call_fail(-3, "cloud render: view " + std::to_string(v) + " is wider or higher than 2^24");
        if ((long long)cams[v].width * (long long)cams[v].height > (long long)INT32_MAX)
            return call_fail(-3, "cloud render: view " + std::to_string(v) + " has more than 2^31 - 1 pixels");
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
    CALLCHK(enter_device(c->device));
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
    if (!c || !ms) return call_fail(-2, "cloud render: bad argument");
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
    PassClock<3> clock;                               // the borders of the two passes of a chunk; marks 0 and 1: of a classify launch
    ObserveScanners sc;                               // all scanners, j0 = 0
    int R = 0, w = 0;
    float* d_zn = nullptr;                            // [n_scanners][6][R][R]
    long long stats[2] = {0, 0};
    float build_pass_ms[2] = {0.0f, 0.0f}, classify_ms = 0.0f;
};

static void observer_release(mpmvs_observer* h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_zn) (void)pool_free(h->d_zn);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // the clock goes here: the stream has been waited for
}

// the device half of mpmvs_observer_create: Zc and Zn of one chunk of scanners after the other; the scan's points are read in place
static int observer_create_device(mpmvs_observer* h, const mpmvs_cloud* scan, const int* owner) {
    CALLCHK(enter_device(scan->device));
    CALLCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const hipStream_t st = h->stream;
    const size_t map = (size_t)6 * (size_t)h->R * (size_t)h->R, total = map * (size_t)h->sc.n;
    CALLCHK(pool_malloc(&h->d_zn, total * 4));
    if (scan->n_fin == 0) {   // nothing lands anywhere
        CALLCHK(hipMemsetD32Async((hipDeviceptr_t)h->d_zn, (int)kRenderInfBits, total, st));
        CALLCHK(hipStreamSynchronize(st));
        return 0;
    }
    const int per = (int)std::min<size_t>((size_t)kObserveChunk, std::max<size_t>(1, kObserveChunkPixels / map));
    const int n = (int)scan->n;
    Scratch d_zc(st), d_owner(st), d_cnt(st);
    CALLCHK(d_zc.alloc(map * (size_t)std::min(per, h->sc.n) * 4));
    CALLCHK(d_cnt.alloc(8));
    CALLCHK(hipMemsetAsync(d_cnt.p, 0, 8, st));
    if (owner) {
        CALLCHK(d_owner.alloc((size_t)n * 4));
        CALLCHK(hipMemcpyAsync(d_owner.p, owner, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    for (int j0 = 0; j0 < h->sc.n; j0 += per) {
        ObserveScanners A = h->sc;
        A.j0 = j0, A.n = std::min(per, h->sc.n - j0);
        const size_t n_pix = map * (size_t)A.n;
        CALLCHK(hipMemsetD32Async((hipDeviceptr_t)d_zc.p, (int)kRenderInfBits, n_pix, st));
        CALLCHK(h->clock.mark(0, st));
        CALLCHK(launch(k_observe_zmin, dim3(((unsigned)n + 255u) / 256u), dim3(256), st, scan->d_xyz, n, d_owner.as<int>(), A, h->R, d_zc.as<uint32_t>()));   // owner: null if not given
        CALLCHK(h->clock.mark(1, st));
        CALLCHK(launch(k_observe_near, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), st, d_zc.as<uint32_t>(), n_pix, h->R, h->w, h->d_zn + map * (size_t)j0,
                       d_cnt.as<unsigned long long>()));
        CALLCHK(h->clock.mark(2, st));
        CALLCHK(hipStreamSynchronize(st));
        for (int p = 0; p < 2; ++p) {
            float ms = 0.0f;
            CALLCHK(h->clock.ms(p, p + 1, &ms));
            h->build_pass_ms[p] += ms;
        }
    }
    unsigned long long covered = 0;
    CALLCHK(hipMemcpyAsync(&covered, d_cnt.p, 8, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    h->stats[0] = (long long)covered;
    return 0;
}

int mpmvs_observer_create(mpmvs_cloud* scan, int n_scanners, const float* scanners_xyz, const int* owner, int face_size, int window, mpmvs_observer** out) {
    if (!out) return call_fail(-2, "observer: bad argument");
    *out = nullptr;
    if (!scanners_xyz) return call_fail(-2, "observer: bad argument");
    if (n_scanners < 1 || n_scanners > MPMVS_OBSERVE_MAX_SCANNERS)
        return call_fail(-2, "observer: the number of scanners must lie in [1, " + std::to_string(MPMVS_OBSERVE_MAX_SCANNERS) + "]");
    for (int k = 0; k < 3 * n_scanners; ++k)
        if (!std::isfinite(scanners_xyz[k])) return call_fail(-2, "observer: scanner " + std::to_string(k / 3) + " has a non-finite coordinate");
    if (face_size < 1 || face_size > MPMVS_OBSERVE_MAX_FACE) return call_fail(-2, "observer: face_size must lie in [1, " + std::to_string(MPMVS_OBSERVE_MAX_FACE) + "]");
    if (window < 0 || window > MPMVS_OBSERVE_MAX_WINDOW) return call_fail(-2, "observer: window must lie in [0, " + std::to_string(MPMVS_OBSERVE_MAX_WINDOW) + "]");
    if ((long long)n_scanners * 6 * face_size * face_size > (1ll << 31)) return call_fail(-3, "observer: more than 2^31 pixels (scanners x 6 x face_size^2)");
    if (!scan) return call_fail(-2, "observer: no scan");   // after the checks that need none
    for (long long i = 0; owner && i < scan->n; ++i)
        if (owner[i] < -1 || owner[i] >= n_scanners)
            return call_fail(-2, "observer: owner[" + std::to_string(i) + "] = " + std::to_string(owner[i]) + " is neither -1 nor a scanner");
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
    CALLCHK(d_q.alloc((size_t)n * 12));
    CALLCHK(d_free.alloc((size_t)n * 4));
    if (out_covered) CALLCHK(d_cov.alloc((size_t)n * 4));
    CALLCHK(hipMemcpyAsync(d_q.p, q_xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
    CALLCHK(h->clock.mark(0, st));
    CALLCHK(launch(k_observe_classify, dim3(((unsigned)n + 255u) / 256u), dim3(256), st, d_q.as<float>(), n, h->sc, h->R, h->d_zn, m1, abs_margin, d_free.as<int>(),
                   d_cov.as<int>()));   // covered: null if not wanted
    CALLCHK(h->clock.mark(1, st));
    CALLCHK(hipMemcpyAsync(out_free, d_free.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (out_covered) CALLCHK(hipMemcpyAsync(out_covered, d_cov.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CALLCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    CALLCHK(h->clock.ms(0, 1, &ms));
    h->classify_ms += ms;
    return 0;
}

int mpmvs_observer_classify(mpmvs_observer* h, long long n_q, const float* q_xyz, float rel, float abs_margin, int* out_free, int* out_covered) {
    if (!std::isfinite(rel) || !(rel >= 0.0f && rel < 1.0f)) return call_fail(-2, "observer: rel must lie in [0, 1)");
    if (!std::isfinite(abs_margin) || !(abs_margin >= 0.0f)) return call_fail(-2, "observer: abs_margin must be finite and not negative");
    if (n_q < 0 || !out_free || (n_q > 0 && !q_xyz)) return call_fail(-2, "observer: bad argument");
    if (n_q > INT32_MAX) return call_fail(-3, "observer: more than 2^31 - 1 queries");
    if (!h) return call_fail(-2, "observer: no handle");   // after the checks that need none
    h->classify_ms = 0.0f;
    if (n_q == 0) return 0;
    CALLCHK(enter_device(h->device));
    const float m1 = 1.0f - rel;
    for (long long q0 = 0; q0 < n_q; q0 += kObserveChunkQueries) {
        const int n = (int)std::min(kObserveChunkQueries, n_q - q0);
        const int rc = observer_classify_chunk(h, n, q_xyz + 3 * q0, m1, abs_margin, out_free + q0, out_covered ? out_covered + q0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

int mpmvs_observer_maps(mpmvs_observer* h, int scanner, float* out_near) {
    if (!h || !out_near) return call_fail(-2, "observer: bad argument");
    if (scanner < 0 || scanner >= h->sc.n) return call_fail(-2, "observer: no scanner " + std::to_string(scanner));
    CALLCHK(enter_device(h->device));
    const size_t map = (size_t)6 * (size_t)h->R * (size_t)h->R;
    CALLCHK(hipMemcpyAsync(out_near, h->d_zn + map * (size_t)scanner, map * 4, hipMemcpyDeviceToHost, h->stream));
    CALLCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int mpmvs_observer_stats(mpmvs_observer* h, long long out[2]) {
    if (!h || !out) return call_fail(-2, "observer: bad argument");
    out[0] = h->stats[0], out[1] = h->stats[1];
    return 0;
}

float mpmvs_observer_ms(mpmvs_observer* h, float build_ms[2]) {
    if (!h) return 0.0f;
    if (build_ms) build_ms[0] = h->build_pass_ms[0], build_ms[1] = h->build_pass_ms[1];
    return h->classify_ms;
}

}  // extern "C"
