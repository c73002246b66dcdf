// mpmvs_fusion.hip -- depth-map fusion of the C ABI declared in include/mpmvs.h: FuseRun, on the request and rules of
// pm_fusion_host.hpp and the kernels of pm_fusion.hpp, and the mpmvs_fuse* entry points.  A PatchMatch context is an opaque
// pointer here: what a resident image needs of it comes from ctx_resident_planes (pm_host.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_fusion.hpp"
#include "pm_tracks_host.hpp"
#include "pm_fusion_host.hpp"

using namespace pm;

extern "C" {

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
        int cx_device = 0;
        hipStream_t cx_stream = nullptr;
        const float4* planes = nullptr;
        if (const int rc = ctx_resident_planes(cx, hv[i].w, hv[i].h, &cx_device, &cx_stream, &planes)) return rc;   // -2: no finished Run() of that size behind it
        if (cx_device == q.device) {
            FUSECHK(hipStreamSynchronize(cx_stream));
        } else {
            // another GPU of the node: its stream is drained there, the planes cross xGMI into a scratch buffer here
            float4* tmp = call.alloc_n<float4>(wh);
            if (!tmp || hipSetDevice(cx_device) != hipSuccess || hipStreamSynchronize(cx_stream) != hipSuccess || hipSetDevice(q.device) != hipSuccess ||
                hipMemcpyPeerAsync(tmp, q.device, planes, cx_device, wh * 16, st) != hipSuccess) {
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

}  // extern "C"
