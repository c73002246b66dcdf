// PatchMatchHost.cpp -- the host half of PatchMatchCUDA and ProcessProblem()
// (reference src/PatchMatch.cpp:506-721, :855-1139) re-pointed at the C ABI of
// include/mpmvs.h.  Error convention of the reference is kept here: print and
// exit(EXIT_FAILURE) (reference src/PatchMatch.cpp:60-65); the C ABI underneath
// never exits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>

#include "PatchMatch.h"

// cv::resize(src, dst, Size(new_cols, new_rows), 0, 0, INTER_LINEAR) for a 1-channel fp32
// image: sample position (x + 0.5) * (src/dst) - 0.5, edge texels replicated.
// OpenCV is absent here, so this follows its documented geometry; the last-bit
// behaviour of its SIMD kernels is "parity unpinned" (SURVEY 8c).
Image ResizeLinear(const Image& src, int new_cols, int new_rows) {
    Image dst(new_rows, new_cols, 1);
    const float sx = (float)src.cols / new_cols, sy = (float)src.rows / new_rows;
    for (int y = 0; y < new_rows; ++y) {
        float fy = (y + 0.5f) * sy - 0.5f;
        int y0 = (int)std::floor(fy);
        float ay = fy - y0;
        if (y0 < 0) { y0 = 0; ay = 0.0f; }
        if (y0 >= src.rows - 1) { y0 = src.rows - 1; ay = 0.0f; }
        const int y1 = std::min(y0 + 1, src.rows - 1);
        for (int x = 0; x < new_cols; ++x) {
            float fx = (x + 0.5f) * sx - 0.5f;
            int x0 = (int)std::floor(fx);
            float ax = fx - x0;
            if (x0 < 0) { x0 = 0; ax = 0.0f; }
            if (x0 >= src.cols - 1) { x0 = src.cols - 1; ax = 0.0f; }
            const int x1 = std::min(x0 + 1, src.cols - 1);
            const float top = src.at(y0, x0) + ax * (src.at(y0, x1) - src.at(y0, x0));
            const float bot = src.at(y1, x0) + ax * (src.at(y1, x1) - src.at(y1, x0));
            dst.at(y, x) = top + ay * (bot - top);
        }
    }
    return dst;
}

// ---------------------------------------------------------------------------
// Problem contexts kept resident between passes.  A cached context is only adopted when device, view list (image buffers
// and sizes) and cameras are the ones it was filled from.  MPMVS_CTX_CACHE_MB (default 65536, 0 = off) bounds the HBM held
// this way; beyond it Release() destroys the context as the reference does.
// ---------------------------------------------------------------------------
#include <atomic>
#include <mutex>
struct ProblemDeviceCache {
    mpmvs_ctx* ctx = nullptr;
    int device = -1;
    std::vector<const void*> image_data;   // the fp32 or byte buffers of the views it was filled from
    std::vector<Camera> cameras;
    uint64_t state_stamp = 0;            // Image::stamp of the maps whose state (planes, costs) the context holds
    std::vector<uint64_t> depth_stamps;  // ... of the source depth maps it holds
    size_t bytes = 0;
    static std::atomic<size_t>& held() {
        static std::atomic<size_t> h(0);
        return h;
    }
    ~ProblemDeviceCache() {
        if (ctx) {
            mpmvs_destroy(ctx);
            held() -= bytes;
        }
    }
};
static size_t ctx_cache_cap() {
    static const size_t cap = [] {
        const char* e = std::getenv("MPMVS_CTX_CACHE_MB");
        return (size_t)(e ? std::strtoull(e, nullptr, 10) : 65536ull) << 20;
    }();
    return cap;
}
// the free lists behind DefaultInitAllocator (PatchMatch.h): exact-size LIFO lists of blocks of at least 1 MB
namespace {
struct BigBlockPool {
    std::mutex mu;
    std::unordered_map<size_t, std::vector<void*>> free_lists;
    size_t cached = 0;
    const size_t cap = [] {
        const char* e = std::getenv("MPMVS_HOST_POOL_MB");
        return (size_t)(e ? std::strtoull(e, nullptr, 10) : 1024ull) << 20;
    }();
};
BigBlockPool& big_pool() {
    static BigBlockPool& p = *new BigBlockPool;   // leaked on purpose: images may be destroyed after static destructors have run
    return p;
}
constexpr size_t kBigBlock = 1u << 20;
}  // namespace
void* PooledAllocate(size_t bytes) {
    if (bytes >= kBigBlock) {
        BigBlockPool& P = big_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.free_lists.find(bytes);
        if (it != P.free_lists.end() && !it->second.empty()) {
            void* p = it->second.back();
            it->second.pop_back();
            P.cached -= bytes;
            return p;
        }
    }
    return ::operator new(bytes);
}
void PooledRelease(void* p, size_t bytes) noexcept {
    if (!p) return;
    if (bytes >= kBigBlock) {
        BigBlockPool& P = big_pool();
        std::lock_guard<std::mutex> lk(P.mu);
        if (P.cached + bytes <= P.cap) {
            try {
                P.free_lists[bytes].push_back(p);
                P.cached += bytes;
                return;
            } catch (...) {
            }
        }
    }
    ::operator delete(p);
}

uint64_t NewImageStamp() {
    static std::atomic<uint64_t> next(1);
    return next.fetch_add(1);
}
void Image::Seal() { SealAs(NewImageStamp()); }
void Image::SealAs(uint64_t s) {
    stamp = s;
    sealed_fingerprint = Fingerprint();
}
// FNV-1a over the bit patterns of up to 4096 evenly strided samples, the first and the last element and the shape
uint64_t Image::Fingerprint() const {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) {
        h ^= v;
        h *= 1099511628211ull;
    };
    mix((uint64_t)rows);
    mix((uint64_t)cols);
    mix((uint64_t)ch);
    const size_t n = data.size();
    if (n == 0) return h;
    const size_t step = n > 4096 ? n / 4096 : 1;
    for (size_t i = 0; i < n; i += step) {
        uint32_t b;
        std::memcpy(&b, &data[i], 4);
        mix(b);
    }
    uint32_t b;
    std::memcpy(&b, &data[n - 1], 4);
    mix(b);
    return h;
}
// MPMVS_PEER_COPY=0: a source depth map that lies in the HBM of ANOTHER device of the process is uploaded from the host copy instead of
// copied GPU to GPU (hipMemcpyPeerAsync) -- the switch for a node whose peer path misbehaves; that branch has not run on two GPUs
// anywhere yet (bench.py --gpus N verifies it once per rank).  Same results either way.
static bool peer_copies_allowed() {
    static const bool on = [] {
        const char* e = std::getenv("MPMVS_PEER_COPY");
        return !(e && std::atoi(e) == 0);
    }();
    return on;
}
void ReleaseDeviceCaches(std::vector<Scene>& Scenes) {
    for (Scene& s : Scenes) s.device_cache.reset();
}
mpmvs_ctx* ResidentResultContext(const Scene& s, int consumer_device) {
    const ProblemDeviceCache* c = s.device_cache.get();
    if (!c || !c->ctx || c->state_stamp == 0) return nullptr;
    if (consumer_device >= 0 && c->device != consumer_device && !peer_copies_allowed()) return nullptr;   // MPMVS_PEER_COPY=0: through the host
    if (s.depth.stamp != c->state_stamp || s.normal.stamp != c->state_stamp || !s.depth.StillSealed() || !s.normal.StillSealed()) return nullptr;
    return c->ctx;
}

void PatchMatchCUDA::ExportDepthDevice(float* d_out) { check(mpmvs_export_depth_device(ctx, d_out), "mpmvs_export_depth_device"); }

void PatchMatchCUDA::check(int rc, const char* what) {
    if (rc != 0) {
        std::cerr << what << " failed (" << rc << "): " << mpmvs_last_error(ctx) << std::endl;
        exit(EXIT_FAILURE);
    }
}

PatchMatchCUDA::~PatchMatchCUDA() {
    if (ctx) mpmvs_destroy(ctx);
    ctx = nullptr;
}

// reference src/PatchMatch.cpp:655-665
void PatchMatchCUDA::SetGeomConsistencyParams(bool geom_consistency, bool planar_prior) {
    params.geom_consistency = geom_consistency;
    if (geom_consistency) {
        params.max_iterations = 2;
        params.geomPlanarPrior = planar_prior;
    } else {
        params.max_iterations = 3;
    }
}
// reference src/PatchMatch.cpp:667-670
void PatchMatchCUDA::SetPlanarPriorParams() { params.planar_prior = true; }
void PatchMatchCUDA::SetFolder(const std::string& in, const std::string& out) {
    input_folder = in;
    output_folder = out;
}

// reference src/PatchMatch.cpp:863-958, minus file reading and rescaling
// MPMVS_HOST_TIMING=1: wall time of every stage of ProcessProblem on stderr
struct StageTimer {
    const bool on = std::getenv("MPMVS_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mpmvs_host] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

void AdjustImageScale(Scene& s) {
    const int max_image_size = s.max_image_size;
    const bool bytes = !s.image8.empty();
    if (bytes && s.target_cols) return;   // done before: target size and K are a cached pair
    const int cols = bytes ? s.image8.cols : s.image.cols, rows = bytes ? s.image8.rows : s.image.rows;
    if (bytes) {
        s.target_cols = cols;
        s.target_rows = rows;
    }
    if (!s.has_image() || (cols <= max_image_size && rows <= max_image_size)) return;
    const float factor_x = static_cast<float>(max_image_size) / cols;
    const float factor_y = static_cast<float>(max_image_size) / rows;
    const float factor = std::min(factor_x, factor_y);
    const int new_cols = (int)std::round(cols * factor);
    const int new_rows = (int)std::round(rows * factor);
    const float scale_x = new_cols / static_cast<float>(cols);
    const float scale_y = new_rows / static_cast<float>(rows);
    if (bytes) {   // resampled on the device (mpmvs_set_views_u8)
        s.target_cols = new_cols;
        s.target_rows = new_rows;
    } else {
        s.image = ResizeLinear(s.image, new_cols, new_rows);
    }
    s.cam.K[0] *= scale_x;
    s.cam.K[2] *= scale_x;
    s.cam.K[4] *= scale_y;
    s.cam.K[5] *= scale_y;
}

void PatchMatchCUDA::PatchMatchInit(std::vector<Scene>& Scenes, const int ID) {
    ref_scene = &Scenes[ID];
    images.clear();
    images8.clear();
    depths.clear();
    depth_slots.clear();
    cameras.clear();
    std::vector<int>& srcID = Scenes[ID].srcID;
    num_img = (int)srcID.size();
    // Adjust image scale (reference src/PatchMatch.cpp:893-925): images larger than max_image_size are shrunk with bilinear
    // interpolation and K follows.  The reference re-reads and re-shrinks the files on every call; here the Scene caches the
    // shrunk image, so the scaled intrinsics are cached with it (s.cam) -- a later call finds a consistent pair.
    for (int i = 0; i < num_img; ++i) {
        Scene& s = Scenes[srcID[i]];
        if (!s.has_image()) {
            std::cout << "Can not read this image !" << srcID[i] << std::endl;
            exit(EXIT_FAILURE);
        }
        AdjustImageScale(s);
    }
    int n_bytes = 0;
    for (int i = 0; i < num_img; ++i) {
        Scene& s = Scenes[srcID[i]];
        images.push_back(&s.image);
        n_bytes += s.image8.empty() ? 0 : 1;
        Camera cam = s.cam;
        cam.height = s.rows();
        cam.width = s.cols();
        cameras.push_back(cam);
    }
    if (n_bytes != 0 && n_bytes != num_img) {   // (no shipped path mixes them: a folder gives bytes, a caller's arrays are fp32)
        std::cout << "The views of a Problem must all be 8-bit or all be fp32 images !" << std::endl;
        exit(EXIT_FAILURE);
    }
    if (n_bytes)
        for (int i = 0; i < num_img; ++i) images8.push_back(&Scenes[srcID[i]].image8);
    params.depth_min = cameras[0].depth_min * 0.6f;  // reference :929-930
    params.depth_max = cameras[0].depth_max * 1.2f;
    params.num_images = num_img;
    if (params.geom_consistency) {
        for (int i = 1; i < num_img; ++i) {
            const Scene& s = Scenes[srcID[i]];
            if (s.depth.empty()) {
                std::cout << "Can not read this depth image !" << std::endl;
                exit(EXIT_FAILURE);
            }
            depths.push_back(&s.depth);
            depth_slots.push_back(&s.device_depth);
        }
    }
}

// reference src/PatchMatch.cpp:960-976
void PatchMatchCUDA::AllocatePatchMatch() {
    const size_t wh = (size_t)cameras[0].width * cameras[0].height;
    views_resident = false;
    if (!ctx && ref_scene && ref_scene->device_cache) {
        // adopt the context a previous pass left for this Problem, if it was filled from the same views
        std::shared_ptr<ProblemDeviceCache> cached = std::move(ref_scene->device_cache);
        ref_scene->device_cache.reset();
        bool same = cached->ctx && cached->device == device && cached->image_data.size() == images.size() &&
                    std::memcmp(cached->cameras.data(), cameras.data(), cameras.size() * sizeof(Camera)) == 0;
        for (size_t i = 0; same && i < images.size(); ++i) same = cached->image_data[i] == ViewBuffer(i);
        if (same) {
            ctx = cached->ctx;
            cached->ctx = nullptr;
            ProblemDeviceCache::held() -= cached->bytes;
            views_resident = true;
            resident_state_stamp = cached->state_stamp;
            resident_depth_stamps = cached->depth_stamps;
        }
    }
    if (!views_resident) {
        resident_state_stamp = 0;
        resident_depth_stamps.clear();
    }
    if (!ctx) ctx = mpmvs_create(device);
    if (!ctx) {
        std::cerr << "mpmvs_create failed: " << mpmvs_last_error(nullptr) << std::endl;
        exit(EXIT_FAILURE);
    }
    // not zero-filled (the reference's new[] is not either): Run() and CudaMemInit write them in full before anything reads
    hostPlaneHypotheses.allocate(wh);
    hostCosts.allocate(wh);
    if (params.geom_consistency) {
        hostGeomCosts.allocate(wh);
        // Run() fills it only when params.geomPlanarPrior is set (ref .cu:1248): otherwise GetGeomCost() would hand out whatever
        // the recycled page-locked block held before (the reference returns uninitialised new[] memory there): zeros instead
        if (!params.geomPlanarPrior) std::memset(hostGeomCosts.data(), 0, wh * sizeof(float));
    }
}

// reference src/PatchMatch.cpp:998-1089
void PatchMatchCUDA::CudaMemInit(Scene& scene) {
    if (!views_resident && !images8.empty()) {
        // Scenes read from a folder: the bytes the files decoded to, at the files' size; the device shrinks what is oversized
        std::vector<const unsigned char*> ptrs;
        std::vector<int> ws, hs;
        for (const Image8* im : images8) {
            ptrs.push_back(im->data.data());
            ws.push_back(im->cols);
            hs.push_back(im->rows);
        }
        check(mpmvs_set_views_u8(ctx, num_img, cameras.data(), ptrs.data(), ws.data(), hs.data(), nullptr), "mpmvs_set_views_u8");
    } else if (!views_resident) {
        std::vector<const float*> ptrs;
        std::vector<size_t> pitches;
        for (int i = 0; i < num_img; ++i) {
            ptrs.push_back(images[i]->data.data());
            pitches.push_back((size_t)images[i]->cols * sizeof(float));
        }
        check(mpmvs_set_views(ctx, num_img, cameras.data(), ptrs.data(), pitches.data()), "mpmvs_set_views");
    }
    host_state_valid = false;
    if (params.geom_consistency) {
        std::vector<const float*> dptr;
        std::vector<int> ws, hs;
        for (const Image* dp : depths) {
            const Image& d = *dp;
            dptr.push_back(d.data.data());
            ws.push_back(d.cols);
            hs.push_back(d.rows);
        }
        // a source depth map the adopted context already holds (same sealed contents, Image::stamp) is not uploaded again:
        // NULL keeps it (include/mpmvs.h).  The reference uploads all of them on every call (:1027-1050).  A map that also lies in
        // HBM with the same stamp (Scene::device_depth: the pass schedule exported it there) is copied from there -- device to
        // device, or GPU to GPU when its Problem runs on another device -- instead of crossing PCIe.
        if (resident_depth_stamps.size() != depths.size()) resident_depth_stamps.assign(depths.size(), 0);
        std::vector<const float*> dev_ptr(depths.size(), nullptr);
        std::vector<int> dev_of(depths.size(), device);
        bool any = false;
        for (size_t i = 0; i < depths.size(); ++i) {
            const Scene::DeviceDepth& slot = *depth_slots[i];
            if (depths[i]->stamp != 0 && depths[i]->stamp == resident_depth_stamps[i] && depths[i]->StillSealed()) {
                dptr[i] = nullptr;
            } else if (slot.ptr && slot.stamp != 0 && slot.stamp == depths[i]->stamp && depths[i]->StillSealed() && (slot.device == device || peer_copies_allowed())) {
                dptr[i] = nullptr;
                dev_ptr[i] = slot.ptr;
                dev_of[i] = slot.device;
                any = true;
            } else {
                any = true;
            }
            resident_depth_stamps[i] = depths[i]->stamp;
        }
        if (any)
            check(mpmvs_set_src_depths_mixed(ctx, num_img - 1, dptr.data(), dev_ptr.data(), dev_of.data(), ws.data(), hs.data()), "mpmvs_set_src_depths_mixed");
        // previous result of this image is the start state (reference :1052-1086)
        if (scene.depth.empty() || scene.normal.empty() || scene.cost.empty()) {
            std::cout << "Can not read this depth image !" << std::endl;
            exit(0);
        }
        // ... unless the adopted context still holds exactly that state: the maps carry the stamp ProcessProblem gave its
        // results when it left the context behind
        const bool state_resident = resident_state_stamp != 0 && scene.depth.stamp == resident_state_stamp &&
                                    scene.normal.stamp == resident_state_stamp && scene.cost.stamp == resident_state_stamp &&
                                    scene.depth.StillSealed() && scene.normal.StillSealed() && scene.cost.StillSealed();
        if (!state_resident) {
            const Image &sn = scene.normal, &sd = scene.depth, &sc = scene.cost;
            const int width = sd.cols, height = sd.rows;
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
            for (int row = 0; row < height; ++row)
                for (int col = 0; col < width; ++col) {
                    const size_t idx = (size_t)row * width + col;
                    hostPlaneHypotheses[idx] = float4{sn.at(row, col, 0), sn.at(row, col, 1), sn.at(row, col, 2), sd.at(row, col)};
                    hostCosts[idx] = sc.at(row, col);
                }
            check(mpmvs_set_state(ctx, hostPlaneHypotheses.data(), hostCosts.data()), "mpmvs_set_state");
        }
    }
    resident_state_stamp = 0;  // Run() changes the state; ProcessProblem notes the stamp of its results afterwards
}

// reference src/PatchMatch.cpp:978-996
void PatchMatchCUDA::CudaPlanarPriorInitialization(const std::vector<float4>& PlaneParams, const Image& masks) {
    const int W = cameras[0].width, H = cameras[0].height;
    StageTimer tm;
    hostPriorPlanes.allocate((size_t)W * H);
    hostPlaneMask.allocate((size_t)W * H);
    tm.lap("  prior: resize");
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const size_t idx = (size_t)i * W + j;
            const float m = masks.at(i, j);
            hostPlaneMask[idx] = (unsigned int)m;
            hostPriorPlanes[idx] = m > 0 ? PlaneParams[(size_t)m - 1] : float4{0, 0, 0, 0};
        }
    tm.lap("  prior: expand");
    check(mpmvs_set_prior(ctx, hostPriorPlanes.data(), hostPlaneMask.data()), "mpmvs_set_prior");
    tm.lap("  prior: mpmvs_set_prior");
}

// reference src/PatchMatch.cpp:554-595 + :978-996 on the device
void PatchMatchCUDA::CudaPlanarPriorInitialization(const std::vector<Triangle>& triangles) {
    static_assert(sizeof(Triangle) == 6 * sizeof(int), "a Triangle is six ints: x1 y1 x2 y2 x3 y3");
    const Rect imageRC{0, 0, cameras[0].width, cameras[0].height};
    // reference :555 keeps the triangles whose three vertices lie inside the image.  A triangulation of the image's own
    // vertices has no others, so the list normally goes to the device as it stands (no copy); the filtered copy is the
    // fallback for a caller's own triangle list
    const size_t n = triangles.size();
    bool all_inside = true;
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static) reduction(&& : all_inside)
    for (long i = 0; i < (long)n; ++i) {
        const Triangle& t = triangles[(size_t)i];
        all_inside = all_inside && imageRC.contains(t.pt1) && imageRC.contains(t.pt2) && imageRC.contains(t.pt3);
    }
    if (all_inside) {
        check(mpmvs_prior_from_triangles(ctx, &params, reinterpret_cast<const int*>(triangles.data()), (int)n), "mpmvs_prior_from_triangles");
        return;
    }
    std::vector<int> tri_xy;
    tri_xy.reserve(n * 6);
    for (const Triangle& t : triangles)
        if (imageRC.contains(t.pt1) && imageRC.contains(t.pt2) && imageRC.contains(t.pt3)) {
            const int v[6] = {t.pt1.x, t.pt1.y, t.pt2.x, t.pt2.y, t.pt3.x, t.pt3.y};
            tri_xy.insert(tri_xy.end(), v, v + 6);
        }
    check(mpmvs_prior_from_triangles(ctx, &params, tri_xy.data(), (int)(tri_xy.size() / 6)), "mpmvs_prior_from_triangles");
}

// reference src/PatchMatch.cu:1188-1254, exactly the stub of INTEGRATION.md section 2: the launches AND the device-to-host
// copies that end the reference's Run() (:1246-1251) are one mpmvs_run_get call; hostGeomCosts travels whenever
// params.geomPlanarPrior is set (:1248), which includes the planar-prior re-run of a geometric pass.
// SetDeferredFetch(true) (not in the reference) turns the copies into a fetch on first host access: between the two Run()
// calls of a planar-prior Problem whose prior is built on the device nothing has to leave HBM.
void PatchMatchCUDA::Run() {
    if (deferred_fetch) {
        check(mpmvs_run(ctx, &params, seed), "mpmvs_run");
        host_state_valid = false;
        return;
    }
    if (params.geomPlanarPrior && hostGeomCosts.empty()) hostGeomCosts.allocate(hostCosts.size());
    check(mpmvs_run_get(ctx, &params, seed, hostPlaneHypotheses.data(), hostCosts.data(), params.geomPlanarPrior ? hostGeomCosts.data() : nullptr),
          "mpmvs_run_get");
    host_state_valid = true;
}
void PatchMatchCUDA::fetch_host_state() {
    if (host_state_valid) return;
    if (hostGeomCosts.empty() && params.geomPlanarPrior) hostGeomCosts.allocate(hostCosts.size());
    check(mpmvs_get(ctx, hostPlaneHypotheses.data(), hostCosts.data(), params.geomPlanarPrior ? hostGeomCosts.data() : nullptr), "mpmvs_get");
    host_state_valid = true;
}

float PatchMatchCUDA::GetDepthFromPlaneParam(const float4 pl, const int x, const int y) {
    const Camera& c = cameras[0];
    return -pl.w * c.K[0] / (((float)x - c.K[2]) * pl.x + (c.K[0] / c.K[4]) * ((float)y - c.K[5]) * pl.y + c.K[0] * pl.z);
}
float PatchMatchCUDA::GetMinDepth() { return params.depth_min; }
float PatchMatchCUDA::GetMaxDepth() { return params.depth_max; }
int PatchMatchCUDA::GetReferenceImageWidth() { return cameras[0].width; }
int PatchMatchCUDA::GetReferenceImageHeight() { return cameras[0].height; }
const Image& PatchMatchCUDA::GetReferenceImage() { return *images[0]; }
const void* PatchMatchCUDA::ViewBuffer(size_t i) const { return images8.empty() ? (const void*)images[i]->data.data() : (const void*)images8[i]->data.data(); }
float4 PatchMatchCUDA::GetPlaneHypothesis(const int index) {
    fetch_host_state();
    return hostPlaneHypotheses[index];
}
float PatchMatchCUDA::GetCost(const int index) {
    fetch_host_state();
    return hostCosts[index];
}
float PatchMatchCUDA::GetGeomCost(const int index) {
    fetch_host_state();
    return hostGeomCosts[index];
}

float4 PatchMatchCUDA::GetPriorPlaneParams(const Triangle triangle, int width) {
    fetch_host_state();
    return mpmvs_host::PriorPlane(cameras[0], triangle, hostPlaneHypotheses.data(), width);
}
std::vector<Triangle> PatchMatchCUDA::DelaunayTriangulation(const Rect boundRC, const std::vector<Point>& points) {
    if (points.empty()) {
        std::cout << "No Point to Triangulate!" << std::endl;
        exit(1);
    }
    return mpmvs_host::Delaunay(boundRC, points);
}
// MPMVS_HOST_PRIOR=1: build the planar prior with the host implementation (planar_prior.cpp) instead of the device kernels
// (pm_prior.hpp); both give the same bits (tests/test_prior_gpu.py)
static bool host_prior_requested() {
    static const bool on = std::getenv("MPMVS_HOST_PRIOR") != nullptr;
    return on;
}
void PatchMatchCUDA::GetTriangulateVertices(std::vector<Point>& Vertices) {
    const int W = GetReferenceImageWidth(), H = GetReferenceImageHeight();
    if (host_prior_requested()) {
        fetch_host_state();
        mpmvs_host::TriangulateVertices(W, H, hostCosts.data(), params.geomPlanarPrior ? hostGeomCosts.data() : nullptr, params.geomPlanarPrior, Vertices);
        return;
    }
    const int cap = 3 * ((W + 4) / 5) * ((H + 4) / 5);
    std::vector<int> xy((size_t)cap * 2);
    int n = 0;
    check(mpmvs_prior_vertices(ctx, params.geomPlanarPrior ? 1 : 0, xy.data(), cap, &n), "mpmvs_prior_vertices");
    Vertices.resize((size_t)n);
    for (int i = 0; i < n; ++i) Vertices[i] = Point(xy[2 * i], xy[2 * i + 1]);
}

// reference src/PatchMatch.cpp:1091-1139
void PatchMatchCUDA::Release(std::vector<Scene>&, const int&) {
    StageTimer tm;
    if (ctx && ref_scene && !cameras.empty()) {
        // leave the context (textures, state) in HBM for the next pass over this Problem, within the cache budget
        size_t bytes = 0;
        for (const Camera& c : cameras) bytes += (size_t)c.width * c.height * 20;           // texture (<= 16 B / texel) + depth map
        bytes += (size_t)cameras[0].width * cameras[0].height * 64;                        // planes, costs, masks, prior, padded image
        if (ProblemDeviceCache::held() + bytes <= ctx_cache_cap()) {
            auto keep = std::make_shared<ProblemDeviceCache>();
            keep->ctx = ctx;
            keep->device = device;
            for (size_t i = 0; i < images.size(); ++i) keep->image_data.push_back(ViewBuffer(i));
            keep->cameras = cameras;
            keep->state_stamp = resident_state_stamp;
            keep->depth_stamps = resident_depth_stamps;
            keep->bytes = bytes;
            ProblemDeviceCache::held() += bytes;
            ref_scene->device_cache = std::move(keep);
            ctx = nullptr;
        }
    }
    if (ctx) mpmvs_destroy(ctx);
    ctx = nullptr;
    tm.lap("  release: context");
    hostPlaneHypotheses.clear();
    hostCosts.clear();
    hostGeomCosts.clear();
    hostPriorPlanes.clear();
    hostPlaneMask.clear();
    if (ctx) mpmvs_destroy(ctx);
    ctx = nullptr;
}

// reference src/PatchMatch.cpp:506-638

void ProcessProblem(std::vector<Scene>& Scenes, const int ID, bool geom_consistency, bool planar_prior, uint64_t seed,
                    int device, int max_scale, ProblemResult* results) {
    Scene& scene = Scenes[ID];
    StageTimer tm;
    PatchMatchCUDA MP;
    MP.SetDevice(device);
    MP.SetSeed(seed);
    MP.SetMaxScale(max_scale);
    MP.SetGeomConsistencyParams(geom_consistency, planar_prior);
    MP.PatchMatchInit(Scenes, ID);
    tm.lap("PatchMatchInit");
    MP.AllocatePatchMatch();
    MP.CudaMemInit(Scenes[ID]);
    tm.lap("Allocate + CudaMemInit");
    // the first Run() of a planar-prior Problem whose prior is built on the device: no host code reads its maps (the
    // reference's Run() would copy 46 MB that the second Run() overwrites), so its copies are deferred = never made
    MP.SetDeferredFetch(planar_prior && !host_prior_requested());
    MP.Run();
    MP.SetDeferredFetch(false);
    tm.lap("Run");

    const int width = MP.GetReferenceImageWidth();
    const int height = MP.GetReferenceImageHeight();

    if (planar_prior) {
        MP.SetPlanarPriorParams();
        MP.SetGeomConsistencyParams(false, true);
        const Rect imageRC{0, 0, width, height};
        std::vector<Point> Vertices;
        MP.GetTriangulateVertices(Vertices);
        tm.lap("GetTriangulateVertices");
        const auto triangles = MP.DelaunayTriangulation(imageRC, Vertices);
        tm.lap("DelaunayTriangulation");
        if (host_prior_requested()) {
            Image mask_tri;
            std::vector<float4> planeParams_tri;
            mpmvs_host::BuildPrior(MP.GetReferenceCamera(), width, height, triangles, MP.GetPlaneHypotheses(), MP.GetMinDepth(), MP.GetMaxDepth(),
                                   planeParams_tri, mask_tri);
            tm.lap("BuildPrior (host)");
            MP.CudaPlanarPriorInitialization(planeParams_tri, mask_tri);
        } else {
            MP.CudaPlanarPriorInitialization(triangles);  // raster, planes and mask on the device
        }
        tm.lap("CudaPlanarPriorInit");
        MP.SetSeed(seed + 0x9E3779B97F4A7C15ull);  // second Run(): its own RNG streams
        MP.Run();
        tm.lap("Run (prior)");
        MP.SetGeomConsistencyParams(geom_consistency, planar_prior);
    }

    ProblemResult local;
    ProblemResult& out = results ? *results : local;
    // In-place mode overwrites the Scene's maps anyway (they were consumed by CudaMemInit): their storage takes the new maps,
    // so that a pass neither allocates nor page-faults 38 MB of fresh memory.  Every element is written below.
    if (!results) {
        out.depth = std::move(scene.depth);
        out.normal = std::move(scene.normal);
        out.cost = std::move(scene.cost);
    }
    auto sized = [&](Image& img, int channels) {
        if (img.rows != height || img.cols != width || img.ch != channels || img.data.size() != (size_t)height * width * channels)
            img = Image::Uninitialized(height, width, channels);   // every element is written by the parallel loop below (first touch there)
    };
    sized(out.depth, 1);
    sized(out.normal, 3);
    sized(out.cost, 1);
    const float4* host_planes = MP.GetPlaneHypotheses();
    const float* host_costs = MP.GetCosts();
    float *pd = out.depth.data.data(), *pn = out.normal.data.data(), *pc = out.cost.data.data();
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
    for (int row = 0; row < height; ++row)
        for (int col = 0; col < width; ++col) {
            const size_t idx = (size_t)row * width + col;
            const float4 pl = host_planes[idx];
            pd[idx] = pl.w;
            pn[3 * idx] = pl.x;
            pn[3 * idx + 1] = pl.y;
            pn[3 * idx + 2] = pl.z;
            pc[idx] = host_costs[idx];
        }
    // the three maps are exactly what the context holds now: one stamp for them and for the context that Release() leaves
    // with the Scene, so that the next pass over this Problem finds its start state in HBM
    const uint64_t stamp = NewImageStamp();
    out.depth.SealAs(stamp);
    out.normal.SealAs(stamp);
    out.cost.SealAs(stamp);
    MP.NoteResidentState(stamp);
    // a pass schedule that hands depth maps over in HBM: this Problem's new map goes into the buffer it provided (on the device the
    // Problem ran on), to be promoted at the pass barrier
    if (scene.device_depth_next.ptr && scene.device_depth_next.device == MP.GetDevice()) {
        MP.ExportDepthDevice(scene.device_depth_next.ptr);
        scene.device_depth_next.stamp = stamp;
    } else {
        scene.device_depth_next.stamp = 0;
    }
    if (!results) {
        scene.depth = std::move(out.depth);
        scene.normal = std::move(out.normal);
        scene.cost = std::move(out.cost);
    }
    tm.lap("results");
    MP.Release(Scenes, ID);
    tm.lap("Release");
}

// ---------------------------------------------------------------------------
// C entry points used by the Python tests / bench (ctypes)
// ---------------------------------------------------------------------------
extern "C" {

// vertices -> out_xy (2 ints each); returns the count (may exceed cap: call again)
int mpmvs_host_triangulate_vertices(int w, int h, const float* costs, const float* geom_costs, int geomPlanarPrior, int* out_xy, int cap) {
    std::vector<Point> v;
    mpmvs_host::TriangulateVertices(w, h, costs, geom_costs, geomPlanarPrior != 0, v);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) {
        out_xy[2 * i] = v[i].x;
        out_xy[2 * i + 1] = v[i].y;
    }
    return (int)v.size();
}

// triangles -> out_xy (6 ints each); returns the count
int mpmvs_host_delaunay(int w, int h, const int* xy, int n, int* out_xy, int cap) {
    (void)w;
    (void)h;
    if (n < 0 || cap < 0) return -1;
    return (int)mpmvs_host::DelaunayXY(xy, (size_t)n, out_xy, (size_t)cap);
}

// the whole host prior construction of ProcessProblem (reference src/PatchMatch.cpp:532-604)
// from a finished Run(): planes = (world normal, depth) float4, costs, geom costs ->
// per-pixel prior planes (float4) + mask (u32), as CudaPlanarPriorInitialization uploads them.
// Returns the number of triangles used, or -1.
int mpmvs_host_build_prior(const mpmvs_camera* cam, int w, int h, const float* planes4, const float* costs, const float* geom_costs,
                           int geomPlanarPrior, float depth_min, float depth_max, float* prior4, uint32_t* mask) {
    std::vector<Point> v;
    mpmvs_host::TriangulateVertices(w, h, costs, geom_costs, geomPlanarPrior != 0, v);
    if (v.empty()) return -1;
    const auto tris = mpmvs_host::Delaunay(Rect{0, 0, w, h}, v);
    std::vector<float4> pp;
    Image m;
    mpmvs_host::BuildPrior(*cam, w, h, tris, (const float4*)planes4, depth_min, depth_max, pp, m);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const size_t idx = (size_t)i * w + j;
            mask[idx] = (uint32_t)m.at(i, j);
            float4 o{0, 0, 0, 0};
            if (m.at(i, j) > 0) o = pp[(size_t)m.at(i, j) - 1];
            std::memcpy(prior4 + 4 * idx, &o, 16);
        }
    return (int)pp.size();
}

// Raster + plane fit + depth-range test for an EXPLICIT triangle list (tri_xy = n x {x1 y1 x2 y2 x3 y3}, labelled 1..n in
// the given order; reference src/PatchMatch.cpp:554-595).  plane_out (n x 4, may be NULL) receives the per-triangle planes.
// Lets the fixtures of tests/golden/prior_golden_v1.npz pin triangle order ("last one wins") and plane fit separately
// from the Delaunay triangulation.  Returns the number of triangles kept (all vertices inside the image), or -1.
int mpmvs_host_prior_from_triangles(const mpmvs_camera* cam, int w, int h, const int* tri_xy, int n, const float* planes4, float depth_min,
                                    float depth_max, float* prior4, uint32_t* mask, float* plane_out) {
    if (!cam || !tri_xy || n < 0 || !planes4 || !prior4 || !mask) return -1;
    std::vector<Triangle> tris;
    tris.reserve(n);
    for (int i = 0; i < n; ++i)
        tris.push_back(Triangle(Point(tri_xy[6 * i], tri_xy[6 * i + 1]), Point(tri_xy[6 * i + 2], tri_xy[6 * i + 3]),
                                Point(tri_xy[6 * i + 4], tri_xy[6 * i + 5])));
    std::vector<float4> pp;
    Image m;
    mpmvs_host::BuildPrior(*cam, w, h, tris, (const float4*)planes4, depth_min, depth_max, pp, m);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const size_t idx = (size_t)i * w + j;
            mask[idx] = (uint32_t)m.at(i, j);
            float4 o{0, 0, 0, 0};
            if (m.at(i, j) > 0) o = pp[(size_t)m.at(i, j) - 1];
            std::memcpy(prior4 + 4 * idx, &o, 16);
        }
    if (plane_out) std::memcpy(plane_out, pp.data(), pp.size() * sizeof(float4));
    return (int)pp.size();
}

// bilinear resize probe (ResizeLinear)
// test hook of the residency safety net (Image::StillSealed): seal a rows x cols map, then overwrite `n_writes` elements
// starting at `first` DIRECTLY in `data` (a writer that forgot to reset the stamp); returns 1 if the map still counts as sealed
int mpmvs_host_test_seal(const float* src, int rows, int cols, long first, long n_writes, float value) {
    Image im(rows, cols);
    std::memcpy(im.data.data(), src, im.data.size() * sizeof(float));
    im.Seal();
    for (long i = 0; i < n_writes && first + i < (long)im.data.size(); ++i) im.data[first + i] = value;
    return im.StillSealed() ? 1 : 0;
}

int mpmvs_host_resize_linear(const float* src, int w, int h, float* dst, int new_w, int new_h) {
    Image s(h, w, 1);
    std::memcpy(s.data.data(), src, s.data.size() * sizeof(float));
    const Image d = ResizeLinear(s, new_w, new_h);
    std::memcpy(dst, d.data.data(), d.data.size() * sizeof(float));
    return 0;
}

// One Problem through the reference's pass schedule (src/main.cpp:20-41) with the
// source depth maps held fixed (SURVEY 8d cfg 2/3): photometric pass, then
// geom_iterations geometric passes, with the planar-prior re-run where the
// reference schedules it.  images[0]/cams[0] is the reference view.
int mpmvs_host_run_pipeline(int device, int n, const mpmvs_camera* cams, const float* const* images, int max_scale,
                            int geom_iterations, int planar_prior, int geomPlanarPrior, uint64_t seed,
                            const float* const* src_depths, float* out_depth, float* out_normal3, float* out_cost, int max_image_size) {
    StageTimer tm;
    std::vector<Scene> Scenes(n);
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        Scene& s = Scenes[i];
        s.refID = i;
        s.cam = cams[i];
        if (max_image_size > 0) s.max_image_size = max_image_size;
        s.image = Image::Uninitialized(cams[i].height, cams[i].width, 1);
        std::memcpy(s.image.data.data(), images[i], s.image.data.size() * sizeof(float));
        if (i > 0 && src_depths) {
            s.depth = Image::Uninitialized(cams[i].height, cams[i].width, 1);
            std::memcpy(s.depth.data.data(), src_depths[i - 1], s.depth.data.size() * sizeof(float));
            s.depth.Seal();  // held fixed over the passes: uploaded once
        }
    }
    Scenes[0].estimate = true;
    for (int i = 0; i < n; ++i) Scenes[0].srcID.push_back(i);
    tm.lap("pipeline: scenes from arrays");
    bool pp = !geomPlanarPrior && planar_prior;  // reference src/main.cpp:20
    ProcessProblem(Scenes, 0, false, pp, seed, device, max_scale);
    for (int g = 0; g < geom_iterations; ++g) {
        pp = (geomPlanarPrior && g != geom_iterations - 1);  // reference src/main.cpp:31-34
        ProcessProblem(Scenes, 0, true, pp, seed + 1 + (uint64_t)g, device, max_scale);
    }
    tm.lap("pipeline: passes (above)");
    const Scene& r = Scenes[0];
    const int rows = r.depth.rows;
    const size_t row1 = (size_t)r.depth.cols, row3 = 3 * row1;
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
    for (int y = 0; y < rows; ++y) {   // 38 MB into the caller's (usually untouched) arrays: first touch on many threads
        std::memcpy(out_depth + y * row1, r.depth.data.data() + y * row1, row1 * sizeof(float));
        std::memcpy(out_normal3 + y * row3, r.normal.data.data() + y * row3, row3 * sizeof(float));
        std::memcpy(out_cost + y * row1, r.cost.data.data() + y * row1, row1 * sizeof(float));
    }
    tm.lap("pipeline: copy out");
    Scenes.clear();
    tm.lap("pipeline: release scenes");
    return 0;
}
}  // extern "C"
