// PatchMatch.h -- host-side mirror of the reference's PatchMatch.h interface
// (reference include/PatchMatch.h:29-156) for the MI355X build.
//
// Same names, argument meaning and call order as the reference, so that
// ProcessProblem() reads like the reference's (src/PatchMatch.cpp:506-638):
//     PatchMatchCUDA MP; MP.SetGeomConsistencyParams(..); MP.PatchMatchInit(..);
//     MP.AllocatePatchMatch(); MP.CudaMemInit(..); MP.Run(); ... MP.Release(..);
// Differences, all forced by the platform:
//   * the private CUDA handles (textures, curandState, device pointers;
//     reference PatchMatch.h:95-117) are one opaque mpmvs_ctx* (include/mpmvs.h);
//   * OpenCV is not available on the target image, so cv::Mat / cv::Point /
//     cv::Rect are replaced by the minimal Image / Point / Rect below and the
//     Delaunay triangulation + plane fit are our own (planar_prior.cpp);
//   * scenes are held in memory (Scene::image, ::depth, ::normal, ::cost); the
//     DMB / JPEG / cam.txt file formats are a "next" row;
//   * a Run() takes its RNG seed from SetSeed() instead of clock64()
//     (reference src/PatchMatch.cu:546) and the device from SetDevice()
//     instead of cudaSetDevice(0) (reference src/PatchMatch.cpp:509).
#ifndef MPMVS_HOST_PATCHMATCH_H_
#define MPMVS_HOST_PATCHMATCH_H_

#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mpmvs.h"

struct float4 {
    float x, y, z, w;
};
struct float3 {
    float x, y, z;
};

// reference include/PatchMatch.h:35-67, same layouts (they ARE the C-ABI structs)
typedef mpmvs_camera Camera;
struct PatchMatchParams : mpmvs_params {
    PatchMatchParams() {
        max_iterations = 3;
        nSizeHalfWindow = 5;
        num_images = 5;
        max_image_size = 3200;
        nSizeStep = 2;
        sigma_spatial = 5.0f;
        sigma_color = 3.0f;
        top_k = 4;
        depth_min = 0.0f;
        depth_max = 1.0f;
        max_scale = 2;
        scaled_cols = 0.0f;
        scaled_rows = 0.0f;
        geom_consistency = 0;
        geomPlanarPrior = 0;
        planar_prior = 0;
    }
};

struct Point {
    int x, y;
    Point() {}  // deliberately writes nothing (like cv::Point's storage in a resized vector would not be, but a vector of half a
                // million triangles is then allocated without a serial zero-fill); every use assigns before it reads
    Point(int x_, int y_) : x(x_), y(y_) {}
};
struct Rect {
    int x, y, width, height;
    bool contains(const Point& p) const { return p.x >= x && p.y >= y && p.x < x + width && p.y < y + height; }
};
// reference include/PatchMatch.h:69-72
struct Triangle {
    Point pt1, pt2, pt3;
    Triangle() {}
    Triangle(const Point a, const Point b, const Point c) : pt1(a), pt2(b), pt3(c) {}
};

// dense row-major fp32 image with `ch` interleaved channels (stands in for cv::Mat_<float>)
//
// `stamp` lets the device residency below recognise contents it already holds: 0 = unknown (every fresh image, and every
// image written through at()); Seal() gives the present contents a unique stamp that travels with copies and moves.  Code
// that writes `data` directly after sealing should reset the stamp; as a safety net a sealed image also carries a fingerprint
// of its contents (Fingerprint(): 4096 strided samples + the size), and an upload is only skipped while StillSealed() finds the
// fingerprint unchanged -- a writer that forgot the stamp is then merely slower, not wrong (unless it changed none of the samples).
// std::allocator whose value-less construct() default-initialises: a vector<float, ...>(n) or resize(n) then allocates without the
// serial zero fill (and its page faults) of 30 MB maps that are written in full right afterwards, mostly by a parallel loop
// Large blocks (>= 1 MB: the 7.7 / 23 / 31 MB maps of a Problem) come from a per-size free list instead of mmap / munmap: handing
// 170 MB of maps back to the kernel cost a ProcessProblem schedule 11 ms, and as much again in page faults when the next Problem
// mapped them afresh (round 5).  At most MPMVS_HOST_POOL_MB (default 1024) stay cached.
void* PooledAllocate(size_t bytes);
void PooledRelease(void* p, size_t bytes) noexcept;
template <class T>
struct DefaultInitAllocator : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = DefaultInitAllocator<U>;
    };
    DefaultInitAllocator() = default;
    template <class U>
    DefaultInitAllocator(const DefaultInitAllocator<U>&) {}
    T* allocate(size_t n) { return static_cast<T*>(PooledAllocate(n * sizeof(T))); }
    void deallocate(T* p, size_t n) noexcept { PooledRelease(p, n * sizeof(T)); }
    template <class U>
    void construct(U* p) {
        ::new (static_cast<void*>(p)) U;
    }
    template <class U, class... Args>
    void construct(U* p, Args&&... args) {
        ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...);
    }
};
struct Image {
    int rows = 0, cols = 0, ch = 1;
    uint64_t stamp = 0;
    uint64_t sealed_fingerprint = 0;
    std::vector<float, DefaultInitAllocator<float>> data;
    Image() {}
    Image(int r, int c, int channels = 1, float v = 0.0f) : rows(r), cols(c), ch(channels), data((size_t)r * c * channels, v) {}
    // the same shape with UNINITIALISED contents: for maps whose every element is written before it is read
    static Image Uninitialized(int r, int c, int channels = 1) {
        Image im;
        im.rows = r;
        im.cols = c;
        im.ch = channels;
        im.data.resize((size_t)r * c * channels);
        return im;
    }
    bool empty() const { return data.empty(); }
    float& at(int r, int c, int k = 0) {
        stamp = 0;
        return data[((size_t)r * cols + c) * ch + k];
    }
    float at(int r, int c, int k = 0) const { return data[((size_t)r * cols + c) * ch + k]; }
    void Seal();  // the contents are final until the next write: a new unique stamp (+ fingerprint)
    void SealAs(uint64_t s);  // the same with a stamp shared by several maps (the results of one ProcessProblem)
    uint64_t Fingerprint() const;
    bool StillSealed() const { return stamp != 0 && sealed_fingerprint == Fingerprint(); }
};
uint64_t NewImageStamp();

// Host arrays of PatchMatchCUDA (the reference's `new float4[...]`, src/PatchMatch.cpp:966-972,979-982): page-locked
// memory from the C ABI's pool, not zero-filled -- every user writes them in full before reading.
template <class T>
class HostArray {
    T* p = nullptr;
    size_t n = 0;
    bool pinned = false;

   public:
    HostArray() {}
    HostArray(const HostArray&) = delete;
    HostArray& operator=(const HostArray&) = delete;
    ~HostArray() { clear(); }
    void allocate(size_t count) {
        if (count == n && p) return;
        clear();
        p = static_cast<T*>(mpmvs_alloc_pinned(count * sizeof(T)));
        pinned = p != nullptr;
        if (!p) p = static_cast<T*>(std::malloc(count * sizeof(T) + 1));  // pageable fallback: slower copies, same results
        n = count;
    }
    void clear() {
        if (p && pinned) mpmvs_free_pinned(p);
        if (p && !pinned) std::free(p);
        p = nullptr;
        n = 0;
    }
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    T* data() { return p; }
    const T* data() const { return p; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

// Device residency of one Problem between the passes of the schedule: the context with the packed textures
// of the Problem's views stays in HBM after Release() and the next ProcessProblem of the same Problem on the same device
// adopts it instead of uploading the images again.  Opaque here; owned by the Problem's reference Scene.
struct ProblemDeviceCache;

// 8-bit image as cv::imread returns it (interleaved channels; colour = B,G,R)
struct Image8 {
    int rows = 0, cols = 0, ch = 1;
    std::vector<unsigned char> data;
    bool empty() const { return data.empty(); }
};

// reference include/utility.h:17-26 (+ in-memory results instead of .dmb files)
struct Scene {
    bool estimate = false;
    int refID = 0;
    std::vector<int> srcID;  // srcID[0] is the image itself, then its source views
    Image image;             // grey, fp32 0..255: filled by a caller that hands fp32 arrays in (mpmvs_host_run_pipeline); empty for a
                             // Scene read from a folder, which keeps ...
    Image8 image8;           // ... the decoded bytes at the FILE's size: a quarter of the fp32 image, shrunk on the device
    int target_cols = 0, target_rows = 0;   // image8 only: the size the Problems run at, set by AdjustImageScale together with the scaled K
    // the size every consumer of the Scene works at (result maps, exchange buffers, fusion)
    int cols() const { return image8.empty() ? image.cols : (target_cols ? target_cols : image8.cols); }
    int rows() const { return image8.empty() ? image.rows : (target_rows ? target_rows : image8.rows); }
    bool has_image() const { return !image.empty() || !image8.empty(); }
    Camera cam{};            // what ReadCamera() would return for this image
    Image depth;             // last estimated depth map        (depths.dmb)
    Image normal;            // last estimated world normals    (normals.dmb)
    Image cost;              // last estimated costs            (costs.dmb)
    int max_image_size = 3200;
    std::shared_ptr<ProblemDeviceCache> device_cache;  // see ProblemDeviceCache; dropped with the Scene or by ReleaseDeviceCaches
    // The depth map as it lies in HBM (round 5): a dense device buffer of rows x cols floats on `device` whose contents are those of
    // the host map with the same stamp.  A pass schedule that keeps its Problems' contexts resident (RunFolderJacobi) lets
    // ProcessProblem export every new depth map into device_depth_next and promotes it to device_depth at the pass barrier; the
    // Problems of the next pass that list this image as a source then copy it device to device (or GPU to GPU) instead of
    // uploading Scene::depth from the host -- the reference's depths.dmb round trip (src/PatchMatch.cpp:620-633 -> :941-948)
    // without leaving HBM.  ptr == nullptr (the default): the host map is uploaded as before.  The buffers belong to whoever set them.
    struct DeviceDepth {
        float* ptr = nullptr;
        int device = -1;
        uint64_t stamp = 0;
    };
    DeviceDepth device_depth, device_depth_next;
};
// gives the HBM held by cached Problem contexts back (end of a schedule)
void ReleaseDeviceCaches(std::vector<Scene>& Scenes);
// The context Release() left with the Scene, if its device state still is exactly s.depth / s.normal / s.cost (same stamp): the
// consumer of the final maps (RunFusion in its resident form) reads them from there instead of uploading them.  nullptr otherwise.
// consumer_device >= 0: the device the consumer runs on -- a context on ANOTHER device is only offered while GPU-to-GPU copies are
// allowed (MPMVS_PEER_COPY, default on).
mpmvs_ctx* ResidentResultContext(const Scene& s, int consumer_device = -1);

// bilinear resize used by PatchMatchInit's "Adjust image scale" (reference src/PatchMatch.cpp:893-925)
Image ResizeLinear(const Image& src, int new_cols, int new_rows);
// that step for one Scene: an image above s.max_image_size is shrunk in place and s.cam.K follows (no-op otherwise).  A Scene that
// holds bytes (image8) only gets its target size and the scaled K -- same arithmetic, cached as a pair like the shrunk image --
// and is resampled on the device by mpmvs_set_views_u8.
void AdjustImageScale(Scene& s);

class PatchMatchCUDA {
   private:
    int num_img = 0;
    std::vector<const Image*> images;
    std::vector<const Image8*> images8;  // the views as bytes (Scenes read from a folder): all of them or none
    std::vector<const Image*> depths;  // source depth maps of the previous pass (owned by the Scenes)
    std::vector<const Scene::DeviceDepth*> depth_slots;  // ... and where each lies in HBM, if it does (Scene::device_depth)
    std::vector<Camera> cameras;
    mpmvs_ctx* ctx = nullptr;  // replaces reference PatchMatch.h:95-117
    int device = 0;
    uint64_t seed = 0;
    HostArray<float4> hostPlaneHypotheses;
    HostArray<float> hostCosts;
    HostArray<float> hostGeomCosts;
    HostArray<float4> hostPriorPlanes;
    HostArray<unsigned int> hostPlaneMask;
    PatchMatchParams params;
    std::string input_folder, output_folder;
    Scene* ref_scene = nullptr;     // Scenes[ID] of PatchMatchInit: owner of the device cache
    bool views_resident = false;    // the adopted context already holds this Problem's textures
    uint64_t resident_state_stamp = 0;            // stamp of the depth / normal / cost maps whose state the context holds (0: none)
    std::vector<uint64_t> resident_depth_stamps;  // stamps of the source depth maps the context holds
    bool host_state_valid = false;  // hostPlaneHypotheses / hostCosts mirror the device state
    bool deferred_fetch = false;    // Run() leaves its maps in HBM until the host first reads one (SetDeferredFetch)
    void check(int rc, const char* what);
    void fetch_host_state();        // the device-to-host block of Run() (reference src/PatchMatch.cu:1246-1251) when it was deferred

   public:
    ~PatchMatchCUDA();
    void SetDevice(int dev) { device = dev; }
    void SetSeed(uint64_t s) { seed = s; }
    void SetMaxScale(int s) { params.max_scale = s; }  // the reference has no setter
    // Run() normally ends with the reference's device-to-host copies (src/PatchMatch.cu:1246-1251); with deferred fetch the maps
    // are copied when GetPlaneHypothesis / GetCost / GetGeomCost is first called (the first Run() of a planar-prior Problem
    // whose prior is built on the device then copies nothing)
    void SetDeferredFetch(bool on) { deferred_fetch = on; }
    const PatchMatchParams& GetParams() const { return params; }

    void SetGeomConsistencyParams(bool geom_consistency, bool planar_prior);
    void SetPlanarPriorParams();
    void SetFolder(const std::string& in, const std::string& out);
    void PatchMatchInit(std::vector<Scene>& Scenes, const int ID);
    void AllocatePatchMatch();
    void CudaMemInit(Scene& scene);
    void CudaPlanarPriorInitialization(const std::vector<float4>& PlaneParams, const Image& masks);
    // the same from the triangle list: rasterisation, plane fit and depth-range test of reference src/PatchMatch.cpp:554-595
    // run on the device (mpmvs_prior_from_triangles); nothing but the triangles crosses PCIe
    void CudaPlanarPriorInitialization(const std::vector<Triangle>& triangles);
    void Run();

    float GetDepthFromPlaneParam(const float4 plane_hypothesis, const int x, const int y);
    float GetMinDepth();
    float GetMaxDepth();
    int GetReferenceImageWidth();
    int GetReferenceImageHeight();
    const Image& GetReferenceImage();           // the fp32 image; empty for a Scene that holds bytes
    const void* ViewBuffer(size_t i) const;     // the host buffer view i is uploaded from (bytes or fp32): identity of a resident context's contents
    const Camera& GetReferenceCamera() const { return cameras[0]; }
    float4 GetPlaneHypothesis(const int index);
    const float4* GetPlaneHypotheses() {  // the whole hostPlaneHypotheses array (no per-pixel call)
        fetch_host_state();
        return hostPlaneHypotheses.data();
    }
    const float* GetCosts() {  // the whole hostCosts array
        fetch_host_state();
        return hostCosts.data();
    }
    float GetCost(const int index);
    // the geometric-cost map of the last Run() that copied it (ref .cu:1248: only with params.geomPlanarPrior); zeros where the reference
    // would return uninitialised memory (geometric mode without geomPlanarPrior)
    float GetGeomCost(const int index);

    float4 GetPriorPlaneParams(const Triangle triangle, int width);
    std::vector<Triangle> DelaunayTriangulation(const Rect boundRC, const std::vector<Point>& points);
    void GetTriangulateVertices(std::vector<Point>& Vertices);

    // the maps with this stamp are what the device state holds now (ProcessProblem calls it with the stamp of its results):
    // the next pass over this Problem then skips the upload of its start state
    void NoteResidentState(uint64_t stamp) { resident_state_stamp = stamp; }
    // the context's depth map (GetDepthandNormal + median filter of the last Run()) into a dense device buffer on the context's device
    void ExportDepthDevice(float* d_out);
    int GetDevice() const { return device; }
    void Release(std::vector<Scene>& Scenes, const int& ID);
};

// reference src/PatchMatch.cpp:506-638, in memory: results go to Scenes[ID].depth/normal/cost.
// `results` (optional) receives the outputs without touching Scenes[ID], which is
// what a Jacobi pass over many Problems needs.
struct ProblemResult {
    Image depth, normal, cost;
};
void ProcessProblem(std::vector<Scene>& Scenes, const int ID, bool geom_consistency, bool planar_prior,
                    uint64_t seed = 0, int device = 0, int max_scale = 2, ProblemResult* results = nullptr);

// ---- planar prior construction (planar_prior.cpp), usable without a device ----
namespace mpmvs_host {
// Threads for the library's OpenMP loops: min(16, hardware threads), MPMVS_HOST_THREADS overrides.  Never the OpenMP default:
// on a many-core host inside a container with a CPU quota (256 hardware threads, 16 CPUs of quota on the target boxes) a
// 256-thread team spins its quota away after every loop and the whole process is throttled for tens of milliseconds.
int OmpThreads();
// a schedule that drives k Problems from k host threads at once (RunFolderJacobi) says so: each caller's loops then take 1/k of the threads
void SetConcurrentCallers(int k);
// reference src/PatchMatch.cpp:782-853
void TriangulateVertices(int width, int height, const float* costs, const float* geom_costs, bool geomPlanarPrior,
                         std::vector<Point>& Vertices);
// reference src/PatchMatch.cpp:757-780 (cv::Subdiv2D replaced by an exact divide-and-conquer Delaunay, parallel on the host)
std::vector<Triangle> Delaunay(const Rect boundRC, const std::vector<Point>& points);
long long DelaunayXY(const int* xy, size_t count, int* tri_xy, size_t cap);
// reference src/PatchMatch.cpp:723-755 (cv::SVD::solveZ of three points = the plane through them)
float4 PriorPlane(const Camera& cam, const Triangle& t, const float4* planes, int width);
// reference src/PatchMatch.cpp:554-595: rasterise the triangles into a label mask, fit planes,
// drop pixels whose prior depth leaves [depth_min, depth_max]
void BuildPrior(const Camera& cam, int width, int height, const std::vector<Triangle>& triangles, const float4* planes,
                float depth_min, float depth_max, std::vector<float4>& planeParams, Image& mask);
}  // namespace mpmvs_host

#endif
