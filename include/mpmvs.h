/* mpmvs.h -- C ABI of the MI355X-native PatchMatch hot path of MP-MVS.
 *
 * This is the drop-in boundary: everything below
 * PatchMatchCUDA's host methods in the reference goes through these entry
 * points.  The reference has no C ABI of its own; each function names the
 * reference interface it replaces (paths relative to the reference repo).
 * Plain pointers and sizes only; no HIP, torch or OpenCV types.
 *
 * Conventions
 *   - every function returning int returns 0 on success and a negative code on
 *     failure; mpmvs_last_error() then describes it.  Nothing here calls exit()
 *     (the reference prints and exits, src/PatchMatch.cpp:60-65; the C++ wrapper
 *     in mp-mvs_amd/host keeps that behaviour for drop-in use).
 *   - a context is bound to one HIP device and one stream; distinct contexts may
 *     be driven from distinct host threads.  Device state (planes, costs,
 *     selected views, geometric costs) persists across mpmvs_run calls, as the
 *     reference's does between the two Run() calls of ProcessProblem
 *     (src/PatchMatch.cpp:522,606).
 *   - images, depth maps, costs: row-major fp32; planes: row-major float4
 *     (nx, ny, nz, w).  Host inputs are copied at set_* time.
 */
#ifndef MPMVS_H_
#define MPMVS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* include/PatchMatch.h:35-46 (struct Camera), identical layout, 112 bytes */
typedef struct mpmvs_camera {
    float K[9];
    float R[9];
    float t[3];
    float C[3];
    int height;
    int width;
    float depth_min;
    float depth_max;
} mpmvs_camera;

/* include/PatchMatch.h:48-67 (struct PatchMatchParams), identical layout, 56 bytes.
 * Live fields: max_iterations, num_images, sigma_spatial, sigma_color, top_k,
 * depth_min, depth_max, max_scale, geom_consistency, planar_prior,
 * geomPlanarPrior.  The others are carried but unused, as in the reference. */
typedef struct mpmvs_params {
    int max_iterations;
    int nSizeHalfWindow;
    int num_images;
    int max_image_size;
    int nSizeStep;
    float sigma_spatial;
    float sigma_color;
    int top_k;
    float depth_min;
    float depth_max;
    int max_scale;
    float scaled_cols;
    float scaled_rows;
    unsigned char geom_consistency;
    unsigned char geomPlanarPrior;
    unsigned char planar_prior;
} mpmvs_params;

typedef struct mpmvs_ctx mpmvs_ctx;

#define MPMVS_MAX_SRC_VIEWS 32 /* src/PatchMatch.cu:500, width of the view bitmask */

/* kernel kinds for mpmvs_step, in the launch order of PatchMatchCUDA::Run()
 * (src/PatchMatch.cu:1188-1254) */
enum {
    MPMVS_KIND_INIT = 0,         /* InitializeScore   src/PatchMatch.cu:536  */
    MPMVS_KIND_BLACK = 1,        /* BlackPixelUpdate  src/PatchMatch.cu:1000 */
    MPMVS_KIND_RED = 2,          /* RedPixelUpdate    src/PatchMatch.cu:1011 */
    MPMVS_KIND_DEPTH_NORMAL = 3, /* GetDepthandNormal src/PatchMatch.cu:1021 */
    MPMVS_KIND_FILTER_BLACK = 4, /* BlackPixelFilter  src/PatchMatch.cu:1152 */
    MPMVS_KIND_FILTER_RED = 5    /* RedPixelFilter    src/PatchMatch.cu:1164 */
};

/* number of visible HIP devices (replaces the hard-coded cudaSetDevice(0),
 * src/PatchMatch.cpp:509) */
int mpmvs_device_count(void);
/* Which build of the library this is: 0 = bilinear interpolation with exact fp32 fractions (libmpmvs_hip.so, the default), 8 = the
 * fractions quantised to 8 bits as CUDA's texture unit does for the reference's tex2D fetches (reference src/PatchMatch.cu:377;
 * libmpmvs_hip_q8.so, opt-in: closer to the reference BINARY by the last digit of north_star's 1e-3, slower per tap). */
int mpmvs_texture_filter_bits(void);

/* PatchMatchCUDA construction + AllocatePatchMatch (src/PatchMatch.cpp:516,960-976) */
mpmvs_ctx* mpmvs_create(int device);
/* PatchMatchCUDA::Release (src/PatchMatch.cpp:1091-1139) */
void mpmvs_destroy(mpmvs_ctx* ctx);
/* checkCudaCall's message (src/PatchMatch.cpp:60-65); ctx may be NULL after a
 * failed mpmvs_create */
const char* mpmvs_last_error(const mpmvs_ctx* ctx);

/* CudaMemInit image/camera upload (src/PatchMatch.cpp:999-1025): view 0 is the
 * reference image, 1..n-1 the sources; sizes come from cams[i].width/height;
 * pitch_bytes[i] is the host row pitch (NULL = tightly packed).
 * The images are read before the call returns (the caller may release them); the transfer
 * and the unpacking on the device are only ENQUEUED on the context's stream by then (since
 * round 6), so the upload of one Problem overlaps the work of other contexts and this
 * context's next calls.  A transfer that fails later is reported by the next call that
 * waits for the stream (mpmvs_run*, mpmvs_get, ...) as -100. */
int mpmvs_set_views(mpmvs_ctx* ctx, int n, const mpmvs_camera* cams, const float* const* images,
                    const size_t* pitch_bytes);
/* The same upload from the BYTES the image files decoded to (the reference's imread(GRAYSCALE) before its convertTo,
 * src/PatchMatch.cpp:877-882), at the files' own size: an image larger than its camera is shrunk on the device (the
 * reference's cv::resize(INTER_LINEAR), :893-925).  cams[i].width/height is the size the Problem runs at and cams[i].K is
 * already scaled to it, exactly as for mpmvs_set_views; src_widths[i] x src_heights[i] is the size of images[i] (both NULL:
 * every image already has its camera's size); pitch_bytes[i] is the host row pitch in bytes (NULL = tightly packed).
 * DEFINED BY EQUIVALENCE: the context ends in the state that mpmvs_set_views produces for the fp32 images F_i, where
 * F_i = (float)bytes if the sizes agree and otherwise F_i = ResizeLinear((float)bytes, width, height) as
 * mp-mvs_amd/host/PatchMatchHost.cpp states it: fp32, no contraction, sample position (x + 0.5f) * (src / dst) - 0.5f, an
 * index below 0 or at / beyond the last one clamped with weight 0, value = top + ay * (bot - top) with
 * top = s00 + ax * (s10 - s00).  Any ratio is legal; shrinking is the case that matters.
 * Texture format: the sources take the 8-byte fp16 texels iff no SOURCE view is resampled and fp32 is not forced
 * (mpmvs_set_texture_format); otherwise all sources take the 16-byte fp32 texels, the ones that were not resampled included.
 * The reference image becomes the padded fp32 image either way.  (For a resampled image that happens to be all integers
 * mpmvs_set_views would pick the 8-byte texels; both formats are bit-exact against the same oracle, so results agree.)
 * Asynchronous like mpmvs_set_views: the bytes are read before the call returns, transfers and kernels are only enqueued, a
 * later failure surfaces as -100 from the next call that waits.  The host work per image is one row-wise memcpy into the
 * page-locked stage: no per-pixel test, no conversion.  Errors as for mpmvs_set_views (no half-built Problem is left behind);
 * additionally -2 for a non-positive source size, a pitch smaller than the source width or only one of the two size arrays,
 * and -3 for a source image of 2^32 bytes or more.  MPMVS_STAGE_MB groups the views by their source bytes. */
int mpmvs_set_views_u8(mpmvs_ctx* ctx, int n, const mpmvs_camera* cams, const unsigned char* const* images,
                       const int* src_widths, const int* src_heights, const size_t* pitch_bytes);
/* probe: the resampling of mpmvs_set_views_u8 on its own, synchronous.  src = src_h rows of src_w bytes, pitch_bytes apart
 * (0 = tightly packed); out = dense fp32 image of dst_h x dst_w pixels on the host.  0, -2 (bad argument), -3 (too large) or
 * -100 (device error). */
int mpmvs_resize_u8(int device, const unsigned char* src, int src_w, int src_h, size_t pitch_bytes, int dst_w, int dst_h,
                    float* out);

/* CudaMemInit source depth upload for geometric consistency
 * (src/PatchMatch.cpp:1027-1050, read at :941-948); n_src == n-1.  depths[i] == NULL keeps the map of source i that an
 * earlier call uploaded (its size must be the one stated): a caller that knows which maps changed since the last pass
 * uploads only those. */
int mpmvs_set_src_depths(mpmvs_ctx* ctx, int n_src, const float* const* depths, const int* widths,
                         const int* heights, const size_t* pitch_bytes);
/* same, from dense device buffers (pointers valid on the context's device);
 * used by the multi-GPU pass barrier, which all-gathers depth maps in HBM */
int mpmvs_set_src_depths_device(mpmvs_ctx* ctx, int n_src, const float* const* d_depths, const int* widths,
                                const int* heights);
/* both at once, per source: d_depths[i] != NULL copies from a dense device buffer that lies on device src_devices[i] (the
 * context's own: device-to-device; another one of the process: a peer copy; src_devices == NULL: all on the context's device);
 * else depths[i] != NULL uploads from the host (tightly packed rows); else the map of an earlier call is kept.  What the C++ pass
 * schedule uses to hand the depth maps of one pass to the Problems of the next without the round trip through host memory (the
 * reference's depths.dmb files, src/PatchMatch.cpp:620-633 -> :941-948).  Either pointer array may be NULL. */
int mpmvs_set_src_depths_mixed(mpmvs_ctx* ctx, int n_src, const float* const* depths, const float* const* d_depths,
                               const int* src_devices, const int* widths, const int* heights);

/* CudaMemInit start state for geometric-consistency passes
 * (src/PatchMatch.cpp:1073-1086): planes = (world normal, depth) float4, costs
 * fp32; either may be NULL to leave it unchanged */
int mpmvs_set_state(mpmvs_ctx* ctx, const void* planes4, const void* costs);
/* selected-view bitmasks (cudaSelectedViews, include/PatchMatch.h:108); only
 * needed to reproduce a single kernel step from a given state */
int mpmvs_set_selected_views(mpmvs_ctx* ctx, const void* sel_u32);
/* geometric costs (cudaGeomCosts, include/PatchMatch.h:110; written by a geometric Run()); only needed to reproduce the
 * vertex selection of the prior from a given state */
int mpmvs_set_geom_costs(mpmvs_ctx* ctx, const void* geom_costs);
/* CudaPlanarPriorInitialization (src/PatchMatch.cpp:978-996): per-pixel prior
 * plane (n, d) in the reference-camera frame and mask (>0 = has prior) */
int mpmvs_set_prior(mpmvs_ctx* ctx, const void* prior_planes4, const void* mask_u32);

/* ---- planar prior built on the device (the host block of ProcessProblem between its two Run() calls,
 * src/PatchMatch.cpp:532-604): the maps of the first Run() stay in HBM, only the vertex list and the triangle list cross
 * PCIe; the Delaunay triangulation itself stays with the caller (mp-mvs_amd/host: PatchMatchCUDA::DelaunayTriangulation). */
/* GetTriangulateVertices (src/PatchMatch.cpp:782-853) from the costs (geom_rule != 0: and geometric costs, the
 * geomPlanarPrior branch :810-850) the last mpmvs_run left on the device: per 5x5 cell the reliable pixels, in cell raster
 * order.  out_xy receives (x, y) pairs of at most cap vertices; *n the number found (if it exceeds cap, call again). */
int mpmvs_prior_vertices(mpmvs_ctx* ctx, int geom_rule, int* out_xy, int cap, int* n);
/* triangle rasterisation (src/PatchMatch.cpp:554-570, a later triangle overwrites an earlier one), GetPriorPlaneParams
 * (:723-755) with the depths of the last mpmvs_run, the depth-range test (:583-595, params->depth_min/max) and
 * CudaPlanarPriorInitialization (:978-996), all on the device.  tri_xy = n x {x1 y1 x2 y2 x3 y3}, every vertex inside
 * the image (the caller drops the others as :555 does); triangle k is label k + 1.  Installs the prior like
 * mpmvs_set_prior.  -2: a vertex outside the image (refused before anything is counted or launched); -3: an image side above
 * 65 535, the limit of the vertex list's (y << 16) | x packing. */
int mpmvs_prior_from_triangles(mpmvs_ctx* ctx, const mpmvs_params* params, const int* tri_xy, int n);
/* the p-rows mpmvs_prior_from_triangles dispatches for a triangle whose longest edge has the integer square edge_sq[i]
 * (pm::prior_rows, csrc/pm_prior.hpp): never fewer than the reference's `for (float p = 0; p < 1.0; p += step)` runs, never
 * 64 or more above.  -1 for an edge_sq outside [0, 2 * 65535^2], the largest an image of 65 535 x 65 535 holds.  Host arithmetic
 * only, no device is touched; for tests and tools. */
int mpmvs_prior_rows(const long long* edge_sq, int n, int* rows);
/* the installed prior planes (float4) and mask (u32) back on the host, for tests; either may be NULL */
int mpmvs_get_prior(mpmvs_ctx* ctx, void* prior_planes4, void* mask_u32);

/* PatchMatchCUDA::Run() (src/PatchMatch.cu:1188-1254) without its final
 * device-to-host copies: InitializeScore, the red/black schedule selected by
 * params, GetDepthandNormal, both filters.  `seed` replaces
 * curand_init(clock64(), ...) (src/PatchMatch.cu:546).  Blocks until done.
 * params->geom_consistency together with params->planar_prior is rejected (-7):
 * the reference never runs that combination (ProcessProblem clears
 * geom_consistency before the prior Run(), src/PatchMatch.cpp:535).
 * The red/black passes of one window scale (BlackPixelUpdate / RedPixelUpdate, :1211-1236) are ONE launch whose blocks wait for
 * their neighbours of the pass before (same launch numbering, same results; MPMVS_CHAIN=0 in the environment of mpmvs_create
 * launches one kernel per pass).  -101: such a launch gave up waiting (a bounded wait that a correct build never exhausts);
 * the context's results are invalid, the context itself stays usable. */
int mpmvs_run(mpmvs_ctx* ctx, const mpmvs_params* params, uint64_t seed);
/* Run() together with the device-to-host copies that end it in the reference (src/PatchMatch.cu:1246-1251): planes (float4 =
 * world normal + depth), costs and geometric costs into host buffers of W*H elements (each may be NULL; pinned memory makes
 * the copies asynchronous).  The reference copies hostGeomCosts whenever params.geomPlanarPrior is set (:1248) -- also in
 * the planar-prior re-run of a geometric pass, where the flag is still set (src/PatchMatch.cpp:535,655-665) and the map is the
 * one the geometric Run() left on the device -- so a caller passes `params.geomPlanarPrior ? hostGeomCosts : NULL` and any
 * Run() accepts the buffer: it receives what cudaGeomCosts holds.  The cost maps are final after the last update launch and
 * travel while the median filter still runs.  Same results as mpmvs_run followed by mpmvs_get. */
int mpmvs_run_get(mpmvs_ctx* ctx, const mpmvs_params* params, uint64_t seed, void* planes4, void* costs, void* geom_costs);
/* Pipelined form of mpmvs_run_get for a caller that works through many Problems / seeds on one context (the reference's Run()
 * ends with blocking cudaMemcpy calls, src/PatchMatch.cu:1246-1251: 38 MB at PCIe rate = 4 % of a cfg-1 step during which the
 * GPU idles).  The call enqueues the launches of Run(), stages the result maps on the device and returns at once; the maps
 * reach the (page-locked) host buffers on a second stream while the NEXT mpmvs_run_get_async of this context already runs.
 * Consecutive calls need different host buffers; mpmvs_wait() returns when every outstanding call has delivered.  Between the
 * first such call and mpmvs_wait() the context rejects every other entry point (-8).  Results: those of mpmvs_run_get. */
int mpmvs_run_get_async(mpmvs_ctx* ctx, const mpmvs_params* params, uint64_t seed, void* planes4, void* costs, void* geom_costs);
int mpmvs_wait(mpmvs_ctx* ctx);
/* one kernel of Run(), for parity tests; launch_id selects the RNG stream the
 * way Run() numbers its launches (0 = InitializeScore, then in launch order) */
int mpmvs_step(mpmvs_ctx* ctx, const mpmvs_params* params, uint64_t seed, int kind, int iter, int scale,
               uint32_t launch_id);

/* the cudaMemcpy device-to-host block of Run() (src/PatchMatch.cu:1246-1251);
 * any pointer may be NULL */
int mpmvs_get(mpmvs_ctx* ctx, void* planes4, void* costs, void* geom_costs);
int mpmvs_get_selected_views(mpmvs_ctx* ctx, void* sel_u32);
/* dense fp32 depth map (plane .w) written to a device buffer of H*W floats; the
 * multi-GPU barrier all-gathers these (replaces the depths.dmb round trip,
 * src/PatchMatch.cpp:620-633 -> :941-948) */
int mpmvs_export_depth_device(mpmvs_ctx* ctx, float* d_out);

/* ---- probes used by the parity tests ------------------------------------ */
/* ComputeBilateralNCC (src/PatchMatch.cu:325-414) of per-pixel camera-frame
 * planes against every source view; out is [num_images-1][H][W] */
int mpmvs_eval_ncc(mpmvs_ctx* ctx, const mpmvs_params* params, const void* planes_cam4, int scale, void* out);
/* the same for nh planes per pixel (planes_cam4 = [nh][H][W] float4, out = [nh][num_images-1][H][W]) with a choice of
 * the lane mapping: only 0 (one thread per pixel) exists; the cooperative lane-group mappings tried in round 2 were removed.  *kernel_ms
 * (may be NULL) receives the device time of the kernel (HIP events). */
int mpmvs_eval_ncc_multi(mpmvs_ctx* ctx, const mpmvs_params* params, const void* planes_cam4, int nh, int scale, int mapping,
                         void* out, float* kernel_ms);
/* ComputeGeomConsistencyCost (src/PatchMatch.cu:617-640); out [num_images-1][H][W] */
int mpmvs_eval_geom(mpmvs_ctx* ctx, const mpmvs_params* params, const void* planes_cam4, void* out);
/* ComputeHomography (src/PatchMatch.cu:228-279) for one plane and source view
 * (0-based); H9 receives 9 floats, row-major */
int mpmvs_homography(mpmvs_ctx* ctx, const void* plane4, int src_view, void* H9);
/* canonical device math, fn: 0 rcp, 1 exp, 2 sin, 3 cos, 4 acos, 5 fract */
int mpmvs_math(int fn, const void* in, void* out, int n);
/* exhaustive check of the kernels' reciprocal against the rule the CPU oracle implements, over all 2^32 float bit patterns
 * (about a second): counts[0] inputs z with z and 1 / z normal, counts[1] of those whose result differs from the correctly
 * rounded quotient 1.0f / z, counts[2] all other inputs, counts[3] of those that break the rule "signed zero where 1 / z is
 * denormal, not finite for zero / denormal / infinite / NaN z".  counts[1] == counts[3] == 0 is what lets the oracle divide. */
int mpmvs_verify_rcp(unsigned long long counts[4]);
/* first n uniforms of RNG stream (seed, pixel, launch_id) */
int mpmvs_rng(uint64_t seed, uint32_t pix, uint32_t launch_id, int n, void* out);

/* ---- depth-map fusion ---------------------------------------- */
/* RunFusion's per-pixel consistency check and averaging (src/PatchMatch.cpp:287-504) in
 * the deterministic "snapshot" formulation of DESIGN.md section 8.  Image k has
 * cams[k] (width/height = size of its maps), depths[k] (fp32), normals[k] (3 fp32 per
 * pixel, world frame), colors[k] (8-bit, color_channels = 3: interleaved B,G,R as the
 * reference's cv::Vec3b image, :324; or 1: grey, replicated), estimate[k] (0 = skip),
 * and the view list src_ids[src_off[k] .. src_off[k+1]) whose first entry is k itself
 * (Scene::srcID); a list that names a view twice, or image k among its own sources, is rejected (-2), and so are, before
 * anything is launched, a list whose first entry is not k, an estimated image with an empty list, and an estimated image with
 * more than 1 + MPMVS_MAX_SRC_VIEWS entries.  A list that holds only k is legal and yields no point.  sky may be NULL, or hold per image NULL or an 8-bit mask of the map's
 * size: pixels with sky > 0 are masked when their image is fused (:385-388).
 * Outputs per image: out_valid (1 where a fused point was produced), out_points9
 * (x y z nx ny nz c0 c1 c2 per pixel, colour in the input channel order), out_masks
 * (pixels consumed by points of other images, and sky pixels).  Host buffers in and out. */
/* use_dynamic_consistency is a set of flags: */
#define MPMVS_FUSE_DYNAMIC_CONSISTENCY 1 /* config `use_dynamic_consistency` (src/PatchMatch.cpp:458) */
#define MPMVS_FUSE_REFERENCE_ORDER 2     /* the reference's sequential masking order (in-place masks, persistent used_list,
                                            src/PatchMatch.cpp:382,416,470-495) instead of the snapshot formulation: same result as
                                            the sequential loop, computed as a parallel fixpoint */
int mpmvs_fuse(int device, int n, const mpmvs_camera* cams, const int* estimate, const float* const* depths,
               const float* const* normals, const unsigned char* const* colors, int color_channels,
               const unsigned char* const* sky, const int* src_off, const int* src_ids, int use_dynamic_consistency,
               unsigned char* const* out_valid, float* const* out_points9, unsigned char* const* out_masks);

/* The same fusion, but the points are compacted on the device and come back as the vertex records of the reference's
 * binary PLY (StoreColorPlyFileBinaryPointCloud, src/PatchMatch.cpp:145-198): 27 bytes each = x y z nx ny nz (float32)
 * red green blue (uint8; colors must then be B,G,R or grey), non-finite coordinates zeroed, in the reference's PointCloud
 * order (image index, then raster).  *records receives a buffer to release with mpmvs_free; out_masks may be NULL.
 * Returns the number of points, or a negative error code. */
long long mpmvs_fuse_ply(int device, int n, const mpmvs_camera* cams, const int* estimate, const float* const* depths,
                         const float* const* normals, const unsigned char* const* colors, int color_channels,
                         const unsigned char* const* sky, const int* src_off, const int* src_ids, int use_dynamic_consistency,
                         unsigned char** records, unsigned char* const* out_masks);
void mpmvs_free(void* p);

/* Both calls for maps that never left HBM: ctxs[i] != NULL names the PatchMatch context whose last Run() estimated image i
 * (its state holds world normal + depth per pixel, what the reference's Run() copies out, src/PatchMatch.cu:1246, ProcessProblem
 * writes to depths.dmb / normals.dmb, src/PatchMatch.cpp:610-633, and RunFusion reads back, :334-336).  Such an image is not
 * uploaded (19 of its 19 + channels bytes per pixel stay where they are): its planes are split into the fusion's arrays on the
 * device, or copied GPU to GPU first when the context lives on another device of the process.  depths[i] / normals[i] are used
 * for the images without a context; both arrays may be NULL when every image has one.  The context must have completed a Run()
 * (mpmvs_run / mpmvs_run_get, or mpmvs_wait after the pipelined form) at the size of cams[i], else -2.  Same results, bit for
 * bit, as the host-array forms on the maps mpmvs_get returns. */
int mpmvs_fuse_ctx(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs, const float* const* depths,
                   const float* const* normals, const unsigned char* const* colors, int color_channels,
                   const unsigned char* const* sky, const int* src_off, const int* src_ids, int use_dynamic_consistency,
                   unsigned char* const* out_valid, float* const* out_points9, unsigned char* const* out_masks);
long long mpmvs_fuse_ply_ctx(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs,
                             const float* const* depths, const float* const* normals, const unsigned char* const* colors,
                             int color_channels, const unsigned char* const* sky, const int* src_off, const int* src_ids,
                             int use_dynamic_consistency, unsigned char** records, unsigned char* const* out_masks);

/* Tracks: which pixels of which images each fused point was averaged from.
 * A point is produced by pixel t (raster index r * W_i + c) of image i, whose view list is src_ids[src_off[i] ..) with slot 0 =
 * i itself.  Its TRACK is the sequence (i, t), followed in ascending slot order j = 1 .. num_ngb - 1 by (src_ids[j], q_j) for
 * every slot whose source pixel q_j passed the consistency test against t in the evaluation that produced the point; q_j is the
 * raster index sr * W_s + sc in source image s = src_ids[j], at THAT image's own width (the images of a call may differ in size).
 *  - The track has num + 1 entries, the divisor of the point's averages: at least 2 with MPMVS_FUSE_DYNAMIC_CONSISTENCY, 3 without.
 *  - Snapshot formulation: the entries after the first are exactly the pixels the point marks in out_masks.
 *  - MPMVS_FUSE_REFERENCE_ORDER: the entries are the pixel's own consistent source pixels in the final fixpoint pass, not the
 *    carried used_list entries, which only mask: there the marks are a superset of the tracks.
 *  - DEFINING PROPERTY: the track alone reproduces the point bit for bit.  With X(s, q) the back-projection of pixel q of image s
 *    at its depth (x = q % W_s, y = q / W_s;  ((depth * (x - K[2])) / K[0], (depth * (y - K[5])) / K[4], depth) rotated by R^T
 *    and moved by C, fp32, as the fusion computes it), the position is ((X(i, t) + X(s_1, q_1)) + ...) / (float)length in fp32, in
 *    track order; normal and colour are the same sums of normals[s][q] and colors[s][q] over the same divisor.
 * mpmvs_fuse_ply_tracks is mpmvs_fuse_ply_ctx -- same arguments, flags, errors and records; ctxs may be NULL, which is
 * mpmvs_fuse_ply -- and returns the tracks as CSR in the PLY's point order: *track_off has count + 1 entries, track_off[0] = 0,
 * and point p owns entries track_off[p] .. track_off[p + 1) of *track_image (image index) and *track_pixel (raster index), which
 * have track_off[count] entries each.  All four buffers are released with mpmvs_free; on failure none is allocated.  A NULL
 * track_* pointer is -2; a view whose pixels x list length exceeds 2^31 - 1 is -3.  Device memory for the tracks is bounded by
 * the largest view (pixels x list length), not by the dataset: every image's tracks go to the host before the next is fused. */
long long mpmvs_fuse_ply_tracks(int device, int n, const mpmvs_camera* cams, const int* estimate, mpmvs_ctx* const* ctxs,
                                const float* const* depths, const float* const* normals, const unsigned char* const* colors,
                                int color_channels, const unsigned char* const* sky, const int* src_off, const int* src_ids,
                                int use_dynamic_consistency, unsigned char** records, long long** track_off, int32_t** track_image,
                                int32_t** track_pixel, unsigned char* const* out_masks);

/* device time (ms, HIP events) of the kernels of the last mpmvs_fuse / mpmvs_fuse_ply call */
float mpmvs_fuse_kernel_ms(void);
/* fixpoint passes of the last MPMVS_FUSE_REFERENCE_ORDER call: sum over the images and the largest count of one image */
void mpmvs_fuse_passes(int* total, int* max_per_image);

/* ---- sky-mask refinement --------------------------------------- */
/* The device half of bilateral_filter (SkySegment/src/SkyRegionDetect.cu:36-66: the
 * allocations, copies and the Pixel_bilateral_filter launch, :3-34): bgr is the 8-bit
 * B,G,R image (height x width x 3), mask the coarse sky probability already resized to
 * the image (fp32, height x width), out receives 255.0f / 0.0f per pixel.  Host buffers. */
int mpmvs_sky_bilateral(int device, const unsigned char* bgr, const float* mask, float* out, int height, int width);
/* device time (ms, HIP events) of the kernel of the last mpmvs_sky_bilateral call */
float mpmvs_sky_kernel_ms(void);

/* ---- sky-segmentation network ------------ */
/* The network that produces the coarse sky mask: the reference loads an ncnn .param / .bin pair (SkySegment::SkySegment,
 * SkySegment/src/SkyRegionDetect.cpp:541-547) and runs it through ncnn on the CPU (maskExtractor, :549-561).  Here the pair is
 * data for an inference engine on the device (csrc/pm_skyseg.hpp).  Supported operators: Input, Convolution (3x3 with pad =
 * dilation, or 1x1; stride 1, group 1; activation none / ReLU / sigmoid; weight tag 0x01306B47 = fp16 or 0 = fp32), Pooling (max
 * 2x2 stride 2, ncnn's default pad mode = ceil mode), Interp (bilinear to a fixed size, no align_corner), BinaryOp (sum of two
 * blobs), Concat (channels), Split, Sigmoid.  Anything else is refused at load with one of the codes below and a
 * mpmvs_last_error(NULL) text that names the layer (the text is per host thread, as after a failed mpmvs_create). */
#define MPMVS_SKYSEG_E_FILE (-20)     /* a file cannot be read */
#define MPMVS_SKYSEG_E_MAGIC (-21)    /* not an ncnn text .param: wrong magic, or a malformed count / layer line */
#define MPMVS_SKYSEG_E_LAYER (-22)    /* unknown layer type (also: a second Input, a Concat along another axis) */
#define MPMVS_SKYSEG_E_CONV (-23)     /* Convolution with stride != 1, group != 1, a non-square kernel, another kernel / pad / activation */
#define MPMVS_SKYSEG_E_TAG (-24)      /* int8 or unknown weight tag */
#define MPMVS_SKYSEG_E_POOL (-25)     /* Pooling other than max 2x2 stride 2 */
#define MPMVS_SKYSEG_E_INTERP (-26)   /* Interp other than bilinear to a fixed size without align_corner */
#define MPMVS_SKYSEG_E_BINARY (-27)   /* BinaryOp other than the sum of two blobs */
#define MPMVS_SKYSEG_E_ORDER (-28)    /* a blob is read before it is written (or written twice) */
#define MPMVS_SKYSEG_E_SHORT (-29)    /* the .bin ends before the last weight */
#define MPMVS_SKYSEG_E_LEFTOVER (-30) /* the .bin has bytes left over after the last weight */
#define MPMVS_SKYSEG_E_SHAPE (-31)    /* the graph does not close for the given input size (Concat / sum of different sizes, channel count) */
#define MPMVS_SKYSEG_E_OUTPUT (-32)   /* no blob of the requested output name */
#define MPMVS_SKYSEG_E_NOKEEP (-33)   /* mpmvs_skyseg_blob without keep mode, or before the first run in keep mode */
#define MPMVS_SKYSEG_E_NOBLOB (-34)   /* mpmvs_skyseg_blob: no live blob of that name */
#define MPMVS_SKYSEG_MAX_CONCAT 6     /* most parts a Concat that feeds a Convolution may have */
typedef struct mpmvs_skyseg mpmvs_skyseg;
/* What the loader makes of the pair for an in_h x in_w input, without touching a device: counts[0] layers, [1] blobs (as the
 * .param declares them), [2] convolutions, [3] live layers (those output_blob depends on; NULL / "" = the last layer's output),
 * [4] bytes of the .bin consumed, [5] multiply-adds of all convolutions per image.  0 or a code above (-2: bad argument). */
int mpmvs_skyseg_inspect(const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, long long counts[6]);
/* Net::load_param + load_model (SkyRegionDetect.cpp:543-546): reads the pair, repacks the weights for the matrix instruction,
 * plans one arena for the intermediate blobs by liveness and uploads.  A failed load leaves no device allocation behind. */
int mpmvs_skyseg_load(int device, const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, mpmvs_skyseg** net);
/* ex.input + ex.extract (SkyRegionDetect.cpp:553-556): the bare network.  chw_fp32_in = input channels x in_h x in_w floats,
 * out = the output blob (channels x height x width floats); host buffers.  Blocks until done.  Deterministic. */
int mpmvs_skyseg_run(mpmvs_skyseg* net, const float* chw_fp32_in, float* out);
/* maskExtractor (SkyRegionDetect.cpp:549-561) with the pyrDown loop in front of it (src/PatchMatch.cpp:16-18): bgr = h rows of w
 * B,G,R byte triples, pitch_bytes apart (0 = tightly packed).  While h > 768 and w > 768 the image is halved (5x5 binomial,
 * reflect-101 border, (s + 128) >> 8, size (w / 2, h / 2)); then resized to the network's input size with the ResizeLinear
 * geometry, rounded to bytes, split into R,G,B planes and normalised ((v - mean) * norm with the reference's constants); then
 * the network runs.  All on the device.  out_prob = the output blob.  The network must take 3 channels (-2 otherwise). */
int mpmvs_skyseg_run_u8(mpmvs_skyseg* net, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out_prob);
/* probe: only the preprocessing of mpmvs_skyseg_run_u8; out_chw receives the 3 x in_h x in_w floats the network would be given */
int mpmvs_skyseg_preprocess_u8(mpmvs_skyseg* net, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out_chw);
/* keep != 0: every blob gets its own place in the arena (no reuse), so that mpmvs_skyseg_blob can fetch any of them after a
 * run; 0 (the default) plans by liveness again.  The results are the same bits either way. */
int mpmvs_skyseg_set_keep(mpmvs_skyseg* net, int keep);
/* the blob `name` of the last run (keep mode only): dims[0..2] = channels, height, width (always written when the blob exists);
 * out may be NULL to ask for the size alone.  A Concat result is assembled here, on the way out. */
int mpmvs_skyseg_blob(mpmvs_skyseg* net, const char* name, float* out, int dims[3]);
/* shape of the input and of the output blob: dims[0..2] input c, h, w, dims[3..5] output c, h, w; kernel launches per run in dims[6] */
int mpmvs_skyseg_dims(const mpmvs_skyseg* net, int dims[7]);
/* device time (ms, HIP events) of the last run: the kernels of the network, without the copies; for mpmvs_skyseg_run_u8
 * *pre_ms (may be NULL) receives the time of the preprocessing kernels in front of it */
float mpmvs_skyseg_ms(const mpmvs_skyseg* net, float* pre_ms);
void mpmvs_skyseg_destroy(mpmvs_skyseg* net);

/* ---- view selection of a COLMAP sparse model (tools/colmap2mvs.py) ------------ */
/* The pair scores and per-image view lists of the reference's colmap2mvsnet_acm.py (calc_score, then the reversed
 * argsort of each score row), restated point-major (csrc/pm_viewsel.hpp, contract in DESIGN.md section 11).
 * centers: n_images x 3 camera centres (float64), xyz: n_points x 3, obs_off: n_images + 1 offsets into obs_pt, which holds
 * every image's point3D_ids in file order as dense point indices (-1: none).  out_ids / out_scores (n_images x num_view,
 * num_view <= n_images) receive each row by score descending, then index descending.  shared / small (n_images x n_images,
 * either may be NULL; for tests) receive the counts of each pair i < j in [i][j], zero below the diagonal.  Host buffers.
 * Returns 0, -1 (bad arguments; checked before the device is touched), -2 (n_images above MPMVS_VIEW_SELECT_MAX_IMAGES)
 * or -100 (HIP failure). */
#define MPMVS_VIEW_SELECT_MAX_IMAGES 32768
int mpmvs_view_select(int device, int n_images, const double* centers, int n_points, const double* xyz, const int64_t* obs_off,
                      const int32_t* obs_pt, int num_view, int32_t* out_ids, int32_t* out_scores, uint32_t* shared, uint32_t* small);
/* device time (ms, HIP events) of the kernels of the last mpmvs_view_select call */
float mpmvs_view_select_kernel_ms(void);

/* ---- undistortion of COLMAP camera models (tools/colmap2mvs.py --undistort) --- */
/* model_id indexes COLMAP's 11 camera models in the order of mp-mvs_amd/colmap.py CAMERA_MODELS (0 SIMPLE_PINHOLE ... 10
 * THIN_PRISM_FISHEYE); params holds the model's n_params parameters in the order of a cameras file (f | fx fy, cx, cy, then the
 * distortion terms).  The models, the output-camera rule and the warp are stated once, in fp64 without contraction and without
 * any libm transcendental on the forward path, in mp-mvs_amd/csrc/pm_undistort_model.hpp (contract: DESIGN.md section 12). */
/* The PINHOLE camera an image of the given camera is resampled to: COLMAP's UndistortCamera rule with the options
 * blank_pixels (0: no blank pixel in the output ... 1: every source pixel kept), min_scale and max_scale (COLMAP's defaults:
 * 0, 0.2, 2.0).  out_pinhole receives fx fy cx' cy' (the focal lengths are the source's), *out_width / *out_height the size
 * W' x H'; a SIMPLE_PINHOLE or PINHOLE source comes back unchanged.  Host only: touches no device.
 * Returns 0, or -2 for an unknown model, a wrong parameter count, a parameter that is not finite, a focal length or size that
 * is not positive, or options outside 0 <= blank_pixels <= 1, 0 < min_scale <= max_scale. */
int mpmvs_undistort_camera(int model_id, const double* params, int n_params, int width, int height, double blank_pixels,
                           double min_scale, double max_scale, double out_pinhole[4], int* out_width, int* out_height);
/* The warp: src = height rows of width pixels of `channels` (1 or 3) interleaved bytes, pitch_bytes apart (0 = tightly packed),
 * taken by the camera (model_id, params); out = dense dst_height x dst_width x channels bytes of the PINHOLE camera dst_pinhole
 * (fx fy cx cy); out_valid (may be NULL) = dst_height x dst_width bytes, 1 where the pixel has a source and 0 where not.
 * DEFINED BY EQUIVALENCE: the bytes of the host statement in mp-mvs_amd/host/undistort.cpp, bit for bit.  Per output pixel
 * (X, Y): u = (X + 0.5 - cx) / fx, v = (Y + 0.5 - cy) / fy, (x, y) = forward map of the model, sx = x - 0.5, sy = y - 0.5; the
 * pixel is valid iff 0 <= sx <= width - 1 and 0 <= sy <= height - 1, otherwise every channel is 0; x0 = floor(sx),
 * ax = sx - x0, x1 = min(x0 + 1, width - 1), likewise in y; per channel top = s00 + ax * (s10 - s00),
 * bot = s01 + ax * (s11 - s01), val = top + ay * (bot - top) in fp64; the byte is (int)(val + 0.5).
 * The validity rule is strict, so an identity warp (a pinhole camera, or a model with all-zero distortion, onto its own pinhole
 * and size) returns the source bytes everywhere it is valid, but with a focal length that is no power of two
 * fx * ((X + 0.5 - cx) / fx) + cx - 0.5 can miss X by an ulp and put a pixel of the outermost row or column just outside the
 * image: that pixel comes back 0 / invalid.  Callers that need the identity copy such images (the converter does).
 * Host buffers in and out; blocks until done; runs on a stream of its own.  Returns 0, -2 (a NULL src / out / dst_pinhole,
 * channels other than 1 or 3, a non-positive size, a pitch below width * channels, a camera mpmvs_undistort_camera refuses;
 * checked before the device is touched), -3 (an output of 2^31 bytes or more, a source row of 2^31 bytes or more, or a source
 * of 2^40 bytes or more) or -100 (HIP failure, a bad device included). */
int mpmvs_undistort_u8(int device, const unsigned char* src, int channels, int width, int height, size_t pitch_bytes, int model_id,
                       const double* params, int n_params, const double dst_pinhole[4], int dst_width, int dst_height,
                       unsigned char* out, unsigned char* out_valid);
/* device time (ms, HIP events) of the kernel of the calling thread's last successful mpmvs_undistort_u8 call */
float mpmvs_undistort_kernel_ms(void);

/* ---- point clouds: exact capped nearest neighbour (mp-mvs_amd/cloud.py, tools/eval_ply.py) --- */
/* A target cloud on one device and, per query point, its nearest target point within a radius: what the accuracy /
 * completeness / F1 score of a fused cloud against a ground-truth scan needs.
 * DEFINED BY EQUIVALENCE with the brute-force statement, bit for bit and independent of scheduling:
 *   r2 = radius * radius in fp32.
 *   For query q and target p: dx = qx - px, likewise dy, dz, all in fp32; d2 = (dx*dx + dy*dy) + dz*dz in fp32, no contraction.
 *   p is a candidate iff all its coordinates are finite and d2 <= r2.
 *   out_d2 = the smallest candidate d2; out_idx = the smallest index among the candidates that attain it (duplicates and the
 *   order in which the device handles the points do not show in the result).
 *   No candidate, or a query with a non-finite coordinate: out_d2 = +inf, out_idx = -1.
 * The search structure is a sparse uniform grid of cell edge max(radius, 2^-60) * (1 + 2^-10) addressed through a hash table
 * (mp-mvs_amd/csrc/pm_cloud.hpp); it is built by the first call with a radius and cached in the handle per radius: a later call
 * with the same radius reuses it, another radius builds its own (a handle keeps up to 8 grids; one more radius takes over the
 * buffers of the least recently used one).
 * Errors (text through mpmvs_last_error with a NULL context, per host thread): -2 = a NULL xyz with n > 0, a negative count, a radius
 * that is not finite or <= 0, a NULL cloud or out_d2; -3 = n or n_q above 2^31 - 1, more than 2^29 finite target points (the
 * table's slot count, a power of two of at least twice the finite points, is held to 2^30), or a target whose finite bounding box
 * spans more than 2^21 cells along an axis at this radius (the text names the axis and the ratio; the handle stays usable);
 * -100 = HIP failure, a bad device included.  All but -100 are found before the device is touched.  n == 0 and n_q == 0 are legal. */
typedef struct mpmvs_cloud mpmvs_cloud;
/* target cloud: n points, xyz = n x 3 fp32 (what a PLY holds); uploaded once, stays in HBM.  *cloud is NULL after a failure,
 * which leaves no allocation behind. */
int mpmvs_cloud_create(int device, long long n, const float* xyz, mpmvs_cloud** cloud);
/* per query point: squared distance to, and index of, its nearest target point within `radius`; host buffers, blocks until
 * done; n_q == 0 returns 0 and touches no output */
int mpmvs_cloud_nearest(mpmvs_cloud* cloud, float radius, long long n_q, const float* q_xyz, float* out_d2, int32_t* out_idx /* may be NULL */);
/* stats of the grid of the last call: [0] finite target points, [1] occupied cells, [2] points in the fullest cell, [3] table slots */
int mpmvs_cloud_stats(const mpmvs_cloud* cloud, long long stats[4]);
/* device ms (HIP events) of the last call's query passes (the binning of the queries and the query kernel); *build_ms (may be
 * NULL) of the grid build it needed (0 if reused) */
float mpmvs_cloud_kernel_ms(const mpmvs_cloud* cloud, float* build_ms);
void mpmvs_cloud_destroy(mpmvs_cloud* cloud);

/* ---- point clouds: voxel-grid downsampling (mp-mvs_amd/cloud.py, tools/downsample_ply.py, tools/eval_ply.py --voxel) --- */
/* One output point per occupied cell of a uniform grid of edge `voxel`: the mean position, the normalised sum of the normals and
 * the rounded mean colour of the cell's members, as the Tanks and Temples and ETH3D protocols resample both clouds before they
 * measure, so that a score does not weigh a surface by how densely it was sampled.  A stateless call:
 * host buffers in and out, a stream of its own, blocks until done.  It returns the number m of occupied voxels, or a negative code.
 * *out_xyz (m x 3), *out_normals (m x 3, iff normals), *out_rgb (m x 3, iff rgb), *out_count (m) and *out_first (m) receive
 * buffers to release with mpmvs_free; on failure none is allocated and all are NULL; m == 0 (n == 0, or no point with three finite
 * coordinates) sets them to NULL too and launches nothing.  out_voxel_of is the caller's, n entries, and may be NULL.
 * DEFINED BY EQUIVALENCE with this plain loop, bit for bit and independent of scheduling (fp64 unless stated, no contraction):
 *   A point TAKES PART iff its three coordinates are finite; otherwise out_voxel_of[i] = -1.
 *   mn[a] = the minimum of the points that take part along axis a (fp32, found on the host as mpmvs_cloud_create finds it).
 *   e = (double)voxel;  o[a] = (double)mn[a] - 0.5 * e   (the usual origin rule: the lowest point lies at a cell centre).
 *   t_a = ((double)x_a - o[a]) / e;  c_a = floor(t_a): a point exactly on a cell border belongs to the upper cell.  o[a] <= mn[a],
 *   so c_a >= 0; every c_a must be below 2^21 (-3 otherwise, found on the host from the maximum along the axis).
 *   The voxels (occupied cells) are numbered in the order of their smallest member index, i.e. by first appearance in the input:
 *   out_first[v] = that index, out_count[v] = the number of members, out_voxel_of[i] = v.
 *   fix(x) = llrint(x * 2^30), round to nearest even.
 *   Position: every member adds fix(t_a - c_a) to the int64 S[v][a]; each term is at most 2^30 and a voxel has at most 2^31 - 1
 *     members: no overflow.  out_xyz[v][a] = (float)(o[a] + ((double)c_a + (double)S[v][a] / ((double)count * 2^30)) * e).
 *   Normals: a member whose normal has a non-finite component adds nothing; any other adds fix(max(-1, min(1, (double)n_a))) to the
 *     int64 N[v][a].  L = sqrt(((double)N0*N0 + (double)N1*N1) + (double)N2*N2);  out_normals[v][a] = (float)((double)N[v][a] / L),
 *     and 0.0f on all three axes when L == 0.
 *   Colour: C[v][k] = the integer sum of the members' bytes;  out_rgb[v][k] = (2 * C + count) / (2 * count) in integer division
 *     (round half up).
 * The sums are integers: the order in which the device adds them never shows.
 * Errors (text through mpmvs_last_error with a NULL context, per host thread): -2 = a NULL xyz with n > 0, a negative n, a voxel
 * that is not finite or <= 0, a NULL out_xyz, out_count or out_first, out_normals or out_rgb NULL while its input is given;
 * -3 = n above 2^31 - 1, more than 2^29 finite points (the hash table's limit, as for mpmvs_cloud_create), or the cell-span limit
 * above (the text names the axis and the ratio); -100 = HIP failure, a bad device included.  All but -100 are found before the
 * device is touched. */
long long mpmvs_cloud_voxel_downsample(int device, long long n, const float* xyz, const float* normals /* n x 3 or NULL */,
                                       const unsigned char* rgb /* n x 3 or NULL */, float voxel, float** out_xyz,
                                       float** out_normals /* NULL iff normals NULL */, unsigned char** out_rgb /* NULL iff rgb NULL */,
                                       int32_t** out_count, int32_t** out_first, int32_t* out_voxel_of /* caller's, n entries, may be NULL */);
/* device ms (HIP events) of the calling thread's last successful call, the sum of its passes; 0 when it launched nothing */
float mpmvs_cloud_voxel_ms(void);
/* the same per pass (mp-mvs_amd/csrc/pm_voxel.hpp): insert, first, flag + scan, number, accumulate, finish */
void mpmvs_cloud_voxel_pass_ms(float ms[6]);

/* ---- point clouds: k nearest neighbours and outlier removal (mp-mvs_amd/cloud.py, tools/clean_ply.py) --- */
/* The k nearest targets of every query within a radius (mp-mvs_amd/csrc/pm_knn.hpp).
 * DEFINED BY EQUIVALENCE with brute force, bit for bit and independent of scheduling, on the candidate rule of mpmvs_cloud_nearest:
 *   r2 = radius * radius in fp32;  d2 = (dx*dx + dy*dy) + dz*dz in fp32, no contraction;  a target is a candidate iff all its
 *   coordinates are finite and d2 <= r2.
 *   q_xyz == NULL: the queries are the handle's own n points (n_q must equal n), and target i is NOT a candidate of query i.  The
 *   exclusion is by index, not by distance: an exact duplicate of point i is a neighbour at d2 = +0.
 *   Row i of out_d2 / out_idx (k entries each) holds the min(k, candidates) lexicographically smallest pairs (d2 bits, index) in
 *   ascending order, the rest of the row +inf / -1.  out_within[i] = the number of ALL candidates, not capped by k.
 *   A query with a non-finite coordinate: a row of +inf / -1 and within = 0.
 * The call uses the handle's grids and their per-radius cache: a radius built by mpmvs_cloud_nearest or an align pass is not built
 * again.  The queries are served in chunks of 2^23 / k (2^18 at k = 32), so the device holds at most 2^23 list entries -- 64 MB
 * with indices -- however many queries there are.
 * Errors: -2 = a NULL cloud or out_d2, k outside [1, MPMVS_KNN_MAX_K], n_q < 0, a NULL q_xyz with n_q != n, a radius that is not
 * finite or <= 0; -3 = the limits of mpmvs_cloud_nearest; -100 = HIP failure.  All but -100 are found before the device is touched.
 * n_q == 0 returns 0 and writes nothing. */
#define MPMVS_KNN_MAX_K 32
int mpmvs_cloud_knn(mpmvs_cloud* cloud, float radius, int k, long long n_q, const float* q_xyz /* NULL: the cloud's own points */,
                    float* out_d2 /* n_q x k */, int32_t* out_idx /* n_q x k, may be NULL */, int32_t* out_within /* n_q, may be NULL */);
/* device ms (HIP events) of the last mpmvs_cloud_knn call's query passes, all chunks; *build_ms (may be NULL) of the grid build it
 * needed (0 if reused) */
float mpmvs_cloud_knn_ms(const mpmvs_cloud* cloud, float* build_ms);

/* Statistical and radius outlier removal in one pass over the self-excluded k nearest neighbours.  A stateless call like
 * mpmvs_cloud_voxel_downsample: host buffers in and out, a stream of its own, blocks until done.  It returns the number of points
 * kept, or a negative code.  DEFINED BY this plain loop (fp64 unless stated, no contraction):
 *   A point TAKES PART iff its three coordinates are finite.  For point i take the answer of mpmvs_cloud_knn with q_xyz == NULL at
 *   `radius`.  Fewer than k candidates: mean[i] = +inf (fp32), the point is ISOLATED.  Otherwise s = sqrt((double)d2_0), then
 *   s = s + sqrt((double)d2_j) for j = 1 .. k - 1 in ascending list order, mean[i] = (float)(s / (double)k) (IEEE sqrt and quotient).
 *   A point that does not take part has mean = +inf and within = 0.
 *   Over the c points with a finite mean: a_i = (double)mean[i] / (double)radius;  fix(x) = llrint(x * 2^30);
 *   S1 = sum of fix(a_i), S2 = sum of fix(a_i * a_i) in int64 (a_i is at most slightly above 1 and c <= 2^31 - 1: no overflow; the
 *   sums are integers, so their order never shows);  den = (double)c * 2^30;  mu = (double)S1 / den;
 *   var = max(0, (double)S2 / den - mu * mu) (the population variance);  sigma = sqrt(var);
 *   T = (mu + std_ratio * sigma) * (double)radius, and T = +inf outright when std_ratio is +inf;  c == 0: mu = sigma = T = 0.
 *   keep[i] = 1 iff mean[i] is finite and (double)mean[i] <= T and within[i] >= min_within (min_within = 0 switches the radius
 *   rule off), else 0.
 *   counts = {points taking part, c, kept};  stats = {mu * radius, sigma * radius, T}.
 * Errors: -2 = a NULL xyz or out_keep with n > 0, a negative n, a radius that is not finite or <= 0, k outside
 * [1, MPMVS_KNN_MAX_K], a std_ratio that is negative or NaN, min_within < 0; -3 = the limits of mpmvs_cloud_create and of a grid:
 * n above 2^31 - 1, more than 2^29 finite points, a finite bounding box of more than 2^21 cells along an axis at this radius (the
 * text names the axis and the ratio); -100 = HIP failure, a bad device included.  All but -100 are found before the device is
 * touched.  n == 0, or no point that takes part, returns 0, writes an all-zero keep and launches nothing. */
long long mpmvs_cloud_outliers(int device, long long n, const float* xyz, float radius, int k, double std_ratio, int min_within,
                               unsigned char* out_keep /* n */, float* out_mean /* n, may be NULL */, int32_t* out_within /* n, may be NULL */,
                               long long counts[3] /* may be NULL */, double stats[3] /* may be NULL */);
/* device ms (HIP events) of the calling thread's last successful call: the grid build and the query passes; 0 when it launched nothing */
float mpmvs_cloud_outliers_ms(void);

/* ---- point clouds: normals from the k nearest neighbours (mp-mvs_amd/cloud.py, tools/normals_ply.py) --- */
/* A surface normal and a curvature per point of the handle's cloud, fitted to its k nearest neighbours within a radius
 * (mp-mvs_amd/csrc/pm_normals.hpp).  DEFINED BY EQUIVALENCE with this plain loop, bit for bit and independent
 * of scheduling.  The arithmetic is fp64 unless stated, with no contraction, and uses only + - * / sqrt fabs and comparisons; -x
 * changes the sign bit;  max0(x) = x > 0 ? x : +0.
 *   NEIGHBOURHOOD.  For point i = (p_0, p_1, p_2) with finite coordinates take the answer of mpmvs_cloud_knn with q_xyz == NULL at
 *   `radius` and `k` (point i is not its own neighbour; an exact duplicate of it is).  m = min(k, within[i]);  out_within[i] is that
 *   call's within.  A point with a non-finite coordinate has m = 0 and within = 0.
 *   SUMS over the m list entries j in ascending list order:  e_j[a] = (double)p_idx_j[a] - (double)p_i[a] (exact: both are fp32);
 *   s_a = sum of e_j[a];  Q_ab = sum of e_j[a] * e_j[b] for the six a <= b; the first term initialises each sum and the others are
 *   added in list order.  C_ab = Q_ab - (s_a * s_b) / (double)(m + 1): the scatter matrix of the m neighbours and the point itself
 *   about their mean, written about p_i so that nothing large cancels.
 *   EIGENVECTORS by cyclic Jacobi: A = C (symmetric), V = identity; exactly 8 sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r
 *   the third index.  A pair with a_pq == 0 is skipped.  Otherwise
 *     theta = (a_qq - a_pp) / (2.0 * a_pq);  t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
 *     c = 1.0 / sqrt(t * t + 1.0);  s = t * c;
 *     a_pp <- a_pp - t * a_pq;  a_qq <- a_qq + t * a_pq;  a_pq <- 0;
 *     a_rp <- c * a_rp - s * a_rq;  a_rq <- s * a_rp + c * a_rq   (both from the old values);
 *     for each row i of V:  v_ip <- c * v_ip - s * v_iq;  v_iq <- s * v_ip + c * v_iq   (both from the old values).
 *   PICK.  d = (a_00, a_11, a_22);  i0 = the index of the smallest d, ties to the lowest index;  d_mid = the smaller of the other
 *   two;  tr = (max0(d_0) + max0(d_1)) + max0(d_2).
 *   The normal is DEFINED iff m >= 2 and d_mid > 0.  Undefined -- a non-finite point, fewer than two neighbours, all neighbours on the
 *   point or on one exact line through it -- gives out_normals = 0 0 0 and out_curvature = +inf.  A neighbourhood that is collinear
 *   only up to rounding can pass, with an arbitrary but still deterministic normal across the line; its curvature says so (the
 *   surface variation of a line is that of a perfect plane, 0 up to rounding, and d_mid is at the rounding level of the largest d).
 *   Defined: n = column i0 of V;  out_curvature[i] = (float)(max0(d_i0) / tr), the "surface variation", in [0, 1/3] up to rounding.
 *   SIGN.  Canonical: if the component of n with the largest fabs (ties: the lowest index) is < 0, n <- -n.  orient == 0: that is
 *   all.  orient == 1: w_a = view[a] - (double)p_i[a];  dot = (n_0 * w_0 + n_1 * w_1) + n_2 * w_2;  n <- -n iff dot < 0: the normal
 *   looks at the scanner.  orient == 2: the same with w_a = (double)ref_normals[3 i + a].  A NaN or zero dot keeps the canonical sign.
 *   out_normals[3 i + a] = (float)n_a.
 * The call uses the handle's grids and their per-radius cache exactly as mpmvs_cloud_knn does.  One launch serves all n points (at
 * most 20 bytes are written per point); the reference normals, when given, are uploaded once per call.
 * Errors: -2 = a NULL cloud or out_normals, k outside [2, MPMVS_KNN_MAX_K], a radius that is not finite or <= 0, orient outside
 * 0..2, orient == 1 with a NULL or non-finite view, orient == 2 with NULL ref_normals; -3 = the grid's limits, as for
 * mpmvs_cloud_knn; -100 = HIP failure.  All but -100 are found before the device is touched.  n == 0 returns 0 and writes nothing. */
int mpmvs_cloud_normals(mpmvs_cloud* cloud, float radius, int k, int orient, const double view[3] /* orient == 1 */,
                        const float* ref_normals /* n x 3, orient == 2 */, float* out_normals /* n x 3 */,
                        float* out_curvature /* n, may be NULL */, int32_t* out_within /* n, may be NULL */);
/* device ms (HIP events) of the last mpmvs_cloud_normals call's query passes (binning and kernel); *build_ms (may be NULL) of the
 * grid build it needed (0 if reused): what mpmvs_cloud_knn_ms reports of a knn call */
float mpmvs_cloud_normals_ms(const mpmvs_cloud* cloud, float* build_ms);

/* ---- point clouds: connected components within a radius (mp-mvs_amd/cloud.py, tools/clean_ply.py --cluster_radius) --- */
/* Euclidean cluster extraction: the connected components of the graph "two points of the handle's cloud are neighbours iff they are
 * within a radius" (mp-mvs_amd/csrc/pm_components.hpp), so that the small detached clusters of a fused cloud,
 * which the outlier rules above keep because every point of such a cluster has close neighbours, can be told by their size.
 * DEFINED BY EQUIVALENCE with this plain loop, bit for bit and independent of scheduling:
 *   A point TAKES PART iff its three coordinates are finite.
 *   Points i != j that both take part are ADJACENT iff d2 <= r2, on the candidate rule of mpmvs_cloud_nearest: r2 = radius * radius
 *   in fp32;  dx = x_i - x_j, likewise dy, dz, in fp32;  d2 = (dx*dx + dy*dy) + dz*dz in fp32, no contraction; the comparison is
 *   inclusive.  The rule is SYMMETRIC: x_i - x_j and x_j - x_i are exact negatives of each other (a correctly rounded difference
 *   changes sign with its operands), the squares of exact negatives are equal, and the two sums add equal terms in the same order.
 *   Adjacency is therefore an undirected graph, and its connected components are defined.
 *   out_label[i] = the SMALLEST INDEX among the points of i's connected component; -1 for a point that does not take part.  An exact
 *   duplicate of a point is adjacent to it at d2 = +0.  A point without a neighbour is a component of its own: out_label[i] = i.
 *   out_size[i] = the number of points of that component; 0 for a point that does not take part.
 *   counts = {points taking part, components, size of the largest component, label of the largest component}; among components of
 *   equal size the smallest label counts as the largest.  No point taking part: counts = {0, 0, 0, -1}.
 * The labels are what a union-find over all adjacent pairs gives, in any order of the pairs: the device unites them concurrently in
 * one pass, without locks (DESIGN.md section 20 has the argument).  The call uses the handle's grids and their per-radius cache
 * exactly as mpmvs_cloud_knn does: a radius built by mpmvs_cloud_nearest, mpmvs_cloud_knn, mpmvs_cloud_normals or an align pass is not
 * built again.  The handle keeps n ints of scratch from the first call on, released with the handle.
 * Errors: -2 = a NULL cloud, a NULL out_label with n > 0, a radius that is not finite or <= 0; -3 = the limits of
 * mpmvs_cloud_nearest (the cell span at this radius; the text names the axis and the ratio); -100 = HIP failure.  All but -100 are
 * found before the device is touched, and a refused call writes nothing.  n == 0, or no point that takes part, returns 0, writes
 * -1 / 0 into the outputs and launches nothing. */
int mpmvs_cloud_components(mpmvs_cloud* cloud, float radius, int32_t* out_label /* n */, int32_t* out_size /* n, may be NULL */,
                           long long counts[4] /* may be NULL */);
/* device ms (HIP events) of the last mpmvs_cloud_components call, the sum of its passes; *build_ms (may be NULL) of the grid build it
 * needed (0 if reused) */
float mpmvs_cloud_components_ms(const mpmvs_cloud* cloud, float* build_ms);
/* the same per pass: hook (the initialisation, the binning and the union-find pass over the edges), flatten, size (0 when neither
 * out_size nor counts was asked for) */
int mpmvs_cloud_components_pass_ms(const mpmvs_cloud* cloud, float ms[3]);

/* ---- point clouds: z-buffer render into cameras (mp-mvs_amd/cloud.py, tools/eval_depth.py) --- */
/* The per-view ground-truth depth map of a scan: the handle's cloud rendered into n_views pinhole cameras with a visibility test,
 * so that the back of the scene does not shine through the gaps between front points.
 * DEFINED BY EQUIVALENCE with the plain-loop statement, bit for bit and independent of scheduling.  For view v with camera c
 * (K, R, t row-major, W = c.width, H = c.height; depth_min / depth_max unused) and point i = (p0, p1, p2), everything in fp32, no
 * contraction, correctly rounded quotients (project_depth of mp-mvs_amd/csrc/pm_device.hpp):
 *   t0 = ((R0*p0 + R1*p1) + R2*p2) + t[0], t1 and t2 alike;  z = (K6*t0 + K7*t1) + K8*t2;
 *   u = ((K0*t0 + K1*t1) + K2*t2) / z;  v = ((K3*t0 + K4*t1) + K5*t2) / z;  fu = u + 0.5f, fv = v + 0.5f (pixel centres at integers).
 *   The point is IN VIEW iff its three coordinates are finite, z is finite and z > 0, fu >= 0, fu < (float)W, fv >= 0 and
 *   fv < (float)H (a comparison with a NaN is false); then px = (int)fu, py = (int)fv.
 *   Zc[y][x] = the smallest z of the in-view points with (px, py) = (x, y); +inf if there is none.
 *   Z1[y][x] = the smallest Zc[y'][x'] over |x' - x| <= splat, |y' - y| <= splat inside the image.
 *   m = 1.0f + occl_rel.
 *   depth[y][x] = Zc[y][x] if it is finite and Zc[y][x] <= Z1[y][x] * m (an fp32 product), else 0.0f ("no depth").
 *   idx[y][x] = the smallest i among the in-view points of that pixel whose z has the bits of Zc[y][x] where depth != 0, else -1.
 * In point terms: a point is hidden if some point whose pixel lies within Chebyshev distance splat of its own is nearer by more
 * than the factor m; the nearest visible point of a pixel wins, and if the nearest point of a pixel is hidden so are all its others.
 * splat = 0 is the plain z-buffer.  THE SLOPE RULE: a slanted surface hides itself once occl_rel is below splat x the relative
 * change of depth per pixel along the surface; raise occl_rel with splat on steep or close scenes.  The defaults of the Python
 * layer (splat 1, occl_rel 0.02) are starting values from the synthetic scene only.
 * Host buffers in and out: out_depth[v] holds H*W floats, out_idx (NULL, or NULL entries: not wanted) H*W int32.  Blocks until done.
 * n_views == 0 returns 0 and touches nothing; a cloud without a finite point gives all 0.0f / -1 without touching the device.
 * Views may differ in size; any n_views is served, a few views per launch.  The handle's search grids are not touched.
 * Errors (text through the last-error call with a NULL context): -2 = a NULL cloud, n_views < 0, splat outside
 * [0, MPMVS_RENDER_MAX_SPLAT], occl_rel not finite or < 0 (these four are checked first, also for n_views == 0), NULL cams or
 * out_depth, a NULL out_depth[v], a non-positive width or height; -3 = a width or height above 2^24, a view of more than
 * 2^31 - 1 pixels; -100 = HIP failure.  All but -100 are found before the device is touched. */
#define MPMVS_RENDER_MAX_SPLAT 8
int mpmvs_cloud_render_depth(mpmvs_cloud* cloud, int n_views, const mpmvs_camera* cams, int splat, float occl_rel, float* const* out_depth,
                             int32_t* const* out_idx /* NULL, or NULL entries: not wanted */);
/* device ms (HIP events) of the last render call's kernels, all chunks of views added up */
float mpmvs_cloud_render_ms(const mpmvs_cloud* cloud);
/* the same per pass: ms[0] z-min, ms[1] index (0 when no index map was wanted), ms[2] resolve */
int mpmvs_cloud_render_pass_ms(const mpmvs_cloud* cloud, float ms[3]);

/* ---- point clouds: the space a scan's scanners observed (mp-mvs_amd/cloud.py: Observer, tools/eval_ply.py --scanners) --- */
/* A terrestrial scanner observed the segment from its own position to every surface sample: that is free space.  A reconstruction
 * point inside it and far from every scan point is certainly wrong; a point beyond the surface, or along a ray that returned
 * nothing, lies in space nobody measured and says nothing about accuracy.  Per scanner position the handle keeps a range image
 * over the full sphere, as a cube map of six R x R faces, made from a scan on the device; any number of query points are then
 * classified per scanner as free, covered but not free, or not covered (mp-mvs_amd/csrc/pm_observe.hpp).
 * This is the project's own formulation of observed-space masking, not a port of ETH3D's program and not verified against it.
 * DEFINED BY EQUIVALENCE with this plain-loop statement, bit for bit and independent of scheduling; everything is fp32 without
 * contraction and with correctly rounded quotients.  Scanner j sits at S_j (three finite numbers), R = face_size, w = window.
 *   FACE AND PIXEL of a point p for scanner j:  d_a = p_a - S_j,a for each axis a (one subtraction), A_a = |d_a|;  m = the lowest
 *   axis index that attains max(A_0, A_1, A_2);  z = A_m.  The point TAKES PART iff its three coordinates are finite, z is finite
 *   and z > 0 (a difference that overflows, and the scanner's own position, take no part).  face f = 2 m + (d_m < 0 ? 1 : 0);
 *   b = (m + 1) % 3, c = (m + 2) % 3;  h = (float)R * 0.5f;  x = h * (d_b / z) + h,  y = h * (d_c / z) + h: a quotient, a product
 *   and a sum, each rounded.  |d_b| <= z and the quotient is correctly rounded, so 0 <= x <= R.
 *   px = x >= (float)R ? R - 1 : (int)x, py alike: every point that takes part has exactly one face and one pixel per scanner.
 *   MAPS.  Zc[j][f][py][px] = the smallest z of the scan points that take part for j and land in that pixel; +inf if none.
 *   owner == NULL: every scan point takes part for every scanner.  owner given (int32 [n], n the count of the cloud handle): point i
 *   enters the maps of scanner owner[i] only, and of none when owner[i] == -1.
 *   Zn[j][f][y][x] = the smallest Zc[j][f][y'][x'] over |x' - x| <= w, |y' - y| <= w clipped to the same face.  The window does not
 *   cross onto the neighbouring faces: a stated simplification, near a face edge the test is a little less conservative.
 *   window == 0 gives Zn == Zc.
 *   CLASSIFICATION of a query q for scanner j with the margins rel (finite, in [0, 1)) and abs_margin (finite, >= 0):
 *   q is COVERED iff it takes part and Zn at its (face, pixel) is finite;  q is FREE iff it is covered and
 *   z + abs_margin < Zn * (1.0f - rel): each side one rounded operation after the rounded 1.0f - rel.
 *   out_free[q] = the number of scanners for which q is free, out_covered[q] (may be NULL) for which it is covered; a query with a
 *   non-finite coordinate has 0 and 0.
 * mpmvs_observer_create reads the resident points of the cloud handle (the scan is uploaded once for the searches and for this),
 * during the call only: the observer keeps no reference, and destroying the cloud afterwards is legal.  The cloud's search grids and
 * their cache are not touched.  Only Zn stays resident (scanners x 6 R^2 floats); Zc is scratch of the call, for a few scanners at a
 * time.  *out is NULL after a failure, which leaves no allocation behind.  A scan without a finite point is legal: every pixel is
 * +inf and nothing is covered.  Host buffers in and out; every call blocks until done; n_q == 0 is legal and writes nothing.
 * Errors (text through mpmvs_last_error with a NULL context, per host thread): -2 = a NULL handle or required pointer, n_scanners
 * outside [1, MPMVS_OBSERVE_MAX_SCANNERS], a non-finite scanner coordinate, face_size outside [1, MPMVS_OBSERVE_MAX_FACE], window
 * outside [0, MPMVS_OBSERVE_MAX_WINDOW], an owner value that is neither -1 nor a scanner, rel or abs_margin out of range, a negative
 * n_q, a scanner index out of range in mpmvs_observer_maps; -3 = n_scanners * 6 * face_size^2 above 2^31 pixels, n_q above 2^31 - 1;
 * -100 = HIP failure.  All but -100 are found before the device is touched. */
#define MPMVS_OBSERVE_MAX_SCANNERS 64
#define MPMVS_OBSERVE_MAX_FACE 4096
#define MPMVS_OBSERVE_MAX_WINDOW 8
typedef struct mpmvs_observer mpmvs_observer;
int mpmvs_observer_create(mpmvs_cloud* scan, int n_scanners, const float* scanners_xyz /* n_scanners x 3 */, const int* owner /* n, or NULL */,
                          int face_size, int window, mpmvs_observer** out);
int mpmvs_observer_classify(mpmvs_observer* obs, long long n_q, const float* q_xyz, float rel, float abs_margin, int* out_free /* n_q */,
                            int* out_covered /* n_q, may be NULL */);
/* Zn of one scanner: 6 * R * R floats, face-major, +inf = nothing */
int mpmvs_observer_maps(mpmvs_observer* obs, int scanner, float* out_near);
/* out[0] = the pixels with a finite Zn, out[1] = all pixels (n_scanners * 6 * R^2) */
int mpmvs_observer_stats(mpmvs_observer* obs, long long out[2]);
/* device ms (HIP events) of the last classify call's kernel, all launches; build_ms (may be NULL) receives those of the create's two
 * passes, all chunks of scanners added up: [0] z-min, [1] window minimum */
float mpmvs_observer_ms(mpmvs_observer* obs, float build_ms[2]);
void mpmvs_observer_destroy(mpmvs_observer* obs);

/* ---- point clouds: registration to a target handle, ICP on the device (mp-mvs_amd/cloud.py, tools/eval_ply.py --refine) --- */
/* Point-to-point ICP with an optional scale, as the Tanks and Temples protocol refines a given alignment before it measures
 * (DESIGN.md section 15).  The moving ("source") cloud is uploaded once per align handle; a PASS transforms it on the device by
 * M (12 doubles, row-major 3 x 4: A = M[:, :3], t = M[:, 3]), takes every transformed point's nearest target within `radius`
 * and reduces the matched pairs to 18 integers; per pass 12 doubles go up and 18 int64 come down.
 * THE PASS IS DEFINED BY EQUIVALENCE with this plain loop, bit for bit and independent of scheduling:
 *   frame (from the target's finite bounding box mn, mx and the radius, on the host, in fp64):
 *     o[a] = 0.5 * ((double)mn[a] + (double)mx[a]);  h = 0.5 * max_a((double)mx[a] - (double)mn[a]) + 2.0 * (double)radius;
 *     u = the smallest power of two >= h;  iu = 1 / u;  frame = {o[0], o[1], o[2], u}.
 *   per source point s (fp64 unless stated, no contraction); it is skipped if one of its coordinates is not finite:
 *     y_k = (float)(((A[k][0]*sx + A[k][1]*sy) + A[k][2]*sz) + t[k]),  k = 0, 1, 2;
 *     (d2, j) = the answer of the nearest-neighbour statement above for the query y at this radius; no candidate: skipped;
 *     a = ((double)y - o) * iu;  b = ((double)p_j - o) * iu   (every component is at most 1 in magnitude by the choice of u);
 *   fix(x) = llrint(x * 2^30), round to nearest even; every matched source adds
 *     1 to sums[0];  fix(a_k) to sums[1 + k];  fix(b_k) to sums[4 + k];  fix(a_i * b_j) to sums[7 + 3 i + j];
 *     fix((a_x*a_x + a_y*a_y) + a_z*a_z) to sums[16];  fix((double)d2 * (iu * iu)) to sums[17].
 *   Every |term| <= 3 and at most 2^31 - 1 sources add one, so every |sum| < 3 * 2^61: no overflow.  The sums are integers:
 *   the order in which the device adds them never shows.
 * THE SOLVE is host code and never touches a device: Umeyama's closed form in fp64 in the normalised frame (means, cross-
 * covariance and source variance from the sums, rotation from a 3 x 3 Jacobi SVD with the determinant sign fix, scale 1 unless
 * with_scale), mapped back to world units through o and u as an update D and composed as M_out = D * M_in.
 * *rmse (may be NULL) = sqrt(sums[17] / 2^30 / n) * u: the RMS distance of the matched pairs BEFORE the update (0 if n = 0).
 * It returns 1 and sets M_out = M_in when fewer than 3 pairs matched, when the source variance is <= 0 or when the largest
 * singular value is 0; anything else is answered as the formula gives it.  Collinear pairs leave a rotation about their line
 * open: they are the caller's problem.
 * THE ICP CALL is this loop of the two calls above and nothing else: run a pass at M, solve; M = M_out; stop after the solve
 * whose update D (what the solve returns for M_in = identity) moves none of the 8 corners o +- u of the frame's box by more than
 * eps (x' = ((D[k][0]*x0 + D[k][1]*x1) + D[k][2]*x2) + D[k][3], distance = sqrt((dx*dx + dy*dy) + dz*dz), fp64), after
 * max_iter passes, or at a solve that returns 1.  *iters = passes run, *inliers = sums[0] and *rmse of the last pass (each may
 * be NULL).  Its M equals the caller's own loop over the two calls in every bit.  When a pass inside the loop fails (a HIP failure,
 * or -2 because an update took M out of the finite numbers) the call returns that code at once: M_inout holds the transform
 * that pass was given, and *iters, *inliers and *rmse are not written.
 * The handle BORROWS the target: the target must outlive it, and calls on the two handles must not run concurrently.  A pass
 * uses the target's grids and their per-radius cache (a radius used by a nearest-neighbour call before is not built again).
 * Errors: -2 = NULL arguments, a negative count, a radius that is not finite or <= 0, a non-finite M, max_iter < 1, an eps that is
 * negative or NaN; -3 = n_s above 2^31 - 1, or the cell-span limit of the nearest-neighbour call; -100 = HIP failure.  All but -100
 * are found before the device is touched.  n_s == 0 gives all-zero sums, a target without a finite point all-zero sums and an
 * all-zero frame; neither launches anything. */
typedef struct mpmvs_align mpmvs_align;
int mpmvs_align_create(mpmvs_cloud* target, long long n_s, const float* s_xyz, mpmvs_align** h);
int mpmvs_align_sums(mpmvs_align* h, float radius, const double M[12], long long sums[18], double frame[4]);
int mpmvs_align_solve(const long long sums[18], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse);
int mpmvs_align_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M_inout[12], long long* iters,
                    long long* inliers, double* rmse);
/* device ms (HIP events) of the last pass of either kind (point-to-point or point-to-plane): binning + kernel; 0 when the pass
 * launched nothing */
float mpmvs_align_ms(const mpmvs_align* h);
void mpmvs_align_destroy(mpmvs_align* h);

/* Point-to-plane ICP on the same handle (mp-mvs_amd/csrc/pm_align_plane.hpp, pm_align_host.hpp): the
 * residual of a pair is its distance along the TARGET's normal, so a source may slide along a surface whose samples are not its
 * own -- what point-to-point ICP cannot do when the two clouds sample the same surfaces at different points.  The calls above
 * are untouched by these: both kinds of pass may be mixed on one handle.
 * TARGET NORMALS.  mpmvs_align_set_normals takes n_t x 3 floats in the target's caller order (n_t = the count the target handle
 * was created with; e.g. the output of mpmvs_cloud_normals) and uploads them once onto the ALIGN handle, which owns the buffer; the
 * target handle is untouched, so two align handles on one target may hold different normals.  A second call replaces them, NULL
 * drops them.  Neither the sign nor the length of a normal matters.
 * THE PASS IS DEFINED BY EQUIVALENCE with this plain loop, bit for bit and independent of scheduling.  The frame, y, (d2, j), a, b
 * and iu are exactly those of mpmvs_align_sums, and a source is skipped for the same reasons as there.  It is also skipped when
 * the normal of target j is unusable:  n = (double)nrm_j,  q = (n0*n0 + n1*n1) + n2*n2;  unusable iff q is not finite or q == 0
 * (the undefined 0 0 0 of mpmvs_cloud_normals drops out here).  Otherwise, in fp64 without contraction, with + - * / sqrt only:
 *     nh_k = n_k / sqrt(q);   e = a - b;   r = (e0*nh0 + e1*nh1) + e2*nh2;
 *     c = a x nh:  c0 = a1*nh2 - a2*nh1,  c1 = a2*nh0 - a0*nh2,  c2 = a0*nh1 - a1*nh0;   g = (a0*nh0 + a1*nh1) + a2*nh2;
 *     J = (c0, c1, c2, nh0, nh1, nh2, g)
 *   and with fix as above the matched source adds
 *     1 to sums[0];  fix(J_i * J_j) for i <= j, row by row (00 01 .. 06 11 12 .. 66), to sums[1..28];  fix(J_i * r) to sums[29 + i];
 *     fix(r * r) to sums[36];  fix((double)d2 * (iu * iu)) to sums[37].
 *   OVERFLOW.  |a_k| <= 1 as above and |nh_k| <= 1, so |c_k| <= sqrt 2 and |g| <= sqrt 3.  A matched y is within
 *   radius (1 + 4 * 2^-24) of its target along every axis and u >= 2 radius, so |e_k| <= (1 + 4 * 2^-24) / 2 and |r| < 0.87.
 *   Every |term| is at most 3 up to rounding and strictly below 4; at most 2^31 - 1 sources contribute, so every
 *   |sum| <= 2^32 (2^31 - 1) < 2^63.
 *   SIGN.  Negating a normal negates nh, c, g and r exactly, and every term is a product of two of them: flipping any or all of the
 *   normals leaves all 38 sums unchanged in every bit.
 * THE SOLVE is host code and never touches a device: one Gauss-Newton step in the normalised frame.  s = 2^-30;  H = J^T J (7 x 7,
 * symmetric) from sums[1..28] * s and gvec = J^T r from sums[29..35] * s;  m = 7 with scale, else the leading 6;  H x = -gvec by
 * LDL^T without pivoting, x = (omega[3], t[3], sigma);  pivot j is d_j = H_jj - sum over k < j of L_jk^2 d_k.  It returns 1 and sets
 * M_out = M_in when fewer than m pairs matched, when a pivot is not finite, when a pivot is <= 2^-20 times the diagonal entry H_jj
 * it started from (a direction the pairs do not observe: one plane, two parallel planes, the scale about the apex of a three-plane
 * corner; the rounding of a sum is at most n 2^-31 against a diagonal of n mean(J_j^2), so a pivot that small is rounding), or when,
 * with scale, 1 + sigma is not a positive finite number.  Otherwise R = the rotation of the unit quaternion
 * (1, omega / 2) / |(1, omega / 2)| -- a proper rotation for every omega, with one sqrt --, c = 1 + sigma (1 without scale), and the
 * update maps back and composes exactly as in mpmvs_align_solve:  D = [c R | o - c R o + u t],  M_out = D * M_in.
 * *rmse_plane = sqrt(sums[36] / 2^30 / n) * u and *rmse_point = sqrt(sums[37] / 2^30 / n) * u: the RMS distance of the matched pairs
 * along the normals, and between the points, BEFORE the update (0 if n = 0).  Either pointer may be NULL.
 * THE ICP CALL is the loop of the two calls above and nothing else, with the stop rule and the failure semantics of mpmvs_align_icp
 * word for word: it stops after the solve whose update D moves none of the 8 corners o +- u by more than eps, after max_iter passes,
 * or at a solve that returns 1; *iters, *inliers (sums[0]), *rmse_plane and *rmse_point are those of the last pass (each may be
 * NULL); its M equals the caller's own loop over the two calls in every bit; a pass that fails inside the loop returns its code at
 * once, M_inout holds the transform that pass was given, and the four outputs are not written.
 * Errors: as for the point-to-point calls; in addition a plane pass or plane ICP on a handle without normals returns -2 before the
 * device is touched.  n_s == 0 gives all-zero sums, a target without a finite point all-zero sums and an all-zero frame; neither
 * launches anything.  mpmvs_align_set_normals: -2 = a NULL handle, -100 = HIP failure. */
int mpmvs_align_set_normals(mpmvs_align* h, const float* nrm /* n_t x 3, or NULL: drop them */);
int mpmvs_align_plane_sums(mpmvs_align* h, float radius, const double M[12], long long sums[38], double frame[4]);
int mpmvs_align_plane_solve(const long long sums[38], const double frame[4], int with_scale, const double M_in[12], double M_out[12],
                            double* rmse_plane, double* rmse_point);
int mpmvs_align_plane_icp(mpmvs_align* h, float radius, int with_scale, int max_iter, double eps, double M_inout[12], long long* iters,
                          long long* inliers, double* rmse_plane, double* rmse_point);

/* ---- surface: TSDF volume and marching tetrahedra (mp-mvs_amd/mesh.py, tools/mesh_ply.py) --- */
/* Depth maps to a triangle mesh: the maps are integrated into a dense truncated-signed-distance volume, and the zero level set is
 * extracted by marching tetrahedra on the Kuhn split of every cell (mp-mvs_amd/csrc/pm_tsdf.hpp).  Both calls
 * are DEFINED BY EQUIVALENCE with the plain loops below, bit for bit and independent of scheduling.
 *
 * THE VOLUME is a dense lattice of dims = (nx, ny, nz) sample points, x fastest: voxel (i, j, k) has the linear index
 * (k*ny + j)*nx + i and the position P_a = (float)((double)origin[a] + (double)i_a * (double)voxel) along axis a.  Per voxel the
 * handle keeps sum (fp32), weight (int32) and, with colour, four uint32: the B, G, R sums and their count.  A fresh handle is all
 * zero.  mpmvs_tsdf_create touches no device: the handle opens `device` with the first get, set, integrate or mesh call that passes
 * its argument checks (-100 from that call if it cannot).  Limits: every dim >= 1, n_vox <= 2^30 (-3), origin, voxel and trunc
 * finite, voxel and trunc > 0, the far corner of the lattice finite in fp32, device >= 0.
 *
 * mpmvs_tsdf_integrate, fp32 throughout, no contraction, correctly rounded quotients.  For every voxel, the views in call order --
 * successive calls continue the same sums, so two calls give the bits of one call with the concatenated view list -- and per view
 * with camera c (K, R, t row-major, W = c.width, H = c.height; C, depth_min, depth_max unused):
 *   1. xc = ((R[0]*Px + R[1]*Py) + R[2]*Pz) + t[0]; yc and z likewise from rows 1 and 2 of R and t[1], t[2].
 *   2. Skip unless z > 0.
 *   3. fu = ((K[0]*xc)/z + K[2]) + 0.5f and fv = ((K[4]*yc)/z + K[5]) + 0.5f.
 *   4. Skip unless fu >= 0 && fu < (float)W && fv >= 0 && fv < (float)H (a comparison with a NaN is false).
 *   5. ix = (int)floorf(fu), iy = (int)floorf(fv);  6. d = depth[iy*W + ix].
 *   7. Skip unless d is finite and d > 0.   8. s = d - z.   9. Skip if s < -trunc.
 *   10. sum += fminf(1.0f, s / trunc) and weight += 1.
 *   11. With colour, and only if also s <= trunc: the pixel's three bytes are added to the B, G, R sums and 1 to the count; a grey
 *       image (color_channels == 1) adds its byte to all three.
 * depths[v] holds H*W floats, colors[v] H*W*color_channels bytes, tightly packed; views may differ in size.  colors is NULL iff the
 * volume has no colour.  n_views == 0 returns 0 and touches nothing.  Blocks until done.
 * Errors: -2 = a NULL handle, n_views < 0, colours given to a volume without colour or missing for one with colour, color_channels
 * not 1 or 3 when colours are given, NULL cams or depths, a NULL depths[v] or colors[v], a non-positive width or height; -3 = a width
 * or height above 2^24, a view of more than 2^31 - 1 pixels, more than 2^23 views integrated over the handle's life (so that the
 * colour sums cannot overflow); -100 = HIP failure.  All but -100 are found before the device is touched.
 *
 * mpmvs_tsdf_get copies the volume out (color4 may be NULL), mpmvs_tsdf_set replaces it (tests, and volumes computed elsewhere); with
 * colour a NULL color4 in set clears the colour sums.  Weights may be anything: a negative weight is never valid.  -2 = a NULL handle,
 * sum or weight, or a color4 for a volume without colour.
 *
 * mpmvs_tsdf_mesh(min_weight):
 *   CORNERS.  A corner (voxel) is VALID iff weight >= min_weight, min_weight >= 1; its value is f = sum / (float)weight; it is
 *   INSIDE iff f < 0 (exact zero and NaN are outside).
 *   TETRAHEDRA.  Cell (i, j, k), i < nx-1, j < ny-1, k < nz-1, is cut into six tetrahedra, one per permutation (a, b, c) of the axes,
 *   in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx, with the vertices v0 = corner 000, v1 = v0 + e_a, v2 = v1 + e_b,
 *   v3 = corner 111.  A tetrahedron EMITS iff its four corners are valid and it has 1, 2 or 3 inside corners.
 *   EDGES AND VERTICES.  Mesh vertices sit on lattice edges (A, B), B = A + off, off one of the 7 SLOTS 100, 010, 001, 110, 101, 011,
 *   111 (as x y z); the edge is owned by voxel A.  A vertex exists iff at least one emitted triangle uses its edge.  Vertices are
 *   numbered by owner linear index ascending, then slot ascending.  Position: t = fA / (fA - fB), p_a = PA_a + t * (PB_a - PA_a),
 *   always from A to B, so every tetrahedron that uses the edge sees the same vertex.  Colour per channel from the corner means
 *   m = (float)sum_c / (float)count where count > 0: both corners have a mean: mA + t*(mB - mA); one has: that mean; neither: 128.
 *   The byte is (int)(val + 0.5f) (saturated to 0..255 and 0 for a NaN, which cannot arise while 0 <= t <= 1), written R, G, B.
 *   TRIANGLES, ordered by cell linear index, then tetrahedron 0..5, then triangle 0 / 1.  With e(p, q) the vertex on the edge
 *   between tetrahedron vertices p and q, and inside / outside corners listed in tetrahedron vertex order:
 *     1 inside {a}, outside o1 < o2 < o3:   (e(a,o1), e(a,o2), e(a,o3))
 *     3 inside a1 < a2 < a3, outside {o}:   (e(a1,o), e(a2,o), e(a3,o))
 *     2 inside a < b, outside c < d:        (e(a,c), e(a,d), e(b,d)) and (e(a,c), e(b,d), e(b,c))
 *   ORIENTATION.  Seen from outside (the positive side, where the cameras are) a triangle is counter-clockwise.  This is decided
 *   combinatorially per (tetrahedron, case): the winding for which (p1-p0) x (p2-p0) points from the mean of the inside corners to
 *   the mean of the outside corners WHEN EVERY VERTEX IS PUT AT THE MIDPOINT OF ITS EDGE; if the listed winding is the other one,
 *   the triangle's last two vertices are swapped.  The surface is combinatorially manifold and consistently oriented by
 *   construction; where invalid corners punch holes it has a boundary.
 *   ANCHOR: the 10 x 9 x 8 lattice with unit spacing, every corner valid, f = (float)(sqrt((i-4.3)^2 + (j-3.9)^2 + (k-3.4)^2) - 2.7)
 *   evaluated in fp64, gives 410 vertices, 1224 edges, 816 triangles.
 * Returns the vertex count; *out_xyz (n x 3 floats), *out_rgb (n x 3 bytes; NULL iff the volume has no colour), *out_tri (*n_tri x 3
 * int32) receive buffers to release with mpmvs_free.  An empty result returns 0 with *n_tri = 0 and all buffers NULL: a volume with a
 * dimension of 1 has no cell and launches nothing; a volume with nothing valid or without a sign change is found empty after the mark
 * and scan passes and launches no further pass.  On failure no buffer is allocated and the outputs are not written.
 * Errors: -2 = a NULL handle, out_xyz, out_tri or n_tri, min_weight < 1, out_rgb NULL for a volume with colour or given for one
 * without; -3 = more than 2^31 - 1 vertices or triangles (counted in 64 bits before anything is emitted; the handle stays usable);
 * -100 = HIP failure. */
typedef struct mpmvs_tsdf mpmvs_tsdf;
int mpmvs_tsdf_create(int device, const float origin[3], float voxel, const int dims[3], float trunc, int with_color, mpmvs_tsdf** h);
int mpmvs_tsdf_integrate(mpmvs_tsdf* h, int n_views, const mpmvs_camera* cams, const float* const* depths,
                         const unsigned char* const* colors /* NULL iff the volume has no colour */, int color_channels /* 1 or 3 (B,G,R) */);
int mpmvs_tsdf_get(mpmvs_tsdf* h, float* sum /* n_vox */, int32_t* weight /* n_vox */, uint32_t* color4 /* n_vox x 4: B G R sums, count; may be NULL */);
int mpmvs_tsdf_set(mpmvs_tsdf* h, const float* sum, const int32_t* weight, const uint32_t* color4);
long long mpmvs_tsdf_mesh(mpmvs_tsdf* h, int min_weight, float** out_xyz, unsigned char** out_rgb /* NULL iff no colour */, int32_t** out_tri,
                          long long* n_tri);
/* device ms (HIP events): ms[0] the kernels of the last integrate call, all chunks added up; ms[1..4] mark + count, scan, vertices,
 * triangles of the last mesh call (0 for a pass that did not run) */
int mpmvs_tsdf_pass_ms(const mpmvs_tsdf* h, float ms[5]);
void mpmvs_tsdf_destroy(mpmvs_tsdf* h);

/* ---- surface: the brick-sparse TSDF volume (mp-mvs_amd/mesh.py: SparseVolume, tools/mesh_ply.py --sparse) --- */
/* The same handle type with the same origin, voxel, dims, trunc and with_color, but dims are VIRTUAL: only bricks near the surface
 * exist (mp-mvs_amd/csrc/pm_tsdf_sparse.hpp).  There are two statements, A and B; everything else is the dense
 * statement above under a mask.  Both are bit for bit and independent of scheduling.
 *
 * GEOMETRY.  A BRICK is 8 x 8 x 8 voxels: brick (I, J, K) covers the voxels 8I..8I+7 on each axis, cut off at dims.  The BRICK GRID has
 * b_a = ceil(dims[a] / 8) bricks per axis; a brick's linear index is (K*by + J)*bx + I, a voxel's LOCAL INDEX within its brick
 * (lk*8 + lj)*8 + li.  A voxel EXISTS iff its brick is allocated; a voxel that does not exist has weight 0 and is never valid.
 * BRICK-MAJOR ORDER: bricks ascending by linear index, voxels within a brick ascending by local index.  This order replaces the
 * dense linear index wherever the dense contract orders things: vertices by owner then slot, triangles by cell then tetrahedron
 * then triangle.  Where bricks are stored is not observable; every output is in brick-major order.
 *
 * mpmvs_tsdf_create_sparse touches no device, like mpmvs_tsdf_create.  pad (in voxels) and max_bricks are fixed here.  Limits: every
 * dim >= 1, origin, voxel, trunc finite, voxel and trunc > 0, the far corner finite in fp32, device >= 0, pad finite and
 * 0 <= pad <= 8, max_bricks >= 1 (all -2); bx*by*bz <= 2^24, max_bricks <= 2^21 (2^30 voxels, the index width of the mesh scratch),
 * n_s <= 2^16 (all -3).  On failure *h is not written.
 *
 * A. ALLOCATE.  mpmvs_tsdf_allocate(h, n_views, cams, depths) allocates a set of bricks that is a pure function of its arguments (the
 * set is order-free).  fp32 with no contraction and correctly rounded quotients, except where a double is written out.
 *   n_s = max(1, (int)ceil(4.0*(double)trunc/(double)voxel)).
 *   A pixel (ix, iy) of a view (K, R, t, W, H as above) takes part iff d = depth[iy*W + ix] is finite and > 0.  For each such pixel
 *   and m = 0..n_s:
 *   1. z = (float)(((double)d - (double)trunc) + (double)m * ((2.0*(double)trunc)/(double)n_s)).  Skip unless z > 0.
 *   2. xc = (((float)ix - K[2]) * z) / K[0] and yc = (((float)iy - K[5]) * z) / K[4].  (The pixel centre is ix, not ix + 0.5: step 3
 *      of the integration adds 0.5 before floorf.)
 *   3. a = xc - t[0], b = yc - t[1], c = z - t[2];  P_x = (R[0]*a + R[3]*b) + R[6]*c,  P_y = (R[1]*a + R[4]*b) + R[7]*c,
 *      P_z = (R[2]*a + R[5]*b) + R[8]*c.
 *   4. g_a = (P_a - origin[a]) / voxel per axis a.  Skip the sample unless all three are finite.
 *   5. Per axis lo = floorf(g_a - pad), hi = floorf(g_a + pad).  Skip the sample if hi < 0 or lo > n_a - 1 on any axis (compared as
 *      the integers they are); clamp both to [0, n_a - 1]; mark every brick of the box [lo>>3 .. hi>>3]^3 (at most 27).
 *   Bricks already allocated stay, with their contents.  A new brick starts all zero.  If the call would raise the brick count above
 *   max_bricks it returns -3 and changes nothing: all views are marked and counted before any brick is committed.
 *   The argument checks and codes are those of mpmvs_tsdf_integrate (without the colours and the limit on the number of views);
 *   -2 on a dense handle; n_views == 0 returns 0 and touches nothing.  pad = 1.0 is the default of mesh.py and the tools, an untuned
 *   starting value.
 *
 * B. MASKED-DENSE EQUIVALENCE.
 *   mpmvs_tsdf_integrate on a sparse handle never allocates: it applies the eleven steps above, unchanged, to every existing voxel
 *   and to no other.  A brick holds exactly the dense sums of all views integrated since it was allocated.  With every allocate
 *   before the first integrate, the state is the dense volume with the non-existing voxels zeroed, however the view list is split
 *   over calls.
 *   mpmvs_tsdf_mesh on a sparse handle equals the dense mesh statement on the virtual lattice with the weight of every non-existing
 *   voxel set to 0, vertices and triangles renumbered into brick-major order.  Cells, tetrahedra, slots, t, colours, winding, the -3
 *   rule and the empty-result rule (also: a handle without a brick launches nothing) are the dense ones.  CONSEQUENCE: the sparse
 *   mesh is a sub-mesh of the dense mesh of the same views: the same vertex positions bit for bit and a subset of the triangles,
 *   never a different triangle.
 *
 * mpmvs_tsdf_bricks returns the brick count; *coords (may be NULL: count only) receives n x 3 (I, J, K) in ascending linear index,
 * to release with mpmvs_free, NULL when the count is 0.  mpmvs_tsdf_get_bricks copies n_bricks*512 entries per array in brick-major
 * order (color4 may be NULL); voxels cut off by dims read 0.  mpmvs_tsdf_set_bricks replaces the whole volume with the given bricks
 * (tests, and volumes computed elsewhere): coords strictly ascending by linear index and inside the grid (-2), n <= max_bricks (-3),
 * found before anything is written; entries of cut-off voxels are ignored and stored as 0; with colour a NULL color4 clears the
 * colour sums.  mpmvs_tsdf_sparse_stats: info = the brick count, max_bricks, the cells of the brick grid, the bytes of device memory
 * the handle holds between calls; ms = the device ms of the last allocate: marking (all chunks), scan + commit.
 * On a sparse handle mpmvs_tsdf_integrate, _mesh, _pass_ms and _destroy work as above; mpmvs_tsdf_get and _set return -2.  On a dense
 * handle allocate, bricks, get_bricks, set_bricks and sparse_stats return -2.  A NULL handle is -2 everywhere. */
int mpmvs_tsdf_create_sparse(int device, const float origin[3], float voxel, const int dims[3], float trunc, int with_color, float pad,
                             long long max_bricks, mpmvs_tsdf** h);
int mpmvs_tsdf_allocate(mpmvs_tsdf* h, int n_views, const mpmvs_camera* cams, const float* const* depths);
long long mpmvs_tsdf_bricks(mpmvs_tsdf* h, int32_t** coords);
int mpmvs_tsdf_get_bricks(mpmvs_tsdf* h, float* sum, int32_t* weight, uint32_t* color4);
int mpmvs_tsdf_set_bricks(mpmvs_tsdf* h, long long n, const int32_t* coords, const float* sum, const int32_t* weight, const uint32_t* color4);
int mpmvs_tsdf_sparse_stats(const mpmvs_tsdf* h, long long info[4], float ms[2]);

/* ---- surface: cleaning and shading an indexed triangle mesh (mp-mvs_amd/mesh.py: Mesh, tools/clean_mesh.py) --- */
/* A handle for an indexed triangle mesh resident on the device: n vertices (xyz fp32, optional rgb bytes) and m triangles of three
 * int32 indices, wherever it came from (mpmvs_tsdf_mesh, a PLY file).  Kernels and per-thread bodies: mp-mvs_amd/csrc/pm_mesh.hpp and
 * pm_unionfind.hpp; DESIGN.md section 24.  The three statements below are bit for bit and independent of scheduling.
 *
 * mpmvs_mesh_create touches no device and copies its inputs; the handle opens `device` with the first operation that passes its
 * argument checks and has something to do.  -2, with *h not written: a NULL h, n < 0 or m < 0, a NULL xyz with n > 0, a NULL tri with
 * m > 0, device < 0, a triangle with an index outside [0, n) (the text names the first such triangle and the index).  -3: n or m
 * above 2^30.  n == 0 and m == 0 are legal.  The mesh has colour iff rgb is not NULL.
 * Every refusal of an operation writes nothing and is found before the device is touched, except -100 (HIP failure).  An operation
 * with nothing to do (n == 0, or m == 0 where only triangles matter) answers on the host and launches nothing.  A NULL handle is -2
 * everywhere.
 *
 * 1. COMPONENTS.  mpmvs_mesh_components.  Two vertices are JOINED iff some triangle names both; a repeated index inside a triangle
 *    is legal and joins what it names.  The components are the classes of the transitive closure over all n vertices.
 *    Connectivity is BY INDEX, NOT BY POSITION: coincident vertices with different indices are not welded.
 *      out_label[v] = the smallest vertex index of v's component; a vertex that no triangle names has out_label[v] = v.
 *      out_verts[v] = the number of vertices of that component.
 *      out_tris[v]  = its number of triangles; a triangle belongs to the component of its first index.
 *      counts = {components with at least one triangle, vertices no triangle names, triangles of the largest component, its label}:
 *               largest by triangle count, among equals the smallest label; with m == 0 {0, n, 0, -1}.
 *    -2: a NULL handle, a NULL out_label with n > 0.  out_verts, out_tris and counts may be NULL.
 *
 * 2. AREA-WEIGHTED VERTEX NORMALS.  mpmvs_mesh_normals.  All in fp64, no contraction, only + - * / sqrt, comparisons and one llrint,
 *    each correctly rounded.
 *    1. A vertex is FINITE iff its three coordinates are.  ext = the largest per-axis (double)max - (double)min over the finite
 *       vertices.  With no finite vertex, ext == 0 or m == 0 every normal is (0, 0, 0) and n_defined = 0.
 *    2. B = 2.0 * (ext * ext); e = the integer with 2^(e-1) <= B < 2^e (frexp); b = the least integer with max(m, 1) <= 2^b;
 *       scale = ldexp(1.0, 61 - b - e).  Every cross-product component is at most B in magnitude (an edge component is at most ext
 *       because rounding is monotone; a product of two at most fl(ext*ext); their difference at most twice that, which is B), so
 *       every term is below 2^(61-b) in magnitude; a triangle with a repeated index has C = 0 exactly, so a vertex receives at most
 *       m non-zero terms and every sum stays below 2^61 < 2^62 in magnitude.
 *    3. For every triangle (a, b, c) whose three vertices are finite: u = P_b - P_a, w = P_c - P_a per component from the floats
 *       converted to double; C = (u_y*w_z - u_z*w_y, u_z*w_x - u_x*w_z, u_x*w_y - u_y*w_x); F_k = llrint(C_k * scale), to nearest
 *       even; S[a] += F, S[b] += F, S[c] += F in int64 (a triangle that names a vertex twice adds twice; its C is 0 anyway).
 *    4. Per vertex x, y, z = (double)S_k, len = sqrt((x*x + y*y) + z*z); len == 0 gives (0, 0, 0), otherwise
 *       out = ((float)(x/len), (float)(y/len), (float)(z/len)).  n_defined counts the vertices with len > 0.
 *    Integer addition commutes: the order of the triangles never shows.  e follows ext, so scaling every coordinate by a power of
 *    two leaves every bit of the output unchanged (short of overflow and underflow of the floats).  The triangles of mpmvs_tsdf_mesh
 *    are counter-clockwise seen from outside, so its normals point to the positive side, where the cameras are.
 *    -2: a NULL handle, a NULL out_normals with n > 0.  n_defined may be NULL.
 *
 * 3. SELECT.  mpmvs_mesh_select compacts the mesh on the device; the handle itself is not changed.  A triangle is kept iff all three
 *    of its vertices have keep[v] != 0.  A vertex is kept iff keep[v] != 0 and, with drop_unreferenced != 0, some kept triangle names
 *    it.  Kept vertices keep their order and are renumbered 0..n'-1; kept triangles keep their order and carry the new numbers;
 *    out_src[new] = old.  Returns n'; *out_xyz (n' x 3 floats), *out_rgb (n' x 3 bytes), *out_tri (*m_out x 3 int32; NULL when
 *    *m_out == 0) and *out_src (n' int32) receive buffers to release with mpmvs_free.  An empty result returns 0 with *m_out = 0 and
 *    all buffers NULL.  On failure no buffer is allocated and the outputs are not written.
 *    -2: a NULL handle, a NULL keep with n > 0, a NULL out_xyz, out_tri or m_out, out_rgb NULL for a mesh with colour or given for
 *    one without.  out_src may be NULL.
 *
 * mpmvs_mesh_pass_ms: device ms (HIP events): ms[0..2] the hook (with init), flatten and size passes of the last components call,
 * ms[3..4] accumulate and finish of the last normals call, ms[5..7] flag, scan and emit of the last select call; 0 for a pass that
 * did not run in the last call of its kind. */
typedef struct mpmvs_mesh mpmvs_mesh;
int mpmvs_mesh_create(int device, long long n, const float* xyz, const unsigned char* rgb /* n x 3, may be NULL */, long long m,
                      const int32_t* tri /* m x 3 */, mpmvs_mesh** h);
int mpmvs_mesh_components(mpmvs_mesh* h, int32_t* out_label /* n */, int32_t* out_verts /* n, may be NULL */, int32_t* out_tris /* n, may be NULL */,
                          long long counts[4] /* may be NULL */);
int mpmvs_mesh_normals(mpmvs_mesh* h, float* out_normals /* n x 3 */, long long* n_defined /* may be NULL */);
long long mpmvs_mesh_select(mpmvs_mesh* h, const unsigned char* keep /* n */, int drop_unreferenced, float** out_xyz,
                            unsigned char** out_rgb /* NULL iff the mesh has no colour */, int32_t** out_tri,
                            int32_t** out_src /* new vertex -> old index; may be NULL */, long long* m_out);
int mpmvs_mesh_pass_ms(const mpmvs_mesh* h, float ms[8]);
void mpmvs_mesh_destroy(mpmvs_mesh* h);

/* 4. SIMPLIFY.  mpmvs_simplify_mesh: Rossignac-Borrel vertex clustering on a uniform grid of edge e = (double)cell; the representative
 *    of a cluster is the mean of its vertices (placement 0) or the minimiser of its plane quadric (placement 1: Garland-Heckbert's
 *    unweighted planes, Lindstrom's pseudo-inverse about the cell mean, and his rule that the representative stays in its cell).
 *    Kernels and per-thread bodies: mp-mvs_amd/csrc/pm_simplify.hpp on the passes of pm_cloud.hpp and pm_voxel.hpp; DESIGN.md section
 *    25.  Bit for bit and independent of scheduling.  Arithmetic is fp64 unless stated, no contraction, only + - * / sqrt floor fabs,
 *    comparisons and llrint.  The handle is not changed.  Returns the number n' of clusters; every buffer is released with mpmvs_free.
 *    A. CLUSTERS.  The clusters are exactly the voxels of mpmvs_cloud_voxel_downsample called on the handle's n vertices with voxel =
 *       cell, no normals and the handle's colours: the same rule for taking part (three finite coordinates), the same origin o, t_a, c_a
 *       and numbering by smallest member index; out_count, out_cluster_of (-1 for a non-finite vertex) and out_rgb are that call's
 *       out_count, out_voxel_of and out_rgb.  With placement == 0 out_xyz is that call's out_xyz bit for bit, and out_placed is all 0.
 *    B. QUADRICS (placement == 1).  For every triangle (a, b, c) whose three vertices are finite: u, w and C as in statement 2, step 3;
 *       L = sqrt((Cx*Cx + Cy*Cy) + Cz*Cz); a triangle with !(L > 0) or a non-finite L adds nothing; nh_k = C_k / L.  For each of its
 *       three corners v with cluster k = cluster_of[v]: q_a = (t_a - c_a) - 0.5 of that vertex (its place in its cell, the centre at
 *       0), delta = (nh_x*q_x + nh_y*q_y) + nh_z*q_z; fix() of the six products nh_i*nh_j (i <= j) and of the three nh_i*delta is added
 *       to the int64 sums Q[k][6] and R[k][3], fix(x) = llrint(x * 2^30) to nearest even, and 1 to T[k] (a triangle with two corners in
 *       one cluster adds to it twice).  Every term is at most 2^30 in magnitude and a cluster receives at most 3m <= 3 * 2^30 of them:
 *       no sum overflows.
 *       Per cluster: x0_a = (double)S_a / ((double)count * 2^30) - 0.5 with S the position sums of the voxel statement.  T == 0:
 *       placed = 0.  Otherwise A_ij = (double)Q_ij / 2^30, r_i = (double)R_i / 2^30; eight cyclic Jacobi sweeps on A exactly as
 *       mpmvs_cloud_normals runs them (pairs (0,1), (0,2), (1,2); a pair whose entry is 0 is skipped) give d_0..d_2 and the columns of
 *       V; lmax = the largest d.  !(lmax > 0): placed = 2.  Otherwise g_i = r_i - ((A_i0*x0_0 + A_i1*x0_1) + A_i2*x0_2) with the
 *       original A; y_j = ((V_0j*g_0 + V_1j*g_1) + V_2j*g_2) / d_j for each j with d_j > 1e-3 * lmax, else 0;
 *       x_i = x0_i + ((V_i0*y_0 + V_i1*y_1) + V_i2*y_2).  If all three fabs(x_i) <= 0.5 (false for a NaN): placed = 1 and
 *       out_xyz[k][a] = (float)(o[a] + ((double)c_a + (0.5 + x_a)) * e); otherwise placed = 2.  A cluster with placed 0 or 2 gets the
 *       mean of A bit for bit.
 *    C. TRIANGLES.  (A, B, C) = the clusters of (a, b, c).  The triangle has a NON-FINITE vertex if one of them is -1; otherwise it is
 *       COLLAPSED if two are equal; otherwise ALIVE with key = the three numbers ascending.  An alive triangle is KEPT iff no alive
 *       triangle of smaller index has the same key (duplicates and fold-overs go, the first survives).  Kept triangles keep their
 *       order and are written as (A, B, C) in the original corner order; out_tri_src[new] = old.  counts = {non-finite, collapsed,
 *       duplicates dropped}; *m_out = the number kept (*out_tri and *out_tri_src NULL when 0).  Clusters that no kept triangle names
 *       are still output: mpmvs_mesh_select with drop_unreferenced on the result removes them.
 *    -2: a NULL handle, a cell that is not finite or <= 0, a placement outside {0, 1}, a NULL out_xyz, out_tri or m_out, out_rgb NULL
 *    for a mesh with colour or given for one without.  -3: the limits of the voxel call (more than 2^21 cells along an axis: the
 *    text names the axis).  On failure nothing is allocated or written.  n == 0 or no finite vertex: returns 0 with all buffers
 *    NULL, *m_out = 0, counts filled on the host, out_cluster_of all -1; nothing is launched.
 *    mpmvs_simplify_mesh_ms: device ms (HIP events) of the last call: cluster (the voxel passes up to the numbering), position
 *    accumulate, quadric accumulate, place, classify + insert, flag + scan, emit; 0 for a pass that did not run. */
long long mpmvs_simplify_mesh(mpmvs_mesh* h, float cell, int placement /* 0 mean, 1 quadric */,
                              float** out_xyz, unsigned char** out_rgb /* NULL iff the mesh has no colour */,
                              int32_t** out_tri, long long* m_out,
                              int32_t* out_cluster_of /* caller's, n entries, may be NULL */,
                              int32_t** out_count /* may be NULL */, unsigned char** out_placed /* may be NULL */,
                              int32_t** out_tri_src /* may be NULL */, long long counts[3] /* may be NULL */);
int mpmvs_simplify_mesh_ms(const mpmvs_mesh* h, float ms[7]);

/* 5. DISTANCE.  mpmvs_surface_distance: per point of a cloud handle the exact capped distance to the SURFACE of the mesh, not to its
 *    vertices, and the triangle that attains it.  N is the cloud's point count; the queries are the cloud's own points and the results
 *    are indexed by the cloud's point index.  Kernels and per-thread bodies: mp-mvs_amd/csrc/pm_surface.hpp on the grid of
 *    pm_cloud.hpp; DESIGN.md section 26.  Bit for bit the plain loop below and independent of scheduling.  Arithmetic is fp64 unless
 *    stated, no contraction; only + - * /, comparisons and one conversion to fp32, to nearest even.
 *      A triangle t = (a, b, c) TAKES PART iff its three vertices have three finite coordinates each; a point q iff its three are.
 *      r2 = radius * radius in fp32, as in mpmvs_cloud_nearest.  dot(u, v) = (u_x*v_x + u_y*v_y) + u_z*v_z.
 *      ab = B - A, ac = C - A, ap = q - A, bp = q - B, cp = q - C, per component from the floats converted to double.
 *      s1 = dot(ab, ap), s2 = dot(ac, ap), s3 = dot(ab, bp), s4 = dot(ac, bp), s5 = dot(ab, cp), s6 = dot(ac, cp).
 *      vc = s1*s4 - s3*s2, vb = s5*s2 - s1*s6, va = s3*s6 - s5*s4.
 *    The closest point X is given by the first of these rules that applies, each tested exactly as written (a comparison with a NaN
 *    is false):
 *      1. s1 <= 0 && s2 <= 0:                              X = A.
 *      2. s3 >= 0 && s4 <= s3:                             X = B.
 *      3. vc <= 0 && s1 >= 0 && s3 <= 0:                   v = s1 / (s1 - s3), X_k = A_k + v*ab_k.
 *      4. s6 >= 0 && s5 <= s6:                             X = C.
 *      5. vb <= 0 && s2 >= 0 && s6 <= 0:                   w = s2 / (s2 - s6), X_k = A_k + w*ac_k.
 *      6. va <= 0 && (s4 - s3) >= 0 && (s5 - s6) >= 0:     w = (s4 - s3) / ((s4 - s3) + (s5 - s6)), X_k = B_k + w*(C_k - B_k).
 *      7. otherwise:                                       den = (va + vb) + vc, v = vb / den, w = vc / den,
 *                                                          X_k = (A_k + v*ab_k) + w*ac_k.
 *    e = q - X, dd = (e_x*e_x + e_y*e_y) + e_z*e_z, D = (float)dd.  t is a CANDIDATE of q iff D <= r2 (false for a NaN).  A degenerate
 *    triangle follows the sequence literally: what it yields is deterministic, and where it yields a NaN it is no candidate.
 *      out_d2[i]  = the smallest candidate D;
 *      out_tri[i] = the smallest triangle index among the candidates that attain it (duplicate triangles, the order of the triangles
 *                   on the device and the order of the points never show);
 *      with no candidate, or for a point that takes no part: out_d2 = +inf, out_tri = -1.
 *      counts = {points with a candidate, points that take part}.
 *    -2, with every output untouched: a NULL handle of either kind, a NULL out_d2 with N > 0, a radius that is not finite or <= 0, two
 *    handles on different devices.  -3: what the cloud's grid at this radius refuses (more than 2^21 cells along an axis, worded as
 *    mpmvs_cloud_nearest words it).  -100: HIP failure.  All but -100 are found before the device is touched.  N == 0 touches nothing;
 *    with m == 0, no triangle or no point taking part the call answers on the host (+inf, -1, the counts) and launches nothing.
 *    Neither handle is changed, except that the cloud may gain a cached grid for this radius, under the rules of its grid cache; the
 *    time of that build stays with the cloud's own report (mpmvs_cloud_kernel_ms).
 *    mpmvs_surface_distance_ms: device ms (HIP events) of the last call on this mesh handle, the total returned and, in pass_ms, the
 *    init, scatter and finish passes; 0 for a call that launched nothing.
 *
 * 6. SAMPLE.  mpmvs_surface_sample: deterministic samples of the surface at a given spacing, so that a mesh can stand where a point
 *    cloud is asked for.  Returns the number K of samples; the buffers are released with mpmvs_free; with K == 0 all are NULL, and
 *    nothing is launched for a mesh without a participating triangle.  Bit for bit the plain loop below.  Arithmetic is fp64 unless
 *    stated, no contraction; only + - * / sqrt ceil, integer arithmetic and one conversion to fp32.
 *      h_s = (double)spacing.  A triangle with a non-finite vertex yields no sample.  For any other triangle: l2 = the largest of its
 *      three squared edge lengths, each (dx*dx + dy*dy) + dz*dz; Lm = sqrt(l2); ratio = Lm / h_s; s = max(1, (long long)ceil(ratio));
 *      !(ratio <= 4096) is a refusal.  (A triangle of size 0 has s = 1 and yields its one vertex position.)
 *      The triangle yields s*s samples, the centroids of the sub-triangles of its regular s-subdivision, enumerated by k = 0 .. s*s-1:
 *      u = s*s - 1 - k; g = the largest integer with g*g <= u; i = s - 1 - g; l = k - (2*s*i - i*i); j = l >> 1;
 *      (na, nb) = (3i + 1, 3j + 1) for even l and (3i + 2, 3j + 2) for odd l; nc = 3s - na - nb (always >= 1).
 *      x_k = (float)(((na*A_k + nb*B_k) + nc*C_k) / (double)(3s)), the integers converted to double exactly.
 *      Samples are output triangle by triangle in index order, k ascending; out_tri_of[sample] = t.
 *      out_rgb = (2*(na*Ca + nb*Cb + nc*Cc) + 3s) / (2*3s) in integer division, per channel.
 *      out_normals = nh = C / L of statement 4B converted to float, the same face normal for every sample of the triangle; (0, 0, 0)
 *      where !(L > 0) or L is not finite.
 *    Every sub-triangle's longest edge is at most `spacing`, so every point of a participating triangle lies within 2/3 * spacing of
 *    one of its samples (a centroid is two thirds of a median from a vertex, and a median is no longer than the longest edge).
 *    -2, with nothing allocated or written: a NULL handle, a spacing that is not finite or <= 0, a NULL out_xyz or out_tri_of, out_rgb
 *    NULL for a mesh with colour or given for one without.  -3: a triangle with !(ratio <= 4096) (the text names the first such
 *    triangle), or more than 2^30 samples in all (the text names the total).  The mesh handle drops its host copy at the first upload,
 *    so these two -3 refusals are found after the count pass on the device: the only refusals of the family that may touch the
 *    device first.  -100: HIP failure.  out_normals may be NULL.
 *    mpmvs_surface_sample_ms: device ms of the last call, the total returned and, in pass_ms, count, scan and emit. */
int mpmvs_surface_distance(mpmvs_mesh* surface, mpmvs_cloud* points, float radius, float* out_d2 /* N */, int32_t* out_tri /* N, may be NULL */,
                           long long counts[2] /* may be NULL */);
float mpmvs_surface_distance_ms(const mpmvs_mesh* surface, float pass_ms[3] /* may be NULL */);
long long mpmvs_surface_sample(mpmvs_mesh* h, float spacing, float** out_xyz, int32_t** out_tri_of,
                               unsigned char** out_rgb /* NULL iff the mesh has no colour */, float** out_normals /* may be NULL */);
float mpmvs_surface_sample_ms(const mpmvs_mesh* h, float pass_ms[3] /* may be NULL */);

/* 7. RENDER.  mpmvs_surface_render_depth: the mesh rasterised into pinhole cameras: per pixel the depth of the nearest surface along
 *    the pixel's ray and the triangle it shows.  No parameter: a mesh has no gaps, so the splat and occlusion heuristics of
 *    mpmvs_cloud_render_depth have no counterpart.  Kernels and per-thread bodies: mp-mvs_amd/csrc/pm_raster.hpp; DESIGN.md section 27.
 *    Bit for bit the plain loop below, whatever the order of triangles, views and threads.  Arithmetic is fp64, one operation per step
 *    in the order written, no contraction; camera and vertex floats are converted to double first.  Pixel centres are at integers.
 *    depth_min / depth_max and C of the cameras are not read.
 *    For view v with K, R, t (row-major), W x H, and triangle i = (a, b, c), per vertex p:
 *      X_j = ((R[3j]*p0 + R[3j+1]*p1) + R[3j+2]*p2) + t[j];   q_j = (K[3j]*X0 + K[3j+1]*X1) + K[3j+2]*X2;   q = (q.x, q.y, q.z), q.z
 *      the project's depth.  There is no inverse of K and no clipping anywhere.
 *      The triangle TAKES PART in the view iff all nine q components are finite and max(qa.z, qb.z, qc.z) > 0: one behind the camera
 *      plane is skipped by rule, one that crosses the plane is rendered unclipped.
 *      nbc = qb x qc, nca = qc x qa, nab = qa x qb with (u x v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x): two products
 *      and one difference each.  det = (qa.x*nbc.x + qa.y*nbc.y) + qa.z*nbc.z.
 *      Per pixel (x, y): E0 = (x*nbc.x + y*nbc.y) + nbc.z, E1 and E2 alike from nca and nab; S = (E0 + E1) + E2.
 *      The pixel is a CANDIDATE iff (E0 >= 0 && E1 >= 0 && E2 >= 0, or E0 <= 0 && E1 <= 0 && E2 <= 0) and S != 0.  Both windings render;
 *      zeros are inclusive, so a pixel centre on a shared edge belongs to both triangles.  An edge's function depends on its two
 *      vertices only and swapping them negates every bit of it, so two triangles that share an edge leave no pixel between them.
 *      z = det / S; if z < zlo then z = zlo; if z > zhi then z = zhi, zlo and zhi the smallest and largest of the three q.z (a
 *      comparison with a NaN is false).  zf = (float)z.  The pixel is COVERED by the triangle iff zf is finite and zf > 0.
 *      key = (bits(zf) << 32) | i.  Per pixel the minimum key over the covering triangles: the nearest depth, and among equal depths
 *      the smallest triangle index.  out_depth[v][y*W + x] = zf of the minimum, or 0.0f where nothing covers; out_tri = i, or -1.
 *    counts = {(triangle, view) pairs taking part, pixels covered summed over the views, pairs that went down the large-triangle path}:
 *    the first two follow from the statement, the third is a diagnostic of the implementation and depends on MPMVS_RASTER_LARGE.
 *    -2: a NULL handle or n_views < 0 (checked first, also for n_views == 0); NULL cams or out_depth, a NULL out_depth[v], a width or
 *    height <= 0.  -3: a width or height above 2^24, or a view of more than 2^31 - 1 pixels.  -100: HIP failure.  All but -100 are found
 *    before the device is touched, with every output untouched.  n_views == 0 returns 0 and touches nothing; a mesh without a triangle
 *    of three finite vertices is answered on the host (0.0f, -1).  The buffers are host buffers and the call blocks; the handle is
 *    unchanged.  out_tri, or any out_tri[v], may be NULL: not wanted.
 *    mpmvs_surface_render_ms: device ms (HIP events) of the last call on this handle, the total returned and, in pass_ms, the init,
 *    small, large and resolve passes summed over the chunks of views; 0 for a call that launched nothing.
 *    mpmvs_surface_render_work: diagnostics of the last call on this handle, not part of the statement: work[0] = the pixels of the
 *    boxes the pairs were tested in, work[1] = the atomic minima issued (it depends on the order of the threads); 0 for a call that
 *    launched nothing.  -2: a NULL argument. */
int mpmvs_surface_render_depth(mpmvs_mesh* surface, int n_views, const mpmvs_camera* cams, float* const* out_depth /* out_depth[v]: H*W */,
                               int32_t* const* out_tri /* NULL, or NULL entries: not wanted */, long long counts[3] /* may be NULL */);
float mpmvs_surface_render_ms(const mpmvs_mesh* surface, float pass_ms[4] /* may be NULL: init, small, large, resolve */);
int mpmvs_surface_render_work(const mpmvs_mesh* surface, long long work[2]);

/* ---- host arrays ------------------------------------------------------------ */
/* Page-locked host memory for the arrays the reference allocates with new[] in AllocatePatchMatch and
 * CudaPlanarPriorInitialization (hostPlaneHypotheses, hostCosts, hostGeomCosts, hostPriorPlanes, hostPlaneMask;
 * src/PatchMatch.cpp:966-972,979-982): with them the copies of mpmvs_run_get / mpmvs_get / mpmvs_set_state / mpmvs_set_prior
 * are DMA transfers at PCIe rate and, inside mpmvs_run_get, asynchronous.  Any host memory works; this is the fast kind.
 * Released buffers are pooled per size.  NULL on failure. */
void* mpmvs_alloc_pinned(size_t bytes);
void mpmvs_free_pinned(void* p);
/* Device memory on `device` for callers that keep data in HBM between calls (the exchange slots that receive
 * mpmvs_export_depth_device and feed mpmvs_set_src_depths_mixed); pooled per (device, size) like the contexts' own buffers. */
void* mpmvs_device_alloc(int device, size_t bytes);
/* The caller must have synchronised every consumer of the buffer (the contexts that were given it through
 * mpmvs_set_src_depths_mixed / mpmvs_export_depth_device have finished their calls: those entry points wait for their copies):
 * a freed buffer is handed out again at once. */
void mpmvs_device_free(int device, void* p);

/* How `device` reaches `peer` inside this process: *can_access = hipDeviceCanAccessPeer (-1 if the runtime refused to say),
 * *link_type / *hops = hipExtGetLinkTypeAndHopCount (4 = xGMI, 2 = PCIe; -1 = unknown).  The copies of mpmvs_set_src_depths_mixed
 * and mpmvs_fuse_*_ctx between devices take this path; bench.py --gpus N prints the table per rank before it measures.  (The
 * reference is pinned to device 0, src/PatchMatch.cpp:509.) */
int mpmvs_peer_info(int device, int peer, int* can_access, int* link_type, int* hops);

/* ---- resident texture format ---------------------------------------------- */
/* Source images whose pixels are all integers in [0, 255] (the reference's
 * imread(GRAYSCALE) -> convertTo(CV_32F) path, src/PatchMatch.cpp:877-882) are
 * kept in HBM as a quad-packed 8-bit texture (one dword load per bilinear tap);
 * results are bit-identical to the fp32 format.  force_fp32 != 0 before
 * mpmvs_set_views keeps fp32 regardless.  mpmvs_texture_format returns 1 for
 * the 8-bit format, 0 for fp32. */
int mpmvs_set_texture_format(mpmvs_ctx* ctx, int force_fp32);
int mpmvs_texture_format(mpmvs_ctx* ctx);

/* ---- measurement --------------------------------------------------------- */
/* HIP-event timing of the launches of the last mpmvs_run, on the context's
 * stream: ms[k] / count[k] per kernel kind (6 entries each). Profiling is off
 * by default (events add a little host work per launch). */
int mpmvs_set_profiling(mpmvs_ctx* ctx, int enable);
int mpmvs_get_kernel_times(mpmvs_ctx* ctx, float* ms6, int* count6);

/* ---- the chained update launch: self-check and fault injection ------------- */
/* Run() chains the black / red passes of a window scale into ONE launch whose blocks wait for their neighbours of the pass
 * before (no counterpart in the reference, which synchronises the device after every pass, src/PatchMatch.cu:1211-1236).
 * The first mpmvs_create on a device runs a small Problem both ways and compares the results bit for bit; on a mismatch
 * every context of that device launches one kernel per pass instead (MPMVS_CHAIN_SELFCHECK=0 skips the check, MPMVS_CHAIN=0
 * selects the per-pass form outright).  mpmvs_chain_status: 1 = chained launches in use by this context, 0 = per-pass launches by
 * request, -1 = per-pass launches because the self-check failed on this device. */
int mpmvs_chain_status(mpmvs_ctx* ctx);
/* Fault injection for tests: from now on the update block at raster position `block_pos` never signals its first pass, and a
 * waiting block gives up after `spin_limit` polls (<= 0: the default of about a second).  The affected mpmvs_run* returns -101
 * ("results invalid"; with mpmvs_run_get_async the host buffers of every outstanding call are invalid once mpmvs_wait returns
 * -101), the context stays usable.  block_pos < 0 switches the fault off. */
int mpmvs_dbg_chain_stall(mpmvs_ctx* ctx, int block_pos, int spin_limit);

/* ---- per-view costs kept from InitializeScore ------------------------------ */
/* InitializeScore evaluates every pixel's plane against every source view; the context keeps these costs (4 x views x W x H bytes)
 * and the first black and the first red update pass that follow at the same window scale read them back instead of evaluating the
 * unchanged plane again ("the current plane under the new weights", src/PatchMatch.cu:901-913) -- the same bits, one evaluation
 * round per view less.  Anything else that writes the planes or changes the views ends their validity.
 * enable = 0: every pass recomputes; 1: the default; < 0: leave the setting as it is.  *passes_served (may be NULL): update passes
 * of this context enqueued so far with the kept costs in use.  For tests and same-process A/B measurements. */
int mpmvs_dbg_own_costs(mpmvs_ctx* ctx, int enable, int* passes_served);

#ifdef __cplusplus
}
#endif
#endif /* MPMVS_H_ */
