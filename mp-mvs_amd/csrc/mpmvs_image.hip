// mpmvs_image.hip -- the stateless image calls of the C ABI declared in include/mpmvs.h, each one DeviceCall (pm_host.hpp) with
// host buffers in and out: the joint-bilateral sky-mask refinement (pm_sky.hpp), the view selection of a COLMAP model
// (pm_viewsel.hpp) and the undistortion of COLMAP camera models (pm_undistort.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_sky.hpp"
#include "pm_viewsel.hpp"
#include "pm_undistort.hpp"

using namespace pm;

extern "C" {

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
    if (launch(k_sky_bilateral, grid, dim3(256), st, d_img, d_mask, d_out, height, width) != hipSuccess) return -100;
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

}  // extern "C"
