// undistort.cpp -- the host statement of the undistortion warp (mpmvs_host_undistort_u8): what mpmvs_undistort_u8 must equal bit
// for bit, built from the same model header as the kernel (../csrc/pm_undistort_model.hpp), plus probes of that header's atan,
// forward map and inverse for the tests.  Contract: DESIGN.md section 12.
#include <cstddef>
#include <cstring>

#include "../csrc/pm_undistort_model.hpp"
#include "PatchMatch.h"

extern "C" {

// same arguments as mpmvs_undistort_u8 without the device; 0 or -2
int mpmvs_host_undistort_u8(const unsigned char* src, int channels, int width, int height, size_t pitch_bytes, int model_id, const double* params,
                            int n_params, const double dst_pinhole[4], int dst_width, int dst_height, unsigned char* out, unsigned char* out_valid) {
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
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
    for (int Y = 0; Y < dst_height; ++Y) {
        unsigned char* o = out + (size_t)Y * dst_width * channels;
        for (int X = 0; X < dst_width; ++X, o += channels) {
            const UndTap t = und_tap(m, dst_pinhole, X, Y, width, height);
            if (out_valid) out_valid[(size_t)Y * dst_width + X] = t.valid ? 1 : 0;
            if (!t.valid) {
                std::memset(o, 0, (size_t)channels);
                continue;
            }
            const unsigned char* r0 = src + (size_t)t.y0 * pitch_bytes;
            const unsigned char* r1 = src + (size_t)t.y1 * pitch_bytes;
            for (int c = 0; c < channels; ++c)
                o[c] = und_blend(t, (double)r0[t.x0 * channels + c], (double)r0[t.x1 * channels + c], (double)r1[t.x0 * channels + c],
                                 (double)r1[t.x1 * channels + c]);
        }
    }
    return 0;
}

// the size of the OpenMP team the statement above runs on (for tools/bench_undistort.py)
int mpmvs_host_undistort_threads(void) { return mpmvs_host::OmpThreads(); }

// probes (tests): the header's atan, forward map (n points (u, v) -> (x, y)) and inverse (n points (x, y) -> (u, v))
void mpmvs_host_undistort_atan(const double* x, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = und_atan(x[i]);
}

int mpmvs_host_undistort_forward(int model_id, const double* params, int n_params, const double* uv, int n, double* xy) {
    UndModel m;
    if (!und_model_init(m, model_id, params, n_params)) return -2;
    for (int i = 0; i < n; ++i) und_img_from_cam(m, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
    return 0;
}

int mpmvs_host_undistort_inverse(int model_id, const double* params, int n_params, const double* xy, int n, double* uv) {
    UndModel m;
    if (!und_model_init(m, model_id, params, n_params)) return -2;
    for (int i = 0; i < n; ++i) und_cam_from_img(m, xy[2 * i], xy[2 * i + 1], uv[2 * i], uv[2 * i + 1]);
    return 0;
}

}  // extern "C"
