// pm_undistort_model.hpp -- COLMAP's 11 camera models as ONE statement shared by the device kernel (pm_undistort.hpp), the HIP
// library's host entry (mpmvs_undistort_camera) and the host library (host/undistort.cpp): the forward map "normalised pinhole
// coordinates (u, v) -> distorted image point", and, for the host alone, its inverse and the output-camera rule.  Contract:
// DESIGN.md section 12.  Includable without HIP.
//
// All arithmetic is fp64, evaluated left to right as written; both libraries are built with -ffp-contract=off, and fp64 / and
// sqrt are IEEE-exact on the host and on gfx950.  No libm / ocml transcendental is called on the forward path:
// und_atan() is built from + - * / sqrt, and tan(omega / 2) of the FOV model is a per-camera constant formed on the host.  The
// forward map therefore gives the same bits on both sides for every model.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define UND_HD __host__ __device__ __forceinline__
#else
#define UND_HD inline
#endif

// model ids and parameter order: mp-mvs_amd/colmap.py CAMERA_MODELS / PARAMS
enum UndModelId {
    UND_SIMPLE_PINHOLE = 0, UND_PINHOLE, UND_SIMPLE_RADIAL, UND_RADIAL, UND_OPENCV, UND_OPENCV_FISHEYE, UND_FULL_OPENCV, UND_FOV,
    UND_SIMPLE_RADIAL_FISHEYE, UND_RADIAL_FISHEYE, UND_THIN_PRISM_FISHEYE, UND_NUM_MODELS
};

// one camera: fx fy cx cy (f for both where the model has one), the remaining parameters in file order, zero padded
struct UndModel {
    int id;
    double fx, fy, cx, cy;
    double k[8];
    double tan_half;   // FOV: tan(omega / 2), formed on the host
};

// atan from + - * / sqrt: |x| > 1 folds to 1 / x; three halvings a <- a / (1 + sqrt(1 + a * a)) bring the argument below
// tan(pi / 32); there 18 terms of the alternating series (Horner) are exact to the last bit; times 8, then pi / 2 - for the fold.
UND_HD double und_atan(double x) {
    const bool neg = x < 0.0;
    double a = neg ? -x : x;
    const bool fold = a > 1.0;
    if (fold) a = 1.0 / a;
    a = a / (1.0 + sqrt(1.0 + a * a));
    a = a / (1.0 + sqrt(1.0 + a * a));
    a = a / (1.0 + sqrt(1.0 + a * a));
    const double z = a * a;
    double s = 1.0 / 35.0;
    s = 1.0 / 33.0 - z * s;
    s = 1.0 / 31.0 - z * s;
    s = 1.0 / 29.0 - z * s;
    s = 1.0 / 27.0 - z * s;
    s = 1.0 / 25.0 - z * s;
    s = 1.0 / 23.0 - z * s;
    s = 1.0 / 21.0 - z * s;
    s = 1.0 / 19.0 - z * s;
    s = 1.0 / 17.0 - z * s;
    s = 1.0 / 15.0 - z * s;
    s = 1.0 / 13.0 - z * s;
    s = 1.0 / 11.0 - z * s;
    s = 1.0 / 9.0 - z * s;
    s = 1.0 / 7.0 - z * s;
    s = 1.0 / 5.0 - z * s;
    s = 1.0 / 3.0 - z * s;
    s = 1.0 - z * s;
    double r = 8.0 * (a * s);
    if (fold) r = 1.5707963267948966 - r;
    return neg ? -r : r;
}

// (u, v) -> (u, v) * atan(r) / r: the first step of the three *_FISHEYE models (identity for r <= 1e-12)
UND_HD void und_fisheye(double u, double v, double& uu, double& vv) {
    const double r = sqrt(u * u + v * v);
    if (r > 1e-12) {
        const double th = und_atan(r);
        uu = u * th / r;
        vv = v * th / r;
    } else {
        uu = u;
        vv = v;
    }
}

// the distortion of the three *_FISHEYE models in their own (uu, vv) coordinates: (uu, vv) -> (uu + du, vv + dv)
UND_HD void und_distort_theta(const UndModel& m, double uu, double vv, double& xo, double& yo) {
    const double t2 = uu * uu + vv * vv;
    double du, dv;
    if (m.id == UND_SIMPLE_RADIAL_FISHEYE) {
        const double rad = m.k[0] * t2;
        du = uu * rad;
        dv = vv * rad;
    } else if (m.id == UND_RADIAL_FISHEYE) {
        const double rad = m.k[0] * t2 + m.k[1] * t2 * t2;
        du = uu * rad;
        dv = vv * rad;
    } else {   // THIN_PRISM_FISHEYE: k1 k2 p1 p2 k3 k4 sx1 sy1
        const double t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double rad = m.k[0] * t2 + m.k[1] * t4 + m.k[4] * t6 + m.k[5] * t8;
        du = uu * rad + 2.0 * m.k[2] * uu * vv + m.k[3] * (t2 + 2.0 * uu * uu) + m.k[6] * t2;
        dv = vv * rad + 2.0 * m.k[3] * uu * vv + m.k[2] * (t2 + 2.0 * vv * vv) + m.k[7] * t2;
    }
    xo = uu + du;
    yo = vv + dv;
}

UND_HD bool und_is_theta_model(int id) { return id == UND_SIMPLE_RADIAL_FISHEYE || id == UND_RADIAL_FISHEYE || id == UND_THIN_PRISM_FISHEYE; }

// normalised pinhole (u, v) -> normalised distorted point (u + du, v + dv) (for the *_FISHEYE models: uu + du, vv + dv)
UND_HD void und_distort(const UndModel& m, double u, double v, double& xo, double& yo) {
    const double r2 = u * u + v * v;
    double du = 0.0, dv = 0.0;
    switch (m.id) {
        case UND_SIMPLE_RADIAL: {
            const double rad = m.k[0] * r2;
            du = u * rad;
            dv = v * rad;
        } break;
        case UND_RADIAL: {
            const double rad = m.k[0] * r2 + m.k[1] * r2 * r2;
            du = u * rad;
            dv = v * rad;
        } break;
        case UND_OPENCV: {   // k1 k2 p1 p2
            const double rad = m.k[0] * r2 + m.k[1] * r2 * r2;
            du = u * rad + 2.0 * m.k[2] * u * v + m.k[3] * (r2 + 2.0 * u * u);
            dv = v * rad + 2.0 * m.k[3] * u * v + m.k[2] * (r2 + 2.0 * v * v);
        } break;
        case UND_FULL_OPENCV: {   // k1 k2 p1 p2 k3 k4 k5 k6
            const double r4 = r2 * r2, r6 = r4 * r2;
            const double rad = (1.0 + m.k[0] * r2 + m.k[1] * r4 + m.k[4] * r6) / (1.0 + m.k[5] * r2 + m.k[6] * r4 + m.k[7] * r6);
            du = u * rad + 2.0 * m.k[2] * u * v + m.k[3] * (r2 + 2.0 * u * u) - u;
            dv = v * rad + 2.0 * m.k[3] * u * v + m.k[2] * (r2 + 2.0 * v * v) - v;
        } break;
        case UND_OPENCV_FISHEYE: {   // k1 k2 k3 k4
            const double r = sqrt(r2);
            if (r > 1e-12) {
                const double th = und_atan(r);
                const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
                const double thd = th * (1.0 + m.k[0] * t2 + m.k[1] * t4 + m.k[2] * t6 + m.k[3] * t8);
                du = u * thd / r - u;
                dv = v * thd / r - v;
            }
        } break;
        case UND_FOV: {
            const double w = m.k[0], w2 = w * w;
            double factor;
            if (w2 < 1e-12) {
                factor = w2 * r2 / 3.0 - w2 / 12.0 + 1.0;
            } else if (r2 < 1e-12) {
                factor = -2.0 * m.tan_half * (4.0 * r2 * m.tan_half * m.tan_half - 3.0) / (3.0 * w);
            } else {
                const double r = sqrt(r2);
                factor = und_atan(2.0 * m.tan_half * r) / (r * w);
            }
            du = u * factor - u;
            dv = v * factor - v;
        } break;
        case UND_SIMPLE_RADIAL_FISHEYE:
        case UND_RADIAL_FISHEYE:
        case UND_THIN_PRISM_FISHEYE: {
            double uu, vv;
            und_fisheye(u, v, uu, vv);
            und_distort_theta(m, uu, vv, xo, yo);
            return;
        }
        default: break;   // SIMPLE_PINHOLE, PINHOLE
    }
    xo = u + du;
    yo = v + dv;
}

// THE forward map: normalised pinhole coordinates -> image point of the distorted camera (pixel centres at +0.5)
UND_HD void und_img_from_cam(const UndModel& m, double u, double v, double& x, double& y) {
    double xn, yn;
    und_distort(m, u, v, xn, yn);
    x = m.fx * xn + m.cx;
    y = m.fy * yn + m.cy;
}

// ---- host only (plain host functions: the inverse needs libm's tan) --------------------------------------------------------------------------------------------------------------
// number of parameters of model `id` in a cameras file (0: unknown id)
inline int und_num_params(int id) {
    static const int n[UND_NUM_MODELS] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12};
    return id >= 0 && id < UND_NUM_MODELS ? n[id] : 0;
}

// params in file order -> UndModel; false for an unknown model, a wrong count or a focal length that is not finite and positive
inline bool und_model_init(UndModel& m, int id, const double* params, int n_params) {
    if (!params || und_num_params(id) == 0 || n_params != und_num_params(id)) return false;
    m = UndModel();
    m.id = id;
    const bool one_f = id == UND_SIMPLE_PINHOLE || id == UND_SIMPLE_RADIAL || id == UND_RADIAL || id == UND_SIMPLE_RADIAL_FISHEYE || id == UND_RADIAL_FISHEYE;
    int k = 0;
    m.fx = params[k++];
    m.fy = one_f ? m.fx : params[k++];
    m.cx = params[k++];
    m.cy = params[k++];
    for (int i = 0; k < n_params; ++i) m.k[i] = params[k++];
    for (int i = 0; i < n_params; ++i)
        if (!std::isfinite(params[i])) return false;
    if (!(m.fx > 0.0) || !(m.fy > 0.0)) return false;
    m.tan_half = id == UND_FOV ? std::tan(m.k[0] / 2.0) : 0.0;
    return true;
}

inline bool und_is_pinhole(const UndModel& m) { return m.id == UND_SIMPLE_PINHOLE || m.id == UND_PINHOLE; }

// Newton on g(p) = target with a central-difference Jacobian (COLMAP's IterativeUndistortion): steps max(1e-15, |1e-6 p|),
// at most 100 iterations, done when the squared step is below 1e-20
template <typename G>
inline void und_newton(G g, double tx, double ty, double& px, double& py) {
    px = tx;
    py = ty;
    for (int it = 0; it < 100; ++it) {
        const double s0 = std::fmax(1e-15, std::fabs(1e-6 * px)), s1 = std::fmax(1e-15, std::fabs(1e-6 * py));
        double gx, gy, ax, ay, bx, by, cx, cy, dx, dy;
        g(px, py, gx, gy);
        g(px - s0, py, ax, ay);
        g(px + s0, py, bx, by);
        g(px, py - s1, cx, cy);
        g(px, py + s1, dx, dy);
        const double j00 = (bx - ax) / (2.0 * s0), j01 = (dx - cx) / (2.0 * s1);
        const double j10 = (by - ay) / (2.0 * s0), j11 = (dy - cy) / (2.0 * s1);
        const double det = j00 * j11 - j01 * j10;
        const double ex = gx - tx, ey = gy - ty;
        const double stx = (j11 * ex - j01 * ey) / det, sty = (j00 * ey - j10 * ex) / det;
        if (!std::isfinite(stx) || !std::isfinite(sty)) return;
        px -= stx;
        py -= sty;
        if (stx * stx + sty * sty < 1e-20) return;
    }
}

// the inverse of und_img_from_cam, for border points.  The *_FISHEYE models are inverted in (uu, vv), then
// (u, v) = (uu, vv) * tan(theta) / theta (tan is host-only, so libm serves).
inline void und_cam_from_img(const UndModel& m, double x, double y, double& u, double& v) {
    const double tx = (x - m.cx) / m.fx, ty = (y - m.cy) / m.fy;
    if (und_is_pinhole(m)) {
        u = tx;
        v = ty;
        return;
    }
    if (und_is_theta_model(m.id)) {
        double uu, vv;
        und_newton([&](double a, double b, double& xo, double& yo) { und_distort_theta(m, a, b, xo, yo); }, tx, ty, uu, vv);
        const double th = std::sqrt(uu * uu + vv * vv);
        const double s = th > 1e-12 ? std::tan(th) / th : 1.0;
        u = uu * s;
        v = vv * s;
        return;
    }
    und_newton([&](double a, double b, double& xo, double& yo) { und_distort(m, a, b, xo, yo); }, tx, ty, u, v);
}

// COLMAP's UndistortCamera rule: the PINHOLE camera (fx, fy, cx', cy') of size W' x H' that the image of `m`
// (width x height) is resampled to.  blank in [0, 1]: 0 = no blank pixel in the output, 1 = every source pixel kept.
inline bool und_output_camera(const UndModel& m, int width, int height, double blank, double min_scale, double max_scale, double out_pinhole[4],
                              int& out_w, int& out_h) {
    out_pinhole[0] = m.fx;
    out_pinhole[1] = m.fy;
    out_pinhole[2] = m.cx;
    out_pinhole[3] = m.cy;
    out_w = width;
    out_h = height;
    if (und_is_pinhole(m)) return true;
    const double inf = HUGE_VAL;
    double left_min = inf, left_max = -inf, right_min = inf, right_max = -inf;
    double top_min = inf, top_max = -inf, bottom_min = inf, bottom_max = -inf;
    for (int y = 0; y < height; ++y) {
        double u, v;
        und_cam_from_img(m, 0.5, y + 0.5, u, v);
        const double l = m.fx * u + m.cx;
        und_cam_from_img(m, width - 0.5, y + 0.5, u, v);
        const double r = m.fx * u + m.cx;
        left_min = std::fmin(left_min, l);
        left_max = std::fmax(left_max, l);
        right_min = std::fmin(right_min, r);
        right_max = std::fmax(right_max, r);
    }
    for (int x = 0; x < width; ++x) {
        double u, v;
        und_cam_from_img(m, x + 0.5, 0.5, u, v);
        const double t = m.fy * v + m.cy;
        und_cam_from_img(m, x + 0.5, height - 0.5, u, v);
        const double b = m.fy * v + m.cy;
        top_min = std::fmin(top_min, t);
        top_max = std::fmax(top_max, t);
        bottom_min = std::fmin(bottom_min, b);
        bottom_max = std::fmax(bottom_max, b);
    }
    const double cx = m.cx, cy = m.cy;
    const double min_sx = std::fmin(cx / (cx - left_min), (width - 0.5 - cx) / (right_max - cx));
    const double min_sy = std::fmin(cy / (cy - top_min), (height - 0.5 - cy) / (bottom_max - cy));
    const double max_sx = std::fmax(cx / (cx - left_max), (width - 0.5 - cx) / (right_min - cx));
    const double max_sy = std::fmax(cy / (cy - top_max), (height - 0.5 - cy) / (bottom_min - cy));
    double sx = 1.0 / (min_sx * blank + max_sx * (1.0 - blank));
    double sy = 1.0 / (min_sy * blank + max_sy * (1.0 - blank));
    if (!std::isfinite(sx) || !std::isfinite(sy)) return false;
    sx = std::fmin(std::fmax(sx, min_scale), max_scale);
    sy = std::fmin(std::fmax(sy, min_scale), max_scale);
    out_w = (int)std::fmax(1.0, sx * width);
    out_h = (int)std::fmax(1.0, sy * height);
    out_pinhole[2] = cx * out_w / width;
    out_pinhole[3] = cy * out_h / height;
    return true;
}

// argument check shared by mpmvs_undistort_camera and the host statement
inline bool und_options_ok(int width, int height, double blank, double min_scale, double max_scale) {
    return width > 0 && height > 0 && blank >= 0.0 && blank <= 1.0 && min_scale > 0.0 && min_scale <= max_scale && std::isfinite(max_scale);
}

// ---- the warp, per output pixel (shared by the kernel and the host statement) -------------------------------------------------
// source position of output pixel (X, Y) of the pinhole (fx', fy', cx', cy'): sx = x - 0.5, sy = y - 0.5 of the forward map.
// Valid iff 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN is invalid).
struct UndTap {
    bool valid;
    int x0, x1, y0, y1;
    double ax, ay;
};
UND_HD UndTap und_tap(const UndModel& m, const double* dst_pinhole, int X, int Y, int W, int H) {
    const double u = (X + 0.5 - dst_pinhole[2]) / dst_pinhole[0], v = (Y + 0.5 - dst_pinhole[3]) / dst_pinhole[1];
    double x, y;
    und_img_from_cam(m, u, v, x, y);
    const double sx = x - 0.5, sy = y - 0.5;
    UndTap t;
    t.valid = sx >= 0.0 && sx <= (double)(W - 1) && sy >= 0.0 && sy <= (double)(H - 1);
    if (!t.valid) {
        t.x0 = t.x1 = t.y0 = t.y1 = 0;
        t.ax = t.ay = 0.0;
        return t;
    }
    const double fx0 = floor(sx), fy0 = floor(sy);
    t.x0 = (int)fx0;
    t.y0 = (int)fy0;
    t.ax = sx - fx0;
    t.ay = sy - fy0;
    t.x1 = t.x0 + 1 < W - 1 ? t.x0 + 1 : W - 1;   // at the last column / row the second tap repeats the first, its weight is 0
    t.y1 = t.y0 + 1 < H - 1 ? t.y0 + 1 : H - 1;
    return t;
}
// one channel: fp64 bilinear value, rounded as (int)(val + 0.5)
UND_HD unsigned char und_blend(const UndTap& t, double s00, double s10, double s01, double s11) {
    const double top = s00 + t.ax * (s10 - s00);
    const double bot = s01 + t.ax * (s11 - s01);
    const double val = top + t.ay * (bot - top);
    return (unsigned char)(int)(val + 0.5);
}
