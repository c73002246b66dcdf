// mesh_render_check.cpp -- the passes of csrc/pm_raster.hpp replayed on the host through the header's own __host__ __device__ code:
// the init, small, large and resolve bodies of mpmvs_surface_render_depth thread by thread in scrambled orders (the atomic minimum as a
// plain minimum), both launches of the large pass (a wave per pair; a block per slice of a pair) with their items and lanes scrambled
// and one setup per item, the threshold forced low and high, with buffers of exactly the library's
// sizes; each against a plain loop written out below, which knows no box, no list and no early exit: every (triangle, pixel) pair.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_render_check tools/mesh_render_check.cpp && build/mesh_render_check [thin]
// `thin` (a number, default 1) divides the random cases' sizes.  Prints one line per case and "all equal"; exit status 1 if an output
// differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "pm_raster.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = (nblk_rev ? ((size_t)(count) + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_]; \
            if (i < (size_t)(count)) call;                                                   \
        }

static int failures = 0;

struct Cam {
    float K[9], R[9], t[3];
    int w, h;
};
struct Scene {
    std::vector<float> xyz;
    std::vector<int32_t> tri;
    std::vector<Cam> cams;
    size_t m() const { return tri.size() / 3; }
};
struct Maps {
    std::vector<std::vector<float>> depth;
    std::vector<std::vector<int32_t>> tri;
    long long pairs = 0, covered = 0, listed = 0, split = 0;
};

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// THE PLAIN LOOP, from include/mpmvs.h
static void plain(const Scene& s, Maps& out) {
    out = Maps();
    for (const Cam& c : s.cams) {
        const size_t npix = (size_t)c.w * (size_t)c.h;
        std::vector<unsigned long long> keys(npix, 0x7f800000ffffffffull);
        for (size_t i = 0; i < s.m(); ++i) {
            double q[3][3];
            bool fin = true;
            for (int v = 0; v < 3; ++v) {
                const float* p = &s.xyz[3 * (size_t)s.tri[3 * i + v]];
                double X[3];
                for (int j = 0; j < 3; ++j) {
                    const double a = (double)c.R[3 * j] * (double)p[0], b = (double)c.R[3 * j + 1] * (double)p[1], d = (double)c.R[3 * j + 2] * (double)p[2];
                    const double ab = a + b, abd = ab + d;
                    X[j] = abd + (double)c.t[j];
                }
                for (int j = 0; j < 3; ++j) {
                    const double a = (double)c.K[3 * j] * X[0], b = (double)c.K[3 * j + 1] * X[1], d = (double)c.K[3 * j + 2] * X[2];
                    const double ab = a + b;
                    q[v][j] = ab + d;
                    fin = fin && std::isfinite(q[v][j]);
                }
            }
            const double zhi = std::max(q[0][2], std::max(q[1][2], q[2][2])), zlo = std::min(q[0][2], std::min(q[1][2], q[2][2]));
            if (!fin || !(zhi > 0.0)) continue;
            ++out.pairs;
            double n[3][3];
            const int e[3][2] = {{1, 2}, {2, 0}, {0, 1}};
            for (int k = 0; k < 3; ++k) {
                const double *u = q[e[k][0]], *v = q[e[k][1]];
                n[k][0] = u[1] * v[2] - u[2] * v[1];
                n[k][1] = u[2] * v[0] - u[0] * v[2];
                n[k][2] = u[0] * v[1] - u[1] * v[0];
            }
            const double d01 = q[0][0] * n[0][0] + q[0][1] * n[0][1], det = d01 + q[0][2] * n[0][2];
            for (int y = 0; y < c.h; ++y)
                for (int x = 0; x < c.w; ++x) {
                    double E[3];
                    for (int k = 0; k < 3; ++k) {
                        const double a = (double)x * n[k][0] + (double)y * n[k][1];
                        E[k] = a + n[k][2];
                    }
                    const double S01 = E[0] + E[1], S = S01 + E[2];
                    const bool pos = E[0] >= 0 && E[1] >= 0 && E[2] >= 0, neg = E[0] <= 0 && E[1] <= 0 && E[2] <= 0;
                    if (!(pos || neg) || !(S != 0)) continue;
                    double z = det / S;
                    if (z < zlo) z = zlo;
                    if (z > zhi) z = zhi;
                    const float zf = (float)z;
                    if (!(std::isfinite(zf) && zf > 0.0f)) continue;
                    const unsigned long long key = ((unsigned long long)bits_of(zf) << 32) | (unsigned long long)i;
                    unsigned long long& k = keys[(size_t)y * (size_t)c.w + (size_t)x];
                    k = std::min(k, key);
                }
        }
        std::vector<float> d(npix);
        std::vector<int32_t> a(npix);
        for (size_t p = 0; p < npix; ++p) {
            const bool none = keys[p] == 0x7f800000ffffffffull;
            const uint32_t b = (uint32_t)(keys[p] >> 32);
            float f;
            std::memcpy(&f, &b, 4);
            d[p] = none ? 0.0f : f;
            a[p] = none ? -1 : (int32_t)(keys[p] & 0xffffffffull);
            out.covered += none ? 0 : 1;
        }
        out.depth.push_back(d);
        out.tri.push_back(a);
    }
}

// the library's call, replayed: chunks of kRasterChunk views, every buffer of exactly the size mpmvs_surface_render_depth asks for
static void replay(const Scene& s, int large, std::mt19937& rng, Maps& out) {
    out = Maps();
    const size_t m = s.m();
    for (size_t v0 = 0; v0 < s.cams.size(); v0 += kRasterChunk) {
        const size_t v1 = std::min(s.cams.size(), v0 + (size_t)kRasterChunk);
        size_t total = 0;
        for (size_t v = v0; v < v1; ++v) total += (size_t)s.cams[v].w * (size_t)s.cams[v].h;
        std::vector<unsigned long long> keys(total);
        std::vector<float> depth(total);
        std::vector<int32_t> arg(total);
        const size_t cap = m * (v1 - v0);
        std::vector<unsigned long long> list(cap);
        unsigned long long n_list[2] = {0, 0};
        RasterTally tally = {0, 0, 0};
        RasterChunkArgs A;
        std::memset(&A, 0, sizeof A);
        A.n = (int)(v1 - v0);
        A.large = large;
        size_t at = 0;
        for (size_t v = v0; v < v1; ++v) {
            RasterView& V = A.v[v - v0];
            std::memcpy(V.K, s.cams[v].K, sizeof V.K);
            std::memcpy(V.R, s.cams[v].R, sizeof V.R);
            std::memcpy(V.t, s.cams[v].t, sizeof V.t);
            V.w = s.cams[v].w, V.h = s.cams[v].h;
            V.keys = keys.data() + at;
            at += (size_t)V.w * (size_t)V.h;
        }
        std::shuffle(order256, order256 + 256, rng);
        nblk_rev = (rng() & 1) != 0;
        REPLAY(total, raster_init_one(i, keys.data()));
        REPLAY(m, raster_small_one(i, s.xyz.data(), s.tri.data(), A, list.data(), cap, n_list, tally));
        out.pairs += (long long)tally.part;
        // the large pass, both launches as k_raster_large runs them: the items in a scrambled order, one setup per item, its lanes in another
        for (int split = 0; split < 2; ++split) {
            std::vector<size_t> items(split ? (size_t)n_list[1] * kRasterSlices : (size_t)n_list[0]);
            std::iota(items.begin(), items.end(), (size_t)0);
            std::shuffle(items.begin(), items.end(), rng);
            const unsigned lanes = split ? 256u : 64u;
            for (size_t item : items) {
                const unsigned long long e = split ? list[cap - 1 - item / kRasterSlices] : list[item];
                const uint32_t slice = split ? (uint32_t)(item % kRasterSlices) : 0u;
                RasterTri T;
                if (!raster_large_setup(T, e, s.xyz.data(), s.tri.data(), A)) continue;
                std::shuffle(order256, order256 + 256, rng);
                for (unsigned l = 0; l < 256; ++l)
                    if (order256[l] < lanes) raster_large_lane(T, e, A, slice * 256u * (split ? 1u : 0u) + order256[l], split ? (uint32_t)kRasterSlices * 256u : 64u);
            }
        }
        REPLAY(total, out.covered += raster_resolve_one(i, keys.data(), depth.data(), arg.data()) ? 1 : 0);
        out.listed += (long long)(n_list[0] + n_list[1]);
        out.split += (long long)n_list[1];
        at = 0;
        for (size_t v = v0; v < v1; ++v) {
            const size_t npix = (size_t)s.cams[v].w * (size_t)s.cams[v].h;
            out.depth.emplace_back(depth.begin() + at, depth.begin() + at + npix);
            out.tri.emplace_back(arg.begin() + at, arg.begin() + at + npix);
            at += npix;
        }
    }
}

static void check(const std::string& name, const Scene& s, std::mt19937& rng) {
    Maps want;
    plain(s, want);
    for (int large : {0, kRasterLargeDefault, 1 << 30}) {
        Maps got;
        replay(s, large, rng, got);
        bool eq = got.pairs == want.pairs && got.covered == want.covered && got.depth.size() == want.depth.size();
        for (size_t v = 0; eq && v < want.depth.size(); ++v)
            eq = std::memcmp(got.depth[v].data(), want.depth[v].data(), want.depth[v].size() * 4) == 0 && got.tri[v] == want.tri[v];
        if (large == 0) eq = eq && got.listed == got.pairs;
        if (large == 1 << 30) eq = eq && got.listed == 0;
        std::printf("%s, large %d: %lld pairs, %lld covered, listed %lld of %lld (%lld shared by blocks): %s\n", name.c_str(), large, want.pairs, want.covered,
                    got.listed, got.pairs, got.split, eq ? "equal" : "DIFFERENT");
        if (!eq) ++failures;
    }
}

static Cam look_at(const double eye[3], const double target[3], double f, int w, int h, double skew = 0.0, double k6 = 0.0, double k7 = 0.0) {
    double z[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
    const double zl = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double& a : z) a /= zl;
    double up[3] = {0, 0, 1};
    if (std::fabs(z[2]) > 0.99) up[0] = 1, up[2] = 0;
    double x[3] = {z[1] * up[2] - z[2] * up[1], z[2] * up[0] - z[0] * up[2], z[0] * up[1] - z[1] * up[0]};
    const double xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    for (double& a : x) a /= xl;
    const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    Cam c;
    const double* rows[3] = {x, y, z};
    for (int j = 0; j < 3; ++j) {
        for (int a = 0; a < 3; ++a) c.R[3 * j + a] = (float)rows[j][a];
        c.t[j] = (float)-(rows[j][0] * eye[0] + rows[j][1] * eye[1] + rows[j][2] * eye[2]);
    }
    const float K[9] = {(float)f, (float)skew, (float)((w - 1) / 2.0), 0.0f, (float)f, (float)((h - 1) / 2.0), (float)k6, (float)k7, 1.0f};
    std::memcpy(c.K, K, sizeof K);
    c.w = w, c.h = h;
    return c;
}

static Cam origin_cam(double f, int w, int h) {
    const double eye[3] = {0, 0, 0}, target[3] = {0, 0, 1};
    Cam c = look_at(eye, target, f, w, h);
    const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(c.R, R, sizeof R);
    c.t[0] = c.t[1] = c.t[2] = 0.0f;
    return c;
}

static Scene soup(std::mt19937& rng, int m, int w, int h, int n_cams) {
    std::uniform_real_distribution<double> U(-1.5, 1.5), S(-0.1, 0.1), P(0.0, 1.0);
    Scene s;
    const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (int t = 0; t < m; ++t) {
        const double c[3] = {U(rng), U(rng), U(rng)};
        const bool big = P(rng) < 0.1;
        for (int v = 0; v < 3; ++v) {
            for (int a = 0; a < 3; ++a) s.xyz.push_back((float)(big ? U(rng) : c[a] + S(rng)));
            if (P(rng) < 0.01) s.xyz[s.xyz.size() - 1 - rng() % 3] = bad[rng() % 3];
            s.tri.push_back(3 * t + v);
        }
        if (P(rng) < 0.03) s.tri[3 * t + 1] = s.tri[3 * t];   // a repeated index
    }
    for (int k = 0; k < n_cams; ++k) {
        const double eye[3] = {U(rng) * (k % 3 == 0 ? 0.2 : 2.0), U(rng) * (k % 3 == 0 ? 0.2 : 2.0), U(rng)}, target[3] = {U(rng), U(rng), U(rng)};
        const int ww = k % 4 == 3 ? 1 : (k % 4 == 2 ? 5 : w), hh = k % 4 == 3 ? 1 : (k % 4 == 2 ? 4 : h);
        s.cams.push_back(look_at(eye, target, 0.9 * ww + 1, ww, hh, k % 2 ? 0.3 : 0.0, k % 2 ? 1e-4 : 0.0, k % 2 ? -2e-4 : 0.0));
    }
    return s;
}

int main(int argc, char** argv) {
    const int thin = argc > 1 ? std::max(1, std::atoi(argv[1])) : 1;
    std::mt19937 rng(20260);
    std::iota(order256, order256 + 256, 0u);

    // crossing and behind triangles, seen from the origin
    {
        Scene s;
        s.xyz = {-3, -2, 5, 3, -2, 5, 0, 1, -5,     // crosses the camera plane
                 -1, -1, -2, 1, -1, -3, 0, 1, -4,   // behind
                 -1, -1, 3, 1, -1, 3, 0, 1, 3,      // in front
                 -1, 0, 0, 1, 0, 0, 0, 1, 0};       // in the camera plane: max z = 0, takes no part
        s.tri = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
        s.cams = {origin_cam(80, 96, 64), origin_cam(4, 5, 4), origin_cam(1, 1, 1)};
        check("crossing and behind", s, rng);
    }
    // a triangle larger than the image, and one that fills it while crossing the plane
    {
        Scene s;
        s.xyz = {-100, -100, 4, 100, -100, 4, 0, 200, 4, -50, -60, 2, 50, -60, 2, 0, 90, -1};
        s.tri = {0, 1, 2, 3, 4, 5};
        s.cams = {origin_cam(90, 128, 96), origin_cam(5, 5, 4), origin_cam(1, 1, 1)};   // 12 288 pixels: above kRasterSplit
        check("larger than the image", s, rng);
    }
    // degenerate triangles and non-finite vertices
    {
        Scene s;
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        s.xyz = {0, 0, 2, 1, 0, 2, 0, 1, 2, 2, 0, 2, nan, 0, 2, 0, inf, 2, 1e30f, 1e30f, 1e30f, -1e30f, 1e30f, 1e30f, 0, -1e30f, 1e30f};
        s.tri = {0, 0, 0, 0, 0, 1, 0, 1, 3, 0, 1, 2, 0, 1, 4, 5, 1, 2, 6, 7, 8};
        s.cams = {origin_cam(20, 50, 37), origin_cam(3e30, 5, 4)};
        check("degenerate and non-finite", s, rng);
    }
    // 70 001 copies of one triangle over one pixel, and over a 5 x 4 image
    {
        Scene s;
        s.xyz = {-1, -1, 2, 1, -1, 2, 0, 1, 2};
        for (int k = 0; k < 70001 / (thin > 1 ? 7 : 1); ++k) s.tri.insert(s.tri.end(), {0, 1, 2});
        s.cams = {origin_cam(1, 1, 1), origin_cam(4, 5, 4)};
        check("copies over one pixel", s, rng);
    }
    // random soups: tiny and small images, two chunks of views (9 cameras)
    for (int k = 0; k < std::max(2, 12 / thin); ++k) {
        const Scene s = soup(rng, std::max(20, (50 + 150 * k) / thin), 50, 37, k % 3 == 0 ? 9 : 3);
        check("soup " + std::to_string(k), s, rng);
    }
    if (failures) {
        std::printf("%d cases differ\n", failures);
        return 1;
    }
    std::printf("all equal\n");
    return 0;
}
