// mesh_distance_check.cpp -- the passes of csrc/pm_surface.hpp replayed on the host through the header's own __host__ __device__ code:
// the init, scatter and finish bodies of mpmvs_surface_distance thread by thread in scrambled orders on a grid built by replaying
// pm_cloud.hpp (the atomic minimum as a plain minimum), the large-triangle path with its lanes in scrambled order and with the
// threshold forced low and high, and the count and emit bodies of mpmvs_surface_sample; each against a plain loop written out below,
// which knows no grid: every (point, triangle) pair, and every sample by two nested loops over the lattice.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_distance_check tools/mesh_distance_check.cpp && build/mesh_distance_check
// Prints one line per case and "all equal"; exit status 1 if an output differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "pm_surface.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = (nblk_rev ? ((size_t)(count) + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_]; \
            if (i < (size_t)(count)) call;                                                   \
        }

static bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
static int failures = 0;

struct Mesh {
    std::vector<float> xyz;
    std::vector<int32_t> tri;
    std::vector<unsigned char> rgb;
    size_t m() const { return tri.size() / 3; }
};

struct Grid {
    std::vector<unsigned long long> keys;
    std::vector<int> off;
    std::vector<uint4> pts;
    SurfaceGrid S;
    long long n_fin = 0;
};

// the grid build of the cloud handle, replayed, and the SurfaceGrid as mpmvs_surface_distance fills it
static bool build(const std::vector<float>& t, float radius, int large, Grid& G) {
    const size_t n = t.size() / 3;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    G.n_fin = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!finite3(&t[3 * i])) continue;
        for (int a = 0; a < 3; ++a) {
            mn[a] = G.n_fin ? std::min(mn[a], t[3 * i + a]) : t[3 * i + a];
            mx[a] = G.n_fin ? std::max(mx[a], t[3 * i + a]) : t[3 * i + a];
        }
        ++G.n_fin;
    }
    if (!G.n_fin) return false;
    const size_t slots = (size_t)1 << cloud_slots_log2(G.n_fin);
    const double edge = cloud_edge(radius);
    G.keys.assign(slots, kCloudEmpty); G.off.assign(slots + 1, 0); G.pts.assign((size_t)G.n_fin, uint4{0, 0, 0, 0});
    std::vector<int> cnt(slots, 0), slot_of(n);
    REPLAY(n, cloud_insert_one(i, t.data(), (double)mn[0], (double)mn[1], (double)mn[2], edge, (unsigned)(slots - 1), G.keys.data(), cnt.data(), slot_of.data()));
    for (size_t s = 0; s < slots; ++s) G.off[s + 1] = G.off[s] + cnt[s];
    REPLAY(n, cloud_scatter_one(i, t.data(), slot_of.data(), G.off.data(), cnt.data(), G.pts.data()));
    CloudGrid& g = G.S.g;
    for (int a = 0; a < 3; ++a) g.mn[a] = (double)mn[a];
    g.edge = edge; g.r2 = radius * radius; g.mask = (unsigned)(slots - 1);
    g.keys = G.keys.data(); g.off = G.off.data(); g.pts = G.pts.data();
    G.S.gmax = 0.0;
    for (int a = 0; a < 3; ++a) {
        G.S.hi[a] = std::min(std::max(cloud_cell(mx[a], g.mn[a], edge), 0), kCloudAxisCells - 1);
        G.S.gmax = std::max(G.S.gmax, std::max(std::fabs((double)mn[a]), std::fabs((double)mx[a]) + edge));
    }
    G.S.reach = ((double)radius + 0.8660254037844387 * edge) * (1.0 + 0x1p-8);
    G.S.large = large;
    return true;
}

// ---- the plain loop of the distance: its own arithmetic, no grid -----------------------------------------------------------------------
static double dot3(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
static float plain_d2(const float* fa, const float* fb, const float* fc, const float* fq) {
    double A[3], B[3], C[3], q[3], ab[3], ac[3], ap[3], bp[3], cp[3], X[3];
    for (int k = 0; k < 3; ++k) {
        A[k] = fa[k]; B[k] = fb[k]; C[k] = fc[k]; q[k] = fq[k];
        ab[k] = B[k] - A[k]; ac[k] = C[k] - A[k]; ap[k] = q[k] - A[k]; bp[k] = q[k] - B[k]; cp[k] = q[k] - C[k];
    }
    const double s1 = dot3(ab, ap), s2 = dot3(ac, ap), s3 = dot3(ab, bp), s4 = dot3(ac, bp), s5 = dot3(ab, cp), s6 = dot3(ac, cp);
    const double vc = s1 * s4 - s3 * s2, vb = s5 * s2 - s1 * s6, va = s3 * s6 - s5 * s4;
    int rule = 7;
    if (s1 <= 0 && s2 <= 0) rule = 1;
    else if (s3 >= 0 && s4 <= s3) rule = 2;
    else if (vc <= 0 && s1 >= 0 && s3 <= 0) rule = 3;
    else if (s6 >= 0 && s5 <= s6) rule = 4;
    else if (vb <= 0 && s2 >= 0 && s6 <= 0) rule = 5;
    else if (va <= 0 && (s4 - s3) >= 0 && (s5 - s6) >= 0) rule = 6;
    for (int k = 0; k < 3; ++k) {
        switch (rule) {
            case 1: X[k] = A[k]; break;
            case 2: X[k] = B[k]; break;
            case 3: X[k] = A[k] + (s1 / (s1 - s3)) * ab[k]; break;
            case 4: X[k] = C[k]; break;
            case 5: X[k] = A[k] + (s2 / (s2 - s6)) * ac[k]; break;
            case 6: X[k] = B[k] + ((s4 - s3) / ((s4 - s3) + (s5 - s6))) * (C[k] - B[k]); break;
            default: {
                const double den = (va + vb) + vc;
                X[k] = (A[k] + (vb / den) * ab[k]) + (vc / den) * ac[k];
            }
        }
    }
    const double e[3] = {q[0] - X[0], q[1] - X[1], q[2] - X[2]};
    return (float)((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

static void plain_distance(const Mesh& M, const std::vector<float>& pts, float radius, std::vector<float>& d2, std::vector<int32_t>& arg, long long counts[2]) {
    const size_t n = pts.size() / 3;
    const float r2 = radius * radius;
    d2.assign(n, std::numeric_limits<float>::infinity());
    arg.assign(n, -1);
    counts[0] = counts[1] = 0;
    std::vector<char> t_ok(M.m());
    for (size_t t = 0; t < M.m(); ++t)
        t_ok[t] = finite3(&M.xyz[3 * (size_t)M.tri[3 * t]]) && finite3(&M.xyz[3 * (size_t)M.tri[3 * t + 1]]) && finite3(&M.xyz[3 * (size_t)M.tri[3 * t + 2]]);
    for (size_t i = 0; i < n; ++i) {
        if (!finite3(&pts[3 * i])) continue;
        ++counts[1];
        for (size_t t = 0; t < M.m(); ++t) {
            if (!t_ok[t]) continue;
            const float D = plain_d2(&M.xyz[3 * (size_t)M.tri[3 * t]], &M.xyz[3 * (size_t)M.tri[3 * t + 1]], &M.xyz[3 * (size_t)M.tri[3 * t + 2]], &pts[3 * i]);
            if (!(D <= r2)) continue;
            if (arg[i] < 0 || D < d2[i]) d2[i] = D, arg[i] = (int32_t)t;
        }
        if (arg[i] >= 0) ++counts[0];
    }
}

// one distance case at one threshold: the three passes replayed, the listed triangles by 256 lanes in a scrambled order
static void distance_case(const char* name, const Mesh& M, const std::vector<float>& pts, float radius, std::mt19937& rng, std::vector<int> larges = {kSurfaceLargeDefault, 0, 1 << 30}) {
    std::vector<float> want_d2;
    std::vector<int32_t> want_arg;
    long long want_counts[2];
    plain_distance(M, pts, radius, want_d2, want_arg, want_counts);
    const size_t n = pts.size() / 3, m = M.m();
    for (int large : larges) {
        std::shuffle(order256, order256 + 256, rng);
        nblk_rev = !nblk_rev;
        Grid G;
        std::vector<float> d2(n, -7.0f);
        std::vector<int32_t> arg(n, -7);
        long long found = 0;
        size_t listed = 0;
        if (build(pts, radius, large, G)) {
            std::vector<unsigned long long> keys(n, 0);
            std::vector<int32_t> list(std::max<size_t>(m, 1), -1);
            unsigned long long n_list = 0;
            REPLAY(n, surface_init_one(i, keys.data()));
            REPLAY(m, surface_scatter_one(i, M.xyz.data(), M.tri.data(), G.S, keys.data(), list.data(), &n_list));
            listed = (size_t)n_list;
            std::vector<int> lanes(256);
            std::iota(lanes.begin(), lanes.end(), 0);
            for (size_t k = 0; k < listed; ++k) {
                std::shuffle(lanes.begin(), lanes.end(), rng);
                for (int lane : lanes) surface_large_lane(k, lane, 256, M.xyz.data(), M.tri.data(), G.S, keys.data(), list.data());
            }
            REPLAY(n, found += surface_finish_one(i, keys.data(), d2.data(), arg.data()) ? 1 : 0);
        } else {   // no finite point: the entry point answers on the host
            d2.assign(n, std::numeric_limits<float>::infinity());
            arg.assign(n, -1);
        }
        const bool ok = std::memcmp(d2.data(), want_d2.data(), n * 4) == 0 && arg == want_arg && found == want_counts[0];
        printf("distance %s, radius %g, large > %d (%zu of %zu triangles listed), %lld of %lld points with a candidate: %s\n", name, (double)radius, large, listed, m,
               want_counts[0], want_counts[1], ok ? "equal" : "DIFFERS");
        if (!ok) ++failures;
    }
}

// ---- the plain loop of the sampler: rows and columns of the lattice, no k -> (i, l) arithmetic ---------------------------------------------
static void plain_sample(const Mesh& M, float spacing, bool color, std::vector<float>& xyz, std::vector<int32_t>& of, std::vector<unsigned char>& rgb, std::vector<float>& nrm,
                         long long* first_bad) {
    *first_bad = -1;
    const double h = (double)spacing;
    for (size_t t = 0; t < M.m(); ++t) {
        const float* f[3] = {&M.xyz[3 * (size_t)M.tri[3 * t]], &M.xyz[3 * (size_t)M.tri[3 * t + 1]], &M.xyz[3 * (size_t)M.tri[3 * t + 2]]};
        if (!(finite3(f[0]) && finite3(f[1]) && finite3(f[2]))) continue;
        double P[3][3], l2 = 0.0;
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) P[c][a] = (double)f[c][a];
        for (int c = 0; c < 3; ++c) {
            const double* U = P[c];
            const double* V = P[(c + 1) % 3];
            const double dx = V[0] - U[0], dy = V[1] - U[1], dz = V[2] - U[2];
            l2 = std::max(l2, (dx * dx + dy * dy) + dz * dz);
        }
        const double ratio = std::sqrt(l2) / h;
        if (!(ratio <= 4096.0)) {
            if (*first_bad < 0) *first_bad = (long long)t;
            continue;
        }
        const long long s = std::max(1ll, (long long)std::ceil(ratio));
        const double u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        const double C[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double L = std::sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2]);
        for (long long i = 0; i < s; ++i)               // row i has 2 (s - i) - 1 sub-triangles, upright and inverted alternating
            for (long long l = 0; l < 2 * (s - i) - 1; ++l) {
                const long long j = l / 2, na = 3 * i + 1 + (l % 2), nb = 3 * j + 1 + (l % 2), nc = 3 * s - na - nb;
                for (int a = 0; a < 3; ++a) xyz.push_back((float)((((double)na * P[0][a] + (double)nb * P[1][a]) + (double)nc * P[2][a]) / (double)(3 * s)));
                of.push_back((int32_t)t);
                if (color)
                    for (int a = 0; a < 3; ++a) {
                        const long long ca = M.rgb[3 * (size_t)M.tri[3 * t] + a], cb = M.rgb[3 * (size_t)M.tri[3 * t + 1] + a], cc = M.rgb[3 * (size_t)M.tri[3 * t + 2] + a];
                        rgb.push_back((unsigned char)((2 * (na * ca + nb * cb + nc * cc) + 3 * s) / (6 * s)));
                    }
                for (int a = 0; a < 3; ++a) nrm.push_back((L > 0.0 && std::isfinite(L)) ? (float)(C[a] / L) : 0.0f);
            }
    }
}

static void sample_case(const char* name, const Mesh& M, float spacing, std::mt19937& rng) {
    const bool color = !M.rgb.empty();
    std::vector<float> want_xyz, want_nrm;
    std::vector<int32_t> want_of;
    std::vector<unsigned char> want_rgb;
    long long want_bad;
    plain_sample(M, spacing, color, want_xyz, want_of, want_rgb, want_nrm, &want_bad);
    std::shuffle(order256, order256 + 256, rng);
    nblk_rev = !nblk_rev;
    const size_t m = M.m();
    std::vector<int> cnt(m, -7), off(m, 0);
    uint32_t first_bad = 0xffffffffu;
    unsigned long long total = 0;
    REPLAY(m, total += (unsigned long long)surface_count_one(i, M.xyz.data(), M.tri.data(), (double)spacing, cnt.data(), &first_bad));
    bool ok = (first_bad == 0xffffffffu ? -1 : (long long)first_bad) == want_bad;
    size_t K = 0;
    if (ok && want_bad < 0) {
        for (size_t t = 0; t < m; ++t) off[t] = (int)K, K += (size_t)cnt[t];
        ok = K == total && K == want_of.size();
        if (ok && K) {
            std::vector<float> xyz(3 * K, -7.0f), nrm(3 * K, -7.0f);
            std::vector<int32_t> of(K, -7);
            std::vector<unsigned char> rgb(color ? 3 * K : 0, 7);
            REPLAY(K, surface_emit_one(i, M.xyz.data(), color ? M.rgb.data() : nullptr, M.tri.data(), (int)m, (double)spacing, off.data(), xyz.data(), of.data(),
                                       color ? rgb.data() : nullptr, nrm.data()));
            ok = std::memcmp(xyz.data(), want_xyz.data(), 12 * K) == 0 && of == want_of && rgb == want_rgb && std::memcmp(nrm.data(), want_nrm.data(), 12 * K) == 0;
        }
    }
    printf("sample %s, spacing %g, %zu triangles, %zu samples, first beyond the limit %lld: %s\n", name, (double)spacing, m, K, want_bad, ok ? "equal" : "DIFFERS");
    if (!ok) ++failures;
}

// ---- scenes ------------------------------------------------------------------------------------------------------------------------------
static Mesh random_mesh(std::mt19937& rng, int nt, float box, float size, bool color) {
    std::uniform_real_distribution<float> c(-box, box), d(-size, size);
    Mesh M;
    for (int t = 0; t < nt; ++t) {
        const float o[3] = {c(rng), c(rng), c(rng)};
        for (int k = 0; k < 3; ++k) {
            for (int a = 0; a < 3; ++a) M.xyz.push_back(o[a] + d(rng));
            M.tri.push_back(3 * t + k);
            if (color)
                for (int a = 0; a < 3; ++a) M.rgb.push_back((unsigned char)(rng() & 255));
        }
    }
    return M;
}
static std::vector<float> random_points(std::mt19937& rng, int n, float box) {
    std::uniform_real_distribution<float> c(-box, box);
    std::vector<float> p((size_t)3 * n);
    for (float& v : p) v = c(rng);
    return p;
}

int main() {
    std::mt19937 rng(20260);
    std::iota(order256, order256 + 256, 0u);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // random triangles among random points, at radii below, at and above the triangles' size
    for (float radius : {0.05f, 0.3f, 1.5f}) {
        Mesh M = random_mesh(rng, 300, 2.0f, 0.4f, false);
        distance_case("300 random triangles, 3000 points", M, random_points(rng, 3000, 2.2f), radius, rng);
    }
    {   // a lattice of points on cell borders: coordinates at multiples of the radius, the triangle corners too
        std::vector<float> p;
        for (int z = 0; z < 6; ++z)
            for (int y = 0; y < 12; ++y)
                for (int x = 0; x < 12; ++x) p.insert(p.end(), {0.25f * x, 0.25f * y, 0.25f * z});
        Mesh M;
        M.xyz = {0.5f, 0.5f, 0.5f, 2.0f, 0.75f, 0.5f, 1.0f, 2.25f, 0.75f, 0.0f, 0.0f, 0.0f, 2.75f, 0.0f, 0.0f, 0.0f, 2.75f, 1.25f};
        M.tri = {0, 1, 2, 3, 4, 5, 2, 1, 0, 0, 1, 2};   // with a reversed and a repeated triangle: the smallest index wins
        for (float radius : {0.25f, 0.5f}) distance_case("a lattice of points on cell borders", M, p, radius, rng);
    }
    {   // a triangle larger than the whole grid, and one wholly outside the cloud's box
        Mesh M;
        M.xyz = {-100, -100, 0.1f, 100, -100, -0.1f, 0, 150, 0.0f, 50, 50, 50, 60, 50, 50, 50, 60, 55};
        M.tri = {0, 1, 2, 3, 4, 5};
        distance_case("a triangle larger than the grid and one outside it", M, random_points(rng, 2000, 1.0f), 0.125f, rng);
        M.tri = {3, 4, 5};
        distance_case("a triangle wholly outside the cloud's box", M, random_points(rng, 500, 1.0f), 0.125f, rng);
    }
    {   // 70 001 points in one cell against one triangle
        std::vector<float> p = random_points(rng, 70001, 0.01f);
        Mesh M;
        M.xyz = {-0.02f, -0.02f, 0.001f, 0.03f, -0.01f, -0.002f, 0.0f, 0.03f, 0.0f};
        M.tri = {0, 1, 2};
        distance_case("70001 points in one cell, one triangle", M, p, 1.0f, rng, {kSurfaceLargeDefault, 0});
    }
    {   // 70 001 triangles over one point (and a second point far off)
        Mesh M = random_mesh(rng, 70001, 0.05f, 0.2f, false);
        distance_case("70001 triangles over one point", M, {0.01f, -0.02f, 0.03f, 5.0f, 5.0f, 5.0f}, 0.5f, rng, {kSurfaceLargeDefault, 0});
    }
    {   // non-finite vertices and points; a cloud without a finite point
        Mesh M = random_mesh(rng, 60, 1.0f, 0.5f, false);
        M.xyz[4] = nan; M.xyz[40] = inf; M.xyz[100] = -inf;
        std::vector<float> p = random_points(rng, 700, 1.2f);
        p[5] = nan; p[300] = inf; p[901] = -inf;
        distance_case("non-finite vertices and points", M, p, 0.4f, rng);
        distance_case("no finite point", M, {nan, 0, 0, 0, inf, 0}, 0.4f, rng, {kSurfaceLargeDefault});
    }
    {   // degenerate triangles follow the sequence literally
        Mesh M;
        M.xyz = {0, 0, 0, 0, 0, 0, 1, 0, 0, 0.5f, 0.5f, 0.5f};
        M.tri = {0, 0, 0, 0, 1, 2, 0, 2, 2, 3, 3, 3, 0, 2, 3};
        distance_case("degenerate triangles", M, random_points(rng, 800, 1.0f), 0.6f, rng);
    }

    // the sampler: a fan of one huge and many tiny triangles, colours, non-finite vertices, a zero-size triangle, the limit
    {
        Mesh M = random_mesh(rng, 400, 1.0f, 0.01f, true);
        for (int a = 0; a < 9; ++a) M.xyz[a] = (a % 4 == 0) ? 3.0f : -2.0f + 0.7f * a;   // triangle 0 is huge
        M.xyz[9 * 7 + 2] = nan;
        for (int a = 0; a < 9; ++a) M.xyz[9 * 9 + a] = M.xyz[9 * 9 + a % 3];               // triangle 9 has size 0
        for (float spacing : {0.05f, 0.01f, 0.5f, 8.0f}) sample_case("one huge among 400 tiny, with colour", M, spacing, rng);
        sample_case("beyond the limit of 4096", M, 0.0005f, rng);
    }
    {
        Mesh M;
        M.xyz = {3, 4, 0, 0, 0, 0, 0, 4, 0};
        M.tri = {0, 1, 2};
        for (float spacing : {5.0f, 2.5f, 5.0f / 3.0f, 5.0f / 7.0f, std::nextafter(2.5f, 0.0f), std::nextafter(2.5f, 9.0f)}) sample_case("the 3-4-5 triangle", M, spacing, rng);
        sample_case("random triangles without colour", random_mesh(rng, 1000, 5.0f, 1.0f, false), 0.11f, rng);
    }

    if (failures) {
        printf("%d case(s) DIFFER\n", failures);
        return 1;
    }
    printf("all equal\n");
    return 0;
}
