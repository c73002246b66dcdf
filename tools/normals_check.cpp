// normals_check.cpp -- the normal estimation of csrc/pm_normals.hpp replayed on the host, thread by thread in a scrambled order,
// through the header's own __host__ __device__ code (the grid build and the query binning of pm_cloud.hpp, then normal_one<K> per
// thread for every list size K), with buffers of exactly the sizes mpmvs_cloud_normals of mpmvs_cloud.hip gives them, against the loop
// of include/mpmvs.h written out below on its own: a plain sort of all candidates, the matrix and V as arrays.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/normals_check tools/normals_check.cpp && build/normals_check
// Prints one line per case and "all equal"; exit status 1 if an output differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_normals.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = (nblk_rev ? ((size_t)(count) + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_]; \
            if (i < (size_t)(count)) call;                                                   \
        }

static bool finite3(const float* p) { return cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]); }
static int failures = 0;

struct Grid {
    std::vector<unsigned long long> keys;
    std::vector<int> off;
    std::vector<uint4> pts;
    CloudGrid g;
    long long n_fin = 0;
};

// the grid build of cloud_build, replayed
static bool build(const std::vector<float>& t, float radius, Grid& G) {
    const size_t n = t.size() / 3;
    float mn[3] = {0, 0, 0};
    G.n_fin = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!finite3(&t[3 * i])) continue;
        for (int a = 0; a < 3; ++a) mn[a] = G.n_fin ? std::min(mn[a], t[3 * i + a]) : t[3 * i + a];
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
    for (int a = 0; a < 3; ++a) G.g.mn[a] = (double)mn[a];
    G.g.edge = edge; G.g.r2 = radius * radius; G.g.mask = (unsigned)(slots - 1);
    G.g.keys = G.keys.data(); G.g.off = G.off.data(); G.g.pts = G.pts.data();
    return true;
}

// the serving order of the n points: k_cloud_qbin, the scan, k_cloud_qorder
static void bin(const float* q, size_t nq, const CloudGrid& g, std::vector<int>& order) {
    int lg = 8;
    while ((1ll << lg) < (long long)nq) ++lg;
    const size_t bins = (size_t)1 << lg;
    std::vector<int> qcnt(bins, 0), qbin(nq), qoff(bins + 1, 0);
    order.assign(nq, -1);
    REPLAY(nq, cloud_qbin_one(i, q, g, (unsigned)(bins - 1), qcnt.data(), qbin.data()));
    for (size_t b = 0; b < bins; ++b) qoff[b + 1] = qoff[b] + qcnt[b];
    REPLAY(nq, cloud_qorder_one(i, qbin.data(), qoff.data(), qcnt.data(), order.data()));
}

// ---- the loop of include/mpmvs.h for point i, on its own ------------------------------------------------------------------------
static double max0(double x) { return x > 0.0 ? x : 0.0; }

static void plain(const std::vector<float>& x, size_t i, float radius, int k, int orient, const double* view, const float* ref, float n_out[3], float& curv,
                  int32_t& within) {
    n_out[0] = n_out[1] = n_out[2] = 0.0f;
    curv = INFINITY;
    within = 0;
    const float* p = &x[3 * i];
    if (!finite3(p)) return;
    std::vector<unsigned long long> keys;
    const float r2 = radius * radius;
    for (size_t t = 0; t < x.size() / 3; ++t) {
        if (t == i || !finite3(&x[3 * t])) continue;
        const float dx = p[0] - x[3 * t], dy = p[1] - x[3 * t + 1], dz = p[2] - x[3 * t + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= r2) keys.push_back(((unsigned long long)cloud_bits(d2) << 32) | (unsigned)t);
    }
    std::sort(keys.begin(), keys.end());
    within = (int32_t)keys.size();
    const int m = std::min(k, (int)within);
    if (m < 2) return;
    double s[3] = {0, 0, 0}, A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int j = 0; j < m; ++j) {
        const float* q = &x[3 * (size_t)(keys[j] & 0xffffffffu)];
        const double e[3] = {(double)q[0] - (double)p[0], (double)q[1] - (double)p[1], (double)q[2] - (double)p[2]};
        for (int a = 0; a < 3; ++a) {
            s[a] = j == 0 ? e[a] : s[a] + e[a];
            for (int b = a; b < 3; ++b) A[a][b] = j == 0 ? e[a] * e[b] : A[a][b] + e[a] * e[b];
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) A[a][b] = A[b][a] = A[a][b] - (s[a] * s[b]) / (double)(m + 1);
    static const int pairs[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
    for (int sweep = 0; sweep < 8; ++sweep)
        for (const int* pq : pairs) {
            const int P = pq[0], Q = pq[1], R = pq[2];
            const double apq = A[P][Q];
            if (apq == 0.0) continue;
            const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
            const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
            const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
            A[P][P] = A[P][P] - t * apq;
            A[Q][Q] = A[Q][Q] + t * apq;
            A[P][Q] = A[Q][P] = 0.0;
            const double arp = A[R][P], arq = A[R][Q];
            A[R][P] = A[P][R] = c * arp - sn * arq;
            A[R][Q] = A[Q][R] = sn * arp + c * arq;
            for (int r = 0; r < 3; ++r) {
                const double vp = V[r][P], vq = V[r][Q];
                V[r][P] = c * vp - sn * vq;
                V[r][Q] = sn * vp + c * vq;
            }
        }
    const double d[3] = {A[0][0], A[1][1], A[2][2]};
    int i0 = 0;
    for (int a = 1; a < 3; ++a)
        if (d[a] < d[i0]) i0 = a;
    double dmid = INFINITY;
    for (int a = 0; a < 3; ++a)
        if (a != i0 && d[a] < dmid) dmid = d[a];
    if (!(dmid > 0.0)) return;
    const double tr = (max0(d[0]) + max0(d[1])) + max0(d[2]);
    double n[3] = {V[0][i0], V[1][i0], V[2][i0]};
    int lead = 0;
    for (int a = 1; a < 3; ++a)
        if (std::fabs(n[a]) > std::fabs(n[lead])) lead = a;
    if (n[lead] < 0.0)
        for (double& v : n) v = -v;
    if (orient != 0) {
        double w[3];
        for (int a = 0; a < 3; ++a) w[a] = orient == 1 ? view[a] - (double)p[a] : (double)ref[3 * i + a];
        const double dot = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2];
        if (dot < 0.0)
            for (double& v : n) v = -v;
    }
    for (int a = 0; a < 3; ++a) n_out[a] = (float)n[a];
    curv = (float)(max0(d[i0]) / tr);
}

// ---- one call of mpmvs_cloud_normals, replayed -------------------------------------------------------------------------------------
struct Result {
    std::vector<float> n, curv;
    std::vector<int32_t> within;
    std::vector<size_t> served;   // the points of the first `limit` threads
};

template <int K>
static void replay(const std::vector<float>& x, const Grid& G, int k, int orient, const double* view, const float* ref, bool use_bin, Result& out,
                   size_t limit = ~(size_t)0) {
    const size_t n = x.size() / 3, served = std::min(n, limit);   // `limit`: only the first threads run
    std::vector<int> order;
    if (use_bin) bin(x.data(), n, G.g, order);
    const int* ord = use_bin ? order.data() : nullptr;
    const double v[3] = {orient == 1 ? view[0] : 0.0, orient == 1 ? view[1] : 0.0, orient == 1 ? view[2] : 0.0};
    // exact-size buffers: AddressSanitizer sees any index outside them
    out.n.assign(3 * n, -7.0f); out.curv.assign(n, -7.0f); out.within.assign(n, -7);
    REPLAY(served, normal_one<K>(i, x.data(), ord, G.g, k, orient, v[0], v[1], v[2], ref, out.n.data(), out.curv.data(), out.within.data()));
    std::vector<float> n_only(3 * n, -7.0f);   // out_curvature and out_within NULL
    REPLAY(served, normal_one<K>(i, x.data(), ord, G.g, k, orient, v[0], v[1], v[2], ref, n_only.data(), nullptr, nullptr));
    out.served.clear();
    for (size_t j = 0; j < served; ++j) out.served.push_back(use_bin ? (size_t)order[j] : j);
    if (std::memcmp(n_only.data(), out.n.data(), 12 * n) != 0) out.within.assign(n, -8);   // shows as a difference below
}

static bool run(const char* name, const std::vector<float>& x, float radius, std::vector<int> ks, const double* view = nullptr, const float* ref = nullptr,
                size_t check_step = 1, Result* keep = nullptr, size_t limit = ~(size_t)0) {
    Grid G;
    if (!build(x, radius, G)) { printf("%s: no finite point\n", name); return true; }
    const size_t n = x.size() / 3;
    int variant = 0;
    bool all_ok = true;
    for (int k : ks)
        for (int orient = 0; orient < 3; ++orient, ++variant) {
            if ((orient == 1 && !view) || (orient == 2 && !ref)) continue;
            nblk_rev = variant & 1;
            const bool use_bin = (variant & 2) == 0;
            Result r;
            switch (knn_list_size(k)) {
                case 4: replay<4>(x, G, k, orient, view, ref, use_bin, r, limit); break;
                case 8: replay<8>(x, G, k, orient, view, ref, use_bin, r, limit); break;
                case 16: replay<16>(x, G, k, orient, view, ref, use_bin, r, limit); break;
                default: replay<32>(x, G, k, orient, view, ref, use_bin, r, limit); break;
            }
            bool ok = true;
            for (size_t j = 0; j < r.served.size() && ok; j += check_step) {
                const size_t i = r.served[j];
                float wn[3], wc;
                int32_t ww;
                plain(x, i, radius, k, orient, view, ref, wn, wc, ww);
                ok = std::memcmp(wn, &r.n[3 * i], 12) == 0 && cloud_bits(wc) == cloud_bits(r.curv[i]) && ww == r.within[i];
                if (!ok)
                    printf("%s, k = %d, orient %d, point %zu: %g %g %g / %g / %d against %g %g %g / %g / %d  DIFFERS\n", name, k, orient, i, r.n[3 * i], r.n[3 * i + 1],
                           r.n[3 * i + 2], r.curv[i], r.within[i], wn[0], wn[1], wn[2], wc, ww);
            }
            if (!ok) { ++failures; all_ok = false; }
            if (keep) *keep = r;
        }
    printf("%-36s points = %6zu  radius = %-8g %zu values of k%s%s\n", name, n, (double)radius, ks.size(), view ? ", viewpoint" : "", ref ? ", reference" : "");
    return all_ok;
}

static void expect(bool cond, const char* what) {
    if (!cond) { printf("%s: NOT as expected\n", what); ++failures; }
}

int main() {
    std::mt19937 rng(18);
    for (unsigned t = 0; t < 256; ++t) order256[t] = t;
    std::shuffle(order256, order256 + 256, rng);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    std::normal_distribution<float> N(0.0f, 1.0f);
    const std::vector<int> all_k = {2, 3, 4, 5, 8, 9, 16, 17, 31, 32};

    {   // a random cloud with duplicates, non-finite and far points, the three orientation modes; and scaled by 2^-40 and 2^40
        const size_t n = 2500;
        std::vector<float> x(3 * n), ref(3 * n);
        for (float& v : x) v = 10.0f + 3.0f * U(rng);
        for (float& v : ref) v = N(rng);
        for (size_t i = 0; i < 300; ++i) for (int a = 0; a < 3; ++a) x[3 * (1000 + i) + a] = x[3 * i + a];
        x[3 * 17] = NAN; x[3 * 18 + 1] = INFINITY; x[3 * 19 + 2] = -INFINITY; x[3 * (n - 1)] = NAN;
        for (int a = 0; a < 3; ++a) { x[3 * 20 + a] = 900.0f; x[3 * 23 + a] = -700.0f; }
        ref[3 * 40] = NAN; ref[3 * 41 + 2] = INFINITY;
        for (int a = 0; a < 3; ++a) ref[3 * 42 + a] = 0.0f;
        const double view[3] = {11.5, 11.25, 40.0};
        run("random cloud", x, 0.3f, all_k, view, ref.data());
        run("random cloud, fine", x, 0.05f, {2, 4, 5, 32}, view, ref.data());
        run("random cloud, one cell", x, 4000.0f, {2, 16, 32}, view, ref.data(), 50);
        for (int sh : {-40, 40}) {
            std::vector<float> y(x);
            for (float& v : y) v = std::ldexp(v, sh);
            const double vs[3] = {std::ldexp(view[0], sh), std::ldexp(view[1], sh), std::ldexp(view[2], sh)};
            run(sh < 0 ? "random cloud x 2^-40" : "random cloud x 2^40", y, std::ldexp(0.3f, sh), {3, 8, 16, 32}, vs, ref.data());
        }
    }
    {   // 0 .. 3 candidates, and exactly k - 1, k and k + 1: clusters of m + 1 points, far apart
        std::vector<float> x;
        for (int m : {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33})
            for (int j = 0; j <= m; ++j) { x.push_back(100.0f * (float)m + 0.01f * U(rng)); x.push_back(0.01f * U(rng)); x.push_back(0.01f * U(rng)); }
        run("clusters around k", x, 0.05f, {2, 3, 4, 8, 16, 32});
    }
    {   // all neighbours on the point; exactly collinear neighbours, along an axis and along a diagonal: undefined
        std::vector<float> x;
        for (int j = 0; j < 6; ++j) { x.push_back(1.0f); x.push_back(2.0f); x.push_back(3.0f); }
        for (int j = 0; j < 7; ++j) { x.push_back(50.0f + 0.25f * (float)j); x.push_back(7.0f); x.push_back(-2.0f); }
        for (int j = 0; j < 5; ++j) { x.push_back(90.0f + 0.25f * (float)j); x.push_back(0.25f * (float)j); x.push_back(3.0f); }
        Result r;
        run("duplicates and exact lines", x, 2.0f, {4}, nullptr, nullptr, 1, &r);
        bool undef = true;
        for (size_t i = 0; i < x.size() / 3; ++i)
            undef = undef && cloud_bits(r.n[3 * i]) == 0 && cloud_bits(r.n[3 * i + 1]) == 0 && cloud_bits(r.n[3 * i + 2]) == 0 && std::isinf(r.curv[i]) && r.within[i] >= 4;
        expect(undef, "duplicates and exact lines are undefined");
    }
    {   // an axis-aligned 3 x 3 lattice: the normal exactly (0, 0, 1), the curvature exactly 0; a viewpoint below flips, one in the
        // plane (dot exactly 0) and NaN reference normals keep the canonical sign
        std::vector<float> x, ref;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { x.push_back(4.0f + (float)a); x.push_back(4.0f + (float)b); x.push_back(4.0f); }
        for (int j = 0; j < 9; ++j) { ref.push_back(j == 3 ? NAN : 0.3f); ref.push_back(0.1f); ref.push_back(j == 2 ? 1.0f : -2.0f); }
        const double below[3] = {5.0, 5.0, -9.0}, in_plane[3] = {100.0, -3.0, 4.0};
        Result up, down, flat;
        run("3 x 3 lattice", x, 1.5f, {8}, nullptr, nullptr, 1, &up);
        run("3 x 3 lattice, viewpoint below", x, 1.5f, {8}, below, ref.data(), 1, &down);   // keeps the orient == 2 answer
        bool ok = true, ok_ref = true;
        for (int j = 0; j < 9; ++j) {
            ok = ok && cloud_bits(up.n[3 * j]) == 0 && cloud_bits(up.n[3 * j + 1]) == 0 && up.n[3 * j + 2] == 1.0f && cloud_bits(up.curv[j]) == 0;
            ok_ref = ok_ref && down.n[3 * j + 2] == ((j == 2 || j == 3) ? 1.0f : -1.0f);
        }
        expect(ok, "lattice normals are exactly (0, 0, 1) with curvature 0");
        expect(ok_ref, "reference normals flip, a NaN one keeps the canonical sign");
        Grid G;
        build(x, 1.5f, G);
        replay<8>(x, G, 8, 1, below, nullptr, true, down);
        replay<8>(x, G, 8, 1, in_plane, nullptr, true, flat);
        bool ok_view = true;
        for (int j = 0; j < 9; ++j) ok_view = ok_view && down.n[3 * j + 2] == -1.0f && flat.n[3 * j + 2] == 1.0f;
        expect(ok_view, "a viewpoint below flips, one in the plane keeps the canonical sign");
        run("3 x 3 lattice, viewpoint in plane", x, 1.5f, {8}, in_plane, nullptr);
    }
    {   // 70 001 points in one cell
        std::vector<float> y(3 * 70001);
        for (float& v : y) v = 5.0f + 0.01f * U(rng);
        run("70001 in one cell", y, 1.0f, {32}, nullptr, nullptr, 23, nullptr, 600);   // the first 600 threads, every 23rd of their points compared
    }
    {   // n = 1, n = 257
        std::vector<float> one = {1.0f, -2.0f, 3.0f};
        run("n = 1", one, 0.1f, {2, 32});
        std::vector<float> x(3 * 257);
        for (float& v : x) v = -3.0f + 0.1f * U(rng);
        const double view[3] = {0.0, 0.0, 0.0};
        run("n = 257", x, 1.0f / 64.0f, {2, 9, 16}, view);
    }
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
