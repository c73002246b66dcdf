// knn_check.cpp -- the k-nearest-neighbour search of csrc/pm_knn.hpp replayed on the host, thread by thread in a scrambled order,
// through the header's own __host__ __device__ code (the grid build and the query binning of pm_cloud.hpp, then knn_list_one and
// knn_reduce_one per thread for every list size K), with buffers of exactly the sizes mpmvs_cloud_knn and mpmvs_cloud_outliers of
// mpmvs_cloud.hip give them, against a plain sort of all candidates written out below.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/knn_check tools/knn_check.cpp && build/knn_check
// Prints one line per case and "all equal"; exit status 1 if an output differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_knn.hpp"
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

// ---- the list alone ------------------------------------------------------------------------------------------------------
template <int K>
static void list_case(const char* name, std::vector<unsigned long long> keys) {
    KnnList<K> l;
    knn_clear(l);
    for (unsigned long long v : keys) knn_push(l, v);
    std::sort(keys.begin(), keys.end());
    bool ok = true;
    for (int j = 0; j < K; ++j) ok = ok && l.key[j] == ((size_t)j < keys.size() ? keys[j] : ~0ull);
    if (!ok) { printf("list K = %d, %s: DIFFERS\n", K, name); ++failures; }
}
template <int K>
static void list_cases(std::mt19937& rng) {
    for (int count : {0, 1, K - 1, K, K + 1, 3 * K + 5, 1000}) {
        std::vector<unsigned long long> asc;
        for (int j = 0; j < count; ++j) asc.push_back(((unsigned long long)(0x3f000000u + 7u * (unsigned)(j / 3)) << 32) | (unsigned)j);   // runs of equal d2
        std::vector<unsigned long long> desc(asc.rbegin(), asc.rend()), mix(asc);
        std::shuffle(mix.begin(), mix.end(), rng);
        list_case<K>("ascending", asc);
        list_case<K>("descending", desc);
        list_case<K>("scrambled", mix);
    }
    printf("list K = %2d: candidates fed in ascending, descending and scrambled order, below, at and above K\n", K);
}

// ---- the search ------------------------------------------------------------------------------------------------------------
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

// the serving order of the nq queries at q: k_cloud_qbin, the scan, k_cloud_qorder
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

// brute force: every candidate of query i, sorted
static void plain(const std::vector<float>& t, const float* q, size_t i, float radius, long long self, std::vector<unsigned long long>& keys) {
    keys.clear();
    if (!finite3(q + 3 * i)) return;
    const float r2 = radius * radius;
    for (size_t p = 0; p < t.size() / 3; ++p) {
        if ((long long)p == self || !finite3(&t[3 * p])) continue;
        const float dx = q[3 * i] - t[3 * p], dy = q[3 * i + 1] - t[3 * p + 1], dz = q[3 * i + 2] - t[3 * p + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= r2) keys.push_back(((unsigned long long)cloud_bits(d2) << 32) | (unsigned)p);
    }
    std::sort(keys.begin(), keys.end());
}

// one chunk of mpmvs_cloud_knn (queries i0 .. i0 + cn of q, or of the targets when q is null) and the pass of mpmvs_cloud_outliers
template <int K>
static bool chunk_case(const std::vector<float>& t, const std::vector<float>* q, size_t i0, size_t cn, float radius, int k, const Grid& G, bool use_bin, size_t check_step) {
    const float* qc = (q ? q->data() : t.data()) + 3 * i0;
    const long long self_base = q ? -1ll : (long long)i0;
    std::vector<int> order;
    if (use_bin) bin(qc, cn, G.g, order);
    const int* ord = use_bin ? order.data() : nullptr;
    // exact-size buffers: AddressSanitizer sees any index outside them
    std::vector<float> d2(cn * (size_t)k, -1.0f), mean(cn, -1.0f);
    std::vector<int32_t> idx(cn * (size_t)k, -7), within(cn, -7), within2(cn, -7);
    REPLAY(cn, knn_list_one<K>(i, qc, ord, G.g, self_base, k, d2.data(), idx.data(), within.data()));
    REPLAY(cn, knn_reduce_one<K>(i, qc, ord, G.g, self_base, k, mean.data(), within2.data()));
    std::vector<float> d2_only(cn * (size_t)k, -1.0f);
    REPLAY(cn, knn_list_one<K>(i, qc, ord, G.g, self_base, k, d2_only.data(), nullptr, nullptr));
    bool ok = std::memcmp(d2.data(), d2_only.data(), d2.size() * 4) == 0 && within == within2;
    std::vector<unsigned long long> keys;
    for (size_t i = 0; i < cn && ok; i += check_step) {
        plain(t, qc, i, radius, q ? -1ll : (long long)(i0 + i), keys);
        ok = ok && within[i] == (int32_t)keys.size();
        for (int e = 0; e < k && ok; ++e) {
            const bool found = (size_t)e < keys.size();
            const float want_d2 = found ? cloud_float((uint32_t)(keys[e] >> 32)) : INFINITY;
            ok = ok && cloud_bits(d2[i * k + e]) == cloud_bits(want_d2) && idx[i * k + e] == (found ? (int32_t)(keys[e] & 0xffffffffu) : -1);
        }
        float want_mean = INFINITY;
        if (keys.size() >= (size_t)k) {
            double s = std::sqrt((double)cloud_float((uint32_t)(keys[0] >> 32)));
            for (int e = 1; e < k; ++e) s = s + std::sqrt((double)cloud_float((uint32_t)(keys[e] >> 32)));
            want_mean = (float)(s / (double)k);
        }
        ok = ok && cloud_bits(mean[i]) == cloud_bits(want_mean);
    }
    return ok;
}

static void run(const char* name, const std::vector<float>& t, const std::vector<float>* q, float radius, std::vector<int> ks, size_t check_step = 1, size_t chunk = 1000,
                size_t limit = ~(size_t)0) {
    Grid G;
    if (!build(t, radius, G)) { printf("%s: no finite target\n", name); return; }
    const size_t nq = std::min(limit, q ? q->size() / 3 : t.size() / 3);   // `limit`: only the first queries are served
    int variant = 0;
    for (int k : ks) {
        for (size_t i0 = 0; i0 < nq; i0 += chunk, ++variant) {
            const size_t cn = std::min(chunk, nq - i0);
            nblk_rev = variant & 1;
            const bool use_bin = (variant & 2) == 0;
            bool ok = true;
            switch (knn_list_size(k)) {
                case 4: ok = chunk_case<4>(t, q, i0, cn, radius, k, G, use_bin, check_step); break;
                case 8: ok = chunk_case<8>(t, q, i0, cn, radius, k, G, use_bin, check_step); break;
                case 16: ok = chunk_case<16>(t, q, i0, cn, radius, k, G, use_bin, check_step); break;
                default: ok = chunk_case<32>(t, q, i0, cn, radius, k, G, use_bin, check_step); break;
            }
            if (!ok) { printf("%s, k = %d, chunk at %zu: DIFFERS\n", name, k, i0); ++failures; }
        }
    }
    printf("%-34s targets = %6zu  queries = %6zu (%s)  radius = %g  %zu values of k\n", name, t.size() / 3, nq, q ? "given" : "self", (double)radius, ks.size());
}

int main() {
    std::mt19937 rng(17);
    for (unsigned t = 0; t < 256; ++t) order256[t] = t;
    std::shuffle(order256, order256 + 256, rng);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const std::vector<int> all_k = {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32};

    list_cases<4>(rng); list_cases<8>(rng); list_cases<16>(rng); list_cases<32>(rng);

    {   // a random cloud with duplicates, non-finite and far points: self queries and given ones, three radii
        const size_t n = 2500;
        std::vector<float> x(3 * n), q(3 * 700);
        for (float& v : x) v = 10.0f + 3.0f * U(rng);
        for (float& v : q) v = 10.0f + 3.0f * U(rng);
        for (size_t i = 0; i < 300; ++i) for (int a = 0; a < 3; ++a) x[3 * (1000 + i) + a] = x[3 * i + a];   // duplicates of the query in self mode
        x[3 * 17] = NAN; x[3 * 18 + 1] = INFINITY; x[3 * 19 + 2] = -INFINITY; x[3 * (n - 1)] = NAN;
        for (int a = 0; a < 3; ++a) { x[3 * 20 + a] = 900.0f; x[3 * 23 + a] = -700.0f; }
        q[3 * 5] = NAN; q[3 * 6 + 1] = INFINITY;
        for (int a = 0; a < 3; ++a) q[3 * 7 + a] = x[3 * 40 + a];   // a given query on a target: that target is a candidate at d2 = 0
        run("random cloud", x, nullptr, 0.3f, all_k);
        run("random cloud", x, &q, 0.3f, all_k);
        run("random cloud, fine", x, nullptr, 0.05f, {1, 4, 5, 32});
        run("random cloud, one cell", x, nullptr, 4000.0f, {1, 16, 32}, 50);
        run("random cloud, one cell", x, &q, 4000.0f, {7, 32}, 10);
    }
    {   // exactly k - 1, k and k + 1 candidates: clusters of m + 1 points, far apart
        std::vector<float> x;
        for (int m : {0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33})
            for (int j = 0; j <= m; ++j) { x.push_back(100.0f * (float)m + 0.01f * U(rng)); x.push_back(0.01f * U(rng)); x.push_back(0.01f * U(rng)); }
        run("clusters around k", x, nullptr, 0.05f, {1, 4, 8, 16, 32});
    }
    {   // d2 == r2 and one ulp beyond: the boundary is inclusive
        const float r = 0.25f;
        std::vector<float> x = {0, 0, 0, r, 0, 0, std::nextafter(r, 1.0f), 0, 0, 0, -r, 0, 0, 0, std::nextafter(-r, -1.0f), 0, r, 0};
        run("boundary", x, nullptr, r, {1, 2, 4, 5});
    }
    {   // a 70 000-cell table: one point per cell; and 70 001 points in one cell
        const size_t n = 70000;
        const float radius = 0.01f;
        std::vector<float> x(3 * n), q(3 * 2000);
        std::vector<int> sites(42 * 42 * 42);
        for (size_t s = 0; s < sites.size(); ++s) sites[s] = (int)s;
        std::shuffle(sites.begin(), sites.end(), rng);
        for (size_t i = 0; i < n; ++i) {
            const int c[3] = {sites[i] % 42, (sites[i] / 42) % 42, sites[i] / (42 * 42)};
            for (int a = 0; a < 3; ++a) x[3 * i + a] = (float)(((double)c[a] * 3 + 0.5) * radius * (1 + 0x1p-10) + (0.2 * U(rng) - 0.1) * radius);
        }
        for (size_t i = 0; i < 2000; ++i) for (int a = 0; a < 3; ++a) q[3 * i + a] = x[3 * (rng() % n) + a] + 0.6f * radius * (2.0f * U(rng) - 1.0f);
        run("70000 cells", x, &q, radius, {1, 8});
        run("70000 cells, wide", x, &q, 0.05f, {32}, 20);
        std::vector<float> y(3 * 70001);
        for (float& v : y) v = 5.0f + 0.01f * U(rng);
        run("70001 in one cell", y, nullptr, 1.0f, {32}, 23, 256, 600);   // three chunks of the self queries, every 23rd one compared
    }
    {   // n = 1, n = 257
        std::vector<float> one = {1.0f, -2.0f, 3.0f};
        run("n = 1", one, nullptr, 0.1f, {1, 32});
        std::vector<float> x(3 * 257);
        for (float& v : x) v = -3.0f + 0.1f * U(rng);
        run("n = 257", x, nullptr, 1.0f / 64.0f, {1, 2, 9}, 1, 256);
    }
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
