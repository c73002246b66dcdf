// components_check.cpp -- the connected components of csrc/pm_components.hpp replayed on the host through the header's own
// __host__ __device__ code (the grid build and the binning of pm_cloud.hpp, then cc_init_one, cc_hook_one, cc_flatten_one,
// cc_count_one and cc_gather_one per thread), with buffers of exactly the sizes mpmvs_cloud_components of mpmvs_cloud.hip gives them,
// against a plain union-find over brute-force adjacency written out below.  The hook pass is replayed twice:
//   by threads  thread by thread in a scrambled order (the blocks ascending or descending, with and without the binning);
//   by edges    all unions (i, j) of all threads are collected, shuffled and applied one by one through cc_union, the two ends in
//               either order: a replay by whole threads cannot interleave the unions of two threads, this one does.
// The invariant parent[x] <= x (or -1 for a point that does not take part) is asserted over the whole array after every union of the
// replay by edges, and after every thread of the replay by threads.  Where that would take hours -- more than 20 000 edges, more
// than 5000 points -- it is asserted after every 4096 edges, after every block of 256 threads, and at the end.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/components_check tools/components_check.cpp && build/components_check
// Prints one line per case and "all equal"; exit status 1 on any difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "pm_components.hpp"
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
static std::mt19937 rng(17);

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

// the serving order of the points: k_cloud_qbin, the scan, k_cloud_qorder
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

// ---- the plain statement ----------------------------------------------------------------------------------------------------
static bool adjacent(const std::vector<float>& x, size_t i, size_t j, float r2) {
    const float dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

typedef std::vector<std::pair<int, int>> Edges;   // (i, j) with j < i

// every adjacent pair, by brute force
static void brute_edges(const std::vector<float>& x, float radius, Edges& edges) {
    const size_t n = x.size() / 3;
    const float r2 = radius * radius;
    edges.clear();
    for (size_t i = 0; i < n; ++i) {
        if (!finite3(&x[3 * i])) continue;
        for (size_t j = 0; j < i; ++j)
            if (finite3(&x[3 * j]) && adjacent(x, i, j, r2)) edges.push_back({(int)i, (int)j});
    }
}

struct Answer {
    std::vector<int32_t> label, size;
    long long counts[4];
    bool operator==(const Answer& o) const { return label == o.label && size == o.size && std::memcmp(counts, o.counts, sizeof counts) == 0; }
};

static void take_counts(Answer& a, long long n_fin) {
    long long comps = 0, best = 0, best_label = -1;
    for (size_t i = 0; i < a.label.size(); ++i) {
        if (a.label[i] != (int32_t)i) continue;
        ++comps;
        if (a.size[i] > best) best = a.size[i], best_label = (long long)i;
    }
    a.counts[0] = n_fin, a.counts[1] = comps, a.counts[2] = best, a.counts[3] = best_label;
}

// a plain union-find over the edges: the smaller root becomes the parent, so a root is the smallest index of its set
static void plain(const std::vector<float>& x, const Edges& edges, Answer& a) {
    const size_t n = x.size() / 3;
    std::vector<int> up(n);
    std::iota(up.begin(), up.end(), 0);
    auto root = [&](int v) {
        while (up[v] != v) v = up[v] = up[up[v]];
        return v;
    };
    for (const auto& e : edges) {
        const int a0 = root(e.first), b0 = root(e.second);
        if (a0 != b0) up[std::max(a0, b0)] = std::min(a0, b0);
    }
    a.label.assign(n, -1);
    a.size.assign(n, 0);
    long long n_fin = 0;
    for (size_t i = 0; i < n; ++i)
        if (finite3(&x[3 * i])) a.label[i] = root((int)i), ++n_fin;
    std::vector<int> members(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (a.label[i] >= 0) ++members[a.label[i]];
    for (size_t i = 0; i < n; ++i)
        if (a.label[i] >= 0) a.size[i] = members[a.label[i]];
    take_counts(a, n_fin);
}

// ---- the header's passes ------------------------------------------------------------------------------------------------------
static bool invariant(const std::vector<int>& parent) {
    for (size_t v = 0; v < parent.size(); ++v)
        if (parent[v] > (int)v || parent[v] < -1) return false;
    return true;
}

// flatten, count, gather and the counts, as mpmvs_cloud_components runs them after the hook pass: the parents' ints count the members
static void finish(std::vector<int>& parent, long long n_fin, Answer& a) {
    const size_t n = parent.size();
    a.label.assign(n, -7);
    a.size.assign(n, -7);
    REPLAY(n, cc_flatten_one(i, parent.data(), a.label.data()));
    std::fill(parent.begin(), parent.end(), 0);
    REPLAY(n, cc_count_one(i, a.label.data(), parent.data()));
    REPLAY(n, cc_gather_one(i, a.label.data(), parent.data(), a.size.data()));
    take_counts(a, n_fin);
}

static bool by_threads(const std::vector<float>& x, const Grid& G, bool use_bin, bool every_thread, Answer& a) {
    const size_t n = x.size() / 3;
    std::vector<int> parent(n, -7), order;   // exact size: AddressSanitizer sees any index outside it
    REPLAY(n, cc_init_one(i, x.data(), parent.data()));
    if (use_bin) bin(x.data(), n, G.g, order);
    bool ok = invariant(parent);
    if (every_thread) {   // the replay by edges checks after every single union
        REPLAY(n, (cc_hook_one(i, x.data(), use_bin ? order.data() : nullptr, G.g, parent.data()), ok = ok && invariant(parent)));
    } else {
        for (size_t b_ = 0; b_ < (n + 255) / 256; ++b_) {
            for (unsigned t_ = 0; t_ < 256; ++t_) {
                const size_t i = (nblk_rev ? (n + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_];
                if (i < n) cc_hook_one(i, x.data(), use_bin ? order.data() : nullptr, G.g, parent.data());
            }
            ok = ok && invariant(parent);
        }
    }
    finish(parent, G.n_fin, a);
    return ok;
}

static bool by_edges(const std::vector<float>& x, Edges edges, long long n_fin, bool every_union, Answer& a) {
    const size_t n = x.size() / 3;
    std::vector<int> parent(n, -7);
    REPLAY(n, cc_init_one(i, x.data(), parent.data()));
    std::shuffle(edges.begin(), edges.end(), rng);
    bool ok = true;
    size_t done = 0;
    for (const auto& e : edges) {
        const bool swap = rng() & 1;
        const int r = cc_union(parent.data(), swap ? e.second : e.first, swap ? e.first : e.second);
        ok = ok && parent[r] == r;   // what a union returns is a root when no other thread runs
        if (every_union || (++done & 4095) == 0) ok = ok && invariant(parent);
    }
    ok = ok && invariant(parent);
    finish(parent, n_fin, a);
    return ok;
}

// one cloud at one radius: `edges` (all adjacent pairs) from the caller, or by brute force when null
static void run(const char* name, const std::vector<float>& x, float radius, const Edges* given = nullptr, long long expect_components = -1) {
    const size_t n = x.size() / 3;
    Edges own;
    if (!given) brute_edges(x, radius, own);
    const Edges& edges = given ? *given : own;
    const bool every_thread = n <= 5000, every_union = every_thread && edges.size() <= 20000;
    Answer want;
    plain(x, edges, want);
    if (expect_components >= 0 && want.counts[1] != expect_components) { printf("%s: the statement finds %lld components, not %lld\n", name, want.counts[1], expect_components); ++failures; }
    Grid G;
    bool ok = build(x, radius, G);
    for (int variant = 0; variant < 4 && ok; ++variant) {
        nblk_rev = variant & 1;
        Answer got;
        if (!by_threads(x, G, (variant & 2) == 0, every_thread, got)) { printf("%s, by threads, variant %d: the invariant parent[x] <= x is broken\n", name, variant); ++failures; }
        if (!(got == want)) { printf("%s, by threads, variant %d: DIFFERS\n", name, variant); ++failures; }
    }
    for (int rep = 0; rep < 3 && ok; ++rep) {
        Answer got;
        if (!by_edges(x, edges, G.n_fin, every_union, got)) { printf("%s, by edges, shuffle %d: the invariant parent[x] <= x is broken\n", name, rep); ++failures; }
        if (!(got == want)) { printf("%s, by edges, shuffle %d: DIFFERS\n", name, rep); ++failures; }
    }
    if (!ok) { printf("%s: no finite point\n", name); ++failures; }
    printf("%-40s n = %6zu  radius = %-10.8g edges = %8zu  components = %6lld  largest = %6lld at label %lld\n", name, n, (double)radius, edges.size(),
           want.counts[1], want.counts[2], want.counts[3]);
}

static std::vector<float> permuted(const std::vector<float>& x, const std::vector<int>& perm) {
    std::vector<float> y(x.size());
    for (size_t i = 0; i < perm.size(); ++i)
        for (int a = 0; a < 3; ++a) y[3 * i + a] = x[3 * perm[i] + a];
    return y;
}

int main() {
    for (unsigned t = 0; t < 256; ++t) order256[t] = t;
    std::shuffle(order256, order256 + 256, rng);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);

    for (float shift : {0.0f, 1000.25f}) {   // a chain of 4096 points 257/1024 apart (exact in fp32, shifted too): the deepest trees
        const size_t n = 4096;
        std::vector<float> asc(3 * n, 0.0f);
        for (size_t k = 0; k < n; ++k) asc[3 * k] = shift + (float)k * (257.0f / 1024.0f);
        std::vector<int> rev(n), mix(n);
        std::iota(mix.begin(), mix.end(), 0);
        for (size_t k = 0; k < n; ++k) rev[k] = (int)(n - 1 - k);
        std::shuffle(mix.begin(), mix.end(), rng);
        const std::vector<float> desc = permuted(asc, rev), scr = permuted(asc, mix);
        for (float radius : {257.0f / 1024.0f, 0.25f}) {
            run(shift ? "chain + 1000.25, ascending" : "chain, ascending", asc, radius);
            run(shift ? "chain + 1000.25, descending" : "chain, descending", desc, radius);
            run(shift ? "chain + 1000.25, scrambled" : "chain, scrambled", scr, radius);
        }
    }
    for (int apart = 0; apart < 2; ++apart) {   // two blobs and one pair across them at exactly the radius, and one ulp beyond
        const float r = 0.25f, gap = apart ? std::nextafter(r, 1.0f) : r;
        std::vector<float> x;
        for (int b = 0; b < 2; ++b)
            for (int j = 0; j < 199; ++j) { x.push_back(b ? 3.2f + 0.3f * U(rng) : -3.0f - 0.3f * U(rng)); x.push_back(0.3f * U(rng)); x.push_back(0.3f * U(rng)); }
        x.insert(x.end(), {0.0f, 0.0f, 0.0f, gap, 0.0f, 0.0f});   // the pair: gap - 0 is exact; each end reaches its blob through the steps below
        for (int j = 1; j <= 13; ++j) { x.insert(x.end(), {-0.24f * (float)j, 0.0f, 0.0f}); x.insert(x.end(), {gap + 0.24f * (float)j, 0.0f, 0.0f}); }
        std::vector<int> mix(x.size() / 3);
        std::iota(mix.begin(), mix.end(), 0);
        std::shuffle(mix.begin(), mix.end(), rng);
        run(apart ? "bridge pair one ulp beyond the radius" : "bridge pair at exactly the radius", permuted(x, mix), r, nullptr, apart ? 2 : 1);
    }
    {   // a random cloud with duplicates and non-finite points, on both sides of percolation
        const size_t n = 3000;
        std::vector<float> x(3 * n);
        for (float& v : x) v = 100.0f + U(rng);
        for (size_t i = 0; i < 200; ++i) for (int a = 0; a < 3; ++a) x[3 * (2000 + i) + a] = x[3 * i + a];
        for (size_t i = 0; i < 150; ++i) x[3 * (rng() % n) + rng() % 3] = (i % 3 == 0) ? NAN : (i % 3 == 1 ? INFINITY : -INFINITY);
        x[0] = NAN; x[3 * (n - 1) + 2] = INFINITY;
        for (float radius : {0.04f, 0.055f, 0.065f, 0.09f}) run("random cloud with non-finite points", x, radius);
        run("random cloud, one cell", x, 4000.0f);
    }
    {   // n = 1, n = 257, two points, all but one non-finite
        run("n = 1", {1.0f, -2.0f, 3.0f}, 0.1f);
        run("two duplicates", {1.0f, -2.0f, 3.0f, 1.0f, -2.0f, 3.0f}, 1e-3f);
        run("one finite among non-finite", {NAN, 0.0f, 0.0f, 1.0f, 2.0f, 3.0f, 0.0f, INFINITY, 0.0f}, 0.1f);
        std::vector<float> x(3 * 257);
        for (float& v : x) v = -3.0f + 0.1f * U(rng);
        run("n = 257", x, 1.0f / 64.0f);
    }
    {   // a 70 000-cell table, one point per cell: sites of a 42^3 lattice three cells apart.  The adjacent pairs are those of lattice
        // neighbours (any other two sites are more than 5 fine radii apart): found here on the lattice, not by brute force.
        const size_t n = 70000;
        const float radius = 0.01f;
        const double pitch = 3.0 * radius * (1 + 0x1p-10);
        std::vector<float> x(3 * n);
        std::vector<int> sites(42 * 42 * 42), at(42 * 42 * 42, -1);
        std::iota(sites.begin(), sites.end(), 0);
        std::shuffle(sites.begin(), sites.end(), rng);
        for (size_t i = 0; i < n; ++i) {
            const int c[3] = {sites[i] % 42, (sites[i] / 42) % 42, sites[i] / (42 * 42)};
            at[sites[i]] = (int)i;
            for (int a = 0; a < 3; ++a) x[3 * i + a] = (float)(((double)c[a] + 0.5 / 3.0) * pitch + (0.2 * U(rng) - 0.1) * radius);
        }
        for (float r : {radius, (float)(1.1 * pitch)}) {   // no pair at all; then the axis neighbours (pitch -+ 0.2 radius) and no diagonal one (1.41 pitch)
            Edges edges;
            const float r2 = r * r;
            for (size_t i = 0; i < n; ++i) {
                const int c[3] = {sites[i] % 42, (sites[i] / 42) % 42, sites[i] / (42 * 42)};
                for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
                    const int d[3] = {c[0] + dx, c[1] + dy, c[2] + dz};
                    if (d[0] < 0 || d[0] > 41 || d[1] < 0 || d[1] > 41 || d[2] < 0 || d[2] > 41) continue;
                    const int j = at[d[0] + 42 * (d[1] + 42 * d[2])];
                    if (j >= 0 && j < (int)i && adjacent(x, i, (size_t)j, r2)) edges.push_back({(int)i, j});
                }
            }
            run(r == radius ? "70000 one-point cells" : "70000 points, lattice neighbours joined", x, r, &edges);
        }
    }
    {   // 70 001 exact duplicates in one cell: every pair is adjacent (2.4e9 of them, so no list of edges and no brute force); one
        // component, label 0, size 70 001.  By threads only, and every thread finds the one root after its first union.
        const size_t n = 70001;
        std::vector<float> x(3 * n);
        for (size_t i = 0; i < n; ++i) { x[3 * i] = 5.0f; x[3 * i + 1] = -6.5f; x[3 * i + 2] = 7.25f; }
        Grid G;
        Answer got;
        nblk_rev = true;
        bool ok = build(x, 0.5f, G) && by_threads(x, G, true, false, got);
        ok = ok && got.counts[0] == (long long)n && got.counts[1] == 1 && got.counts[2] == (long long)n && got.counts[3] == 0;
        for (size_t i = 0; i < n && ok; ++i) ok = got.label[i] == 0 && got.size[i] == (int32_t)n;
        if (!ok) { printf("70001 duplicates in one cell: DIFFERS\n"); ++failures; }
        printf("%-40s n = %6zu  radius = 0.5        one component, label 0, size %zu\n", "70001 duplicates in one cell", n, n);
    }
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
