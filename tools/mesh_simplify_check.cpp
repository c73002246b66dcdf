// mesh_simplify_check.cpp -- mpmvs_simplify_mesh replayed on the host through the headers' own __host__ __device__ code: the clustering
// passes as Clusters of csrc/pm_cluster_host.hpp chains them (cloud_insert_one, voxel_first_one, voxel_flag_one, voxel_number_one, voxel_accumulate_one,
// voxel_finish_one) and the new bodies of csrc/pm_simplify.hpp (simp_quadric_one, simp_place_one, simp_classify_one, simp_insert_one,
// simp_owner_one, simp_emit_one), with buffers of exactly the sizes pm_cluster_host.hpp and mpmvs_mesh.hip give them, against plain loops written out below
// (statement 4 of include/mpmvs.h: a std::map over the cells, sequential int64 sums, a Jacobi on arrays, a std::map over the keys).
// Every pass is replayed thread by thread in a scrambled order, the blocks ascending and descending.  The insert pass is also replayed
//   by steps    every alive triangle's probe is a state (simp_probe_begin); one step of one probe picked at random runs at a time
//               (simp_insert_step: one access to the table per step) until all are done, so that the probes of all threads interleave
//               between the read of a slot, its compare-and-swap, the comparison of the keys and the atomic min.
// After every insert replay the table is checked on its own: every slot's owner is the smallest index of its key, every key of an
// alive triangle owns exactly one slot, and at most half of the slots are taken.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_simplify_check tools/mesh_simplify_check.cpp && build/mesh_simplify_check
// Prints one line per case and "all equal"; exit status 1 on any difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "pm_simplify.hpp"
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
static std::mt19937 rng(29);

struct Mesh {
    std::vector<float> xyz;
    std::vector<unsigned char> rgb;   // empty: no colour
    std::vector<int32_t> tri;
    size_t n() const { return xyz.size() / 3; }
    size_t m() const { return tri.size() / 3; }
};
struct Result {
    long long nc = 0;
    std::vector<float> xyz;
    std::vector<unsigned char> rgb, placed;
    std::vector<int32_t> tri, cluster_of, count, src;
    long long counts[3] = {0, 0, 0};
};
template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static bool same_result(const Result& a, const Result& b) {
    return a.nc == b.nc && same(a.xyz, b.xyz) && same(a.rgb, b.rgb) && same(a.placed, b.placed) && same(a.tri, b.tri) && same(a.cluster_of, b.cluster_of) &&
           same(a.count, b.count) && same(a.src, b.src) && std::memcmp(a.counts, b.counts, sizeof a.counts) == 0;
}

static bool finite3(const Mesh& M, size_t v) { return std::isfinite(M.xyz[3 * v]) && std::isfinite(M.xyz[3 * v + 1]) && std::isfinite(M.xyz[3 * v + 2]); }

// ---- statement 4, plainly -------------------------------------------------------------------------------------------------------------
static void plain(const Mesh& M, float cell, int placement, Result& r) {
    const size_t n = M.n(), m = M.m();
    r = Result();
    r.cluster_of.assign(n, -1);
    float mn[3] = {0, 0, 0};
    bool any = false;
    for (size_t v = 0; v < n; ++v) {
        if (!finite3(M, v)) continue;
        for (int a = 0; a < 3; ++a) mn[a] = any ? std::min(mn[a], M.xyz[3 * v + a]) : M.xyz[3 * v + a];
        any = true;
    }
    r.counts[0] = (long long)m;
    if (!any) return;
    const double e = (double)cell;
    double o[3];
    for (int a = 0; a < 3; ++a) o[a] = (double)mn[a] - 0.5 * e;
    // A: the cells in the order of their first member
    std::map<std::array<long long, 3>, int> cells;
    std::vector<std::array<double, 3>> cell_of_cluster;
    std::vector<std::array<long long, 3>> S, Csum;
    std::vector<std::array<double, 3>> frac(n);
    for (size_t v = 0; v < n; ++v) {
        if (!finite3(M, v)) continue;
        std::array<long long, 3> key;
        std::array<double, 3> c;
        std::array<long long, 3> term;
        for (int a = 0; a < 3; ++a) {
            const double t = ((double)M.xyz[3 * v + a] - o[a]) / e;
            c[a] = std::floor(t);
            key[a] = (long long)c[a];
            frac[v][a] = t - c[a];
            term[a] = llrint(frac[v][a] * 0x1p30);
        }
        auto it = cells.find(key);
        if (it == cells.end()) {
            it = cells.emplace(key, (int)cell_of_cluster.size()).first;
            cell_of_cluster.push_back(c);
            S.push_back({0, 0, 0});
            Csum.push_back({0, 0, 0});
            r.count.push_back(0);
        }
        const int k = it->second;
        r.cluster_of[v] = k;
        ++r.count[k];
        for (int a = 0; a < 3; ++a) {
            S[k][a] += term[a];
            if (!M.rgb.empty()) Csum[k][a] += M.rgb[3 * v + a];
        }
    }
    const size_t nc = cell_of_cluster.size();
    r.nc = (long long)nc;
    r.xyz.resize(3 * nc);
    r.placed.assign(nc, 0);
    if (!M.rgb.empty()) r.rgb.resize(3 * nc);
    for (size_t k = 0; k < nc; ++k)
        for (int a = 0; a < 3; ++a) {
            const double den = (double)r.count[k] * 0x1p30;
            r.xyz[3 * k + a] = (float)(o[a] + (cell_of_cluster[k][a] + (double)S[k][a] / den) * e);
            if (!M.rgb.empty()) r.rgb[3 * k + a] = (unsigned char)((2 * Csum[k][a] + r.count[k]) / (2 * (long long)r.count[k]));
        }
    // B: the quadrics
    if (placement == 1 && m > 0) {
        std::vector<std::array<long long, 10>> Q(nc);
        for (auto& q : Q) q.fill(0);
        for (size_t t = 0; t < m; ++t) {
            const size_t v[3] = {(size_t)M.tri[3 * t], (size_t)M.tri[3 * t + 1], (size_t)M.tri[3 * t + 2]};
            if (!finite3(M, v[0]) || !finite3(M, v[1]) || !finite3(M, v[2])) continue;
            double P[3][3];
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) P[c][a] = (double)M.xyz[3 * v[c] + a];
            double u[3], w[3];
            for (int a = 0; a < 3; ++a) u[a] = P[1][a] - P[0][a], w[a] = P[2][a] - P[0][a];
            const double C[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double L = std::sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2]);
            if (!(L > 0.0) || !std::isfinite(L)) continue;
            const double nh[3] = {C[0] / L, C[1] / L, C[2] / L};
            for (int c = 0; c < 3; ++c) {
                double q[3];
                for (int a = 0; a < 3; ++a) q[a] = frac[v[c]][a] - 0.5;
                const double delta = (nh[0] * q[0] + nh[1] * q[1]) + nh[2] * q[2];
                auto& s = Q[(size_t)r.cluster_of[v[c]]];
                int at = 0;
                for (int i = 0; i < 3; ++i)
                    for (int j = i; j < 3; ++j) s[at++] += llrint((nh[i] * nh[j]) * 0x1p30);
                for (int i = 0; i < 3; ++i) s[6 + i] += llrint((nh[i] * delta) * 0x1p30);
                s[9] += 1;
            }
        }
        for (size_t k = 0; k < nc; ++k) {
            if (Q[k][9] == 0) continue;
            double A[3][3], a[3][3], V[3][3], rr[3], x0[3];
            const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) A[i][j] = a[i][j] = (double)Q[k][at[i][j]] / 0x1p30, V[i][j] = i == j ? 1.0 : 0.0;
                rr[i] = (double)Q[k][6 + i] / 0x1p30;
                x0[i] = (double)S[k][i] / ((double)r.count[k] * 0x1p30) - 0.5;
            }
            const int pairs[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
            for (int sweep = 0; sweep < 8; ++sweep)
                for (const auto& pq : pairs) {
                    const int p = pq[0], q = pq[1], o3 = pq[2];
                    const double apq = a[p][q];
                    if (apq == 0.0) continue;
                    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / std::sqrt(tt * tt + 1.0), sn = tt * cs;
                    a[p][p] = a[p][p] - tt * apq;
                    a[q][q] = a[q][q] + tt * apq;
                    a[p][q] = a[q][p] = 0.0;
                    const double arp = a[o3][p], arq = a[o3][q];
                    a[o3][p] = a[p][o3] = cs * arp - sn * arq;
                    a[o3][q] = a[q][o3] = sn * arp + cs * arq;
                    for (int i = 0; i < 3; ++i) {
                        const double vp = V[i][p], vq = V[i][q];
                        V[i][p] = cs * vp - sn * vq;
                        V[i][q] = sn * vp + cs * vq;
                    }
                }
            double lmax = a[0][0];
            for (int j = 1; j < 3; ++j)
                if (a[j][j] > lmax) lmax = a[j][j];
            if (!(lmax > 0.0)) {
                r.placed[k] = 2;
                continue;
            }
            double g[3], y[3], x[3];
            for (int i = 0; i < 3; ++i) g[i] = rr[i] - ((A[i][0] * x0[0] + A[i][1] * x0[1]) + A[i][2] * x0[2]);
            for (int j = 0; j < 3; ++j) y[j] = a[j][j] > 1e-3 * lmax ? ((V[0][j] * g[0] + V[1][j] * g[1]) + V[2][j] * g[2]) / a[j][j] : 0.0;
            bool inside = true;
            for (int i = 0; i < 3; ++i) {
                x[i] = x0[i] + ((V[i][0] * y[0] + V[i][1] * y[1]) + V[i][2] * y[2]);
                inside = inside && std::fabs(x[i]) <= 0.5;
            }
            r.placed[k] = inside ? 1 : 2;
            if (inside)
                for (int i = 0; i < 3; ++i) r.xyz[3 * k + i] = (float)(o[i] + (cell_of_cluster[k][i] + (0.5 + x[i])) * e);
        }
    }
    // C: the triangles
    std::map<std::array<int32_t, 3>, size_t> seen;
    r.counts[0] = 0;
    for (size_t t = 0; t < m; ++t) {
        const std::array<int32_t, 3> cl = {r.cluster_of[M.tri[3 * t]], r.cluster_of[M.tri[3 * t + 1]], r.cluster_of[M.tri[3 * t + 2]]};
        if (cl[0] < 0 || cl[1] < 0 || cl[2] < 0) { ++r.counts[0]; continue; }
        if (cl[0] == cl[1] || cl[1] == cl[2] || cl[0] == cl[2]) { ++r.counts[1]; continue; }
        std::array<int32_t, 3> key = cl;
        std::sort(key.begin(), key.end());
        if (!seen.emplace(key, t).second) { ++r.counts[2]; continue; }
        r.tri.insert(r.tri.end(), cl.begin(), cl.end());
        r.src.push_back((int32_t)t);
    }
}

// ---- the replay ---------------------------------------------------------------------------------------------------------------------
// an exclusive scan as k_scan_tiles / k_scan_totals<Sum> leave it: in-tile offsets and the scanned tile totals; returns the grand total
static int tile_scan(const std::vector<int>& flag, std::vector<int>& excl, std::vector<int>& tiles) {
    const size_t n = flag.size();
    excl.assign(n, -7);
    tiles.assign((n + kScanBlock - 1) / kScanBlock, 0);
    int grand = 0;
    for (size_t b = 0; b < tiles.size(); ++b) {
        int run = 0;
        for (size_t k = b * kScanBlock; k < std::min(n, (b + 1) * kScanBlock); ++k) excl[k] = run, run += flag[k];
        tiles[b] = grand;
        grand += run;
    }
    return grand;
}

// the table after an insert pass, judged on its own
static bool table_right(const std::vector<uint32_t>& table, const std::vector<unsigned char>& cls, const std::vector<int32_t>& key, size_t alive) {
    std::map<std::array<int32_t, 3>, uint32_t> least;
    for (size_t t = 0; t < cls.size(); ++t)
        if (cls[t] == kSimpAlive) least.emplace(std::array<int32_t, 3>{key[3 * t], key[3 * t + 1], key[3 * t + 2]}, (uint32_t)t);   // ascending t: the first stays
    size_t taken = 0;
    for (uint32_t o : table) {
        if (o == kSimpEmpty) continue;
        ++taken;
        if (o >= cls.size() || cls[o] != kSimpAlive) return false;
        auto it = least.find({key[3 * o], key[3 * o + 1], key[3 * o + 2]});
        if (it == least.end() || it->second != o) return false;
        least.erase(it);   // a second slot of the same key would not find it
    }
    return least.empty() && 2 * taken <= table.size() && taken <= alive;
}

enum InsertMode { kByThreads, kBySteps };
static bool replay(const Mesh& M, float cell, int placement, InsertMode mode, Result& r) {
    const size_t n = M.n(), m = M.m();
    r = Result();
    r.cluster_of.assign(n, -1);
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    const long long n_fin = cloud_bbox((long long)n, M.xyz.data(), mn, mx);
    r.counts[0] = (long long)m;
    if (n_fin == 0) return true;
    VoxelGrid g;
    voxel_origin(mn, cell, g);
    double top;
    if (voxel_span_axis(mx, g, &top) >= 0) { printf("the case spans too many cells\n"); exit(3); }
    const size_t slots = (size_t)1 << cloud_slots_log2(n_fin);
    const unsigned char* rgb = M.rgb.empty() ? nullptr : M.rgb.data();
    std::vector<int> slot_of(n, -7), flag(n, -7), num, vtiles, cnt(slots, 0), vox_of_slot(slots, -7);
    std::vector<unsigned long long> keys(slots, kCloudEmpty);
    std::vector<unsigned> first(slots, 0xffffffffu);
    REPLAY(n, cloud_insert_one(i, M.xyz.data(), g.o[0], g.o[1], g.o[2], g.e, (unsigned)(slots - 1), keys.data(), cnt.data(), slot_of.data()));
    REPLAY(n, voxel_first_one(i, slot_of.data(), first.data()));
    REPLAY(n, voxel_flag_one(i, slot_of.data(), first.data(), flag.data()));
    const int nci = tile_scan(flag, num, vtiles);
    for (size_t k = 0; k < n; ++k) num[k] += vtiles[k / kScanBlock];   // k_vs_scan_add
    const size_t nc = (size_t)nci;
    r.nc = nci;
    std::vector<int32_t> out_first(nc, -7);
    r.count.assign(nc, -7);
    std::vector<unsigned long long> acc((rgb ? 2 : 1) * nc * 3, 0), qrt(placement == 1 ? nc * kSimpSums : 0, 0);
    unsigned long long* S = acc.data();
    unsigned long long* C = rgb ? S + 3 * nc : nullptr;
    r.xyz.assign(3 * nc, -7.0f);
    if (rgb) r.rgb.assign(3 * nc, 7);
    r.placed.assign(nc, 0);
    REPLAY(n, voxel_number_one(i, flag.data(), num.data(), slot_of.data(), cnt.data(), vox_of_slot.data(), out_first.data(), r.count.data()));
    REPLAY(n, voxel_accumulate_one(i, M.xyz.data(), nullptr, rgb, g, slot_of.data(), vox_of_slot.data(), S, nullptr, C, r.cluster_of.data()));
    if (placement == 1 && m > 0) REPLAY(m, simp_quadric_one(i, M.xyz.data(), M.tri.data(), g, r.cluster_of.data(), qrt.data()));
    REPLAY(nc, voxel_finish_one(i, M.xyz.data(), out_first.data(), r.count.data(), g, S, nullptr, C, r.xyz.data(), nullptr, rgb ? r.rgb.data() : nullptr));
    if (placement == 1 && m > 0) REPLAY(nc, simp_place_one(i, M.xyz.data(), out_first.data(), r.count.data(), g, S, qrt.data(), r.xyz.data(), r.placed.data()));
    if (m == 0) { r.counts[0] = 0; return true; }
    std::vector<unsigned char> cls(m, 7);
    std::vector<int32_t> key(3 * m, -7);
    long long cc[3] = {0, 0, 0};
    REPLAY(m, ++cc[simp_classify_one(i, M.tri.data(), r.cluster_of.data(), cls.data(), key.data())]);
    r.counts[0] = cc[kSimpNonFinite], r.counts[1] = cc[kSimpCollapsed];
    if (cc[kSimpAlive] == 0) return true;
    const size_t tslots = (size_t)1 << simp_slots_log2(cc[kSimpAlive]);
    const uint32_t mask = (uint32_t)(tslots - 1);
    std::vector<uint32_t> table(tslots, kSimpEmpty);
    if (mode == kByThreads) {
        REPLAY(m, simp_insert_one(i, cls.data(), key.data(), mask, table.data()));
    } else {
        std::vector<size_t> who;
        std::vector<SimpProbe> probe;
        for (size_t t = 0; t < m; ++t)
            if (cls[t] == kSimpAlive) who.push_back(t), probe.push_back(simp_probe_begin(t, key.data(), mask));
        std::vector<unsigned long long> steps(who.size(), 0);
        while (!who.empty()) {
            const size_t j = std::uniform_int_distribution<size_t>(0, who.size() - 1)(rng);
            if (++steps[j] > 2ull * mask + 2ull) { printf("a probe does not end\n"); return false; }
            if (simp_insert_step(who[j], probe[j], key.data(), mask, table.data())) {
                who[j] = who.back(), probe[j] = probe.back(), steps[j] = steps.back();
                who.pop_back(), probe.pop_back(), steps.pop_back();
            }
        }
    }
    if (!table_right(table, cls, key, (size_t)cc[kSimpAlive])) { printf("the table is wrong\n"); return false; }
    std::vector<int> kept(m, 0), excl, ttiles;
    REPLAY(tslots, simp_owner_one(i, table.data(), kept.data()));
    const int nt = tile_scan(kept, excl, ttiles);
    r.tri.assign(3 * (size_t)nt, -7);
    r.src.assign((size_t)nt, -7);
    REPLAY(m, simp_emit_one(i, M.tri.data(), r.cluster_of.data(), kept.data(), excl.data(), ttiles.data(), r.tri.data(), r.src.data()));
    r.counts[2] = cc[kSimpAlive] - nt;
    return true;
}

static void run_case(const std::string& name, const Mesh& M, float cell) {
    bool ok = true;
    Result want[2], got;
    for (int placement = 0; placement < 2; ++placement) plain(M, cell, placement, want[placement]);
    for (int round = 0; round < 3; ++round) {
        std::shuffle(order256, order256 + 256, rng);
        nblk_rev = round & 1;
        for (int placement = 0; placement < 2; ++placement)
            for (InsertMode mode : {kByThreads, kBySteps}) ok = replay(M, cell, placement, mode, got) && same_result(got, want[placement]) && ok;
    }
    long long placed[3] = {0, 0, 0};
    for (unsigned char p : want[1].placed) ++placed[p];
    printf("%-28s n %6zu m %6zu cell %-8g clusters %6lld kept %6zu counts %lld %lld %lld placed %lld %lld %lld: %s\n", name.c_str(), M.n(), M.m(), (double)cell, want[1].nc,
           want[1].src.size(), want[1].counts[0], want[1].counts[1], want[1].counts[2], placed[0], placed[1], placed[2], ok ? "equal" : "DIFFERENT");
    if (!ok) ++failures;
}

// ---- cases --------------------------------------------------------------------------------------------------------------------------
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static int pick(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }

// a random index mesh: the vertices a walk through a box, every triangle inside a window of indices
static Mesh random_mesh(int n, int m, double box, double step, bool flat, bool nans, bool color) {
    Mesh M;
    double p[3] = {uni(-box, box), uni(-box, box), uni(-box, box)};
    const int flat_axis = pick(0, 2);
    for (int v = 0; v < n; ++v) {
        for (int a = 0; a < 3; ++a) {
            p[a] += std::normal_distribution<double>(0.0, step)(rng);
            M.xyz.push_back((float)((flat && a == flat_axis) ? 0.25 * box : p[a]));
        }
        if (nans && pick(0, 9) == 0) M.xyz[3 * v + pick(0, 2)] = pick(0, 1) ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity();
        if (color)
            for (int a = 0; a < 3; ++a) M.rgb.push_back((unsigned char)pick(0, 255));
    }
    const int width = std::max(1, std::min(n, pick(3, std::max(4, n / 2))));
    for (int t = 0; t < m; ++t) {
        const int start = pick(0, n - width);
        for (int k = 0; k < 3; ++k) M.tri.push_back(start + pick(0, width - 1));
    }
    return M;
}
// a box of side 1 as six faces of q x q quads with vertices of their own
static Mesh cube(int q) {
    Mesh M;
    for (int axis = 0; axis < 3; ++axis)
        for (int side = 0; side < 2; ++side) {
            const int base = (int)M.n();
            for (int j = 0; j <= q; ++j)
                for (int i = 0; i <= q; ++i) {
                    float p[3];
                    p[axis] = (float)side, p[(axis + 1) % 3] = (float)i / (float)q, p[(axis + 2) % 3] = (float)j / (float)q;
                    M.xyz.insert(M.xyz.end(), p, p + 3);
                }
            for (int j = 0; j < q; ++j)
                for (int i = 0; i < q; ++i) {
                    const int v = base + j * (q + 1) + i;
                    const int quad[2][3] = {{v, v + 1, v + q + 2}, {v, v + q + 2, v + q + 1}};
                    for (const auto& t : quad) M.tri.insert(M.tri.end(), {t[0], side ? t[1] : t[2], side ? t[2] : t[1]});
                }
        }
    return M;
}
// k triangles over three bundles of vertices, each bundle inside one cell of edge 1 (the last vertex, which no triangle names, puts the
// cell centres on the integers): one key, every insert on one slot
static Mesh one_key(int k, bool reverse) {
    Mesh M;
    const double centre[3][3] = {{0, 0, 0}, {5, 0, 0}, {0, 5, 1}};
    for (const auto& c : centre)
        for (int v = 0; v < 20; ++v)
            for (int a = 0; a < 3; ++a) M.xyz.push_back((float)(c[a] + uni(-0.3, 0.3)));
    M.xyz.insert(M.xyz.end(), {-1.0f, -1.0f, -1.0f});
    const int perms[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
    for (int t = 0; t < k; ++t)
        for (int c = 0; c < 3; ++c) M.tri.push_back(perms[t % 6][c] * 20 + pick(0, 19));
    if (reverse)
        for (int t = 0; t < k / 2; ++t)
            for (int c = 0; c < 3; ++c) std::swap(M.tri[3 * t + c], M.tri[3 * (k - 1 - t) + c]);
    return M;
}
// k triangles about one hub
static Mesh fan(int k) {
    Mesh M;
    M.xyz = {0.0f, 0.0f, 0.3f};
    for (int v = 0; v <= k; ++v) {
        const double ang = v * (2.0 * 3.14159265358979 / (k + 1));
        M.xyz.insert(M.xyz.end(), {(float)std::cos(ang), (float)std::sin(ang), (float)(0.05 * std::sin(7 * ang))});
    }
    for (int t = 0; t < k; ++t) M.tri.insert(M.tri.end(), {0, 1 + t, 2 + t});
    return M;
}
// random triples over a few vertices a cell apart: many duplicates, runs of taken slots
static Mesh few_keys(int k, int clusters) {
    Mesh M;
    for (int v = 0; v < clusters; ++v) M.xyz.insert(M.xyz.end(), {2.0f * (float)(v % 8), 2.0f * (float)(v / 8), 0.5f * (float)(v % 3)});
    for (int t = 0; t < 3 * k; ++t) M.tri.push_back(pick(0, clusters - 1));
    return M;
}

int main() {
    std::iota(order256, order256 + 256, 0u);
    run_case("empty", Mesh(), 1.0f);
    {
        Mesh M;
        M.xyz = {1, 2, 3};
        run_case("one vertex", M, 1.0f);
        M.xyz = {std::numeric_limits<float>::quiet_NaN(), 0, 0, 1, std::numeric_limits<float>::infinity(), 2};
        M.tri = {0, 1, 1};
        run_case("no finite vertex", M, 1.0f);
    }
    for (float cell : {0.25f, 0.1f, 0.07f}) run_case("cube 16", cube(16), cell);
    run_case("cube 16, one cell", cube(16), 8.0f);
    run_case("cube 16, nothing merges", cube(16), 0x1p-12f);
    run_case("one key 3001", one_key(3001, false), 1.0f);
    run_case("one key 3001 reversed", one_key(3001, true), 1.0f);
    run_case("fan 3001", fan(3001), 0.5f);
    run_case("fan 3001, coarse", fan(3001), 0.05f);
    run_case("few keys 4096 / 64", few_keys(4096, 64), 1.0f);
    run_case("few keys 600 / 9", few_keys(600, 9), 1.0f);
    for (int k = 0; k < 24; ++k) {
        const int n = k % 6 ? pick(1, 1500) : pick(1, 30);
        const double box = (const double[]){1e-2, 1.0, 50.0}[pick(0, 2)];
        const Mesh M = random_mesh(n, pick(0, 4 * n), box, box * (const double[]){0.01, 0.05, 0.3}[pick(0, 2)], k % 4 == 1, k % 5 == 3, k % 2 == 0);
        run_case("random " + std::to_string(k), M, (float)(box * (const double[]){0.05, 0.1, 0.2, 0.5}[pick(0, 3)]));
    }
    if (failures) {
        printf("%d cases DIFFERENT\n", failures);
        return 1;
    }
    printf("all equal\n");
    return 0;
}
