// cloud_table_check.cpp -- the passes of csrc/pm_cloud.hpp replayed on the host, thread by thread in a scrambled order, through
// the header's own __host__ __device__ code (the key, packing, hashing and probing arithmetic and the per-thread body of every
// kernel; the scans and the stats are plain loops here), in the launch order of cloud_build / cloud_query of mpmvs_cloud.hip and with
// buffers of exactly their sizes, against the brute-force statement: random clouds with non-finite and far-away points, 70 000
// one-point cells, a full cell of duplicates, the cell-border lattice, and points on multiples of the radius with and without
// a jitter of 1e-5 radius at 40 random radii and offsets; each with binned queries, with caller order and without out_idx.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/cloud_table_check tools/cloud_table_check.cpp && build/cloud_table_check
// Prints one line per case and "all equal"; exit status 1 if any result differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_cloud.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = b_ * 256 + order256[t_];                                        \
            if (i < (size_t)(count)) call;                                                   \
        }

static void scan(const std::vector<int>& cnt, std::vector<int>& off) { off[0] = 0; for (size_t i = 0; i < cnt.size(); ++i) off[i + 1] = off[i] + cnt[i]; }

static void gpu_like(const std::vector<float>& t, const std::vector<float>& q, float radius, bool bin, bool want_idx, std::vector<float>& od2, std::vector<int32_t>& oidx, long long st[4]) {
    const int n = (int)(t.size() / 3), nq = (int)(q.size() / 3);
    float mn[3] = {0,0,0}; long long nf = 0;
    for (int i = 0; i < n; ++i) { const float* p = &t[3*i]; if (!(cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]))) continue; for (int a = 0; a < 3; ++a) mn[a] = nf ? std::min(mn[a], p[a]) : p[a]; ++nf; }
    od2.assign(nq, -1.0f); oidx.assign(nq, -7);
    if (!nf) { od2.assign(nq, INFINITY); oidx.assign(nq, -1); return; }
    const int lg = cloud_slots_log2(nf); const size_t slots = (size_t)1 << lg;
    // exact-size buffers: AddressSanitizer sees any index outside them
    std::vector<unsigned long long> keys(slots, kCloudEmpty); std::vector<int> cnt(slots, 0), off(slots + 1), slot_of(n); std::vector<uint4> pts(nf);
    const double edge = cloud_edge(radius);
    REPLAY(n, cloud_insert_one(i, t.data(), (double)mn[0], (double)mn[1], (double)mn[2], edge, (unsigned)(slots - 1), keys.data(), cnt.data(), slot_of.data()));
    st[0] = nf; st[1] = st[2] = 0; st[3] = (long long)slots;
    for (int c : cnt) { st[1] += c > 0; st[2] = std::max<long long>(st[2], c); }
    scan(cnt, off);
    REPLAY(n, cloud_scatter_one(i, t.data(), slot_of.data(), off.data(), cnt.data(), pts.data()));
    for (int c : cnt) if (c) { printf("count not back to 0\n"); exit(3); }
    CloudGrid g; for (int a = 0; a < 3; ++a) g.mn[a] = mn[a]; g.edge = edge; g.r2 = radius * radius; g.mask = (unsigned)(slots - 1); g.keys = keys.data(); g.off = off.data(); g.pts = pts.data();
    int bl = 8; while (bl < kCloudMaxSlotsLog2 && (1ll << bl) < nq) ++bl;
    const size_t bins = (size_t)1 << bl;
    std::vector<int> qcnt(bins, 0), qoff(bins + 1), qbin(nq), order(nq, -1);
    if (bin) {
        REPLAY(nq, cloud_qbin_one(i, q.data(), g, (unsigned)(bins - 1), qcnt.data(), qbin.data()));
        scan(qcnt, qoff);
        REPLAY(nq, cloud_qorder_one(i, qbin.data(), qoff.data(), qcnt.data(), order.data()));
        std::vector<char> seen(nq, 0); for (int v : order) { if (v < 0 || seen[v]) { printf("order is no permutation\n"); exit(4); } seen[v] = 1; }
    }
    REPLAY(nq, cloud_query_one(i, q.data(), bin ? order.data() : (const int*)nullptr, g, od2.data(), want_idx ? oidx.data() : (int32_t*)nullptr));
}

static void brute(const std::vector<float>& t, const std::vector<float>& q, float radius, std::vector<float>& od2, std::vector<int32_t>& oidx) {
    const float r2 = radius * radius; size_t nq = q.size() / 3, n = t.size() / 3;
    od2.assign(nq, INFINITY); oidx.assign(nq, -1);
    for (size_t i = 0; i < nq; ++i) {
        if (!(cloud_finite(q[3*i]) && cloud_finite(q[3*i+1]) && cloud_finite(q[3*i+2]))) continue;
        for (size_t k = 0; k < n; ++k) {
            if (!(cloud_finite(t[3*k]) && cloud_finite(t[3*k+1]) && cloud_finite(t[3*k+2]))) continue;
            volatile float dx = q[3*i] - t[3*k], dy = q[3*i+1] - t[3*k+1], dz = q[3*i+2] - t[3*k+2];
            volatile float a = dx * dx, b = dy * dy, c = dz * dz; volatile float s = a + b; volatile float d2 = s + c;
            if (d2 <= r2 && (oidx[i] < 0 || d2 < od2[i])) { od2[i] = d2; oidx[i] = (int)k; }
        }
    }
}

static int compare(const char* name, const std::vector<float>& t, const std::vector<float>& q, float radius) {
    std::vector<float> a, b; std::vector<int32_t> ai, bi; long long st[4] = {0,0,0,0}; int bad_total = 0;
    brute(t, q, radius, a, ai);
    for (int mode = 0; mode < 3; ++mode) {
        gpu_like(t, q, radius, mode != 1, mode != 2, b, bi, st);
        size_t bad = 0;
        for (size_t i = 0; i < a.size(); ++i) bad += memcmp(&a[i], &b[i], 4) != 0 || (mode != 2 && ai[i] != bi[i]);
        printf("%-16s r=%-10g mode %d: %zu queries, %zu differ; finite %lld cells %lld fullest %lld slots %lld\n", name, radius, mode, a.size(), bad, st[0], st[1], st[2], st[3]);
        bad_total += bad != 0;
    }
    return bad_total;
}

int main() {
    std::mt19937 g(3);
    for (int i = 0; i < 256; ++i) order256[i] = i;
    std::shuffle(order256, order256 + 256, g);   // threads of a block in a scrambled order
    std::uniform_real_distribution<float> U(0.f, 1.f);
    int fails = 0;
    {
        std::vector<float> t(4500), q(3000);
        for (auto& v : t) v = U(g);
        for (auto& v : q) v = U(g);
        q[9] = NAN; q[100] = INFINITY; q[301] = -INFINITY; t[30] = INFINITY; t[61] = NAN; q[12] = 1e30f; q[16] = -1e30f;
        for (float r : {0.02f, 0.2f, 4.0f}) fails += compare("random", t, q, r);
    }
    {   // one point per cell, > 65536 slots
        const float r = 0.01f; std::vector<float> t, q;
        for (int i = 0; i < 70000; ++i) { int c[3] = {i % 42, (i / 42) % 42, i / 1764}; for (int a = 0; a < 3; ++a) t.push_back((float)((3 * c[a] + 0.5) * r * (1 + 0x1p-10) + (U(g) - 0.5) * 0.2 * r)); }
        for (int i = 0; i < 1500; ++i) { int k = (int)(U(g) * 69999); for (int a = 0; a < 3; ++a) q.push_back(t[3 * k + a] + (U(g) - 0.5f) * 2.0f * r); }
        fails += compare("many cells", t, q, r);
    }
    {   // one full cell and duplicates
        const float r = 0.5f; std::vector<float> t, q;
        for (int i = 0; i < 5000; ++i) for (int a = 0; a < 3; ++a) t.push_back(0.3f + (float)(int)(U(g) * 8) * 0.02f);   // many exact duplicates
        for (int i = 0; i < 50; ++i) for (int a = 0; a < 3; ++a) t.push_back(U(g) * 6 - 3);
        for (int i = 0; i < 300; ++i) for (int a = 0; a < 3; ++a) q.push_back(0.3f + (float)(int)(U(g) * 16 - 4) * 0.01f);
        fails += compare("full cell, ties", t, q, r);
    }
    {
        std::vector<float> t = {0, 0, 0, 0, 1e6f, 0}, q = {0, 0.05f, 0, 0, 1e6f, 0.01f, 5, 5, 5};
        fails += compare("far apart", t, q, 1000.0f);
        std::vector<float> none, nan3 = {NAN, 0, 0};
        fails += compare("no target", none, q, 1.0f);
        fails += compare("nan target", nan3, q, 1.0f);
    }
    for (float shift : {0.0f, 1000.25f, -77.125f}) {
        const float r = 0.25f;
        std::vector<float> t, q;
        for (int i = -4; i <= 4; ++i) for (int j = -4; j <= 4; ++j) for (int k = -4; k <= 4; ++k) { t.push_back(i * r + shift); t.push_back(j * r + shift); t.push_back(k * r + shift); }
        const float steps[3] = {r, std::nextafter(r, 1.0f), r - 0x1p-20f};
        q = t;
        for (float s : steps) for (float sign : {-1.0f, 1.0f}) for (int m = 0; m < 6; ++m)
            for (size_t p = 0; p < t.size() / 3; ++p) {
                float d[3] = {0, 0, 0};
                if (m < 3) d[m] = sign * s; else { d[(m - 3)] = sign * s; d[(m - 2) % 3] = -sign * s; }
                for (int a = 0; a < 3; ++a) q.push_back(t[3 * p + a] + d[a]);
            }
        fails += compare("lattice", t, q, r);
    }
    {   // random radius / offsets / scales: points near cell borders by construction (multiples of radius plus tiny jitter)
        for (int trial = 0; trial < 40; ++trial) {
            const float r = std::ldexp(0.5f + U(g), (int)(U(g) * 20) - 10), shift = (U(g) - 0.5f) * r * 1000.0f;
            std::vector<float> t, q;
            for (int i = 0; i < 600; ++i) for (int a = 0; a < 3; ++a) t.push_back(shift + r * (float)(int)(U(g) * 12) + (U(g) < 0.5f ? 0.0f : (U(g) - 0.5f) * r * 1e-5f));
            for (int i = 0; i < 2000; ++i) for (int a = 0; a < 3; ++a) q.push_back(shift + r * (float)((int)(U(g) * 14) - 1) + (U(g) < 0.5f ? 0.0f : (U(g) - 0.5f) * r * 1e-5f));
            fails += compare("border-jitter", t, q, r);
        }
    }
    printf(fails ? "FAILED %d\n" : "all equal\n", fails);
    return fails != 0;
}
