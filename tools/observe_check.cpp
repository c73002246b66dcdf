// observe_check.cpp -- the three passes of csrc/pm_observe.hpp replayed on the host, thread by thread in a scrambled order, through
// the header's own __host__ __device__ code (the face and pixel rule and the per-thread body of every kernel), in the launch order of
// observer_create_device / observer_classify_chunk of mpmvs_cloud.hip and with buffers of exactly their sizes (Zc for a chunk of
// kObserveChunk scanners, Zn for all of them), against a plain-loop statement of the contract written out on
// its own: random scans and queries with non-finite, far-away and on-the-scanner points, the direction lattice with its ties and
// the clamp at x == R, R = 1, a window larger than the face, an owner per point, more scanners than a chunk, and 70 001 points in
// one pixel.  A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/observe_check tools/observe_check.cpp && build/observe_check
// Prints one line per case and "all equal"; exit status 1 if any result differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_observe.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = b_ * 256 + order256[t_];                                        \
            if (i < (size_t)(count)) call;                                                   \
        }

struct Result {
    std::vector<float> zn;   // [n_scanners][6][R][R]
    std::vector<int> free, cov;
    long long finite = 0;
};

// owner: empty, or one entry per scan point
static void gpu_like(const std::vector<float>& scan, const std::vector<float>& sc, const std::vector<int>& owner, int R, int w, const std::vector<float>& q,
                     float rel, float ab, bool want_cov, Result& out) {
    const size_t n = scan.size() / 3, nq = q.size() / 3, map = (size_t)6 * R * R;
    const int ns = (int)(sc.size() / 3);
    ObserveScanners all;
    memset(&all, 0, sizeof all);
    all.n = ns;
    memcpy(all.s, sc.data(), sc.size() * 4);
    // exact-size buffers: AddressSanitizer sees any index outside them
    out.zn.assign(map * ns, -1.0f);
    out.finite = 0;
    const int per = std::min(kObserveChunk, ns);
    std::vector<uint32_t> zc(map * per);
    for (int j0 = 0; j0 < ns; j0 += per) {
        ObserveScanners A = all;
        A.j0 = j0, A.n = std::min(per, ns - j0);
        const size_t n_pix = map * A.n;
        std::fill(zc.begin(), zc.begin() + n_pix, kRenderInfBits);
        REPLAY(n, observe_point_one(i, scan.data(), owner.empty() ? nullptr : owner.data(), A, R, zc.data()));
        REPLAY(n_pix, out.finite += observe_near_one(i, zc.data(), R, w, out.zn.data() + map * j0));
    }
    out.free.assign(nq, -1);
    out.cov.assign(want_cov ? nq : 0, -1);
    REPLAY(nq, observe_classify_one(i, q.data(), all, R, out.zn.data(), 1.0f - rel, ab, out.free.data(), want_cov ? out.cov.data() : nullptr));
}

// the contract in plain loops; every fp32 operation through a volatile, so that nothing is fused or kept wider
static bool place(const float* p, const float* S, int R, int& f, int& px, int& py, float& z) {
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) return false;
    volatile float d[3], A[3];
    for (int a = 0; a < 3; ++a) d[a] = p[a] - S[a], A[a] = std::fabs(d[a]);
    int m = 0;
    for (int a = 1; a < 3; ++a)
        if (A[a] > A[m]) m = a;
    z = A[m];
    if (!(std::isfinite(z) && z > 0.0f)) return false;
    f = 2 * m + (d[m] < 0.0f ? 1 : 0);
    volatile float h = (float)R * 0.5f;
    volatile float qb = d[(m + 1) % 3] / z, qc = d[(m + 2) % 3] / z;
    volatile float tb = h * qb, tc = h * qc;
    volatile float x = tb + h, y = tc + h;
    px = x >= (float)R ? R - 1 : (int)x;
    py = y >= (float)R ? R - 1 : (int)y;
    return true;
}

static void statement(const std::vector<float>& scan, const std::vector<float>& sc, const std::vector<int>& owner, int R, int w, const std::vector<float>& q,
                      float rel, float ab, Result& out) {
    const size_t n = scan.size() / 3, nq = q.size() / 3, map = (size_t)6 * R * R;
    const int ns = (int)(sc.size() / 3);
    std::vector<float> Zc(map * ns, INFINITY);
    for (int j = 0; j < ns; ++j)
        for (size_t i = 0; i < n; ++i) {
            if (!owner.empty() && owner[i] != j) continue;
            int f, px, py;
            float z;
            if (!place(&scan[3 * i], &sc[3 * j], R, f, px, py, z)) continue;
            float& at = Zc[map * j + ((size_t)f * R + py) * R + px];
            at = std::min(at, z);
        }
    out.zn.assign(map * ns, INFINITY);
    out.finite = 0;
    for (int j = 0; j < ns; ++j)
        for (int f = 0; f < 6; ++f)
            for (int y = 0; y < R; ++y)
                for (int x = 0; x < R; ++x) {
                    float v = INFINITY;
                    for (int yy = y - w; yy <= y + w; ++yy)
                        for (int xx = x - w; xx <= x + w; ++xx)
                            if (yy >= 0 && yy < R && xx >= 0 && xx < R) v = std::min(v, Zc[map * j + ((size_t)f * R + yy) * R + xx]);
                    out.zn[map * j + ((size_t)f * R + y) * R + x] = v;
                    out.finite += std::isfinite(v);
                }
    out.free.assign(nq, 0);
    out.cov.assign(nq, 0);
    volatile float m1 = 1.0f - rel;
    for (size_t i = 0; i < nq; ++i)
        for (int j = 0; j < ns; ++j) {
            int f, px, py;
            float z;
            if (!place(&q[3 * i], &sc[3 * j], R, f, px, py, z)) continue;
            const float zn = out.zn[map * j + ((size_t)f * R + py) * R + px];
            if (!std::isfinite(zn)) continue;
            volatile float lhs = z + ab, rhs = zn * m1;
            ++out.cov[i];
            out.free[i] += lhs < rhs;
        }
}

static int compare(const char* name, const std::vector<float>& scan, const std::vector<float>& sc, const std::vector<int>& owner, int R, int w,
                   const std::vector<float>& q, float rel, float ab) {
    Result a, b;
    statement(scan, sc, owner, R, w, q, rel, ab, a);
    int bad_total = 0;
    for (int want_cov = 1; want_cov >= 0; --want_cov) {
        gpu_like(scan, sc, owner, R, w, q, rel, ab, want_cov != 0, b);
        size_t bad = a.zn.size() != b.zn.size() || a.finite != b.finite, n_free = 0, n_cov = 0;
        for (size_t k = 0; k < a.zn.size() && k < b.zn.size(); ++k) bad += memcmp(&a.zn[k], &b.zn[k], 4) != 0;
        for (size_t k = 0; k < a.free.size(); ++k) {
            n_free += a.free[k] != 0, n_cov += a.cov[k] != 0;
            bad += a.free[k] != b.free[k] || (want_cov && a.cov[k] != b.cov[k]);
        }
        printf("%-16s R %-3d w %d rel %-5g abs %-5g owner %d cov %d: %zu scanners, %zu scan points, %lld of %zu pixels finite, %zu queries (%zu covered, %zu free), %zu differ\n",
               name, R, w, rel, ab, (int)!owner.empty(), want_cov, sc.size() / 3, scan.size() / 3, a.finite, a.zn.size(), a.free.size(), n_cov, n_free, bad);
        bad_total += bad != 0;
    }
    return bad_total;
}

int main() {
    std::mt19937 g(9);
    for (int i = 0; i < 256; ++i) order256[i] = i;
    std::shuffle(order256, order256 + 256, g);   // threads of a block in a scrambled order
    std::uniform_real_distribution<float> U(0.f, 1.f);
    int fails = 0;
    const std::vector<int> none;
    const std::vector<float> sc3 = {0.1f, -0.2f, 0.3f, -1.5f, 0.5f, 0.0f, -3e38f, 0.0f, 0.0f};   // the last one: differences that overflow
    auto junk = [&](size_t n, const std::vector<float>& sc) {
        std::vector<float> xyz(3 * n);
        for (auto& v : xyz) v = U(g) * 4.0f - 2.0f;
        const float bad[] = {NAN, INFINITY, -INFINITY, 1e30f, -1e30f, 3e38f, -3e38f};
        for (size_t k = 0; k < n / 100 + 1; ++k) xyz[(size_t)(U(g) * (3 * n - 1))] = bad[k % 7];
        for (size_t k = 0; k < sc.size() / 3 && k < n; ++k)   // a point on every scanner: z == 0
            for (int a = 0; a < 3; ++a) xyz[3 * (size_t)(U(g) * (n - 1)) + a] = sc[3 * k + a];
        return xyz;
    };
    {   // junk coordinates
        const std::vector<float> scan = junk(20000, sc3), q = junk(5000, sc3);
        for (int R : {1, 2, 3, 8, 16})
            for (int w : {0, 1, 2, 8}) fails += compare("random", scan, sc3, none, R, w, q, R == 8 ? 0.05f : 0.02f, R == 8 ? 0.01f : 0.0f);
        fails += compare("rel 0", scan, sc3, none, 16, 1, q, 0.0f, 0.0f);
        std::vector<int> owner(20000);   // an owner per point, -1 among them
        for (auto& o : owner) o = (int)(U(g) * 4.0f) - 1;
        fails += compare("owner", scan, sc3, owner, 8, 1, q, 0.02f, 0.0f);
        std::vector<float> many;   // kObserveChunk + 3 scanners: two chunks
        for (int j = 0; j < kObserveChunk + 3; ++j) many.insert(many.end(), {U(g) * 2.0f - 1.0f, U(g) * 2.0f - 1.0f, U(g) * 2.0f - 1.0f});
        fails += compare("two chunks", scan, many, none, 8, 1, q, 0.02f, 0.0f);
        std::vector<int> owner11(20000);
        for (auto& o : owner11) o = (int)(U(g) * 12.0f) - 1;
        fails += compare("two chunks", scan, many, owner11, 5, 2, q, 0.02f, 0.0f);
        fails += compare("no point", {}, sc3, none, 4, 1, q, 0.02f, 0.0f);
        fails += compare("nan point", {NAN, 0, 0}, sc3, none, 4, 1, q, 0.02f, 0.0f);
        fails += compare("no query", scan, sc3, none, 4, 1, {}, 0.02f, 0.0f);
    }
    {   // the direction lattice: ties, the clamp at x == R, all six faces; |d_b| one step above and below |d_m|
        const std::vector<float> S = {0.25f, -0.5f, 1.0f};
        std::vector<float> pts;
        for (float s : {0.5f, 1.0f, 3.0f})
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b)
                    for (int c = -1; c <= 1; ++c) pts.insert(pts.end(), {S[0] + s * a, S[1] + s * b, S[2] + s * c});
        for (int m = 0; m < 3; ++m)
            for (float sm : {-1.0f, 1.0f})
                for (float sb : {-1.0f, 1.0f})
                    for (float e : {std::nextafter(1.0f, 0.0f), std::nextafter(1.0f, 2.0f)}) {
                        float d[3] = {0.125f, 0.125f, 0.125f};
                        d[m] = sm, d[(m + 1) % 3] = sb * e;
                        pts.insert(pts.end(), {S[0] + d[0], S[1] + d[1], S[2] + d[2]});
                    }
        std::vector<float> q = pts;
        for (size_t k = 0; k < pts.size(); ++k) q.push_back(S[k % 3] + (pts[k] - S[k % 3]) * 0.5f);   // the same directions, nearer
        for (int R : {1, 2, 3, 8, 64})
            for (int w : {0, 1}) fails += compare("lattice", pts, S, none, R, w, q, 0.0f, 0.0f);
    }
    {   // a window larger than the face
        const std::vector<float> scan = junk(300, sc3), q = junk(300, sc3);
        for (int R : {1, 3, 5}) fails += compare("window > face", scan, sc3, none, R, 8, q, 0.02f, 0.0f);
    }
    {   // 70 001 points on one ray, all into one pixel
        const std::vector<float> S = {0.0f, 0.0f, 0.0f};
        std::vector<float> scan, q;
        for (int k = 0; k < 70001; ++k) {
            const float t = 1.0f + (float)((k * 7919) % 70001) * 1e-4f;
            scan.insert(scan.end(), {0.3f * t, t, -0.2f * t});
        }
        for (int k = 0; k < 64; ++k) q.insert(q.end(), {0.3f * (0.9f + 0.005f * k), 0.9f + 0.005f * k, -0.2f * (0.9f + 0.005f * k)});
        fails += compare("one pixel", scan, S, none, 2, 0, q, 0.0f, 0.0f);
        fails += compare("one pixel", scan, S, none, 1024, 1, q, 0.02f, 0.0f);
    }
    printf(fails ? "FAILED %d\n" : "all equal\n", fails);
    return fails != 0;
}
