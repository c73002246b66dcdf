// align_check.cpp -- the ICP pass of csrc/pm_align.hpp replayed on the host, thread by thread in a scrambled order, through the
// header's own __host__ __device__ code (the transform, the binning, the shared 27-cell search, the pair and its 18 terms per thread; the
// scans, the wave sum -- the xor butterfly with every 64-bit value crossing as two dwords -- the four waves of a block and the
// adds of the blocks are plain loops here), in the launch order of align_pass of mpmvs_cloud.hip and with buffers of exactly their
// sizes, against the plain-loop statement of include/mpmvs.h; |a|, |b| <= 1 is asserted for every matched pair.  Then the solver
// of csrc/pm_align_host.hpp on random, reflected, planar and under-determined inputs.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/align_check tools/align_check.cpp && build/align_check
// Prints one line per case and "all equal"; exit status 1 if a sum differs in a bit or the solver misses a bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_align.hpp"
#include "pm_align_host.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = b_ * 256 + order256[t_];                                        \
            if (i < (size_t)(count)) call;                                                   \
        }

static void scan(const std::vector<int>& cnt, std::vector<int>& off) { off[0] = 0; for (size_t i = 0; i < cnt.size(); ++i) off[i + 1] = off[i] + cnt[i]; }

static bool box(const std::vector<float>& t, float mn[3], float mx[3], long long& nf) {
    nf = 0;
    for (size_t i = 0; i < t.size() / 3; ++i) {
        const float* p = &t[3 * i];
        if (!(cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]))) continue;
        for (int a = 0; a < 3; ++a) { mn[a] = nf ? std::min(mn[a], p[a]) : p[a]; mx[a] = nf ? std::max(mx[a], p[a]) : p[a]; }
        ++nf;
    }
    return nf > 0;
}

// what mpmvs_align_sums does, with the kernels replayed
static void gpu_like(const std::vector<float>& t, const std::vector<float>& src, const double M[12], float radius, bool bin, long long sums[18], double frame[4]) {
    const int n = (int)(t.size() / 3), ns = (int)(src.size() / 3);
    for (int k = 0; k < 18; ++k) sums[k] = 0;
    for (int k = 0; k < 4; ++k) frame[k] = 0.0;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}; long long nf = 0;
    if (!box(t, mn, mx, nf)) return;
    align_frame(mn, mx, radius, frame);
    if (!ns) return;
    const int lg = cloud_slots_log2(nf); const size_t slots = (size_t)1 << lg;
    // exact-size buffers: AddressSanitizer sees any index outside them
    std::vector<unsigned long long> keys(slots, kCloudEmpty); std::vector<int> cnt(slots, 0), off(slots + 1), slot_of(n); std::vector<uint4> pts(nf);
    const double edge = cloud_edge(radius);
    REPLAY(n, cloud_insert_one(i, t.data(), (double)mn[0], (double)mn[1], (double)mn[2], edge, (unsigned)(slots - 1), keys.data(), cnt.data(), slot_of.data()));
    scan(cnt, off);
    REPLAY(n, cloud_scatter_one(i, t.data(), slot_of.data(), off.data(), cnt.data(), pts.data()));
    CloudGrid g; for (int a = 0; a < 3; ++a) g.mn[a] = mn[a]; g.edge = edge; g.r2 = radius * radius; g.mask = (unsigned)(slots - 1); g.keys = keys.data(); g.off = off.data(); g.pts = pts.data();
    AlignXf f; for (int k = 0; k < 12; ++k) f.m[k] = M[k]; for (int k = 0; k < 3; ++k) f.o[k] = frame[k]; f.iu = 1.0 / frame[3];
    int bl = 8; while (bl < kCloudMaxSlotsLog2 && (1ll << bl) < ns) ++bl;
    const size_t bins = (size_t)1 << bl;
    std::vector<int> qcnt(bins, 0), qoff(bins + 1), qbin(ns), order(ns, -1);
    if (bin) {
        REPLAY(ns, align_qbin_one(i, src.data(), f, g, (unsigned)(bins - 1), qcnt.data(), qbin.data()));
        scan(qcnt, qoff);
        REPLAY(ns, cloud_qorder_one(i, qbin.data(), qoff.data(), qcnt.data(), order.data()));
        std::vector<char> seen(ns, 0); for (int v : order) { if (v < 0 || seen[v]) { printf("order is no permutation\n"); exit(4); } seen[v] = 1; }
    }
    unsigned long long dev[18] = {0};
    for (size_t b = 0; b < ((size_t)ns + 255) / 256; ++b) {
        static long long v[256][18];
        for (unsigned tt = 0; tt < 256; ++tt) {
            const unsigned th = order256[tt]; const size_t j = b * 256 + th;
            double a[3] = {0, 0, 0}, b[3] = {0, 0, 0}, dn = 0;
            const bool matched = j < (size_t)ns && align_pair_one(j, src.data(), bin ? order.data() : (const int*)nullptr, f, g, t.data(), a, b, dn);
            for (int k = 0; k < 18; ++k) v[th][k] = matched ? align_term(k, a, b, dn) : 0;
        }
        long long part[4][18];
        for (int w = 0; w < 4; ++w)
            for (int k = 0; k < 18; ++k) {
                long long lane[64], next[64];
                for (int l = 0; l < 64; ++l) lane[l] = v[64 * w + l][k];
                for (int d = 32; d > 0; d >>= 1) {   // the butterfly: the partner's value arrives as two dwords
                    for (int l = 0; l < 64; ++l) {
                        const unsigned lo = (unsigned)((unsigned long long)lane[l ^ d] & 0xffffffffull), hi = (unsigned)((unsigned long long)lane[l ^ d] >> 32);
                        next[l] = (long long)((unsigned long long)lane[l] + (((unsigned long long)hi << 32) | lo));
                    }
                    memcpy(lane, next, sizeof lane);
                }
                part[w][k] = lane[0];
                for (int l = 1; l < 64; ++l) if (lane[l] != lane[0]) { printf("lanes disagree after the butterfly\n"); exit(5); }
            }
        for (int k = 0; k < 18; ++k) {
            const long long s = (long long)(((unsigned long long)part[0][k] + (unsigned long long)part[1][k]) + ((unsigned long long)part[2][k] + (unsigned long long)part[3][k]));
            if (s != 0) dev[k] += (unsigned long long)s;
        }
    }
    for (int k = 0; k < 18; ++k) sums[k] = (long long)dev[k];
}

// the statement, written on its own
static void brute(const std::vector<float>& t, const std::vector<float>& src, const double M[12], float radius, long long sums[18], double frame[4]) {
    for (int k = 0; k < 18; ++k) sums[k] = 0;
    for (int k = 0; k < 4; ++k) frame[k] = 0.0;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}; long long nf = 0;
    if (!box(t, mn, mx, nf)) return;
    double ext = 0;
    for (int a = 0; a < 3; ++a) { frame[a] = 0.5 * ((double)mn[a] + (double)mx[a]); ext = std::max(ext, (double)mx[a] - (double)mn[a]); }
    const double h = 0.5 * ext + 2.0 * (double)radius;
    double u = 1.0; while (u < h) u *= 2.0; while (u * 0.5 >= h) u *= 0.5;
    frame[3] = u;
    const double iu = 1.0 / u; const float r2 = radius * radius;
    for (size_t i = 0; i < src.size() / 3; ++i) {
        const float* s = &src[3 * i];
        if (!(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]))) continue;
        float y[3];
        for (int k = 0; k < 3; ++k) {
            volatile double p0 = M[4 * k] * (double)s[0], p1 = M[4 * k + 1] * (double)s[1], p2 = M[4 * k + 2] * (double)s[2];
            volatile double q = p0 + p1; volatile double r = q + p2; volatile double w = r + M[4 * k + 3];
            y[k] = (float)w;
        }
        if (!(std::isfinite(y[0]) && std::isfinite(y[1]) && std::isfinite(y[2]))) continue;
        long long best = -1; float bd = 0;
        for (size_t k = 0; k < t.size() / 3; ++k) {
            if (!(std::isfinite(t[3*k]) && std::isfinite(t[3*k+1]) && std::isfinite(t[3*k+2]))) continue;
            volatile float dx = y[0] - t[3*k], dy = y[1] - t[3*k+1], dz = y[2] - t[3*k+2];
            volatile float a = dx * dx, b = dy * dy, c = dz * dz; volatile float sm = a + b; volatile float d2 = sm + c;
            if (d2 <= r2 && (best < 0 || d2 < bd)) { bd = d2; best = (long long)k; }
        }
        if (best < 0) continue;
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = ((double)y[k] - frame[k]) * iu; b[k] = ((double)t[3 * best + k] - frame[k]) * iu;
            if (!(std::fabs(a[k]) <= 1.0 && std::fabs(b[k]) <= 1.0)) { printf("|a| or |b| above 1: %g %g\n", a[k], b[k]); exit(6); }
        }
        sums[0] += 1;
        for (int k = 0; k < 3; ++k) {
            sums[1 + k] += llrint(a[k] * 0x1p30); sums[4 + k] += llrint(b[k] * 0x1p30);
            for (int l = 0; l < 3; ++l) { volatile double p = a[k] * b[l]; sums[7 + 3 * k + l] += llrint(p * 0x1p30); }
        }
        volatile double xx = a[0] * a[0], yy = a[1] * a[1], zz = a[2] * a[2]; volatile double s2 = xx + yy; volatile double s3 = s2 + zz;
        sums[16] += llrint(s3 * 0x1p30);
        volatile double i2 = iu * iu; volatile double dd = (double)bd * i2;
        sums[17] += llrint(dd * 0x1p30);
    }
}

static int compare(const char* name, const std::vector<float>& t, const std::vector<float>& src, const double M[12], float radius) {
    long long want[18], got[18]; double wf[4], gf[4]; int bad_total = 0;
    brute(t, src, M, radius, want, wf);
    for (int mode = 0; mode < 2; ++mode) {
        gpu_like(t, src, M, radius, mode == 0, got, gf);
        const bool bad = memcmp(want, got, sizeof want) != 0 || memcmp(wf, gf, sizeof wf) != 0;
        printf("%-18s r=%-8g mode %d: %zu sources, %lld matched, sum[1] %lld sum[17] %lld u %g: %s\n", name, radius, mode, src.size() / 3, want[0], want[1], want[17], wf[3], bad ? "DIFFER" : "equal");
        bad_total += bad;
    }
    return bad_total;
}

// ---- solver ----------------------------------------------------------------------------------------------------------
static void pair_sums(const std::vector<double>& a, const std::vector<double>& b, long long sums[18]) {
    for (int k = 0; k < 18; ++k) sums[k] = 0;
    for (size_t i = 0; i < a.size() / 3; ++i) {
        const double *p = &a[3 * i], *q = &b[3 * i];
        sums[0] += 1;
        double d2 = 0;
        for (int k = 0; k < 3; ++k) {
            sums[1 + k] += llrint(p[k] * 0x1p30); sums[4 + k] += llrint(q[k] * 0x1p30);
            for (int l = 0; l < 3; ++l) sums[7 + 3 * k + l] += llrint(p[k] * q[l] * 0x1p30);
            d2 += (p[k] - q[k]) * (p[k] - q[k]);
        }
        sums[16] += llrint((p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) * 0x1p30);
        sums[17] += llrint(d2 * 0x1p30);
    }
}

static void rot(std::mt19937& g, double R[3][3]) {   // a random rotation from a random unit quaternion
    std::normal_distribution<double> N(0, 1);
    double q[4], n = 0; for (double& v : q) { v = N(g); n += v * v; } n = std::sqrt(n); for (double& v : q) v /= n;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double r[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)}, {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)}, {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    memcpy(R, r, sizeof r);
}

static int solver_case(const char* name, std::mt19937& g, int n, bool planar, bool reflect, int with_scale) {
    std::uniform_real_distribution<double> U(-0.4, 0.4);
    double R[3][3]; rot(g, R);
    const double c = with_scale ? 0.9 + 0.2 * (U(g) + 0.4) : 1.0, tr[3] = {U(g) * 0.2, U(g) * 0.2, U(g) * 0.2};
    std::vector<double> a(3 * n), b(3 * n);
    for (int i = 0; i < n; ++i) {
        double p[3] = {U(g), U(g), planar ? 0.0 : U(g)};
        // quantise as the pass sees them (multiples of 2^-24), so that the fixed-point sums carry the products' rounding only
        for (int k = 0; k < 3; ++k) a[3 * i + k] = std::nearbyint(p[k] * 0x1p24) * 0x1p-24;
        const double* q = &a[3 * i];
        for (int k = 0; k < 3; ++k) b[3 * i + k] = c * (R[k][0] * q[0] + R[k][1] * q[1] + R[k][2] * (reflect ? -q[2] : q[2])) + tr[k];
    }
    long long sums[18]; pair_sums(a, b, sums);
    const double frame[4] = {0, 0, 0, 1}, I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double D[12], rmse = -1;
    const int rc = align_solve(sums, frame, with_scale, I, D, &rmse);
    // always: c R is a scaled rotation with determinant > 0
    double RtR = 0, det; double Rm[3][3];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) Rm[r][k] = D[4 * r + k];
    det = align_det3(Rm);
    const double sc = std::cbrt(det);
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) { double d = 0; for (int m = 0; m < 3; ++m) d += Rm[m][r] * Rm[m][k]; RtR = std::max(RtR, std::fabs(d / (sc * sc) - (r == k))); }
    double err = 0;
    if (!reflect) {   // the known similarity comes back
        for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) err = std::max(err, std::fabs(D[4 * r + k] - c * R[r][k])); err = std::max(err, std::fabs(D[4 * r + 3] - tr[r])); }
    }
    const bool ok = rc == 0 && det > 0 && RtR < 1e-12 && err < 1e-6 && rmse >= 0;
    printf("solver %-22s n=%-5d rc %d det %.6f |RtR-I| %.2e err %.2e rmse %.4g: %s\n", name, n, rc, det, RtR, err, rmse, ok ? "ok" : "BAD");
    return !ok;
}

static int solver_degenerate() {
    int bad = 0;
    const double frame[4] = {1, 2, 3, 4}, Min[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    double out[12], rmse;
    long long sums[18];
    std::vector<double> a = {0.1, 0.2, 0.3, -0.1, 0.0, 0.2}, b = a;
    pair_sums(a, b, sums);                                        // two pairs
    bad += !(align_solve(sums, frame, 1, Min, out, &rmse) == 1 && memcmp(out, Min, sizeof out) == 0);
    for (int k = 0; k < 18; ++k) sums[k] = 0;                     // none
    bad += !(align_solve(sums, frame, 1, Min, out, &rmse) == 1 && memcmp(out, Min, sizeof out) == 0 && rmse == 0.0);
    a = {0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25}; b = {0.1, 0.2, 0.3, 0.3, 0.1, 0.0, -0.2, 0.1, 0.1, 0.0, 0.0, 0.5};
    pair_sums(a, b, sums);                                        // one source position: no variance
    bad += !(align_solve(sums, frame, 1, Min, out, &rmse) == 1 && memcmp(out, Min, sizeof out) == 0);
    a.assign(12, 0.0);
    pair_sums(b, a, sums);                                        // every target at the frame's origin: the covariance vanishes
    bad += !(align_solve(sums, frame, 1, Min, out, &rmse) == 1 && memcmp(out, Min, sizeof out) == 0);
    a = {0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.3, 0.3, 0.3, -0.1, -0.1, -0.1}; b = a;
    pair_sums(a, b, sums);                                        // collinear: answered, finite, and a rotation
    const int rc = align_solve(sums, frame, 0, Min, out, &rmse);
    bool fin = true; for (double v : out) fin = fin && std::isfinite(v);
    bad += !(rc == 0 && fin);
    printf("solver degenerate inputs (collinear: rc %d): %s\n", rc, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    std::mt19937 g(7);
    for (int i = 0; i < 256; ++i) order256[i] = i;
    std::shuffle(order256, order256 + 256, g);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const double S[12] = {1.01 * 0.96, 1.01 * -0.28, 0, 0.12, 1.01 * 0.28, 1.01 * 0.96, 0, -0.1, 0, 0, 1.01, 0.004};
    int fails = 0;
    {
        std::vector<float> t(4500), s(3000);
        for (auto& v : t) v = U(g);
        for (auto& v : s) v = U(g);
        s[9] = NAN; s[100] = INFINITY; s[301] = -INFINITY; t[30] = INFINITY; t[61] = NAN; s[12] = 1e30f; s[16] = -1e30f;
        for (float r : {0.02f, 0.2f, 4.0f}) { fails += compare("random, identity", t, s, I, r); fails += compare("random, similarity", t, s, S, r); }
        for (int ns : {1, 63, 64, 65, 255, 256, 257}) { std::vector<float> c(s.begin() + 30, s.begin() + 30 + 3 * ns); fails += compare("wave borders", t, c, I, 0.2f); }
        const double big[12] = {1e300, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        fails += compare("overflowing M", t, s, big, 0.2f);
    }
    for (int sign : {-1, 0}) {   // corners: terms of +-1, sums past 2^32 and 2^38
        for (int n : {64, 600}) {
            std::vector<float> t, s;
            for (int c = 0; c < 8; ++c) for (int a = 0; a < 3; ++a) t.push_back(((c >> a) & 1) ? 0.96875f : -0.96875f);   // half extent + 2 r = 1 = u
            for (int i = 0; i < n; ++i) { const int c = sign < 0 ? 0 : (int)(U(g) * 8) & 7; for (int a = 0; a < 3; ++a) s.push_back(t[3 * c + a] * (1.0f - 0x1p-12f * U(g))); }
            fails += compare(sign < 0 ? "corners, negative" : "corners, mixed", t, s, I, 0x1p-6f);
        }
    }
    {   // duplicates and ties
        std::vector<float> t = {0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0.5f, 1, 0}, s = {0.5f, 0, 0, 0.9f, 0, 0, 0.1f, 0.1f, 0, 0.5f, 0.5f, 0};
        fails += compare("ties", t, s, I, 0.75f);
        std::vector<float> none, nan3 = {NAN, 0, 0};
        fails += compare("no target", none, s, I, 1.0f);
        fails += compare("nan target", nan3, s, I, 1.0f);
        fails += compare("no source", t, none, I, 1.0f);
        fails += compare("out of reach", t, s, I, 0.01f);
    }
    for (int trial = 0; trial < 20; ++trial) {   // random radii, offsets and scales: u, o and the frame's margin vary
        const float r = std::ldexp(0.5f + U(g), (int)(U(g) * 16) - 8), shift = (U(g) - 0.5f) * r * 300.0f;
        std::vector<float> t, s;
        for (int i = 0; i < 500; ++i) for (int a = 0; a < 3; ++a) t.push_back(shift + r * 10.0f * U(g));
        for (int i = 0; i < 700; ++i) for (int a = 0; a < 3; ++a) s.push_back(shift + r * (12.0f * U(g) - 1.0f));
        fails += compare("random frame", t, s, I, r);
    }
    for (int ws = 0; ws < 2; ++ws) {
        fails += solver_case(ws ? "random, scale" : "random, rigid", g, 500, false, false, ws);
        fails += solver_case(ws ? "planar, scale" : "planar, rigid", g, 500, true, false, ws);
        fails += solver_case(ws ? "reflected, scale" : "reflected, rigid", g, 500, false, true, ws);
        fails += solver_case(ws ? "three points, scale" : "three points, rigid", g, 3, true, false, ws);
    }
    fails += solver_degenerate();
    printf(fails ? "FAILED %d\n" : "all equal\n", fails);
    return fails != 0;
}
