// align_plane_check.cpp -- the point-to-plane pass of csrc/pm_align_plane.hpp replayed on the host, thread by thread in a scrambled
// order, through the header's own __host__ __device__ code (the transform, the binning, the shared 27-cell search, the pair, its
// normal and its 38 terms per thread; the scans, the wave sum -- the xor butterfly with every 64-bit value crossing as two dwords
// -- the four waves of a block and the adds of the blocks are plain loops here), in the launch order of align_pass of
// mpmvs_cloud.hip and with buffers of exactly their sizes, against the plain-loop statement of include/mpmvs.h written on its own;
// |nh| <= 1, |r| < 0.87 and |term| < 4 are asserted for every matched pair, and the sums of the negated normals must keep every
// bit.  Then the solver of csrc/pm_align_host.hpp on random inputs, exact planes, the three-plane corner, too few pairs and a
// step that asks for a scale <= 0.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/align_plane_check tools/align_plane_check.cpp && build/align_plane_check
// Prints one line per case and "all equal"; exit status 1 if a sum differs in a bit or the solver misses a bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_align_plane.hpp"
#include "pm_align_host.hpp"
using namespace pm;

constexpr int T = kAlignPlaneTerms;
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

// what mpmvs_align_plane_sums does, with the kernels replayed
static void gpu_like(const std::vector<float>& t, const std::vector<float>& nrm, const std::vector<float>& src, const double M[12], float radius, bool bin,
                     long long sums[T], double frame[4]) {
    const int n = (int)(t.size() / 3), ns = (int)(src.size() / 3);
    for (int k = 0; k < T; ++k) sums[k] = 0;
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
    std::vector<unsigned long long> dev(T, 0);   // the device buffer of the sums
    for (size_t b = 0; b < ((size_t)ns + 255) / 256; ++b) {
        static long long v[256][T];
        for (unsigned tt = 0; tt < 256; ++tt) {
            const unsigned th = order256[tt]; const size_t j = b * 256 + th;
            AlignPlanePair p = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const bool matched = j < (size_t)ns && align_plane_pair_one(j, src.data(), bin ? order.data() : (const int*)nullptr, f, g, t.data(), nrm.data(), p);
            for (int k = 0; k < T; ++k) v[th][k] = matched ? align_plane_term(k, p) : 0;
        }
        long long part[4][T];
        for (int w = 0; w < 4; ++w)
            for (int k = 0; k < T; ++k) {
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
        for (int k = 0; k < T; ++k) {
            const long long s = (long long)(((unsigned long long)part[0][k] + (unsigned long long)part[1][k]) + ((unsigned long long)part[2][k] + (unsigned long long)part[3][k]));
            if (s != 0) dev[k] += (unsigned long long)s;
        }
    }
    for (int k = 0; k < T; ++k) sums[k] = (long long)dev[k];
}

static long long fixv(double x) { volatile double s = x * 0x1p30; return llrint(s); }

// the statement, written on its own
static void brute(const std::vector<float>& t, const std::vector<float>& nrm, const std::vector<float>& src, const double M[12], float radius, long long sums[T],
                  double frame[4]) {
    for (int k = 0; k < T; ++k) sums[k] = 0;
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
        const double n[3] = {(double)nrm[3 * best], (double)nrm[3 * best + 1], (double)nrm[3 * best + 2]};
        volatile double q0 = n[0] * n[0], q1 = n[1] * n[1], q2 = n[2] * n[2]; volatile double q01 = q0 + q1; volatile double q = q01 + q2;
        if (!std::isfinite(q) || q == 0.0) continue;
        volatile double len = std::sqrt(q);
        double a[3], e[3], nh[3];
        for (int k = 0; k < 3; ++k) {
            volatile double ak = ((double)y[k] - frame[k]) * iu, bk = ((double)t[3 * best + k] - frame[k]) * iu, ek = ak - bk, nk = n[k] / len;
            a[k] = ak, e[k] = ek, nh[k] = nk;
            if (!(std::fabs(ak) <= 1.0 && std::fabs(bk) <= 1.0 && std::fabs(nk) <= 1.0)) { printf("|a|, |b| or |nh| above 1: %g %g %g\n", ak, bk, nk); exit(6); }
        }
        auto dot = [](const double* x, const double* z) { volatile double p0 = x[0] * z[0], p1 = x[1] * z[1], p2 = x[2] * z[2]; volatile double s01 = p0 + p1; volatile double s = s01 + p2; return (double)s; };
        auto cross = [](double x1, double z2, double x2, double z1) { volatile double p = x1 * z2, m = x2 * z1; volatile double d = p - m; return (double)d; };
        const double r = dot(e, nh);
        const double J[7] = {cross(a[1], nh[2], a[2], nh[1]), cross(a[2], nh[0], a[0], nh[2]), cross(a[0], nh[1], a[1], nh[0]), nh[0], nh[1], nh[2], dot(a, nh)};
        if (!(std::fabs(r) < 0.87)) { printf("|r| = %g\n", r); exit(7); }
        sums[0] += 1;
        int k = 1;
        for (int ii = 0; ii < 7; ++ii)
            for (int jj = ii; jj < 7; ++jj) { volatile double p = J[ii] * J[jj]; if (!(std::fabs(p) < 4.0)) { printf("|term| = %g\n", p); exit(8); } sums[k++] += fixv(p); }
        for (int ii = 0; ii < 7; ++ii) { volatile double p = J[ii] * r; sums[k++] += fixv(p); }
        volatile double rr = r * r; sums[k++] += fixv(rr);
        volatile double i2 = iu * iu; volatile double dd = (double)bd * i2;
        sums[k++] += fixv(dd);
    }
}

static int compare(const char* name, const std::vector<float>& t, const std::vector<float>& nrm, const std::vector<float>& src, const double M[12], float radius) {
    long long want[T], got[T]; double wf[4], gf[4]; int bad_total = 0;
    brute(t, nrm, src, M, radius, want, wf);
    std::vector<float> neg(nrm); for (auto& v : neg) v = -v;
    for (int mode = 0; mode < 3; ++mode) {   // binned, caller order, binned with every normal negated
        gpu_like(t, mode == 2 ? neg : nrm, src, M, radius, mode != 1, got, gf);
        const bool bad = memcmp(want, got, sizeof want) != 0 || memcmp(wf, gf, sizeof wf) != 0;
        printf("%-18s r=%-8g mode %d: %zu sources, %lld matched, sum[7] %lld sum[29] %lld sum[36] %lld u %g: %s\n", name, radius, mode, src.size() / 3, want[0], want[7], want[29], want[36], wf[3], bad ? "DIFFER" : "equal");
        bad_total += bad;
    }
    return bad_total;
}

// ---- solver ----------------------------------------------------------------------------------------------------------
// sources a (normalised frame) against the planes (nh, d): nh . x = d
static void plane_pair_sums(const std::vector<double>& a, const std::vector<double>& nh, const std::vector<double>& d, long long sums[T]) {
    for (int k = 0; k < T; ++k) sums[k] = 0;
    for (size_t i = 0; i < d.size(); ++i) {
        const double *p = &a[3 * i], *n = &nh[3 * i];
        const double g = p[0] * n[0] + p[1] * n[1] + p[2] * n[2], r = g - d[i];
        const double J[7] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2], g};
        sums[0] += 1;
        int k = 1;
        for (int ii = 0; ii < 7; ++ii) for (int jj = ii; jj < 7; ++jj) sums[k++] += llrint(J[ii] * J[jj] * 0x1p30);
        for (int ii = 0; ii < 7; ++ii) sums[k++] += llrint(J[ii] * r * 0x1p30);
        sums[k++] += llrint(r * r * 0x1p30);
        sums[k++] += llrint(r * r * 0x1p30);
    }
}

static void rot(const double w[3], double R[3][3]) {   // the rotation of the quaternion (1, w / 2) normalised, written on its own
    const double n = std::sqrt(1 + 0.25 * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2])), q0 = 1 / n, x = 0.5 * w[0] / n, y = 0.5 * w[1] / n, z = 0.5 * w[2] / n;
    const double r[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - q0 * z), 2 * (x * z + q0 * y)}, {2 * (x * y + q0 * z), 1 - 2 * (x * x + z * z), 2 * (y * z - q0 * x)}, {2 * (x * z - q0 * y), 2 * (y * z + q0 * x), 1 - 2 * (x * x + y * y)}};
    memcpy(R, r, sizeof r);
}

// n sources that a small known similarity (w, tr, sg) would put exactly on their planes; planes: 0 = random normals, 1 = one
// exact plane, 2 = two parallel planes, 3 = the three planes of a corner at `apex`.  The solver must return the step -- to first
// order: the error is of the order of the step squared -- or refuse (want_rc 1).
static int solver_case(const char* name, std::mt19937& g, int n, int planes, int with_scale, int want_rc) {
    std::uniform_real_distribution<double> U(-0.4, 0.4);
    std::normal_distribution<double> N(0, 1);
    const double w[3] = {1e-4 * U(g), 1e-4 * U(g), 1e-4 * U(g)}, tr[3] = {1e-4 * U(g), 1e-4 * U(g), 1e-4 * U(g)}, sg = with_scale ? 1e-4 * U(g) : 0.0;
    const double apex[3] = {0.1, -0.2, 0.05};
    double R[3][3]; rot(w, R);
    std::vector<double> a(3 * n), nh(3 * n), d(n);
    for (int i = 0; i < n; ++i) {
        double* p = &a[3 * i]; double* m = &nh[3 * i];
        for (int k = 0; k < 3; ++k) p[k] = std::nearbyint(U(g) * 0x1p24) * 0x1p-24;
        if (planes == 0) { double l = 0; for (int k = 0; k < 3; ++k) { m[k] = N(g); l += m[k] * m[k]; } l = std::sqrt(l); for (int k = 0; k < 3; ++k) m[k] /= l; }
        else for (int k = 0; k < 3; ++k) m[k] = (planes == 3 ? k == i % 3 : k == 2) ? 1.0 : 0.0;
        double moved[3];
        for (int k = 0; k < 3; ++k) moved[k] = (1 + sg) * (R[k][0] * p[0] + R[k][1] * p[1] + R[k][2] * p[2]) + tr[k];
        if (planes == 0) d[i] = moved[0] * m[0] + moved[1] * m[1] + moved[2] * m[2];   // the plane passes through the moved source
        if (planes == 1) d[i] = 0.125;
        if (planes == 2) d[i] = i % 2 ? 0.125 : -0.25;
        if (planes == 3) d[i] = apex[i % 3];
        if (planes == 3) p[i % 3] = apex[i % 3];   // on its plane already: the scale about the apex is free
    }
    long long sums[T]; plane_pair_sums(a, nh, d, sums);
    const double frame[4] = {0, 0, 0, 1}, I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double D[12], rp = -1, rq = -1;
    const int rc = align_plane_solve(sums, frame, with_scale, I, D, &rp, &rq);
    double err = 0, RtR = 0, Rm[3][3];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) Rm[r][k] = D[4 * r + k];
    const double det = align_det3(Rm), sc = std::cbrt(det);
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) { double v = 0; for (int m = 0; m < 3; ++m) v += Rm[m][r] * Rm[m][k]; RtR = std::max(RtR, std::fabs(v / (sc * sc) - (r == k))); }
    // the step comes back where the pairs over-determine it; m pairs for m unknowns have no bound on their condition, and the
    // grain of the fixed-point residuals (2^-30) shows through it: those cases check the count gate and the shape of D only
    if (planes == 0 && n >= 100) for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) err = std::max(err, std::fabs(D[4 * r + k] - (1 + sg) * R[r][k])); err = std::max(err, std::fabs(D[4 * r + 3] - tr[r])); }
    bool ok = rc == want_rc && rp >= 0 && rq >= 0;
    if (rc == 0) ok = ok && det > 0 && RtR < 1e-12 && err < 1e-7 && (with_scale || std::fabs(det - 1) < 1e-12);
    else ok = ok && memcmp(D, I, sizeof D) == 0;
    printf("solver %-26s n=%-5d rc %d (want %d) det %.9f |RtR-I| %.2e err %.2e rmse_plane %.3g: %s\n", name, n, rc, want_rc, det, RtR, err, rp, ok ? "ok" : "BAD");
    return !ok;
}

static int solver_refusals(std::mt19937& g) {
    int bad = 0;
    std::uniform_real_distribution<double> U(-0.4, 0.4);
    const double frame[4] = {1, 2, 3, 4}, Min[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    double out[12], rp, rq;
    long long sums[T];
    for (int k = 0; k < T; ++k) sums[k] = 0;                       // no pairs
    bad += !(align_plane_solve(sums, frame, 1, Min, out, &rp, &rq) == 1 && memcmp(out, Min, sizeof out) == 0 && rp == 0.0 && rq == 0.0);
    bad += !(align_plane_solve(sums, frame, 0, Min, out, nullptr, nullptr) == 1 && memcmp(out, Min, sizeof out) == 0);
    // well-conditioned sums, then the count below m
    std::vector<double> a(3 * 200), nh(3 * 200), d(200);
    for (int i = 0; i < 200; ++i) { double l = 0; for (int k = 0; k < 3; ++k) { a[3 * i + k] = U(g); nh[3 * i + k] = U(g); l += nh[3 * i + k] * nh[3 * i + k]; } for (int k = 0; k < 3; ++k) nh[3 * i + k] /= std::sqrt(l); d[i] = 0.3 * U(g); }
    plane_pair_sums(a, nh, d, sums);
    bad += !(align_plane_solve(sums, frame, 1, Min, out, &rp, &rq) == 0);
    sums[0] = 6;
    bad += !(align_plane_solve(sums, frame, 1, Min, out, &rp, &rq) == 1 && memcmp(out, Min, sizeof out) == 0);
    bad += !(align_plane_solve(sums, frame, 0, Min, out, &rp, &rq) == 0);
    sums[0] = 5;
    bad += !(align_plane_solve(sums, frame, 0, Min, out, &rp, &rq) == 1 && memcmp(out, Min, sizeof out) == 0);
    // gvec = 1.5 H e_6: the step is sigma = -1.5, a scale of -0.5
    sums[0] = 200;
    const int col6[7] = {7, 13, 18, 22, 25, 27, 28};   // H_06 .. H_66 in the row-by-row triangle
    for (int i = 0; i < 7; ++i) sums[29 + i] = llrint(1.5 * (double)sums[col6[i]]);
    bad += !(align_plane_solve(sums, frame, 1, Min, out, &rp, &rq) == 1 && memcmp(out, Min, sizeof out) == 0);
    for (int i = 0; i < 7; ++i) sums[29 + i] = llrint(1.0 * (double)sums[col6[i]]);   // sigma = -1: a scale of 0 up to rounding
    const int rc0 = align_plane_solve(sums, frame, 1, Min, out, &rp, &rq);
    bool fin = true; for (double v : out) fin = fin && std::isfinite(v);
    bad += !fin;
    sums[1] = -sums[1];                                            // a negative first pivot
    bad += !(align_plane_solve(sums, frame, 0, Min, out, &rp, &rq) == 1 && memcmp(out, Min, sizeof out) == 0);
    printf("solver refusals (sigma = -1: rc %d): %s\n", rc0, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    std::mt19937 g(7);
    for (int i = 0; i < 256; ++i) order256[i] = i;
    std::shuffle(order256, order256 + 256, g);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::normal_distribution<float> N(0.f, 1.f);
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const double S[12] = {1.01 * 0.96, 1.01 * -0.28, 0, 0.12, 1.01 * 0.28, 1.01 * 0.96, 0, -0.1, 0, 0, 1.01, 0.004};
    int fails = 0;
    {
        std::vector<float> t(4500), s(3000), nrm(4500);
        for (auto& v : t) v = U(g);
        for (auto& v : s) v = U(g);
        for (size_t i = 0; i < 1500; ++i) { const float len = std::ldexp(1.0f, (int)(U(g) * 40) - 20); for (int a = 0; a < 3; ++a) nrm[3 * i + a] = N(g) * len; }
        for (int a = 0; a < 3; ++a) { nrm[3 * 7 + a] = 0.0f; nrm[3 * 11 + a] = 1e-40f * (a + 1); nrm[3 * 13 + a] = 3e38f; }   // 0 0 0, subnormal, a finite length whose square is far above fp32
        nrm[3 * 20] = NAN; nrm[3 * 21 + 1] = INFINITY; nrm[3 * 22 + 2] = -INFINITY; nrm[3 * 23] = -0.0f; nrm[3 * 23 + 1] = -0.0f; nrm[3 * 23 + 2] = 0.0f;
        s[9] = NAN; s[100] = INFINITY; s[301] = -INFINITY; t[30] = INFINITY; t[61] = NAN; s[12] = 1e30f; s[16] = -1e30f;
        for (float r : {0.02f, 0.2f, 4.0f}) { fails += compare("random, identity", t, nrm, s, I, r); fails += compare("random, similarity", t, nrm, s, S, r); }
        for (int ns : {1, 63, 64, 65, 255, 256, 257}) { std::vector<float> c(s.begin() + 30, s.begin() + 30 + 3 * ns); fails += compare("wave borders", t, nrm, c, I, 0.2f); }
        const double big[12] = {1e300, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        fails += compare("overflowing M", t, nrm, s, big, 0.2f);
        std::vector<float> none(4500, 0.0f);
        fails += compare("no usable normal", t, none, s, I, 0.2f);
    }
    for (int sign : {-1, 0}) {   // corners with diagonal normals: |g| ~ sqrt 3 * 0.97, g * g ~ 2.8 * 2^30 per pair; sums past 2^32 and 2^38
        for (int n : {64, 600}) {
            std::vector<float> t, s, nrm;
            for (int c = 0; c < 8; ++c) for (int a = 0; a < 3; ++a) { t.push_back(((c >> a) & 1) ? 0.96875f : -0.96875f); nrm.push_back(((c >> a) & 1) ? 2.0f : -2.0f); }   // half extent + 2 r = 1 = u
            for (int i = 0; i < n; ++i) { const int c = sign < 0 ? 0 : (int)(U(g) * 8) & 7; for (int a = 0; a < 3; ++a) s.push_back(t[3 * c + a] * (1.0f - 0x1p-12f * U(g))); }
            fails += compare(sign < 0 ? "corners, one" : "corners, mixed", t, nrm, s, I, 0x1p-6f);
        }
    }
    {   // ties between targets with different normals, and empty inputs
        std::vector<float> t = {0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0.5f, 1, 0}, s = {0.5f, 0.1f, 0, 0.9f, 0, 0.1f, 0.1f, 0.1f, 0, 0.5f, 0.5f, 0};
        std::vector<float> nrm = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1};
        fails += compare("ties", t, nrm, s, I, 0.75f);
        std::vector<float> none, nan3 = {NAN, 0, 0}, n1 = {0, 0, 1};
        fails += compare("no target", none, none, s, I, 1.0f);
        fails += compare("nan target", nan3, n1, s, I, 1.0f);
        fails += compare("no source", t, nrm, none, I, 1.0f);
        fails += compare("out of reach", t, nrm, s, I, 0.01f);
    }
    for (int trial = 0; trial < 20; ++trial) {   // random radii, offsets and scales: u, o and the frame's margin vary
        const float r = std::ldexp(0.5f + U(g), (int)(U(g) * 16) - 8), shift = (U(g) - 0.5f) * r * 300.0f;
        std::vector<float> t, s, nrm;
        for (int i = 0; i < 500; ++i) for (int a = 0; a < 3; ++a) { t.push_back(shift + r * 10.0f * U(g)); nrm.push_back(N(g)); }
        for (int i = 0; i < 700; ++i) for (int a = 0; a < 3; ++a) s.push_back(shift + r * (12.0f * U(g) - 1.0f));
        fails += compare("random frame", t, nrm, s, I, r);
    }
    for (int ws = 0; ws < 2; ++ws) {
        fails += solver_case(ws ? "random, scale" : "random, rigid", g, 500, 0, ws, 0);
        fails += solver_case(ws ? "seven pairs, scale" : "six pairs, rigid", g, ws ? 7 : 6, 0, ws, 0);
        fails += solver_case(ws ? "one plane, scale" : "one plane, rigid", g, 500, 1, ws, 1);
        fails += solver_case(ws ? "parallel planes, scale" : "parallel planes, rigid", g, 500, 2, ws, 1);
        fails += solver_case(ws ? "corner, scale" : "corner, rigid", g, 600, 3, ws, ws);
    }
    fails += solver_refusals(g);
    printf(fails ? "FAILED %d\n" : "all equal\n", fails);
    return fails != 0;
}
