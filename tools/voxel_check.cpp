// voxel_check.cpp -- the voxel-grid downsampling of csrc/pm_voxel.hpp replayed on the host, thread by thread in a scrambled order,
// through the header's own __host__ __device__ code (the insert of pm_cloud.hpp, then first, flag, number, accumulate and finish
// per thread; the scan is a plain loop here), in the launch order of Clusters of csrc/pm_cluster_host.hpp, which mpmvs_cloud_voxel_downsample
// of mpmvs_cloud.hip runs, and with buffers of exactly their sizes, against the plain-loop statement of include/mpmvs.h written out below with std::map.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/voxel_check tools/voxel_check.cpp && build/voxel_check
// Prints one line per case and "all equal"; exit status 1 if an output differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "pm_voxel.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = (nblk_rev ? ((size_t)(count) + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_]; \
            if (i < (size_t)(count)) call;                                                   \
        }

struct Result {
    std::vector<float> xyz, nrm;
    std::vector<unsigned char> rgb;
    std::vector<int32_t> count, first, voxel_of;
};

static bool finite3(const float* p) { return cloud_finite(p[0]) && cloud_finite(p[1]) && cloud_finite(p[2]); }

static bool lowest(const std::vector<float>& x, float mn[3], long long& nf) {
    nf = 0;
    for (size_t i = 0; i < x.size() / 3; ++i) {
        if (!finite3(&x[3 * i])) continue;
        for (int a = 0; a < 3; ++a) mn[a] = nf ? std::min(mn[a], x[3 * i + a]) : x[3 * i + a];
        ++nf;
    }
    return nf > 0;
}

// the statement of include/mpmvs.h
static void plain(const std::vector<float>& x, const float* nrm, const unsigned char* rgb, float voxel, Result& r) {
    const size_t n = x.size() / 3;
    r = Result();
    r.voxel_of.assign(n, -1);
    float mn[3] = {0, 0, 0}; long long nf = 0;
    if (!lowest(x, mn, nf)) return;
    const double e = (double)voxel;
    double o[3]; for (int a = 0; a < 3; ++a) o[a] = (double)mn[a] - 0.5 * e;
    struct Vox { int v; std::array<double, 3> c; long long cnt, S[3], N[3], C[3]; int32_t first; };
    std::map<std::array<long long, 3>, int> cell_of;
    std::vector<Vox> vox;
    for (size_t i = 0; i < n; ++i) {
        if (!finite3(&x[3 * i])) continue;
        double t[3], c[3]; std::array<long long, 3> key;
        for (int a = 0; a < 3; ++a) { t[a] = ((double)x[3 * i + a] - o[a]) / e; c[a] = std::floor(t[a]); key[a] = (long long)c[a]; }
        auto it = cell_of.find(key);
        if (it == cell_of.end()) {
            it = cell_of.emplace(key, (int)vox.size()).first;
            Vox v{}; v.v = (int)vox.size(); v.c = {c[0], c[1], c[2]}; v.first = (int32_t)i;
            vox.push_back(v);
        }
        Vox& v = vox[it->second];
        r.voxel_of[i] = v.v;
        ++v.cnt;
        for (int a = 0; a < 3; ++a) v.S[a] += llrint((t[a] - c[a]) * 0x1p30);
        if (nrm && finite3(&nrm[3 * i]))
            for (int a = 0; a < 3; ++a) v.N[a] += llrint(std::max(-1.0, std::min(1.0, (double)nrm[3 * i + a])) * 0x1p30);
        if (rgb) for (int k = 0; k < 3; ++k) v.C[k] += rgb[3 * i + k];
    }
    for (const Vox& v : vox) {
        r.count.push_back((int32_t)v.cnt); r.first.push_back(v.first);
        for (int a = 0; a < 3; ++a) r.xyz.push_back((float)(o[a] + (v.c[a] + (double)v.S[a] / ((double)v.cnt * 0x1p30)) * e));
        if (nrm) {
            const double L = std::sqrt(((double)v.N[0] * (double)v.N[0] + (double)v.N[1] * (double)v.N[1]) + (double)v.N[2] * (double)v.N[2]);
            for (int a = 0; a < 3; ++a) r.nrm.push_back(L == 0.0 ? 0.0f : (float)((double)v.N[a] / L));
        }
        if (rgb) for (int k = 0; k < 3; ++k) r.rgb.push_back((unsigned char)((2 * v.C[k] + v.cnt) / (2 * v.cnt)));
    }
}

// what mpmvs_cloud_voxel_downsample does, with the kernels replayed
static void gpu_like(const std::vector<float>& x, const float* nrm, const unsigned char* rgb, float voxel, bool want_map, Result& r) {
    const size_t n = x.size() / 3;
    r = Result();
    if (want_map) r.voxel_of.assign(n, -7);
    float mn[3] = {0, 0, 0}; long long nf = 0;
    if (!lowest(x, mn, nf)) { if (want_map) r.voxel_of.assign(n, -1); return; }
    VoxelGrid g; voxel_origin(mn, voxel, g);
    const int lg = cloud_slots_log2(nf); const size_t slots = (size_t)1 << lg;
    // exact-size buffers: AddressSanitizer sees any index outside them
    std::vector<unsigned long long> keys(slots, kCloudEmpty); std::vector<int> cnt(slots, 0), slot_of(n), flag(n), num(n), vox_of_slot(slots, -1);
    std::vector<unsigned> first(slots, ~0u);
    REPLAY(n, cloud_insert_one(i, x.data(), g.o[0], g.o[1], g.o[2], g.e, (unsigned)(slots - 1), keys.data(), cnt.data(), slot_of.data()));
    REPLAY(n, voxel_first_one(i, slot_of.data(), first.data()));
    REPLAY(n, voxel_flag_one(i, slot_of.data(), first.data(), flag.data()));
    int m = 0; for (size_t i = 0; i < n; ++i) { num[i] = m; m += flag[i]; }
    if (m <= 0 || m > nf) { printf("m = %d of %lld finite points\n", m, nf); exit(4); }
    const size_t mv = (size_t)m;
    r.first.assign(mv, -1); r.count.assign(mv, -1); r.xyz.assign(3 * mv, 0.0f);
    if (nrm) r.nrm.assign(3 * mv, 0.0f);
    if (rgb) r.rgb.assign(3 * mv, 0);
    const size_t parts = 1 + (nrm ? 1 : 0) + (rgb ? 1 : 0);
    std::vector<unsigned long long> acc(parts * 3 * mv, 0);
    unsigned long long* S = acc.data(); unsigned long long* N = nrm ? acc.data() + 3 * mv : nullptr; unsigned long long* Cc = rgb ? acc.data() + 3 * mv * (nrm ? 2 : 1) : nullptr;
    REPLAY(n, voxel_number_one(i, flag.data(), num.data(), slot_of.data(), cnt.data(), vox_of_slot.data(), r.first.data(), r.count.data()));
    REPLAY(n, voxel_accumulate_one(i, x.data(), nrm, rgb, g, slot_of.data(), vox_of_slot.data(), S, N, Cc, want_map ? r.voxel_of.data() : nullptr));
    REPLAY(mv, voxel_finish_one(i, x.data(), r.first.data(), r.count.data(), g, S, N, Cc, r.xyz.data(), nrm ? r.nrm.data() : nullptr, rgb ? r.rgb.data() : nullptr));
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static int failures = 0;
static void run(const char* name, const std::vector<float>& x, const std::vector<float>* nrm, const std::vector<unsigned char>* rgb, float voxel) {
    Result want, got;
    plain(x, nrm ? nrm->data() : nullptr, rgb ? rgb->data() : nullptr, voxel, want);
    for (int variant = 0; variant < 4; ++variant) {
        const bool use_n = nrm && (variant & 1) == 0, use_c = rgb && (variant & 2) == 0, want_map = variant != 3;
        nblk_rev = variant & 1;
        gpu_like(x, use_n ? nrm->data() : nullptr, use_c ? rgb->data() : nullptr, voxel, want_map, got);
        const bool ok = same(got.xyz, want.xyz) && same(got.count, want.count) && same(got.first, want.first) && (!want_map || same(got.voxel_of, want.voxel_of)) &&
                        (!use_n || same(got.nrm, want.nrm)) && (!use_c || same(got.rgb, want.rgb));
        if (!ok) { printf("%s, variant %d: DIFFERS\n", name, variant); ++failures; }
    }
    printf("%-28s n = %7zu  m = %7zu  voxel = %g\n", name, x.size() / 3, want.count.size(), (double)voxel);
}

int main() {
    std::mt19937 rng(16);
    for (unsigned t = 0; t < 256; ++t) order256[t] = t;
    std::shuffle(order256, order256 + 256, rng);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);

    {   // the border lattice, at the origin and shifted
        for (float shift : {0.0f, 1000.25f}) {
            std::vector<float> x;
            const float mn = 2.0f + shift, vx = 0.25f;
            for (int axis = 0; axis < 3; ++axis)
                for (int k = 0; k < 6; ++k) {
                    const float b = mn + ((float)k + 0.5f) * vx;
                    for (float v : {b, std::nextafter(b, -INFINITY), std::nextafter(b, INFINITY)}) {
                        float p[3] = {mn, mn, mn}; p[axis] = v;
                        x.insert(x.end(), p, p + 3);
                    }
                }
            x.insert(x.end(), {mn, mn, mn});
            run(shift == 0.0f ? "border lattice" : "border lattice + 1000.25", x, nullptr, nullptr, vx);
        }
    }
    {   // a random cloud with everything in it
        const size_t n = 5000;
        std::vector<float> x(3 * n), nr(3 * n); std::vector<unsigned char> c(3 * n);
        for (size_t i = 0; i < 3 * n; ++i) { x[i] = 10.0f + 3.0f * U(rng); nr[i] = 2.4f * U(rng) - 1.2f; c[i] = (unsigned char)(rng() & 255); }
        for (size_t i = 0; i < 300; ++i) for (int a = 0; a < 3; ++a) x[3 * (1000 + i) + a] = x[3 * i + a];   // duplicates
        x[3 * 17] = NAN; x[3 * 18 + 1] = INFINITY; x[3 * 19 + 2] = -INFINITY; x[3 * 4999] = NAN;
        for (int a = 0; a < 3; ++a) x[3 * 20 + a] = 900.0f;   // far away
        nr[3 * 5 + 1] = NAN; nr[3 * 1005] = INFINITY;
        for (int a = 0; a < 3; ++a) { x[3 * 21 + a] = 500.0f; x[3 * 22 + a] = 500.0f; nr[3 * 22 + a] = -nr[3 * 21 + a]; }   // n, -n alone in a voxel
        for (int a = 0; a < 3; ++a) { c[3 * 21 + a] = 0; c[3 * 22 + a] = 1; }                                              // {0, 1} -> 1
        run("random cloud", x, &nr, &c, 0.2f);
        run("random cloud, fine", x, &nr, &c, 0.003f);
        run("random cloud, one voxel", x, &nr, &c, 4000.0f);
    }
    {   // 70 001 points in one voxel, then in 70 001 voxels; n = 1, 257, 0, all non-finite
        const size_t n = 70001;
        std::vector<float> x(3 * n), nr(3 * n, 0.577f); std::vector<unsigned char> c(3 * n, 200);
        for (size_t i = 0; i < 3 * n; ++i) x[i] = 5.0f + 0.01f * U(rng);
        run("70001 in one voxel", x, &nr, &c, 1.0f);
        for (size_t i = 0; i < n; ++i) { x[3 * i] = 1.0f + (float)(i % 300) / 256.0f; x[3 * i + 1] = 1.0f + (float)(i / 300) / 256.0f; x[3 * i + 2] = 1.5f; }
        run("70001 one-point voxels", x, &nr, &c, 1.0f / 512.0f);
        std::vector<float> one = {1.0f, -2.0f, 3.0f};
        run("n = 1", one, nullptr, nullptr, 0.1f);
        x.resize(3 * 257); nr.resize(3 * 257); c.resize(3 * 257);
        run("n = 257", x, &nr, &c, 1.0f / 64.0f);
        std::vector<float> none;
        run("n = 0", none, nullptr, nullptr, 0.1f);
        std::vector<float> bad = {NAN, 0, 0, 0, INFINITY, 0};
        run("all non-finite", bad, nullptr, nullptr, 0.1f);
    }
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
