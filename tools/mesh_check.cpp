// mesh_check.cpp -- the TSDF integration and the four marching-tetrahedra passes of csrc/pm_tsdf.hpp replayed on the host, thread by
// thread in a scrambled order, through the header's own __host__ __device__ code (the block test and the per-voxel body of the
// integration; mark, vertices and triangles per thread; the scans are plain loops here, laid out as the kernels lay them out), in the
// launch order of mpmvs_tsdf_integrate / mpmvs_tsdf_mesh of mpmvs_mesh.hip and with buffers of exactly their sizes, against the
// plain-loop statements of include/mpmvs.h written out below on their own: std::map for the vertices, the case rule and the midpoint
// rule evaluated in floating point per tetrahedron.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_check tools/mesh_check.cpp && build/mesh_check
// Prints one line per case and "all equal"; exit status 1 if an output differs in a bit, or if the anchor's counts are not
// 410 / 1224 / 816.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "pm_tsdf.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = (nblk_rev ? ((size_t)(count) + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_]; \
            if (i < (size_t)(count)) call;                                                   \
        }

struct Volume {
    int nx, ny, nz;
    float origin[3], voxel, trunc;
    std::vector<float> sum;
    std::vector<int32_t> weight;
    std::vector<uint32_t> color;   // 4 per voxel, or empty
    size_t n() const { return (size_t)nx * ny * nz; }
    TsdfVol vol() const {
        TsdfVol V;
        V.nx = nx; V.ny = ny; V.nz = nz; V.trunc = trunc;
        for (int a = 0; a < 3; ++a) V.o[a] = (double)origin[a];
        V.voxel = (double)voxel;
        return V;
    }
    float pos(int a, int i) const { return (float)((double)origin[a] + (double)i * (double)voxel); }
};

struct Mesh {
    std::vector<float> xyz;
    std::vector<unsigned char> rgb;
    std::vector<int32_t> tri;
};

// ---- the statement of mpmvs_tsdf_mesh ---------------------------------------------------------------------------------------
static const int kSlots[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};

static void plain_mesh(const Volume& v, int min_weight, Mesh& r) {
    r = Mesh();
    const int nx = v.nx, ny = v.ny, nz = v.nz;
    auto lin = [&](const std::array<int, 3>& c) { return ((size_t)c[2] * ny + c[1]) * nx + c[0]; };
    auto valid = [&](const std::array<int, 3>& c) { return v.weight[lin(c)] >= min_weight; };
    auto value = [&](const std::array<int, 3>& c) { return v.sum[lin(c)] / (float)v.weight[lin(c)]; };
    typedef std::pair<size_t, int> Key;   // owner, slot
    std::vector<std::array<Key, 3>> tris;
    int perm[3] = {0, 1, 2};
    std::vector<std::array<int, 3>> perms;
    do perms.push_back({perm[0], perm[1], perm[2]}); while (std::next_permutation(perm, perm + 3));
    for (int k = 0; k + 1 < nz; ++k)
        for (int j = 0; j + 1 < ny; ++j)
            for (int i = 0; i + 1 < nx; ++i)
                for (const auto& p : perms) {
                    std::array<int, 3> c[4];
                    c[0] = {i, j, k};
                    c[1] = c[0]; c[1][p[0]] += 1;
                    c[2] = c[1]; c[2][p[1]] += 1;
                    c[3] = {i + 1, j + 1, k + 1};
                    if (!(valid(c[0]) && valid(c[1]) && valid(c[2]) && valid(c[3]))) continue;
                    std::vector<int> in, out;
                    for (int q = 0; q < 4; ++q) (value(c[q]) < 0.0f ? in : out).push_back(q);
                    std::vector<std::array<std::pair<int, int>, 3>> list;
                    if (in.size() == 1) list.push_back({{{in[0], out[0]}, {in[0], out[1]}, {in[0], out[2]}}});
                    else if (in.size() == 3) list.push_back({{{in[0], out[0]}, {in[1], out[0]}, {in[2], out[0]}}});
                    else if (in.size() == 2) {
                        list.push_back({{{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}}});
                        list.push_back({{{in[0], out[0]}, {in[1], out[1]}, {in[1], out[0]}}});
                    }
                    double min_[3] = {0, 0, 0}, mout[3] = {0, 0, 0};
                    for (int q : in) for (int a = 0; a < 3; ++a) min_[a] += (double)c[q][a] / (double)in.size();
                    for (int q : out) for (int a = 0; a < 3; ++a) mout[a] += (double)c[q][a] / (double)out.size();
                    for (const auto& t : list) {
                        std::array<Key, 3> keys;
                        double P[3][3];
                        for (int e = 0; e < 3; ++e) {
                            const int lo = std::min(t[e].first, t[e].second), hi = std::max(t[e].first, t[e].second);
                            int slot = -1;
                            for (int s = 0; s < 7; ++s)
                                if (c[hi][0] - c[lo][0] == kSlots[s][0] && c[hi][1] - c[lo][1] == kSlots[s][1] && c[hi][2] - c[lo][2] == kSlots[s][2]) slot = s;
                            if (slot < 0) { printf("no slot\n"); exit(4); }
                            keys[e] = Key(lin(c[lo]), slot);
                            for (int a = 0; a < 3; ++a) P[e][a] = 0.5 * ((double)c[lo][a] + (double)c[hi][a]);
                        }
                        double u[3], w[3];
                        for (int a = 0; a < 3; ++a) { u[a] = P[1][a] - P[0][a]; w[a] = P[2][a] - P[0][a]; }
                        const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                        double dot = 0.0;
                        for (int a = 0; a < 3; ++a) dot += n[a] * (mout[a] - min_[a]);
                        if (dot < 0.0) std::swap(keys[1], keys[2]);
                        tris.push_back(keys);
                    }
                }
    std::map<Key, int32_t> number;
    for (const auto& t : tris) for (const Key& k : t) number[k] = 0;
    int32_t next = 0;
    for (auto& kv : number) kv.second = next++;
    for (const auto& t : tris) for (const Key& k : t) r.tri.push_back(number[k]);
    for (const auto& kv : number) {
        const size_t A = kv.first.first;
        const int ia[3] = {(int)(A % nx), (int)((A / nx) % ny), (int)(A / ((size_t)nx * ny))};
        const int* off = kSlots[kv.first.second];
        const size_t B = (((size_t)(ia[2] + off[2])) * ny + (ia[1] + off[1])) * nx + (ia[0] + off[0]);
        const float fa = v.sum[A] / (float)v.weight[A], fb = v.sum[B] / (float)v.weight[B];
        const float t = fa / (fa - fb);
        for (int a = 0; a < 3; ++a) {
            const float pa = v.pos(a, ia[a]), pb = v.pos(a, ia[a] + off[a]);
            r.xyz.push_back(pa + t * (pb - pa));
        }
        if (!v.color.empty()) {
            const uint32_t *ca = &v.color[4 * A], *cb = &v.color[4 * B];
            unsigned char out[3];
            for (int c = 0; c < 3; ++c) {
                float val = 128.0f;
                if (ca[3] > 0 && cb[3] > 0) {
                    const float ma = (float)ca[c] / (float)ca[3], mb = (float)cb[c] / (float)cb[3];
                    val = ma + t * (mb - ma);
                } else if (ca[3] > 0) val = (float)ca[c] / (float)ca[3];
                else if (cb[3] > 0) val = (float)cb[c] / (float)cb[3];
                out[2 - c] = (unsigned char)(int)(val + 0.5f);
            }
            r.rgb.insert(r.rgb.end(), out, out + 3);
        }
    }
}

// what mpmvs_tsdf_mesh does, with the kernels replayed
static void gpu_like_mesh(const Volume& v, int min_weight, Mesh& r) {
    r = Mesh();
    if (v.nx < 2 || v.ny < 2 || v.nz < 2) return;
    const TsdfVol V = v.vol();
    const size_t n = v.n(), n_tiles = (n + kScanBlock - 1) / kScanBlock;
    // exact-size buffers: AddressSanitizer sees any index outside them
    std::vector<uint32_t> mask(n, 0u);
    std::vector<int> vexcl(n, -7), tcount(n, -7), totals(2 * n_tiles, -7);
    REPLAY(n, tsdf_mark_one(V, i, v.sum.data(), v.weight.data(), min_weight, mask.data(), tcount.data()));
    long long grand[2] = {0, 0};
    for (size_t b = 0; b < n_tiles; ++b) {   // k_tsdf_scan_tiles
        int sv = 0, st = 0;
        for (size_t k = b * kScanBlock; k < std::min(n, (b + 1) * kScanBlock); ++k) {
            vexcl[k] = sv; sv += __builtin_popcount(mask[k]);
            const int c = tcount[k]; tcount[k] = st; st += c;
        }
        totals[b] = sv; totals[n_tiles + b] = st;
        grand[0] += sv; grand[1] += st;
    }
    for (int row = 0; row < 2; ++row) {      // k_scan_totals<Sum>
        int run = 0;
        for (size_t b = 0; b < n_tiles; ++b) { const int c = totals[row * n_tiles + b]; totals[row * n_tiles + b] = run; run += c; }
    }
    if (grand[1] == 0) {
        if (grand[0] != 0) { printf("vertices without a triangle\n"); exit(4); }
        return;
    }
    const uint4* color = v.color.empty() ? nullptr : (const uint4*)v.color.data();
    r.xyz.assign(3 * (size_t)grand[0], -7.0f);
    if (color) r.rgb.assign(3 * (size_t)grand[0], 7);
    r.tri.assign(3 * (size_t)grand[1], -7);
    REPLAY(n, tsdf_vertex_one(V, i, v.sum.data(), v.weight.data(), color, mask.data(), vexcl.data(), totals.data(), r.xyz.data(), color ? r.rgb.data() : nullptr));
    REPLAY(n, tsdf_triangle_one(V, i, v.sum.data(), v.weight.data(), min_weight, mask.data(), vexcl.data(), totals.data(), tcount.data(),
                                totals.data() + n_tiles, r.tri.data()));
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static int failures = 0;
static long long culled = 0;   // (tile, view) pairs the block test skipped

// V, E, F and "every half-edge has exactly one opposite"
static void topology(const Mesh& m, long long& nv, long long& ne, long long& nf, bool& closed) {
    std::map<std::pair<int, int>, int> half;
    std::set<std::pair<int, int>> und;
    for (size_t t = 0; t < m.tri.size() / 3; ++t)
        for (int e = 0; e < 3; ++e) {
            const int a = m.tri[3 * t + e], b = m.tri[3 * t + (e + 1) % 3];
            ++half[{a, b}];
            und.insert({std::min(a, b), std::max(a, b)});
        }
    closed = true;
    for (const auto& kv : half) closed = closed && kv.second == 1 && half.count({kv.first.second, kv.first.first}) == 1;
    nv = (long long)m.xyz.size() / 3; ne = (long long)und.size(); nf = (long long)m.tri.size() / 3;
}

static void run_mesh(const char* name, const Volume& v, int min_weight, bool want_closed = false, const long long* anchor = nullptr) {
    Mesh want, got;
    plain_mesh(v, min_weight, want);
    for (int variant = 0; variant < 2; ++variant) {
        nblk_rev = variant & 1;
        gpu_like_mesh(v, min_weight, got);
        if (!(same(got.xyz, want.xyz) && same(got.rgb, want.rgb) && same(got.tri, want.tri))) { printf("%s, variant %d: DIFFERS\n", name, variant); ++failures; }
    }
    long long nv, ne, nf; bool closed;
    topology(want, nv, ne, nf, closed);
    if (want_closed && !(closed && nv - ne + nf == 2)) { printf("%s: not a closed surface of genus 0\n", name); ++failures; }
    if (anchor && !(nv == anchor[0] && ne == anchor[1] && nf == anchor[2])) { printf("%s: the anchor's counts differ\n", name); ++failures; }
    printf("%-44s %3d x %3d x %3d  min_weight %d  V = %6lld  E = %6lld  F = %6lld  closed %d\n", name, v.nx, v.ny, v.nz, min_weight, nv, ne, nf, (int)closed);
}

static Volume sphere(int nx, int ny, int nz, double cx, double cy, double cz, double rad, bool color, std::mt19937& rng) {
    Volume v;
    v.nx = nx; v.ny = ny; v.nz = nz; v.origin[0] = v.origin[1] = v.origin[2] = 0.0f; v.voxel = 1.0f; v.trunc = 1.0f;
    v.sum.resize(v.n()); v.weight.assign(v.n(), 1);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                v.sum[((size_t)k * ny + j) * nx + i] = (float)(std::sqrt((i - cx) * (i - cx) + (j - cy) * (j - cy) + (k - cz) * (k - cz)) - rad);
    if (color) {
        v.color.resize(4 * v.n());
        for (size_t k = 0; k < v.n(); ++k) {
            const uint32_t cnt = rng() % 4;   // a quarter of the voxels has no colour
            for (int c = 0; c < 3; ++c) v.color[4 * k + c] = cnt ? (rng() % 256) * cnt : 0;
            v.color[4 * k + 3] = cnt;
        }
    }
    return v;
}

// ---- the statement of mpmvs_tsdf_integrate ------------------------------------------------------------------------------------
struct Cam { float K[9], R[9], t[3]; int w, h; std::vector<float> depth; std::vector<unsigned char> color; };

static void plain_integrate(Volume& v, const std::vector<Cam>& cams, int channels) {
    for (int k = 0; k < v.nz; ++k)
        for (int j = 0; j < v.ny; ++j)
            for (int i = 0; i < v.nx; ++i) {
                const size_t vox = ((size_t)k * v.ny + j) * v.nx + i;
                const float px = v.pos(0, i), py = v.pos(1, j), pz = v.pos(2, k);
                for (const Cam& c : cams) {
                    const float xc = ((c.R[0] * px + c.R[1] * py) + c.R[2] * pz) + c.t[0];
                    const float yc = ((c.R[3] * px + c.R[4] * py) + c.R[5] * pz) + c.t[1];
                    const float z = ((c.R[6] * px + c.R[7] * py) + c.R[8] * pz) + c.t[2];
                    if (!(z > 0.0f)) continue;
                    const float fu = (c.K[0] * xc) / z + c.K[2] + 0.5f, fv = (c.K[4] * yc) / z + c.K[5] + 0.5f;
                    if (!(fu >= 0.0f && fu < (float)c.w && fv >= 0.0f && fv < (float)c.h)) continue;
                    const int ix = (int)std::floor(fu), iy = (int)std::floor(fv);
                    const float d = c.depth[(size_t)iy * c.w + ix];
                    if (!(std::isfinite(d) && d > 0.0f)) continue;
                    const float s = d - z;
                    if (s < -v.trunc) continue;
                    v.sum[vox] += std::fmin(1.0f, s / v.trunc);
                    v.weight[vox] += 1;
                    if (channels && s <= v.trunc) {
                        for (int ch = 0; ch < 3; ++ch) v.color[4 * vox + ch] += c.color[((size_t)iy * c.w + ix) * channels + (channels == 3 ? ch : 0)];
                        v.color[4 * vox + 3] += 1;
                    }
                }
            }
}

// what mpmvs_tsdf_integrate does: chunks of kTsdfChunk views, per chunk the blocks of k_tsdf_integrate with their block test
static void gpu_like_integrate(Volume& v, const std::vector<Cam>& cams, int channels) {
    const TsdfVol V = v.vol();
    float pmax = 0.0f;
    const int last[3] = {v.nx - 1, v.ny - 1, v.nz - 1};
    for (int a = 0; a < 3; ++a) pmax = std::max(pmax, std::max(std::fabs(v.pos(a, 0)), std::fabs(v.pos(a, last[a]))));
    for (size_t v0 = 0; v0 < cams.size(); v0 += kTsdfChunk) {
        TsdfChunkArgs A;
        std::memset(&A, 0, sizeof A);
        A.n = (int)std::min(cams.size() - v0, (size_t)kTsdfChunk);
        A.channels = channels;
        for (int q = 0; q < A.n; ++q) {
            const Cam& c = cams[v0 + q];
            TsdfView& W = A.v[q];
            std::memcpy(W.R, c.R, sizeof W.R); std::memcpy(W.t, c.t, sizeof W.t);
            W.K0 = c.K[0]; W.K2 = c.K[2]; W.K4 = c.K[4]; W.K5 = c.K[5];
            W.w = c.w; W.h = c.h;
            W.cull = pmax <= kTsdfCullBound;
            for (float x : c.R) W.cull = W.cull && std::fabs(x) <= kTsdfCullBound;
            for (float x : {c.t[0], c.t[1], c.t[2], W.K0, W.K2, W.K4, W.K5}) W.cull = W.cull && std::fabs(x) <= kTsdfCullBound;
            W.depth = c.depth.data();
            W.color = channels ? c.color.data() : nullptr;
        }
        const int tiles_x = (v.nx + kTsdfTileX - 1) / kTsdfTileX, tiles_y = (v.ny + kTsdfTileY - 1) / kTsdfTileY;
        const size_t tiles = (size_t)tiles_x * tiles_y * v.nz;
        for (size_t b_ = 0; b_ < tiles; ++b_) {
            const size_t b = nblk_rev ? tiles - 1 - b_ : b_;
            const int i0 = (int)(b % tiles_x) * kTsdfTileX, j0 = (int)((b / tiles_x) % tiles_y) * kTsdfTileY, k = (int)(b / ((size_t)tiles_x * tiles_y));
            unsigned live = 0u;
            for (int t = 0; t < A.n; ++t)
                if (tsdf_view_live(V, A.v[t], i0, j0, k)) live |= 1u << t;
            culled += A.n - __builtin_popcount(live);
            if (!live) continue;
            for (unsigned t_ = 0; t_ < 256; ++t_) {
                const unsigned t = order256[t_];
                const int i = i0 + (int)(t & (kTsdfTileX - 1)), j = j0 + (int)(t / kTsdfTileX);
                if (i < v.nx && j < v.ny) tsdf_integrate_one(V, A, live, i, j, k, v.sum.data(), v.weight.data(), channels ? (uint4*)v.color.data() : nullptr);
            }
        }
    }
}

static Cam make_cam(int w, int h, float f, const float C[3], float yaw, float z_sign, int channels, std::mt19937& rng) {
    Cam c;
    const float cy = std::cos(yaw), sy = std::sin(yaw);
    const float R[9] = {cy, 0.0f, sy, 0.0f, 1.0f, 0.0f, -sy * z_sign, 0.0f, cy * z_sign};
    std::memcpy(c.R, R, sizeof R);
    for (int r = 0; r < 3; ++r) c.t[r] = -((c.R[3 * r] * C[0] + c.R[3 * r + 1] * C[1]) + c.R[3 * r + 2] * C[2]);
    const float K[9] = {f, 0.0f, 0.5f * w, 0.0f, f, 0.5f * h, 0.0f, 0.0f, 1.0f};
    std::memcpy(c.K, K, sizeof K);
    c.w = w; c.h = h;
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    c.depth.resize((size_t)w * h);
    for (float& d : c.depth) {
        const unsigned pick = rng() % 16;
        d = pick == 0 ? 0.0f : pick == 1 ? -1.0f : pick == 2 ? NAN : pick == 3 ? INFINITY : 3.0f + 4.0f * U(rng);
    }
    c.color.resize((size_t)w * h * (channels ? channels : 1));
    for (unsigned char& x : c.color) x = (unsigned char)(rng() & 255);
    return c;
}

static void run_integrate(const char* name, int nx, int ny, int nz, int channels, int n_views, std::mt19937& rng) {
    Volume want;
    want.nx = nx; want.ny = ny; want.nz = nz; want.origin[0] = -1.3f; want.origin[1] = -0.7f; want.origin[2] = 3.1f; want.voxel = 0.21f; want.trunc = 0.8f;
    want.sum.assign(want.n(), 0.0f); want.weight.assign(want.n(), 0);
    if (channels) want.color.assign(4 * want.n(), 0u);
    std::vector<Cam> cams;
    for (int q = 0; q < n_views; ++q) {
        const float C[3] = {0.3f * (float)(q % 3) - 0.2f, 0.1f * (float)q, q % 4 == 3 ? 4.0f : -0.5f};   // every fourth camera sits inside the volume
        cams.push_back(make_cam(20 + 4 * (q % 3), 16 + 3 * (q % 2), 14.0f + (float)q, C, 0.05f * (float)q, q % 5 == 4 ? -1.0f : 1.0f, channels, rng));
    }
    plain_integrate(want, cams, channels);
    long long touched = 0;
    for (int32_t w : want.weight) touched += w;
    for (int variant = 0; variant < 2; ++variant) {
        nblk_rev = variant & 1;
        Volume got = want;
        got.sum.assign(got.n(), 0.0f); got.weight.assign(got.n(), 0);
        if (channels) got.color.assign(4 * got.n(), 0u);
        if (variant == 0) gpu_like_integrate(got, cams, channels);
        else {   // two calls with the list split
            std::vector<Cam> a(cams.begin(), cams.begin() + n_views / 2), b(cams.begin() + n_views / 2, cams.end());
            gpu_like_integrate(got, a, channels);
            gpu_like_integrate(got, b, channels);
        }
        if (!(same(got.sum, want.sum) && same(got.weight, want.weight) && same(got.color, want.color))) { printf("%s, variant %d: DIFFERS\n", name, variant); ++failures; }
    }
    printf("%-44s %3d x %3d x %3d  %2d views, %d channel(s): %lld observations, %lld (tile, view) pairs skipped by the block test\n", name, nx, ny, nz, n_views,
           channels, touched, culled);
    culled = 0;
}

int main() {
    std::mt19937 rng(22);
    for (unsigned t = 0; t < 256; ++t) order256[t] = t;
    std::shuffle(order256, order256 + 256, rng);

    {   // the anchor of the contract
        const long long anchor[3] = {410, 1224, 816};
        Volume v = sphere(10, 9, 8, 4.3, 3.9, 3.4, 2.7, false, rng);
        run_mesh("sphere anchor", v, 1, true, anchor);
        Volume c = sphere(10, 9, 8, 4.3, 3.9, 3.4, 2.7, true, rng);
        run_mesh("sphere anchor, colours", c, 1, true, anchor);
    }
    {   // exact zeros on lattice points: radius 2 around (3, 3, 3)
        Volume v = sphere(7, 7, 7, 3.0, 3.0, 3.0, 2.0, true, rng);
        int zeros = 0;
        for (float f : v.sum) zeros += f == 0.0f;
        if (zeros != 6) { printf("expected 6 exact zeros, got %d\n", zeros); ++failures; }
        run_mesh("exact zeros on lattice points", v, 1, true);
    }
    {   // invalid corners punching holes
        Volume v = sphere(10, 9, 8, 4.3, 3.9, 3.4, 2.7, true, rng);
        for (int k = 2; k < 5; ++k) for (int j = 3; j < 6; ++j) for (int i = 5; i < 9; ++i) v.weight[((size_t)k * 9 + j) * 10 + i] = 0;
        v.weight[0] = -3;
        run_mesh("a block of corners at weight 0", v, 1);
    }
    {   // min_weight at, below and above a corner's weight; the sums scale with the weights so that f stays the sphere's
        Volume v = sphere(10, 9, 8, 4.3, 3.9, 3.4, 2.7, true, rng);
        for (size_t k = 0; k < v.n(); ++k) { v.weight[k] = 1 + (int32_t)(rng() % 3); v.sum[k] *= (float)v.weight[k]; }
        for (int mw = 1; mw <= 4; ++mw) run_mesh("mixed weights 1..3", v, mw);
    }
    {   // thin lattices: a dimension of 1 has no cell, of 2 one layer of cells
        for (int thin = 1; thin <= 2; ++thin)
            for (int axis = 0; axis < 3; ++axis) {
                int d[3] = {9, 8, 7};
                d[axis] = thin;
                Volume v = sphere(d[0], d[1], d[2], axis == 0 ? 0.4 : 4.3, axis == 1 ? 0.4 : 3.9, axis == 2 ? 0.4 : 3.4, 2.7, true, rng);
                char name[64];
                snprintf(name, sizeof name, "dimension %d of axis %d", thin, axis);
                run_mesh(name, v, 1);
            }
    }
    {   // 13 x 7 x 5: no dimension a multiple of a block; and lattices longer than a wave and than a scan tile
        Volume v = sphere(13, 7, 5, 6.2, 3.1, 2.1, 1.6, true, rng);
        run_mesh("13 x 7 x 5", v, 1, true);
        Volume w = sphere(70, 3, 3, 34.5, 1.2, 0.9, 30.3, true, rng);
        run_mesh("70 x 3 x 3", w, 1);
        Volume x = sphere(130, 129, 2, 64.5, 63.2, 0.4, 50.3, false, rng);
        run_mesh("130 x 129 x 2", x, 1);
        Volume none = sphere(6, 5, 4, 2.5, 2.5, 2.5, -1.0, false, rng);   // f > 0 everywhere
        run_mesh("constant sign", none, 1);
        std::fill(none.weight.begin(), none.weight.end(), 0);
        run_mesh("nothing valid", none, 1);
    }
    run_integrate("integrate 13 x 7 x 5, no colour", 13, 7, 5, 0, 5, rng);
    run_integrate("integrate 13 x 7 x 5, B G R", 13, 7, 5, 3, 11, rng);
    run_integrate("integrate 70 x 9 x 3, grey", 70, 9, 3, 1, 19, rng);
    run_integrate("integrate 200 x 21 x 4, B G R", 200, 21, 4, 3, 16, rng);   // far wider than any camera sees: most tiles are skipped
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
