// mesh_sparse_check.cpp -- the brick-sparse TSDF volume of csrc/pm_tsdf_sparse.hpp replayed on the host, thread by thread in a
// scrambled order, through the header's own __host__ __device__ code: the marking of mpmvs_tsdf_allocate per pixel, the scan and the
// commit (rank, move, grid and list) per grid cell and per brick entry, the integration per brick (tsdf_brick_live, then the
// per-voxel body) and the mesh's corner tile, mark, vertices and triangles per brick entry; the scans are plain loops laid out as the kernels lay
// them out.  Launch order and buffer sizes are those of mpmvs_mesh.hip.  Against them stand the statements A and B of
// include/mpmvs.h written out below on their own: A as a plain loop over pixels and samples into a std::set, B as the dense loops
// over the virtual lattice with non-existing voxels zeroed, the vertices in a std::map keyed by (brick-major owner, slot).
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_sparse_check tools/mesh_sparse_check.cpp && build/mesh_sparse_check
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
#include <set>
#include <vector>

#include "pm_tsdf_sparse.hpp"
using namespace pm;

static unsigned order512[512];   // the order in which the threads of a block run
static bool nblk_rev = false;    // the blocks in descending order
static int failures = 0;

struct Cam { float K[9], R[9], t[3]; int w, h; std::vector<float> depth; std::vector<unsigned char> color; };

// the virtual lattice, dense on the host: what statement B is stated on
struct Lattice {
    int n[3];
    float origin[3], voxel, trunc, pad;
    std::vector<float> sum;
    std::vector<int32_t> weight;
    std::vector<uint32_t> color;   // 4 per voxel, or empty
    size_t size() const { return (size_t)n[0] * n[1] * n[2]; }
    size_t lin(int i, int j, int k) const { return ((size_t)k * n[1] + j) * n[0] + i; }
    float pos(int a, int i) const { return (float)((double)origin[a] + (double)i * (double)voxel); }
    int b(int a) const { return (n[a] + 7) / 8; }
    int brick_of(int i, int j, int k) const { return ((k >> 3) * b(1) + (j >> 3)) * b(0) + (i >> 3); }
    TsdfVol vol() const {
        TsdfVol V;
        V.nx = n[0]; V.ny = n[1]; V.nz = n[2]; V.trunc = trunc;
        for (int a = 0; a < 3; ++a) V.o[a] = (double)origin[a];
        V.voxel = (double)voxel;
        return V;
    }
};

// ---- statement A, plainly ---------------------------------------------------------------------------------------------------
static void plain_allocate(const Lattice& L, const std::vector<Cam>& cams, std::set<int>& bricks) {
    const int n_s = std::max(1, (int)std::ceil(4.0 * (double)L.trunc / (double)L.voxel));
    for (const Cam& c : cams)
        for (int iy = 0; iy < c.h; ++iy)
            for (int ix = 0; ix < c.w; ++ix) {
                const float d = c.depth[(size_t)iy * c.w + ix];
                if (!(std::isfinite(d) && d > 0.0f)) continue;
                for (int m = 0; m <= n_s; ++m) {
                    const float z = (float)(((double)d - (double)L.trunc) + (double)m * ((2.0 * (double)L.trunc) / (double)n_s));
                    if (!(z > 0.0f)) continue;
                    const float xc = (((float)ix - c.K[2]) * z) / c.K[0], yc = (((float)iy - c.K[5]) * z) / c.K[4];
                    const float a = xc - c.t[0], b = yc - c.t[1], cc = z - c.t[2];
                    const float P[3] = {(c.R[0] * a + c.R[3] * b) + c.R[6] * cc, (c.R[1] * a + c.R[4] * b) + c.R[7] * cc, (c.R[2] * a + c.R[5] * b) + c.R[8] * cc};
                    double lo[3], hi[3];   // integer-valued floats are exact in a double
                    bool skip = false;
                    for (int q = 0; q < 3; ++q) {
                        const float g = (P[q] - L.origin[q]) / L.voxel;
                        if (!std::isfinite(g)) { skip = true; continue; }
                        lo[q] = (double)std::floor(g - L.pad);
                        hi[q] = (double)std::floor(g + L.pad);
                        if (hi[q] < 0.0 || lo[q] > (double)(L.n[q] - 1)) skip = true;
                    }
                    if (skip) continue;
                    int l[3], h[3];
                    for (int q = 0; q < 3; ++q) {
                        l[q] = (int)std::min(std::max(lo[q], 0.0), (double)(L.n[q] - 1)) >> 3;
                        h[q] = (int)std::min(std::max(hi[q], 0.0), (double)(L.n[q] - 1)) >> 3;
                    }
                    for (int K = l[2]; K <= h[2]; ++K)
                        for (int J = l[1]; J <= h[1]; ++J)
                            for (int I = l[0]; I <= h[0]; ++I) bricks.insert((K * L.b(1) + J) * L.b(0) + I);
                }
            }
}

// ---- statement B, integration: the dense eleven steps on the voxels that exist ---------------------------------------------
static void plain_integrate(Lattice& L, const std::set<int>& bricks, const std::vector<Cam>& cams, int channels) {
    for (int k = 0; k < L.n[2]; ++k)
        for (int j = 0; j < L.n[1]; ++j)
            for (int i = 0; i < L.n[0]; ++i) {
                if (!bricks.count(L.brick_of(i, j, k))) continue;
                const size_t vox = L.lin(i, j, k);
                const float px = L.pos(0, i), py = L.pos(1, j), pz = L.pos(2, k);
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
                    if (s < -L.trunc) continue;
                    L.sum[vox] += std::fmin(1.0f, s / L.trunc);
                    L.weight[vox] += 1;
                    if (channels && s <= L.trunc) {
                        for (int ch = 0; ch < 3; ++ch) L.color[4 * vox + ch] += c.color[((size_t)iy * c.w + ix) * channels + (channels == 3 ? ch : 0)];
                        L.color[4 * vox + 3] += 1;
                    }
                }
            }
}

// ---- statement B, mesh: the dense statement with non-existing voxels at weight 0, in brick-major order -----------------------
struct Mesh {
    std::vector<float> xyz;
    std::vector<unsigned char> rgb;
    std::vector<int32_t> tri;
};
static const int kSlots[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};

static void plain_mesh(const Lattice& L, const std::set<int>& bricks, int min_weight, Mesh& r) {
    r = Mesh();
    std::map<int, long long> rank;
    for (int g : bricks) { const long long k = (long long)rank.size(); rank[g] = k; }
    auto exists = [&](const std::array<int, 3>& c) { return bricks.count(L.brick_of(c[0], c[1], c[2])) != 0; };
    auto valid = [&](const std::array<int, 3>& c) { return exists(c) && L.weight[L.lin(c[0], c[1], c[2])] >= min_weight; };
    auto value = [&](const std::array<int, 3>& c) { return L.sum[L.lin(c[0], c[1], c[2])] / (float)L.weight[L.lin(c[0], c[1], c[2])]; };
    auto major = [&](const std::array<int, 3>& c) { return rank[L.brick_of(c[0], c[1], c[2])] * 512 + (((c[2] & 7) * 8 + (c[1] & 7)) * 8 + (c[0] & 7)); };
    struct Key { long long owner; int slot; std::array<int, 3> at; bool operator<(const Key& o) const { return owner != o.owner ? owner < o.owner : slot < o.slot; } };
    std::vector<std::array<Key, 3>> tris;
    int perm[3] = {0, 1, 2};
    std::vector<std::array<int, 3>> perms;
    do perms.push_back({perm[0], perm[1], perm[2]}); while (std::next_permutation(perm, perm + 3));
    for (int g : bricks) {   // ascending
        const int I = g % L.b(0), J = (g / L.b(0)) % L.b(1), K = g / (L.b(0) * L.b(1));
        for (int local = 0; local < 512; ++local) {
            const int i = 8 * I + (local & 7), j = 8 * J + ((local >> 3) & 7), k = 8 * K + (local >> 6);
            if (!(i + 1 < L.n[0] && j + 1 < L.n[1] && k + 1 < L.n[2])) continue;
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
                        keys[e] = Key{major(c[lo]), slot, c[lo]};
                        for (int a = 0; a < 3; ++a) P[e][a] = 0.5 * ((double)c[lo][a] + (double)c[hi][a]);
                    }
                    double u[3], w[3];
                    for (int a = 0; a < 3; ++a) { u[a] = P[1][a] - P[0][a]; w[a] = P[2][a] - P[0][a]; }
                    const double nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                    double dot = 0.0;
                    for (int a = 0; a < 3; ++a) dot += nrm[a] * (mout[a] - min_[a]);
                    if (dot < 0.0) std::swap(keys[1], keys[2]);
                    tris.push_back(keys);
                }
            }
        }
    }
    std::map<Key, int32_t> number;
    for (const auto& t : tris) for (const Key& k : t) number[k] = 0;
    int32_t next = 0;
    for (auto& kv : number) kv.second = next++;
    for (const auto& t : tris) for (const Key& k : t) r.tri.push_back(number[k]);
    for (const auto& kv : number) {
        const std::array<int, 3>& ia = kv.first.at;
        const int* off = kSlots[kv.first.slot];
        const size_t A = L.lin(ia[0], ia[1], ia[2]), B = L.lin(ia[0] + off[0], ia[1] + off[1], ia[2] + off[2]);
        const float fa = L.sum[A] / (float)L.weight[A], fb = L.sum[B] / (float)L.weight[B];
        const float t = fa / (fa - fb);
        for (int a = 0; a < 3; ++a) {
            const float pa = L.pos(a, ia[a]), pb = L.pos(a, ia[a] + off[a]);
            r.xyz.push_back(pa + t * (pb - pa));
        }
        if (!L.color.empty()) {
            const uint32_t *ca = &L.color[4 * A], *cb = &L.color[4 * B];
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

// ---- the handle of mpmvs_mesh.hip, on the host ---------------------------------------------------------------------------------
struct Handle {
    TsdfVol V;
    TsdfAlloc S;
    int bx, by, bz, n_grid;
    bool with_color;
    std::vector<int32_t> grid, list;      // exact sizes: AddressSanitizer sees any index outside them
    std::vector<float> sum;
    std::vector<int32_t> weight;
    std::vector<uint4> color;
    long long n_bricks() const { return (long long)list.size(); }
    TsdfBricks bricks() const { return TsdfBricks{bx, by, bz, grid.data(), list.data()}; }
};

static Handle make_handle(const Lattice& L, bool with_color) {
    Handle h;
    h.V = L.vol();
    h.bx = L.b(0); h.by = L.b(1); h.bz = L.b(2);
    h.n_grid = h.bx * h.by * h.bz;
    h.with_color = with_color;
    h.grid.assign((size_t)h.n_grid, -1);
    h.S.n_s = std::max(1, (int)std::ceil(4.0 * (double)L.trunc / (double)L.voxel));
    h.S.step = (2.0 * (double)L.trunc) / (double)h.S.n_s;
    for (int a = 0; a < 3; ++a) h.S.origin[a] = L.origin[a];
    h.S.voxel = L.voxel;
    h.S.pad = L.pad;
    return h;
}

static void fill_views(const Handle& h, const std::vector<Cam>& cams, size_t v0, int channels, TsdfChunkArgs& A) {
    float pmax = 0.0f;
    const int last[3] = {h.V.nx - 1, h.V.ny - 1, h.V.nz - 1};
    for (int a = 0; a < 3; ++a) pmax = std::max(pmax, std::max(std::fabs(tsdf_pos(h.V, a, 0)), std::fabs(tsdf_pos(h.V, a, last[a]))));
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
}

// what mpmvs_tsdf_allocate does; false = refused at max_bricks (nothing changed)
static bool gpu_like_allocate(Handle& h, const std::vector<Cam>& cams, long long max_bricks) {
    std::vector<uint32_t> flags((size_t)h.n_grid, 0u);
    for (size_t v0 = 0; v0 < cams.size(); v0 += kTsdfChunk) {
        TsdfChunkArgs A;
        fill_views(h, cams, v0, 0, A);
        for (int q_ = 0; q_ < A.n; ++q_) {   // blockIdx.y
            const int q = nblk_rev ? A.n - 1 - q_ : q_;
            const size_t pixels = (size_t)A.v[q].w * A.v[q].h, blocks = (pixels + 255) / 256;
            for (size_t b_ = 0; b_ < blocks; ++b_)
                for (unsigned t_ = 0; t_ < 512; ++t_) {
                    if (order512[t_] >= 256) continue;
                    const size_t pix = (nblk_rev ? blocks - 1 - b_ : b_) * 256 + order512[t_];
                    if (pix < pixels) tsdf_alloc_mark_one(h.V, h.bricks(), h.S, A.v[q], (int)(pix % A.v[q].w), (int)(pix / A.v[q].w), flags.data());
                }
        }
    }
    const int n_tiles = (h.n_grid + kScanBlock - 1) / kScanBlock;
    std::vector<int> excl((size_t)h.n_grid, -7), totals((size_t)n_tiles, -7);
    long long n_new = 0;
    for (int b = 0; b < n_tiles; ++b) {   // k_tsdf_brick_scan
        int run = 0;
        for (int g = b * kScanBlock; g < std::min(h.n_grid, (b + 1) * kScanBlock); ++g) { excl[g] = run; run += (h.grid[g] >= 0 || flags[g]) ? 1 : 0; }
        totals[b] = run;
    }
    for (int b = 0, run = 0; b < n_tiles; ++b) { const int c = totals[b]; totals[b] = run; run += c; n_new = run; }   // k_scan_totals<Sum>
    if (n_new > max_bricks) return false;
    if (n_new == h.n_bricks()) return true;
    std::vector<float> sum((size_t)n_new * 512, 0.0f);
    std::vector<int32_t> weight((size_t)n_new * 512, 0), list((size_t)n_new, -7);
    std::vector<uint4> color(h.with_color ? (size_t)n_new * 512 : 0, make_uint4(0, 0, 0, 0));
    for (long long r_ = 0; r_ < h.n_bricks(); ++r_)   // k_tsdf_brick_move
        for (unsigned t_ = 0; t_ < 512; ++t_)
            tsdf_brick_move_one((int)(nblk_rev ? h.n_bricks() - 1 - r_ : r_), (int)order512[t_], h.list.data(), h.grid.data(), flags.data(), excl.data(), totals.data(),
                                h.sum.data(), h.weight.data(), h.with_color ? h.color.data() : nullptr, sum.data(), weight.data(), h.with_color ? color.data() : nullptr);
    for (int g_ = 0; g_ < h.n_grid; ++g_)   // k_tsdf_brick_commit
        tsdf_brick_commit_one(nblk_rev ? h.n_grid - 1 - g_ : g_, h.grid.data(), flags.data(), excl.data(), totals.data(), list.data());
    h.sum.swap(sum); h.weight.swap(weight); h.color.swap(color); h.list.swap(list);
    return true;
}

static long long culled = 0;   // (brick, view) pairs the block test skipped
static void gpu_like_integrate(Handle& h, const std::vector<Cam>& cams, int channels) {
    if (h.n_bricks() == 0) return;
    for (size_t v0 = 0; v0 < cams.size(); v0 += kTsdfChunk) {
        TsdfChunkArgs A;
        fill_views(h, cams, v0, channels, A);
        for (long long r_ = 0; r_ < h.n_bricks(); ++r_) {
            const int r = (int)(nblk_rev ? h.n_bricks() - 1 - r_ : r_);
            int I, J, K;
            tsdf_brick_coords(h.bricks(), h.list[(size_t)r], I, J, K);
            unsigned live = 0u;
            for (int t = 0; t < A.n; ++t)
                if (tsdf_brick_live(h.V, A.v[t], I, J, K)) live |= 1u << t;
            culled += A.n - __builtin_popcount(live);
            if (!live) continue;
            for (unsigned t_ = 0; t_ < 512; ++t_)
                tsdf_sparse_integrate_one(h.V, A, live, r, I, J, K, (int)order512[t_], h.sum.data(), h.weight.data(), h.with_color ? h.color.data() : nullptr);
        }
    }
}

// a block: the neighbour table, then (with_tile) the corner tile entry by entry in the scrambled order, then the threads
#define REPLAY_BRICKS(with_tile, call)                                                 \
    for (long long r_ = 0; r_ < h.n_bricks(); ++r_) {                                  \
        int I, J, K, nb[8];                                                            \
        tsdf_brick_coords(h.bricks(), h.list[(size_t)(nblk_rev ? h.n_bricks() - 1 - r_ : r_)], I, J, K); \
        for (int c = 0; c < 8; ++c) tsdf_brick_resolve(h.bricks(), I, J, K, c, nb);    \
        std::vector<float> tile_f(with_tile ? kBrickTile : 0, -7.0f);                  \
        std::vector<unsigned char> tile_v(with_tile ? kBrickTile : 0, 7);              \
        if (with_tile)                                                                 \
            for (int round = 0; round < 2; ++round)                                    \
                for (unsigned t_ = 0; t_ < 512; ++t_) {                                \
                    const int c = (int)order512[t_] + 512 * round;                     \
                    if (c < kBrickTile) tsdf_tile_load_one(nb, c, h.sum.data(), h.weight.data(), min_weight, tile_f.data(), tile_v.data()); \
                }                                                                      \
        for (unsigned t_ = 0; t_ < 512; ++t_) {                                        \
            const int local = (int)order512[t_];                                       \
            call;                                                                      \
        }                                                                              \
    }

static void gpu_like_mesh(const Handle& h, int min_weight, Mesh& r) {
    r = Mesh();
    if (h.V.nx < 2 || h.V.ny < 2 || h.V.nz < 2 || h.n_bricks() == 0) return;
    const size_t n = (size_t)h.n_bricks() * 512, n_tiles = (n + kScanBlock - 1) / kScanBlock;
    std::vector<uint32_t> mask(n, 0u);
    std::vector<int> vexcl(n, -7), tcount(n, -7), totals(2 * n_tiles, -7);
    REPLAY_BRICKS(true, tsdf_sparse_mark_one(h.V, nb, I, J, K, local, tile_f.data(), tile_v.data(), mask.data(), tcount.data()));
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
    const uint4* color = h.with_color ? h.color.data() : nullptr;
    r.xyz.assign(3 * (size_t)grand[0], -7.0f);
    if (color) r.rgb.assign(3 * (size_t)grand[0], 7);
    r.tri.assign(3 * (size_t)grand[1], -7);
    REPLAY_BRICKS(false, tsdf_sparse_vertex_one(h.V, nb, I, J, K, local, h.sum.data(), h.weight.data(), color, mask.data(), vexcl.data(), totals.data(), r.xyz.data(),
                                                color ? r.rgb.data() : nullptr));
    REPLAY_BRICKS(true, tsdf_sparse_triangle_one(h.V, nb, I, J, K, local, tile_f.data(), tile_v.data(), mask.data(), vexcl.data(), totals.data(), tcount.data(),
                                                 totals.data() + n_tiles, r.tri.data()));
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

// the handle's pool against the lattice: every existing voxel equal in every bit, every cut-off entry 0
static bool same_volume(const Handle& h, const Lattice& L, const std::set<int>& bricks) {
    if (std::vector<int32_t>(bricks.begin(), bricks.end()) != h.list) return false;
    for (size_t r = 0; r < h.list.size(); ++r) {
        if (h.grid[(size_t)h.list[r]] != (int32_t)r) return false;
        int I, J, K;
        tsdf_brick_coords(h.bricks(), h.list[r], I, J, K);
        for (int local = 0; local < 512; ++local) {
            const int i = 8 * I + (local & 7), j = 8 * J + ((local >> 3) & 7), k = 8 * K + (local >> 6);
            const size_t e = r * 512 + (size_t)local;
            float s = 0.0f; int32_t w = 0; uint32_t c[4] = {0, 0, 0, 0};
            if (i < L.n[0] && j < L.n[1] && k < L.n[2]) {
                s = L.sum[L.lin(i, j, k)]; w = L.weight[L.lin(i, j, k)];
                if (h.with_color) std::memcpy(c, &L.color[4 * L.lin(i, j, k)], 16);
            }
            if (std::memcmp(&s, &h.sum[e], 4) != 0 || w != h.weight[e]) return false;
            if (h.with_color && std::memcmp(c, &h.color[e], 16) != 0) return false;
        }
    }
    long long present = 0;
    for (int32_t g : h.grid) present += g >= 0;
    return present == h.n_bricks();
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
    for (float& d : c.depth) {   // a wall with bumps, and the depths that take no part
        const unsigned pick = rng() % 16;
        d = pick == 0 ? 0.0f : pick == 1 ? -1.0f : pick == 2 ? NAN : pick == 3 ? INFINITY : 3.6f + 0.9f * U(rng);
    }
    c.color.resize((size_t)w * h * (channels ? channels : 1));
    for (unsigned char& x : c.color) x = (unsigned char)(rng() & 255);
    return c;
}

// allocate (in two calls), integrate (all views, then again after a later allocate), mesh: every stage against its statement
static void run_pipeline(const char* name, int nx, int ny, int nz, float pad, int channels, int n_views, std::mt19937& rng) {
    Lattice L;
    L.n[0] = nx; L.n[1] = ny; L.n[2] = nz;
    L.origin[0] = -1.3f; L.origin[1] = -0.7f; L.origin[2] = 3.1f; L.voxel = 0.21f; L.trunc = 0.45f; L.pad = pad;
    std::vector<Cam> cams;
    for (int q = 0; q < n_views; ++q) {
        const float C[3] = {0.3f * (float)(q % 3) - 0.2f, 0.1f * (float)q, q % 4 == 3 ? 4.0f : -0.5f};   // every fourth camera sits inside the volume
        cams.push_back(make_cam(20 + 4 * (q % 3), 16 + 3 * (q % 2), 14.0f + (float)q, C, 0.05f * (float)q, q % 5 == 4 ? -1.0f : 1.0f, channels, rng));
    }
    const std::vector<Cam> head(cams.begin(), cams.begin() + n_views / 2), tail(cams.begin() + n_views / 2, cams.end());
    for (int variant = 0; variant < 2; ++variant) {
        nblk_rev = variant & 1;
        L.sum.assign(L.size(), 0.0f); L.weight.assign(L.size(), 0);
        L.color.assign(channels ? 4 * L.size() : 0, 0u);
        Handle h = make_handle(L, channels != 0);
        std::set<int> b1, b2;
        plain_allocate(L, head, b1);
        b2 = b1;
        plain_allocate(L, tail, b2);
        bool ok = gpu_like_allocate(h, head, 1 << 21) && same_volume(h, L, b1);
        ok = ok && gpu_like_allocate(h, head, (long long)b1.size()) && same_volume(h, L, b1);   // the same views: no change, and exactly at the cap
        plain_integrate(L, b1, head, channels);
        gpu_like_integrate(h, head, channels);
        ok = ok && same_volume(h, L, b1);
        if (b2.size() > b1.size()) {
            ok = ok && !gpu_like_allocate(h, cams, (long long)b2.size() - 1) && same_volume(h, L, b1);   // refused: nothing changed
        }
        ok = ok && gpu_like_allocate(h, cams, (long long)b2.size()) && same_volume(h, L, b2);           // old bricks moved, new ones zero
        plain_integrate(L, b2, tail, channels);
        gpu_like_integrate(h, tail, channels);
        ok = ok && same_volume(h, L, b2);
        long long observed = 0;
        for (int32_t w : L.weight) observed += w;
        Mesh want, got;
        size_t tris = 0;
        for (int mw = 1; mw <= 2; ++mw) {
            plain_mesh(L, b2, mw, want);
            gpu_like_mesh(h, mw, got);
            ok = ok && same(got.xyz, want.xyz) && same(got.rgb, want.rgb) && same(got.tri, want.tri);
            if (mw == 1) tris = want.tri.size() / 3;
        }
        if (!ok) { printf("%s, variant %d: DIFFERS\n", name, variant); ++failures; }
        if (variant == 1)
            printf("%-34s %3d x %3d x %3d pad %.1f %2d views %d ch: bricks %3zu -> %3zu of %3d, %7lld observations, %5zu triangles, %lld (brick, view) pairs culled\n",
                   name, nx, ny, nz, pad, n_views, channels, b1.size(), b2.size(), h.n_grid, observed, tris, culled);
    }
    culled = 0;
}

// the mesh alone, on a volume set brick by brick (mpmvs_tsdf_set_bricks): a sphere on the lattice, some bricks missing
static void run_mesh(const char* name, int nx, int ny, int nz, double cx, double cy, double cz, double rad, bool color, const std::vector<int>& missing, std::mt19937& rng,
                     long long want_tris = -1) {
    Lattice L;
    L.n[0] = nx; L.n[1] = ny; L.n[2] = nz;
    L.origin[0] = 0.25f; L.origin[1] = -1.5f; L.origin[2] = 3.0f; L.voxel = 0.375f; L.trunc = 1.0f; L.pad = 1.0f;
    L.sum.resize(L.size()); L.weight.assign(L.size(), 1);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) L.sum[L.lin(i, j, k)] = (float)(std::sqrt((i - cx) * (i - cx) + (j - cy) * (j - cy) + (k - cz) * (k - cz)) - rad);
    for (size_t k = 0; k < L.size(); k += 37) L.weight[k] = (int32_t)(rng() % 3) - 1;   // -1, 0, 1: holes
    if (color) {
        L.color.resize(4 * L.size());
        for (size_t k = 0; k < L.size(); ++k) {
            const uint32_t cnt = rng() % 4;
            for (int c = 0; c < 3; ++c) L.color[4 * k + c] = cnt ? (rng() % 256) * cnt : 0;
            L.color[4 * k + 3] = cnt;
        }
    }
    std::set<int> bricks;
    for (int g = 0; g < L.b(0) * L.b(1) * L.b(2); ++g)
        if (!std::count(missing.begin(), missing.end(), g)) bricks.insert(g);
    Handle h = make_handle(L, color);
    h.list.assign(bricks.begin(), bricks.end());
    for (size_t r = 0; r < h.list.size(); ++r) h.grid[(size_t)h.list[r]] = (int32_t)r;
    h.sum.assign(h.list.size() * 512, 0.0f); h.weight.assign(h.list.size() * 512, 0);
    if (color) h.color.assign(h.list.size() * 512, make_uint4(0, 0, 0, 0));
    for (size_t r = 0; r < h.list.size(); ++r) {
        int I, J, K;
        tsdf_brick_coords(h.bricks(), h.list[r], I, J, K);
        for (int local = 0; local < 512; ++local) {
            const int i = 8 * I + (local & 7), j = 8 * J + ((local >> 3) & 7), k = 8 * K + (local >> 6);
            if (!(i < nx && j < ny && k < nz)) continue;
            h.sum[r * 512 + local] = L.sum[L.lin(i, j, k)];
            h.weight[r * 512 + local] = L.weight[L.lin(i, j, k)];
            if (color) std::memcpy(&h.color[r * 512 + local], &L.color[4 * L.lin(i, j, k)], 16);
        }
    }
    Mesh want, got;
    plain_mesh(L, bricks, 1, want);
    for (int variant = 0; variant < 2; ++variant) {
        nblk_rev = variant & 1;
        gpu_like_mesh(h, 1, got);
        if (!(same(got.xyz, want.xyz) && same(got.rgb, want.rgb) && same(got.tri, want.tri))) { printf("%s, variant %d: DIFFERS\n", name, variant); ++failures; }
    }
    if (want_tris >= 0 && (long long)want.tri.size() / 3 != want_tris) { printf("%s: %zu triangles, expected %lld\n", name, want.tri.size() / 3, want_tris); ++failures; }
    printf("%-34s %3d x %3d x %3d  bricks %3zu of %3d  V = %6zu  F = %6zu\n", name, nx, ny, nz, bricks.size(), h.n_grid, want.xyz.size() / 3, want.tri.size() / 3);
}

int main() {
    std::mt19937 rng(23);
    for (unsigned t = 0; t < 512; ++t) order512[t] = t;
    std::shuffle(order512, order512 + 512, rng);

    run_mesh("sphere across eight bricks", 17, 17, 9, 8.2, 7.9, 4.1, 3.7, true, {}, rng);
    run_mesh("... one brick missing", 17, 17, 9, 8.2, 7.9, 4.1, 3.7, true, {4}, rng);
    run_mesh("... the upper layer missing", 17, 17, 9, 8.2, 7.9, 4.1, 3.7, false, {9, 10, 11, 12, 13, 14, 15, 16, 17}, rng);
    run_mesh("a single brick, empty neighbours", 20, 20, 20, 4.2, 4.1, 3.9, 3.5, true, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26}, rng);
    run_mesh("13 x 7 x 5, bricks cut off", 13, 7, 5, 6.2, 3.1, 2.1, 1.6, true, {}, rng);
    run_mesh("130 x 129 x 2", 130, 129, 2, 64.5, 63.2, 0.4, 50.3, false, {}, rng);
    run_mesh("nz = 1", 10, 9, 1, 4.3, 3.9, 0.0, 2.7, false, {}, rng, 0);
    run_mesh("no brick", 10, 9, 8, 4.3, 3.9, 3.4, 2.7, false, {0, 1, 2, 3}, rng, 0);
    run_pipeline("pipeline 13 x 7 x 5", 13, 7, 5, 1.0f, 0, 5, rng);
    run_pipeline("pipeline 17 x 17 x 9, B G R", 17, 17, 9, 0.0f, 3, 11, rng);
    run_pipeline("pipeline 70 x 9 x 3, grey", 70, 9, 3, 1.0f, 1, 19, rng);
    run_pipeline("pipeline 40 x 33 x 26, pad 8", 40, 33, 26, 8.0f, 3, 6, rng);
    run_pipeline("pipeline 200 x 21 x 12", 200, 21, 12, 0.5f, 3, 16, rng);   // far wider than any camera sees
    if (failures) { printf("%d case(s) differ\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
