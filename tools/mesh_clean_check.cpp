// mesh_clean_check.cpp -- the components, vertex normals and select of csrc/pm_mesh.hpp replayed on the host through the header's
// own __host__ __device__ code (mesh_cc_hook_one, cc_flatten_one, cc_count_one, mesh_tri_count_one, cc_gather_one;
// mesh_nrm_accum_one, mesh_nrm_finish_one; mesh_sel_vert_one, mesh_sel_tri_one, mesh_emit_vert_one, mesh_emit_tri_one), with
// buffers of exactly the sizes mpmvs_mesh.hip gives them, against plain loops written out below (statements 1 to 3 of
// include/mpmvs.h).  Every pass is replayed thread by thread in a scrambled order, the blocks ascending and descending.  The hook pass
// is also replayed
//   by edges    all unions (a, b) and (a, c) of all triangles are collected, shuffled and applied one by one through cc_union, the two
//               ends in either order: a replay by whole threads cannot interleave the unions of two threads, this one does.
// The invariant parent[x] <= x is asserted over the whole array after every union of the replay by edges and after every thread of
// the replay by threads; where that would take hours (more than 20 000 edges, more than 5000 vertices), after every 4096 edges,
// after every block of 256 threads, and at the end.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/mesh_clean_check tools/mesh_clean_check.cpp && build/mesh_clean_check
// Prints one line per case and "all equal"; exit status 1 on any difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "pm_mesh.hpp"
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

static int failures = 0;
static std::mt19937 rng(23);

struct Mesh {
    std::vector<float> xyz;
    std::vector<unsigned char> rgb;   // empty: no colour
    std::vector<int32_t> tri;
    size_t n() const { return xyz.size() / 3; }
    size_t m() const { return tri.size() / 3; }
};

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

// ---- statement 1, plainly: a sequential union-find whose root is the smallest index --------------------------------------------------
struct Components {
    std::vector<int32_t> label, verts, tris;
    long long counts[4];
};
static void plain_components(const Mesh& M, Components& r) {
    const size_t n = M.n(), m = M.m();
    std::vector<int> up(n);
    std::iota(up.begin(), up.end(), 0);
    auto root = [&](int x) { while (up[x] != x) x = up[x]; return x; };
    for (size_t t = 0; t < m; ++t)
        for (int k = 1; k < 3; ++k) {
            const int a = root(M.tri[3 * t]), b = root(M.tri[3 * t + k]);
            if (a != b) up[std::max(a, b)] = std::min(a, b);
        }
    r.label.resize(n); r.verts.assign(n, 0); r.tris.assign(n, 0);
    std::vector<int> nv(n, 0), nt(n, 0);
    std::vector<char> named(n, 0);
    for (size_t v = 0; v < n; ++v) { r.label[v] = root((int)v); ++nv[r.label[v]]; }
    for (size_t t = 0; t < m; ++t) {
        ++nt[r.label[M.tri[3 * t]]];
        for (int k = 0; k < 3; ++k) named[M.tri[3 * t + k]] = 1;
    }
    r.counts[0] = 0; r.counts[1] = 0; r.counts[2] = 0; r.counts[3] = -1;
    for (size_t v = 0; v < n; ++v) {
        r.verts[v] = nv[r.label[v]]; r.tris[v] = nt[r.label[v]];
        if (!named[v]) ++r.counts[1];
        if (r.label[v] == (int32_t)v && nt[v] > 0) {
            ++r.counts[0];
            if (nt[v] > r.counts[2]) { r.counts[2] = nt[v]; r.counts[3] = (long long)v; }
        }
    }
}

static bool invariant(const std::vector<int>& parent) {
    for (size_t x = 0; x < parent.size(); ++x)
        if (parent[x] < 0 || parent[x] > (int)x) return false;
    return true;
}

// what mpmvs_mesh_components does after the hook pass, with the kernels replayed; the counts as the host takes them
static void finish_components(const Mesh& M, std::vector<int>& parent, Components& r) {
    const size_t n = M.n(), m = M.m();
    r.label.assign(n, -7); r.verts.assign(n, -7); r.tris.assign(n, -7);
    std::vector<int> cnt(2 * n, 0);
    REPLAY(n, cc_flatten_one(i, parent.data(), r.label.data()));
    REPLAY(n, cc_count_one(i, r.label.data(), cnt.data()));
    REPLAY(m, mesh_tri_count_one(i, M.tri.data(), r.label.data(), cnt.data() + n));
    REPLAY(n, cc_gather_one(i, r.label.data(), cnt.data(), r.verts.data()));
    REPLAY(n, cc_gather_one(i, r.label.data(), cnt.data() + n, r.tris.data()));
    long long comps = 0, unnamed = 0, best = 0, best_label = -1;
    for (size_t v = 0; v < n; ++v) {
        if (r.tris[v] == 0) ++unnamed;
        if (r.label[v] != (int32_t)v || r.tris[v] == 0) continue;
        ++comps;
        if (r.tris[v] > best) best = r.tris[v], best_label = (long long)v;
    }
    r.counts[0] = comps; r.counts[1] = unnamed; r.counts[2] = best; r.counts[3] = best_label;
}
static bool same_components(const Components& a, const Components& b) {
    return same(a.label, b.label) && same(a.verts, b.verts) && same(a.tris, b.tris) && std::memcmp(a.counts, b.counts, sizeof a.counts) == 0;
}

static void components_by_threads(const Mesh& M, Components& r) {
    const size_t n = M.n(), m = M.m();
    std::vector<int> parent(n);
    std::iota(parent.begin(), parent.end(), 0);   // k_mesh_cc_init
    const bool every = n <= 5000;
    for (size_t b_ = 0; b_ < (m + 255) / 256; ++b_) {
        for (unsigned t_ = 0; t_ < 256; ++t_) {
            const size_t i = (nblk_rev ? (m + 255) / 256 - 1 - b_ : b_) * 256 + order256[t_];
            if (i >= m) continue;
            mesh_cc_hook_one(i, M.tri.data(), parent.data());
            if (every && !invariant(parent)) { printf("parent[x] <= x broken after thread %zu\n", i); exit(3); }
        }
        if (!invariant(parent)) { printf("parent[x] <= x broken after block %zu\n", b_); exit(3); }
    }
    finish_components(M, parent, r);
}

static void components_by_edges(const Mesh& M, Components& r) {
    const size_t n = M.n(), m = M.m();
    std::vector<std::pair<int, int>> edges;
    edges.reserve(2 * m);
    for (size_t t = 0; t < m; ++t)
        for (int k = 1; k < 3; ++k) edges.push_back(rng() & 1 ? std::make_pair(M.tri[3 * t], M.tri[3 * t + k]) : std::make_pair(M.tri[3 * t + k], M.tri[3 * t]));
    std::shuffle(edges.begin(), edges.end(), rng);
    std::vector<int> parent(n);
    std::iota(parent.begin(), parent.end(), 0);
    const bool every = edges.size() <= 20000 && n <= 5000;
    for (size_t e = 0; e < edges.size(); ++e) {
        cc_union(parent.data(), edges[e].first, edges[e].second);
        if ((every || e % 4096 == 4095) && !invariant(parent)) { printf("parent[x] <= x broken after edge %zu\n", e); exit(3); }
    }
    if (!invariant(parent)) { printf("parent[x] <= x broken at the end\n"); exit(3); }
    finish_components(M, parent, r);
}

// ---- statement 2, plainly --------------------------------------------------------------------------------------------------------------
static bool fin3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
static long long plain_normals(const Mesh& M, std::vector<float>& out) {
    const size_t n = M.n(), m = M.m();
    out.assign(3 * n, 0.0f);
    double lo[3], hi[3];
    bool any = false;
    for (size_t v = 0; v < n; ++v) {
        if (!fin3(&M.xyz[3 * v])) continue;
        for (int a = 0; a < 3; ++a) {
            const double x = (double)M.xyz[3 * v + a];
            lo[a] = any ? std::min(lo[a], x) : x;
            hi[a] = any ? std::max(hi[a], x) : x;
        }
        any = true;
    }
    double ext = 0.0;
    if (any)
        for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[a] - lo[a]);
    if (!any || ext == 0.0 || m == 0) return 0;
    const double B = 2.0 * (ext * ext);
    int e = 0, b = 0;
    while (std::ldexp(1.0, e) <= B) ++e;        // 2^(e-1) <= B < 2^e, found without frexp
    while (std::ldexp(1.0, e - 1) > B) --e;
    while (((size_t)1 << b) < std::max(m, (size_t)1)) ++b;
    const double scale = std::ldexp(1.0, 61 - b - e);
    std::vector<long long> S(3 * n, 0);
    for (size_t t = 0; t < m; ++t) {
        const int32_t* q = &M.tri[3 * t];
        if (!(fin3(&M.xyz[3 * q[0]]) && fin3(&M.xyz[3 * q[1]]) && fin3(&M.xyz[3 * q[2]]))) continue;
        double u[3], w[3];
        for (int a = 0; a < 3; ++a) {
            u[a] = (double)M.xyz[3 * q[1] + a] - (double)M.xyz[3 * q[0] + a];
            w[a] = (double)M.xyz[3 * q[2] + a] - (double)M.xyz[3 * q[0] + a];
        }
        const double C[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        for (int k = 0; k < 3; ++k) {
            const long long F = std::llrint(C[k] * scale);
            if (std::llabs(F) > (1ll << 61) / (long long)m) { printf("a term above 2^61 / m\n"); exit(5); }   // 2^(61-b) <= 2^61 / m
            for (int c = 0; c < 3; ++c) S[3 * q[c] + k] += F;
        }
    }
    long long defined = 0;
    for (size_t v = 0; v < n; ++v) {
        const double x = (double)S[3 * v], y = (double)S[3 * v + 1], z = (double)S[3 * v + 2];
        const double len = std::sqrt((x * x + y * y) + z * z);
        if (len == 0.0) continue;
        out[3 * v] = (float)(x / len); out[3 * v + 1] = (float)(y / len); out[3 * v + 2] = (float)(z / len);
        ++defined;
    }
    return defined;
}
static long long replay_normals(const Mesh& M, std::vector<float>& out) {
    const size_t n = M.n(), m = M.m();
    out.assign(3 * n, -7.0f);
    const double scale = mesh_scale(M.xyz.data(), (long long)n, (long long)m);
    if (n == 0 || scale == 0.0) { out.assign(3 * n, 0.0f); return 0; }
    std::vector<long long> S(3 * n, 0);
    REPLAY(m, mesh_nrm_accum_one(i, M.xyz.data(), M.tri.data(), scale, S.data()));
    long long defined = 0;
    REPLAY(n, defined += mesh_nrm_finish_one(i, S.data(), out.data()));
    return defined;
}

// ---- statement 3, plainly ---------------------------------------------------------------------------------------------------------------
struct Selected {
    std::vector<float> xyz;
    std::vector<unsigned char> rgb;
    std::vector<int32_t> tri, src;
};
static void plain_select(const Mesh& M, const std::vector<unsigned char>& keep, bool drop, Selected& r) {
    r = Selected();
    const size_t n = M.n(), m = M.m();
    std::vector<char> tk(m, 0), vk(n, 0);
    for (size_t t = 0; t < m; ++t) tk[t] = keep[M.tri[3 * t]] && keep[M.tri[3 * t + 1]] && keep[M.tri[3 * t + 2]];
    for (size_t v = 0; v < n; ++v) vk[v] = keep[v] != 0 && !drop;
    if (drop)
        for (size_t t = 0; t < m; ++t)
            if (tk[t])
                for (int k = 0; k < 3; ++k) vk[M.tri[3 * t + k]] = 1;
    std::vector<int32_t> renum(n, -1);
    for (size_t v = 0; v < n; ++v) {
        if (!vk[v]) continue;
        renum[v] = (int32_t)r.src.size();
        r.src.push_back((int32_t)v);
        for (int k = 0; k < 3; ++k) r.xyz.push_back(M.xyz[3 * v + k]);
        if (!M.rgb.empty())
            for (int k = 0; k < 3; ++k) r.rgb.push_back(M.rgb[3 * v + k]);
    }
    for (size_t t = 0; t < m; ++t)
        if (tk[t])
            for (int k = 0; k < 3; ++k) r.tri.push_back(renum[M.tri[3 * t + k]]);
}
// k_scan_tiles and k_scan_totals<Sum> as sums: excl[k] = the flags before k in its tile, tile[b] = the flags before tile b
static int replay_scan(const std::vector<int>& flag, std::vector<int>& excl, std::vector<int>& tile) {
    const size_t n = flag.size(), tiles = (n + kScanBlock - 1) / kScanBlock;
    excl.assign(n, -7); tile.assign(tiles, -7);
    int run = 0;
    for (size_t b = 0; b < tiles; ++b) {
        int s = 0;
        for (size_t k = b * kScanBlock; k < std::min(n, (b + 1) * kScanBlock); ++k) { excl[k] = s; s += flag[k]; }
        tile[b] = run; run += s;
    }
    return run;
}
static void replay_select(const Mesh& M, const std::vector<unsigned char>& keep, bool drop, Selected& r) {
    r = Selected();
    const size_t n = M.n(), m = M.m();
    if (n == 0 || (drop && m == 0)) return;
    std::vector<int> vflag(n, -7), tflag(m, -7), vexcl, texcl, vtile, ttile;
    REPLAY(n, mesh_sel_vert_one(i, keep.data(), drop, vflag.data()));
    REPLAY(m, mesh_sel_tri_one(i, M.tri.data(), keep.data(), drop, tflag.data(), vflag.data()));
    const size_t nv = (size_t)replay_scan(vflag, vexcl, vtile), nt = (size_t)replay_scan(tflag, texcl, ttile);
    if (nv == 0) return;
    r.xyz.assign(3 * nv, -7.0f); r.src.assign(nv, -7); r.tri.assign(3 * nt, -7);
    if (!M.rgb.empty()) r.rgb.assign(3 * nv, 7);
    REPLAY(n, mesh_emit_vert_one(i, M.xyz.data(), M.rgb.empty() ? nullptr : M.rgb.data(), vflag.data(), vexcl.data(), vtile.data(), r.xyz.data(), r.rgb.data(), r.src.data()));
    REPLAY(m, mesh_emit_tri_one(i, M.tri.data(), tflag.data(), texcl.data(), ttile.data(), vexcl.data(), vtile.data(), r.tri.data()));
}

// ---- a case -----------------------------------------------------------------------------------------------------------------------------
static void run_case(const char* name, const Mesh& M, bool select_too = true) {
    Components want, got;
    plain_components(M, want);
    std::vector<float> wn, gn;
    const long long wd = plain_normals(M, wn);
    bool ok = true;
    for (int variant = 0; variant < 2; ++variant) {
        nblk_rev = variant & 1;
        components_by_threads(M, got);
        ok = ok && same_components(got, want);
        components_by_edges(M, got);
        ok = ok && same_components(got, want);
        ok = ok && replay_normals(M, gn) == wd && same(gn, wn);
    }
    int selects = 0;
    if (select_too) {
        std::vector<unsigned char> keep(M.n());
        Selected ws, gs;
        for (int mask = 0; mask < 5; ++mask) {
            for (size_t v = 0; v < M.n(); ++v)
                keep[v] = mask == 0 ? 1 : mask == 1 ? 0 : mask == 2 ? (v % 2 == 0) * 3 : mask == 3 ? (rng() % 4 != 0) * 255 : want.label[v] != want.counts[3];
            for (int drop = 0; drop < 2; ++drop) {
                nblk_rev = (mask + drop) & 1;
                plain_select(M, keep, drop, ws);
                replay_select(M, keep, drop, gs);
                ok = ok && same(gs.xyz, ws.xyz) && same(gs.rgb, ws.rgb) && same(gs.tri, ws.tri) && same(gs.src, ws.src);
                ++selects;
            }
        }
    }
    if (!ok) { printf("%s: DIFFERS\n", name); ++failures; }
    printf("%-44s n = %7zu  m = %7zu  components %6lld  unnamed %6lld  largest %7lld (label %6lld)  normals %7lld  selects %d\n", name, M.n(), M.m(), want.counts[0],
           want.counts[1], want.counts[2], want.counts[3], wd, selects);
}

static Mesh renumber(const Mesh& M, const std::vector<int>& perm) {   // vertex v becomes perm[v]
    Mesh R = M;
    for (size_t v = 0; v < M.n(); ++v) {
        for (int k = 0; k < 3; ++k) R.xyz[3 * perm[v] + k] = M.xyz[3 * v + k];
        if (!M.rgb.empty())
            for (int k = 0; k < 3; ++k) R.rgb[3 * perm[v] + k] = M.rgb[3 * v + k];
    }
    for (size_t k = 0; k < M.tri.size(); ++k) R.tri[k] = perm[M.tri[k]];
    return R;
}
static Mesh strip(int k) {
    Mesh M;
    for (int v = 0; v < k + 2; ++v) { M.xyz.push_back((float)(v / 2)); M.xyz.push_back((float)(v % 2)); M.xyz.push_back(0.01f * (float)v); }
    for (int t = 0; t < k; ++t) { M.tri.push_back(t % 2 ? t + 1 : t); M.tri.push_back(t % 2 ? t : t + 1); M.tri.push_back(t + 2); }
    return M;
}
// the mesh of a sphere through the per-thread bodies of pm_tsdf.hpp, as tools/mesh_check.cpp replays mpmvs_tsdf_mesh
static Mesh sphere_mesh(int nx, int ny, int nz, double cx, double cy, double cz, double rad) {
    TsdfVol V;
    V.nx = nx; V.ny = ny; V.nz = nz; V.trunc = 1.0f; V.o[0] = V.o[1] = V.o[2] = 0.0; V.voxel = 1.0;
    const size_t n = (size_t)nx * ny * nz, tiles = (n + kScanBlock - 1) / kScanBlock;
    std::vector<float> sum(n);
    std::vector<int32_t> weight(n, 1);
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) sum[((size_t)k * ny + j) * nx + i] = (float)(std::sqrt((i - cx) * (i - cx) + (j - cy) * (j - cy) + (k - cz) * (k - cz)) - rad);
    std::vector<uint32_t> mask(n, 0u);
    std::vector<int> vexcl(n), tcount(n), totals(2 * tiles);
    nblk_rev = false;
    REPLAY(n, tsdf_mark_one(V, i, sum.data(), weight.data(), 1, mask.data(), tcount.data()));
    int gv = 0, gt = 0;
    for (size_t b = 0; b < tiles; ++b) {
        int sv = 0, st = 0;
        for (size_t k = b * kScanBlock; k < std::min(n, (b + 1) * kScanBlock); ++k) {
            vexcl[k] = sv; sv += __builtin_popcount(mask[k]);
            const int c = tcount[k]; tcount[k] = st; st += c;
        }
        totals[b] = gv; totals[tiles + b] = gt; gv += sv; gt += st;
    }
    Mesh M;
    M.xyz.assign(3 * (size_t)gv, 0.0f); M.tri.assign(3 * (size_t)gt, 0);
    REPLAY(n, tsdf_vertex_one(V, i, sum.data(), weight.data(), (const uint4*)nullptr, mask.data(), vexcl.data(), totals.data(), M.xyz.data(), (unsigned char*)nullptr));
    REPLAY(n, tsdf_triangle_one(V, i, sum.data(), weight.data(), 1, mask.data(), vexcl.data(), totals.data(), tcount.data(), totals.data() + tiles, M.tri.data()));
    return M;
}

int main() {
    for (unsigned k = 0; k < 256; ++k) order256[k] = k;
    std::shuffle(order256, order256 + 256, rng);
    {   // a strip of 4096 triangles numbered ascending, descending and scrambled
        const Mesh S = strip(4096);
        std::vector<int> perm(S.n());
        std::iota(perm.begin(), perm.end(), 0);
        run_case("strip of 4096, ascending", S);
        std::reverse(perm.begin(), perm.end());
        run_case("strip of 4096, descending", renumber(S, perm));
        std::shuffle(perm.begin(), perm.end(), rng);
        run_case("strip of 4096, scrambled", renumber(S, perm));
    }
    {   // a fan of 70 001 triangles around one vertex, the hub numbered first and last
        const int k = 70001;
        for (int hub_last = 0; hub_last < 2; ++hub_last) {
            Mesh M;
            const int hub = hub_last ? k + 1 : 0, first = hub_last ? 0 : 1;
            M.xyz.assign(3 * (size_t)(k + 2), 0.0f);
            M.xyz[3 * hub + 2] = 0.3f;
            for (int v = 0; v <= k; ++v) {
                const double a = 6.283185307179586 * v / (k + 1);
                M.xyz[3 * (first + v)] = (float)std::cos(a); M.xyz[3 * (first + v) + 1] = (float)std::sin(a); M.xyz[3 * (first + v) + 2] = (float)(0.05 * std::sin(7 * a));
            }
            for (int t = 0; t < k; ++t) { M.tri.push_back(hub); M.tri.push_back(first + t); M.tri.push_back(first + t + 1); }
            run_case(hub_last ? "fan of 70001, hub last" : "fan of 70001, hub first", M);
        }
    }
    {   // 70 001 one-triangle components, the vertices of a triangle far apart in the numbering, with colours
        const int k = 70001;
        Mesh M;
        for (int v = 0; v < 3 * k; ++v)
            for (int a = 0; a < 3; ++a) { M.xyz.push_back((float)(rng() % 2048) * 0.125f); M.rgb.push_back((unsigned char)(rng() % 256)); }
        for (int t = 0; t < k; ++t) { M.tri.push_back(2 * k + t); M.tri.push_back(t); M.tri.push_back(2 * k - 1 - t); }
        run_case("70001 one-triangle components", M);
    }
    {   // select masks of all, none and every other vertex at n = m = 70 001: 274 tiles, the scan of the tile totals carries into
        // a second round
        const int n = 70001;
        Mesh M;
        for (int v = 0; v < n; ++v)
            for (int a = 0; a < 3; ++a) M.xyz.push_back((float)((3 * v + a) % 8191));
        for (int t = 0; t < n; ++t) { M.tri.push_back(t); M.tri.push_back((t + 1) % n); M.tri.push_back((t + 2) % n); }
        run_case("ring, n = m = 70001", M);
    }
    {   // triangles with repeated indices among ordinary ones; vertex 9 is named only by (9, 9, 9), vertex 10 by nothing
        Mesh M;
        const float p[11][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0.5f}, {3, 0, 0}, {4, 0, 0}, {3, 1, 0}, {6, 6, 6}, {7, 6, 6}, {9, 9, 9}, {5, 5, 5}};
        const int t[7][3] = {{0, 1, 2}, {1, 3, 2}, {2, 2, 4}, {5, 6, 5}, {7, 8, 8}, {9, 9, 9}, {4, 5, 6}};
        for (auto& q : p) M.xyz.insert(M.xyz.end(), q, q + 3);
        for (auto& q : t) M.tri.insert(M.tri.end(), q, q + 3);
        run_case("repeated indices", M);
        Mesh R;   // random triangles in narrow windows: many repeats, many components
        const int n = 3000;
        for (int v = 0; v < 3 * n; ++v) R.xyz.push_back((float)(rng() % 64) - 32.0f);
        for (int k = 0; k < 2 * n; ++k) { const int w = (int)(rng() % (n - 4)); for (int a = 0; a < 3; ++a) R.tri.push_back(w + (int)(rng() % 4)); }
        run_case("random windows of 4, repeats", R);
    }
    Mesh anchor = sphere_mesh(10, 9, 8, 4.3, 3.9, 3.4, 2.7);
    {   // the anchor sphere of the TSDF contract: 410 vertices, 816 triangles, one component, every normal outwards
        if (anchor.n() != 410 || anchor.m() != 816) { printf("the anchor's counts differ\n"); ++failures; }
        run_case("sphere anchor", anchor);
        std::vector<float> nrm;
        if (replay_normals(anchor, nrm) != 410) { printf("sphere anchor: an undefined normal\n"); ++failures; }
        const double c[3] = {4.3, 3.9, 3.4};
        for (size_t v = 0; v < anchor.n(); ++v) {
            double dot = 0.0;
            for (int a = 0; a < 3; ++a) dot += (double)nrm[3 * v + a] * ((double)anchor.xyz[3 * v + a] - c[a]);
            if (!(dot > 0.0)) { printf("sphere anchor: normal %zu points inwards\n", v); ++failures; break; }
        }
        Mesh big = anchor, small = anchor;   // scaled by 2^40 and 2^-40: the same bits
        for (float& x : big.xyz) x = std::ldexp(x, 40);
        for (float& x : small.xyz) x = std::ldexp(x, -40);
        std::vector<float> nb, ns;
        replay_normals(big, nb); replay_normals(small, ns);
        if (!same(nb, nrm) || !same(ns, nrm)) { printf("sphere anchor: a power of two shows in the normals\n"); ++failures; }
    }
    {   // non-finite vertices: one coordinate of every 17th vertex, and of vertex 0
        Mesh M = anchor;
        const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
        for (size_t v = 0; v < M.n(); v += 17) M.xyz[3 * v + v % 3] = bad[(v / 17) % 3];
        run_case("sphere anchor, non-finite vertices", M);
        for (float& x : M.xyz) x = bad[0];
        run_case("no finite vertex", M);
        Mesh P = anchor;   // all vertices in one place: no extent
        for (float& x : P.xyz) x = 2.5f;
        run_case("no extent", P);
        Mesh E;
        run_case("empty", E);
        E.xyz.assign(3 * 300, 1.0f);
        run_case("300 vertices, no triangle", E);
    }
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("all equal\n");
    return 0;
}
