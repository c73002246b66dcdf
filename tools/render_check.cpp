// render_check.cpp -- the three passes of csrc/pm_render.hpp replayed on the host, thread by thread in a scrambled order, through
// the header's own __host__ __device__ code (the projection, the in-view test and the per-thread body of every kernel), in the
// launch order of cloud_render_chunk of mpmvs_cloud.hip and with buffers of exactly its sizes (the views of a chunk behind one
// another, chunks of kRenderChunk views), against a plain-loop statement of the contract: random clouds
// with non-finite, far-away and behind-the-camera points in views of different sizes, more views than a chunk, a 1 x 1 view, the
// image-border values, the visibility threshold, and a window larger than the image; each with all, some and no index maps.
// A host program, so that it runs under the sanitizers without a GPU:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Imp-mvs_amd/csrc -o build/render_check tools/render_check.cpp && build/render_check
// Prints one line per case and "all equal"; exit status 1 if any result differs in a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pm_render.hpp"
using namespace pm;

static unsigned order256[256];   // the order in which the 256 threads of a block run
#define REPLAY(count, call)                                                                  \
    for (size_t b_ = 0; b_ < ((size_t)(count) + 255) / 256; ++b_)                            \
        for (unsigned t_ = 0; t_ < 256; ++t_) {                                              \
            const size_t i = b_ * 256 + order256[t_];                                        \
            if (i < (size_t)(count)) call;                                                   \
        }

struct Cam {
    CamDev c;
    int w, h;
};
struct Maps {
    std::vector<std::vector<float>> depth;
    std::vector<std::vector<int32_t>> idx;   // empty where not wanted
};

// want[v]: an index map for view v
static void gpu_like(const std::vector<float>& xyz, const std::vector<Cam>& cams, int splat, float occl_rel, const std::vector<char>& want, Maps& out) {
    const size_t n = xyz.size() / 3;
    const int nv = (int)cams.size();
    const float m = 1.0f + occl_rel;
    out.depth.assign(nv, {});
    out.idx.assign(nv, {});
    for (int v0 = 0; v0 < nv; v0 += kRenderChunk) {
        const int v1 = std::min(nv, v0 + kRenderChunk);
        size_t total = 0;
        bool any_idx = false;
        for (int v = v0; v < v1; ++v) total += (size_t)cams[v].w * cams[v].h, any_idx = any_idx || want[v];
        // exact-size buffers: AddressSanitizer sees any index outside them
        std::vector<uint32_t> zc(total, kRenderInfBits), idx(any_idx ? total : 0, kRenderNoIdx);
        std::vector<float> depth(total, -1.0f);
        RenderChunkArgs A;
        memset(&A, 0, sizeof A);
        A.n = v1 - v0;
        size_t at = 0;
        for (int v = v0; v < v1; ++v) {
            RenderView& V = A.v[v - v0];
            V.cam = cams[v].c, V.w = cams[v].w, V.h = cams[v].h;
            V.zc = zc.data() + at;
            V.idx = want[v] ? idx.data() + at : nullptr;
            at += (size_t)V.w * V.h;
        }
        REPLAY(n, render_point_one<false>(i, xyz.data(), A));
        if (any_idx) REPLAY(n, render_point_one<true>(i, xyz.data(), A));
        at = 0;
        for (int k = 0; k < A.n; ++k) {
            const RenderView& V = A.v[k];
            const size_t npix = (size_t)V.w * V.h;
            REPLAY(npix, render_resolve_one(i, V.zc, V.w, V.h, splat, m, depth.data() + at, V.idx));
            out.depth[v0 + k].assign(depth.begin() + at, depth.begin() + at + npix);
            if (V.idx) {
                out.idx[v0 + k].resize(npix);
                memcpy(out.idx[v0 + k].data(), V.idx, npix * 4);
            }
            at += npix;
        }
    }
}

// the contract in plain loops; every fp32 operation through a volatile, so that nothing is fused or kept wider
static void statement(const std::vector<float>& xyz, const std::vector<Cam>& cams, int splat, float occl_rel, Maps& out) {
    const size_t n = xyz.size() / 3;
    out.depth.assign(cams.size(), {});
    out.idx.assign(cams.size(), {});
    for (size_t v = 0; v < cams.size(); ++v) {
        const CamDev& c = cams[v].c;
        const int W = cams[v].w, H = cams[v].h;
        std::vector<float> Zc((size_t)W * H, INFINITY);
        std::vector<int32_t> first((size_t)W * H, -1);
        for (size_t i = 0; i < n; ++i) {
            const float* p = &xyz[3 * i];
            if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
            volatile float t[3];
            for (int r = 0; r < 3; ++r) {
                volatile float a = c.R[3 * r] * p[0], b = c.R[3 * r + 1] * p[1], d = c.R[3 * r + 2] * p[2];
                volatile float s = a + b;
                volatile float s2 = s + d;
                t[r] = s2 + c.t[r];
            }
            volatile float row[3];
            for (int r = 0; r < 3; ++r) {
                volatile float a = c.K[3 * r] * t[0], b = c.K[3 * r + 1] * t[1], d = c.K[3 * r + 2] * t[2];
                volatile float s = a + b;
                row[r] = s + d;
            }
            const float z = row[2];
            if (!(std::isfinite(z) && z > 0.0f)) continue;
            volatile float u = row[0] / z, w = row[1] / z;
            volatile float fu = u + 0.5f, fv = w + 0.5f;
            if (!(fu >= 0.0f && fu < (float)W && fv >= 0.0f && fv < (float)H)) continue;
            const size_t pix = (size_t)(int)fv * W + (int)fu;
            if (z < Zc[pix]) Zc[pix] = z, first[pix] = (int32_t)i;   // i ascends: the first index of the minimum stays
        }
        volatile float m = 1.0f + occl_rel;
        out.depth[v].assign((size_t)W * H, 0.0f);
        out.idx[v].assign((size_t)W * H, -1);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                float z1 = INFINITY;
                for (int yy = y - splat; yy <= y + splat; ++yy)
                    for (int xx = x - splat; xx <= x + splat; ++xx)
                        if (yy >= 0 && yy < H && xx >= 0 && xx < W) z1 = std::min(z1, Zc[(size_t)yy * W + xx]);
                const float own = Zc[(size_t)y * W + x];
                volatile float lim = z1 * m;
                if (std::isfinite(own) && own <= lim) out.depth[v][(size_t)y * W + x] = own, out.idx[v][(size_t)y * W + x] = first[(size_t)y * W + x];
            }
    }
}

static int compare(const char* name, const std::vector<float>& xyz, const std::vector<Cam>& cams, int splat, float occl_rel) {
    Maps a, b;
    statement(xyz, cams, splat, occl_rel, a);
    int bad_total = 0;
    for (int mode = 0; mode < 3; ++mode) {   // all index maps, every other one, none
        std::vector<char> want(cams.size());
        for (size_t v = 0; v < cams.size(); ++v) want[v] = mode == 0 || (mode == 1 && v % 2 == 0);
        gpu_like(xyz, cams, splat, occl_rel, want, b);
        size_t bad = 0, pixels = 0, covered = 0;
        for (size_t v = 0; v < cams.size(); ++v) {
            pixels += a.depth[v].size();
            if (b.depth[v].size() != a.depth[v].size() || (want[v] ? b.idx[v].size() != a.idx[v].size() : !b.idx[v].empty())) { ++bad; continue; }
            for (size_t k = 0; k < a.depth[v].size(); ++k) {
                covered += a.depth[v][k] != 0.0f;
                bad += memcmp(&a.depth[v][k], &b.depth[v][k], 4) != 0 || (want[v] && a.idx[v][k] != b.idx[v][k]);
            }
        }
        printf("%-18s splat %d occl %-5g mode %d: %zu views, %zu pixels, %zu covered, %zu differ\n", name, splat, occl_rel, mode, cams.size(), pixels, covered, bad);
        bad_total += bad != 0;
    }
    return bad_total;
}

static Cam pinhole(int w, int h, float f, float cx, float cy, float yaw, float tx, float ty, float tz) {
    Cam c;
    memset(&c, 0, sizeof c);
    const float K[9] = {f, 0, cx, 0, f, cy, 0, 0, 1}, R[9] = {std::cos(yaw), 0, std::sin(yaw), 0, 1, 0, -std::sin(yaw), 0, std::cos(yaw)};
    memcpy(c.c.K, K, sizeof K);
    memcpy(c.c.R, R, sizeof R);
    c.c.t[0] = tx, c.c.t[1] = ty, c.c.t[2] = tz;
    c.w = w, c.h = h;
    return c;
}

int main() {
    std::mt19937 g(5);
    for (int i = 0; i < 256; ++i) order256[i] = i;
    std::shuffle(order256, order256 + 256, g);   // threads of a block in a scrambled order
    std::uniform_real_distribution<float> U(0.f, 1.f);
    int fails = 0;
    {   // random cube around the origin, cameras of different sizes in front of it; junk among the points
        std::vector<float> xyz(3 * 20000);
        for (auto& v : xyz) v = U(g) * 4.0f - 2.0f;
        xyz[9] = NAN, xyz[100] = INFINITY, xyz[301] = -INFINITY, xyz[12] = 1e30f, xyz[16] = -1e30f, xyz[20] = 3e38f;
        for (int i = 0; i < 3000; ++i) {   // exact duplicates: ties for the index pass
            const int a = (int)(U(g) * 19999), b = (int)(U(g) * 19999);
            for (int k = 0; k < 3; ++k) xyz[3 * a + k] = xyz[3 * b + k];
        }
        std::vector<Cam> cams = {pinhole(64, 48, 40.0f, 31.5f, 23.5f, 0.0f, 0, 0, 5.0f), pinhole(33, 57, 30.0f, 16.0f, 28.0f, 0.3f, 0.2f, -0.1f, 4.0f),
                                 pinhole(1, 1, 1.0f, 0.0f, 0.0f, 0.0f, 0, 0, 5.0f), pinhole(50, 37, 35.0f, 25.0f, 18.0f, -0.4f, 0, 0, 1.0f)};
        for (int splat : {0, 1, 2, 8})
            for (float occl : {0.0f, 0.02f}) fails += compare("random", xyz, cams, splat, occl);
        std::vector<Cam> many;   // kRenderChunk + 3 views: two chunks
        for (int v = 0; v < kRenderChunk + 3; ++v) many.push_back(pinhole(20 + 3 * v, 31 - v, 18.0f + v, 10.0f + v, 15.0f, 0.1f * v - 0.5f, 0, 0, 4.5f));
        fails += compare("two chunks", xyz, many, 1, 0.02f);
        std::vector<float> none, nan3 = {NAN, 0, 0};
        fails += compare("no point", none, cams, 1, 0.02f);
        fails += compare("nan point", nan3, cams, 1, 0.02f);
    }
    {   // identity camera 7 x 5: the values around u = -0.5 / 6.5 and v = -0.5 / 4.5, at z = 1 and doubled at z = 2
        Cam c = pinhole(7, 5, 1.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0);
        std::vector<float> xyz;
        for (float zz : {1.0f, 2.0f}) {
            for (float e : {-0.5f, 6.5f})
                for (float x : {std::nextafter(e, -INFINITY), e, std::nextafter(e, INFINITY)}) xyz.insert(xyz.end(), {x * zz, 2.0f * zz, zz});
            for (float e : {-0.5f, 4.5f})
                for (float y : {std::nextafter(e, -INFINITY), e, std::nextafter(e, INFINITY)}) xyz.insert(xyz.end(), {3.0f * zz, y * zz, zz});
        }
        for (int splat : {0, 1}) fails += compare("borders", xyz, {c}, splat, 0.02f);
    }
    for (float occl : {0.02f, 0.0f}) {   // identity camera 9 x 3: the visibility threshold to the last bit
        Cam c = pinhole(9, 3, 1.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0);
        const float m = 1.0f + occl, zb = 2.0f * m, zb2 = std::nextafter(zb, INFINITY);
        std::vector<float> xyz = {8, 2, 2, 5 * zb, zb, zb, 3 * zb2, zb2, zb2, 700, 100, 100};
        for (int splat : {0, 1, 2, 3}) fails += compare("threshold", xyz, {c}, splat, occl);
    }
    {   // the window larger than the image
        Cam c = pinhole(5, 4, 3.0f, 2.0f, 1.5f, 0.0f, 0, 0, 3.0f);
        std::vector<float> xyz(3 * 60);
        for (auto& v : xyz) v = U(g) * 2.0f - 1.0f;
        for (int splat : {0, 8}) fails += compare("window > image", xyz, {c}, splat, 0.3f);
    }
    printf(fails ? "FAILED %d\n" : "all equal\n", fails);
    return fails != 0;
}
