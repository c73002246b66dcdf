// oracle/ref_driver.cpp
//
// TEST INFRASTRUCTURE ONLY.  extern "C" entry points over the REFERENCE'S OWN device code, compiled for the host: the two files
// included below are copies of the reference's kernel sources, cut before their first host function, that `make ref` writes
// into oracle/_ref/ (never committed) and compiles against the stand-in headers of oracle/ref_shim/.  Everything in this file
// is the project's: it holds arrays, plays the CUDA threads of a launch one after the other with the reference's block shape
// and grid sizes, and hands the reference's functions their arguments.  tests/ref_common.py loads the result.
//
// Built twice (oracle/Makefile): libmpmvs_ref.so with -ffp-contract=off (IEEE operations as written) and libmpmvs_ref_fma.so
// with -ffp-contract=fast -mfma (the compiler contracts a * b + c as nvcc does): two real builds of the same formulas.
// the reference's text is compiled as it is: its unused parameters and variables are not this project's to fix (everything
// after the pop, and the stand-in headers, compile under -Wall -Wextra)
#include "cuda_standin.h"
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-parameter"
#pragma GCC diagnostic ignored "-Wunused-variable"
#pragma GCC diagnostic ignored "-Wunused-but-set-variable"
#pragma GCC diagnostic ignored "-Wmaybe-uninitialized"
#pragma GCC diagnostic ignored "-Wsign-compare"
#include "PatchMatch_device.inc"
#include "SkyRegionDetect_device.inc"
#pragma GCC diagnostic pop

#include <cstring>
#include <vector>

thread_local uint3 blockIdx, threadIdx;
thread_local dim3 blockDim, gridDim;
int g_ref_draw_overflow = 0;

namespace {

struct RefCtx {
    int n_img = 0, W = 0, H = 0;
    std::vector<Camera> cams;
    std::vector<std::vector<float>> img_px, depth_px;
    std::vector<RefTexture> img_tex, depth_tex;
    std::vector<cudaTextureObject_t> images, depths;
    std::vector<float4> planes, prior;
    std::vector<float> costs, geom;
    std::vector<unsigned int> sel, mask;
    std::vector<curandState> rand;
};

// the reference's launch shape (Run(): blocks of 32 x 16; the init grid covers the image, the checkerboard grid covers
// ceil((H / 2) / 16) block rows of 16 thread rows, each thread row two image rows)
constexpr int kBlockW = 32, kBlockH = 16;
inline dim3 grid_init(int W, int H) { return dim3((W + kBlockW - 1) / kBlockW, (H + kBlockH - 1) / kBlockH, 1); }
inline dim3 grid_checker(int W, int H) { return dim3((W + kBlockW - 1) / kBlockW, ((H / 2) + kBlockH - 1) / kBlockH, 1); }

template <class F>
void launch(dim3 grid, F&& body) {
    gridDim = grid;
    blockDim = dim3(kBlockW, kBlockH, 1);
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            blockIdx = uint3{bx, by, 0};
            for (unsigned ty = 0; ty < (unsigned)kBlockH; ++ty)
                for (unsigned tx = 0; tx < (unsigned)kBlockW; ++tx) {
                    threadIdx = uint3{tx, ty, 0};
                    body();
                }
        }
}

}  // namespace

extern "C" {

RefCtx* ref_create(int n_img, const Camera* cams, const float* const* images, int q8) {
    RefCtx* c = new RefCtx();
    c->n_img = n_img;
    c->cams.assign(cams, cams + n_img);
    c->W = cams[0].width;
    c->H = cams[0].height;
    c->img_px.resize(n_img);
    c->img_tex.resize(n_img);
    for (int i = 0; i < n_img; ++i) {
        const size_t n = (size_t)cams[i].width * cams[i].height;
        c->img_px[i].assign(images[i], images[i] + n);
        c->img_tex[i] = RefTexture{c->img_px[i].data(), cams[i].width, cams[i].height, q8};
    }
    for (int i = 0; i < n_img; ++i) c->images.push_back(&c->img_tex[i]);
    const size_t wh = (size_t)c->W * c->H;
    c->planes.assign(wh, float4{0, 0, 0, 0});
    c->prior.assign(wh, float4{0, 0, 0, 0});
    c->costs.assign(wh, 0.0f);
    c->geom.assign(wh, 0.0f);
    c->sel.assign(wh, 0u);
    c->mask.assign(wh, 0u);
    c->rand.assign(wh, curandState{nullptr, 0, 0});
    return c;
}
void ref_destroy(RefCtx* c) { delete c; }

// source depth maps (one per source view), contiguous rows
void ref_set_src_depths(RefCtx* c, const float* const* depths, const int* widths, const int* heights, int q8) {
    const int n = c->n_img - 1;
    c->depth_px.assign(n, std::vector<float>());
    c->depth_tex.assign(n, RefTexture{nullptr, 0, 0, 0});
    c->depths.clear();
    for (int i = 0; i < n; ++i) {
        c->depth_px[i].assign(depths[i], depths[i] + (size_t)widths[i] * heights[i]);
        c->depth_tex[i] = RefTexture{c->depth_px[i].data(), widths[i], heights[i], q8};
    }
    for (int i = 0; i < n; ++i) c->depths.push_back(&c->depth_tex[i]);
}
void ref_set_prior(RefCtx* c, const float* prior4, const unsigned int* mask) {
    const size_t wh = (size_t)c->W * c->H;
    std::memcpy(c->prior.data(), prior4, wh * 16);
    std::memcpy(c->mask.data(), mask, wh * 4);
}
void ref_set_state(RefCtx* c, const float* planes4, const float* costs, const unsigned int* sel) {
    const size_t wh = (size_t)c->W * c->H;
    if (planes4) std::memcpy(c->planes.data(), planes4, wh * 16);
    if (costs) std::memcpy(c->costs.data(), costs, wh * 4);
    if (sel) std::memcpy(c->sel.data(), sel, wh * 4);
}
void ref_get(RefCtx* c, float* planes4, float* costs, unsigned int* sel, float* geom) {
    const size_t wh = (size_t)c->W * c->H;
    if (planes4) std::memcpy(planes4, c->planes.data(), wh * 16);
    if (costs) std::memcpy(costs, c->costs.data(), wh * 4);
    if (sel) std::memcpy(sel, c->sel.data(), wh * 4);
    if (geom) std::memcpy(geom, c->geom.data(), wh * 4);
}

// ---- per function ---------------------------------------------------------------------------------------------------------
// ComputeHomography for a camera-frame plane and the 0-based source view v
void ref_homography(RefCtx* c, const float* plane4, int v, float* H9) {
    ComputeHomography(c->cams[0], c->cams[v + 1], float4{plane4[0], plane4[1], plane4[2], plane4[3]}, H9);
}
// ComputeBilateralNCC of per-pixel camera-frame planes against every source view; out is [V][H][W]
void ref_eval_ncc(RefCtx* c, const PatchMatchParams* prm, const float* planes4, int scale, float* out) {
    const int V = prm->num_images - 1;
    const size_t wh = (size_t)c->W * c->H;
    for (int y = 0; y < c->H; ++y)
        for (int x = 0; x < c->W; ++x) {
            const float4 pl = ((const float4*)planes4)[(size_t)y * c->W + x];
            for (int v = 0; v < V; ++v)
                out[(size_t)v * wh + (size_t)y * c->W + x] = ComputeBilateralNCC(c->images[0], c->cams[0], c->images[v + 1], c->cams[v + 1], make_int2(x, y), pl, *prm, scale);
        }
}
// ComputeGeomConsistencyCost of per-pixel camera-frame planes; out is [V][H][W]
int ref_eval_geom(RefCtx* c, const PatchMatchParams* prm, const float* planes4, float* out) {
    const int V = prm->num_images - 1;
    if ((int)c->depths.size() != V) return -1;
    const size_t wh = (size_t)c->W * c->H;
    for (int y = 0; y < c->H; ++y)
        for (int x = 0; x < c->W; ++x) {
            const float4 pl = ((const float4*)planes4)[(size_t)y * c->W + x];
            for (int v = 0; v < V; ++v) out[(size_t)v * wh + (size_t)y * c->W + x] = ComputeGeomConsistencyCost(c->depths[v], c->cams[0], c->cams[v + 1], pl, make_int2(x, y));
        }
    return 0;
}
// ComputeMultiViewInitialCostandSelectedViews of per-pixel camera-frame planes; costs and selected views are [H][W]
void ref_eval_initial(RefCtx* c, const PatchMatchParams* prm, const float* planes4, int scale, float* costs, unsigned int* sel) {
    for (int y = 0; y < c->H; ++y)
        for (int x = 0; x < c->W; ++x) {
            const size_t idx = (size_t)y * c->W + x;
            costs[idx] = ComputeMultiViewInitialCostandSelectedViews(c->images.data(), c->cams.data(), make_int2(x, y), ((const float4*)planes4)[idx], &sel[idx], *prm, scale);
        }
}

// ---- per launch -------------------------------------------------------------------------------------------------------------
// One kernel of Run().  kind as in include/mpmvs.h (0 InitializeScore, 1 BlackPixelUpdate, 2 RedPixelUpdate, 3 GetDepthandNormal,
// 4 BlackPixelFilter, 5 RedPixelFilter).  draws: [H * W][cap] uniforms, row idx = y * W + x, consumed from the left by that pixel.
// Returns the largest number of draws any pixel asked for, -1 if one asked for more than cap, -2 for a bad kind or missing input.
int ref_launch(RefCtx* c, const PatchMatchParams* prm, int kind, int iter, int scale, const float* draws, int cap) {
    const size_t wh = (size_t)c->W * c->H;
    if (prm->num_images != c->n_img) return -2;
    if (prm->geom_consistency && (int)c->depths.size() != c->n_img - 1) return -2;
    for (size_t i = 0; i < wh; ++i) c->rand[i] = curandState{draws ? draws + i * (size_t)cap : nullptr, 0, draws ? cap : 0};
    g_ref_draw_overflow = 0;
    Camera* cams = c->cams.data();
    const cudaTextureObject_t* images = c->images.data();
    const cudaTextureObject_t* depths = c->depths.empty() ? nullptr : c->depths.data();
    float4* planes = c->planes.data();
    float* costs = c->costs.data();
    curandState* rs = c->rand.data();
    unsigned int* sel = c->sel.data();
    float4* prior = c->prior.data();
    unsigned int* mask = c->mask.data();
    float* geom = c->geom.data();
    const PatchMatchParams p = *prm;
    switch (kind) {
        case 0: launch(grid_init(c->W, c->H), [&] { InitializeScore(images, cams, planes, costs, rs, sel, prior, mask, p, scale); }); break;
        case 1: launch(grid_checker(c->W, c->H), [&] { BlackPixelUpdate(images, depths, cams, planes, costs, rs, sel, prior, mask, p, iter, scale, geom); }); break;
        case 2: launch(grid_checker(c->W, c->H), [&] { RedPixelUpdate(images, depths, cams, planes, costs, rs, sel, prior, mask, p, iter, scale, geom); }); break;
        case 3: launch(grid_init(c->W, c->H), [&] { GetDepthandNormal(cams, planes, p); }); break;
        case 4: launch(grid_checker(c->W, c->H), [&] { BlackPixelFilter(cams, planes, costs); }); break;
        case 5: launch(grid_checker(c->W, c->H), [&] { RedPixelFilter(cams, planes, costs); }); break;
        default: return -2;
    }
    if (g_ref_draw_overflow) return -1;
    int most = 0;
    for (size_t i = 0; i < wh; ++i) most = c->rand[i].pos > most ? c->rand[i].pos : most;
    return most;
}

// ---- sky filter -------------------------------------------------------------------------------------------------------------
// Pixel_bilateral_filter over a BGR uint8 image [h][w][3] and a float mask [h][w]
void ref_sky_bilateral(const unsigned char* bgr, const float* mask, float* out, int h, int w) {
    launch(grid_init(w, h), [&] { Pixel_bilateral_filter(bgr, mask, out, h, w); });
}

}  // extern "C"
