// oracle/ref_host_driver.cpp
//
// TEST INFRASTRUCTURE ONLY.  extern "C" entry points over the REFERENCE'S OWN host code: the two files included below are pieces
// of the reference's src/PatchMatch.cpp -- the block from its PLY writer to the end of RunFusion, and the definitions of
// GetCost, GetGeomCost, GetReferenceImageWidth, GetReferenceImageHeight and GetTriangulateVertices -- that `make ref` cuts into
// oracle/_ref/ (never committed) and compiles against the stand-in header oracle/ref_shim/host_standin.h.  Everything in this
// file is the project's: it holds the arrays of one call, serves them to the reference's readers by image number, and hands
// the reference's functions their arguments.  tests/ref_common.py loads the result.
//
// Built twice (oracle/Makefile), both with -ffp-contract=off -O2 -fno-fast-math -DBUILD_NCNN (the sky branch of RunFusion is
// compiled): libmpmvs_ref_host.so, whose cv::Vec3f `/=` divides, and libmpmvs_ref_host_rcp.so (-DMPMVS_REF_VEC_RCP), whose `/=`
// multiplies by the fp32 reciprocal.
// The reference's text is compiled as it is: its warnings are not this project's to fix.
#include "host_standin.h"

#include <type_traits>

// Which arithmetic of RunFusion runs in double is decided by overload resolution on these four calls as this translation unit
// sees them: <math.h> of a C++ library declares the float overloads in the global namespace, so exp(float) and fabs(float) are
// the float functions; pow(float, int) promotes both arguments to double, and the sqrt of that double is the double function.
static_assert(std::is_same<decltype(exp(1.0f)), float>::value, "exp(float) must resolve to the float function");
static_assert(std::is_same<decltype(fabs(1.0f)), float>::value, "fabs(float) must resolve to the float function");
static_assert(std::is_same<decltype(pow(1.0f, 2)), double>::value, "pow(float, int) must resolve to the double function");
static_assert(std::is_same<decltype(sqrt(1.0)), double>::value, "sqrt(double) must resolve to the double function");

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-parameter"
#pragma GCC diagnostic ignored "-Wunused-variable"
#pragma GCC diagnostic ignored "-Wunused-but-set-variable"
#pragma GCC diagnostic ignored "-Wmaybe-uninitialized"
#pragma GCC diagnostic ignored "-Wsign-compare"
#pragma GCC diagnostic ignored "-Wformat"
#include "PatchMatch_fusion.inc"
#include "PatchMatch_vertices.inc"
#pragma GCC diagnostic pop

#include <cstring>

int g_refh_resampled = 0;

namespace {

// the arrays of the call in flight, by image number
struct Registry {
    int n = 0;
    const Camera* cams = nullptr;
    const float* const* depths = nullptr;
    const float* const* normals = nullptr;
    const unsigned char* const* bgr = nullptr;
    const unsigned char* const* sky = nullptr;
    bool bad_path = false;
} g_reg;

// the image number of a path the reference composed: its last run of eight digits
int image_number(const std::string& path) {
    int run = 0;
    for (size_t i = path.size(); i-- > 0;) {
        run = (path[i] >= '0' && path[i] <= '9') ? run + 1 : 0;
        if (run == 8) {
            const int id = std::stoi(path.substr(i, 8));
            if (id >= 0 && id < g_reg.n) return id;
            break;
        }
    }
    g_reg.bad_path = true;
    return 0;
}

}  // namespace

cv::Mat cv::imread(const std::string& path, int) {
    const int k = image_number(path);
    const int h = g_reg.cams[k].height, w = g_reg.cams[k].width;
    if (path.find("skymask") != std::string::npos) {
        cv::Mat m(h, w, (size_t)1);
        if (g_reg.sky && g_reg.sky[k]) std::memcpy(m.store->data(), g_reg.sky[k], (size_t)h * w);
        return m;
    }
    cv::Mat m(h, w, (size_t)3);
    std::memcpy(m.store->data(), g_reg.bgr[k], (size_t)h * w * 3);
    return m;
}
Camera ReadCamera(const std::string& cam_path) { return g_reg.cams[image_number(cam_path)]; }
bool readDepthDmb(const std::string file_path, cv::Mat_<float>& depth) {
    const int k = image_number(file_path);
    depth = cv::Mat_<float>(g_reg.cams[k].height, g_reg.cams[k].width);
    std::memcpy(depth.store->data(), g_reg.depths[k], depth.store->size());
    return true;
}
bool readNormalDmb(const std::string file_path, cv::Mat_<cv::Vec3f>& normal) {
    const int k = image_number(file_path);
    normal = cv::Mat_<cv::Vec3f>(g_reg.cams[k].height, g_reg.cams[k].width);
    std::memcpy(normal.store->data(), g_reg.normals[k], normal.store->size());
    return true;
}

extern "C" {

// RunFusion over n estimated images with refID == index.  cams[k] carries the size of image k's maps; bgr[k] is [h][w][3];
// sky is NULL (config.sky_seg off) or per image a [h][w] mask or NULL (served as all zero); the source ids of image i are
// src_ids[src_off[i] .. src_off[i + 1]), image i itself first, as GenerateSampleList leaves them.  The reference's own writer
// writes <out_folder>/MPMVS_model.ply: the only output.  Returns 0, -1 if anything would have been resampled, -2 for a path
// without a known image number.
int refh_fuse(int n, const Camera* cams, const float* const* depths, const float* const* normals, const unsigned char* const* bgr,
              const unsigned char* const* sky, const int* src_off, const int* src_ids, int use_dynamic, const char* out_folder) {
    g_reg = Registry{n, cams, depths, normals, bgr, sky, false};
    g_refh_resampled = 0;
    ConfigParams config;
    config.input_folder = "registered";
    config.output_folder = out_folder;
    config.sky_seg = sky != nullptr;
    config.use_dynamic_consistency = use_dynamic != 0;
    std::vector<Scene> scenes(n);
    for (int i = 0; i < n; ++i) {
        scenes[i].estimate = true;
        scenes[i].refID = i;
        scenes[i].srcID.assign(src_ids + src_off[i], src_ids + src_off[i + 1]);
    }
    std::streambuf* const chatter = std::cout.rdbuf(nullptr);  // the reference reports every image on stdout
    RunFusion(config, scenes);
    std::cout.rdbuf(chatter);
    std::cout.clear();
    const bool bad_path = g_reg.bad_path;
    g_reg = Registry{};
    return g_refh_resampled ? -1 : (bad_path ? -2 : 0);
}

// GetTriangulateVertices over one cost map (and, for the geometric rule, one geometric cost map) of w x h pixels.
// Returns the number of vertices; out_xy receives the first `cap` of them as x, y pairs.
int refh_vertices(const float* costs, const float* geom, int w, int h, int geom_rule, int* out_xy, int cap) {
    PatchMatchCUDA pm;
    Camera cam{};
    cam.width = w;
    cam.height = h;
    pm.cameras.push_back(cam);
    pm.hostCosts = const_cast<float*>(costs);
    pm.hostGeomCosts = const_cast<float*>(geom);
    pm.params = PatchMatchParams{};
    pm.params.geomPlanarPrior = geom_rule ? 1 : 0;
    std::vector<cv::Point> v;
    pm.GetTriangulateVertices(v);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) {
        out_xy[2 * i] = v[i].x;
        out_xy[2 * i + 1] = v[i].y;
    }
    return (int)v.size();
}

}  // extern "C"
