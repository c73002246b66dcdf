// scene_io.h -- file formats either side of the hot path and the
// file-based ProcessProblem; same names as the reference (include/utility.h:59-62,
// include/PatchMatch.h:75-78) with cv::Mat replaced by Image.
#ifndef MPMVS_HOST_SCENE_IO_H_
#define MPMVS_HOST_SCENE_IO_H_

#include <string>
#include <vector>

#include "PatchMatch.h"

bool readDepthDmb(const std::string file_path, Image& depth);
int writeDepthDmb(const std::string file_path, const Image& depth);
bool readNormalDmb(const std::string file_path, Image& normal);
int writeNormalDmb(const std::string file_path, const Image& normal);
Camera ReadCamera(const std::string& cam_path);
// reference GenerateSampleList(const ConfigParams&, ...): the two config values it uses are passed directly
void GenerateSampleList(const std::string& input_folder, int maxSourceImageNum, int maxImageSize, std::vector<Scene>& Scenes);
// reference include/PatchMatch.h:29-33,77
struct PointList {
    float3 coord;
    float3 normal;
    float3 color;
};
void StoreColorPlyFileBinaryPointCloud(const std::string& plyFilePath, const std::vector<PointList>& pc);
// reference RunFusion(const ConfigParams&, const std::vector<Scene>&) (include/PatchMatch.h:85); returns the point count
// resident = true (no counterpart in the reference, whose passes hand over through files): the maps are Scenes[i].depth / .normal as the
// pass schedule left them in memory, and where a Problem's context still holds them in HBM (ResidentResultContext) they are fused from
// there without an upload (mpmvs_fuse_ply_ctx); cameras, colour images and sky masks are read as before.  Same PLY, byte for byte.
// write_vis = true: the fusion also returns every point's track (mpmvs_fuse_ply_tracks) and <output>/MPMVS_model.ply.vis is written
// beside the same PLY -- COLMAP's point-visibility file: uint64 number of points, per point uint32 k and k x uint32 image id, little
// endian, the images of the point's track in track order, numbered as pair.txt numbers them (Scene::refID).
long RunFusion(const std::string& input_folder, const std::string& output_folder, std::vector<Scene>& Scenes, bool use_dynamic_consistency, int device = 0,
               bool sky_seg = false, bool resident = false, bool write_vis = false);
// cv::imread(path, IMREAD_GRAYSCALE) + convertTo(CV_32F) (reference src/PatchMatch.cpp:877-882): JPEG (own decoder,
// jpeg_decode.h), binary PGM (P5) or PPM (P6, converted with OpenCV's fixed-point BGR2GRAY weights); format by content
bool readGrayImage(const std::string& path, Image& img);
// the same without the convertTo: the bytes imread returns, which is what the 8-bit entry takes (mpmvs_set_views_u8)
bool readGrayImage8(const std::string& path, Image8& img);
// The grey image of a Scene that is read from a folder: the decoded bytes at the file's size (Scene::image8).  With
// MPMVS_HOST_FLOAT_IMAGES=1 in the environment (read on every call; for A/B runs) the image is widened to fp32 into Scene::image as
// before the 8-bit entry existed: AdjustImageScale then shrinks it on the host and CudaMemInit takes mpmvs_set_views.
bool readSceneImage(const std::string& path, Scene& s);
// cv::imread(path, IMREAD_COLOR) (reference :324): JPEG, PPM or PGM -> 3 channels B,G,R
bool readColorImage(const std::string& path, Image8& bgr);
bool writeGrayImage(const std::string& path, const Image8& img);  // binary PGM
// <folder>/%08d with the first existing extension of .jpg .jpeg .JPG .ppm .pgm ("" if none)
std::string FindImageFile(const std::string& image_folder, int id);
Image8 ResizeLinear8(const Image8& src, int new_cols, int new_rows);
// reference SkySegment/include/SkyRegionDetect.h:43 bilateral_filter(img, mask_, result): the coarse probability mask is resized
// to the image (cv::resize INTER_LINEAR, SkyRegionDetect.cu:40-41) and refined on the GPU (mpmvs_sky_bilateral); result = 255 / 0
bool bilateral_filter(const Image8& img_bgr, const Image& mask, Image& result, int device = 0);
// reference GenerateSkyRegionMask (src/PatchMatch.cpp:4-57) without the segmentation network: for every image reads the
// network's output as the reference stores it, <input>/MPMVS/2333_<id>/skymask.{jpg,pgm} (8 bit = 255 x probability), resizes
// image and mask as :21-34 do, refines, and writes skymask_refine.pgm (0 / 255) beside it.  Returns the number of masks written or -1.
int RefineSkyMasks(const std::string& input_folder, const std::vector<Scene>& Scenes, int max_image_size, int device = 0);
// cv::pyrDown(src, dst, Size(cols / 2, rows / 2)) for 8-bit images (5x5 binomial, reflect-101, (s + 128) >> 8)
Image8 PyrDown8(const Image8& src);
// the input of the segmentation network for a B,G,R image, stated on the host (what mpmvs_skyseg_run_u8 computes on the device, bit
// for bit): pyrDown while rows > 768 && cols > 768, ResizeLinear8 to the network's size, R,G,B planes, (v - mean) * norm.
// Returns 3 * net_rows rows of net_cols floats (the planes one below the other).
Image SkyPreprocess(const Image8& bgr, int net_rows, int net_cols);
// reference SkySegment/include/SkyRegionDetect.h SkySegment(param, model) / maskExtractor(bgr): the network runs on the GPU
// (mpmvs_skyseg_*, csrc/pm_skyseg.hpp) instead of ncnn on the CPU.  maskExtractor returns the 384 x 384 sky probability
// (empty on failure) and includes the pyrDown loop of the caller (src/PatchMatch.cpp:16-18), which the device does.
class SkySegment {
public:
    SkySegment(const char* param, const char* model, int device = 0);
    ~SkySegment();
    SkySegment(const SkySegment&) = delete;
    SkySegment& operator=(const SkySegment&) = delete;
    bool ok() const { return net_ != nullptr; }
    Image maskExtractor(const Image8& bgr);

private:
    mpmvs_skyseg* net_ = nullptr;
};
// reference GenerateSkyRegionMask (src/PatchMatch.cpp:4-57) in full: network, resize of the fp32 probability and of the image
// (:21-35), refinement of the fp32 mask (:47); writes <input>/MPMVS/2333_<id>/skymask.pgm (255 x probability, :44) and
// skymask_refine.pgm (0 / 255); skymask_fuse.jpg is a visualisation and is not written.  model_dir holds
// skysegsmall_sim-opt-fp16.{param,bin}.  Returns the number of images done or -1.
int GenerateSkyRegionMask(const std::string& input_folder, const std::vector<Scene>& Scenes, const std::string& model_dir, int max_image_size, int device = 0);
// The pass loops of the reference's main() (src/main.cpp:20-41) over a dataset folder in the JACOBI order of DESIGN.md
// section 7: every Problem of a pass reads the previous pass's maps (kept in memory), so the Problems of a pass are
// independent and are processed by `workers` host threads dealt round-robin to `devices` -- the Delaunay / file work of
// one Problem overlaps the kernels of others, and several GPUs are used from one process.  Results do not depend on
// workers or devices, and equal SceneScheduler's (mp-mvs_amd/schedule.py).  Writes the same depths/normals/costs.dmb files.
// in_memory (optional): no result files are written; the final maps of every estimated image are handed over instead.
// fuse (optional): the reference's last step (RunFusion, src/main.cpp:49) at the end of the schedule, while the Problems' contexts are
// still resident: their final maps are fused straight out of HBM (RunFusion with resident = true) into <input>/MPMVS/MPMVS_model.ply.
struct FuseAtEnd {
    bool use_dynamic_consistency = true;
    bool sky_seg = false;
    bool write_vis = false;   // also write MPMVS_model.ply.vis (RunFusion)
    int device = 0;
    long points = -1;   // out: number of fused points (-1: fusion failed)
};
int RunFolderJacobi(const std::string& input_folder, int max_src, int max_image_size, int geom_iterations, bool planar_prior,
                    bool geomPlanarPrior, int max_scale, uint64_t seed, const std::vector<int>& devices, int workers,
                    std::vector<ProblemResult>* in_memory = nullptr, FuseAtEnd* fuse = nullptr);
void ProcessProblem(const std::string& input_folder, const std::string& output_folder, std::vector<Scene>& Scenes, const int ID,
                    bool geom_consistency, bool planar_prior, uint64_t seed = 0, int device = 0, int max_scale = 2);

#endif
