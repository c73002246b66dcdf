// scene_io.cpp -- the on-disk formats either side of the hot path:
//   DMB maps      reference src/utility.cpp:193-308   (int32 type=1, h, w, nb; h*w*nb fp32, row-major)
//   *_cam.txt     reference src/PatchMatch.cpp:109-143 (ReadCamera)
//   pair.txt      reference src/PatchMatch.cpp:67-107  (GenerateSampleList)
// and the file-based ProcessProblem of the reference (src/PatchMatch.cpp:506-638):
// reads images + cameras (+ the previous pass's depths/normals/costs.dmb for
// geometric consistency), runs the in-memory ProcessProblem, writes
// depths.dmb / normals.dmb / costs.dmb under <output>/2333_<id>.
// Images: the reference reads <input>/images/%08d.jpg through OpenCV; here the same
// files are read by the decoder of jpeg_decode.h (row f-3); binary PGM / PPM files of
// the same name are accepted as well.
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>

#include <cmath>

#include "PatchMatch.h"
#include "jpeg_decode.h"
#include "scene_io.h"

// ---------------------------------------------------------------------------
// DMB
// ---------------------------------------------------------------------------
static bool read_dmb(const std::string& path, Image& img, int channels) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        std::cout << "Error opening file " << path << std::endl;
        return false;
    }
    int32_t type = -1, h = 0, w = 0, nb = 0;
    bool ok = fread(&type, 4, 1, f) == 1 && fread(&h, 4, 1, f) == 1 && fread(&w, 4, 1, f) == 1 && fread(&nb, 4, 1, f) == 1;
    if (!ok || type != 1 || h <= 0 || w <= 0 || nb != channels) {
        fclose(f);
        return false;
    }
    img = Image::Uninitialized(h, w, channels);   // filled by the read below
    ok = fread(img.data.data(), sizeof(float), (size_t)h * w * nb, f) == (size_t)h * w * nb;
    fclose(f);
    return ok;
}

static int write_dmb(const std::string& path, const Image& img) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        std::cout << "Error opening file " << path << std::endl;
        return -1;
    }
    const int32_t hdr[4] = {1, img.rows, img.cols, img.ch};
    fwrite(hdr, 4, 4, f);
    fwrite(img.data.data(), sizeof(float), img.data.size(), f);
    fclose(f);
    return 0;
}

bool readDepthDmb(const std::string file_path, Image& depth) { return read_dmb(file_path, depth, 1); }
int writeDepthDmb(const std::string file_path, const Image& depth) { return write_dmb(file_path, depth); }
bool readNormalDmb(const std::string file_path, Image& normal) { return read_dmb(file_path, normal, 3); }
int writeNormalDmb(const std::string file_path, const Image& normal) { return write_dmb(file_path, normal); }

// ---------------------------------------------------------------------------
// cameras and the Problem list
// ---------------------------------------------------------------------------
// `<id>_cam.txt` (MVSNet layout): the keyword "extrinsic" followed by a 4x4 world-to-camera matrix [R t; 0 0 0 1],
// the keyword "intrinsic" followed by the 3x3 K, then "depth_min interval depth_num depth_max".  The camera centre
// C = -R^T t is derived here as the reference does when it loads a camera.
namespace {
struct CamTokens {
    std::ifstream in;
    std::string path;
    void expect_word(const char* word) {
        std::string w;
        if (!(in >> w) || w != word) die("missing section '" + std::string(word) + "'");
    }
    float number() {
        float v;
        if (!(in >> v)) die("number expected");
        return v;
    }
    [[noreturn]] void die(const std::string& why) const {
        std::cout << "camera file " << path << ": " << why << std::endl;
        exit(1);
    }
};
}  // namespace

Camera ReadCamera(const std::string& cam_path) {
    CamTokens tk;
    tk.path = cam_path;
    tk.in.open(cam_path);
    if (!tk.in.is_open()) tk.die("cannot be opened");
    Camera cam{};
    tk.expect_word("extrinsic");
    for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) {
            const float v = tk.number();
            if (row < 3 && col < 3) cam.R[3 * row + col] = v;
            if (row < 3 && col == 3) cam.t[row] = v;
        }
    tk.expect_word("intrinsic");
    for (int k = 0; k < 9; ++k) cam.K[k] = tk.number();
    for (int k = 0; k < 3; ++k) cam.C[k] = -(cam.R[k] * cam.t[0] + cam.R[3 + k] * cam.t[1] + cam.R[6 + k] * cam.t[2]);
    cam.depth_min = tk.number();
    (void)tk.number();  // depth interval
    (void)tk.number();  // number of depth planes
    cam.depth_max = tk.number();
    return cam;
}

// `pair.txt`: the number of entries, then per entry the reference image id and a line "n id_0 score_0 ...
// id_{n-1} score_{n-1}" of candidate source views, best first.  Scene k describes image k: ids that pair.txt skips get a
// placeholder that is never estimated.  A candidate is kept when its score is positive and its POSITION in the list is
// below maxSourceImageNum (the position counts dropped candidates too, as in the reference); srcID[0] is the image itself.
// An id outside [0, number of scenes) -- a malformed file; the reference would index out of bounds -- is dropped with a
// warning, so that every srcID can be used as an index by the passes and by the fusion.
void GenerateSampleList(const std::string& input_folder, int maxSourceImageNum, int maxImageSize, std::vector<Scene>& Scenes) {
    Scenes.clear();
    const std::string list_path = input_folder + "/pair.txt";
    std::ifstream in(list_path);
    if (!in.is_open()) {
        std::cout << "view list " << list_path << " cannot be opened" << std::endl;
        exit(1);
    }
    int entries = 0;
    in >> entries;
    for (int e = 0; e < entries; ++e) {
        int ref = -1, listed = 0;
        if (!(in >> ref >> listed) || ref < (int)Scenes.size()) {
            std::cout << "view list " << list_path << ": entry " << e << " is malformed (ids must ascend)" << std::endl;
            exit(1);
        }
        Scene placeholder;
        placeholder.estimate = false;
        Scenes.resize((size_t)ref, placeholder);
        Scene sc;
        sc.max_image_size = maxImageSize;
        sc.refID = ref;
        sc.estimate = listed != 0;
        sc.srcID.assign(1, ref);
        for (int pos = 0; pos < listed; ++pos) {
            int id = -1;
            float score = 0.0f;
            in >> id >> score;
            if (score > 0.0f && pos < maxSourceImageNum) sc.srcID.push_back(id);
        }
        Scenes.push_back(sc);
    }
    const int n = (int)Scenes.size();
    for (Scene& sc : Scenes) {
        std::vector<int> kept;
        for (int id : sc.srcID) {
            if (id >= 0 && id < n)
                kept.push_back(id);
            else
                std::cerr << "view list " << list_path << ": image " << sc.refID << " names source " << id << ", which does not exist; dropped" << std::endl;
        }
        sc.srcID.swap(kept);
    }
}

// ---------------------------------------------------------------------------
// images: JPEG through the own decoder, or binary PGM / PPM
// ---------------------------------------------------------------------------
static bool read_file(const std::string& path, std::vector<unsigned char>& buf) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n > 0 && fread(buf.data(), 1, buf.size(), f) == buf.size();
    fclose(f);
    return ok;
}

// binary PNM body: P5 (1 channel) or P6 (3 channels, R,G,B), maxval 255
static bool parse_pnm(const std::vector<unsigned char>& buf, Image8& img) {
    if (buf.size() < 7 || buf[0] != 'P' || (buf[1] != '5' && buf[1] != '6')) return false;
    size_t i = 2;
    auto next_int = [&](int& v) {
        while (i < buf.size() && (buf[i] == '#' || buf[i] == ' ' || buf[i] == '\n' || buf[i] == '\r' || buf[i] == '\t')) {
            if (buf[i] == '#')
                while (i < buf.size() && buf[i] != '\n') ++i;
            else
                ++i;
        }
        if (i >= buf.size() || buf[i] < '0' || buf[i] > '9') return false;
        v = 0;
        while (i < buf.size() && buf[i] >= '0' && buf[i] <= '9') v = v * 10 + (buf[i++] - '0');
        return true;
    };
    int w = 0, h = 0, maxv = 0;
    if (!next_int(w) || !next_int(h) || !next_int(maxv) || maxv != 255 || w <= 0 || h <= 0) return false;
    ++i;  // the single whitespace after maxval
    const int ch = buf[1] == '6' ? 3 : 1;
    const size_t need = (size_t)w * h * ch;
    if (i + need > buf.size()) return false;
    img.rows = h;
    img.cols = w;
    img.ch = ch;
    img.data.assign(buf.begin() + i, buf.begin() + i + need);
    return true;
}

static bool read_image8(const std::string& path, int channels, Image8& img) {
    std::vector<unsigned char> buf;
    if (!read_file(path, buf)) return false;
    if (buf.size() > 2 && buf[0] == 0xFF && buf[1] == 0xD8) {
        std::string err;
        int w = 0, h = 0;
        if (!DecodeJpeg(buf.data(), buf.size(), channels, img.data, w, h, err)) {
            std::cout << "JPEG decode failed for " << path << ": " << err << std::endl;
            return false;
        }
        img.rows = h;
        img.cols = w;
        img.ch = channels;
        return true;
    }
    Image8 raw;
    if (!parse_pnm(buf, raw)) return false;
    const size_t n = (size_t)raw.rows * raw.cols;
    img.rows = raw.rows;
    img.cols = raw.cols;
    img.ch = channels;
    if (raw.ch == channels) {
        img.data.swap(raw.data);
        if (channels == 3)  // P6 is R,G,B
            for (size_t k = 0; k < n; ++k) std::swap(img.data[3 * k], img.data[3 * k + 2]);
    } else if (channels == 3) {
        img.data.resize(n * 3);
        for (size_t k = 0; k < n; ++k) img.data[3 * k] = img.data[3 * k + 1] = img.data[3 * k + 2] = raw.data[k];
    } else {
        // OpenCV's 8-bit BGR2GRAY: (B*1868 + G*9617 + R*4899 + 8192) >> 14
        img.data.resize(n);
        for (size_t k = 0; k < n; ++k)
            img.data[k] = (unsigned char)((raw.data[3 * k + 2] * 1868 + raw.data[3 * k + 1] * 9617 + raw.data[3 * k] * 4899 + 8192) >> 14);
    }
    return true;
}

bool readGrayImage(const std::string& path, Image& img) {
    Image8 g;
    if (!read_image8(path, 1, g)) return false;
    img = Image::Uninitialized(g.rows, g.cols, 1);
    for (size_t i = 0; i < g.data.size(); ++i) img.data[i] = (float)g.data[i];  // convertTo(CV_32FC1), reference :882
    return true;
}

bool readGrayImage8(const std::string& path, Image8& img) { return read_image8(path, 1, img); }

bool readSceneImage(const std::string& path, Scene& s) {
    const char* e = std::getenv("MPMVS_HOST_FLOAT_IMAGES");
    s.target_cols = s.target_rows = 0;
    if (e && std::atoi(e) != 0) {
        s.image8 = Image8();
        return readGrayImage(path, s.image);
    }
    s.image = Image();
    return readGrayImage8(path, s.image8);
}

bool readColorImage(const std::string& path, Image8& bgr) { return read_image8(path, 3, bgr); }

bool writeGrayImage(const std::string& path, const Image8& img) {
    if (img.ch != 1) return false;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P5\n%d %d\n255\n", img.cols, img.rows);
    const bool ok = fwrite(img.data.data(), 1, img.data.size(), f) == img.data.size();
    fclose(f);
    return ok;
}

// cv::resize(INTER_LINEAR) of an 8-bit image: channel-wise through the fp32 ResizeLinear, rounded to nearest
// (OpenCV's 8-bit path uses 11-bit fixed-point weights; the two can differ by one grey level)
Image8 ResizeLinear8(const Image8& src, int new_cols, int new_rows) {
    Image8 out;
    out.rows = new_rows;
    out.cols = new_cols;
    out.ch = src.ch;
    out.data.resize((size_t)new_rows * new_cols * src.ch);
    for (int k = 0; k < src.ch; ++k) {
        Image plane(src.rows, src.cols, 1);
        for (size_t i = 0; i < plane.data.size(); ++i) plane.data[i] = (float)src.data[i * src.ch + k];
        const Image r = ResizeLinear(plane, new_cols, new_rows);
        for (size_t i = 0; i < r.data.size(); ++i) {
            const float v = std::nearbyintf(r.data[i]);
            out.data[i * src.ch + k] = (unsigned char)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v);
        }
    }
    return out;
}

static std::string id8(int id) {
    std::stringstream s;
    s << std::setw(8) << std::setfill('0') << id;
    return s.str();
}

static std::string find_with_ext(const std::string& stem) {
    for (const char* ext : {".jpg", ".jpeg", ".JPG", ".ppm", ".pgm"}) {
        struct stat st;
        if (stat((stem + ext).c_str(), &st) == 0) return stem + ext;
    }
    return "";
}

std::string FindImageFile(const std::string& image_folder, int id) { return find_with_ext(image_folder + "/" + id8(id)); }

// reference src/PatchMatch.cpp:506-638 with its file traffic
void ProcessProblem(const std::string& input_folder, const std::string& output_folder, std::vector<Scene>& Scenes, const int ID,
                    bool geom_consistency, bool planar_prior, uint64_t seed, int device, int max_scale) {
    Scene& scene = Scenes[ID];
    std::cout << "Processing image " << id8(scene.refID) << " ..." << std::endl;
    const std::string result_folder = output_folder + "/2333_" + id8(scene.refID);
    mkdir(result_folder.c_str(), 0777);
    // PatchMatchInit's file half (reference :871-890, :934-950, :1052-1063)
    for (int sid : scene.srcID) {
        Scene& s = Scenes[sid];
        if (!s.has_image()) {
            if (!readSceneImage(FindImageFile(input_folder + "/images", sid), s)) {
                std::cout << "Can not read this image !" << input_folder + "/images/" + id8(sid) + ".jpg" << std::endl;
                exit(EXIT_FAILURE);
            }
            s.cam = ReadCamera(input_folder + "/cams/" + id8(sid) + "_cam.txt");
        }
        if (geom_consistency) {
            const std::string prev = input_folder + "/MPMVS/2333_" + id8(sid);
            if (!readDepthDmb(prev + "/depths.dmb", s.depth)) {
                std::cout << "Can not read this depth image !" << std::endl;
                exit(EXIT_FAILURE);
            }
            if (sid == scene.refID) {
                if (!readNormalDmb(prev + "/normals.dmb", s.normal) || !readDepthDmb(prev + "/costs.dmb", s.cost)) {
                    std::cout << "Can not read this depth image !" << std::endl;
                    exit(EXIT_FAILURE);
                }
            }
        }
    }
    ProblemResult res;
    ProcessProblem(Scenes, ID, geom_consistency, planar_prior, seed, device, max_scale, &res);
    writeDepthDmb(result_folder + "/depths.dmb", res.depth);
    writeNormalDmb(result_folder + "/normals.dmb", res.normal);
    writeDepthDmb(result_folder + "/costs.dmb", res.cost);
    std::cout << "Processing image " << id8(scene.refID) << " done!" << std::endl;
}

// ---------------------------------------------------------------------------
// Jacobi pass schedule with worker threads (see scene_io.h)
// ---------------------------------------------------------------------------
int RunFolderJacobi(const std::string& input_folder, int max_src, int max_image_size, int geom_iterations, bool planar_prior,
                    bool geomPlanarPrior, int max_scale, uint64_t seed, const std::vector<int>& devices, int workers,
                    std::vector<ProblemResult>* in_memory, FuseAtEnd* fuse) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, max_image_size > 0 ? max_image_size : 3200, Scenes);
    const int n = (int)Scenes.size();
    if (n == 0 || devices.empty()) return -1;
    const std::string out = input_folder + "/MPMVS";
    mkdir(out.c_str(), 0777);
    // every image that is a reference or a source: decode, read its camera, shrink if oversized -- once, in parallel,
    // so that the Problems only READ the Scenes afterwards
    std::vector<char> needed(n, 0);
    for (const Scene& s : Scenes)
        if (s.estimate)
            for (int id : s.srcID)
                if (id >= 0 && id < n) needed[id] = 1;
    std::atomic<bool> ok(true);
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(dynamic, 1)
    for (int i = 0; i < n; ++i) {
        if (!needed[i]) continue;
        Scene& s = Scenes[i];
        if (!readSceneImage(FindImageFile(input_folder + "/images", i), s)) {
            ok = false;
            continue;
        }
        s.cam = ReadCamera(input_folder + "/cams/" + id8(i) + "_cam.txt");
        AdjustImageScale(s);
    }
    if (!ok) {
        std::cout << "Can not read every image of " << input_folder << "/images" << std::endl;
        return -1;
    }
    std::vector<int> todo;
    for (int i = 0; i < n; ++i)
        if (Scenes[i].estimate) todo.push_back(i);
    const int nworkers = std::max(1, std::min(workers, (int)todo.size()));
    // the maps a pass replaces become the storage of the pass after the next (ProcessProblem keeps buffers of the right size):
    // after the first two passes no pass allocates or page-faults fresh result memory
    std::vector<ProblemResult> spare(n);
    mpmvs_host::SetConcurrentCallers(nworkers);
    // Device-side hand-over of the depth maps (round 5; MPMVS_FOLDER_HOST_EXCHANGE=1 keeps the host staging of rounds 1-4): every
    // Problem owns two dense depth buffers on its device.  ProcessProblem exports the map of pass k into one of them while the
    // Problems of pass k still read the maps of pass k - 1 from the other (Jacobi); the barrier swaps them, and the Problems of
    // pass k + 1 copy their source maps out of HBM -- device to device, or GPU to GPU when the source's Problem lives on another
    // device of `devices` (hipMemcpyPeerAsync; that branch has not run anywhere yet: the pool has one-GPU boxes only).
    const bool device_exchange = geom_iterations > 0 && std::getenv("MPMVS_FOLDER_HOST_EXCHANGE") == nullptr;
    std::vector<std::pair<int, float*>> exchange_buffers;   // (device, pointer): released at the end
    if (device_exchange)
        for (size_t k = 0; k < todo.size(); ++k) {
            Scene& s = Scenes[todo[k]];
            const int device = devices[k % devices.size()];
            const size_t bytes = (size_t)s.rows() * s.cols() * sizeof(float);
            for (Scene::DeviceDepth* slot : {&s.device_depth, &s.device_depth_next}) {
                slot->ptr = static_cast<float*>(mpmvs_device_alloc(device, bytes));
                slot->device = device;
                slot->stamp = 0;
                if (slot->ptr) exchange_buffers.push_back({device, slot->ptr});
            }
            if (!s.device_depth.ptr || !s.device_depth_next.ptr) s.device_depth.ptr = s.device_depth_next.ptr = nullptr;   // no memory: this map travels through the host
        }
    auto run_pass = [&](bool geom, bool pp, uint64_t pass_seed) {
        std::vector<ProblemResult> results(n);
        for (int i : todo) results[i] = std::move(spare[i]);
        std::atomic<size_t> next(0);
        auto work = [&](int) {
            for (;;) {
                const size_t k = next.fetch_add(1);
                if (k >= todo.size()) return;
                const int i = todo[k];
                const int device = devices[k % devices.size()];  // fixed per Problem: its context stays resident there between passes
                ProcessProblem(Scenes, i, geom, pp, pass_seed + (uint64_t)i, device, max_scale, &results[i]);
                if (in_memory) continue;  // the caller takes the final maps from memory: no files
                const std::string folder = out + "/2333_" + id8(Scenes[i].refID);
                mkdir(folder.c_str(), 0777);
                writeDepthDmb(folder + "/depths.dmb", results[i].depth);
                writeNormalDmb(folder + "/normals.dmb", results[i].normal);
                writeDepthDmb(folder + "/costs.dmb", results[i].cost);
            }
        };
        std::vector<std::thread> pool;
        for (int w = 1; w < nworkers; ++w) pool.emplace_back(work, w);
        work(0);
        for (std::thread& t : pool) t.join();
        // the barrier of the pass: only now do the new maps become what the next pass reads
        for (int i : todo) {
            std::swap(Scenes[i].depth, results[i].depth);
            std::swap(Scenes[i].normal, results[i].normal);
            std::swap(Scenes[i].cost, results[i].cost);
            spare[i] = std::move(results[i]);  // the maps of the pass before: storage for the pass after the next
            std::swap(Scenes[i].device_depth, Scenes[i].device_depth_next);   // ... and the same hand-over in HBM
        }
    };
    run_pass(false, !geomPlanarPrior && planar_prior, seed);
    for (int g = 0; g < geom_iterations; ++g) run_pass(true, geomPlanarPrior && g != geom_iterations - 1, seed + 100003ull * (g + 1));
    mpmvs_host::SetConcurrentCallers(1);
    for (int i : todo) Scenes[i].device_depth = Scenes[i].device_depth_next = Scene::DeviceDepth();
    for (const auto& b : exchange_buffers) mpmvs_device_free(b.first, b.second);
    // the final maps are still in the Problems' contexts (Release() left them with the Scenes): fuse them from there
    if (fuse) fuse->points = RunFusion(input_folder, out, Scenes, fuse->use_dynamic_consistency, fuse->device, fuse->sky_seg, true, fuse->write_vis);
    if (in_memory) {
        in_memory->assign(n, ProblemResult());
        for (int i : todo) {
            (*in_memory)[i].depth = std::move(Scenes[i].depth);
            (*in_memory)[i].normal = std::move(Scenes[i].normal);
            (*in_memory)[i].cost = std::move(Scenes[i].cost);
        }
    }
    return (int)todo.size();
}

// ---------------------------------------------------------------------------
// binary PLY of fused points (reference src/PatchMatch.cpp:145-198): x y z nx ny nz as
// float32, then red green blue as uchar; the colour triple is stored blue-first in
// PointList::color (OpenCV BGR) and written red-first; non-finite coordinates become 0
// ---------------------------------------------------------------------------
static void WritePlyHeader(FILE* out, size_t n_vertices) {
    fprintf(out, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\n", n_vertices);
    fprintf(out, "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n");
    fprintf(out, "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n");
}

void StoreColorPlyFileBinaryPointCloud(const std::string& plyFilePath, const std::vector<PointList>& pc) {
    std::cout << "store 3D points to ply file" << std::endl;
    FILE* out = fopen(plyFilePath.c_str(), "wb");
    if (!out) {
        std::cout << "Error opening file " << plyFilePath << std::endl;
        return;
    }
    WritePlyHeader(out, pc.size());
    for (const PointList& p : pc) {
        float3 X = p.coord;
        const bool finite = (X.x < FLT_MAX && X.x > -FLT_MAX) && (X.y < FLT_MAX && X.y > -FLT_MAX) && (X.z < FLT_MAX && X.z >= -FLT_MAX);
        if (!finite) X = float3{0.0f, 0.0f, 0.0f};
        const char rgb[3] = {(char)(int)p.color.z, (char)(int)p.color.y, (char)(int)p.color.x};
        fwrite(&X, sizeof(float), 3, out);
        fwrite(&p.normal, sizeof(float), 3, out);
        fwrite(rgb, 1, 3, out);
    }
    fclose(out);
}

// ---------------------------------------------------------------------------
// sky masks (reference src/PatchMatch.cpp:4-57, SkySegment/src/SkyRegionDetect.cu:36-66)
// ---------------------------------------------------------------------------
bool bilateral_filter(const Image8& img, const Image& mask, Image& result, int device) {
    if (img.ch != 3 || img.empty() || mask.empty()) return false;
    const Image m2 = (mask.rows != img.rows || mask.cols != img.cols) ? ResizeLinear(mask, img.cols, img.rows) : mask;
    result = Image(img.rows, img.cols, 1);
    return mpmvs_sky_bilateral(device, img.data.data(), m2.data.data(), result.data.data(), img.rows, img.cols) == 0;
}

int RefineSkyMasks(const std::string& input_folder, const std::vector<Scene>& Scenes, int max_image_size, int device) {
    int written = 0;
    for (const Scene& s : Scenes) {
        Image8 bgr, coarse8;
        if (!readColorImage(FindImageFile(input_folder + "/images", s.refID), bgr)) return -1;
        const std::string res = input_folder + "/MPMVS/2333_" + id8(s.refID);
        const std::string coarse_file = find_with_ext(res + "/skymask");
        if (coarse_file.empty() || !read_image8(coarse_file, 1, coarse8)) {
            std::cout << "Can not read the coarse sky mask " << res << "/skymask.*" << std::endl;
            return -1;
        }
        int w = bgr.cols, h = bgr.rows;
        if (bgr.cols > max_image_size || bgr.rows > max_image_size) {  // reference :24-32
            const float factor = std::min((float)max_image_size / bgr.cols, (float)max_image_size / bgr.rows);
            w = (int)std::round(bgr.cols * factor);
            h = (int)std::round(bgr.rows * factor);
            bgr = ResizeLinear8(bgr, w, h);
        }
        Image coarse(coarse8.rows, coarse8.cols, 1);
        for (size_t i = 0; i < coarse.data.size(); ++i) coarse.data[i] = (float)coarse8.data[i] / 255.0f;  // the file holds 255 * probability (:44)
        Image refined;
        if (!bilateral_filter(bgr, coarse, refined, device)) return -1;
        Image8 out;
        out.rows = h;
        out.cols = w;
        out.ch = 1;
        out.data.resize(refined.data.size());
        for (size_t i = 0; i < refined.data.size(); ++i) out.data[i] = refined.data[i] > 0.0f ? 255 : 0;
        mkdir((input_folder + "/MPMVS").c_str(), 0777);
        mkdir(res.c_str(), 0777);
        if (!writeGrayImage(res + "/skymask_refine.pgm", out)) return -1;
        ++written;
    }
    return written;
}

// ---------------------------------------------------------------------------
// the segmentation network in front of the refinement (reference src/PatchMatch.cpp:4-57, SkySegment/src/SkyRegionDetect.cpp:541-561)
// ---------------------------------------------------------------------------
static int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// cv::pyrDown(src, dst, Size(cols / 2, rows / 2)) of an 8-bit image: 5x5 binomial [1 4 6 4 1]^2 / 256 around (2x, 2y),
// reflect-101 border, (s + 128) >> 8.  Restated from OpenCV's documented behaviour, not pinned against its output.
Image8 PyrDown8(const Image8& src) {
    Image8 out;
    out.rows = src.rows / 2;
    out.cols = src.cols / 2;
    out.ch = src.ch;
    out.data.resize((size_t)out.rows * out.cols * out.ch);
    static const int kw[5] = {1, 4, 6, 4, 1};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < out.rows; ++y)
        for (int x = 0; x < out.cols; ++x)
            for (int c = 0; c < src.ch; ++c) {
                int s = 0;
                for (int j = 0; j < 5; ++j) {
                    const int yy = reflect101(2 * y + j - 2, src.rows);
                    int row = 0;
                    for (int k = 0; k < 5; ++k) row += kw[k] * (int)src.data[((size_t)yy * src.cols + reflect101(2 * x + k - 2, src.cols)) * src.ch + c];
                    s += kw[j] * row;
                }
                out.data[((size_t)y * out.cols + x) * out.ch + c] = (unsigned char)((s + 128) >> 8);
            }
    return out;
}

// What mpmvs_skyseg_run_u8 feeds the network, stated on the host: the pyrDown loop (src/PatchMatch.cpp:16-18), the resize to the
// network's size with ResizeLinear8 (ncnn's from_pixels_resize resizes the bytes; its fixed-point coefficients are not
// reproduced: parity unpinned), B,G,R -> R,G,B planes, (v - mean) * norm (SkyRegionDetect.cpp:627-630).  3 planes, planar.
Image SkyPreprocess(const Image8& bgr, int net_rows, int net_cols) {
    Image8 img = bgr;
    while (img.rows > 768 && img.cols > 768) img = PyrDown8(img);
    const Image8 small = (img.rows != net_rows || img.cols != net_cols) ? ResizeLinear8(img, net_cols, net_rows) : img;
    const float mean_vals[3] = {0.485f * 255.f, 0.456f * 255.f, 0.406f * 255.f};
    const float norm_vals[3] = {1 / 0.229f / 255.f, 1 / 0.224f / 255.f, 1 / 0.225f / 255.f};
    Image out(3 * net_rows, net_cols, 1);  // three planes one below the other
    const size_t hw = (size_t)net_rows * net_cols;
    for (int c = 0; c < 3; ++c)
        for (size_t i = 0; i < hw; ++i) out.data[c * hw + i] = ((float)small.data[i * 3 + (2 - c)] - mean_vals[c]) * norm_vals[c];
    return out;
}

SkySegment::SkySegment(const char* param, const char* model, int device) {
    if (mpmvs_skyseg_load(device, param, model, 384, 384, "1959", &net_) != 0) {  // input size and output blob: SkyRegionDetect.cpp:627,636
        std::cout << "SkySegment: " << mpmvs_last_error(nullptr) << std::endl;
        net_ = nullptr;
    }
}
SkySegment::~SkySegment() {
    if (net_) mpmvs_skyseg_destroy(net_);
}
Image SkySegment::maskExtractor(const Image8& bgr) {
    Image out;
    if (!net_ || bgr.ch != 3 || bgr.empty()) return out;
    out = Image(384, 384, 1);
    if (mpmvs_skyseg_run_u8(net_, bgr.data.data(), bgr.rows, bgr.cols, 0, out.data.data()) != 0) {
        std::cout << "SkySegment: " << mpmvs_last_error(nullptr) << std::endl;
        return Image();
    }
    return out;
}

int GenerateSkyRegionMask(const std::string& input_folder, const std::vector<Scene>& Scenes, const std::string& model_dir, int max_image_size, int device) {
    const std::string stem = model_dir + "/skysegsmall_sim-opt-fp16";  // the file names of the reference (src/PatchMatch.cpp:5-6)
    SkySegment Skyseg((stem + ".param").c_str(), (stem + ".bin").c_str(), device);
    if (!Skyseg.ok()) return -1;
    int written = 0;
    for (const Scene& s : Scenes) {
        Image8 bgr;
        if (!readColorImage(FindImageFile(input_folder + "/images", s.refID), bgr)) return -1;
        const Image prob = Skyseg.maskExtractor(bgr);  // runs the pyrDown loop of :16-18 on the device
        if (prob.empty()) return -1;
        int w = bgr.cols, h = bgr.rows;
        if (bgr.cols > max_image_size || bgr.rows > max_image_size) {  // :24-32
            const float factor = std::min((float)max_image_size / bgr.cols, (float)max_image_size / bgr.rows);
            w = (int)std::round(bgr.cols * factor);
            h = (int)std::round(bgr.rows * factor);
            bgr = ResizeLinear8(bgr, w, h);
        }
        const Image mask = ResizeLinear(prob, w, h);  // :34, the fp32 mask: the reference refines it as it is and only STORES 8 bits
        Image refined;
        if (!bilateral_filter(bgr, mask, refined, device)) return -1;
        Image8 coarse8, out;
        coarse8.rows = out.rows = h;
        coarse8.cols = out.cols = w;
        coarse8.ch = out.ch = 1;
        coarse8.data.resize(mask.data.size());
        out.data.resize(refined.data.size());
        for (size_t i = 0; i < mask.data.size(); ++i) {  // 255 * mask, saturate-rounded (:44)
            const float v = std::nearbyintf(255.0f * mask.data[i]);
            coarse8.data[i] = (unsigned char)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v);
        }
        for (size_t i = 0; i < refined.data.size(); ++i) out.data[i] = refined.data[i] > 0.0f ? 255 : 0;
        const std::string res = input_folder + "/MPMVS/2333_" + id8(s.refID);
        mkdir((input_folder + "/MPMVS").c_str(), 0777);
        mkdir(res.c_str(), 0777);
        if (!writeGrayImage(res + "/skymask.pgm", coarse8) || !writeGrayImage(res + "/skymask_refine.pgm", out)) return -1;
        ++written;
    }
    return written;
}

// ---------------------------------------------------------------------------
// RunFusion over a dataset folder (reference src/PatchMatch.cpp:287-504): reads every
// estimated image's depths.dmb / normals.dmb, camera and colour image (B,G,R), and with
// sky_seg its skymask_refine image (:360-372, :385-388), fuses them on the GPU (mpmvs_fuse,
// the snapshot formulation of DESIGN.md section 8) and writes <output>/MPMVS_model.ply.
// Returns the number of points, or -1.
// ---------------------------------------------------------------------------
// MPMVS_FUSE_ORDER=reference selects the reference's sequential masking order (a parallel fixpoint on the device, include/mpmvs.h
// MPMVS_FUSE_REFERENCE_ORDER) instead of the default snapshot formulation
static bool fuse_reference_order() {
    const char* e = std::getenv("MPMVS_FUSE_ORDER");
    return e && std::string(e) == "reference";
}

// COLMAP's point-visibility file (little endian: uint64 number of points, per point uint32 k and k x uint32 image id) from the
// tracks of mpmvs_fuse_ply_tracks; the id written for image index i is Scenes[i].refID, the number pair.txt gives the image
static bool write_vis_file(const std::string& path, long long count, const long long* off, const int32_t* image, const std::vector<Scene>& Scenes) {
    FILE* out = fopen(path.c_str(), "wb");
    if (!out) return false;
    auto put32 = [&](uint32_t v) {
        const unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
        return fwrite(b, 1, 4, out) == 4;
    };
    const uint64_t n = (uint64_t)count;
    bool ok = put32((uint32_t)n) && put32((uint32_t)(n >> 32));
    for (long long p = 0; p < count && ok; ++p) {
        ok = put32((uint32_t)(off[p + 1] - off[p]));
        for (long long e = off[p]; e < off[p + 1] && ok; ++e) ok = put32((uint32_t)Scenes[(size_t)image[e]].refID);
    }
    return (fclose(out) == 0) && ok;
}

long RunFusion(const std::string& input_folder, const std::string& output_folder, std::vector<Scene>& Scenes, bool use_dynamic_consistency, int device,
               bool sky_seg, bool resident, bool write_vis) {
    const int n = (int)Scenes.size();
    std::vector<Camera> cams(n);
    std::vector<int> estimate(n, 0), src_off(1, 0), src_ids;
    std::vector<Image> depths(n), normals(n);
    std::vector<Image8> colors(n), sky(n);
    std::vector<mpmvs_ctx*> ctxs(n, nullptr);
    std::vector<const float*> dp(n, nullptr), np_(n, nullptr);
    for (int i = 0; i < n; ++i) {
        Scene& s = Scenes[i];
        if (s.estimate) {
            std::cout << "Reading image " << id8(i) << "..." << std::endl;
            const std::string res = input_folder + "/MPMVS/2333_" + id8(s.refID);
            if (resident) {
                // the maps the pass schedule left in memory -- and in HBM, where the Problem's context still holds exactly them
                if (s.depth.empty() || s.normal.empty() || s.normal.rows != s.depth.rows || s.normal.cols != s.depth.cols) return -1;
                ctxs[i] = ResidentResultContext(s, device);
                depths[i].rows = s.depth.rows, depths[i].cols = s.depth.cols;   // sizes only: the samples stay with the Scene
                dp[i] = s.depth.data.data();
                np_[i] = s.normal.data.data();
            } else {
                if (!readDepthDmb(res + "/depths.dmb", depths[i]) || !readNormalDmb(res + "/normals.dmb", normals[i])) return -1;
                dp[i] = depths[i].data.data();
                np_[i] = normals[i].data.data();
            }
            if (!readColorImage(FindImageFile(input_folder + "/images", s.refID), colors[i])) return -1;
            cams[i] = ReadCamera(input_folder + "/cams/" + id8(s.refID) + "_cam.txt");
            if (colors[i].rows != depths[i].rows || colors[i].cols != depths[i].cols) {  // RescaleImageAndCamera, reference :262-284
                const float sx = depths[i].cols / (float)colors[i].cols, sy = depths[i].rows / (float)colors[i].rows;
                colors[i] = ResizeLinear8(colors[i], depths[i].cols, depths[i].rows);
                cams[i].K[0] *= sx;
                cams[i].K[2] *= sx;
                cams[i].K[4] *= sy;
                cams[i].K[5] *= sy;
            }
            if (sky_seg) {
                Image8 m;
                const std::string mask_file = find_with_ext(res + "/skymask_refine");
                if (mask_file.empty() || !read_image8(mask_file, 1, m)) {
                    std::cout << "Can not read the sky mask of image " << id8(s.refID) << std::endl;
                    return -1;
                }
                sky[i] = (m.rows != depths[i].rows || m.cols != depths[i].cols) ? ResizeLinear8(m, depths[i].cols, depths[i].rows) : m;
            }
            cams[i].width = depths[i].cols;
            cams[i].height = depths[i].rows;
            estimate[i] = 1;
            for (int id : s.srcID) src_ids.push_back(id);
        } else {  // placeholder image (reference :314-322): 1x1, never estimated, never a source
            cams[i] = Camera{};
            cams[i].width = cams[i].height = 1;
            depths[i] = Image(1, 1, 1);
            normals[i] = Image(1, 1, 3);
            dp[i] = depths[i].data.data();
            np_[i] = normals[i].data.data();
            colors[i].rows = colors[i].cols = 1;
            colors[i].ch = 3;
            colors[i].data.assign(3, 0);
            src_ids.push_back(i);
        }
        src_off.push_back((int)src_ids.size());
    }
    std::vector<const unsigned char*> gp(n), sp(n, nullptr);
    for (int i = 0; i < n; ++i) {
        gp[i] = colors[i].data.data();
        if (!sky[i].empty()) sp[i] = sky[i].data.data();
    }
    // the points come back compacted as PLY vertex records (what StoreColorPlyFileBinaryPointCloud would write for the
    // reference's PointCloud vector): only they cross PCIe
    unsigned char* records = nullptr;
    const int fuse_flags = (use_dynamic_consistency ? MPMVS_FUSE_DYNAMIC_CONSISTENCY : 0) | (fuse_reference_order() ? MPMVS_FUSE_REFERENCE_ORDER : 0);
    long long* track_off = nullptr;
    int32_t *track_image = nullptr, *track_pixel = nullptr;
    const long long count = write_vis ? mpmvs_fuse_ply_tracks(device, n, cams.data(), estimate.data(), resident ? ctxs.data() : nullptr, dp.data(), np_.data(),
                                                              gp.data(), 3, sky_seg ? sp.data() : nullptr, src_off.data(), src_ids.data(), fuse_flags, &records,
                                                              &track_off, &track_image, &track_pixel, nullptr)
                            : resident ? mpmvs_fuse_ply_ctx(device, n, cams.data(), estimate.data(), ctxs.data(), dp.data(), np_.data(), gp.data(), 3,
                                                          sky_seg ? sp.data() : nullptr, src_off.data(), src_ids.data(), fuse_flags, &records, nullptr)
                                      : mpmvs_fuse_ply(device, n, cams.data(), estimate.data(), dp.data(), np_.data(), gp.data(), 3, sky_seg ? sp.data() : nullptr,
                                                       src_off.data(), src_ids.data(), fuse_flags, &records, nullptr);
    if (count < 0) return -1;
    std::cout << "store 3D points to ply file" << std::endl;
    const std::string ply = output_folder + "/MPMVS_model.ply";
    FILE* out = fopen(ply.c_str(), "wb");
    if (!out) {
        std::cout << "Error opening file " << ply << std::endl;
        mpmvs_free(records);
        mpmvs_free(track_off);
        mpmvs_free(track_image);
        mpmvs_free(track_pixel);
        return -1;
    }
    WritePlyHeader(out, (size_t)count);
    bool ok = fwrite(records, 27, (size_t)count, out) == (size_t)count;
    fclose(out);
    mpmvs_free(records);
    if (write_vis) {
        ok = ok && write_vis_file(ply + ".vis", count, track_off, track_image, Scenes);
        mpmvs_free(track_off);
        mpmvs_free(track_image);
        mpmvs_free(track_pixel);
    }
    return ok ? (long)count : -1;
}

// ---------------------------------------------------------------------------
// C entry points for the tests
// ---------------------------------------------------------------------------
extern "C" {
int mpmvs_host_write_dmb(const char* path, const float* data, int h, int w, int nb) {
    Image img(h, w, nb);
    std::memcpy(img.data.data(), data, img.data.size() * sizeof(float));
    return write_dmb(path, img);
}
// returns 0 and fills h, w, nb (and data when non-null and large enough), or -1
int mpmvs_host_read_dmb(const char* path, float* data, size_t capacity_floats, int* h, int* w, int* nb) {
    for (int ch = 1; ch <= 3; ch += 2) {
        Image img;
        FILE* f = fopen(path, "rb");
        if (!f) return -1;
        fclose(f);
        if (read_dmb(path, img, ch)) {
            *h = img.rows;
            *w = img.cols;
            *nb = img.ch;
            if (data && capacity_floats >= img.data.size()) std::memcpy(data, img.data.data(), img.data.size() * sizeof(float));
            return 0;
        }
    }
    return -1;
}
// points9: n rows of x y z nx ny nz c0 c1 c2 (colour in PointList order)
int mpmvs_host_write_ply(const char* path, const float* points9, int n) {
    std::vector<PointList> pc((size_t)n);
    for (int i = 0; i < n; ++i) {
        const float* p = points9 + 9 * (size_t)i;
        pc[i].coord = float3{p[0], p[1], p[2]};
        pc[i].normal = float3{p[3], p[4], p[5]};
        pc[i].color = float3{p[6], p[7], p[8]};
    }
    StoreColorPlyFileBinaryPointCloud(path, pc);
    return 0;
}
int mpmvs_host_read_camera(const char* path, mpmvs_camera* out) {
    *out = ReadCamera(path);
    return 0;
}
// pair.txt -> for each scene: estimate flag, refID, number of ids, ids (srcID[0] = refID); flat int array
int mpmvs_host_sample_list(const char* input_folder, int max_src, int max_size, int* out, int cap) {
    std::vector<Scene> S;
    GenerateSampleList(input_folder, max_src, max_size, S);
    int n = 0;
    auto put = [&](int v) {
        if (n < cap) out[n] = v;
        ++n;
    };
    put((int)S.size());
    for (const Scene& s : S) {
        put(s.estimate ? 1 : 0);
        put(s.refID);
        put((int)s.srcID.size());
        for (int id : s.srcID) put(id);
    }
    return n;
}
int mpmvs_host_read_pgm(const char* path, float* data, size_t capacity_floats, int* h, int* w) {
    Image img;
    if (!readGrayImage(path, img)) return -1;
    *h = img.rows;
    *w = img.cols;
    if (data && capacity_floats >= img.data.size()) std::memcpy(data, img.data.data(), img.data.size() * sizeof(float));
    return 0;
}
// the reference's main() pass loops (src/main.cpp:20-41) over a dataset folder, sequentially
// and in place (Gauss-Seidel through the files, as the reference does)
// reference main()'s last step (src/main.cpp:49): fuse the maps of a processed folder into
// <folder>/MPMVS/MPMVS_model.ply; returns the number of points or -1
long mpmvs_host_fuse_folder(const char* input_folder, int device, int max_src, int use_dynamic_consistency, int sky_seg) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, 3200, Scenes);  // RunFusion does not use the image-size limit
    const std::string in = input_folder;
    return RunFusion(in, in + "/MPMVS", Scenes, use_dynamic_consistency != 0, device, sky_seg != 0);
}
// the same, and with write_vis != 0 the points' visibility beside the PLY: <folder>/MPMVS/MPMVS_model.ply.vis (scene_io.h)
long mpmvs_host_fuse_folder_vis(const char* input_folder, int device, int max_src, int use_dynamic_consistency, int sky_seg, int write_vis) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, 3200, Scenes);
    const std::string in = input_folder;
    return RunFusion(in, in + "/MPMVS", Scenes, use_dynamic_consistency != 0, device, sky_seg != 0, false, write_vis != 0);
}
int mpmvs_host_refine_sky_masks(const char* input_folder, int device, int max_src, int max_image_size) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, max_image_size, Scenes);
    return RefineSkyMasks(input_folder, Scenes, max_image_size, device);
}
int mpmvs_host_generate_sky_masks(const char* input_folder, const char* model_dir, int device, int max_src, int max_image_size) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, max_image_size, Scenes);
    return GenerateSkyRegionMask(input_folder, Scenes, model_dir, max_image_size, device);
}
// the host statement of the network's preprocessing (SkyPreprocess) and of one pyrDown level, for the tests; no device involved
int mpmvs_host_sky_preprocess(const unsigned char* bgr, int h, int w, int net_h, int net_w, float* out_chw) {
    if (!bgr || !out_chw || h <= 0 || w <= 0 || net_h <= 0 || net_w <= 0) return -1;
    Image8 img;
    img.rows = h, img.cols = w, img.ch = 3;
    img.data.assign(bgr, bgr + (size_t)h * w * 3);
    const Image r = SkyPreprocess(img, net_h, net_w);
    std::memcpy(out_chw, r.data.data(), r.data.size() * sizeof(float));
    return 0;
}
int mpmvs_host_pyrdown8(const unsigned char* src, int h, int w, int ch, unsigned char* out) {
    if (!src || !out || h < 2 || w < 2 || ch <= 0) return -1;
    Image8 img;
    img.rows = h, img.cols = w, img.ch = ch;
    img.data.assign(src, src + (size_t)h * w * ch);
    const Image8 r = PyrDown8(img);
    std::memcpy(out, r.data.data(), r.data.size());
    return 0;
}
// cv::imread stand-in for the tests: channels 1 (IMREAD_GRAYSCALE) or 3 (IMREAD_COLOR, B,G,R); call with data = NULL for the size
int mpmvs_host_read_image(const char* path, int channels, unsigned char* data, size_t capacity, int* h, int* w) {
    Image8 img;
    if (!(channels == 3 ? readColorImage(path, img) : read_image8(path, 1, img))) return -1;
    *h = img.rows;
    *w = img.cols;
    if (data && capacity >= img.data.size()) std::memcpy(data, img.data.data(), img.data.size());
    return 0;
}
int mpmvs_host_decode_jpeg(const unsigned char* bytes, size_t size, int channels, unsigned char* data, size_t capacity, int* h, int* w) {
    std::vector<unsigned char> px;
    std::string err;
    if (!DecodeJpeg(bytes, size, channels, px, *w, *h, err)) {
        std::cout << "JPEG decode failed: " << err << std::endl;
        return -1;
    }
    if (data && capacity >= px.size()) std::memcpy(data, px.data(), px.size());
    return 0;
}
// devices: n_devices device indices (NULL = device 0); returns the number of Problems per pass or -1
int mpmvs_host_run_folder_jacobi(const char* input_folder, const int* devices, int n_devices, int workers, int max_src, int geom_iterations,
                                 int planar_prior, int geomPlanarPrior, int max_scale, uint64_t seed, int max_image_size) {
    std::vector<int> dev(devices && n_devices > 0 ? std::vector<int>(devices, devices + n_devices) : std::vector<int>{0});
    return RunFolderJacobi(input_folder, max_src, max_image_size, geom_iterations, planar_prior != 0, geomPlanarPrior != 0, max_scale, seed, dev, workers);
}
// the schedule and the reference's last step, RunFusion (src/main.cpp:49), in one call: the final maps are fused out of the Problems'
// resident contexts into <input>/MPMVS/MPMVS_model.ply; write_maps = 0 skips the depths / normals / costs .dmb files.  Returns the
// number of fused points, or a negative value.
long mpmvs_host_run_folder_jacobi_fused(const char* input_folder, const int* devices, int n_devices, int workers, int max_src, int geom_iterations,
                                        int planar_prior, int geomPlanarPrior, int max_scale, uint64_t seed, int max_image_size, int use_dynamic_consistency,
                                        int sky_seg, int write_maps) {
    std::vector<int> dev(devices && n_devices > 0 ? std::vector<int>(devices, devices + n_devices) : std::vector<int>{0});
    std::vector<ProblemResult> res;
    FuseAtEnd fuse;
    fuse.use_dynamic_consistency = use_dynamic_consistency != 0;
    fuse.sky_seg = sky_seg != 0;
    fuse.device = dev[0];
    const int rc = RunFolderJacobi(input_folder, max_src, max_image_size, geom_iterations, planar_prior != 0, geomPlanarPrior != 0, max_scale, seed, dev,
                                   workers, write_maps ? nullptr : &res, &fuse);
    return rc < 0 ? (long)rc : fuse.points;
}
// the same without result files: the final maps of image i go to depth_out[i] (H*W), normal_out[i] (H*W*3), cost_out[i]
// (H*W) for i < n_out (NULL entries are skipped); sizes are the caller's to know (the images' own, shrunk to max_image_size)
int mpmvs_host_run_folder_jacobi_mem(const char* input_folder, const int* devices, int n_devices, int workers, int max_src, int geom_iterations,
                                     int planar_prior, int geomPlanarPrior, int max_scale, uint64_t seed, int max_image_size,
                                     float* const* depth_out, float* const* normal_out, float* const* cost_out, int n_out) {
    std::vector<int> dev(devices && n_devices > 0 ? std::vector<int>(devices, devices + n_devices) : std::vector<int>{0});
    std::vector<ProblemResult> res;
    const int rc = RunFolderJacobi(input_folder, max_src, max_image_size, geom_iterations, planar_prior != 0, geomPlanarPrior != 0, max_scale, seed, dev,
                                   workers, &res);
    if (rc < 0) return rc;
    for (int i = 0; i < n_out && i < (int)res.size(); ++i) {
        if (res[i].depth.empty()) continue;
        if (depth_out && depth_out[i]) std::memcpy(depth_out[i], res[i].depth.data.data(), res[i].depth.data.size() * sizeof(float));
        if (normal_out && normal_out[i]) std::memcpy(normal_out[i], res[i].normal.data.data(), res[i].normal.data.size() * sizeof(float));
        if (cost_out && cost_out[i]) std::memcpy(cost_out[i], res[i].cost.data.data(), res[i].cost.data.size() * sizeof(float));
    }
    return rc;
}
int mpmvs_host_run_folder(const char* input_folder, int device, int max_src, int geom_iterations, int planar_prior,
                          int geomPlanarPrior, int max_scale, uint64_t seed, int max_image_size) {
    std::vector<Scene> Scenes;
    GenerateSampleList(input_folder, max_src, max_image_size > 0 ? max_image_size : 3200, Scenes);
    const std::string in = input_folder, out = in + "/MPMVS";
    mkdir(out.c_str(), 0777);
    bool pp = !geomPlanarPrior && planar_prior;
    for (size_t i = 0; i < Scenes.size(); ++i)
        if (Scenes[i].estimate) ProcessProblem(in, out, Scenes, (int)i, false, pp, seed + i, device, max_scale);
    for (int g = 0; g < geom_iterations; ++g) {
        pp = geomPlanarPrior && g != geom_iterations - 1;
        for (size_t i = 0; i < Scenes.size(); ++i)
            if (Scenes[i].estimate) ProcessProblem(in, out, Scenes, (int)i, true, pp, seed + 100003ull * (g + 1) + i, device, max_scale);
    }
    return 0;
}
}  // extern "C"
