// colmap_io.cpp -- reader of a COLMAP sparse model (cameras / images / points3D, .txt or .bin), the input of the
// converter to the MVSNet-style folder (mp-mvs_amd/colmap.py, tools/colmap2mvs.py).  Same fields as COLMAP's
// scripts/python/read_write_model.py reads; binary layout little-endian with uint64 counts and int64 point3D ids
// (-1: none).  The tracks of points3D are not used (view selection walks the images' point3D_ids, as the reference
// converter does), so only id and xyz of a point are kept.
//
// C ABI: mpmvs_host_colmap_read parses and returns a handle plus the array sizes, mpmvs_host_colmap_fill copies the
// arrays out and mpmvs_host_colmap_free releases the handle (the size-then-fill pattern of mpmvs_host_sample_list,
// without parsing twice).  Errors come back as a code and a message, never as an exit.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

struct ModelDef {
    const char* name;
    int num_params;
};
// COLMAP's camera model ids 0..10 (src/colmap/sensor/models.h)
const ModelDef kModels[] = {{"SIMPLE_PINHOLE", 3}, {"PINHOLE", 4},       {"SIMPLE_RADIAL", 4},         {"RADIAL", 5},
                            {"OPENCV", 8},         {"OPENCV_FISHEYE", 8}, {"FULL_OPENCV", 12},          {"FOV", 5},
                            {"SIMPLE_RADIAL_FISHEYE", 4}, {"RADIAL_FISHEYE", 5}, {"THIN_PRISM_FISHEYE", 12}};
constexpr int kNumModels = 11, kMaxParams = 12;

struct Model {
    std::vector<int32_t> cam_id, cam_model;
    std::vector<int64_t> cam_width, cam_height;
    std::vector<double> cam_params;  // kMaxParams per camera, zero padded
    std::vector<int32_t> img_id, img_cam;
    std::vector<double> img_q, img_t;
    std::vector<std::string> img_name;
    std::vector<std::vector<int64_t>> img_pts;  // point3D ids as read
    std::vector<int64_t> pt_id;
    std::vector<double> pt_xyz;
    // filled by finish(): images by ascending id, point ids -> dense indices
    std::vector<int64_t> obs_off;
    std::vector<int32_t> obs_pt;
    std::vector<int> order;
};

struct Error {
    std::string msg;
};

[[noreturn]] void fail(const std::string& m) { throw Error{m}; }

// ---- binary ----
struct Bin {
    std::string path;
    std::vector<unsigned char> buf;
    size_t pos = 0;
    explicit Bin(const std::string& p) : path(p) {
        std::ifstream in(p, std::ios::binary);
        if (!in) fail("cannot open " + p);
        buf.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    }
    void need(size_t n) {
        if (buf.size() - pos < n) fail(path + ": truncated at byte " + std::to_string(pos));
    }
    template <typename T>
    T get() {
        need(sizeof(T));
        T v;
        std::memcpy(&v, buf.data() + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
    std::string cstr() {
        const size_t b = pos;
        while (true) {
            need(1);
            if (buf[pos++] == 0) break;
        }
        return std::string((const char*)buf.data() + b, pos - b - 1);
    }
    uint64_t count(size_t min_record) {
        const uint64_t n = get<uint64_t>();
        if (min_record && n > (buf.size() - pos) / min_record) fail(path + ": truncated (count " + std::to_string(n) + " exceeds the file)");
        return n;
    }
};

void read_cameras_bin(const std::string& p, Model& m) {
    Bin b(p);
    const uint64_t n = b.count(24);
    for (uint64_t k = 0; k < n; ++k) {
        const int32_t id = b.get<int32_t>(), model = b.get<int32_t>();
        const uint64_t w = b.get<uint64_t>(), h = b.get<uint64_t>();
        if (model < 0 || model >= kNumModels) fail(p + ": camera " + std::to_string(id) + " has unknown model id " + std::to_string(model));
        m.cam_id.push_back(id);
        m.cam_model.push_back(model);
        m.cam_width.push_back((int64_t)w);
        m.cam_height.push_back((int64_t)h);
        for (int j = 0; j < kMaxParams; ++j) m.cam_params.push_back(j < kModels[model].num_params ? b.get<double>() : 0.0);
    }
}

void read_images_bin(const std::string& p, Model& m) {
    Bin b(p);
    const uint64_t n = b.count(64 + 1 + 8);
    for (uint64_t k = 0; k < n; ++k) {
        m.img_id.push_back(b.get<int32_t>());
        for (int j = 0; j < 4; ++j) m.img_q.push_back(b.get<double>());
        for (int j = 0; j < 3; ++j) m.img_t.push_back(b.get<double>());
        m.img_cam.push_back(b.get<int32_t>());
        m.img_name.push_back(b.cstr());
        const uint64_t np = b.count(24);
        std::vector<int64_t> ids(np);
        for (uint64_t j = 0; j < np; ++j) {
            (void)b.get<double>();
            (void)b.get<double>();
            ids[j] = b.get<int64_t>();
        }
        m.img_pts.push_back(std::move(ids));
    }
}

void read_points_bin(const std::string& p, Model& m) {
    Bin b(p);
    const uint64_t n = b.count(43 + 8);
    m.pt_id.reserve(n);
    m.pt_xyz.reserve(3 * n);
    for (uint64_t k = 0; k < n; ++k) {
        m.pt_id.push_back((int64_t)b.get<uint64_t>());
        for (int j = 0; j < 3; ++j) m.pt_xyz.push_back(b.get<double>());
        b.need(3 + 8);
        b.pos += 3 + 8;  // rgb, error
        const uint64_t len = b.count(8);
        b.pos += 8 * len;  // track (image id, point2D index): not used
    }
}

// ---- text ----
struct Text {
    std::string path;
    std::ifstream in;
    int line_no = 0;
    explicit Text(const std::string& p) : path(p), in(p) {
        if (!in) fail("cannot open " + p);
    }
    bool raw_line(std::string& s) {
        if (!std::getline(in, s)) return false;
        ++line_no;
        if (!s.empty() && s.back() == '\r') s.pop_back();
        return true;
    }
    // next line that is neither empty nor a comment
    bool data_line(std::string& s) {
        while (raw_line(s)) {
            const size_t f = s.find_first_not_of(" \t");
            if (f != std::string::npos && s[f] != '#') return true;
        }
        return false;
    }
    [[noreturn]] void bad(const std::string& why) { fail(path + ":" + std::to_string(line_no) + ": " + why); }
};

std::vector<std::string> split(const std::string& s) {
    std::vector<std::string> t;
    std::istringstream is(s);
    std::string w;
    while (is >> w) t.push_back(w);
    return t;
}

double to_d(Text& t, const std::string& s) {
    char* e = nullptr;
    errno = 0;
    const double v = std::strtod(s.c_str(), &e);
    if (e == s.c_str() || *e) t.bad("'" + s + "' is not a number");
    return v;
}

int64_t to_i(Text& t, const std::string& s) {
    char* e = nullptr;
    errno = 0;
    const long long v = std::strtoll(s.c_str(), &e, 10);
    if (e == s.c_str() || *e || errno) t.bad("'" + s + "' is not an integer");
    return v;
}

void read_cameras_txt(const std::string& p, Model& m) {
    Text t(p);
    std::string s;
    while (t.data_line(s)) {
        const auto e = split(s);
        if (e.size() < 4) t.bad("truncated camera line");
        int model = -1;
        for (int k = 0; k < kNumModels; ++k)
            if (e[1] == kModels[k].name) model = k;
        if (model < 0) t.bad("unknown camera model " + e[1]);
        const int np = kModels[model].num_params;
        if ((int)e.size() != 4 + np) t.bad(e[1] + " takes " + std::to_string(np) + " parameters");
        m.cam_id.push_back((int32_t)to_i(t, e[0]));
        m.cam_model.push_back(model);
        m.cam_width.push_back(to_i(t, e[2]));
        m.cam_height.push_back(to_i(t, e[3]));
        for (int j = 0; j < kMaxParams; ++j) m.cam_params.push_back(j < np ? to_d(t, e[4 + j]) : 0.0);
    }
}

void read_images_txt(const std::string& p, Model& m) {
    Text t(p);
    std::string s;
    while (t.data_line(s)) {
        const auto e = split(s);
        if (e.size() < 10) t.bad("truncated image line");
        m.img_id.push_back((int32_t)to_i(t, e[0]));
        for (int j = 0; j < 4; ++j) m.img_q.push_back(to_d(t, e[1 + j]));
        for (int j = 0; j < 3; ++j) m.img_t.push_back(to_d(t, e[5 + j]));
        m.img_cam.push_back((int32_t)to_i(t, e[8]));
        m.img_name.push_back(e[9]);
        std::string pl;
        if (!t.raw_line(pl)) t.bad("image " + e[0] + " has no POINTS2D line (truncated file)");
        const auto q = split(pl);
        if (q.size() % 3) t.bad("POINTS2D line of image " + e[0] + " is not a list of (X, Y, POINT3D_ID)");
        std::vector<int64_t> ids(q.size() / 3);
        for (size_t j = 0; j < ids.size(); ++j) ids[j] = to_i(t, q[3 * j + 2]);
        m.img_pts.push_back(std::move(ids));
    }
}

void read_points_txt(const std::string& p, Model& m) {
    Text t(p);
    std::string s;
    while (t.data_line(s)) {
        const char* c = s.c_str();
        char* e = nullptr;
        errno = 0;
        const long long id = std::strtoll(c, &e, 10);
        if (e == c || errno) t.bad("bad POINT3D_ID");
        m.pt_id.push_back(id);
        for (int j = 0; j < 3; ++j) {
            c = e;
            const double v = std::strtod(c, &e);
            if (e == c) t.bad("truncated point line");
            m.pt_xyz.push_back(v);
        }
    }
}

void finish(Model& m) {
    std::unordered_map<int32_t, int> cams;
    for (size_t k = 0; k < m.cam_id.size(); ++k)
        if (!cams.emplace(m.cam_id[k], (int)k).second) fail("camera id " + std::to_string(m.cam_id[k]) + " appears twice");
    std::unordered_map<int64_t, int32_t> pts;
    pts.reserve(m.pt_id.size());
    if (m.pt_id.size() > (size_t)INT32_MAX) fail("more than 2^31 - 1 points");
    for (size_t k = 0; k < m.pt_id.size(); ++k)
        if (!pts.emplace(m.pt_id[k], (int32_t)k).second) fail("point3D id " + std::to_string(m.pt_id[k]) + " appears twice");
    const size_t n = m.img_id.size();
    if (n == 0) fail("the model has no images");
    m.order.resize(n);
    std::iota(m.order.begin(), m.order.end(), 0);
    std::sort(m.order.begin(), m.order.end(), [&](int a, int b) { return m.img_id[a] < m.img_id[b]; });
    for (size_t k = 1; k < n; ++k)
        if (m.img_id[m.order[k]] == m.img_id[m.order[k - 1]]) fail("image id " + std::to_string(m.img_id[m.order[k]]) + " appears twice");
    m.obs_off.assign(1, 0);
    for (int k : m.order) {
        if (!cams.count(m.img_cam[k]))
            fail("image " + std::to_string(m.img_id[k]) + " names camera " + std::to_string(m.img_cam[k]) + ", which is not in the model");
        bool any = false;
        for (int64_t id : m.img_pts[k]) {
            if (id == -1) {
                m.obs_pt.push_back(-1);
                continue;
            }
            auto it = pts.find(id);
            if (it == pts.end())
                fail("image " + std::to_string(m.img_id[k]) + " observes point3D " + std::to_string(id) + ", which is not in points3D");
            m.obs_pt.push_back(it->second);
            any = true;
        }
        if (!any) fail("image " + std::to_string(m.img_id[k]) + " (" + m.img_name[k] + ") has no observation of a 3D point: its depth range is undefined");
        m.obs_off.push_back((int64_t)m.obs_pt.size());
    }
}

void set_err(char* err, int cap, const std::string& m) {
    if (!err || cap <= 0) return;
    std::snprintf(err, (size_t)cap, "%s", m.c_str());
}

}  // namespace

extern "C" {

// Parses <dir>/{cameras,images,points3D}<ext> (ext ".txt" or ".bin").  sizes[0..4] = cameras, images, observations (total
// length of the images' point3D_ids), points, bytes of the image names (each NUL-terminated).  NULL on error, with the
// message in err.
void* mpmvs_host_colmap_read(const char* dir, const char* ext, int64_t* sizes, char* err, int err_cap) {
    try {
        const std::string d(dir), x(ext);
        if (x != ".txt" && x != ".bin") fail("model extension must be .txt or .bin, not " + x);
        auto* m = new Model();
        try {
            if (x == ".bin") {
                read_cameras_bin(d + "/cameras.bin", *m);
                read_images_bin(d + "/images.bin", *m);
                read_points_bin(d + "/points3D.bin", *m);
            } else {
                read_cameras_txt(d + "/cameras.txt", *m);
                read_images_txt(d + "/images.txt", *m);
                read_points_txt(d + "/points3D.txt", *m);
            }
            finish(*m);
        } catch (...) {
            delete m;
            throw;
        }
        size_t name_bytes = 0;
        for (const auto& s : m->img_name) name_bytes += s.size() + 1;
        sizes[0] = (int64_t)m->cam_id.size();
        sizes[1] = (int64_t)m->img_id.size();
        sizes[2] = (int64_t)m->obs_pt.size();
        sizes[3] = (int64_t)m->pt_id.size();
        sizes[4] = (int64_t)name_bytes;
        return m;
    } catch (const Error& e) {
        set_err(err, err_cap, e.msg);
    } catch (const std::exception& e) {
        set_err(err, err_cap, std::string("COLMAP model: ") + e.what());
    }
    return nullptr;
}

// Copies the arrays out, images in ascending id order.  cam_params: 12 per camera (zero padded); qvec / tvec: 4 / 3 per
// image; obs_off: images + 1 offsets into obs_pt; obs_pt: dense point index (position in points3D) or -1; xyz: 3 per point.
int mpmvs_host_colmap_fill(void* handle, int32_t* cam_id, int32_t* cam_model, int64_t* cam_width, int64_t* cam_height, double* cam_params,
                           int32_t* img_id, double* qvec, double* tvec, int32_t* img_cam, char* names, int64_t* obs_off, int32_t* obs_pt,
                           int64_t* pt_id, double* xyz) {
    if (!handle) return -1;
    const Model& m = *(const Model*)handle;
    auto cp = [](auto* dst, const auto& v) {
        if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    cp(cam_id, m.cam_id);
    cp(cam_model, m.cam_model);
    cp(cam_width, m.cam_width);
    cp(cam_height, m.cam_height);
    cp(cam_params, m.cam_params);
    size_t o = 0;
    for (size_t r = 0; r < m.order.size(); ++r) {
        const int k = m.order[r];
        img_id[r] = m.img_id[k];
        img_cam[r] = m.img_cam[k];
        for (int j = 0; j < 4; ++j) qvec[4 * r + j] = m.img_q[4 * k + j];
        for (int j = 0; j < 3; ++j) tvec[3 * r + j] = m.img_t[3 * k + j];
        std::memcpy(names + o, m.img_name[k].c_str(), m.img_name[k].size() + 1);
        o += m.img_name[k].size() + 1;
    }
    cp(obs_off, m.obs_off);
    cp(obs_pt, m.obs_pt);
    cp(pt_id, m.pt_id);
    cp(xyz, m.pt_xyz);
    return 0;
}

void mpmvs_host_colmap_free(void* handle) { delete (Model*)handle; }

}  // extern "C"
