// oracle/ref_shim/host_standin.h
//
// TEST INFRASTRUCTURE ONLY.  Host stand-ins for what the reference's HOST code (src/PatchMatch.cpp: the PLY writer, the
// projection helpers, RunFusion and GetTriangulateVertices) names from CUDA's vector types, OpenCV and its own headers, so that
// those functions compile here and run on arrays the driver holds (oracle/ref_host_driver.cpp, oracle/Makefile target `ref`).
// Nothing here is taken from the reference, from CUDA's or from OpenCV's headers: the types are the obvious containers.
//
// What a stand-in decides, and why:
//   headers      exactly the standard headers the reference's main.h includes, <math.h> among them and no other math header,
//                and no `using namespace std`: which of exp / fabs / pow / sqrt run in double is decided by overload resolution
//                in this environment (the static_asserts in the driver state the outcome).  <float.h> and
//                <stdio.h> stand for the C headers that reach the reference through CUDA and OpenCV (FLT_MAX, FILE): they
//                declare no function that takes part in that resolution.
//   cv::Mat      a reference-counted 2-D array (copies share, clone() copies), as OpenCV's; at<T>(row, col).  Containers only:
//                no arithmetic on matrices exists here.
//   cv::Vec3f    `a + b` is the component-wise fp32 sum.  `a /= s` is the ONE piece of OpenCV arithmetic RunFusion relies on that
//                cannot be pinned without OpenCV: the default divides each component by s, -DMPMVS_REF_VEC_RCP multiplies each
//                by the fp32 reciprocal 1.f / s (the two builds of the Makefile).  Only the averaged normal goes through it.
//   cv::resize   copies when the sizes are equal; otherwise raises g_refh_resampled, which fails the driver's call: the tests
//                never resample.
//   imread, readDepthDmb, readNormalDmb, ReadCamera
//                serve the arrays the driver registered, keyed by the 8-digit image number in the path.
#ifndef MPMVS_REF_SHIM_HOST_STANDIN_H_
#define MPMVS_REF_SHIM_HOST_STANDIN_H_

// the reference's main.h, in its order
#include <vector>
#include <string>
#include <iostream>
#include <fstream>
#include <sstream>
#include <algorithm>
#include <map>
#include <memory>
#include <iomanip>
#include <math.h>

#include <float.h>
#include <stdio.h>

#include "../../include/mpmvs.h"

typedef unsigned char uchar;

// CUDA's vector types, as PODs
struct int2 { int x, y; };
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }

// byte-compatible mirrors of the reference's PODs (include/mpmvs.h)
typedef mpmvs_camera Camera;
typedef mpmvs_params PatchMatchParams;

extern int g_refh_resampled;  // set by cv::resize when asked to change a size

namespace cv {

enum { CV_8UC1_ = 0, CV_8UC3_ = 16, CV_32FC1_ = 5, CV_32FC3_ = 21 };
enum { IMREAD_GRAYSCALE = 0, IMREAD_COLOR = 1 };
enum { INTER_LINEAR = 1 };

template <class T, int N>
struct Vec {
    T val[N];
    Vec() {
        for (int i = 0; i < N; ++i) val[i] = T(0);
    }
    T& operator[](int i) { return val[i]; }
    const T& operator[](int i) const { return val[i]; }
};
typedef Vec<float, 3> Vec3f;
typedef Vec<uchar, 3> Vec3b;

inline Vec3f operator+(const Vec3f& a, const Vec3f& b) {
    Vec3f r;
    for (int i = 0; i < 3; ++i) r[i] = a[i] + b[i];
    return r;
}
inline Vec3f& operator/=(Vec3f& a, float s) {
#ifdef MPMVS_REF_VEC_RCP
    const float inv = 1.f / s;
    for (int i = 0; i < 3; ++i) a[i] = a[i] * inv;
#else
    for (int i = 0; i < 3; ++i) a[i] = a[i] / s;
#endif
    return a;
}

struct Point {
    int x, y;
    Point() : x(0), y(0) {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

inline size_t refh_elem_size(int type) { return type == CV_8UC1_ ? 1 : type == CV_8UC3_ ? 3 : type == CV_32FC1_ ? 4 : 12; }

struct Mat {
    int rows, cols;
    size_t elem;  // bytes per element
    std::shared_ptr<std::vector<uchar>> store;
    Mat() : rows(0), cols(0), elem(0) {}
    Mat(int r, int c, size_t e) : rows(r), cols(c), elem(e), store(std::make_shared<std::vector<uchar>>((size_t)r * c * e, (uchar)0)) {}
    Mat(int r, int c, int type) : Mat(r, c, refh_elem_size(type)) {}
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    template <class T>
    T& at(int r, int c) {
        return *reinterpret_cast<T*>(store->data() + ((size_t)r * cols + c) * sizeof(T));
    }
    template <class T>
    const T& at(int r, int c) const {
        return *reinterpret_cast<const T*>(store->data() + ((size_t)r * cols + c) * sizeof(T));
    }
    Mat clone() const {
        Mat m(rows, cols, elem);
        if (store) *m.store = *store;
        return m;
    }
};

template <class T>
struct Mat_ : public Mat {
    Mat_() : Mat() {}
    Mat_(int r, int c) : Mat(r, c, sizeof(T)) {}
    Mat_(const Mat& m) : Mat(m) {}
    T& operator()(int r, int c) { return this->template at<T>(r, c); }
    const T& operator()(int r, int c) const { return this->template at<T>(r, c); }
    Mat_ clone() const { return Mat_(Mat::clone()); }
};

inline void resize(const Mat& src, Mat& dst, Size size, double, double, int) {
    if (size.width != src.cols || size.height != src.rows) g_refh_resampled = 1;
    dst = src.clone();
}

Mat imread(const std::string& path, int flags);

}  // namespace cv

#define CV_8UC1 cv::CV_8UC1_

// the reference's own structures, reduced to the members its fusion and its vertex picker touch
struct PointList {
    float3 coord, normal, color;
};

struct Scene {
    int refID = 0;
    bool estimate = false;
    std::vector<int> srcID;  // srcID[0] is the image itself
};

struct ConfigParams {
    std::string input_folder, output_folder;
    bool sky_seg = false, use_dynamic_consistency = false;
};

struct Triangle {
    cv::Point pt1, pt2, pt3;
    Triangle(const cv::Point a, const cv::Point b, const cv::Point c) : pt1(a), pt2(b), pt3(c) {}
};

// only what the five cut member definitions touch; public, so that the driver can fill it
class PatchMatchCUDA {
public:
    std::vector<Camera> cameras;
    float* hostCosts = nullptr;
    float* hostGeomCosts = nullptr;
    PatchMatchParams params;

    int GetReferenceImageWidth();
    int GetReferenceImageHeight();
    float GetCost(int index);
    float GetGeomCost(int index);
    void GetTriangulateVertices(std::vector<cv::Point>& Vertices);
};

Camera ReadCamera(const std::string& cam_path);
bool readDepthDmb(const std::string file_path, cv::Mat_<float>& depth);
bool readNormalDmb(const std::string file_path, cv::Mat_<cv::Vec3f>& normal);

#endif
