// mpmvs_skyseg.hip -- the sky-segmentation network of the C ABI declared in include/mpmvs.h (mpmvs_skyseg): the model reader
// of pm_skyseg_model.hpp, the layer kernels of pm_skyseg.hpp and the handle that runs them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mpmvs.h"
#include "pm_host.hpp"
#include "pm_skyseg.hpp"
#include "pm_skyseg_model.hpp"

using namespace pm;

extern "C" {

// ---------------------------------------------------------------------------
// sky-segmentation network (pm_skyseg.hpp, pm_skyseg_model.hpp).  Errors of these entry points are
// reported through mpmvs_last_error(NULL) (per host thread, like a failed mpmvs_create).
// ---------------------------------------------------------------------------
struct mpmvs_skyseg {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    skyseg::Model m;
    float* d_arena = nullptr;
    float* d_const = nullptr;            // repacked / raw weights and the biases of every live convolution
    std::vector<size_t> w_at, b_at;      // per layer: float offsets into d_const
    std::vector<char> use_mfma;          // per layer
    int launches = 0;
    bool ran = false;
    float net_ms = 0.0f, pre_ms = 0.0f;
};

int mpmvs_skyseg_inspect(const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, long long counts[6]) {
    if (!counts) return call_fail(-2, "skyseg: bad argument");
    skyseg::Model m;
    std::string err;
    const int rc = skyseg::load_model(param_path, bin_path, in_h, in_w, output_blob, m, err);
    if (rc) return call_fail(rc, err);
    counts[0] = (long long)m.layers.size();
    counts[1] = m.n_blobs_declared;
    counts[2] = m.n_conv;
    counts[3] = m.n_live;
    counts[4] = m.weight_bytes;
    counts[5] = m.macs;
    return 0;
}

static void seg_release(mpmvs_skyseg* n) {
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    if (n->d_arena) (void)pool_free(n->d_arena);
    if (n->d_const) (void)pool_free(n->d_const);
    for (hipEvent_t e : n->ev)
        if (e) (void)hipEventDestroy(e);
    if (n->stream) (void)hipStreamDestroy(n->stream);
    delete n;
}

static int seg_load_device(mpmvs_skyseg* n) {
    skyseg::Model& m = n->m;
    CALLCHK(enter_device(n->device));
    CALLCHK(hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : n->ev) CALLCHK(hipEventCreate(&e));
    std::vector<float> host;
    n->w_at.assign(m.layers.size(), 0);
    n->b_at.assign(m.layers.size(), 0);
    n->use_mfma.assign(m.layers.size(), 0);
    for (int li : m.order) {
        const skyseg::Layer& L = m.layers[li];
        if (L.op != skyseg::OP_CONV) continue;
        const float* w = m.weights.data() + L.w_off;
        n->w_at[li] = host.size();
        if (L.k == 3 && L.cout > 1) {  // operand layout of k_seg_conv3_mfma
            n->use_mfma[li] = 1;
            const int pairs = (L.cin + 1) / 2;
            int mt = (L.cout + 31) / 32;
            if (mt > 1) mt = (mt + 1) / 2 * 2;
            host.resize(host.size() + (size_t)pairs * 9 * mt * 64, 0.0f);
            float* d = host.data() + n->w_at[li];
            for (int cp = 0; cp < pairs; ++cp)
                for (int t = 0; t < 9; ++t)
                    for (int j = 0; j < mt; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int c = 2 * cp + (lane >> 5), co = j * 32 + (lane & 31);
                            if (c < L.cin && co < L.cout) d[(((size_t)cp * 9 + t) * mt + j) * 64 + lane] = w[((size_t)co * L.cin + c) * 9 + t];
                        }
        } else {
            host.insert(host.end(), w, w + (size_t)L.cout * L.cin * L.k * L.k);
        }
        host.resize((host.size() + 63) / 64 * 64, 0.0f);
        n->b_at[li] = host.size();
        host.insert(host.end(), m.biases.begin() + L.b_off, m.biases.begin() + L.b_off + L.cout);
        host.resize((host.size() + 63) / 64 * 64, 0.0f);
    }
    if (host.empty()) host.resize(64, 0.0f);
    CALLCHK(pool_malloc(&n->d_const, host.size() * 4));
    CALLCHK(hipMemcpyAsync(n->d_const, host.data(), host.size() * 4, hipMemcpyHostToDevice, n->stream));
    CALLCHK(hipStreamSynchronize(n->stream));  // `host` goes away
    CALLCHK(pool_malloc(&n->d_arena, std::max<size_t>(m.arena_floats, 64) * 4));
    return 0;
}

int mpmvs_skyseg_load(int device, const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_blob, mpmvs_skyseg** net) {
    if (!net) return call_fail(-2, "skyseg: bad argument");
    *net = nullptr;
    mpmvs_skyseg* n = new mpmvs_skyseg;
    n->device = device;
    std::string err;
    int rc = skyseg::load_model(param_path, bin_path, in_h, in_w, output_blob, n->m, err);  // all of the checking: no device touched yet
    if (rc) {
        delete n;
        return call_fail(rc, err);
    }
    rc = seg_load_device(n);
    if (rc) {
        seg_release(n);
        return rc;
    }
    *net = n;
    return 0;
}

void mpmvs_skyseg_destroy(mpmvs_skyseg* n) {
    if (!n) return;
    (void)enter_device(n->device);
    seg_release(n);
}

static float* seg_ptr(const mpmvs_skyseg* n, const skyseg::Seg& s) {
    const skyseg::Buf& b = n->m.bufs[s.buf];
    return n->d_arena + b.off + (size_t)s.coff * b.h * b.w;
}

// enqueues the kernels of the network on the net's stream (the input blob is already in place)
static int seg_enqueue(mpmvs_skyseg* n) {
    const skyseg::Model& m = n->m;
    int launches = 0;
    for (int li : m.order) {
        const skyseg::Layer& L = m.layers[li];
        const skyseg::Blob& in = m.blobs[L.in[0]];
        const skyseg::Blob& ob = m.blobs[L.out[0]];
        float* out = seg_ptr(n, ob.segs[0]);
        const int ohw = ob.h * ob.w;
        switch (L.op) {
            case skyseg::OP_CONV: {
                SegSrcs s{};
                s.n = (int)in.segs.size();
                for (int i = 0; i < s.n; ++i) {
                    s.p[i] = seg_ptr(n, in.segs[i]);
                    s.c[i] = in.segs[i].c;
                }
                const float *w = n->d_const + n->w_at[li], *b = n->d_const + n->b_at[li];
                if (n->use_mfma[li]) {
                    const int mt = (L.cout + 31) / 32, per_block = (kSegConvThreads / 64) * kSegPT * 32;
                    const dim3 grid((ohw + per_block - 1) / per_block, mt > 1 ? (mt + 1) / 2 : 1);
                    const int mt_total = mt > 1 ? (mt + 1) / 2 * 2 : 1;
                    if (mt > 1)
                        hipLaunchKernelGGL(k_seg_conv3_mfma<2>, grid, dim3(kSegConvThreads), 0, n->stream, s, w, b, out, ob.h, ob.w, (L.cin + 1) / 2, mt_total, L.cout, L.dil, L.act);
                    else
                        hipLaunchKernelGGL(k_seg_conv3_mfma<1>, grid, dim3(kSegConvThreads), 0, n->stream, s, w, b, out, ob.h, ob.w, (L.cin + 1) / 2, mt_total, L.cout, L.dil, L.act);
                } else {
                    hipLaunchKernelGGL(k_seg_conv_direct, dim3((ohw + 255) / 256, L.cout), dim3(256), 0, n->stream, s, w, b, out, ob.h, ob.w, L.cin, L.k, L.dil, L.act);
                }
                ++launches;
                break;
            }
            case skyseg::OP_POOL:
            case skyseg::OP_INTERP:
            case skyseg::OP_SIGMOID: {
                int cdone = 0;
                for (const skyseg::Seg& sg : in.segs) {  // a Concat result: one launch per part
                    const float* src = seg_ptr(n, sg);
                    float* dst = out + (size_t)cdone * ohw;
                    const int total = sg.c * ohw;
                    const dim3 grid((total + 255) / 256);
                    if (L.op == skyseg::OP_POOL) hipLaunchKernelGGL(k_seg_pool2, grid, dim3(256), 0, n->stream, src, dst, sg.c, in.h, in.w, ob.h, ob.w);
                    else if (L.op == skyseg::OP_INTERP) hipLaunchKernelGGL(k_seg_interp, grid, dim3(256), 0, n->stream, src, dst, sg.c, in.h, in.w, ob.h, ob.w);
                    else hipLaunchKernelGGL(k_seg_sigmoid, grid, dim3(256), 0, n->stream, src, dst, total);
                    cdone += sg.c;
                    ++launches;
                }
                break;
            }
            case skyseg::OP_ADD: {
                const int total = ob.c * ohw;
                hipLaunchKernelGGL(k_seg_add, dim3((total + 255) / 256), dim3(256), 0, n->stream, seg_ptr(n, in.segs[0]), seg_ptr(n, m.blobs[L.in[1]].segs[0]), out, total);
                ++launches;
                break;
            }
            default:
                return call_fail(-100, "skyseg: layer " + L.name + " has no kernel");  // a missing kernel is an error
        }
    }
    CALLCHK(hipGetLastError());
    n->launches = launches;
    return 0;
}

static int seg_copy_out(mpmvs_skyseg* n, const skyseg::Blob& b, float* out) {
    size_t done = 0;
    for (const skyseg::Seg& s : b.segs) {
        const size_t fl = (size_t)s.c * b.h * b.w;
        CALLCHK(hipMemcpyAsync(out + done, seg_ptr(n, s), fl * 4, hipMemcpyDeviceToHost, n->stream));
        done += fl;
    }
    CALLCHK(hipStreamSynchronize(n->stream));
    return 0;
}

static int seg_run_tail(mpmvs_skyseg* n, float* out) {
    CALLCHK(hipEventRecord(n->ev[1], n->stream));
    int rc = seg_enqueue(n);
    if (rc) {
        (void)hipStreamSynchronize(n->stream);
        return rc;
    }
    CALLCHK(hipEventRecord(n->ev[2], n->stream));
    rc = seg_copy_out(n, n->m.blobs[n->m.output_blob], out);
    if (rc) return rc;
    (void)hipEventElapsedTime(&n->net_ms, n->ev[1], n->ev[2]);
    n->ran = true;
    return 0;
}

int mpmvs_skyseg_run(mpmvs_skyseg* n, const float* in, float* out) {
    if (!n || !in || !out) return call_fail(-2, "skyseg: bad argument");
    CALLCHK(enter_device(n->device));
    const skyseg::Blob& ib = n->m.blobs[n->m.input_blob];
    CALLCHK(hipMemcpyAsync(seg_ptr(n, ib.segs[0]), in, (size_t)ib.c * ib.h * ib.w * 4, hipMemcpyHostToDevice, n->stream));
    n->pre_ms = 0.0f;
    return seg_run_tail(n, out);
}

// the preprocessing of mpmvs_skyseg_run_u8, enqueued: bytes -> pyrDown loop -> resize + normalise into the input blob
static int seg_preprocess(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch, Scratch& a, Scratch& b) {
    const skyseg::Blob& ib = n->m.blobs[n->m.input_blob];
    if (!bgr || h <= 0 || w <= 0 || h > 32768 || w > 32768) return call_fail(-2, "skyseg: bad image size");
    if (ib.c != 3) return call_fail(-2, "skyseg: the network does not take a 3-channel image");
    if (pitch == 0) pitch = (size_t)w * 3;
    if (pitch < (size_t)w * 3) return call_fail(-2, "skyseg: pitch smaller than a row");
    CALLCHK(a.alloc((size_t)w * h * 3));
    CALLCHK(hipMemcpy2DAsync(a.p, (size_t)w * 3, bgr, pitch, (size_t)w * 3, (size_t)h, hipMemcpyHostToDevice, n->stream));
    CALLCHK(hipEventRecord(n->ev[0], n->stream));
    unsigned char *cur = a.as<unsigned char>(), *other = nullptr;
    if (h > 768 && w > 768) {
        CALLCHK(b.alloc((size_t)(w / 2) * (h / 2) * 3));
        other = b.as<unsigned char>();
    }
    while (h > 768 && w > 768) {  // src/PatchMatch.cpp:16-18
        const int ow = w / 2, oh = h / 2;
        const int total = ow * oh * 3;
        hipLaunchKernelGGL(k_seg_pyrdown, dim3((total + 255) / 256), dim3(256), 0, n->stream, cur, other, w, h, ow, oh, 3);
        std::swap(cur, other);  // the next level fits the first buffer: it is a quarter of it
        w = ow, h = oh;
    }
    SegNorm nm;
    nm.mean[0] = 0.485f * 255.f, nm.mean[1] = 0.456f * 255.f, nm.mean[2] = 0.406f * 255.f;  // SkyRegionDetect.cpp:628-629
    nm.norm[0] = 1 / 0.229f / 255.f, nm.norm[1] = 1 / 0.224f / 255.f, nm.norm[2] = 1 / 0.225f / 255.f;
    const int total = 3 * ib.h * ib.w;
    CALLCHK(launch(k_seg_resize_norm, dim3((total + 255) / 256), dim3(256), n->stream, cur, w, h, seg_ptr(n, ib.segs[0]), ib.w, ib.h, (float)w / ib.w, (float)h / ib.h, nm));
    return 0;
}

int mpmvs_skyseg_run_u8(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out) {
    if (!n || !out) return call_fail(-2, "skyseg: bad argument");
    CALLCHK(enter_device(n->device));
    Scratch a(n->stream), b(n->stream);
    int rc = seg_preprocess(n, bgr, h, w, pitch_bytes, a, b);
    if (!rc) rc = seg_run_tail(n, out);   // (ends synchronised)
    if (!rc) (void)hipEventElapsedTime(&n->pre_ms, n->ev[0], n->ev[1]);
    return rc;
}

int mpmvs_skyseg_preprocess_u8(mpmvs_skyseg* n, const unsigned char* bgr, int h, int w, size_t pitch_bytes, float* out_chw) {
    if (!n || !out_chw) return call_fail(-2, "skyseg: bad argument");
    CALLCHK(enter_device(n->device));
    Scratch a(n->stream), b(n->stream);
    int rc = seg_preprocess(n, bgr, h, w, pitch_bytes, a, b);
    if (!rc) rc = seg_copy_out(n, n->m.blobs[n->m.input_blob], out_chw);
    n->ran = false;  // the blobs of the last run are no longer all there
    return rc;
}

int mpmvs_skyseg_set_keep(mpmvs_skyseg* n, int keep) {
    if (!n) return call_fail(-2, "skyseg: bad argument");
    if ((keep != 0) == n->m.keep) return 0;
    CALLCHK(enter_device(n->device));
    CALLCHK(hipStreamSynchronize(n->stream));
    const size_t before = n->m.arena_floats;
    skyseg::plan(n->m, keep != 0);
    n->ran = false;
    if (std::max<size_t>(n->m.arena_floats, 64) != std::max<size_t>(before, 64)) {
        (void)pool_free(n->d_arena);
        n->d_arena = nullptr;
        if (pool_malloc(&n->d_arena, std::max<size_t>(n->m.arena_floats, 64) * 4) != hipSuccess) {
            (void)hipGetLastError();
            skyseg::plan(n->m, !keep);  // back to the plan that fitted
            CALLCHK(pool_malloc(&n->d_arena, std::max<size_t>(n->m.arena_floats, 64) * 4));
            return call_fail(-100, "skyseg: no memory for the arena of the keep mode");
        }
    }
    return 0;
}

int mpmvs_skyseg_blob(mpmvs_skyseg* n, const char* name, float* out, int dims[3]) {
    if (!n || !name || !dims) return call_fail(-2, "skyseg: bad argument");
    const skyseg::Model& m = n->m;
    int id = -1;
    for (int i = 0; i < (int)m.blobs.size(); ++i)
        if (m.blobs[i].name == name) id = i;
    bool live = id >= 0;
    if (live)
        for (const skyseg::Seg& s : m.blobs[id].segs) live = live && m.bufs[s.buf].first >= 0;
    if (!live) return call_fail(MPMVS_SKYSEG_E_NOBLOB, std::string("skyseg: no live blob named ") + name);
    dims[0] = m.blobs[id].c, dims[1] = m.blobs[id].h, dims[2] = m.blobs[id].w;
    if (!out) return 0;
    if (!m.keep || !n->ran) return call_fail(MPMVS_SKYSEG_E_NOKEEP, "skyseg: blobs can be fetched after a run in keep mode only");
    CALLCHK(enter_device(n->device));
    return seg_copy_out(n, m.blobs[id], out);
}

int mpmvs_skyseg_dims(const mpmvs_skyseg* n, int dims[7]) {
    if (!n || !dims) return call_fail(-2, "skyseg: bad argument");
    const skyseg::Blob &i = n->m.blobs[n->m.input_blob], &o = n->m.blobs[n->m.output_blob];
    dims[0] = i.c, dims[1] = i.h, dims[2] = i.w, dims[3] = o.c, dims[4] = o.h, dims[5] = o.w;
    int launches = 0;
    for (int li : n->m.order) {
        const skyseg::Layer& L = n->m.layers[li];
        launches += (L.op == skyseg::OP_POOL || L.op == skyseg::OP_INTERP || L.op == skyseg::OP_SIGMOID) ? (int)n->m.blobs[L.in[0]].segs.size() : 1;
    }
    dims[6] = launches;
    return 0;
}

float mpmvs_skyseg_ms(const mpmvs_skyseg* n, float* pre_ms) {
    if (!n) return 0.0f;
    if (pre_ms) *pre_ms = n->pre_ms;
    return n->net_ms;
}

}  // extern "C"
