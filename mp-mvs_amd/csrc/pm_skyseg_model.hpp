// pm_skyseg_model.hpp -- host-side loader of the sky-segmentation network: an ncnn .param / .bin pair
// read into a flat layer list, shapes inferred from the input size, dead layers dropped, buffers planned by liveness.
// The reference hands the files to ncnn (SkySegment/src/SkyRegionDetect.cpp:541-561); here they are data for the engine in
// pm_skyseg.hpp.  Pure C++: nothing in this file touches a device (mpmvs_skyseg_inspect runs on a machine without one).
//
// Supported, and nothing else: Input; Convolution 3x3 (pad = dilation) or 1x1, stride 1, group 1, bias optional, activation none /
// ReLU / sigmoid, weight tag 0x01306B47 (fp16, block padded to 4 bytes) or 0 (fp32); Pooling max 2x2 stride 2 in ncnn's default
// "full" pad mode (= ceil mode); Interp bilinear to a fixed size without align_corner; BinaryOp add of two blobs; Concat along
// channels; Split; Sigmoid.  Every other layer or parameter is refused with its own code and a text that names the layer.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mpmvs.h"

namespace skyseg {

enum Op { OP_INPUT = 0, OP_CONV, OP_POOL, OP_INTERP, OP_ADD, OP_CONCAT, OP_SPLIT, OP_SIGMOID };

// a blob is a list of channel runs of real buffers: Split aliases its input, Concat strings its inputs together (it never copies)
struct Seg {
    int buf;   // index into Model::bufs
    int coff;  // first channel inside that buffer
    int c;     // channels
};
struct Blob {
    std::string name;
    int c = 0, h = 0, w = 0;
    bool written = false;
    std::vector<Seg> segs;
};
struct Buf {
    int c = 0, h = 0, w = 0;
    int first = 0, last = 0;  // live-layer positions of the producer and of the last reader
    size_t off = 0;           // float offset inside the arena
    size_t floats() const { return (size_t)c * h * w; }
};
struct Layer {
    int op = 0;
    std::string name;
    std::vector<int> in, out;  // blob ids
    int cout = 0, k = 0, dil = 1, pad = 0, act = 0, cin = 0, has_bias = 0;
    size_t w_off = 0, b_off = 0;  // float offsets into Model::weights (ncnn order [cout][cin][ky][kx]) / Model::biases
    bool live = false;
};
struct Model {
    std::vector<Layer> layers;
    std::vector<Blob> blobs;
    std::vector<Buf> bufs;
    std::vector<float> weights, biases;
    std::vector<int> order;  // live layers that launch something, in file order
    int n_blobs_declared = 0, n_conv = 0, n_live = 0;
    int input_blob = -1, output_blob = -1;
    long long weight_bytes = 0, macs = 0;
    size_t arena_floats = 0;
    bool keep = false;
};

static inline float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t u;
    if (e == 0) {
        if (m == 0) {
            u = s;
        } else {  // subnormal half: normalise
            int sh = 0;
            while (!(m & 1024u)) {
                m <<= 1;
                ++sh;
            }
            u = s | ((uint32_t)(113 - sh) << 23) | ((m & 1023u) << 13);
        }
    } else if (e == 31) {
        u = s | 0x7f800000u | (m << 13);
    } else {
        u = s | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static inline bool read_file(const char* path, std::string& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    std::fclose(f);
    return true;
}

static inline std::vector<std::string> split_ws(const std::string& line) {
    std::vector<std::string> t;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
        if (j > i) t.push_back(line.substr(i, j - i));
        i = j;
    }
    return t;
}

// Plans the arena: every real buffer gets a float offset; with keep == false a buffer's space is handed on once its last reader
// has run (first fit over a free list, in launch order, so the plan is a function of the graph alone).
static inline void plan(Model& m, bool keep) {
    m.keep = keep;
    const size_t kAlign = 64;  // floats: 256-byte aligned buffers
    auto up = [&](size_t v) { return (v + kAlign - 1) / kAlign * kAlign; };
    size_t top = 0;
    if (keep) {
        for (Buf& b : m.bufs) {
            if (b.first < 0) continue;
            b.off = top;
            top += up(b.floats());
        }
        m.arena_floats = top;
        return;
    }
    std::map<size_t, size_t> free_list;  // offset -> size, coalesced
    auto release = [&](size_t off, size_t size) {
        auto it = free_list.emplace(off, size).first;
        auto nx = std::next(it);
        if (nx != free_list.end() && it->first + it->second == nx->first) {
            it->second += nx->second;
            free_list.erase(nx);
        }
        if (it != free_list.begin()) {
            auto pv = std::prev(it);
            if (pv->first + pv->second == it->first) {
                pv->second += it->second;
                free_list.erase(it);
            }
        }
    };
    const int steps = (int)m.order.size() + 1;  // position 0 is the input upload
    std::vector<std::vector<int>> born(steps + 1), dies(steps + 1);
    for (int i = 0; i < (int)m.bufs.size(); ++i) {
        if (m.bufs[i].first < 0) continue;
        born[m.bufs[i].first].push_back(i);
        dies[m.bufs[i].last].push_back(i);
    }
    for (int s = 0; s < steps; ++s) {
        for (int i : born[s]) {
            const size_t need = up(m.bufs[i].floats());
            bool placed = false;
            for (auto it = free_list.begin(); it != free_list.end(); ++it)
                if (it->second >= need) {
                    const size_t off = it->first, rest = it->second - need;
                    free_list.erase(it);
                    if (rest) free_list.emplace(off + need, rest);
                    m.bufs[i].off = off;
                    placed = true;
                    break;
                }
            if (!placed) {
                m.bufs[i].off = top;
                top += need;
            }
        }
        // a buffer read for the last time at step s is free from step s + 1 on (an output never overlaps its own inputs)
        for (int i : dies[s]) release(m.bufs[i].off, up(m.bufs[i].floats()));
    }
    m.arena_floats = top;
}

static inline int refuse(std::string& err, int code, const std::string& text) {
    err = text;
    return code;
}

// Reads and checks the pair; on success `m` is complete (plan() done for keep == false).  bin_path may be NULL only for
// shape-only uses; here it is always given.
static inline int load_model(const char* param_path, const char* bin_path, int in_h, int in_w, const char* output_name, Model& m, std::string& err) {
    if (!param_path || !bin_path || in_h <= 0 || in_w <= 0 || in_h > 8192 || in_w > 8192) return refuse(err, -2, "skyseg: bad argument");
    std::string text, bin;
    if (!read_file(param_path, text)) return refuse(err, MPMVS_SKYSEG_E_FILE, std::string("skyseg: cannot read ") + param_path);
    if (!read_file(bin_path, bin)) return refuse(err, MPMVS_SKYSEG_E_FILE, std::string("skyseg: cannot read ") + bin_path);
    std::vector<std::vector<std::string>> lines;
    for (size_t i = 0; i < text.size();) {
        size_t j = text.find('\n', i);
        if (j == std::string::npos) j = text.size();
        std::vector<std::string> t = split_ws(text.substr(i, j - i));
        if (!t.empty()) lines.push_back(t);
        i = j + 1;
    }
    if (lines.size() < 2 || lines[0].size() != 1 || lines[0][0] != "7767517") return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: wrong magic (not an ncnn text .param)");
    if (lines[1].size() != 2) return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: malformed layer / blob count line");
    const long n_layers = std::strtol(lines[1][0].c_str(), nullptr, 10);
    m.n_blobs_declared = (int)std::strtol(lines[1][1].c_str(), nullptr, 10);
    if (n_layers <= 0 || n_layers != (long)lines.size() - 2) return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: layer count does not match the file");

    std::map<std::string, int> blob_id;
    size_t bin_off = 0;
    auto blob_of = [&](const std::string& name) {
        auto it = blob_id.find(name);
        if (it != blob_id.end()) return it->second;
        Blob b;
        b.name = name;
        m.blobs.push_back(b);
        return blob_id[name] = (int)m.blobs.size() - 1;
    };
    auto new_buf = [&](int c, int h, int w) {
        Buf b;
        b.c = c, b.h = h, b.w = w, b.first = -1, b.last = -1;
        m.bufs.push_back(b);
        return (int)m.bufs.size() - 1;
    };
    for (long li = 0; li < n_layers; ++li) {
        const std::vector<std::string>& t = lines[li + 2];
        if (t.size() < 4) return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: malformed layer line " + std::to_string(li));
        Layer L;
        L.name = t[1];
        const std::string& type = t[0];
        const long ni = std::strtol(t[2].c_str(), nullptr, 10), no = std::strtol(t[3].c_str(), nullptr, 10);
        if (ni < 0 || no < 0 || (long)t.size() < 4 + ni + no) return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: malformed layer line of " + L.name);
        std::map<int, std::string> prm;
        for (size_t i = 4 + ni + no; i < t.size(); ++i) {
            const size_t eq = t[i].find('=');
            if (eq == std::string::npos) return refuse(err, MPMVS_SKYSEG_E_MAGIC, "skyseg: malformed parameter of " + L.name);
            prm[(int)std::strtol(t[i].substr(0, eq).c_str(), nullptr, 10)] = t[i].substr(eq + 1);
        }
        auto geti = [&](int key, long def) {
            auto it = prm.find(key);
            return it == prm.end() ? def : std::strtol(it->second.c_str(), nullptr, 10);
        };
        auto getf = [&](int key, double def) {
            auto it = prm.find(key);
            return it == prm.end() ? def : std::strtod(it->second.c_str(), nullptr);
        };
        for (long i = 0; i < ni; ++i) {
            auto it = blob_id.find(t[4 + i]);
            if (it == blob_id.end() || !m.blobs[it->second].written)
                return refuse(err, MPMVS_SKYSEG_E_ORDER, "skyseg: layer " + L.name + " reads blob " + t[4 + i] + " before it is written");
            L.in.push_back(it->second);
        }
        for (long i = 0; i < no; ++i) {
            if (blob_id.count(t[4 + ni + i])) return refuse(err, MPMVS_SKYSEG_E_ORDER, "skyseg: layer " + L.name + " writes blob " + t[4 + ni + i] + " a second time");
            L.out.push_back(blob_of(t[4 + ni + i]));
        }
        auto in_blob = [&](int i) -> Blob& { return m.blobs[L.in[i]]; };
        auto set_out = [&](int i, int c, int h, int w, bool fresh, const std::vector<Seg>* segs) {
            Blob& b = m.blobs[L.out[i]];
            b.c = c, b.h = h, b.w = w, b.written = true;
            if (fresh) b.segs = {Seg{new_buf(c, h, w), 0, c}};
            else b.segs = *segs;
        };
        auto need = [&](long a, long b) { return ni == a && no == b; };
        const std::string shape_err = "skyseg: layer " + L.name + " has the wrong number of inputs or outputs";
        if (type == "Input") {
            L.op = OP_INPUT;
            if (!need(0, 1)) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            if (m.input_blob >= 0) return refuse(err, MPMVS_SKYSEG_E_LAYER, "skyseg: second Input layer " + L.name);
            m.input_blob = L.out[0];
            set_out(0, (int)geti(2, 0), in_h, in_w, true, nullptr);  // channels: parameter 2, else fixed by the first convolution that reads it
        } else if (type == "Convolution") {
            L.op = OP_CONV;
            if (!need(1, 1)) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            L.cout = (int)geti(0, 0), L.k = (int)geti(1, 0), L.dil = (int)geti(2, 1), L.pad = (int)geti(4, 0), L.has_bias = (int)geti(5, 0), L.act = (int)geti(9, 0);
            const long wcount = geti(6, 0);
            const std::string who = "skyseg: Convolution " + L.name;
            if (geti(3, 1) != 1 || geti(13, geti(3, 1)) != 1) return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": stride other than 1");
            if (geti(7, 1) != 1) return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": group other than 1");
            if (geti(11, L.k) != L.k || geti(12, L.dil) != L.dil || geti(14, L.pad) != L.pad || geti(15, L.pad) != L.pad || geti(16, L.pad) != L.pad)
                return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": non-square kernel, dilation or padding");
            if (geti(8, 0) != 0) return refuse(err, MPMVS_SKYSEG_E_TAG, who + ": int8 weights");
            if ((L.k != 1 && L.k != 3) || L.cout <= 0 || L.dil < 1 || L.dil > 64 || L.pad != L.dil * (L.k - 1) / 2 || getf(18, 0.0) != 0.0)
                return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": only 3x3 with pad = dilation and 1x1 are supported");
            if (L.act != 0 && L.act != 1 && L.act != 4) return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": activation other than none / ReLU / sigmoid");
            Blob& a = in_blob(0);
            const long per = (long)L.cout * L.k * L.k;
            if (wcount <= 0 || wcount % per) return refuse(err, MPMVS_SKYSEG_E_CONV, who + ": weight count is no multiple of outputs x kernel");
            L.cin = (int)(wcount / per);
            if (a.c == 0 && L.in[0] == m.input_blob) {  // the input's channel count is whatever its first reader takes
                a.c = L.cin;
                m.bufs[a.segs[0].buf].c = L.cin;
                a.segs[0].c = L.cin;
            }
            if (a.c != L.cin) return refuse(err, MPMVS_SKYSEG_E_SHAPE, who + ": weight count asks for " + std::to_string(L.cin) + " input channels, the blob has " + std::to_string(a.c));
            // weights: tag, block, then the biases
            if (bin_off + 4 > bin.size()) return refuse(err, MPMVS_SKYSEG_E_SHORT, who + ": weight file ends before the weight tag");
            uint32_t tag;
            std::memcpy(&tag, bin.data() + bin_off, 4);
            bin_off += 4;
            L.w_off = m.weights.size();
            if (tag == 0x01306B47u) {
                const size_t bytes = ((size_t)wcount * 2 + 3) / 4 * 4;
                if (bin_off + bytes > bin.size()) return refuse(err, MPMVS_SKYSEG_E_SHORT, who + ": weight file ends inside the weights");
                m.weights.resize(L.w_off + (size_t)wcount);
                for (long i = 0; i < wcount; ++i) {
                    uint16_t h;
                    std::memcpy(&h, bin.data() + bin_off + 2 * (size_t)i, 2);
                    m.weights[L.w_off + (size_t)i] = half_to_float(h);
                }
                bin_off += bytes;
            } else if (tag == 0u) {
                const size_t bytes = (size_t)wcount * 4;
                if (bin_off + bytes > bin.size()) return refuse(err, MPMVS_SKYSEG_E_SHORT, who + ": weight file ends inside the weights");
                m.weights.resize(L.w_off + (size_t)wcount);
                std::memcpy(m.weights.data() + L.w_off, bin.data() + bin_off, bytes);
                bin_off += bytes;
            } else {
                char hex[16];
                std::snprintf(hex, sizeof hex, "0x%08X", tag);
                return refuse(err, MPMVS_SKYSEG_E_TAG, who + ": weight tag " + hex + " (only fp16 0x01306B47 and raw fp32 0 are read)");
            }
            L.b_off = m.biases.size();
            m.biases.resize(L.b_off + (size_t)L.cout, 0.0f);
            if (L.has_bias) {
                const size_t bytes = (size_t)L.cout * 4;
                if (bin_off + bytes > bin.size()) return refuse(err, MPMVS_SKYSEG_E_SHORT, who + ": weight file ends inside the biases");
                std::memcpy(m.biases.data() + L.b_off, bin.data() + bin_off, bytes);
                bin_off += bytes;
            }
            set_out(0, L.cout, a.h, a.w, true, nullptr);
            ++m.n_conv;
        } else if (type == "Pooling") {
            L.op = OP_POOL;
            if (!need(1, 1)) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            if (geti(0, 0) != 0 || geti(1, 0) != 2 || geti(2, 1) != 2 || geti(3, 0) != 0 || geti(4, 0) != 0 || geti(5, 0) != 0 || geti(11, 2) != 2 || geti(12, 2) != 2 ||
                geti(13, 0) != 0 || geti(7, 0) != 0)
                return refuse(err, MPMVS_SKYSEG_E_POOL, "skyseg: Pooling " + L.name + ": only max 2x2 stride 2 in the default pad mode is supported");
            Blob& a = in_blob(0);
            set_out(0, a.c, (a.h + 1) / 2, (a.w + 1) / 2, true, nullptr);
        } else if (type == "Interp") {
            L.op = OP_INTERP;
            if (!need(1, 1)) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            const long oh = geti(3, 0), ow = geti(4, 0);
            if (geti(0, 0) != 2 || geti(6, 0) != 0 || oh <= 0 || ow <= 0 || oh > 8192 || ow > 8192 || geti(5, 0) != 0)
                return refuse(err, MPMVS_SKYSEG_E_INTERP, "skyseg: Interp " + L.name + ": only bilinear to a fixed size without align_corner is supported");
            Blob& a = in_blob(0);
            set_out(0, a.c, (int)oh, (int)ow, true, nullptr);
        } else if (type == "BinaryOp") {
            L.op = OP_ADD;
            if (geti(0, 0) != 0 || geti(1, 0) != 0 || ni != 2 || no != 1)
                return refuse(err, MPMVS_SKYSEG_E_BINARY, "skyseg: BinaryOp " + L.name + ": only the sum of two blobs is supported");
            Blob &a = in_blob(0), &b = in_blob(1);
            if (a.c != b.c || a.h != b.h || a.w != b.w)
                return refuse(err, MPMVS_SKYSEG_E_SHAPE, "skyseg: BinaryOp " + L.name + " adds blobs of different sizes (the graph does not close for this input size)");
            if (a.segs.size() != 1 || b.segs.size() != 1) return refuse(err, MPMVS_SKYSEG_E_BINARY, "skyseg: BinaryOp " + L.name + ": an operand is a Concat result");
            set_out(0, a.c, a.h, a.w, true, nullptr);
        } else if (type == "Concat") {
            L.op = OP_CONCAT;
            if (ni < 1 || no != 1 || geti(0, 0) != 0) return refuse(err, MPMVS_SKYSEG_E_LAYER, "skyseg: Concat " + L.name + ": only along channels");
            std::vector<Seg> segs;
            int c = 0;
            for (long i = 0; i < ni; ++i) {
                Blob& a = in_blob((int)i);
                if (a.h != in_blob(0).h || a.w != in_blob(0).w)
                    return refuse(err, MPMVS_SKYSEG_E_SHAPE, "skyseg: Concat " + L.name + " joins blobs of different sizes (the graph does not close for this input size)");
                segs.insert(segs.end(), a.segs.begin(), a.segs.end());
                c += a.c;
            }
            set_out(0, c, in_blob(0).h, in_blob(0).w, false, &segs);
        } else if (type == "Split") {
            L.op = OP_SPLIT;
            if (ni != 1 || no < 1) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            for (long i = 0; i < no; ++i) set_out((int)i, in_blob(0).c, in_blob(0).h, in_blob(0).w, false, &in_blob(0).segs);
        } else if (type == "Sigmoid") {
            L.op = OP_SIGMOID;
            if (!need(1, 1)) return refuse(err, MPMVS_SKYSEG_E_MAGIC, shape_err);
            set_out(0, in_blob(0).c, in_blob(0).h, in_blob(0).w, true, nullptr);
        } else {
            return refuse(err, MPMVS_SKYSEG_E_LAYER, "skyseg: layer " + L.name + " has the unsupported type " + type);
        }
        if (L.op != OP_INPUT && L.op != OP_CONV)
            for (int b : L.in)
                if (m.blobs[b].c == 0) return refuse(err, MPMVS_SKYSEG_E_SHAPE, "skyseg: layer " + L.name + " reads the input before a convolution fixed its channel count");
        if (L.op == OP_CONV) m.macs += (long long)L.cout * L.cin * L.k * L.k * m.blobs[L.out[0]].h * m.blobs[L.out[0]].w;
        m.layers.push_back(L);
    }
    if (m.input_blob < 0) return refuse(err, MPMVS_SKYSEG_E_LAYER, "skyseg: the graph has no Input layer");
    if (bin_off != bin.size())
        return refuse(err, MPMVS_SKYSEG_E_LEFTOVER, "skyseg: " + std::to_string(bin.size() - bin_off) + " bytes of the weight file are left over after the last convolution");
    m.weight_bytes = (long long)bin_off;

    // output: the named blob, or the output of the last layer
    if (output_name && *output_name) {
        auto it = blob_id.find(output_name);
        if (it == blob_id.end()) return refuse(err, MPMVS_SKYSEG_E_OUTPUT, std::string("skyseg: no blob named ") + output_name);
        m.output_blob = it->second;
    } else {
        m.output_blob = m.layers.back().out[0];
    }
    // liveness: walk back from the output
    std::vector<char> need_blob(m.blobs.size(), 0);
    need_blob[m.output_blob] = 1;
    for (int li = (int)m.layers.size() - 1; li >= 0; --li) {
        Layer& L = m.layers[li];
        bool used = false;
        for (int b : L.out) used = used || need_blob[b];
        L.live = used;
        if (used) {
            ++m.n_live;
            for (int b : L.in) need_blob[b] = 1;
        }
    }
    if (!m.layers.empty() && !need_blob[m.input_blob]) return refuse(err, MPMVS_SKYSEG_E_OUTPUT, "skyseg: the output does not depend on the input");
    // launch order and buffer lifetimes (position 0 = the upload of the input)
    for (int li = 0; li < (int)m.layers.size(); ++li) {
        const Layer& L = m.layers[li];
        if (!L.live) continue;
        int pos;
        if (L.op == OP_INPUT) pos = 0;
        else if (L.op == OP_SPLIT || L.op == OP_CONCAT) pos = -1;
        else {
            m.order.push_back(li);
            pos = (int)m.order.size();
        }
        if (pos < 0) continue;
        if (L.op == OP_CONV && (int)m.blobs[L.in[0]].segs.size() > MPMVS_SKYSEG_MAX_CONCAT)
            return refuse(err, MPMVS_SKYSEG_E_CONV, "skyseg: Convolution " + L.name + " reads a Concat of more than " + std::to_string(MPMVS_SKYSEG_MAX_CONCAT) + " parts");
        for (int b : L.in)
            for (const Seg& s : m.blobs[b].segs) m.bufs[s.buf].last = pos;
        Buf& o = m.bufs[m.blobs[L.out[0]].segs[0].buf];
        o.first = o.last = pos;
    }
    for (const Seg& s : m.blobs[m.output_blob].segs) m.bufs[s.buf].last = (int)m.order.size() + 1;
    plan(m, false);
    return 0;
}

}  // namespace skyseg
