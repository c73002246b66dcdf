// pm_stage.hpp -- the host-only half of the image upload (mpmvs_api.hip, upload_views): where each image lies in the staging
// buffer, how the images are grouped under the staging limit, and the row work that fills the buffer on a few host threads.
// No HIP header and nothing of mpmvs_ctx: tests/stage_cpu_main.cpp compiles this file alone and checks every staged byte.
#pragma once

#include <pthread.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace pmstage {

// a small persistent pool for the row work (thread creation costs as much as converting an image); a caller that finds it
// busy -- several Problems upload at once in the multi-Problem schedule -- works with a few short-lived threads instead
class RowPool {
    std::vector<std::thread> workers;
    std::mutex mu, busy;
    std::condition_variable wake;
    const std::function<void()>* job = nullptr;
    std::atomic<int> running{0};
    unsigned long generation = 0;
    bool quit = false;
    void worker() {
        unsigned long seen = 0;
        for (;;) {
            const std::function<void()>* fn;
            {
                std::unique_lock<std::mutex> lk(mu);
                wake.wait(lk, [&] { return quit || generation != seen; });
                if (quit) return;
                seen = generation;
                fn = job;
            }
            (*fn)();
            running.fetch_sub(1, std::memory_order_release);
        }
    }

   public:
    RowPool() {
        const unsigned hw = std::thread::hardware_concurrency();
        const int n = (int)std::max(1u, std::min(16u, hw ? hw : 1u));
        for (int t = 1; t < n; ++t) workers.emplace_back(&RowPool::worker, this);
    }
    ~RowPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        wake.notify_all();
        for (std::thread& t : workers) t.join();
    }
    // a forked child inherits this object but not its threads: it works on its own thread
    static std::atomic<bool>& forked() {
        static std::atomic<bool> f(false);
        return f;
    }
    // fn() on every worker and on the caller (fn pulls its own work items from a shared counter)
    void run(const std::function<void()>& fn) {
        if (forked().load(std::memory_order_relaxed)) {
            fn();
            return;
        }
        if (!busy.try_lock()) {
            std::vector<std::thread> tmp;
            for (int t = 0; t < 3; ++t) tmp.emplace_back(fn);
            fn();
            for (std::thread& t : tmp) t.join();
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            job = &fn;
            running.store((int)workers.size(), std::memory_order_relaxed);
            ++generation;
        }
        wake.notify_all();
        fn();
        while (running.load(std::memory_order_acquire) > 0) std::this_thread::yield();
        busy.unlock();
    }
};
inline RowPool& row_pool() {
    // deliberately leaked (never destroyed at process exit): in the child of a fork() the object names threads that do not exist
    // there and its condition variable still counts the parent's waiters -- joining / destroying them blocks forever in exit()
    static RowPool& p = *new RowPool;
    static const int registered = pthread_atfork(nullptr, nullptr, [] { RowPool::forked().store(true); });
    (void)registered;
    return p;
}

// one image as the caller holds it and as it is staged: w x h pixels, rows `pitch` bytes apart
struct HostImage {
    const char* px;
    int w, h;
    size_t pitch;
};

// Deals the rows of images [first, last) to the pool in chunks of `chunk` consecutive rows (counted through the images one after
// another).  For each piece of a chunk that lies in one image: body(image, first_row, n_rows), on whichever thread drew the chunk.
template <class Body>
inline void deal_rows(const HostImage* im, int first, int last, long chunk, Body&& body) {
    std::vector<long> row0(last - first + 1, 0);
    for (int i = first; i < last; ++i) row0[i - first + 1] = row0[i - first] + im[i].h;
    const long total_rows = row0[last - first];
    std::atomic<long> next(0);
    const std::function<void()> work = [&]() {
        for (;;) {
            const long r0 = next.fetch_add(chunk);
            if (r0 >= total_rows) return;
            const long r1 = std::min(r0 + chunk, total_rows);
            int k = 0;
            for (long r = r0; r < r1;) {
                while (r >= row0[k + 1]) ++k;
                const long rows = std::min(r1, row0[k + 1]) - r;   // of this image in this chunk
                body(first + k, (int)(r - row0[k]), (int)rows);
                r += rows;
            }
        }
    };
    row_pool().run(work);
}

// The images are staged in GROUPS of consecutive views of at most MPMVS_STAGE_MB (default 512) megabytes: ordinary inputs are
// one group (one pass over the images, no synchronisation); very many large views (33 x 3200 x 3200 floats = 1.35 GB) go
// through bounded staging buffers that are re-used group by group.
inline size_t stage_limit_bytes() {
    size_t limit = 512;
    if (const char* e = std::getenv("MPMVS_STAGE_MB")) limit = (size_t)std::max(1, std::atoi(e));
    return limit << 20;
}

struct StagePlan {
    std::vector<size_t> slot;       // slot[i]: byte offset of image i among ALL images, 256-byte aligned; slot[n] ends the last
    std::vector<int> group_first;   // group g holds the images [group_first[g], group_first[g + 1])
    size_t stage_bytes = 0;         // the largest group: the size of the staging buffer (and of its device twin)
    int groups() const { return (int)group_first.size() - 1; }
    // where image i of group g starts in the staging buffer
    size_t at(int g, int i) const { return slot[i] - slot[group_first[g]]; }
};

// a slot of w * h * px_bytes per image; a group is closed before the image that would take it past `limit` (one image is never split)
inline StagePlan plan_stage(const HostImage* im, int n, size_t px_bytes, size_t limit) {
    StagePlan p;
    p.slot.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) p.slot[i + 1] = p.slot[i] + (((size_t)im[i].w * im[i].h * px_bytes + 255) & ~(size_t)255);
    p.group_first.push_back(0);
    for (int i = 1; i < n; ++i)
        if (p.slot[i + 1] - p.slot[p.group_first.back()] > limit) p.group_first.push_back(i);
    p.group_first.push_back(n);
    for (int g = 0; g < p.groups(); ++g) p.stage_bytes = std::max(p.stage_bytes, p.slot[p.group_first[g + 1]] - p.slot[p.group_first[g]]);
    return p;
}

// The byte entry: rows of bytes, copied as they are.  Contiguous rows of a span go in one memcpy.
inline void stage_byte_rows(const HostImage* im, const StagePlan& plan, int g, char* stage) {
    deal_rows(im, plan.group_first[g], plan.group_first[g + 1], 64, [&](int i, int y, int rows) {
        const size_t w = (size_t)im[i].w, pitch = im[i].pitch;
        char* o = stage + plan.at(g, i) + (size_t)y * w;
        const char* in = im[i].px + (size_t)y * pitch;
        if (pitch == w)
            std::memcpy(o, in, (size_t)rows * w);
        else
            for (int q = 0; q < rows; ++q) std::memcpy(o + (size_t)q * w, in + (size_t)q * pitch, w);
    });
}

// Is every pixel of the fp32 rows an integer in [0, 255] (the reference's imread(GRAYSCALE) -> CV_32F input, ref .cpp:877-882)?
// The reference image is one group (view 0: ref_u8), the sources another (the texture format is the same for all of them: src_u8);
// a group's rows are skipped once its flag has dropped.  STAGE: the rows are written as bytes on the way, image i as w * h bytes at
// slot[i] -- optimistically, whatever turns out inexact is staged again by stage_known.
template <bool STAGE>
inline void exact_sweep(const HostImage* im, int n, bool try_src_u8, char* stage, const StagePlan* plan, bool& ref_u8, bool& src_u8) {
    std::atomic<bool> ref_exact(true), src_exact(try_src_u8);
    deal_rows(im, 0, n, 32, [&](int i, int y0, int rows) {
        std::atomic<bool>& exact = i == 0 ? ref_exact : src_exact;
        const int w = im[i].w;
        for (int y = y0; y < y0 + rows; ++y) {
            if (!exact.load(std::memory_order_relaxed)) return;
            const float* row = (const float*)(im[i].px + (size_t)y * im[i].pitch);
            unsigned char* o = nullptr;
            if constexpr (STAGE) o = (unsigned char*)(stage + plan->slot[i]) + (size_t)y * w;
            bool ok = true;
            for (int x = 0; x < w; ++x) {
                const float f = row[x];
                const int q = (int)(f >= 0.0f && f <= 255.0f ? f : -1.0f);
                ok &= (float)q == f;
                if constexpr (STAGE) o[x] = (unsigned char)q;
            }
            if (!ok) exact.store(false, std::memory_order_relaxed);
        }
    });
    ref_u8 = ref_exact.load();
    src_u8 = src_exact.load();
}

// Stages the fp32 images of group g whose formats are known (ref_u8 / src_u8): bytes or fp32 rows.  only_f32: the byte rows are
// there already (the staging sweep of exact_sweep wrote them).
inline void stage_known(const HostImage* im, const StagePlan& plan, int g, char* stage, bool ref_u8, bool src_u8, bool only_f32 = false) {
    deal_rows(im, plan.group_first[g], plan.group_first[g + 1], 32, [&](int i, int y0, int rows) {
        const bool u8 = i == 0 ? ref_u8 : src_u8;
        if (u8 && only_f32) return;
        const size_t w = (size_t)im[i].w;
        char* base = stage + plan.at(g, i);
        for (int y = y0; y < y0 + rows; ++y) {
            const float* row = (const float*)(im[i].px + (size_t)y * im[i].pitch);
            if (u8) {
                unsigned char* o = (unsigned char*)base + (size_t)y * w;
                for (size_t x = 0; x < w; ++x) o[x] = (unsigned char)(int)row[x];
            } else {
                std::memcpy(base + (size_t)y * w * 4, row, w * 4);
            }
        }
    });
}

// The fp32 entry with ONE group decides the formats WHILE it stages: one optimistic byte sweep over all images, then a second
// sweep only for the fp32 rows of whatever turned out not to be 8-bit exact.
inline void stage_deciding(const HostImage* im, int n, const StagePlan& plan, bool try_src_u8, char* stage, bool& ref_u8, bool& src_u8) {
    exact_sweep<true>(im, n, try_src_u8, stage, &plan, ref_u8, src_u8);
    if (!(ref_u8 && src_u8)) stage_known(im, plan, 0, stage, ref_u8, src_u8, true);
}

}  // namespace pmstage
