// planar_prior.cpp -- host construction of the planar prior that feeds the
// second Run() of a Problem:
//   vertices   reference src/PatchMatch.cpp:782-853  GetTriangulateVertices
//   Delaunay   reference src/PatchMatch.cpp:757-780  (cv::Subdiv2D there)
//   plane fit  reference src/PatchMatch.cpp:723-755  (cv::SVD::solveZ there)
//   raster     reference src/PatchMatch.cpp:554-595
// OpenCV is absent from the target image, so the triangulation is an own
// divide-and-conquer Delaunay with exact integer predicates, and the 3-point
// null-space solve is the closed form (cross product).  Parity note: for point
// sets with four or more cocircular points (common on a pixel grid) the Delaunay
// triangulation is not unique and cv::Subdiv2D's choice, as well as its triangle
// ORDER (which decides which triangle owns a shared border pixel), cannot be
// reproduced without OpenCV: "parity unpinned" against the reference on those
// two points.  The vertex selection equals the reference's own
// GetTriangulateVertices compiled for the host (oracle/ref_host_driver.cpp),
// vertex for vertex under both rules: ties, partial cells, the never-assigned
// (0, 0) points and a NaN cost in a cell included
// (tests/test_reference_host_cpu.py).  The rest -- the raster, and the plane fit
// behind cv::SVD -- is pinned by fixtures generated without this repository
// (tests/golden/make_prior_golden.py: vertex selection and raster as
// step-by-step restatements, Delaunay triangle sets from Qhull on
// general-position points, planes from numpy's SVD;
// tests/test_prior_golden_cpu.py), the device kernels (csrc/pm_prior.hpp) equal
// this file bit for bit (tests/test_prior_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <memory>
#include <thread>
#include <unistd.h>
#include <vector>

#include "PatchMatch.h"

// a polite busy-wait step: the x86 PAUSE hint, the arm64 equivalent, or a yield anywhere else
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("isb" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

namespace mpmvs_host {
static std::atomic<int> g_concurrent_callers{1};
void SetConcurrentCallers(int k) { g_concurrent_callers.store(k < 1 ? 1 : k); }
int OmpThreads() {
    int base;
    if (const char* e = std::getenv("MPMVS_HOST_THREADS")) {
        base = std::max(1, std::atoi(e));
    } else {
        const unsigned hc = std::thread::hardware_concurrency();
        base = (int)std::min(16u, std::max(1u, hc));
    }
    return std::max(1, base / g_concurrent_callers.load(std::memory_order_relaxed));
}

// ---------------------------------------------------------------------------
// vertices: the image is cut into 5x5-pixel cells (smaller at the right / bottom border) and every cell may contribute its
// most reliable pixels (SURVEY a-16).  Two selection rules:
//   plain rule       the pixel of lowest cost, if that cost is a valid one (< 2) and below 0.1;
//   geometric rule   the (up to) three pixels of lowest cost among those with cost < 1 and geometric cost < 0.4, in
//                    ascending cost, as long as their cost stays below max(0.2, 0.85 * cell cost sum / (x_end * y_end)) --
//                    the divisor is the product of the cell's absolute END coordinates, not its area (the reference's
//                    formula, kept because it decides which vertices exist).
// Ties keep the first pixel in raster order.  Both rules are applied by CellPicker below, one cell at a time, cells in
// raster order, which is also the order of the vertex list.
// ---------------------------------------------------------------------------
namespace {
struct CellPicker {
    static constexpr int kCell = 5;
    const float* cost;
    const float* geom;
    int width, height;

    // lowest valid cost of the cell [x0, x1) x [y0, y1) and where it sits
    bool best_pixel(int x0, int y0, int x1, int y1, Point& where, float& lowest) const {
        lowest = 2.0f;
        bool any = false;
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                const float c = cost[(size_t)y * width + x];
                if (c < 2.0f && c < lowest) {
                    lowest = c;
                    where = Point(x, y);
                    any = true;
                }
            }
        return any;
    }

    // the three lowest costs among the geometrically consistent pixels of the cell, ascending; returns how many pass the
    // cell's adaptive threshold
    int best_three(int x0, int y0, int x1, int y1, Point (&where)[3]) const {
        float low[3] = {2.0f, 2.0f, 2.0f};
        float sum = 0.0f;
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                const size_t i = (size_t)y * width + x;
                const float c = cost[i];
                sum += c;
                if (!(c < 1.0f && geom[i] < 0.4f && c < low[2])) continue;
                // insert into the sorted triple; an equal cost stays behind the earlier pixel
                int slot = 2;
                while (slot > 0 && low[slot - 1] > c) {
                    low[slot] = low[slot - 1];
                    where[slot] = where[slot - 1];
                    --slot;
                }
                low[slot] = c;
                where[slot] = Point(x, y);
            }
        const float scaled = (float)((double)(sum / (float)(y1 * x1)) * 0.85);
        const float limit = scaled < 0.2f ? 0.2f : scaled;  // std::max(scaled, 0.2f) of ref :842: a NaN sum stays NaN, no vertex passes
        int n = 0;
        while (n < 3 && low[n] < limit) ++n;
        return n;
    }
};
}  // namespace

void TriangulateVertices(int width, int height, const float* costs, const float* geom_costs, bool geomPlanarPrior,
                         std::vector<Point>& Vertices) {
    Vertices.clear();
    const CellPicker pick{costs, geom_costs, width, height};
    for (int y0 = 0; y0 < height; y0 += CellPicker::kCell)
        for (int x0 = 0; x0 < width; x0 += CellPicker::kCell) {
            const int x1 = std::min(width, x0 + CellPicker::kCell), y1 = std::min(height, y0 + CellPicker::kCell);
            if (geomPlanarPrior) {
                // (0, 0) like the reference's `std::vector<cv::Point> points(3)` (ref :812): where the cell's threshold exceeds
                // the initial 2.0 -- costs of a geometric Run() reach 2.6, and the divisor of the first cells is small -- the
                // reference pushes these never-assigned points, i.e. pixel (0, 0) becomes a vertex
                Point p[3] = {Point(0, 0), Point(0, 0), Point(0, 0)};
                const int n = pick.best_three(x0, y0, x1, y1, p);
                Vertices.insert(Vertices.end(), p, p + n);
            } else {
                Point p;
                float lowest;
                if (pick.best_pixel(x0, y0, x1, y1, p, lowest) && lowest < 0.1f) Vertices.push_back(p);
            }
        }
}

// ---------------------------------------------------------------------------
// Delaunay triangulation: divide and conquer with alternating cuts, exact integer predicates, parallel subtrees.
//
// The point set is halved at the median along x, the halves along y, and so on (pieces stay roughly square, so a merge only
// touches the edges next to its seam).  Pieces of two or three points are built directly; two triangulated halves are zipped
// together from their lower common tangent upwards, deleting the edges of either side that fail the empty-circle test
// against the other side (Guibas & Stolfi 1985, with Dwyer's 1987 alternation of the cut direction).  A cut along y is the
// same procedure in the frame rotated by -90 degrees, (u, v) = (y, -x): orientation and in-circle tests do not change under
// a rotation, only the ORDER of the points (y ascending, ties x descending) and the two hull edges a piece hands to its
// parent do, and the latter are found by a walk around the piece's hull.
//
// Mesh: directed half-edges 2k / 2k+1 of edge k, each with its origin and its counter-clockwise / clockwise neighbour around
// that origin.  The piece of points [l, r) owns the edge slots [3l, 3r) (a planar graph on n points has fewer than 3n edges),
// so subtrees never share memory and the top levels of the recursion run on their own threads; the result -- triangles listed
// by their lowest half-edge -- does not depend on the number of threads.
// Cocircular quadruples (common on a pixel grid) keep whichever diagonal the zip meets first: a valid Delaunay triangulation,
// deterministic, not necessarily cv::Subdiv2D's choice (see the parity note at the top).
// ---------------------------------------------------------------------------
namespace {
typedef __int128 i128;

// Worker threads: a persistent pool, created on first use and pinned once, each worker to its own CPU of the process's
// affinity mask.  (Until round 3 every call spawned its own threads and pinned them: on the target hosts -- micro-VM kernels --
// a freshly created thread stays on its creator's CPU for tens of milliseconds, longer than the whole triangulation, and even
// with explicit placement the 15 thread creations and migrations of a call cost more than the triangulation itself:
// 22 ms on 16 threads against 60 ms on one.)  One call at a time uses the pool; a caller that finds it busy -- several
// Problems triangulate at once in the multi-Problem schedule -- runs its triangulation on its own thread instead.
// set in the child of a fork(): the pool object is inherited, its threads are not
static std::atomic<bool> g_pool_forked(false);

class HostPool {
    // One parallel sweep: its own object, shared with the workers by reference count, so that a worker that wakes late (descheduled
    // by another tenant of the host) finds an exhausted sweep and leaves -- it never meets the next sweep's parameters half-way and
    // the caller never waits for a thread that has nothing left to do.  (Until round 5 every worker had to check in and out of
    // every sweep: one worker scheduled a millisecond late cost every one of the ~20 level sweeps of a triangulation that
    // millisecond, 8 -> 23 ms from one call to the next on a shared host.)
    struct Sweep {
        std::function<void(int)> job;
        int ntasks = 0;
        std::atomic<int> next{0}, done{0};
    };
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable wake;
    std::shared_ptr<Sweep> current;          // guarded by mu
    std::atomic<unsigned long> generation{0};
    bool quit = false;
    std::mutex busy;

    static void take_part(Sweep& sw) {
        for (;;) {
            const int i = sw.next.fetch_add(1, std::memory_order_relaxed);
            if (i >= sw.ntasks) return;
            sw.job(i);
            sw.done.fetch_add(1, std::memory_order_release);
        }
    }
    void worker(int slot, std::vector<int> cpus) {
        if (cpus.size() >= 2) {
            cpu_set_t one;
            CPU_ZERO(&one);
            CPU_SET(cpus[(size_t)slot % cpus.size()], &one);
            pthread_setaffinity_np(pthread_self(), sizeof(one), &one);
        }
        unsigned long seen = 0;
        for (;;) {
            // the sweeps of one triangulation follow each other within microseconds: look for the next one for a moment before going
            // to sleep (a futex wake-up per worker and sweep otherwise)
            for (int spin = 0; spin < 4000 && generation.load(std::memory_order_acquire) == seen; ++spin) cpu_relax();
            std::shared_ptr<Sweep> sw;
            {
                std::unique_lock<std::mutex> lk(mu);
                wake.wait(lk, [&] { return quit || generation.load(std::memory_order_relaxed) != seen; });
                if (quit) return;
                seen = generation.load(std::memory_order_relaxed);
                sw = current;
            }
            if (sw) take_part(*sw);
        }
    }

   public:
    explicit HostPool(int threads) {
        // Pinning is opt-in since round 5 (MPMVS_HOST_PIN=1): the workers live as long as the process, so the scheduler has all the
        // time it needs to spread them, and a worker pinned to a CPU that another tenant of the host keeps busy cannot get away
        // from it.  (Round 2 pinned because its threads were created per call and stayed on their creator's CPU for longer than
        // the triangulation took.)
        std::vector<int> cpus;
        const char* pin = std::getenv("MPMVS_HOST_PIN");
        cpu_set_t set;
        CPU_ZERO(&set);
        if (pin && std::atoi(pin) != 0 && sched_getaffinity(0, sizeof(set), &set) == 0)
            for (int i = 0; i < CPU_SETSIZE; ++i)
                if (CPU_ISSET(i, &set)) cpus.push_back(i);
        // slot 0 is the caller's place: the workers take the CPUs after it, spread over the mask (SMT siblings are usually
        // numbered half the mask apart, so neighbours in the list are distinct cores).  Several processes of one box (one rank
        // per GPU) share the mask: each starts at its own stretch of it -- LOCAL_RANK x pool size, or a stretch picked by the
        // process id -- instead of all pinning onto the same CPUs.
        int base = 0;
        if (!cpus.empty()) {
            const char* lr = std::getenv("LOCAL_RANK");
            base = (int)(((lr ? (long)std::atoi(lr) : (long)(getpid() % 64)) * threads) % (long)cpus.size());
        }
        for (int t = 1; t < threads; ++t) workers.emplace_back(&HostPool::worker, this, base + t, cpus);
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        wake.notify_all();
        for (std::thread& t : workers) t.join();
    }
    int size() const { return (int)workers.size() + 1; }
    bool try_acquire() { return busy.try_lock(); }
    void release() { busy.unlock(); }
    // fn(i) for i in [0, n) on the workers and the caller; returns when every TASK is done (workers that are still on their way to
    // the sweep find it exhausted).  Only between try_acquire / release.
    void run(int n, const std::function<void(int)>& fn) {
        if (n <= 0) return;
        if (n == 1 || workers.empty()) {
            for (int i = 0; i < n; ++i) fn(i);
            return;
        }
        auto sw = std::make_shared<Sweep>();
        sw->job = fn;
        sw->ntasks = n;
        {
            std::lock_guard<std::mutex> lk(mu);
            current = sw;
            generation.fetch_add(1, std::memory_order_release);
        }
        wake.notify_all();
        take_part(*sw);
        while (sw->done.load(std::memory_order_acquire) < n) std::this_thread::yield();
    }
};

int HostThreads() {
    if (const char* e = std::getenv("MPMVS_HOST_THREADS")) return std::max(1, std::atoi(e));
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::min(16u, std::max(1u, hc));
}
// The pool of the process, acquired for one triangulation: nullptr when one thread is asked for or when another caller holds
// it.  It is rebuilt when MPMVS_HOST_THREADS asks for another size than it has (tests walk through thread counts).
HostPool* AcquireSharedPool() {
    static std::mutex mu;
    // never destroyed at process exit (a raw pointer, deliberately leaked): in the child of a fork() the object names threads
    // that do not exist there and its condition variable still counts the parent's waiters -- joining the one or destroying the
    // other blocks forever in exit().  Only a change of MPMVS_HOST_THREADS deletes a pool (in the process that built it).
    static HostPool* pool = nullptr;
    // a forked child inherits the pool object but not its threads: it triangulates on its own thread
    static const int registered = pthread_atfork(nullptr, nullptr, [] { g_pool_forked.store(true); });
    (void)registered;
    if (g_pool_forked.load(std::memory_order_relaxed)) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    const int want = HostThreads();
    if (want < 2) return nullptr;
    if (pool && pool->size() == want) return pool->try_acquire() ? pool : nullptr;
    if (pool) {
        if (!pool->try_acquire()) return nullptr;  // in use at its old size: this caller runs on its own thread
        pool->release();
        delete pool;
    }
    pool = new HostPool(want);
    return pool->try_acquire() ? pool : nullptr;
}

struct Zipper {
    const Point* P;
    bool wide;  // coordinates span 2^13 or more: the in-circle determinant needs 128 bits
    // not value-initialised: every piece sets up its own slots, so the pages are first touched by the thread that uses them
    std::unique_ptr<int[]> next, prev, org, ids;

    struct Piece {
        int le, re;              // ccw hull edge out of the first point / cw hull edge out of the last point (in the piece's order)
        int free_head, free_tail;  // unused edge slots of the piece, linked through next[]
    };

    static int sym(int e) { return e ^ 1; }
    int dest(int e) const { return org[e ^ 1]; }
    int lnext(int e) const { return prev[e ^ 1]; }
    int rprev(int e) const { return next[e ^ 1]; }

    long long ccw(int a, int b, int c) const {
        return (long long)(P[b].x - P[a].x) * (P[c].y - P[a].y) - (long long)(P[b].y - P[a].y) * (P[c].x - P[a].x);
    }
    bool left_of(int p, int e) const { return ccw(p, org[e], dest(e)) > 0; }
    bool right_of(int p, int e) const { return ccw(p, dest(e), org[e]) > 0; }
    // d strictly inside the circle through the counter-clockwise triangle (a, b, c)
    bool in_circle(int a, int b, int c, int d) const {
        const long long ax = P[a].x - P[d].x, ay = P[a].y - P[d].y, bx = P[b].x - P[d].x, by = P[b].y - P[d].y, cx = P[c].x - P[d].x,
                        cy = P[c].y - P[d].y;
        const long long a2 = ax * ax + ay * ay, b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
        if (!wide) return ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx) > 0;
        return (i128)ax * (by * c2 - b2 * cy) - (i128)ay * (bx * c2 - b2 * cx) + (i128)a2 * (bx * cy - by * cx) > 0;
    }
    // order of the points along the cut direction: axis 0 = (x, then y), axis 1 = (y, then -x)
    bool before(int axis, int a, int b) const {
        if (axis == 0) return P[a].x != P[b].x ? P[a].x < P[b].x : P[a].y < P[b].y;
        return P[a].y != P[b].y ? P[a].y < P[b].y : P[a].x > P[b].x;
    }

    void splice(int a, int b) {
        const int an = next[a], bn = next[b];
        next[a] = bn;
        next[b] = an;
        prev[bn] = a;
        prev[an] = b;
    }
    int make_edge(Piece& pc, int o, int d) {
        const int e = pc.free_head;
        pc.free_head = next[e];
        if (pc.free_head < 0) pc.free_tail = -1;
        next[e] = prev[e] = e;
        next[e ^ 1] = prev[e ^ 1] = e ^ 1;
        org[e] = o;
        org[e ^ 1] = d;
        return e;
    }
    void release(Piece& pc, int e) {
        e &= ~1;
        org[e] = org[e ^ 1] = -1;
        next[e] = pc.free_head;
        if (pc.free_head < 0) pc.free_tail = e;
        pc.free_head = e;
    }
    int connect(Piece& pc, int a, int b) {
        const int e = make_edge(pc, dest(a), org[b]);
        splice(e, lnext(a));
        splice(e ^ 1, b);
        return e;
    }
    void delete_edge(Piece& pc, int e) {
        splice(e, prev[e]);
        splice(e ^ 1, prev[e ^ 1]);
        release(pc, e);
    }

    // hull edges of a piece for a parent that cuts along `axis`: walk the hull counter-clockwise once
    void reorient(Piece& pc, int axis) const {
        int e = pc.le, lo = pc.le, hi_in = -1;
        int vmin = org[e], vmax = -1;
        do {
            const int v = dest(e);  // e arrives at v, rprev(e) leaves it along the hull
            if (vmax < 0 || before(axis, vmax, v)) {
                vmax = v;
                hi_in = e;
            }
            const int out = rprev(e);
            if (before(axis, v, vmin)) {
                vmin = v;
                lo = out;
            }
            e = out;
        } while (e != pc.le);
        pc.le = lo;
        pc.re = sym(hi_in);
    }

    Piece leaf(int l, int r, int axis) {
        const int n = r - l;
        std::sort(ids.get() + l, ids.get() + r, [&](int a, int b) { return before(axis, a, b); });
        Piece pc;
        pc.free_head = pc.free_tail = -1;
        for (int k = 3 * r - 1; k >= 3 * l; --k) {  // every slot of the piece starts free, lowest slot first
            org[2 * k] = org[2 * k + 1] = -1;
            next[2 * k] = pc.free_head;
            if (pc.free_head < 0) pc.free_tail = 2 * k;
            pc.free_head = 2 * k;
        }
        const int s1 = ids[l], s2 = ids[l + 1];
        const int a = make_edge(pc, s1, s2);
        if (n == 2) {
            pc.le = a;
            pc.re = a ^ 1;
            return pc;
        }
        const int s3 = ids[l + 2];
        const int b = make_edge(pc, s2, s3);
        splice(a ^ 1, b);
        const long long o = ccw(s1, s2, s3);
        if (o > 0) {
            connect(pc, b, a);
            pc.le = a;
            pc.re = b ^ 1;
        } else if (o < 0) {
            const int c = connect(pc, b, a);
            pc.le = c ^ 1;
            pc.re = c;
        } else {  // collinear: a chain of two edges
            pc.le = a;
            pc.re = b ^ 1;
        }
        return pc;
    }

    // the piece of the points ids[l .. r), cut along `axis`, on the calling thread
    Piece build(int l, int r, int axis) {
        const int n = r - l;
        if (n <= 3) return leaf(l, r, axis);
        const int m = l + n / 2;
        split(l, m, r, axis);
        Piece L = build(l, m, axis ^ 1);
        Piece R = build(m, r, axis ^ 1);
        return merge(L, R, axis);
    }
    void split(int l, int m, int r, int axis) {
        std::nth_element(ids.get() + l, ids.get() + m, ids.get() + r, [&](int a, int b) { return before(axis, a, b); });
    }
    // zips the triangulated halves of a cut along `axis` together
    Piece merge(Piece L, Piece R, int axis) {
        reorient(L, axis);
        reorient(R, axis);
        Piece pc;
        // the free slots of both halves serve the merge
        if (L.free_head < 0) {
            pc.free_head = R.free_head;
            pc.free_tail = R.free_tail;
        } else {
            pc.free_head = L.free_head;
            pc.free_tail = L.free_tail;
            if (R.free_head >= 0) {
                next[L.free_tail] = R.free_head;
                pc.free_tail = R.free_tail;
            }
        }
        int ldo = L.le, ldi = L.re, rdi = R.le, rdo = R.re;
        // lower common tangent
        for (;;) {
            if (left_of(org[rdi], ldi))
                ldi = lnext(ldi);
            else if (right_of(org[ldi], rdi))
                rdi = rprev(rdi);
            else
                break;
        }
        int basel = connect(pc, sym(rdi), ldi);
        if (org[ldi] == org[ldo]) ldo = sym(basel);
        if (org[rdi] == org[rdo]) rdo = basel;
        for (;;) {
            int lcand = next[sym(basel)];
            const bool lvalid0 = right_of(dest(lcand), basel);
            if (lvalid0)
                while (in_circle(dest(basel), org[basel], dest(lcand), dest(next[lcand]))) {
                    const int t = next[lcand];
                    delete_edge(pc, lcand);
                    lcand = t;
                }
            int rcand = prev[basel];
            const bool rvalid0 = right_of(dest(rcand), basel);
            if (rvalid0)
                while (in_circle(dest(basel), org[basel], dest(rcand), dest(prev[rcand]))) {
                    const int t = prev[rcand];
                    delete_edge(pc, rcand);
                    rcand = t;
                }
            const bool lvalid = right_of(dest(lcand), basel), rvalid = right_of(dest(rcand), basel);
            if (!lvalid && !rvalid) break;
            if (!lvalid || (rvalid && in_circle(dest(lcand), org[lcand], org[rcand], dest(rcand))))
                basel = connect(pc, rcand, sym(basel));
            else
                basel = connect(pc, sym(basel), sym(lcand));
        }
        pc.le = ldo;
        pc.re = rdo;
        return pc;
    }
};

}  // namespace

namespace {
// distinct points (the first occurrence stays): a bitmap over the bounding box, or a sort when that would be huge.
// Returns false when the extent is beyond the exact range of the predicates.
bool DistinctPoints(const Point* pts, size_t count, std::vector<Point>& out, bool& wide) {
    out.clear();
    if (count == 0) return true;
    int x0 = pts[0].x, x1 = x0, y0 = pts[0].y, y1 = y0;
    for (size_t i = 0; i < count; ++i) {
        x0 = std::min(x0, pts[i].x);
        x1 = std::max(x1, pts[i].x);
        y0 = std::min(y0, pts[i].y);
        y1 = std::max(y1, pts[i].y);
    }
    const long long bw = (long long)x1 - x0 + 1, bh = (long long)y1 - y0 + 1;
    if (bw >= (1 << 24) || bh >= (1 << 24)) return false;  // the 128-bit in-circle determinant is exact below 2^24
    wide = bw >= (1 << 13) || bh >= (1 << 13);
    out.reserve(count);
    if (bw * bh <= (1LL << 28)) {
        std::vector<uint64_t> seen((size_t)((bw * bh + 63) / 64), 0);
        for (size_t i = 0; i < count; ++i) {
            const long long k = (long long)(pts[i].y - y0) * bw + (pts[i].x - x0);
            if (seen[(size_t)(k >> 6)] >> (k & 63) & 1) continue;
            seen[(size_t)(k >> 6)] |= 1ULL << (k & 63);
            out.push_back(pts[i]);
        }
    } else {
        std::vector<size_t> idx(count);
        for (size_t i = 0; i < count; ++i) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return pts[a].x != pts[b].x ? pts[a].x < pts[b].x : pts[a].y < pts[b].y; });
        std::vector<char> keep(count, 1);
        for (size_t i = 1; i < count; ++i)
            if (pts[idx[i]].x == pts[idx[i - 1]].x && pts[idx[i]].y == pts[idx[i - 1]].y) keep[idx[i]] = 0;
        for (size_t i = 0; i < count; ++i)
            if (keep[i]) out.push_back(pts[i]);
    }
    return true;
}

// A finished triangulation; triangles are listed by their lowest half-edge, in half-edge order.
struct Triangulation {
    std::vector<Point> pts;
    Zipper z;
    HostPool* pool = nullptr;  // held for the duration of run() + write() when not null
    int chunks = 1, E = 0;
    std::vector<size_t> first;  // first[c] = number of triangles in the half-edge chunks before c; first[chunks] = total
    // Every chunk of half-edges lists its triangles ONCE into a staging buffer of its own (first touched by the thread that
    // fills it); write() then only copies.  (Until round 3 the faces were walked twice, once to count and once to write:
    // two pointer-chasing passes over 6 n half-edges.)
    std::vector<std::unique_ptr<Triangle[]>> staged;

    ~Triangulation() {
        if (pool) pool->release();
    }

    // the triangles whose lowest half-edge lies in [e0, e1), written to out; returns their number
    size_t faces(int e0, int e1, Triangle* out) const {
        size_t k = 0;
        for (int e = e0; e < e1; ++e) {
            const int a = z.org[e];
            if (a < 0) continue;
            const int e2 = z.lnext(e);
            if (e2 < e) continue;
            const int e3 = z.lnext(e2);
            if (e3 < e || z.dest(e3) != a) continue;
            const int b = z.org[e2], c = z.org[e3];
            if (z.ccw(a, b, c) <= 0) continue;  // the outer face of a three-cornered hull
            out[k++] = Triangle(pts[(size_t)a], pts[(size_t)b], pts[(size_t)c]);
        }
        return k;
    }
    void parallel(int n, const std::function<void(int)>& fn) const {
        if (pool)
            pool->run(n, fn);
        else
            for (int i = 0; i < n; ++i) fn(i);
    }
    int chunk_begin(int c) const { return (int)((long long)E * c / chunks); }

    // Divide and conquer, level by level, so that every level is one parallel sweep of the pool: the cuts of the top `depth`
    // levels (level d: 2^d medians, each over its own range), then the 2^depth subtrees (each built on one thread), then the
    // merges back up.  The ranges, the order of the points inside them and therefore the triangulation are the ones the plain
    // recursion produces: the result does not depend on the number of threads.
    void build_levels(int n, int depth) {
        std::vector<std::vector<int>> bound((size_t)depth + 1);  // bound[d]: the 2^d + 1 range boundaries of level d
        bound[0] = {0, n};
        for (int d = 0; d < depth; ++d) {
            const std::vector<int>& b = bound[(size_t)d];
            std::vector<int>& nb = bound[(size_t)d + 1];
            nb.resize(2 * (b.size() - 1) + 1);
            for (size_t i = 0; i + 1 < b.size(); ++i) {
                nb[2 * i] = b[i];
                nb[2 * i + 1] = b[i] + (b[i + 1] - b[i]) / 2;
            }
            nb.back() = n;
            parallel((int)b.size() - 1, [&](int i) { z.split(b[(size_t)i], nb[2 * (size_t)i + 1], b[(size_t)i + 1], d & 1); });
        }
        std::vector<Zipper::Piece> piece((size_t)1 << depth);
        const std::vector<int>& lb = bound[(size_t)depth];
        parallel((int)piece.size(), [&](int i) { piece[(size_t)i] = z.build(lb[(size_t)i], lb[(size_t)i + 1], depth & 1); });
        for (int d = depth - 1; d >= 0; --d) {
            std::vector<Zipper::Piece> up((size_t)1 << d);
            parallel((int)up.size(), [&](int i) { up[(size_t)i] = z.merge(piece[2 * (size_t)i], piece[2 * (size_t)i + 1], d & 1); });
            piece.swap(up);
        }
    }

    bool run(const Point* points, size_t count) {
        bool wide = false;
        const bool timing = std::getenv("MPMVS_HOST_TIMING") != nullptr;
        auto t_prev = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (!timing) return;
            const auto now = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[mpmvs_host]     delaunay: %-18s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
            t_prev = now;
        };
        if (!DistinctPoints(points, count, pts, wide)) return false;
        lap("distinct points");
        const int n = (int)pts.size();
        first.assign(2, 0);
        if (n < 3) return true;
        z.P = pts.data();
        z.wide = wide;
        z.next.reset(new int[(size_t)6 * n]);
        z.prev.reset(new int[(size_t)6 * n]);
        z.org.reset(new int[(size_t)6 * n]);
        z.ids.reset(new int[(size_t)n]);
        for (int i = 0; i < n; ++i) z.ids[i] = i;
        if (n >= 4096) {
            pool = AcquireSharedPool();  // nullptr: one thread asked for, or another Problem's triangulation has the pool -- run on this thread
        }
        const int threads = pool ? pool->size() : 1;
        lap("allocate");
        // four subtrees per thread: the pool's dynamic claiming evens out what the point distribution makes uneven
        int depth = 0;
        while (pool && (1 << depth) < 4 * threads && (n >> (depth + 1)) >= 512) ++depth;
        build_levels(n, depth);
        lap("build");
        E = 6 * n;
        chunks = pool ? 4 * threads : 1;
        std::vector<size_t> counts((size_t)chunks, 0);
        staged.resize((size_t)chunks);
        parallel(chunks, [&](int c) {
            // a triangle is listed by its lowest half-edge and a face has three: at most one triangle per half-edge of the chunk
            const int e0 = chunk_begin(c), e1 = chunk_begin(c + 1);
            staged[(size_t)c].reset(new Triangle[(size_t)(e1 - e0)]);  // Triangle() writes nothing: only the pages that get used are touched
            counts[(size_t)c] = faces(e0, e1, staged[(size_t)c].get());
        });
        first.assign((size_t)chunks + 1, 0);
        for (int c = 0; c < chunks; ++c) first[(size_t)c + 1] = first[(size_t)c] + counts[(size_t)c];
        lap("list faces");
        return true;
    }
    size_t total() const { return first.back(); }
    // all triangles into out[0 .. total())
    void write(Triangle* out) const {
        if (total() == 0) return;
        parallel(chunks, [&](int c) {
            const size_t k = first[(size_t)c + 1] - first[(size_t)c];
            if (k) std::memcpy(static_cast<void*>(out + first[(size_t)c]), staged[(size_t)c].get(), k * sizeof(Triangle));
        });
    }
};
}  // namespace

std::vector<Triangle> Delaunay(const Rect boundRC, const std::vector<Point>& points) {
    (void)boundRC;
    std::vector<Triangle> results;
    const bool timing = std::getenv("MPMVS_HOST_TIMING") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mpmvs_host]     delaunay: %-18s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    };
    {
        Triangulation t;
        if (!t.run(points.data(), points.size())) return results;
        lap("(run)");
        results.resize(t.total());
        lap("result storage");
        t.write(results.data());
        lap("copy out");
    }
    lap("release");
    return results;
}

// the same from / into plain arrays (xy pairs in, six ints per triangle out): returns the number of triangles, writes them only
// if they all fit into `cap`; -1 when the coordinates are out of range
long long DelaunayXY(const int* xy, size_t count, int* tri_xy, size_t cap) {
    static_assert(sizeof(Point) == 2 * sizeof(int) && sizeof(Triangle) == 6 * sizeof(int), "Point / Triangle are plain int tuples");
    Triangulation t;
    if (!t.run(reinterpret_cast<const Point*>(xy), count)) return -1;
    if (t.total() <= cap) t.write(reinterpret_cast<Triangle*>(tri_xy));
    return (long long)t.total();
}

// ---------------------------------------------------------------------------
// plane through the three back-projected triangle vertices
// ---------------------------------------------------------------------------
static void point_on_ref_cam(const Camera& cam, int x, int y, float depth, double X[3]) {
    // reference src/PatchMatch.cpp:200-209 (Get3DPointonRefCam), fp32 there
    X[0] = (double)(depth * ((float)x - cam.K[2]) / cam.K[0]);
    X[1] = (double)(depth * ((float)y - cam.K[5]) / cam.K[4]);
    X[2] = (double)depth;
}

float4 PriorPlane(const Camera& cam, const Triangle& t, const float4* planes, int width) {
    double X1[3], X2[3], X3[3];
    point_on_ref_cam(cam, t.pt1.x, t.pt1.y, planes[(size_t)t.pt1.y * width + t.pt1.x].w, X1);
    point_on_ref_cam(cam, t.pt2.x, t.pt2.y, planes[(size_t)t.pt2.y * width + t.pt2.x].w, X2);
    point_on_ref_cam(cam, t.pt3.x, t.pt3.y, planes[(size_t)t.pt3.y * width + t.pt3.x].w, X3);
    const double u[3] = {X2[0] - X1[0], X2[1] - X1[1], X2[2] - X1[2]};
    const double v[3] = {X3[0] - X1[0], X3[1] - X1[1], X3[2] - X1[2]};
    double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    double norm = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(norm > 1e-30)) {  // collinear points: no unique plane; take the fronto-parallel one
        n[0] = 0.0;
        n[1] = 0.0;
        n[2] = -1.0;
        norm = 1.0;
    }
    double d = -(n[0] * X1[0] + n[1] * X1[1] + n[2] * X1[2]);
    if (d < 0) norm = -norm;  // reference src/PatchMatch.cpp:746-752: offset made positive
    float4 o;
    o.x = (float)(n[0] / norm);
    o.y = (float)(n[1] / norm);
    o.z = (float)(n[2] / norm);
    o.w = (float)(d / norm);
    return o;
}

static float depth_from_plane(const Camera& cam, const float4 pl, int x, int y) {
    // reference src/PatchMatch.cpp:650-653
    return -pl.w * cam.K[0] / (((float)x - cam.K[2]) * pl.x + (cam.K[0] / cam.K[4]) * ((float)y - cam.K[5]) * pl.y + cam.K[0] * pl.z);
}

void BuildPrior(const Camera& cam, int width, int height, const std::vector<Triangle>& triangles, const float4* planes,
                float depth_min, float depth_max, std::vector<float4>& planeParams, Image& mask) {
    const Rect imageRC{0, 0, width, height};
    // triangles the reference keeps (all three vertices inside the image), in order:
    // triangle k gets label k + 1 and its plane is planeParams[k]
    std::vector<int> keep;
    keep.reserve(triangles.size());
    for (size_t i = 0; i < triangles.size(); ++i) {
        const Triangle& t = triangles[i];
        if (imageRC.contains(t.pt1) && imageRC.contains(t.pt2) && imageRC.contains(t.pt3)) keep.push_back((int)i);
    }
    planeParams.assign(keep.size(), float4{0, 0, 0, 0});
    // A pixel covered by several triangles keeps the label of the LAST one in the
    // reference's sequential loop = the largest label: an atomic max over triangles
    // processed in parallel gives the same mask.
    std::vector<uint32_t> label((size_t)width * height, 0u);
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(dynamic, 256)
    for (long k = 0; k < (long)keep.size(); ++k) {
        const Triangle& t = triangles[keep[k]];
        const uint32_t lab = (uint32_t)k + 1u;
        // the squares in double as the reference's pow(.., 2) forms them (src/PatchMatch.cpp:557-559): an int product wraps from 46 341 px on
        auto edge = [](Point a, Point b) {
            const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y;
            return (float)std::sqrt(dx * dx + dy * dy);
        };
        const float L01 = edge(t.pt1, t.pt2), L02 = edge(t.pt1, t.pt3), L12 = edge(t.pt2, t.pt3);
        const float max_edge = std::max(L01, std::max(L02, L12));
        const float step = (float)(1.0 / max_edge);
        // barycentric stepping of the reference (src/PatchMatch.cpp:564-570)
        for (float p = 0; p < 1.0; p += step) {
            for (float q = 0; q < 1.0 - p; q += step) {
                const int x = (int)((double)(p * (float)t.pt1.x + q * (float)t.pt2.x) + (1.0 - p - q) * t.pt3.x);
                const int y = (int)((double)(p * (float)t.pt1.y + q * (float)t.pt2.y) + (1.0 - p - q) * t.pt3.y);
                if (x >= 0 && y >= 0 && x < width && y < height) {
                    uint32_t* cell = &label[(size_t)y * width + x];
                    uint32_t cur = __atomic_load_n(cell, __ATOMIC_RELAXED);
                    while (cur < lab && !__atomic_compare_exchange_n(cell, &cur, lab, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
                    }
                }
            }
            if (!(step > 0.0f) || !std::isfinite(step)) break;  // degenerate triangle: one sample
        }
        planeParams[k] = PriorPlane(cam, t, planes, width);
    }
    mask = Image(height, width, 1, 0.0f);
#pragma omp parallel for num_threads(mpmvs_host::OmpThreads()) schedule(static)
    for (int j = 0; j < height; ++j)
        for (int i = 0; i < width; ++i) {
            const uint32_t lab = label[(size_t)j * width + i];
            if (lab > 0) {
                const float d = depth_from_plane(cam, planeParams[lab - 1], i, j);
                if (d <= depth_max && d >= depth_min) mask.data[(size_t)j * width + i] = (float)lab;  // (not at(): no stamp write from a parallel loop)
            }
        }
}

}  // namespace mpmvs_host
