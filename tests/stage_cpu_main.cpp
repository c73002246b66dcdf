// Stand-alone check of mp-mvs_amd/csrc/pm_stage.hpp (built and run by tests/test_stage_cpu.py; no GPU, no HIP): images are
// staged into plain malloc'ed buffers through the staging plan and the row dealer -- the byte copy of mpmvs_set_views_u8, the
// deciding and the known-format sweeps of mpmvs_set_views -- and every staged byte is compared with a naive double loop; the
// bytes between and after the slots must keep their fill pattern.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pm_stage.hpp"

using namespace pmstage;

namespace {
constexpr unsigned char kFill = 0xA5;
constexpr size_t kTail = 64;   // guard bytes behind the staging buffer
int g_checks = 0, g_failed = 0;

#define EXPECT(cond, ...)                         \
    do {                                          \
        ++g_checks;                               \
        if (!(cond)) {                            \
            ++g_failed;                           \
            std::printf("FAILED %s: ", #cond);    \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
        }                                         \
    } while (0)

struct Size {
    int w, h, pad;   // pad: extra PIXELS per row of the caller's array
};

unsigned pixel(int i, int x, int y) { return ((unsigned)i * 131u + (unsigned)x * 7u + (unsigned)y * 13u + ((unsigned)(x * y) >> 2)) & 255u; }

// the caller's arrays of one case; T = unsigned char or float
template <class T>
struct Images {
    std::vector<std::vector<T>> px;
    std::vector<HostImage> im;
    explicit Images(const std::vector<Size>& sizes) {
        for (size_t i = 0; i < sizes.size(); ++i) {
            const Size s = sizes[i];
            const size_t pitch = (size_t)s.w + s.pad;
            px.emplace_back(pitch * s.h, (T)77);   // (the padding holds a value no staged byte may pick up by accident: see at())
            for (int y = 0; y < s.h; ++y)
                for (int x = 0; x < s.w; ++x) px[i][y * pitch + x] = (T)pixel((int)i, x, y);
        }
        for (size_t i = 0; i < sizes.size(); ++i) im.push_back({(const char*)px[i].data(), sizes[i].w, sizes[i].h, ((size_t)sizes[i].w + sizes[i].pad) * sizeof(T)});
    }
    T at(int i, int x, int y) const { return px[i][(size_t)y * (im[i].pitch / sizeof(T)) + x]; }
    int n() const { return (int)im.size(); }
};

struct Stage {
    std::vector<unsigned char> buf;
    explicit Stage(size_t bytes) : buf(bytes + kTail, kFill) {}
    char* p() { return (char*)buf.data(); }
};

// [from, to) of the buffer still holds the fill pattern
void expect_fill(const Stage& st, size_t from, size_t to, const char* what, int g, int i) {
    size_t bad = 0;
    for (size_t k = from; k < to; ++k) bad += st.buf[k] != kFill;
    EXPECT(bad == 0, "%s: %zu bytes behind image %d of group %d were overwritten", what, bad, i, g);
}

void check_plan(const StagePlan& plan, int n, const char* what) {
    EXPECT((int)plan.slot.size() == n + 1 && plan.group_first.front() == 0 && plan.group_first.back() == n, "%s: plan shape", what);
    for (int i = 0; i <= n; ++i) EXPECT(plan.slot[i] % 256 == 0, "%s: slot %d is not 256-byte aligned", what, i);
    for (int g = 0; g < plan.groups(); ++g) {
        EXPECT(plan.group_first[g] < plan.group_first[g + 1], "%s: group %d is empty", what, g);
        EXPECT(plan.slot[plan.group_first[g + 1]] - plan.slot[plan.group_first[g]] <= plan.stage_bytes, "%s: group %d does not fit the stage", what, g);
    }
}

// image i of group g was staged as `px_bytes` per pixel at its slot; what follows up to the next slot (the last image: to the end
// of the buffer and its guard) is untouched
template <class T>
void check_staged(const Images<T>& in, const StagePlan& plan, int g, const Stage& st, int i, bool as_bytes, const char* what) {
    const HostImage& m = in.im[i];
    const size_t at = plan.at(g, i), px_bytes = as_bytes ? 1 : sizeof(T);
    size_t bad = 0;
    for (int y = 0; y < m.h; ++y)
        for (int x = 0; x < m.w; ++x) {
            const T v = in.at(i, x, y);
            const size_t k = at + ((size_t)y * m.w + x) * px_bytes;
            if (as_bytes) {
                bad += st.buf[k] != (unsigned char)(int)v;
            } else {
                bad += std::memcmp(&st.buf[k], &v, sizeof(T)) != 0;
            }
        }
    EXPECT(bad == 0, "%s: %zu pixels of image %d (group %d) differ from the naive copy", what, bad, i, g);
    const bool last = i + 1 == plan.group_first[g + 1];
    expect_fill(st, at + (size_t)m.w * m.h * px_bytes, last ? st.buf.size() : plan.at(g, i + 1), what, g, i);
}

// the byte entry
StagePlan run_bytes(const char* what, const std::vector<Size>& sizes, size_t limit) {
    const Images<unsigned char> in(sizes);
    const StagePlan plan = plan_stage(in.im.data(), in.n(), 1, limit);
    check_plan(plan, in.n(), what);
    for (int g = 0; g < plan.groups(); ++g) {
        Stage st(plan.stage_bytes);
        stage_byte_rows(in.im.data(), plan, g, st.p());
        for (int i = plan.group_first[g]; i < plan.group_first[g + 1]; ++i) check_staged(in, plan, g, st, i, true, what);
    }
    return plan;
}

// the fp32 entry: one group decides while it stages, several groups probe first and stage group by group.  (bad_i, bad_x, bad_y): a
// pixel that is no integer (bad_i < 0: none)
StagePlan run_f32(const char* what, const std::vector<Size>& sizes, size_t limit, bool try_src_u8, int bad_i = -1, int bad_x = 0, int bad_y = 0) {
    Images<float> in(sizes);
    if (bad_i >= 0) in.px[bad_i][(size_t)bad_y * (in.im[bad_i].pitch / 4) + bad_x] = 100.5f;
    const bool want_ref = bad_i != 0, want_src = try_src_u8 && bad_i < 1;
    const StagePlan plan = plan_stage(in.im.data(), in.n(), 4, limit);
    check_plan(plan, in.n(), what);
    bool ref_u8 = false, src_u8 = false;
    if (plan.groups() > 1) exact_sweep<false>(in.im.data(), in.n(), try_src_u8, nullptr, nullptr, ref_u8, src_u8);
    for (int g = 0; g < plan.groups(); ++g) {
        Stage st(plan.stage_bytes);
        if (plan.groups() == 1)
            stage_deciding(in.im.data(), in.n(), plan, try_src_u8, st.p(), ref_u8, src_u8);
        else
            stage_known(in.im.data(), plan, g, st.p(), ref_u8, src_u8);
        EXPECT(ref_u8 == want_ref && src_u8 == want_src, "%s: formats %d %d, expected %d %d", what, ref_u8, src_u8, want_ref, want_src);
        for (int i = plan.group_first[g]; i < plan.group_first[g + 1]; ++i) check_staged(in, plan, g, st, i, i == 0 ? want_ref : want_src, what);
    }
    return plan;
}

// every row of every image is handed out exactly once, in spans that stay inside one image and one chunk
void run_dealer(const char* what, const std::vector<Size>& sizes, int first, int last, long chunk) {
    const Images<unsigned char> in(sizes);
    std::vector<std::vector<std::atomic<int>>> seen;
    for (const HostImage& m : in.im) seen.emplace_back(m.h);
    std::atomic<int> bad_span(0);
    deal_rows(in.im.data(), first, last, chunk, [&](int i, int y, int rows) {
        if (i < first || i >= last || y < 0 || rows < 1 || rows > chunk || y + rows > in.im[i].h) {
            bad_span++;
            return;
        }
        for (int k = y; k < y + rows; ++k) seen[i][k]++;
    });
    EXPECT(bad_span == 0, "%s: %d spans outside their image or longer than a chunk", what, bad_span.load());
    for (int i = 0; i < in.n(); ++i)
        for (int y = 0; y < in.im[i].h; ++y) EXPECT(seen[i][y] == (i >= first && i < last ? 1 : 0), "%s: row %d of image %d dealt %d times", what, y, i, seen[i][y].load());
}
}  // namespace

int main() {
    const size_t one_group = (size_t)512 << 20;
    const std::vector<Size> tiny{{1, 1, 0}, {1, 7, 0}, {7, 1, 0}};
    // 168 rows: no multiple of 32 or 64; the 100-row image takes several chunks
    const std::vector<Size> mixed{{33, 20, 0}, {17, 45, 0}, {64, 3, 0}, {5, 100, 0}};
    // the first chunk (32 or 64 rows) spans three images
    const std::vector<Size> three{{9, 10, 0}, {9, 5, 0}, {9, 40, 0}};
    const std::vector<Size> padded{{33, 20, 3}, {17, 45, 1}, {64, 3, 16}, {5, 100, 7}};
    // five slots of 512 bytes under a limit of 1024: groups {0, 1}, {2, 3}, {4}
    const std::vector<Size> five_u8{{20, 15, 0}, {19, 16, 2}, {30, 10, 0}, {10, 30, 0}, {23, 13, 1}};
    const std::vector<Size> five_f32{{10, 10, 0}, {9, 11, 2}, {12, 8, 0}, {8, 12, 0}, {11, 9, 1}};

    run_dealer("dealer, tiny", tiny, 0, 3, 32);
    run_dealer("dealer, chunk of 7", mixed, 0, 4, 7);
    run_dealer("dealer, images 1..2 only", mixed, 1, 3, 32);
    run_dealer("dealer, three images in a chunk", three, 0, 3, 64);

    run_bytes("bytes, tiny", tiny, one_group);
    run_bytes("bytes, mixed", mixed, one_group);
    run_bytes("bytes, three in a chunk", three, one_group);
    run_bytes("bytes, padded", padded, one_group);
    {
        const StagePlan p = run_bytes("bytes, three groups", five_u8, 1024);
        EXPECT(p.groups() == 3 && p.group_first[2] == 4, "bytes: %d groups, the last from image %d", p.groups(), p.group_first[p.groups() - 1]);
    }

    run_f32("fp32, tiny", tiny, one_group, true);
    run_f32("fp32, mixed", mixed, one_group, true);
    run_f32("fp32, three in a chunk", three, one_group, true);
    run_f32("fp32, padded", padded, one_group, true);
    run_f32("fp32, forced fp32 sources", padded, one_group, false);
    run_f32("fp32, inexact reference", mixed, one_group, true, 0, 32, 19);
    // an inexact pixel in the last row of the last source: found by the last chunk, every source is staged again as fp32
    run_f32("fp32, inexact last row", mixed, one_group, true, 3, 4, 99);
    run_f32("fp32, inexact last row, padded", padded, one_group, true, 3, 4, 99);
    {
        const StagePlan p = run_f32("fp32, three groups", five_f32, 1024, true);
        EXPECT(p.groups() == 3 && p.group_first[2] == 4, "fp32: %d groups, the last from image %d", p.groups(), p.group_first[p.groups() - 1]);
        run_f32("fp32, three groups, inexact last row", five_f32, 1024, true, 4, 10, 8);
        run_f32("fp32, three groups, inexact reference", five_f32, 1024, true, 0, 0, 0);
    }

    std::printf("%s: %d checks, %d failed\n", g_failed ? "FAILED" : "ok", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
