// fuse_lists_check.cpp -- the rules a depth-map fusion call's arguments must keep before anything touches the device
// (csrc/pm_fusion_host.hpp, fuse_check_request; FuseRun::run of mpmvs_fusion.hip calls it first) against a table of requests and
// the codes they must end with: every rule broken alone, the accepted ends of each range, the track bound with and without
// tracks, and requests with two faults that pin the precedence -1 before -2 before -3.  A host program, so that it runs under
// the sanitizers without a GPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Imp-mvs_amd/csrc
//       -o build/fuse_lists_check tools/fuse_lists_check.cpp && build/fuse_lists_check          (one command line)
// Prints one line per case and "all equal"; exit status 1 if any code differs.
#include <cstdio>
#include <vector>

#include "pm_fusion_host.hpp"
using namespace pm;

constexpr int kSlots = 33;   // pm_fusion.hpp: kMaxFuseNgb = kMaxViews + 1

// one request of n images of w x h; lists[i] is image i's complete list.  The vectors are exactly as long as the request says, so
// that a read past a list is a sanitizer error
struct Case {
    const char* name;
    int want;
    int n, channels;
    std::vector<int> estimate;
    std::vector<std::vector<int>> lists;
    bool tracks = false, entered = true;
    int w = 33, h = 9;
    bool no_off = false, no_ids = false;
    std::vector<int> off_override;   // the offsets to hand over instead of those of `lists`
};

static bool run_case(const Case& c) {
    std::vector<int> off(1, 0), ids;
    for (const std::vector<int>& l : c.lists) {
        ids.insert(ids.end(), l.begin(), l.end());
        off.push_back((int)ids.size());
    }
    if (!c.off_override.empty()) off = c.off_override;
    ids.reserve(1);   // no id at all is still an array (NULL is a case of its own)
    std::vector<mpmvs_camera> cams((size_t)(c.n > 0 ? c.n : 0));
    for (mpmvs_camera& cam : cams) cam = mpmvs_camera{}, cam.width = c.w, cam.height = c.h;
    TrackSink sink;
    FuseRequest q{0, c.n, cams.data(), c.estimate.data(), nullptr, nullptr, nullptr, nullptr, c.channels, nullptr, c.no_off ? nullptr : off.data(),
                  c.no_ids ? nullptr : ids.data(), 0};
    q.tracks = c.tracks ? &sink : nullptr;
    const int got = fuse_check_request(q, c.entered, kSlots);
    std::printf("%-58s want %2d got %2d  %s\n", c.name, c.want, got, got == c.want ? "equal" : "DIFFERENT");
    return got == c.want;
}

static std::vector<int> iota_list(int first, int count) {
    std::vector<int> l;
    for (int k = 0; k < count; ++k) l.push_back(first + k);
    return l;
}

int main() {
    const std::vector<std::vector<int>> good = {{0, 1, 2}, {1, 0, 2}, {2, 1}};
    std::vector<Case> cases = {
        {"three images, well formed", 0, 3, 3, {1, 1, 1}, good},
        {"the same, grey, with tracks", 0, 3, 1, {1, 1, 1}, good, true},
        // -1
        {"n = 0", -1, 0, 3, {}, {}},
        {"n = -1", -1, -1, 3, {}, {}},
        {"channels 2", -1, 3, 2, {1, 1, 1}, good},
        {"the device cannot be selected", -1, 3, 3, {1, 1, 1}, good, false, false},
        // -2
        {"src_off NULL", -2, 3, 3, {1, 1, 1}, good, false, true, 33, 9, true},
        {"src_ids NULL", -2, 3, 3, {1, 1, 1}, good, false, true, 33, 9, false, true},
        {"src_off[0] = 1", -2, 3, 3, {1, 1, 1}, {{9, 0, 1, 2}, {1, 0, 2}, {2, 1}}, false, true, 33, 9, false, false, {1, 4, 7, 9}},
        {"descending offsets", -2, 3, 3, {1, 1, 1}, good, false, true, 33, 9, false, false, {0, 3, 2, 8}},
        {"a list that does not start with its own image", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {0, 2}, {2, 1}}},
        {"the same on an image that is not estimated", -2, 3, 3, {1, 0, 1}, {{0, 1, 2}, {0, 2}, {2, 1}}},
        {"an estimated image with an empty list", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {}, {2, 1}}},
        {"id -1", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {1, -1}, {2, 1}}},
        {"id n", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {1, 3}, {2, 1}}},
        {"an id twice", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {1, 0, 2, 0}, {2, 1}}},
        {"an id twice on an image that is not estimated", -2, 3, 3, {1, 1, 0}, {{0, 1, 2}, {1, 0}, {2, 1, 1}}},
        {"the image itself among its sources", -2, 3, 3, {1, 1, 1}, {{0, 1, 2}, {1, 0, 1}, {2, 1}}},
        // the accepted ends
        {"an unestimated image with an empty list", 0, 3, 3, {1, 0, 1}, {{0, 1, 2}, {}, {2, 1}}},
        {"nothing estimated, no list at all", 0, 3, 3, {0, 0, 0}, {{}, {}, {}}},
        {"one image, its own list only", 0, 1, 1, {1}, {{0}}},
        // two faults: the earlier code wins
        {"channels 2 and src_off NULL: -1 before -2", -1, 3, 2, {1, 1, 1}, good, false, true, 33, 9, true},
        {"n = 0 and src_off NULL: -1 before -2", -1, 0, 3, {}, {}, false, true, 33, 9, true},
        {"no device and an id twice: -1 before -2", -1, 3, 3, {1, 1, 1}, {{0, 1, 1}, {1, 0}, {2, 1}}, false, false},
    };
    {
        // kSlots slots exactly are accepted, kSlots + 1 are not -- and an unestimated image may have them
        const int n = kSlots + 1;
        Case c{"kMaxFuseNgb slots exactly", 0, n, 3, std::vector<int>((size_t)n, 0), std::vector<std::vector<int>>((size_t)n)};
        c.estimate[0] = 1;
        c.lists[0] = iota_list(0, kSlots);
        cases.push_back(c);
        c.name = "kMaxFuseNgb + 1 slots", c.want = -2;
        c.lists[0] = iota_list(0, kSlots + 1);
        cases.push_back(c);
        c.name = "kMaxFuseNgb + 1 slots on an image that is not estimated", c.want = 0;
        c.estimate[0] = 0, c.estimate[1] = 1, c.lists[1] = {1, 0};
        cases.push_back(c);
    }
    {
        // the track bound: 46341^2 pixels x 1 slot is the first square past 2^31 - 1 -- refused only when tracks are asked for, only
        // on an estimated image, and after every -2 rule
        Case c{"46341 x 46341 x 1 slot, no tracks", 0, 2, 3, {1, 1}, {{0}, {1, 0}}, false, true, 46341, 46341};
        cases.push_back(c);
        c.name = "the same with tracks", c.want = -3, c.tracks = true;
        cases.push_back(c);
        c.name = "46340 x 46340 x 1 slot with tracks", c.want = 0, c.w = c.h = 46340;
        c.lists = {{0}, {1}};
        cases.push_back(c);
        c.name = "46340 x 46340 x 2 slots with tracks", c.want = -3;
        c.lists = {{0}, {1, 0}};
        cases.push_back(c);
        c.name = "the same, that image not estimated", c.want = 0, c.estimate = {1, 0};
        cases.push_back(c);
        c.name = "past the track bound and an id twice: -2 before -3", c.want = -2, c.estimate = {1, 1};
        c.lists = {{0, 1, 1}, {1, 0}};
        cases.push_back(c);
        c.name = "past the track bound and channels 2: -1 before -3", c.want = -1, c.channels = 2;
        c.lists = {{0}, {1, 0}};
        cases.push_back(c);
    }
    bool ok = true;
    for (const Case& c : cases) ok &= run_case(c);
    std::printf(ok ? "all equal\n" : "FAILED\n");
    return ok ? 0 : 1;
}
