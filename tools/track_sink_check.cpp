// track_sink_check.cpp -- the growing host arrays of the fusion's tracks (csrc/pm_tracks_host.hpp, TrackSink) driven the way
// FuseRun::ship_tracks of mpmvs_fusion.hip drives them -- per image reserve(points, entries), a copy of exactly that many offsets and entries to
// the tails, commit, and finish at the end -- against plain vectors: images with no points, with one point, with many, entry
// counts that force every array to be moved several times, an empty result, a sink dropped without finish(), and a commit that
// does not continue the arrays.  A host program, so that it runs under the sanitizers without a GPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Imp-mvs_amd/csrc
//       -o build/track_sink_check tools/track_sink_check.cpp && build/track_sink_check          (one command line)
// Prints one line per case and "all equal"; exit status 1 if any result differs.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pm_tracks_host.hpp"
using namespace pm;

// one run: images[k] = track lengths of the points of image k.  The "device" side is a staging buffer of one image's size.
static bool run_case(const char* name, const std::vector<std::vector<int>>& images, bool finish) {
    std::vector<long long> want_off(1, 0);
    std::vector<int32_t> want_image, want_pixel;
    TrackSink sink;
    bool ok = true;
    long long base = 0;
    for (size_t k = 0; k < images.size() && ok; ++k) {
        std::vector<long long> st_off;
        std::vector<int32_t> st_image, st_pixel;
        for (size_t p = 0; p < images[k].size(); ++p) {
            st_off.push_back(base + (long long)st_image.size());
            for (int e = 0; e < images[k][p]; ++e) {
                st_image.push_back((int32_t)(e ? (k + e) % 7 : k));
                st_pixel.push_back((int32_t)(p * 31 + e));
            }
        }
        const size_t np = st_off.size(), ne = st_image.size();
        ok = sink.reserve(np, ne);
        if (ok && np) {
            std::memcpy(sink.off_tail(), st_off.data(), np * sizeof(long long));
            std::memcpy(sink.image_tail(), st_image.data(), ne * sizeof(int32_t));
            std::memcpy(sink.pixel_tail(), st_pixel.data(), ne * sizeof(int32_t));
        }
        ok = ok && sink.commit(np, ne);
        base += (long long)ne;
        want_off.pop_back();
        want_off.insert(want_off.end(), st_off.begin(), st_off.end());
        want_off.push_back(base);
        want_image.insert(want_image.end(), st_image.begin(), st_image.end());
        want_pixel.insert(want_pixel.end(), st_pixel.begin(), st_pixel.end());
    }
    ok = ok && sink.points() == want_off.size() - 1 && sink.entries() == want_image.size();
    if (ok && finish) {
        long long* off = nullptr;
        int32_t *image = nullptr, *pixel = nullptr;
        ok = sink.finish(&off, &image, &pixel) && off && image && pixel;
        ok = ok && std::memcmp(off, want_off.data(), want_off.size() * sizeof(long long)) == 0;
        ok = ok && (want_image.empty() || (std::memcmp(image, want_image.data(), want_image.size() * 4) == 0 &&
                                           std::memcmp(pixel, want_pixel.data(), want_pixel.size() * 4) == 0));
        ok = ok && sink.points() == 0 && sink.entries() == 0;   // handed over: the sink is empty again
        std::free(off);
        std::free(image);
        std::free(pixel);
    }
    std::printf("%-44s %8zu points %9zu entries  %s\n", name, want_off.size() - 1, want_image.size(), ok ? "equal" : "DIFFERENT");
    return ok;
}

int main() {
    std::mt19937 rng(7);
    bool ok = true;
    ok &= run_case("no image", {}, true);
    ok &= run_case("images without points", {{}, {}, {}}, true);
    ok &= run_case("one point", {{2}}, true);
    ok &= run_case("empty images between full ones", {{}, {2, 3, 6}, {}, {}, {4}, {}}, true);
    {
        // sizes that grow and shrink: every array is moved several times, and sometimes not at all
        std::vector<std::vector<int>> images;
        for (int k = 0; k < 40; ++k) {
            const int np = (k % 5 == 3) ? 0 : (int)(rng() % (k < 20 ? 50 : 20000));
            std::vector<int> len(np);
            for (int& l : len) l = 2 + (int)(rng() % 32);   // a track has 2 .. 33 entries
            images.push_back(len);
        }
        ok &= run_case("40 images, up to 20 000 points each", images, true);
        ok &= run_case("the same, dropped without finish()", images, false);
    }
    {
        // what was copied in must continue the arrays: a first offset that is not the number of entries so far is refused
        TrackSink sink;
        bool refused = sink.reserve(2, 5);
        if (refused) {
            sink.off_tail()[0] = 0, sink.off_tail()[1] = 2;
            refused = sink.commit(2, 5) && sink.reserve(1, 2);
        }
        if (refused) {
            sink.off_tail()[0] = 4;   // 5 entries so far
            refused = !sink.commit(1, 2) && sink.points() == 2 && sink.entries() == 5;
        }
        // ... and so is a commit of more than was reserved
        refused = refused && !sink.commit(1000000, 0) && !sink.commit(0, 1000000);
        std::printf("%-44s %s\n", "commits that do not fit are refused", refused ? "equal" : "DIFFERENT");
        ok &= refused;
    }
    std::printf(ok ? "all equal\n" : "FAILED\n");
    return ok ? 0 : 1;
}
