// candidate_tile_check.cpp -- the candidate-cost tile of the update kernel (csrc/pm_cand_tile.hpp) replayed on the host through the
// header's own index functions: for every block of an image the tile is filled item by item as update_body fills it (items dealt
// to NT threads, positions outside the image replaced), every pixel of the block of the pass's colour looks its 88 neighbours up
// in it, and `pos` and `flags` are compared with the direct statement of the search (bounds tests on the image, ref .cu:798-816).
// Sizes 17x9, 47x24, 62x54, 96x87, 1x1 and 40x3, both block shapes (16x8 one wave, 16x32 four waves) and both colours, with
// random costs that include equal values, +0.0, 2.0, the search's start value, infinity and NaN.
// The tile is an array of exactly CandTile::floats, so AddressSanitizer sees any index outside it; a cell that no fill item wrote
// is marked, and a lookup that touches one is an error.  It tests the indexing only.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Imp-mvs_amd/csrc -o build/candidate_tile_check \
//       tools/candidate_tile_check.cpp && build/candidate_tile_check
// Prints one line per case and "all equal"; exit status 1 if anything differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "pm_cand_tile.hpp"
using namespace pm;

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

template <int BW, int BH, int NT>
static long check(int W, int H, int parity, const std::vector<float>& costs, long& lookups) {
    typedef CandTile<BW, BH> CT;
    long bad = 0;
    const int nbx = (W + BW - 1) / BW, nby = (H + BH - 1) / BH;
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            const int x0 = bx * BW, y0 = by * BH;
            std::vector<float> tile(CT::floats);
            std::vector<char> written(CT::floats, 0);
            // the fill, as the kernel deals it: thread t of NT takes the items t, t + NT, ...
            constexpr int rounds = (CT::items + NT - 1) / NT;
            for (int t = 0; t < NT; ++t)
                for (int k = 0; k < rounds; ++k) {
                    const int i = t + k * NT;
                    if (i >= CT::items) continue;
                    int r, c, nx, ny;
                    cand_tile_cell<BW, BH>(i, r, c);
                    cand_tile_position<BW, BH>(r, c, x0, y0, parity, nx, ny);
                    const int cx = nx < 0 ? 0 : (nx > W - 1 ? W - 1 : nx), cy = ny < 0 ? 0 : (ny > H - 1 ? H - 1 : ny);
                    const float v = costs[(size_t)cy * W + cx];
                    const size_t at = (size_t)r * CT::pitch + c;
                    if (r < 0 || r >= CT::rows || c < 0 || c >= CT::cols || written[at]) { printf("fill item %d: cell (%d, %d) twice or outside\n", i, r, c); ++bad; continue; }
                    tile.at(at) = (cx == nx && cy == ny) ? v : kCandNone;
                    written[at] = 1;
                }
            // every thread of the block searches, with or without a pixel in the image (the kernel does the same)
            for (int ly = 0; ly < BH; ++ly)
                for (int l = 0; l < BW / 2; ++l) {
                    const int y = y0 + ly, x = x0 + 2 * l + ((y + parity) & 1);
                    int te, to;
                    cand_tile_bases<BW, BH>(x, y, x0, y0, te, to);
                    for (int k = 0; k < 8; ++k) {
                        float best = kCandNone, dbest = kCandNone;
                        int bpos = 0, dpos = 0;
                        for (int d = 0; d < kNumDirs[k]; ++d) {
                            const int dx = kDirs[k][d].x, dy = kDirs[k][d].y, nx = x + dx, ny = y + dy;
                            const int at = cand_tile_index<BW, BH>(te, to, dx, dy);
                            ++lookups;
                            if (at < 0 || at >= CT::floats || !written[at]) { printf("%dx%d block (%d, %d) pixel (%d, %d) offset (%d, %d): cell %d not filled\n", W, H, bx, by, x, y, dx, dy, at); ++bad; continue; }
                            const float v = tile.at(at);
                            if (best > v) { best = v; bpos = ny * W + nx; }
                            // the direct statement
                            const bool inside = nx >= 0 && ny >= 0 && nx < W && ny < H;
                            if (inside && !same_bits(v, costs[(size_t)ny * W + nx])) { printf("pixel (%d, %d) offset (%d, %d): wrong cost\n", x, y, dx, dy); ++bad; }
                            if (inside && dbest > costs[(size_t)ny * W + nx]) { dbest = costs[(size_t)ny * W + nx]; dpos = ny * W + nx; }
                        }
                        if (bpos != dpos || (best < kCandNone) != (dbest < kCandNone)) { printf("pixel (%d, %d) region %d: pos %d flag %d, direct %d %d\n", x, y, k, bpos, best < kCandNone, dpos, dbest < kCandNone); ++bad; }
                        if (bpos < 0 || bpos >= W * H) { printf("pixel (%d, %d) region %d: pos %d outside the image\n", x, y, k, bpos); ++bad; }
                    }
                }
        }
    return bad;
}

int main() {
    static_assert(CandTile<16, 8>::floats <= 2 * 36 * 64 && CandTile<16, 32>::floats <= 2 * 36 * 256, "the tile fits the weight records' area");
    const int sizes[][2] = {{17, 9}, {47, 24}, {62, 54}, {96, 87}, {1, 1}, {40, 3}};
    const float special[] = {2.0f, 0.0f, 3.402823466e+38f, INFINITY, NAN, 0.5f, 0.5f, 0.5f};
    std::mt19937 rng(12345);
    long bad = 0;
    for (auto& s : sizes)
        for (int mode = 0; mode < 3; ++mode) {   // 0: random costs, 1: all equal, 2: random with special values
            const int W = s[0], H = s[1];
            std::vector<float> costs((size_t)W * H);
            for (auto& c : costs) c = mode == 1 ? 0.25f : (mode == 2 && rng() % 4 == 0) ? special[rng() % 8] : (float)(rng() % 2000) * 0.001f;
            for (int parity = 0; parity < 2; ++parity) {
                long lookups = 0;
                const long b1 = check<16, 8, 64>(W, H, parity, costs, lookups), b4 = check<16, 32, 256>(W, H, parity, costs, lookups);
                printf("%3dx%-3d costs %d colour %d: %ld lookups, %ld differences\n", W, H, mode, parity, lookups, b1 + b4);
                bad += b1 + b4;
            }
        }
    printf(bad ? "DIFFERENCES: %ld\n" : "all equal\n", bad);
    return bad ? 1 : 0;
}
