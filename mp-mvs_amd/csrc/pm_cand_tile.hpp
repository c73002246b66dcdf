// pm_cand_tile.hpp -- the candidate-cost tile of the update kernel: its geometry and its index arithmetic, nothing else.
//
// The checkerboard propagation looks up the stored costs of 88 neighbours per pixel (kDirs below: eight regions, ref .cu:769-779).
// The pixels of a block ask for nearly the same neighbours, so the block stages them once in LDS (update_body, pm_kernels.hpp)
// and every pixel searches the tile instead of the image.
//
// What a block at (x0, y0) of BW x BH pixels can ask for: kDirs reaches 23 pixels, so the positions lie in
// [x0 - 23, x0 + BW + 22] x [y0 - 23, y0 + BH + 22], and every offset has odd |dx| + |dy|, so only positions of the OTHER
// checkerboard colour are ever read.  The tile keeps exactly that colour: row r holds image row y0 - 23 + r, and column c of
// that row holds image column x0 - 24 + 2 c + q, where q is 0 or 1 so that the position has the other colour.  The wedges
// reach 11 rows above and below a pixel and only the vertical strip (dx = 0) reaches further, so rows further than 11 from the
// block are filled only under the block's own BW columns; cells that no pixel of the block can ask for are never written and
// never read.  A position outside the image holds kCandNone, the value the search starts from: its strict comparison can then
// never choose it, which is what the bounds test of the direct statement does.
//
// Pitch 40 floats: the 8 lanes of a row of a wave read consecutive columns and the 4 rows of a 32-lane half lie 8 banks apart
// (ds_read_b32 has 32 banks per half wave), so the entries with even dx read without a bank conflict; with odd dx the rows of
// the two row parities are shifted by one column against each other and two lanes of a half share a bank.
//
// Host and device compile the same functions: tools/candidate_tile_check.cpp replays the fill and the lookups on the CPU.
#pragma once

#if defined(__HIPCC__)
#define PM_CT_FN __host__ __device__ __forceinline__
#define PM_CT_TABLE __device__ constexpr
#else
#define PM_CT_FN inline
#define PM_CT_TABLE constexpr
#endif

namespace pm {

// sampling regions of the checkerboard propagation, ref .cu:769-779
struct Off {
    signed char x, y;
};
PM_CT_TABLE Off kDirs[8][12] = {
    {{-5, -6}, {5, -6}, {-6, -7}, {6, -7}, {-7, -8}, {7, -8}, {-8, -9}, {8, -9}, {-9, -10}, {9, -10}, {-10, -11}, {10, -11}},
    {{-5, 6}, {5, 6}, {-6, 7}, {6, 7}, {-7, 8}, {7, 8}, {-8, 9}, {8, 9}, {-9, 10}, {9, 10}, {-10, 11}, {10, 11}},
    {{-6, -5}, {-6, 5}, {-7, -6}, {-7, 6}, {-8, -7}, {-8, 7}, {-9, -8}, {-9, 8}, {-10, -9}, {-10, 9}, {-11, -10}, {-11, 10}},
    {{6, -5}, {6, 5}, {7, -6}, {7, 6}, {8, -7}, {8, 7}, {9, -8}, {9, 8}, {10, -9}, {10, 9}, {11, -10}, {11, 10}},
    {{0, -5}, {0, -7}, {0, -9}, {0, -11}, {0, -13}, {0, -15}, {0, -17}, {0, -19}, {0, -21}, {0, -23}, {0, 0}, {0, 0}},
    {{0, 5}, {0, 7}, {0, 9}, {0, 11}, {0, 13}, {0, 15}, {0, 17}, {0, 19}, {0, 21}, {0, 23}, {0, 0}, {0, 0}},
    {{-5, 0}, {-7, 0}, {-9, 0}, {-11, 0}, {-13, 0}, {-15, 0}, {-17, 0}, {-19, 0}, {-21, 0}, {-23, 0}, {0, 0}, {0, 0}},
    {{5, 0}, {7, 0}, {9, 0}, {11, 0}, {13, 0}, {15, 0}, {17, 0}, {19, 0}, {21, 0}, {23, 0}, {0, 0}, {0, 0}}};
PM_CT_TABLE int kNumDirs[8] = {12, 12, 12, 12, 10, 10, 10, 10};

constexpr float kCandNone = 3.402823466e+38f;   // "no candidate yet" of the search (ref .cu:798-816), and the tile's value outside the image

template <int BW, int BH>
struct CandTile {
    static_assert(BW % 2 == 0, "the block's first column is even: the colour of a tile cell follows from its row alone");
    static constexpr int reach = 23;               // the longest offset of kDirs (the cross)
    static constexpr int wedge = 11;               // the longest offset of the regions that also move sideways
    static constexpr int cols = (BW + 2 * (reach + 1)) / 2;   // image columns x0 - 24 .. x0 + BW + 23, one colour
    static constexpr int pitch = 40;
    static constexpr int rows = BH + 2 * reach;
    static constexpr int floats = rows * pitch;
    // the fill: the full-width band of the rows within `wedge` of the block, then the block's own columns of the rows beyond
    static constexpr int band_row0 = reach - wedge, band_rows = BH + 2 * wedge, band_items = band_rows * cols;
    static constexpr int strip_col0 = (reach + 1) / 2, strip_cols = BW / 2, strip_items = 2 * band_row0 * strip_cols;
    static constexpr int items = band_items + strip_items;
    static_assert(cols <= pitch && pitch % 32 == 8, "rows of a half wave 8 banks apart");
};

// item i of the fill (0 <= i < items) -> the tile cell (r, c) it writes
template <int BW, int BH>
PM_CT_FN void cand_tile_cell(int i, int& r, int& c) {
    typedef CandTile<BW, BH> T;
    if (i < T::band_items) {
        r = T::band_row0 + i / T::cols;
        c = i % T::cols;
    } else {
        const int j = i - T::band_items, rr = j / T::strip_cols;
        r = rr < T::band_row0 ? rr : rr + T::band_rows;
        c = T::strip_col0 + j % T::strip_cols;
    }
}
// the image position that cell (r, c) holds in a pass of colour `parity`
template <int BW, int BH>
PM_CT_FN void cand_tile_position(int r, int c, int x0, int y0, int parity, int& nx, int& ny) {
    typedef CandTile<BW, BH> T;
    ny = y0 - T::reach + r;
    nx = x0 - (T::reach + 1) + 2 * c + ((ny + parity + 1) & 1);
}
// The lookups of pixel (x, y) of the block: two bases, one for the offsets with even dx and one for those with odd dx, and a
// constant per offset on top (the immediate of the ds_read).
template <int BW, int BH>
PM_CT_FN void cand_tile_bases(int x, int y, int x0, int y0, int& even, int& odd) {
    typedef CandTile<BW, BH> T;
    even = (y - y0) * T::pitch + ((x - x0) >> 1);
    odd = (y - y0) * T::pitch + ((x - x0 + 1) >> 1);
}
template <int BW, int BH>
PM_CT_FN int cand_tile_index(int even, int odd, int dx, int dy) {
    typedef CandTile<BW, BH> T;
    return ((dx & 1) ? odd + (dx + T::reach) / 2 : even + (dx + T::reach + 1) / 2) + (dy + T::reach) * T::pitch;
}

}  // namespace pm
