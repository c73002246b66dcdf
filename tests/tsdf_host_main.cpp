// tsdf_host_main.cpp -- two host functions of csrc/pm_tsdf.hpp as they are compiled, for tests/test_tsdf_fuzz_cpu.py: the block test
// tsdf_box_live<4 | 8> on the boxes and views it is given, and the colour byte tsdf_byte.  Built with hipcc (the header holds kernels)
// and run on the host; it calls no HIP function and needs no GPU.
// Input, text on stdin, any number of requests:
//   byte n v_1 .. v_n                                      -> one line with the n bytes
//   live ox oy oz voxel nx ny nz corners n_views n_boxes   (corners: 4 or 8)
//        then per view R[9] t[3] K0 K2 K4 K5 w h cull, then per box i0 i1 j0 j1 k0 k1
//                                                          -> one line per view with a 0 (dead) or 1 (live) per box
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pm_tsdf.hpp"

using namespace pm;

static bool word(char* buf) { return scanf("%63s", buf) == 1; }
static double num() {
    char buf[64];
    if (!word(buf)) { fprintf(stderr, "input ends inside a request\n"); exit(3); }
    return strtod(buf, nullptr);   // decimal text of a float's value, nan and inf included: exact
}

int main() {
    char mode[64];
    while (word(mode)) {
        if (!strcmp(mode, "byte")) {
            const int n = (int)num();
            for (int q = 0; q < n; ++q) printf("%d ", (int)tsdf_byte((float)num()));
            printf("\n");
        } else if (!strcmp(mode, "live")) {
            TsdfVol V{};
            for (int a = 0; a < 3; ++a) V.o[a] = (double)(float)num();
            V.voxel = (double)(float)num();
            V.nx = (int)num(); V.ny = (int)num(); V.nz = (int)num();
            const int corners = (int)num(), n_views = (int)num(), n_boxes = (int)num();
            std::vector<TsdfView> views((size_t)n_views);
            for (TsdfView& W : views) {
                memset(&W, 0, sizeof W);
                for (float& x : W.R) x = (float)num();
                for (float& x : W.t) x = (float)num();
                W.K0 = (float)num(); W.K2 = (float)num(); W.K4 = (float)num(); W.K5 = (float)num();
                W.w = (int)num(); W.h = (int)num(); W.cull = (int)num();
            }
            std::vector<int> boxes((size_t)n_boxes * 6);
            for (int& x : boxes) x = (int)num();
            for (const TsdfView& W : views) {
                for (int b = 0; b < n_boxes; ++b) {
                    const int* x = &boxes[(size_t)b * 6];
                    const bool live = corners == 4 ? tsdf_box_live<4>(V, W, x[0], x[1], x[2], x[3], x[4], x[5]) : tsdf_box_live<8>(V, W, x[0], x[1], x[2], x[3], x[4], x[5]);
                    putchar(live ? '1' : '0');
                }
                putchar('\n');
            }
        } else {
            fprintf(stderr, "unknown request %s\n", mode);
            return 2;
        }
    }
    return 0;
}
