// pm_tsdf_sparse.hpp -- the brick-sparse TSDF volume: only bricks of 8 x 8 x 8 voxels near the surface exist (mpmvs_tsdf_create_sparse,
// mpmvs_tsdf_allocate; contract: include/mpmvs.h, statements A and B).  Everything here is the dense statement
// of pm_tsdf.hpp under a mask, in BRICK-MAJOR ORDER: bricks ascend by their linear index in the brick grid, voxels within a brick by
// their local index (lk*8 + lj)*8 + li.  The pool keeps the bricks in that order (a brick's pool position is its rank), so entry
// e = rank*512 + local of sum / weight / colour is also the index of the mesh passes' masks and counts, those arrays are linear, and
// the scan kernels of pm_tsdf.hpp apply as they are.
//
// Allocate: k_tsdf_alloc_mark   one thread per pixel walks the n_s + 1 samples of its ray (statement A) and ORs a flag per brick of
//                               each sample's box into a dense array over the brick grid; the set of flags is order-free
//           k_tsdf_brick_scan   "allocated or flagged" per grid cell, scanned per tile with the block scan of pm_scan.hpp; the totals
//                               by k_scan_totals<Sum>; the host refuses on the new count before anything is written
//           k_tsdf_brick_move   an old brick's 512 entries to its new rank (only when bricks existed before)
//           k_tsdf_brick_commit grid[g] = rank, list[rank] = g
// Integrate (k_tsdf_sparse_integrate): one block per brick, one thread per voxel; per view the block asks tsdf_box_live of
//   pm_tsdf.hpp with the 8 corners of the brick's box; the per-voxel body is tsdf_integrate_at of pm_tsdf.hpp.
// Mesh: the four passes of pm_tsdf.hpp with one block per brick.  A cell's corners lie in up to 8 bricks (the brick itself and its
//   neighbours towards +x, +y, +z); their ranks are resolved once per block from the grid (tsdf_brick_resolve) and every corner is
//   addressed through that table (tsdf_brick_at).  A corner in a brick that does not exist has weight 0: it is never valid.  Mark and
//   triangles read the corners' validity and values from a 9 x 9 x 9 tile that the block stages in LDS (tsdf_tile_load_one).
// Shared with the dense volume: tsdf_box_live, tsdf_integrate_at and the mesh bodies tsdf_mark_cell / tsdf_vertex_cell /
//   tsdf_triangle_cell; the sparse side supplies the corner addressing (TsdfBrickAt) and the cell's bits from the tile (tsdf_tile_cell).
// The per-thread bodies are host and device code: tools/mesh_sparse_check.cpp replays them thread by thread under the sanitizers.
#pragma once

#include "pm_tsdf.hpp"

namespace pm {

constexpr int kBrick = 8, kBrickVox = 512;

struct TsdfBricks {
    int bx, by, bz;         // bricks per axis: ceil(dims / 8)
    const int32_t* grid;    // [bx*by*bz]: the rank of the brick, -1 if it does not exist
    const int32_t* list;    // [n_bricks]: the linear index of the brick of each rank
};

// statement A's constants
struct TsdfAlloc {
    int n_s;
    double step;            // (2.0 * (double)trunc) / (double)n_s
    float origin[3], voxel, pad;
};

__host__ __device__ inline void tsdf_brick_coords(const TsdfBricks& B, int g, int& I, int& J, int& K) {
    I = g % B.bx;
    const int r = g / B.bx;
    J = r % B.by;
    K = r / B.by;
}

// an integer-valued float (the result of floorf) as an int for comparisons with 0 and n - 1 < 2^30: exact in between, -1 below 0
// and 2^30 from 2^30 on, so that every comparison and clamp of step 5 has the outcome it has on the real values
__host__ __device__ inline int tsdf_floor_int(float f) { return f < 0.0f ? -1 : f >= 0x1p30f ? (1 << 30) : (int)f; }

// ---- A. allocate ---------------------------------------------------------------------------------------------------------------
// pixel (ix, iy) of view W: flags[g] |= 1 for every brick g of the boxes of its samples.  A sample whose box of bricks equals the
// previous sample's is skipped (most consecutive samples of a ray); a flag that already reads 1 is not ORed again.
__host__ __device__ inline void tsdf_alloc_mark_one(const TsdfVol& V, const TsdfBricks& B, const TsdfAlloc& S, const TsdfView& W, int ix, int iy, uint32_t* flags) {
    const float d = W.depth[(size_t)iy * (size_t)W.w + (size_t)ix];
    if (!(tsdf_finite(d) && d > 0.0f)) return;
    const float fx = (float)ix - W.K2, fy = (float)iy - W.K5;
    const int n[3] = {V.nx, V.ny, V.nz};
    int plo[3] = {-1, -1, -1}, phi[3] = {-1, -1, -1};
    for (int m = 0; m <= S.n_s; ++m) {
        const float z = (float)(((double)d - (double)V.trunc) + (double)m * S.step);
        if (!(z > 0.0f)) continue;
        const float xc = (fx * z) / W.K0, yc = (fy * z) / W.K4;
        const float a = xc - W.t[0], b = yc - W.t[1], c = z - W.t[2];
        const float P[3] = {(W.R[0] * a + W.R[3] * b) + W.R[6] * c, (W.R[1] * a + W.R[4] * b) + W.R[7] * c, (W.R[2] * a + W.R[5] * b) + W.R[8] * c};
        int lo[3], hi[3];
        bool skip = false;
        for (int q = 0; q < 3; ++q) {
            const float g = (P[q] - S.origin[q]) / S.voxel;
            if (!tsdf_finite(g)) { skip = true; break; }
            lo[q] = tsdf_floor_int(floorf(g - S.pad));
            hi[q] = tsdf_floor_int(floorf(g + S.pad));
            if (hi[q] < 0 || lo[q] > n[q] - 1) { skip = true; break; }
            lo[q] = (lo[q] < 0 ? 0 : lo[q]) >> 3;
            hi[q] = (hi[q] > n[q] - 1 ? n[q] - 1 : hi[q]) >> 3;
        }
        if (skip) continue;
        if (lo[0] == plo[0] && lo[1] == plo[1] && lo[2] == plo[2] && hi[0] == phi[0] && hi[1] == phi[1] && hi[2] == phi[2]) continue;
        for (int q = 0; q < 3; ++q) { plo[q] = lo[q]; phi[q] = hi[q]; }
        for (int K = lo[2]; K <= hi[2]; ++K)
            for (int J = lo[1]; J <= hi[1]; ++J)
                for (int I = lo[0]; I <= hi[0]; ++I) {
                    const size_t g = ((size_t)K * (size_t)B.by + (size_t)J) * (size_t)B.bx + (size_t)I;
                    if (!flags[g]) tsdf_or(&flags[g], 1u);
                }
    }
}

// blockIdx.y: the view of the chunk; blockIdx.x * 256 + threadIdx.x: its pixel
__global__ __launch_bounds__(256) void k_tsdf_alloc_mark(TsdfVol V, TsdfBricks B, TsdfAlloc S, TsdfChunkArgs A, uint32_t* flags) {
    const TsdfView& W = A.v[blockIdx.y];
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (size_t)W.w * (size_t)W.h) return;
    tsdf_alloc_mark_one(V, B, S, W, (int)(pix % (size_t)W.w), (int)(pix / (size_t)W.w), flags);
}

// per tile of kScanBlock grid cells: excl[g] = the bricks (old or flagged) before g in its tile, totals[tile] = the tile's bricks
__global__ __launch_bounds__(kScanBlock) void k_tsdf_brick_scan(const int32_t* __restrict__ grid, const uint32_t* __restrict__ flags, int n_grid, int* __restrict__ excl,
                                                                int* __restrict__ totals) {
    const int g = (int)(blockIdx.x * kScanBlock + threadIdx.x);
    int total;
    const int r = block_excl_scan<Sum>(g < n_grid && (grid[g] >= 0 || flags[g]) ? 1 : 0, 0, total);
    if (g < n_grid) excl[g] = r;
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// the new rank of grid cell g after the scan (tile totals scanned in place), -1 if it holds no brick
__host__ __device__ inline int tsdf_brick_rank(int g, const int32_t* __restrict__ grid, const uint32_t* __restrict__ flags, const int* __restrict__ excl,
                                               const int* __restrict__ totals) {
    return (grid[g] >= 0 || flags[g]) ? excl[g] + totals[g / kScanBlock] : -1;
}

// entry `local` of old brick `r` to its new place; the new arrays are zero before
__host__ __device__ inline void tsdf_brick_move_one(int r, int local, const int32_t* __restrict__ list_old, const int32_t* __restrict__ grid, const uint32_t* __restrict__ flags,
                                                    const int* __restrict__ excl, const int* __restrict__ totals, const float* __restrict__ sum_old,
                                                    const int32_t* __restrict__ weight_old, const uint4* __restrict__ color_old, float* __restrict__ sum,
                                                    int32_t* __restrict__ weight, uint4* __restrict__ color) {
    const size_t from = (size_t)r * kBrickVox + (size_t)local;
    const size_t to = (size_t)tsdf_brick_rank(list_old[r], grid, flags, excl, totals) * kBrickVox + (size_t)local;
    sum[to] = sum_old[from];
    weight[to] = weight_old[from];
    if (color) color[to] = color_old[from];
}
__global__ __launch_bounds__(kBrickVox) void k_tsdf_brick_move(const int32_t* __restrict__ list_old, const int32_t* __restrict__ grid, const uint32_t* __restrict__ flags,
                                                               const int* __restrict__ excl, const int* __restrict__ totals, const float* __restrict__ sum_old,
                                                               const int32_t* __restrict__ weight_old, const uint4* __restrict__ color_old, float* __restrict__ sum,
                                                               int32_t* __restrict__ weight, uint4* __restrict__ color) {
    tsdf_brick_move_one((int)blockIdx.x, (int)threadIdx.x, list_old, grid, flags, excl, totals, sum_old, weight_old, color_old, sum, weight, color);
}

// after the move: the grid and the list of the new set
__host__ __device__ inline void tsdf_brick_commit_one(int g, int32_t* __restrict__ grid, const uint32_t* __restrict__ flags, const int* __restrict__ excl,
                                                      const int* __restrict__ totals, int32_t* __restrict__ list) {
    const int r = tsdf_brick_rank(g, grid, flags, excl, totals);
    grid[g] = r;
    if (r >= 0) list[r] = g;
}
__global__ __launch_bounds__(256) void k_tsdf_brick_commit(int n_grid, int32_t* __restrict__ grid, const uint32_t* __restrict__ flags, const int* __restrict__ excl,
                                                           const int* __restrict__ totals, int32_t* __restrict__ list) {
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g < n_grid) tsdf_brick_commit_one(g, grid, flags, excl, totals, list);
}

// mpmvs_tsdf_set_bricks: an entry of a voxel that dims cut off is stored as 0
__global__ __launch_bounds__(kBrickVox) void k_tsdf_brick_clip(TsdfVol V, TsdfBricks B, float* __restrict__ sum, int32_t* __restrict__ weight, uint4* __restrict__ color) {
    int I, J, K;
    tsdf_brick_coords(B, B.list[blockIdx.x], I, J, K);
    const int l = (int)threadIdx.x;
    if (kBrick * I + (l & 7) < V.nx && kBrick * J + ((l >> 3) & 7) < V.ny && kBrick * K + (l >> 6) < V.nz) return;
    const size_t e = (size_t)blockIdx.x * kBrickVox + (size_t)l;
    sum[e] = 0.0f;
    weight[e] = 0;
    if (color) color[e] = make_uint4(0, 0, 0, 0);
}

// ---- B. integrate --------------------------------------------------------------------------------------------------------------
// tsdf_box_live of pm_tsdf.hpp for the brick at (I, J, K), cut to the lattice
__host__ __device__ inline bool tsdf_brick_live(const TsdfVol& V, const TsdfView& W, int I, int J, int K) {
    const int i0 = kBrick * I, j0 = kBrick * J, k0 = kBrick * K;
    return tsdf_box_live<8>(V, W, i0, i0 + 7 < V.nx - 1 ? i0 + 7 : V.nx - 1, j0, j0 + 7 < V.ny - 1 ? j0 + 7 : V.ny - 1, k0, k0 + 7 < V.nz - 1 ? k0 + 7 : V.nz - 1);
}

// entry `local` of the brick of rank `rank` at (I, J, K); a voxel that dims cut off does not exist and stays 0
__host__ __device__ inline void tsdf_sparse_integrate_one(const TsdfVol& V, const TsdfChunkArgs& A, unsigned live, int rank, int I, int J, int K, int local,
                                                          float* __restrict__ sum, int32_t* __restrict__ weight, uint4* __restrict__ color) {
    const int i = kBrick * I + (local & 7), j = kBrick * J + ((local >> 3) & 7), k = kBrick * K + (local >> 6);
    if (i < V.nx && j < V.ny && k < V.nz) tsdf_integrate_at(V, A, live, i, j, k, (size_t)rank * kBrickVox + (size_t)local, sum, weight, color);
}

__global__ __launch_bounds__(kBrickVox) void k_tsdf_sparse_integrate(TsdfVol V, TsdfBricks B, TsdfChunkArgs A, float* __restrict__ sum, int32_t* __restrict__ weight,
                                                                     uint4* __restrict__ color) {
    __shared__ unsigned live_s;
    int I, J, K;
    tsdf_brick_coords(B, B.list[blockIdx.x], I, J, K);
    if (threadIdx.x == 0) live_s = 0u;
    __syncthreads();
    if ((int)threadIdx.x < A.n && tsdf_brick_live(V, A.v[threadIdx.x], I, J, K)) atomicOr(&live_s, 1u << threadIdx.x);
    __syncthreads();
    const unsigned live = live_s;
    if (live) tsdf_sparse_integrate_one(V, A, live, (int)blockIdx.x, I, J, K, (int)threadIdx.x, sum, weight, color);
}

// ---- B. mesh ---------------------------------------------------------------------------------------------------------------------
// nb[c], c = corner code (bit 0: x, 1: y, 2: z): the rank of the brick at (I, J, K) + c, -1 if it is outside the grid or does not exist
__host__ __device__ inline void tsdf_brick_resolve(const TsdfBricks& B, int I, int J, int K, int c, int* nb) {
    const int i = I + (c & 1), j = J + ((c >> 1) & 1), k = K + (c >> 2);
    nb[c] = (i < B.bx && j < B.by && k < B.bz) ? B.grid[((size_t)k * (size_t)B.by + (size_t)j) * (size_t)B.bx + (size_t)i] : -1;
}
// the entry of the voxel at local (li, lj, lk) + corner code c of a brick whose neighbour table is nb, -1 if it does not exist
__host__ __device__ inline long long tsdf_brick_at(const int* nb, int local, uint32_t c) {
    const int x = (local & 7) + (int)(c & 1u), y = ((local >> 3) & 7) + (int)((c >> 1) & 1u), z = (local >> 6) + (int)((c >> 2) & 1u);
    const int r = nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
    return r < 0 ? -1ll : (long long)r * kBrickVox + (long long)((((z & 7) << 3 | (y & 7)) << 3) | (x & 7));
}
// the corner addressing that the mesh bodies of pm_tsdf.hpp ask for; they only follow corners that are valid, so the entry exists
struct TsdfBrickAt {
    const int* nb;
    int local;
    __host__ __device__ long long operator()(uint32_t c) const { return tsdf_brick_at(nb, local, c); }
};

struct TsdfBrickCell {
    int i, j, k;      // the voxel on the virtual lattice
    bool cell;        // it is the corner 000 of a cell
};
__host__ __device__ inline TsdfBrickCell tsdf_brick_cell(const TsdfVol& V, int I, int J, int K, int local) {
    TsdfBrickCell c;
    c.i = kBrick * I + (local & 7); c.j = kBrick * J + ((local >> 3) & 7); c.k = kBrick * K + (local >> 6);
    c.cell = c.i < V.nx - 1 && c.j < V.ny - 1 && c.k < V.nz - 1;
    return c;
}

// The corner tile of a brick: the 9 x 9 x 9 lattice points that its 8 x 8 x 8 cells touch, entry (z*9 + y)*9 + x, each with its
// validity and, if valid, its value f = sum / (float)weight.  A block stages it in LDS once (729 x 5 bytes; each corner is read by up
// to 8 cells), the division is done once per corner instead of once per cell and corner, and the bits are those of tsdf_cell.
// Measured against plain loads through the neighbour table: DESIGN.md section 23.6.
constexpr int kBrickTile = 729;
__host__ __device__ inline void tsdf_tile_load_one(const int* nb, int c, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                   float* tile_f, unsigned char* tile_v) {
    const int x = c % 9, y = (c / 9) % 9, z = c / 81;
    const int r = nb[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
    float f = 0.0f;
    unsigned char ok = 0;
    if (r >= 0) {
        const size_t at = (size_t)r * kBrickVox + (size_t)((((z & 7) << 3 | (y & 7)) << 3) | (x & 7));
        const int32_t w = weight[at];
        if (w >= min_weight) { ok = 1; f = sum[at] / (float)w; }
    }
    tile_f[c] = f;
    tile_v[c] = ok;
}
// tsdf_cell from the tile
__host__ __device__ inline void tsdf_tile_cell(const float* tile_f, const unsigned char* tile_v, int local, uint32_t& valid, uint32_t& inside) {
    valid = inside = 0u;
    const int x = local & 7, y = (local >> 3) & 7, z = local >> 6;
    for (uint32_t c = 0; c < 8; ++c) {
        const int at = ((z + (int)(c >> 2)) * 9 + (y + (int)((c >> 1) & 1u))) * 9 + x + (int)(c & 1u);
        if (!tile_v[at]) continue;
        valid |= 1u << c;
        if (tile_f[at] < 0.0f) inside |= 1u << c;
    }
}

// pass 1 (tsdf_mark_one): mask must be zero before; the tile must be loaded
__host__ __device__ inline void tsdf_sparse_mark_one(const TsdfVol& V, const int* nb, int I, int J, int K, int local, const float* tile_f, const unsigned char* tile_v,
                                                     uint32_t* mask, int* __restrict__ tcount) {
    int nt = 0;
    if (tsdf_brick_cell(V, I, J, K, local).cell) {
        uint32_t valid, inside;
        tsdf_tile_cell(tile_f, tile_v, local, valid, inside);
        nt = tsdf_mark_cell(TsdfBrickAt{nb, local}, valid, inside, mask);
    }
    tcount[(size_t)nb[0] * kBrickVox + (size_t)local] = nt;
}

// pass 3 (tsdf_vertex_one)
__host__ __device__ inline void tsdf_sparse_vertex_one(const TsdfVol& V, const int* nb, int I, int J, int K, int local, const float* __restrict__ sum,
                                                       const int32_t* __restrict__ weight, const uint4* __restrict__ color, const uint32_t* __restrict__ mask,
                                                       const int* __restrict__ vexcl, const int* __restrict__ vtile, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    const size_t vox = (size_t)nb[0] * kBrickVox + (size_t)local;
    const uint32_t m = mask[vox];
    if (!m) return;
    const TsdfBrickCell at = tsdf_brick_cell(V, I, J, K, local);
    tsdf_vertex_cell(V, TsdfBrickAt{nb, local}, at.i, at.j, at.k, vox, m, sum, weight, color, vexcl, vtile, xyz, rgb);
}

// pass 4 (tsdf_triangle_one); the tile must be loaded
__host__ __device__ inline void tsdf_sparse_triangle_one(const TsdfVol& V, const int* nb, int I, int J, int K, int local, const float* tile_f, const unsigned char* tile_v,
                                                         const uint32_t* __restrict__ mask, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                         const int* __restrict__ texcl, const int* __restrict__ ttile, int32_t* __restrict__ tri) {
    if (!tsdf_brick_cell(V, I, J, K, local).cell) return;
    uint32_t valid, inside;
    tsdf_tile_cell(tile_f, tile_v, local, valid, inside);
    tsdf_triangle_cell(TsdfBrickAt{nb, local}, valid, inside, (size_t)nb[0] * kBrickVox + (size_t)local, mask, vexcl, vtile, texcl, ttile, tri);
}

// one block per brick, one thread per voxel; the first 8 threads resolve the neighbour table; mark and triangles then stage the
// corner tile
#define PM_TSDF_BRICK_TILE                                                                                                      \
    __shared__ float tile_f[kBrickTile];                                                                                        \
    __shared__ unsigned char tile_v[kBrickTile];                                                                                \
    for (int c = (int)threadIdx.x; c < kBrickTile; c += kBrickVox) tsdf_tile_load_one(nb, c, sum, weight, min_weight, tile_f, tile_v); \
    __syncthreads();
#define PM_TSDF_BRICK_PROLOGUE                                        \
    __shared__ int nb_s[8];                                           \
    int I, J, K;                                                      \
    tsdf_brick_coords(B, B.list[blockIdx.x], I, J, K);                \
    if (threadIdx.x < 8) tsdf_brick_resolve(B, I, J, K, (int)threadIdx.x, nb_s); \
    __syncthreads();                                                  \
    int nb[8];                                                        \
    for (int c = 0; c < 8; ++c) nb[c] = nb_s[c];

__global__ __launch_bounds__(kBrickVox) void k_tsdf_sparse_mark(TsdfVol V, TsdfBricks B, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                                uint32_t* mask, int* __restrict__ tcount) {
    PM_TSDF_BRICK_PROLOGUE
    PM_TSDF_BRICK_TILE
    tsdf_sparse_mark_one(V, nb, I, J, K, (int)threadIdx.x, tile_f, tile_v, mask, tcount);
}
__global__ __launch_bounds__(kBrickVox) void k_tsdf_sparse_vertices(TsdfVol V, TsdfBricks B, const float* __restrict__ sum, const int32_t* __restrict__ weight,
                                                                    const uint4* __restrict__ color, const uint32_t* __restrict__ mask, const int* __restrict__ vexcl,
                                                                    const int* __restrict__ vtile, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    PM_TSDF_BRICK_PROLOGUE
    tsdf_sparse_vertex_one(V, nb, I, J, K, (int)threadIdx.x, sum, weight, color, mask, vexcl, vtile, xyz, rgb);
}
__global__ __launch_bounds__(kBrickVox) void k_tsdf_sparse_triangles(TsdfVol V, TsdfBricks B, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                                     const uint32_t* __restrict__ mask, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                                     const int* __restrict__ texcl, const int* __restrict__ ttile, int32_t* __restrict__ tri) {
    PM_TSDF_BRICK_PROLOGUE
    PM_TSDF_BRICK_TILE
    tsdf_sparse_triangle_one(V, nb, I, J, K, (int)threadIdx.x, tile_f, tile_v, mask, vexcl, vtile, texcl, ttile, tri);
}
#undef PM_TSDF_BRICK_PROLOGUE
#undef PM_TSDF_BRICK_TILE

}  // namespace pm
