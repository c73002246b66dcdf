// pm_tsdf.hpp -- depth maps to a surface: a dense truncated-signed-distance volume and marching tetrahedra on the Kuhn split of
// its cells (mpmvs_tsdf_*; contract: include/mpmvs.h and DESIGN.md section 22).  Both calls are bit for bit their plain-loop
// statements and independent of scheduling: the integration is voxel-major with the views in call order, so a voxel's sums are
// formed by one thread in one order; all that the mesh passes share are bit masks (an OR of identical bits) and integer scans.
//
// Integrate (k_tsdf_integrate): a block is a tile of 64 x 4 voxels of one z layer, one thread per voxel, so a wave covers 64
//   consecutive i and the traffic of sum / weight / colour is coalesced.  The views of a chunk are kernel arguments, indexed
//   uniformly (scalar loads); the depth and colour images are plain arrays.  Per view the block first asks whether every voxel of
//   its tile lies behind the camera or outside the image (tsdf_view_live = tsdf_box_live on one layer: exact ranges from the four
//   corners of the tile, by the monotonicity of rounded arithmetic, see there) and skips the view if so.  Every voxel is projected
//   from its own position; nothing is stepped incrementally.
// Mesh: four passes, one thread per voxel (a voxel stands for the cell whose corner 000 it is, and owns the 7 edges that leave it in
//   positive directions):
//   1. k_tsdf_mark      per cell: the six tetrahedra, the used edges ORed into the owners' masks, the cell's triangle count (<= 12)
//   2. k_tsdf_scan_tiles / k_tsdf_sum_totals / k_scan_totals<Sum>: exclusive scans of the masks' popcounts and of the triangle
//                       counts with the block scan of pm_scan.hpp; the grand totals in 64 bits, so that the host can refuse a mesh
//                       beyond 2^31 - 1 before an int overflows
//   3. k_tsdf_vertices  per owner: one vertex per set slot, in slot order
//   4. k_tsdf_triangles per cell: the triangles again, a vertex number = the owner's base + the rank of the slot within its mask
// The case analysis and the winding are not typed in: tsdf_case_code builds the triangles of a case from the rule of the contract,
// tsdf_flip_code decides the winding of every (tetrahedron, case) with the vertices at the midpoints of their edges in integer
// arithmetic, both at compile time.
// The bodies of passes 1, 3 and 4 (tsdf_mark_cell, tsdf_vertex_cell, tsdf_triangle_cell) are written once, over an object that says
// where a cell's corners are stored; the brick-sparse volume of pm_tsdf_sparse.hpp runs the same bodies with its own addressing.
// The per-thread bodies are host and device code, so that tools/mesh_check.cpp replays the passes thread by thread under the
// sanitizers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_scan.hpp"

namespace pm {

constexpr int kTsdfChunk = 8;        // views per launch of the integration
constexpr int kTsdfTileX = 64, kTsdfTileY = 4;
constexpr float kTsdfCullBound = 0x1p40f;   // see tsdf_box_live

struct TsdfVol {
    int nx, ny, nz;
    float trunc;
    double o[3], voxel;   // the fp32 arguments widened: P_a = (float)(o[a] + (double)i_a * voxel)
};

struct TsdfView {
    float R[9], t[3];
    float K0, K2, K4, K5;
    int w, h;
    int cull;                     // the block test may be used: the camera and the volume are small enough (tsdf_box_live)
    const float* depth;           // [h * w]
    const unsigned char* color;   // [h * w * channels] or null
};
struct TsdfChunkArgs {
    int n, channels;
    TsdfView v[kTsdfChunk];
};

__host__ __device__ inline float tsdf_pos(const TsdfVol& V, int a, int i) { return (float)(V.o[a] + (double)i * V.voxel); }
__host__ __device__ inline size_t tsdf_index(const TsdfVol& V, int i, int j, int k) { return ((size_t)k * (size_t)V.ny + (size_t)j) * (size_t)V.nx + (size_t)i; }
__host__ __device__ inline bool tsdf_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }   // false for a NaN

__host__ __device__ inline float tsdf_cam_row(const float* R, float t, float px, float py, float pz) { return ((R[0] * px + R[1] * py) + R[2] * pz) + t; }

// Is the view alive for the box of voxels [i0, i1] x [j0, j1] x [k0, k1] (inside the lattice), or does every voxel of it fail step 2
// or step 4 of the statement?  Exact, by the monotonicity of rounded arithmetic.  First for one layer, k0 == k1:
//   With j, k fixed, P_x is a non-decreasing function of i (a rounded sum of a constant and a non-decreasing product), R * P_x is
//   monotone in P_x, and every further rounded sum with a fixed second operand keeps the order: xc, yc and z are monotone in i, in a
//   direction that only the sign of a camera entry decides, and likewise in j.  A function on a rectangle that is monotone in each
//   variable takes its extrema at corners: the four corners give the exact ranges [xc0, xc1], [yc0, yc1], [z0, z1] over the tile.
//   z1 <= 0: every voxel fails z > 0.
//   z0 > 0: a = K0 * xc (rounded) is monotone in xc, the rounded quotient a / z is monotone in a and, for a fixed a, in z; so over
//   the box [a0, a1] x [z0, z1], which holds every (a, z) of the tile, it takes its extrema at the four corner pairs.  Adding K2 and
//   0.5f, rounded, keeps the order: fu of every voxel lies in [fu0, fu1] computed by the statement's own operations.  fu1 < 0 or
//   fu0 >= W: every voxel fails step 4.  fv alike.
// This needs every intermediate to be a number (infinities are fine, a NaN is not): W.cull is set by the host only if every entry of
// R, t, K0, K2, K4, K5 and every |P| is at most 2^40 in magnitude, so that nothing before the quotient exceeds 2^122, and z0 > 0
// keeps the quotient from 0 / 0.  A comparison with a NaN is false and leaves the view alive.  A view that is not culled is simply
// evaluated: the result has the same bits either way.
//   One variable more, k0 < k1: with i, j fixed, P_z is a non-decreasing function of k, R[.][2] * P_z is monotone in P_z, and the
//   rounded sum ((R0*Px + R1*Py) + R2*Pz) + t has the rounded (R0*Px + R1*Py) as a fixed first operand, so xc, yc and z are monotone
//   in k too, in a direction that only the sign of a camera entry decides.  (In i and j the monotone term enters the inner sum, whose
//   rounded result then meets fixed operands: each rounded operation keeps the order.)  A function on a box that is monotone in each
//   variable takes its extrema at the corners: the 8 corners give the exact ranges of xc, yc and z over the box, and from there on
//   the argument is the one above word for word.
__host__ __device__ inline void tsdf_range(float v, float& lo, float& hi) {
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
}
__host__ __device__ inline bool tsdf_axis_dead(float k0, float k2, float c0, float c1, float z0, float z1, float size) {
    const float a0 = k0 * c0, a1 = k0 * c1;
    float q0 = a0 / z0, q1 = q0;
    tsdf_range(a0 / z1, q0, q1);
    tsdf_range(a1 / z0, q0, q1);
    tsdf_range(a1 / z1, q0, q1);
    const float f0 = (q0 + k2) + 0.5f, f1 = (q1 + k2) + 0.5f;
    return f1 < 0.0f || f0 >= size;
}
// kCorners = 4: one layer, k0 == k1, known where the call is written (the dense tile); 8: any box.  A box that happens to have one
// layer may be asked with 8: over duplicated corners the range is the same range.  The count is a template argument because a test
// of k0 == k1 at run time splits the 8 corners into two dependent halves: k_tsdf_sparse_integrate measured 1 to 5 % slower with it.
template <int kCorners>
__host__ __device__ inline bool tsdf_box_live(const TsdfVol& V, const TsdfView& W, int i0, int i1, int j0, int j1, int k0, int k1) {
    static_assert(kCorners == 4 || kCorners == 8, "a layer or a box");
    if (!W.cull) return true;
    float lo[3], hi[3];
    for (int corner = 0; corner < kCorners; ++corner) {
        const float px = tsdf_pos(V, 0, (corner & 1) ? i1 : i0), py = tsdf_pos(V, 1, (corner & 2) ? j1 : j0), pz = tsdf_pos(V, 2, (corner & 4) ? k1 : k0);
        for (int r = 0; r < 3; ++r) {
            const float c = tsdf_cam_row(W.R + 3 * r, W.t[r], px, py, pz);
            if (corner == 0) lo[r] = hi[r] = c;
            else tsdf_range(c, lo[r], hi[r]);
        }
    }
    if (hi[2] <= 0.0f) return false;
    if (!(lo[2] > 0.0f)) return true;
    return !(tsdf_axis_dead(W.K0, W.K2, lo[0], hi[0], lo[2], hi[2], (float)W.w) || tsdf_axis_dead(W.K4, W.K5, lo[1], hi[1], lo[2], hi[2], (float)W.h));
}
// the tile of voxels [i0, i0 + 64) x [j0, j0 + 4) of layer k
__host__ __device__ inline bool tsdf_view_live(const TsdfVol& V, const TsdfView& W, int i0, int j0, int k) {
    return tsdf_box_live<4>(V, W, i0, i0 + kTsdfTileX - 1 < V.nx - 1 ? i0 + kTsdfTileX - 1 : V.nx - 1, j0, j0 + kTsdfTileY - 1 < V.ny - 1 ? j0 + kTsdfTileY - 1 : V.ny - 1, k, k);
}

// voxel (i, j, k), stored at entry `vox` of the arrays, and the views of the chunk whose bit is set in `live`, in order: the one
// per-voxel body of the dense volume (vox = the linear index) and of the brick-sparse one (pm_tsdf_sparse.hpp: vox = the brick-major index)
__host__ __device__ inline void tsdf_integrate_at(const TsdfVol& V, const TsdfChunkArgs& A, unsigned live, int i, int j, int k, size_t vox, float* __restrict__ sum,
                                                  int32_t* __restrict__ weight, uint4* __restrict__ color) {
    const float px = tsdf_pos(V, 0, i), py = tsdf_pos(V, 1, j), pz = tsdf_pos(V, 2, k);
    float s_acc = sum[vox];
    int32_t w_acc = weight[vox];
    uint4 c_acc = color ? color[vox] : make_uint4(0, 0, 0, 0);
    bool touched = false, painted = false;
    for (int v = 0; v < A.n; ++v) {
        if (!((live >> v) & 1u)) continue;
        const TsdfView& W = A.v[v];
        const float xc = tsdf_cam_row(W.R, W.t[0], px, py, pz), yc = tsdf_cam_row(W.R + 3, W.t[1], px, py, pz), z = tsdf_cam_row(W.R + 6, W.t[2], px, py, pz);
        if (!(z > 0.0f)) continue;
        const float fu = ((W.K0 * xc) / z + W.K2) + 0.5f, fv = ((W.K4 * yc) / z + W.K5) + 0.5f;
        if (!(fu >= 0.0f && fu < (float)W.w && fv >= 0.0f && fv < (float)W.h)) continue;
        const size_t pix = (size_t)(int)floorf(fv) * (size_t)W.w + (size_t)(int)floorf(fu);   // 0 <= fu < w <= 2^24: exact and in range
        const float d = W.depth[pix];
        if (!(tsdf_finite(d) && d > 0.0f)) continue;
        const float s = d - z;
        if (s < -V.trunc) continue;
        s_acc += fminf(1.0f, s / V.trunc);
        w_acc += 1;
        touched = true;
        if (color && s <= V.trunc) {
            if (A.channels == 3) {
                const unsigned char* p = W.color + 3 * pix;
                c_acc.x += p[0]; c_acc.y += p[1]; c_acc.z += p[2];
            } else {
                const unsigned g = W.color[pix];
                c_acc.x += g; c_acc.y += g; c_acc.z += g;
            }
            c_acc.w += 1;
            painted = true;
        }
    }
    if (touched) { sum[vox] = s_acc; weight[vox] = w_acc; }
    if (painted) color[vox] = c_acc;
}
__host__ __device__ inline void tsdf_integrate_one(const TsdfVol& V, const TsdfChunkArgs& A, unsigned live, int i, int j, int k, float* __restrict__ sum,
                                                   int32_t* __restrict__ weight, uint4* __restrict__ color) {
    tsdf_integrate_at(V, A, live, i, j, k, tsdf_index(V, i, j, k), sum, weight, color);
}

__global__ __launch_bounds__(256) void k_tsdf_integrate(TsdfVol V, TsdfChunkArgs A, float* __restrict__ sum, int32_t* __restrict__ weight, uint4* __restrict__ color) {
    __shared__ unsigned live_s;
    const unsigned tiles_x = (unsigned)((V.nx + kTsdfTileX - 1) / kTsdfTileX), tiles_y = (unsigned)((V.ny + kTsdfTileY - 1) / kTsdfTileY);
    const unsigned b = blockIdx.x, bx = b % tiles_x, rest = b / tiles_x, by = rest % tiles_y;
    const int k = (int)(rest / tiles_y), i0 = (int)bx * kTsdfTileX, j0 = (int)by * kTsdfTileY;
    if (threadIdx.x == 0) live_s = 0u;
    __syncthreads();
    if ((int)threadIdx.x < A.n && tsdf_view_live(V, A.v[threadIdx.x], i0, j0, k)) atomicOr(&live_s, 1u << threadIdx.x);
    __syncthreads();
    const unsigned live = live_s;
    const int i = i0 + (int)(threadIdx.x & (kTsdfTileX - 1)), j = j0 + (int)(threadIdx.x / kTsdfTileX);
    if (live && i < V.nx && j < V.ny) tsdf_integrate_one(V, A, live, i, j, k, sum, weight, color);
}

// ---- the case analysis, built from the rule --------------------------------------------------------------------------------
// An edge of a tetrahedron between its vertices p < q is the code p | q << 2: always from the lower vertex to the higher one, which
// is also from lattice point A to B = A + off, because the vertices of a Kuhn tetrahedron ascend componentwise.
__host__ __device__ constexpr uint32_t tsdf_edge(int p, int q) { return p < q ? (uint32_t)(p | (q << 2)) : (uint32_t)(q | (p << 2)); }

// inside mask m (bit p: tetrahedron vertex p is inside) -> the number of triangles in bits 0..1 and their edges, 4 bits each, from bit 2
__host__ __device__ constexpr uint32_t tsdf_case_code(unsigned m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int p = 0; p < 4; ++p) {
        if ((m >> p) & 1u) in[ni++] = p;
        else out[no++] = p;
    }
    if (ni == 0 || ni == 4) return 0u;
    uint32_t e[6] = {0, 0, 0, 0, 0, 0};
    int nt = 1;
    if (ni == 1) {
        for (int r = 0; r < 3; ++r) e[r] = tsdf_edge(in[0], out[r]);
    } else if (ni == 3) {
        for (int r = 0; r < 3; ++r) e[r] = tsdf_edge(in[r], out[0]);
    } else {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        e[0] = tsdf_edge(a, c); e[1] = tsdf_edge(a, d); e[2] = tsdf_edge(b, d);
        e[3] = tsdf_edge(a, c); e[4] = tsdf_edge(b, d); e[5] = tsdf_edge(b, c);
        nt = 2;
    }
    uint32_t code = (uint32_t)nt;
    for (int r = 0; r < 3 * nt; ++r) code |= e[r] << (2 + 4 * r);
    return code;
}

// tetrahedron t = the t-th permutation (a, b, c) of the axes in lexicographic order -> the corner codes (bit 0: x, 1: y, 2: z) of its
// vertices v0 = 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 111, 4 bits each
__host__ __device__ constexpr uint32_t tsdf_tet_corners(int t) {
    const int a = t >> 1, r0 = a == 0 ? 1 : 0, r1 = a == 2 ? 1 : 2, b = (t & 1) ? r1 : r0;
    const uint32_t c1 = 1u << a, c2 = c1 | (1u << b);
    return (c1 << 4) | (c2 << 8) | (7u << 12);
}

// the winding of tetrahedron t: bit 2 m + r = triangle r of case m has to swap its last two vertices, so that (p1 - p0) x (p2 - p0)
// points from the mean of the inside corners to the mean of the outside corners when every vertex is put at the midpoint of its edge.
// Integers: midpoints doubled, the difference of the means times (inside count x outside count).  Bit 31: a case whose rule is
// undecided (the scalar product is 0); the static_assert below says there is none.
__host__ __device__ constexpr uint32_t tsdf_flip_code(int t) {
    const uint32_t corners = tsdf_tet_corners(t);
    uint32_t flips = 0u;
    for (unsigned m = 1; m < 15; ++m) {
        int sin[3] = {0, 0, 0}, sout[3] = {0, 0, 0}, ni = 0, no = 0;
        for (int p = 0; p < 4; ++p) {
            const uint32_t c = (corners >> (4 * p)) & 7u;
            for (int a = 0; a < 3; ++a) {
                if ((m >> p) & 1u) sin[a] += (int)((c >> a) & 1u);
                else sout[a] += (int)((c >> a) & 1u);
            }
            if ((m >> p) & 1u) ++ni;
            else ++no;
        }
        const uint32_t code = tsdf_case_code(m);
        const int nt = (int)(code & 3u);
        for (int r = 0; r < nt; ++r) {
            int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int v = 0; v < 3; ++v) {
                const uint32_t e = (code >> (2 + 4 * (3 * r + v))) & 15u;
                const uint32_t cp = (corners >> (4 * (e & 3u))) & 7u, cq = (corners >> (4 * (e >> 2))) & 7u;
                for (int a = 0; a < 3; ++a) P[v][a] = (int)((cp >> a) & 1u) + (int)((cq >> a) & 1u);
            }
            int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) { u[a] = P[1][a] - P[0][a]; w[a] = P[2][a] - P[0][a]; }
            const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            int dot = 0;
            for (int a = 0; a < 3; ++a) dot += n[a] * (ni * sout[a] - no * sin[a]);
            if (dot < 0) flips |= 1u << (2 * m + r);
            if (dot == 0) flips |= 1u << 31;
        }
    }
    return flips;
}
static_assert(((tsdf_flip_code(0) | tsdf_flip_code(1) | tsdf_flip_code(2) | tsdf_flip_code(3) | tsdf_flip_code(4) | tsdf_flip_code(5)) >> 31) == 0u,
              "the midpoint rule decides every winding");

// the same three tables at run time: switches over compile-time constants (no array that device code would have to address)
__host__ __device__ inline uint32_t tsdf_case_word(unsigned m) {
    switch (m) {
#define PM_TSDF_CASE(M) case M: { constexpr uint32_t w = tsdf_case_code(M); return w; }
        PM_TSDF_CASE(1) PM_TSDF_CASE(2) PM_TSDF_CASE(3) PM_TSDF_CASE(4) PM_TSDF_CASE(5) PM_TSDF_CASE(6) PM_TSDF_CASE(7)
        PM_TSDF_CASE(8) PM_TSDF_CASE(9) PM_TSDF_CASE(10) PM_TSDF_CASE(11) PM_TSDF_CASE(12) PM_TSDF_CASE(13) PM_TSDF_CASE(14)
#undef PM_TSDF_CASE
        default: return 0u;
    }
}
__host__ __device__ inline uint32_t tsdf_tet_word(int t, uint32_t& flips) {
    switch (t) {
#define PM_TSDF_TET(T) case T: { constexpr uint32_t c = tsdf_tet_corners(T), f = tsdf_flip_code(T); flips = f; return c; }
        PM_TSDF_TET(0) PM_TSDF_TET(1) PM_TSDF_TET(2) PM_TSDF_TET(3) PM_TSDF_TET(4)
#undef PM_TSDF_TET
        default: { constexpr uint32_t c = tsdf_tet_corners(5), f = tsdf_flip_code(5); flips = f; return c; }
    }
}

// slot of an edge offset (corner code 1..7) in the order 100, 010, 001, 110, 101, 011, 111 of (x, y, z), and the offset of a slot
__host__ __device__ inline int tsdf_slot_of(uint32_t off) { return (int)((0x65423100u >> (4 * off)) & 7u); }
__host__ __device__ inline uint32_t tsdf_off_of(int slot) { return (0x7653421u >> (4 * slot)) & 7u; }
__host__ __device__ inline size_t tsdf_step(const TsdfVol& V, uint32_t code) {
    return (size_t)(code & 1u) + (size_t)((code >> 1) & 1u) * (size_t)V.nx + (size_t)((code >> 2) & 1u) * (size_t)V.nx * (size_t)V.ny;
}

__host__ __device__ inline void tsdf_or(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, bits);
#else
    *p |= bits;
#endif
}
__host__ __device__ inline int tsdf_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

// the eight corners of the cell at `vox` (which must be a cell: i < nx - 1, j < ny - 1, k < nz - 1): bit c of `valid` and `inside`
// for corner code c
__host__ __device__ inline void tsdf_cell(const TsdfVol& V, size_t vox, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                          uint32_t& valid, uint32_t& inside) {
    valid = inside = 0u;
    for (uint32_t c = 0; c < 8; ++c) {
        const size_t at = vox + tsdf_step(V, c);
        const int32_t w = weight[at];
        if (w < min_weight) continue;
        valid |= 1u << c;
        if (sum[at] / (float)w < 0.0f) inside |= 1u << c;
    }
}

// the inside mask of tetrahedron `corners` of a cell, 0 if it does not emit
__host__ __device__ inline unsigned tsdf_tet_case(uint32_t corners, uint32_t valid, uint32_t inside) {
    unsigned m = 0u, ok = 1u;
    for (int p = 0; p < 4; ++p) {
        const uint32_t c = (corners >> (4 * p)) & 7u;
        ok &= valid >> c;
        m |= ((inside >> c) & 1u) << p;
    }
    return (ok & 1u) && m != 15u ? m : 0u;
}

__host__ __device__ inline bool tsdf_is_cell(const TsdfVol& V, size_t vox, int& i, int& j, int& k) {
    i = (int)(vox % (size_t)V.nx);
    const size_t r = vox / (size_t)V.nx;
    j = (int)(r % (size_t)V.ny);
    k = (int)(r / (size_t)V.ny);
    return i < V.nx - 1 && j < V.ny - 1 && k < V.nz - 1;
}

// ---- the per-cell bodies of passes 1, 3 and 4, once for both volumes --------------------------------------------------------------
// All that a volume adds is where a cell's corners are stored: `at(c)` is the entry of corner code c (bit 0: x, 1: y, 2: z) of the
// cell in sum / weight / colour and in the masks and scans, at(0) = `vox`, the cell's own entry.  The dense volume steps through the
// linear index; the brick-sparse one (pm_tsdf_sparse.hpp) goes through its block's neighbour table.  `valid` and `inside` are the
// cell's bits as the caller read them (tsdf_cell, or the sparse volume's staged tile).
struct TsdfDenseAt {
    const TsdfVol& V;
    size_t vox;
    __host__ __device__ size_t operator()(uint32_t c) const { return vox + tsdf_step(V, c); }
};

// pass 1 for a cell: the used edges into their owners' masks (zero before); returns the cell's triangle count
template <class At>
__host__ __device__ inline int tsdf_mark_cell(const At& at, uint32_t valid, uint32_t inside, uint32_t* mask) {
    int nt = 0;
    if ((inside & valid) == 0u || (inside & valid) == 255u) return nt;
    for (int t = 0; t < 6; ++t) {
        uint32_t flips;
        const uint32_t corners = tsdf_tet_word(t, flips);
        const unsigned m = tsdf_tet_case(corners, valid, inside);
        if (!m) continue;
        nt += (int)(tsdf_case_word(m) & 3u);
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (!(((m >> p) ^ (m >> q)) & 1u)) continue;
                const uint32_t cp = (corners >> (4 * p)) & 7u, cq = (corners >> (4 * q)) & 7u;
                tsdf_or(&mask[at(cp)], 1u << tsdf_slot_of(cq ^ cp));   // a corner of an emitting tetrahedron is valid: it exists
            }
    }
    return nt;
}

// pass 1: mask must be zero before
__host__ __device__ inline void tsdf_mark_one(const TsdfVol& V, size_t vox, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                              uint32_t* mask, int* __restrict__ tcount) {
    int i, j, k, nt = 0;
    if (tsdf_is_cell(V, vox, i, j, k)) {
        uint32_t valid, inside;
        tsdf_cell(V, vox, sum, weight, min_weight, valid, inside);
        nt = tsdf_mark_cell(TsdfDenseAt{V, vox}, valid, inside, mask);
    }
    tcount[vox] = nt;
}

__global__ __launch_bounds__(256) void k_tsdf_mark(TsdfVol V, size_t n_vox, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                   uint32_t* mask, int* __restrict__ tcount) {
    const size_t vox = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vox < n_vox) tsdf_mark_one(V, vox, sum, weight, min_weight, mask, tcount);
}

// pass 2, per tile of kScanBlock voxels: vexcl[k] = the set bits of the masks before k in its tile; tcount[k] becomes the triangles
// before k in its tile; totals[tile], totals[n_tiles + tile] = the tile's sums
__global__ __launch_bounds__(kScanBlock) void k_tsdf_scan_tiles(const uint32_t* __restrict__ mask, size_t n_vox, int* __restrict__ vexcl, int* __restrict__ tcount,
                                                                int* __restrict__ totals, int n_tiles) {
    const size_t k = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    int total;
    const int rv = block_excl_scan<Sum>(k < n_vox ? __popc(mask[k]) : 0, 0, total);
    if (k < n_vox) vexcl[k] = rv;
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
    const int rt = block_excl_scan<Sum>(k < n_vox ? tcount[k] : 0, 0, total);
    if (k < n_vox) tcount[k] = rt;
    if (threadIdx.x == 0) totals[n_tiles + blockIdx.x] = total;
}

// grand[row] += the sum of row blockIdx.y of totals[2][n_tiles], in 64 bits (integer atomics: any order gives the same sum)
__global__ __launch_bounds__(kScanBlock) void k_tsdf_sum_totals(const int* __restrict__ totals, int n_tiles, unsigned long long* __restrict__ grand) {
    const size_t k = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    int total;   // a tile's total is at most 12 * 256, a block's at most 12 * 2^16
    (void)block_incl_scan<Sum>(k < (size_t)n_tiles ? totals[(size_t)blockIdx.y * n_tiles + k] : 0, 0, total);
    if (threadIdx.x == 0 && total) atomicAdd(&grand[blockIdx.y], (unsigned long long)total);
}

// the colour byte of a value: (int)(val + 0.5f), saturated to 0..255, 0 for a NaN (neither can happen while 0 <= t <= 1)
__host__ __device__ inline unsigned char tsdf_byte(float val) {
    const float v = val + 0.5f;
    return v >= 255.0f ? (unsigned char)255 : v >= 0.0f ? (unsigned char)(int)v : (unsigned char)0;
}

// pass 3 for the voxel (i, j, k) at entry `vox`, whose mask m is not 0: one vertex per edge that it owns, in slot order.  vexcl /
// vtile: the scans of pass 2 (base = vexcl[vox] + vtile[tile])
template <class At>
__host__ __device__ inline void tsdf_vertex_cell(const TsdfVol& V, const At& at, int i, int j, int k, size_t vox, uint32_t m, const float* __restrict__ sum,
                                                 const int32_t* __restrict__ weight, const uint4* __restrict__ color, const int* __restrict__ vexcl,
                                                 const int* __restrict__ vtile, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    const int ijk[3] = {i, j, k};
    size_t out = (size_t)vexcl[vox] + (size_t)vtile[vox / kScanBlock];
    const float fa = sum[vox] / (float)weight[vox];
    float pa[3];
    for (int a = 0; a < 3; ++a) pa[a] = tsdf_pos(V, a, ijk[a]);
    for (int s = 0; s < 7; ++s) {
        if (!((m >> s) & 1u)) continue;
        const uint32_t off = tsdf_off_of(s);
        const size_t b = at(off);   // a set bit: the far corner is valid, so it exists
        const float fb = sum[b] / (float)weight[b];
        const float t = fa / (fa - fb);
        for (int a = 0; a < 3; ++a) {
            const float pb = tsdf_pos(V, a, ijk[a] + (int)((off >> a) & 1u));
            xyz[3 * out + a] = pa[a] + t * (pb - pa[a]);
        }
        if (rgb) {
            const uint4 ca = color[vox], cb = color[b];
            const unsigned sa[3] = {ca.x, ca.y, ca.z}, sb[3] = {cb.x, cb.y, cb.z};
            for (int c = 0; c < 3; ++c) {   // sums are B, G, R; the bytes go out R, G, B
                float val = 128.0f;
                if (ca.w > 0u && cb.w > 0u) {
                    const float ma = (float)sa[c] / (float)ca.w, mb = (float)sb[c] / (float)cb.w;
                    val = ma + t * (mb - ma);
                } else if (ca.w > 0u) {
                    val = (float)sa[c] / (float)ca.w;
                } else if (cb.w > 0u) {
                    val = (float)sb[c] / (float)cb.w;
                }
                rgb[3 * out + (size_t)(2 - c)] = tsdf_byte(val);
            }
        }
        ++out;
    }
}

// pass 3: the vertices of the edges that voxel `vox` owns
__host__ __device__ inline void tsdf_vertex_one(const TsdfVol& V, size_t vox, const float* __restrict__ sum, const int32_t* __restrict__ weight,
                                                const uint4* __restrict__ color, const uint32_t* __restrict__ mask, const int* __restrict__ vexcl,
                                                const int* __restrict__ vtile, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    const uint32_t m = mask[vox];
    if (!m) return;
    int i, j, k;
    (void)tsdf_is_cell(V, vox, i, j, k);
    tsdf_vertex_cell(V, TsdfDenseAt{V, vox}, i, j, k, vox, m, sum, weight, color, vexcl, vtile, xyz, rgb);
}

__global__ __launch_bounds__(256) void k_tsdf_vertices(TsdfVol V, size_t n_vox, const float* __restrict__ sum, const int32_t* __restrict__ weight,
                                                       const uint4* __restrict__ color, const uint32_t* __restrict__ mask, const int* __restrict__ vexcl,
                                                       const int* __restrict__ vtile, float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
    const size_t vox = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vox < n_vox) tsdf_vertex_one(V, vox, sum, weight, color, mask, vexcl, vtile, xyz, rgb);
}

// pass 4 for the cell at entry `vox`: its triangles again, a vertex number = the owner's base + the rank of the slot within the
// owner's mask.  texcl / ttile: the scans of the triangle counts
template <class At>
__host__ __device__ inline void tsdf_triangle_cell(const At& at, uint32_t valid, uint32_t inside, size_t vox, const uint32_t* __restrict__ mask,
                                                   const int* __restrict__ vexcl, const int* __restrict__ vtile, const int* __restrict__ texcl,
                                                   const int* __restrict__ ttile, int32_t* __restrict__ tri) {
    if ((inside & valid) == 0u || (inside & valid) == 255u) return;
    size_t out = (size_t)texcl[vox] + (size_t)ttile[vox / kScanBlock];
    for (int t = 0; t < 6; ++t) {
        uint32_t flips;
        const uint32_t corners = tsdf_tet_word(t, flips);
        const unsigned m = tsdf_tet_case(corners, valid, inside);
        if (!m) continue;
        const uint32_t code = tsdf_case_word(m);
        const int nt = (int)(code & 3u);
        for (int r = 0; r < nt; ++r) {
            int32_t id[3];
            for (int v = 0; v < 3; ++v) {
                const uint32_t e = (code >> (2 + 4 * (3 * r + v))) & 15u;
                const uint32_t cp = (corners >> (4 * (e & 3u))) & 7u, cq = (corners >> (4 * (e >> 2))) & 7u;
                const size_t owner = at(cp);
                const int slot = tsdf_slot_of(cq ^ cp);
                id[v] = vexcl[owner] + vtile[owner / kScanBlock] + tsdf_popc(mask[owner] & ((1u << slot) - 1u));
            }
            const bool flip = (flips >> (2 * m + r)) & 1u;
            tri[3 * out] = id[0];
            tri[3 * out + 1] = flip ? id[2] : id[1];
            tri[3 * out + 2] = flip ? id[1] : id[2];
            ++out;
        }
    }
}

// pass 4: the triangles of cell `vox`
__host__ __device__ inline void tsdf_triangle_one(const TsdfVol& V, size_t vox, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                  const uint32_t* __restrict__ mask, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                  const int* __restrict__ texcl, const int* __restrict__ ttile, int32_t* __restrict__ tri) {
    int i, j, k;
    if (!tsdf_is_cell(V, vox, i, j, k)) return;
    uint32_t valid, inside;
    tsdf_cell(V, vox, sum, weight, min_weight, valid, inside);
    tsdf_triangle_cell(TsdfDenseAt{V, vox}, valid, inside, vox, mask, vexcl, vtile, texcl, ttile, tri);
}

__global__ __launch_bounds__(256) void k_tsdf_triangles(TsdfVol V, size_t n_vox, const float* __restrict__ sum, const int32_t* __restrict__ weight, int min_weight,
                                                        const uint32_t* __restrict__ mask, const int* __restrict__ vexcl, const int* __restrict__ vtile,
                                                        const int* __restrict__ texcl, const int* __restrict__ ttile, int32_t* __restrict__ tri) {
    const size_t vox = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vox < n_vox) tsdf_triangle_one(V, vox, sum, weight, min_weight, mask, vexcl, vtile, texcl, ttile, tri);
}

}  // namespace pm
