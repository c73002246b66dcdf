// pm_fusion.hpp -- depth-map fusion on the GPU: the consumer of the
// hot path's depth/normal maps (reference RunFusion, src/PatchMatch.cpp:287-504).
//
// The reference fuses sequentially: every accepted point masks the source pixels it
// used, and later pixels / images skip masked pixels, so its result depends on raster
// order (and on a used_list that is never reset between pixels).  That cannot run in
// parallel.  This kernel implements the "snapshot" formulation of DESIGN.md section 8:
// images are still fused in index order, but all pixels of one image read the masks as
// they were when the image started; the masks it produces become visible to the next
// image.  One thread = one pixel; HBM-bound (per pixel: own depth/normal/colour plus,
// per source view, one mask byte, one depth, one normal, one colour).
//
// EXACT mode (k_fuse<true> + k_fuse_carry_local + k_scan_totals<LastValid> + k_fuse_mark) reproduces the reference's
// order-dependent result instead, still in parallel, as a fixpoint: within the image being fused every source pixel q gets a time tau(q) = the raster index of
// the first accepted pixel that masks it (-1: masked before this image, INT_MAX: never).  Given tau, every pixel t can be
// evaluated independently -- source pixel q is masked for t exactly when tau(q) < t -- and yields its consistent source
// pixels and its acceptance; the marks of an accepted pixel are the entries of the reference's used_list at that moment,
// i.e. per source slot the pixel of the LATEST raster index <= t that was consistent with that slot (the list is never
// reset between pixels, ref :382,:416,:470-495): an inclusive "last valid" scan in raster order.  The marks give a new tau;
// iterate until it stops changing.  Each pass is right for at least one more pixel than the one before (a pixel only depends
// on marks of earlier pixels), so the iteration ends at the unique fixpoint = the sequential result; real scenes need a
// handful of passes.
#pragma once

#include "pm_device.hpp"
#include "pm_scan.hpp"

namespace pm {

struct FuseView {
    CamDev cam;
    int w, h;
    const float* depth;
    const float* normal;  // 3 floats per pixel (world)
    const unsigned char* color;  // 8-bit, cch interleaved channels (1 = grey, 3 = B,G,R as cv::Vec3b)
    int cch;
    const unsigned char* sky;    // optional sky mask (> 0 = sky, reference :385-388) or null
    unsigned char* mask;         // snapshot read by the kernel (written only at a thread's own sky pixel)
    unsigned char* mask_next;    // marks written by the kernel
    int* tau;                    // exact mode: time of the first mark inside the image being fused (see above)
    int* tau_new;                // exact mode: the same, as produced by the current pass
};

// reference src/PatchMatch.cpp:211-231
PM_DEV void point_on_world(const CamDev& cam, int x, int y, float depth, float& o0, float& o1, float& o2) {
    backproject(cam, (float)x, (float)y, depth, o0, o1, o2);
}
// (its way back, project_depth, reference src/PatchMatch.cpp:251-261, is pm_device.hpp's: the depth render shares it)
PM_DEV bool round_index(float v, int& out) {
    const float f = v + 0.5f;
    if (!(f > -1.0f && f < 1.0e8f)) return false;
    out = (int)f;
    return true;
}

constexpr int kMaxFuseNgb = kMaxViews + 1;

// (world normal, depth) per pixel -- the state a PatchMatch context holds after Run() (GetDepthandNormal, ref .cu:1021-1034) -- into
// the dense depth map and the 3-float normal map the fusion reads: what the reference routes through depths.dmb / normals.dmb
__global__ __launch_bounds__(256) void k_split_planes(const float4* __restrict__ planes, float* __restrict__ depth, float* __restrict__ normal, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = planes[i];
    depth[i] = p.w;
    normal[3 * i] = p.x;
    normal[3 * i + 1] = p.y;
    normal[3 * i + 2] = p.z;
}

PM_DEV void load_color(const FuseView& V, size_t idx, float& c0, float& c1, float& c2) {
    if (V.cch == 3) {
        c0 = (float)V.color[idx * 3];
        c1 = (float)V.color[idx * 3 + 1];
        c2 = (float)V.color[idx * 3 + 2];
    } else {
        c0 = c1 = c2 = (float)V.color[idx];
    }
}

// EXACT: consq[(j - 1) * N + t] receives, for every pixel t of the image and source slot j, the source pixel that was
// consistent with t (or -1); out_valid is written for every pixel (0 / 1).
// TRACKS (include/mpmvs.h, "tracks"): an accepted pixel also leaves which slots entered its averages -- one u32, bit j - 1 for
// slot j, in row num_ngb - 1 of consq (the row after the last slot's) -- and, in the snapshot formulation, the source pixel
// of each such slot in consq as EXACT writes it.  Rows of slots without a bit, and everything at pixels that are not
// accepted, are not defined in the snapshot formulation; nothing reads them.  consq then has num_ngb rows.
template <bool EXACT, bool TRACKS = false>
__global__ __launch_bounds__(256) void k_fuse(const FuseView* __restrict__ views, int i, const int* __restrict__ src_ids, int num_ngb,
                                              int use_dynamic, unsigned char* __restrict__ out_valid, float* __restrict__ out9,
                                              int* __restrict__ consq) {
    const FuseView& R = views[i];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (c >= R.w || r >= R.h) return;
    const size_t pix = (size_t)r * R.w + c;
    const size_t npix = (size_t)R.w * R.h;
    if (EXACT) {
        out_valid[pix] = 0;
        for (int j = 1; j < num_ngb; ++j) consq[(size_t)(j - 1) * npix + pix] = -1;
    }
    if (R.mask[pix] == 1) return;
    if (R.sky && R.sky[pix] > 0) {  // only this thread ever reads mask[pix] of the image being fused
        R.mask[pix] = 1;
        R.mask_next[pix] = 1;
        return;
    }
    const float ref_depth = R.depth[pix];
    if (ref_depth <= 0.0f) return;
    const float n0 = R.normal[pix * 3], n1 = R.normal[pix * 3 + 1], n2 = R.normal[pix * 3 + 2];
    float X0, X1, X2;
    point_on_world(R.cam, c, r, ref_depth, X0, X1, X2);
    float sp0 = X0, sp1 = X1, sp2 = X2, sn0 = n0, sn1 = n1, sn2 = n2;
    float sc0, sc1, sc2;
    load_color(R, pix, sc0, sc1, sc2);
    int num = 0;
    float dyn = 0.0f;
    unsigned bits = 0;  // TRACKS: the slots that entered the sums
    int used[kMaxFuseNgb];
    for (int j = 0; j < num_ngb; ++j) used[j] = -1;
    for (int j = 1; j < num_ngb; ++j) {
        if (j == num_ngb - 1 && num == 0) break;  // ref :402-403
        const int s = src_ids[j];
        const FuseView& S = views[s];
        float u, v, pd;
        project_depth(S.cam, X0, X1, X2, u, v, pd);
        int sr, sc;
        if (!round_index(v, sr) || !round_index(u, sc)) continue;
        if (!(sc >= 0 && sc < S.w && sr >= 0 && sr < S.h)) continue;
        const size_t sidx = (size_t)sr * S.w + sc;
        if (EXACT ? (S.tau[sidx] < (int)pix) : (S.mask[sidx] == 1)) continue;
        const float sd = S.depth[sidx];
        if (sd <= 0.0f) continue;
        const float m0 = S.normal[sidx * 3], m1 = S.normal[sidx * 3 + 1], m2 = S.normal[sidx * 3 + 2];
        float T0, T1, T2;
        point_on_world(S.cam, sc, sr, sd, T0, T1, T2);
        float bu, bv, bd;
        project_depth(R.cam, T0, T1, T2, bu, bv, bd);
        const float dc = (float)c - bu, dr = (float)r - bv;
        const float err = __builtin_sqrtf(dc * dc + dr * dr);
        if (!(err < 2.0f)) continue;
        const float rel = __builtin_fabsf(bd - ref_depth) / ref_depth;
        if (!(rel < 0.01f)) continue;
        const float dot = (n0 * m0 + n1 * m1) + n2 * m2;
        float angle = d_acos(dot);
        if (angle != angle) angle = 0.0f;  // ref :233-242
        if (angle < 0.174533f) {
            used[j] = (int)sidx;
            if (EXACT) consq[(size_t)(j - 1) * npix + pix] = (int)sidx;
            if (TRACKS) bits |= 1u << (j - 1);
            sp0 += T0;
            sp1 += T1;
            sp2 += T2;
            sn0 += m0;
            sn1 += m1;
            sn2 += m2;
            float g0, g1, g2;
            load_color(S, sidx, g0, g1, g2);
            sc0 += g0;
            sc1 += g1;
            sc2 += g2;
            const float idx = (err + 200.0f * rel) + angle * 10.0f;
            dyn += d_exp(-idx);
            num++;
        }
    }
    const bool ok = use_dynamic ? (num >= 1 && dyn > 0.3f * (float)num) : (num >= 2);
    if (!ok) return;
    const float d = (float)num + 1.0f;
    float* o = out9 + pix * 9;
    o[0] = sp0 / d;
    o[1] = sp1 / d;
    o[2] = sp2 / d;
    o[3] = sn0 / d;
    o[4] = sn1 / d;
    o[5] = sn2 / d;
    o[6] = sc0 / d;
    o[7] = sc1 / d;
    o[8] = sc2 / d;
    out_valid[pix] = 1;
    if (!EXACT)
        for (int j = 1; j < num_ngb; ++j)
            if (used[j] != -1) views[src_ids[j]].mask_next[used[j]] = 1;  // idempotent
    if (TRACKS) {
        if (!EXACT)
            for (int j = 1; j < num_ngb; ++j)
                if (used[j] != -1) consq[(size_t)(j - 1) * npix + pix] = used[j];
        consq[(size_t)(num_ngb - 1) * npix + pix] = (int)bits;
    }
}

// ---------------------------------------------------------------------------
// exact mode: the used_list of the reference as an inclusive "last valid entry" scan over the raster order, per source slot
// (pm_scan.hpp, LastValid).  k_fuse_carry_local scans chunks of 256 pixels in place and records each chunk's last valid
// entry; k_scan_totals<LastValid>, one row per slot, turns those into the entry carried INTO each chunk; k_fuse_mark
// combines both.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void k_fuse_carry_local(int* __restrict__ consq, int npix, int nchunks, int* __restrict__ tails) {
    const int slot = blockIdx.y, chunk = blockIdx.x, t = chunk * kScanBlock + threadIdx.x;
    int* row = consq + (size_t)slot * npix;
    int tail;
    const int v = block_incl_scan<LastValid>(t < npix ? row[t] : -1, -1, tail);
    if (t < npix) row[t] = v;
    if (threadIdx.x == 0) tails[(size_t)slot * nchunks + chunk] = tail;
}

// marks of the accepted pixels: tau_new(q) = min(tau_new(q), t) for every entry of the used_list at time t
__global__ __launch_bounds__(256) void k_fuse_mark(const FuseView* __restrict__ views, const int* __restrict__ src_ids, int num_ngb,
                                                   const unsigned char* __restrict__ out_valid, const int* __restrict__ consq,
                                                   const int* __restrict__ carry, int npix, int nchunks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= npix || !out_valid[t]) return;
    for (int j = 1; j < num_ngb; ++j) {
        int q = consq[(size_t)(j - 1) * npix + t];
        if (q < 0) q = carry[(size_t)(j - 1) * nchunks + (t >> 8)];
        if (q >= 0) atomicMin(&views[src_ids[j]].tau_new[q], t);
    }
}

// tau0 from the masks of the earlier images: -1 = masked already, INT_MAX = free
__global__ __launch_bounds__(256) void k_fuse_tau_init(const unsigned char* __restrict__ mask, int n, int* __restrict__ tau) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) tau[q] = mask[q] == 1 ? -1 : 0x7fffffff;
}
// number of entries in which two tau arrays differ, added to *count
__global__ __launch_bounds__(256) void k_fuse_tau_diff(const int* __restrict__ a, const int* __restrict__ b, int n, int* __restrict__ count) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool d = q < n && a[q] != b[q];
    const unsigned long long m = __ballot(d);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (int)__popcll(m));
}
// the fixpoint's marks become masks for the following images
__global__ __launch_bounds__(256) void k_fuse_tau_to_mask(const int* __restrict__ tau, int n, unsigned char* __restrict__ mask) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n && tau[q] != 0x7fffffff) mask[q] = 1;
}

// ---------------------------------------------------------------------------
// Compaction of one image's fused points into the reference's PointCloud order (raster order inside the image; images are
// appended in index order) as PLY vertex records: x y z nx ny nz (float32) red green blue (uint8), 27 bytes, exactly what
// StoreColorPlyFileBinaryPointCloud writes (ref src/PatchMatch.cpp:145-198).  Three small passes, deterministic:
// per-256-pixel block counts -> exclusive scan (k_scan_totals<Sum>) -> scatter with in-block ranks, counts and ranks
// from the block scan of pm_scan.hpp over the 0/1 predicate.
// ---------------------------------------------------------------------------
constexpr int kPlyRecord = 27;

__global__ __launch_bounds__(kScanBlock) void k_fuse_count(const unsigned char* __restrict__ valid, int n, int* __restrict__ block_counts) {
    const int i = blockIdx.x * kScanBlock + threadIdx.x;
    int total;
    block_excl_scan<Sum>((i < n && valid[i]) ? 1 : 0, 0, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// block_offsets = block_counts after k_scan_totals<Sum>: exclusive prefix sums, [nb] = the image's point count
__global__ __launch_bounds__(kScanBlock) void k_fuse_scatter(const unsigned char* __restrict__ valid, const float* __restrict__ pts9, int n,
                                                             const int* __restrict__ block_offsets, const long long* __restrict__ base,
                                                             unsigned char* __restrict__ records) {
    const int i = blockIdx.x * kScanBlock + threadIdx.x;
    const int v = (i < n && valid[i]) ? 1 : 0;
    int total;
    const int rank = block_excl_scan<Sum>(v, 0, total);
    if (!v) return;
    const long long slot = *base + block_offsets[blockIdx.x] + rank;
    const float* p = pts9 + (size_t)i * 9;
    float rec[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
    const float big = 3.402823466e+38f;  // FLT_MAX
    const bool finite = (rec[0] < big && rec[0] > -big) && (rec[1] < big && rec[1] > -big) && (rec[2] < big && rec[2] >= -big);  // ref :176-178
    if (!finite) rec[0] = rec[1] = rec[2] = 0.0f;
    unsigned char* o = records + slot * kPlyRecord;
    const unsigned char* src = (const unsigned char*)rec;
    for (int k = 0; k < 24; ++k) o[k] = src[k];
    o[24] = (unsigned char)(int)p[8];  // red   <- colour[2] (the image is B,G,R; ref :181-186)
    o[25] = (unsigned char)(int)p[7];  // green
    o[26] = (unsigned char)(int)p[6];  // blue
}

// *base += count of the image just scattered (block_counts[nb] from k_scan_totals)
__global__ void k_fuse_advance(long long* __restrict__ base, const int* __restrict__ image_count) { *base += *image_count; }

// ---------------------------------------------------------------------------
// Tracks: per fused point the (image, pixel) pairs that were averaged, as CSR in the PLY's point order.  Per image: the
// length of every pixel's track (0 where there is no point) -> k_scan_tiles -> k_scan_totals<Sum> -> k_fuse_track_scatter,
// which writes into buffers of ONE image's size: the point's offset at the point's rank within the image (the rank of
// k_fuse_scatter), its entries at tile offset + exclusive.  The host takes both before the next image reuses the buffers;
// *entry_base, advanced by k_fuse_advance, makes the offsets absolute.  consq is the scratch k_fuse<., true> wrote and, in
// reference order, k_fuse_carry_local scanned in place: an entry of the pixel's own survives an inclusive LastValid scan,
// so the bits select exactly the entries of the evaluation that produced the point.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fuse_track_len(const unsigned char* __restrict__ valid, const int* __restrict__ bits, int n,
                                                        int* __restrict__ len) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) len[t] = valid[t] ? __popc((unsigned)bits[t]) + 1 : 0;
}

__global__ __launch_bounds__(kScanBlock) void k_fuse_track_scatter(const unsigned char* __restrict__ valid, const int* __restrict__ consq, int n, int image,
                                                                   const int* __restrict__ src_ids, int num_ngb,
                                                                   const int* __restrict__ block_offsets, const int* __restrict__ tile_offsets,
                                                                   const int* __restrict__ excl, const long long* __restrict__ entry_base,
                                                                   long long* __restrict__ point_off, int* __restrict__ ent_image,
                                                                   int* __restrict__ ent_pixel) {
    const int t = blockIdx.x * kScanBlock + threadIdx.x;
    const int v = (t < n && valid[t]) ? 1 : 0;
    int total;
    const int rank = block_excl_scan<Sum>(v, 0, total);
    if (!v) return;
    int e = tile_offsets[blockIdx.x] + excl[t];
    point_off[block_offsets[blockIdx.x] + rank] = *entry_base + e;
    ent_image[e] = image;
    ent_pixel[e] = t;
    const unsigned bits = (unsigned)consq[(size_t)(num_ngb - 1) * n + t];
    for (int j = 1; j < num_ngb; ++j)
        if (bits >> (j - 1) & 1u) {
            ++e;
            ent_image[e] = src_ids[j];
            ent_pixel[e] = consq[(size_t)(j - 1) * n + t];
        }
}

}  // namespace pm
