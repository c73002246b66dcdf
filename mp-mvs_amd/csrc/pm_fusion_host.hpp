// pm_fusion_host.hpp -- the host end of a depth-map fusion call (mpmvs_fuse*, include/mpmvs.h): what the five entry points
// received, as one struct (FuseRequest), and the rules its arguments must keep before anything touches the device
// (fuse_check_request).  Host code only (no HIP): the stand-alone check tools/fuse_lists_check.cpp drives the rules under the
// address and undefined-behaviour sanitizers.
#pragma once

#include "../../include/mpmvs.h"
#include "pm_tracks_host.hpp"

namespace pm {

// One fusion call.  The inputs as include/mpmvs.h describes them; of the outputs either the per-pixel arrays (out_valid,
// out_points9) or `records` + `n_records` (PLY vertex records, compacted on the device), `tracks` with records only.
struct FuseRequest {
    int device, n;
    const mpmvs_camera* cams;
    const int* estimate;
    mpmvs_ctx* const* ctxs;   // nullable: per image the context whose device state holds its final maps
    const float* const* depths;
    const float* const* normals;
    const unsigned char* const* colors;
    int color_channels;
    const unsigned char* const* sky;
    const int *src_off, *src_ids;
    int flags;
    unsigned char* const* out_valid = nullptr;
    float* const* out_points9 = nullptr;
    unsigned char* const* out_masks = nullptr;
    unsigned char** records = nullptr;
    long long* n_records = nullptr;
    TrackSink* tracks = nullptr;
};

// 0, or the code the call ends with: -1 before -2 before -3.  entered: the device could be selected (its failure is a -1);
// max_slots: the slots of a pixel's used-list (pm_fusion.hpp, kMaxFuseNgb).
inline int fuse_check_request(const FuseRequest& q, bool entered, int max_slots) {
    if (q.n <= 0 || (q.color_channels != 1 && q.color_channels != 3) || !entered) return -1;
    // every view id is used as an index by the caller (host vectors, FuseView table, masks): reject lists that name images that do
    // not exist before anything is launched (the reference looks ids up in a map, src/PatchMatch.cpp:306-312)
    if (!q.src_off || !q.src_ids || q.src_off[0] != 0) return -2;
    // ... and lists that name a view twice or the image itself among its sources: the masks of a source are advanced once per
    // slot (a view named twice would be swapped back and the reference-order fixpoint would never settle), and the reference
    // masks the fused image's own pixels in place, which the per-image snapshot cannot express
    // ... and lists that do not start with their own image (slot 0 is never read as a source: a list without it would lose its
    // first source silently), an estimated image without a list (the scratch rows are addressed with num_ngb - 1), and an
    // estimated image with more slots than a pixel's used-list holds
    for (int i = 0; i < q.n; ++i) {
        const int b = q.src_off[i], e = q.src_off[i + 1];
        if (e < b) return -2;
        const int num_ngb = e - b;
        if (num_ngb > 0 && q.src_ids[b] != i) return -2;
        if (q.estimate[i] && (num_ngb == 0 || num_ngb > max_slots)) return -2;
        for (int k = b; k < e; ++k) {
            if (q.src_ids[k] < 0 || q.src_ids[k] >= q.n) return -2;
            if (k > b && q.src_ids[k] == i) return -2;
            for (int k2 = b; k2 < k; ++k2)
                if (q.src_ids[k2] == q.src_ids[k]) return -2;
        }
    }
    // a track's entries are addressed with int offsets inside one image
    for (int i = 0; i < q.n && q.tracks; ++i)
        if (q.estimate[i] && (long long)q.cams[i].width * q.cams[i].height * (q.src_off[i + 1] - q.src_off[i]) > 0x7fffffffLL) return -3;
    return 0;
}

}  // namespace pm
