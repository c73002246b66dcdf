// pm_scan_host.hpp -- the host side of the library's scan (kernels: pm_scan.hpp), for the calls that turn flags or counts into
// offsets: the cloud grid and its query binning, the clustering passes, the mesh select and the simplification's kept triangles.
// Beside pm_host.hpp and not in it: this function names kernels, and every unit that includes it gets them into its code object.
#pragma once

#include "pm_host.hpp"
#include "pm_scan.hpp"

#pragma GCC visibility push(hidden)

// v[0, n) -> excl, the exclusive scan inside every tile of kScanBlock elements, and tsum, the exclusive scan of the tile totals;
// *grand (may be null) = the total of v.  With `add` the tile offsets are added in place, so that excl is the exclusive scan of the
// whole array; without it the kernels that read excl add tsum themselves.
inline hipError_t scan_offsets(hipStream_t stream, const int* v, int n, int* excl, int* tsum, int* grand, bool add) {
    const unsigned ntiles = ((unsigned)n + pm::kScanBlock - 1u) / pm::kScanBlock;
    hipError_t e = launch(pm::k_scan_tiles, dim3(ntiles), dim3(pm::kScanBlock), stream, v, n, excl, tsum);
    if (e == hipSuccess) e = launch(pm::k_scan_totals<pm::Sum>, dim3(1), dim3(pm::kScanBlock), stream, tsum, (int)ntiles, 0, grand);
    if (e == hipSuccess && add) e = launch(pm::k_vs_scan_add, dim3(ntiles), dim3(pm::kScanBlock), stream, excl, n, tsum);
    return e;
}

#pragma GCC visibility pop
