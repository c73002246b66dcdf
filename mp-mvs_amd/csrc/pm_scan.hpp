// pm_scan.hpp -- the one prefix scan of the library: "scan an array that does not fit one block, then scatter by the
// result", as the prior's vertex compaction (pm_prior.hpp), the fusion's PLY compaction and used_list carry
// (pm_fusion.hpp) and the view selection's track offsets (pm_viewsel.hpp) need it.  Integers only; every scan combines
// `left op right` in element order, so an associative operator need not commute.
//   wave_incl_scan        64 lanes, log-step shuffles
//   block_incl/excl_scan  kScanBlock threads = 4 waves: wave scans plus the totals of the waves before, through LDS
//   k_scan_tiles          per tile of kScanBlock elements: exclusive + scan in the tile (optional) and the tile's total
//   k_scan_totals         one block per row: exclusive scan of the row's tile totals in place, in rounds of kScanBlock
//                         with a running carry (any count), and the row's grand total
//   k_vs_scan_add         adds the scanned tile totals to the in-tile scan: offsets over the whole array
// Every thread of the block must reach a block scan (it synchronises); on return its LDS is free for the next call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pm {

constexpr int kScanBlock = 256;

struct Sum {
    static __device__ __forceinline__ int apply(int left, int right) { return left + right; }
};
// the latest valid (>= 0) entry; identity -1
struct LastValid {
    static __device__ __forceinline__ int apply(int left, int right) { return right >= 0 ? right : left; }
};

template <class Op>
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v = Op::apply(up, v);
    }
    return v;
}

// `inc` = this thread's wave-inclusive value: returns the combined total of the waves before this one, `total` = the block's
template <class Op>
__device__ __forceinline__ int scan_wave_carry(int inc, int identity, int& total) {
    __shared__ int wave_total[kScanBlock / 64];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wave_total[wv] = inc;
    __syncthreads();
    int carry = identity, run = identity;
#pragma unroll
    for (int k = 0; k < kScanBlock / 64; ++k) {
        if (k == wv) carry = run;
        run = Op::apply(run, wave_total[k]);
    }
    total = run;
    __syncthreads();
    return carry;
}

template <class Op>
__device__ __forceinline__ int block_incl_scan(int v, int identity, int& total) {
    const int inc = wave_incl_scan<Op>(v);
    return Op::apply(scan_wave_carry<Op>(inc, identity, total), inc);
}

template <class Op>
__device__ __forceinline__ int block_excl_scan(int v, int identity, int& total) {
    const int inc = wave_incl_scan<Op>(v);
    const int up = __shfl_up(inc, 1, 64);
    return Op::apply(scan_wave_carry<Op>(inc, identity, total), (threadIdx.x & 63) ? up : identity);
}

// The two kernels that are no templates are `inline`: several translation units of the library include this header.  (nvcc would
// ignore the keyword on a kernel, which is all -Wcuda-compat has to say about it; clang gives them the linkage asked for.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
// totals[b] = sum of v[b * kScanBlock ..); excl (if given) [k] = sum of the elements before k in k's tile
inline __global__ __launch_bounds__(kScanBlock) void k_scan_tiles(const int* __restrict__ v, int n, int* __restrict__ excl, int* __restrict__ totals) {
    const size_t k = (size_t)blockIdx.x * kScanBlock + threadIdx.x;
    int total;
    const int r = block_excl_scan<Sum>(k < (size_t)n ? v[k] : 0, 0, total);
    if (excl && k < (size_t)n) excl[k] = r;
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// row blockIdx.x of totals[rows][n] -> its exclusive scan in place; grand (if given) [blockIdx.x] = the row's total
template <class Op>
__global__ __launch_bounds__(kScanBlock) void k_scan_totals(int* __restrict__ totals, int n, int identity, int* __restrict__ grand) {
    int* row = totals + (size_t)blockIdx.x * n;
    int carry = identity;
    for (int base = 0; base < n; base += kScanBlock) {
        const int k = base + threadIdx.x;
        int total;
        const int r = block_excl_scan<Op>(k < n ? row[k] : identity, identity, total);
        if (k < n) row[k] = Op::apply(carry, r);
        carry = Op::apply(carry, total);
    }
    if (grand && threadIdx.x == 0) grand[blockIdx.x] = carry;
}

// off[k] += the scanned total of k's tile (after k_scan_tiles and k_scan_totals<Sum>): the add pass of the view selection's track
// offsets, the cloud grid's slot offsets and the voxel numbering, named after its first user
inline __global__ __launch_bounds__(kScanBlock) void k_vs_scan_add(int* __restrict__ off, int n, const int* __restrict__ tsum) {
    const int64_t k = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    if (k < n) off[k] += tsum[blockIdx.x];
}
#pragma clang diagnostic pop

}  // namespace pm
