// pm_cluster_host.hpp -- the host end of the clustering passes (kernels: pm_cloud.hpp, pm_voxel.hpp, pm_scan.hpp), in their one place:
// points that are resident on the device go into the cells of a uniform grid, one cluster per occupied cell, numbered by first
// appearance.  mpmvs_cloud_voxel_downsample runs the three stages back to back; mpmvs_simplify_mesh puts its quadrics between the
// second and the third and reads the arrays afterwards.  Also the refusals both calls make before they touch the device
// (cluster_refusal).  Each call names itself and its things in the error texts (ClusterNames).
#pragma once

#include <cstdio>
#include <string>

#include "pm_host.hpp"
#include "pm_scan_host.hpp"
#include "pm_voxel.hpp"

#pragma GCC visibility push(hidden)

namespace pm {

// who: opens every text; things: what is clustered; cell: what the call calls its cell size; clusters: what it calls the clusters
struct ClusterNames {
    const char *who, *things, *cell, *clusters;
};

// -3 unless n_fin finite points within [mn, mx] fit a table and a grid of `cell`; else 0 with the table size and the grid
inline int cluster_refusal(const ClusterNames& nm, long long n_fin, const float mn[3], const float mx[3], float cell, int* slots_log2, VoxelGrid* g) {
    *slots_log2 = cloud_slots_log2(n_fin);
    if (*slots_log2 > kCloudMaxSlotsLog2)
        return call_fail(-3, std::string(nm.who) + ": more than 2^29 finite " + nm.things + " (the table would exceed 2^30 slots)");
    voxel_origin(mn, cell, *g);
    if (n_fin > 0) {
        double top = 0.0;
        const int a = voxel_span_axis(mx, *g, &top);
        if (a >= 0) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "%s: the %s span %.6g cells of edge %.6g along %c, more than 2^21 (extent / %s = %.6g)", nm.who, nm.things, top + 1.0,
                          g->e, "xyz"[a], nm.cell, ((double)mx[a] - (double)mn[a]) / g->e);
            return call_fail(-3, msg);
        }
    }
    return 0;
}

// The clusters of n points (d_xyz; n_fin > 0 of them finite) on the caller's stream, which outlives this object: its buffers go back to
// the pool once the stream has been waited for, and the clock, declared first, goes after them.  The stages return 0 or -100.
// every_pass: the borders of all six passes are marked, as mpmvs_cloud_voxel_pass_ms reports them; without it the marks 1, 2 and 7 are
// left out (an event between two kernels costs 2 to 3 us of device time) and the clock tells 0 -> 3, insert to scan, 4 -> 5, number,
// and 5 -> 6, accumulate.  The marks from 8 on are the caller's, for what it puts between and after the stages.
struct Clusters {
    PassClock<16> clock;   // 0 insert 1 first 2 flag + scan 3 (the host reads the count) 4 number 5 accumulate 6 finish 7
    const hipStream_t st;
    const ClusterNames nm;
    const bool every_pass;
    const float* d_xyz = nullptr;
    int n = 0, count = 0;
    VoxelGrid g{};
    Scratch slot_of, flag, num, tsum, total, keys, cnt, first, vox_of_slot;      // stage 1
    Scratch out_first, out_count, cluster_of, acc, out_xyz, out_normals, out_rgb;   // stages 2 and 3, sized by the count
    unsigned long long *S = nullptr, *N = nullptr, *C = nullptr;                   // the sums inside acc: S, then N, then C

    Clusters(hipStream_t stream, const ClusterNames& names, bool mark_every_pass)
        : st(stream), nm(names), every_pass(mark_every_pass), slot_of(st), flag(st), num(st), tsum(st), total(st), keys(st), cnt(st), first(st), vox_of_slot(st), out_first(st),
          out_count(st), cluster_of(st), acc(st), out_xyz(st), out_normals(st), out_rgb(st) {}

    int no_memory() const { return call_fail(-100, std::string(nm.who) + ": no device memory"); }
    dim3 blocks() const { return dim3(((unsigned)n + 255u) / 256u); }

    // Stage 1: the table, a slot per point, the leader of every slot and the scan of the leader flags; waits for the count.
    int mark(const float* xyz, int n_points, long long n_fin, int slots_log2, const VoxelGrid& grid) {
        d_xyz = xyz, n = n_points, g = grid;
        const size_t np = (size_t)n, slots = (size_t)1 << slots_log2;
        if (slot_of.alloc(np * 4) != hipSuccess || flag.alloc(np * 4) != hipSuccess || num.alloc(np * 4) != hipSuccess ||
            tsum.alloc((size_t)blocks().x * 4) != hipSuccess || total.alloc(4) != hipSuccess || keys.alloc(slots * 8) != hipSuccess ||
            cnt.alloc(slots * 4) != hipSuccess || first.alloc(slots * 4) != hipSuccess || vox_of_slot.alloc(slots * 4) != hipSuccess)
            return no_memory();
        CALLCHK(hipMemsetAsync(keys.p, 0xff, slots * 8, st));
        CALLCHK(hipMemsetAsync(cnt.p, 0, slots * 4, st));
        CALLCHK(hipMemsetAsync(first.p, 0xff, slots * 4, st));
        CALLCHK(clock.mark(0, st));
        CALLCHK(launch(k_cloud_insert, blocks(), dim3(256), st, d_xyz, n, g.o[0], g.o[1], g.o[2], g.e, (unsigned)(slots - 1), keys.as<unsigned long long>(),
                       cnt.as<int>(), slot_of.as<int>()));
        if (every_pass) CALLCHK(clock.mark(1, st));
        CALLCHK(launch(k_voxel_first, blocks(), dim3(256), st, n, slot_of.as<int>(), first.as<unsigned>()));
        if (every_pass) CALLCHK(clock.mark(2, st));
        CALLCHK(launch(k_voxel_flag, blocks(), dim3(256), st, n, slot_of.as<int>(), first.as<unsigned>(), flag.as<int>()));
        CALLCHK(scan_offsets(st, flag.as<int>(), n, num.as<int>(), tsum.as<int>(), total.as<int>(), true));
        CALLCHK(clock.mark(3, st));
        CALLCHK(hipMemcpyAsync(&count, total.p, 4, hipMemcpyDeviceToHost, st));
        CALLCHK(hipStreamSynchronize(st));
        if (count <= 0 || (long long)count > n_fin)
            return call_fail(-100, std::string(nm.who) + ": the device counted " + std::to_string(count) + " " + nm.clusters + " for " + std::to_string(n_fin) +
                                       " finite " + nm.things);
        return 0;
    }

    // Stage 2: the clusters' numbers, first members and counts, then the sums of the positions and, where given, of the normals and
    // the colours; cluster_of per point if wanted.  The buffers of stage 3 are allocated here, so that nothing waits between the two.
    int number_and_accumulate(const float* d_normals, const unsigned char* d_rgb, bool want_cluster_of) {
        const size_t np = (size_t)n, m = (size_t)count, parts = 1 + (d_normals ? 1 : 0) + (d_rgb ? 1 : 0);   // 3 x 64 bits per cluster each
        if (out_first.alloc(m * 4) != hipSuccess || out_count.alloc(m * 4) != hipSuccess || out_xyz.alloc(m * 12) != hipSuccess ||
            (d_normals && out_normals.alloc(m * 12) != hipSuccess) || (d_rgb && out_rgb.alloc(m * 3) != hipSuccess) || acc.alloc(parts * m * 24) != hipSuccess ||
            (want_cluster_of && cluster_of.alloc(np * 4) != hipSuccess))
            return no_memory();
        S = acc.as<unsigned long long>();
        N = d_normals ? S + 3 * m : nullptr;
        C = d_rgb ? S + 3 * m * (d_normals ? 2 : 1) : nullptr;
        CALLCHK(hipMemsetAsync(acc.p, 0, parts * m * 24, st));
        CALLCHK(clock.mark(4, st));   // the wait for the count is not device time
        CALLCHK(launch(k_voxel_number, blocks(), dim3(256), st, n, flag.as<int>(), num.as<int>(), slot_of.as<int>(), cnt.as<int>(), vox_of_slot.as<int>(),
                       out_first.as<int32_t>(), out_count.as<int32_t>()));
        CALLCHK(clock.mark(5, st));
        CALLCHK(launch(k_voxel_accumulate, blocks(), dim3(256), st, n, d_xyz, d_normals, d_rgb, g, slot_of.as<int>(), vox_of_slot.as<int>(), S, N, C,
                       cluster_of.as<int32_t>()));
        CALLCHK(clock.mark(6, st));
        return 0;
    }

    // Stage 3: the representative of every cluster: mean position, normalised normal sum, rounded mean colour.
    int finish() {
        CALLCHK(launch(k_voxel_finish, dim3(((unsigned)count + 255u) / 256u), dim3(256), st, count, d_xyz, out_first.as<int32_t>(), out_count.as<int32_t>(), g, S,
                       N, C, out_xyz.as<float>(), out_normals.as<float>(), out_rgb.as<unsigned char>()));
        if (every_pass) CALLCHK(clock.mark(7, st));
        return 0;
    }

    // with every_pass: the device times of the six passes, once the stream is idle; the last one runs from the end of accumulate, so
    // it is the finish pass only for a caller that puts nothing between the two
    int pass_ms(float ms[6]) const {
        static const int border[6][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {5, 6}, {6, 7}};
        for (int p = 0; p < 6; ++p) CALLCHK(clock.ms(border[p][0], border[p][1], &ms[p]));
        return 0;
    }
};

}  // namespace pm

#pragma GCC visibility pop
