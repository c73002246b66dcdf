// pm_components.hpp -- the connected components of a point cloud on the grids of pm_cloud.hpp (mpmvs_cloud_components; contract:
// DESIGN.md section 20 and include/mpmvs.h).  Two finite points i != j are adjacent iff d2 = (dx*dx + dy*dy) + dz*dz <= r2 in fp32,
// no contraction: the candidate rule of mpmvs_cloud_nearest, which is symmetric in its two points (x_i - x_j and x_j - x_i are exact
// negatives, their squares are equal).  label[i] = the smallest index of i's component, size[i] = its number of points; -1 / 0 for a
// point with a non-finite coordinate.  A pure function of the point set: bit for bit the plain union-find over brute-force
// adjacency, independent of scheduling.
//
// A concurrent union-find in ONE pass over the edges (ECL-CC style: Jaiganesh and Burtscher, HPDC 2018), not label propagation: a
// chain of n points costs one pass, not n.
//   parent[]       an int per point of the cloud, indexed by the caller's index (pts[p].w): its own index at the start, -1 for a
//                  point that does not take part (never read again).  Invariant: parent[x] <= x.  A root has parent[x] == x.
//   k_cc_init      parent[i] = i or -1.
//   k_cc_hook      one thread per point, in the binned order of k_cloud_qbin / k_cloud_qorder, its neighbours handed over by
//                  cloud_walk (pm_cloud.hpp).  Only those with an index BELOW its own are united with it: every edge is handled once, by its larger
//                  end.  The thread carries its current root in a register and skips a neighbour whose root is that one.
//   cc_find        follows parent to a root, halving the path on the way: parent[prev] is overwritten with parent[curr], a node
//                  further down the same tree.  Such a store never touches a root (prev was seen with parent[prev] < prev, and a
//                  node that has left the roots never returns: every value ever stored is below its index).
//   cc_link        hooks the larger of two roots under the smaller with a compare-and-swap that expects the larger to be a root
//                  still.  On a lost race it finds the root from the value the swap returned -- strictly below the index it tried
//                  -- and tries again: the larger index of the pair falls with every retry, so the loop ends without any thread
//                  waiting for another.  No lock, no flag, no barrier between blocks.
//   k_cc_flatten   a launch of its own: label[i] = find(i).  All edges are united by then, so a tree is a component, and its root
//                  is below every member and a member itself: the smallest index.
//   k_cc_count     size[label[i]] += 1, an integer atomic, so the order never shows.  The lanes of a wave that share a label add
//                  once, by their number: a cloud that is one component would otherwise send every point to one address.
//   k_cc_gather    out_size[i] = size[label[i]].
// Why stale reads do no harm: every value parent[x] has ever held is a node of x's tree (trees merge, never split) below or at x,
// so a walk over old values still descends inside the tree; only the compare-and-swap decides a hook, and it is exact.  Reads of
// parent inside the hook pass are relaxed atomic loads at agent scope, the halving stores relaxed atomic stores.
// The four counts are taken on the host from the downloaded labels and sizes (mpmvs_cloud.hip).
// The per-thread bodies are host and device code, so that tools/components_check.cpp can replay them thread by thread and edge by
// edge under the sanitizers; there the atomics are plain reads and writes.
// cc_find, cc_link, cc_union and the flatten, count and gather passes know nothing of points: they live in pm_unionfind.hpp, which
// the components of a triangle mesh (pm_mesh.hpp) use as well.  Here are the two passes that read the cloud: init and hook.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_cloud.hpp"
#include "pm_unionfind.hpp"

namespace pm {

// ---- init ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void cc_init_one(size_t i, const float* __restrict__ xyz, int* __restrict__ parent) {
    parent[i] = cloud_finite(xyz[3 * i]) && cloud_finite(xyz[3 * i + 1]) && cloud_finite(xyz[3 * i + 2]) ? (int)i : -1;
}
__global__ __launch_bounds__(256) void k_cc_init(const float* __restrict__ xyz, int n, int* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cc_init_one(i, xyz, parent);
}

// ---- hook: thread j serves point order[j] (order may be null: j itself) -----------------------------------------------------------
__host__ __device__ inline void cc_hook_one(size_t j, const float* __restrict__ xyz, const int* __restrict__ order, const CloudGrid& g, int* __restrict__ parent) {
    const size_t i = order ? (size_t)order[j] : j;
    float x, y, z;
    int cx, cy, cz;
    if (!cloud_query_cell(xyz, i, g, x, y, z, cx, cy, cz)) return;
    const unsigned self = (unsigned)i;
    int root = cc_find(parent, (int)self);
    cloud_walk<1>(cx, cy, cz, g, [&](const uint4& t) {
        if (t.w >= self) return;   // the edge belongs to its larger end: no distance is taken for the others
        if (cloud_d2(x, y, z, t) <= g.r2) {
            const int other = cc_find(parent, (int)t.w);
            if (other != root) root = cc_link(parent, root, other);
        }
    });
}
__global__ __launch_bounds__(256) void k_cc_hook(const float* __restrict__ xyz, int n, const int* __restrict__ order, CloudGrid g, int* __restrict__ parent) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < (size_t)n) cc_hook_one(j, xyz, order, g, parent);
}

}  // namespace pm
