// pm_kernels.hpp -- the __global__ kernels of the PatchMatch hot path for gfx950.
//
// One thread owns one reference pixel.  A 64-wide wavefront is a 16x8 pixel patch of one checkerboard colour (8 lanes x 8
// rows) in the update / filter launches and an 8x8 patch in the all-pixel launches; a block is four waves.  The 36 bilateral
// weight records of the pixel's window live in LDS (written once per pixel and launch, read by every evaluation).
// k_update walks its 14 hypotheses in two phases, each VIEW BY VIEW (the eight propagated candidates of a view back to back,
// then the current plane, then the five refinement candidates of a view back to back), through inlined copies of the
// unrolled 36-tap NCC loop (ncc_core, pm_device.hpp) -- four copies in the photometric kernel's ISA (58 KB of code; the
// instruction cache misses 2.6 k times in 293 M fetches per launch: profiles/r04_scratch_and_icache_bound.txt).
// MFMA is not used: there is no dense contraction on this path.
#pragma once

#include "pm_cand_tile.hpp"
#include "pm_device.hpp"

// waves per SIMD the NCC kernels are compiled for (2: the 72 KB of LDS weight records per block allow no more, and the update
// kernel squeezed into the 168 registers of 3 waves loses more than the third wave gains: profiles/EXPERIMENTS.md 14 and 22)
constexpr int kWavesPerSimd = 2;

namespace pm {

struct LaunchArgs {
    uint64_t seed;
    uint32_t launch;
    int iter;
    int scale;
    int parity;   // 0 black ((x+y) even), 1 red
    int ylimit;   // rows covered by the reference's checkerboard grid (ref .cu:1196)
    int top_k;
    float depth_min, depth_max;
    float two_ss, two_sc;  // 2*sigma_spatial^2, 2*sigma_color^2
    // -sqrt(dx^2 + dy^2) / two_ss of the 36 window taps [column][row] at this launch's scale: the same for every pixel, so the
    // host computes it once per launch (the same fp32 square root and division the kernel used to do 36 times per pixel)
    float spatial[36];
    // view-selection threshold of this iteration, ref .cu:832: `0.8 * expf(iter * iter / -90.0f)` multiplies in DOUBLE (0.8 is a
    // double literal) and rounds once to float; it depends on the iteration only, so the host forms it per launch
    float cost_threshold;
    int init_random;       // InitializeScore branch A (ref .cu:549)
    int use_prior;         // params.planar_prior
};

// (the sampling regions of the checkerboard propagation, kDirs / kNumDirs: pm_cand_tile.hpp)

// Wave shape of the checkerboard launches: 8 rows of 8 same-colour pixels, for both texel formats; a block stacks its waves
// vertically (2x2 or 4x1 arrangements of four waves: 3.52 / 3.61 against 3.45 ms, round 2, profiles/EXPERIMENTS.md 12).  Compact
// 2-D patches reuse more L1 lines between taps than flat rows.  Measured per update launch, cfg 1, view-major order (round 2): fp16
// texels (8 bytes) 8 / 16 / 32 rows: 3.37 / 3.40 / 4.01 ms; fp32 texels (16 bytes) 4 / 8 / 16 rows: 4.18 / 3.97 / 4.04 ms.
// (Slot-major order, mid round 2: fp16 2 / 4 / 8 / 16 rows 4.00 / 3.66 / 3.50 / 3.45 ms.  Round 1, 4-byte u8 quads: 4 rows 3.85,
// 8 rows 3.89, 2 rows 3.98, 16 rows 4.84.  Round 3, fp16: 4 / 8 / 16 rows 2.75 / 2.73 / 2.77 ms.)
constexpr int kWaveRows = 8;
// Threads per block of the update kernel, per variant (the filter keeps 256).  Chained launches (k_update) made small blocks pay
// where the taps of a wave stay close together: a one-wave block holds no LDS for slower siblings and fills freed slots wave by
// wave -- fp16 texels at window scale 0: 2.47 against 2.53 ms per pass (photometric; geometric -1.4 %, prior -1.8 %).  Everywhere
// else the four waves of a 16 x 32 block share lines in the L1 that four unrelated one-wave blocks do not: scale 1 +3.7 %, scale 2
// +34 %, fp32 texels +5 ... +60 % (round 5, 1600x1200, 8 views, tools/bench_scales.py).
template <bool U8, int SCALE>
constexpr int kUpdThreads = (U8 && SCALE == 0) ? 64 : 256;
// block width and height (pixels) of an NT-thread checkerboard launch
constexpr int kChkBlockW = 2 * (64 / kWaveRows);
template <int NT = 256>
constexpr int kChkBlockH = (NT / 64) * kWaveRows;

// Blocks are dealt round-robin to the 8 XCDs (block b and b+8 share an L2):
// renumber so that each XCD works through one contiguous run of the raster
// order, i.e. one horizontal band of the image whose source footprints overlap
// in that XCD's L2 (9.49 -> 8.13 ms per update launch).  Bijective for any
// block count; speed only, never correctness: every pixel is visited once.
PM_DEV int xcd_remap(int id, int n) {
    const int q = n >> 3, r = n & 7, xcd = id & 7, k = id >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// b: the block's position in raster order over the image (the launch decides which block takes which position: xcd_remap for
// the plain launches, the chained update kernel's ticket order)
template <int NT = 256>
PM_DEV bool checker_pixel(const ProblemDev& P, const LaunchArgs& a, int b, int parity, int& x, int& y, int& x0, int& y0) {
    constexpr int kLanesPerRow = 64 / kWaveRows;
    const int nbx = (P.W + kChkBlockW - 1) / kChkBlockW;
    const int by = b / nbx, bx = b - by * nbx;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    x0 = bx * kChkBlockW;
    y0 = by * kChkBlockH<NT>;
    y = y0 + wv * kWaveRows + lane / kLanesPerRow;
    x = x0 + 2 * (lane % kLanesPerRow);
    x += (y + parity) & 1;
    return x < P.W && y < P.H && y < a.ylimit;
}
// all-pixel launches: block = 16x16 pixels, wave = 8x8 patch of it (against 16x4 waves: profiles/EXPERIMENTS.md 49)
// (by0: the first block row of a launch that covers a band of rows only, k_depth_normal in the banded end of Run())
PM_DEV bool dense_pixel(const ProblemDev& P, int& x, int& y, int& x0, int& y0, int by0 = 0) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    x0 = blockIdx.x * 16;
    y0 = (blockIdx.y + by0) * 16;
    y = y0 + (wv >> 1) * 8 + (lane >> 3);
    x = x0 + (wv & 1) * 8 + (lane & 7);
    return x < P.W && y < P.H;
}
PM_DEV bool dense_pixel(const ProblemDev& P, int& x, int& y) {
    int x0, y0;
    return dense_pixel(P, x, y, x0, y0);
}

// dynamic LDS of the NCC kernels (pm_lds, pm_device.hpp): 18 float4 weight records per thread + the reference tile if it fits
inline size_t ncc_lds_bytes(int bw, int bh, int scale) {
    const int radius = 5 * (2 << scale) / 2;
    const int tile = (bw + 2 * radius) * (bh + 2 * radius);
    return (size_t)(kLdsWeightFloats + (tile <= 2048 ? tile : 0)) * sizeof(float);
}

// The update kernel re-uses the tile region after its prologue as the exchange area of the compacted refinement (below):
// 2 KB per wave, whether or not the tile itself is staged in LDS.  72 KB + 8 KB = half a CU's LDS: two blocks per CU as before.
constexpr int kXchgBytesPerWave = 2048;
template <int NT>
constexpr int kLdsXchgFloats = (NT / 64) * kXchgBytesPerWave / 4;  // = the largest LDS-resident reference tile of the update kernel (Win::tile_in_lds)
// (exactly that much: padding the one-wave block so that only 7 or 6 fit a CU costs 8 / 19 %, profiles/EXPERIMENTS.md 45)
template <int NT>
inline size_t update_lds_bytes() { return (size_t)(kLdsWeightFloatsOf<NT> + kLdsXchgFloats<NT>) * sizeof(float); }

// ---------------------------------------------------------------------------
// InitializeScore, ref .cu:536-573 (+ :497-534)
// ---------------------------------------------------------------------------
template <int MAXV, bool U8, int SCALE>
__global__ __launch_bounds__(256, kWavesPerSimd) void k_init(const ProblemDev* __restrict__ Pp, StateDev S, LaunchArgs a) {
    const ProblemDev& P = *Pp;
    int x, y, x0, y0;
    const bool valid = dense_pixel(P, x, y, x0, y0);
    RefWin rw;
    ref_window_of_pixel<SCALE, 16, 16>(P, x, y, x0, y0, valid, a.spatial, a.two_sc, rw);
    if (!valid) return;
    const int idx = y * P.W + x;
    const int V = P.V;
    Rng g = rng_make(a.seed, (uint32_t)idx, a.launch);

    float4 pl;
    if (a.init_random) {
        pl = random_normal(P, x, y, g);
        const float depth = rng_uniform(g) * (a.depth_max - a.depth_min) + a.depth_min;
        pl.w = plane_offset(P, x, y, depth, pl);
    } else if (a.use_prior && S.mask[idx] > 0 && S.costs[idx] >= 0.1f) {
        const float perturbation = 0.02f;
        const float4 pp = S.prior[idx];
        float dpert = pp.w;
        const float dmin_p = (1.0f - 3.0f * perturbation) * dpert;
        const float dmax_p = (1.0f + 3.0f * perturbation) * dpert;
        dpert = rng_uniform(g) * (dmax_p - dmin_p) + dmin_p;
        pl = perturbed_normal(P, x, y, pp, g, 0.18849556f);
        pl.w = dpert;
    } else {
        const float4 st = S.planes[idx];
        pl.x = (P.cam.R[0] * st.x + P.cam.R[1] * st.y) + P.cam.R[2] * st.z;
        pl.y = (P.cam.R[3] * st.x + P.cam.R[4] * st.y) + P.cam.R[5] * st.z;
        pl.z = (P.cam.R[6] * st.x + P.cam.R[7] * st.y) + P.cam.R[8] * st.z;
        pl.w = plane_offset(P, x, y, st.w, pl);
    }
    S.planes[idx] = pl;

    float cv[MAXV], sorted[MAXV];
    float m0, m1, m2;
    plane_to_m(P, pl, m0, m1, m2);
    int n_valid = 0;
    // every per-view cost of the stored plane is kept (S.own): the first update pass of either colour needs exactly these numbers
    // for "the current plane under the new weights" (update_body, phase B) as long as the pixel still holds this plane
    const size_t wh = (size_t)P.W * P.H;
    for (int v = 0; v < V; ++v) {
        const float c = ncc_cost<U8, SCALE, true>(P.views[v], rw, x, y, m0, m1, m2);
        (S.own + v * wh)[idx] = c;
        cv[v] = c;
        sorted[v] = c;
        if (c < 2.0f) n_valid++;
    }
    for (int i = 1; i < V; ++i) {
        const float tmp = sorted[i];
        int j = i;
        for (; j >= 1 && tmp < sorted[j - 1]; --j) sorted[j] = sorted[j - 1];
        sorted[j] = tmp;
    }
    uint32_t sel = 0;
    float cost = 2.0f;
    const int top_k = n_valid < a.top_k ? n_valid : a.top_k;
    if (top_k > 0) {
        float csum = 0.0f;
        for (int i = 0; i < top_k; ++i) csum += sorted[i];
        const float thr = sorted[top_k - 1];
        for (int v = 0; v < V; ++v)
            if (cv[v] <= thr) sel |= (1u << v);
        cost = csum / (float)top_k;
    }
    S.costs[idx] = cost;
    S.sel[idx] = sel;
}

// A private array that has to live in private MEMORY (plain loads and stores, scheduled like any others) instead of being
// promoted to registers: its address is shown to an empty asm statement.
PM_DEV void keep_in_memory(float* p) { asm volatile("" : : "v"(p)); }

// A loaded value that has to be loaded where the source says, whatever is done with it afterwards: without this a load whose
// value is used under a condition is moved under that condition, into a branch of its own.
PM_DEV float loaded_here(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// An index whose address arithmetic has to stay where it is used: without this the 64-bit addresses of the eight neighbour
// planes are formed once, ahead of the slot loop, and then spilled around the evaluations.
PM_DEV int pinned_here(int i) {
    asm volatile("" : "+v"(i));
    return i;
}

// Write-through stores (sc0 sc1) of the per-pixel results: the bytes go to memory at once instead of waiting in the XCD's L2, so
// that a block on ANOTHER XCD can read them within the same launch once the storing wave has waited for them (s_waitcnt vmcnt(0))
// and signalled (k_update below).  Inline asm: hipcc has no 16-byte store with cache-policy bits; the compiler's own vmcnt
// bookkeeping stays conservative with an extra store in flight, and k_update drains the counter itself before it signals.
PM_DEV void st_f32x4_wt(float4* p, const float4 v) {
    const f32x4q d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(d) : "memory");
}
PM_DEV void st_f32_wt(float* p, float v) { asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory"); }
PM_DEV void st_u32_wt(uint32_t* p, uint32_t v) { asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory"); }

PM_DEV float prior_term_body(float depth_diff, float angle_cos, float two_ds2, float two_as2) {
    const float ad = d_acos(angle_cos);
    return 0.5f + d_exp(-depth_diff * depth_diff / two_ds2) * d_exp(-ad * ad / two_as2);
}
// as a real call for the many-view variants of the update kernel: inlined three times next to the unrolled NCC loops it pushed
// the variants above 8 views into hundreds of spilled registers
__device__ __attribute__((noinline)) float prior_term_call(float depth_diff, float angle_cos, float two_ds2, float two_as2) {
    return prior_term_body(depth_diff, angle_cos, two_ds2, two_as2);
}
template <bool CALL>
PM_DEV float prior_term(float depth_diff, float angle_cos, float two_ds2, float two_as2) {
    if constexpr (CALL)
        return prior_term_call(depth_diff, angle_cos, two_ds2, two_as2);
    else
        return prior_term_body(depth_diff, angle_cos, two_ds2, two_as2);
}

// The points of update_body where a measurement build stamps the time (WaveTimer below; the callback is empty in every other build).
enum Stamp {
    kStampFirstEval,   // the prologue is over: the first NCC evaluation of phase A starts
    kStampPhaseA,      // phase A is over: every candidate's cost against every view is known
    kStampWeighted,    // view weights drawn, weighted candidate costs formed, min_idx known
    kStampCurrent,     // the current plane is evaluated under the new weights
    kStampDealBegin,   // acceptance of the best neighbour, draws and candidate planes done: in front of the first dealt round
    kStampDealEnd,     // behind the last dealt round
    kStampSections,
    kStampRound = kStampSections,   // top of a dealt round
    kStampPublished,                // behind the barrier that follows the publishing
    kStampEvaluated,                // behind the barrier that follows the evaluation
    kStampCollected                 // behind the barrier that follows the collecting
};
#ifdef PM_DBG_WAVETIME
// Measurement builds only: every wave of the update kernel records when it entered the kernel, when its block's dependencies were met
// (ready), when it started its first phase-A evaluation (first_eval: ready .. first_eval is the block's prologue -- reference tile,
// candidate tile, search, weight records) and when it ended (s_memrealtime, 100 MHz) and where it ran (HW_ID: SIMD / CU / SH / SE, XCC_ID), the first 4 u64 of the wave's record at
// [launch id % 16][raster block][wave]; tools/wave_timeline.py turns the records into the slot occupancy over time.
//
// The second half of the record (4 more u64) splits the wave's life after the prologue into the sections of update_body (the stamp
// points above, `Stamp`): the ticks from each section mark to the next as 32-bit fields, and -- accumulated over the dealt rounds --
// the ticks between the top of a round and the barrier behind the owners' publishing, and between the barrier behind the evaluation
// and the one behind the collecting: what a round spends OUTSIDE ncc_cost.  A section stamp first waits for the wave's outstanding
// loads, LDS operations and stores (they belong to the section that issued them) and for its own result.
constexpr int kWaveRecWords = 8;   // u64 per wave record (mpmvs_api.hip sizes the buffer with it, tools/wave_timeline.py reads it)
struct WaveTimer {
    unsigned long long t_enter, t_ready, t_eval;
    unsigned long long t_mark[kStampSections], t_round;
    unsigned publish, collect, rounds;
    PM_DEV static unsigned long long now_drained() {
        unsigned long long t;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
        return t;
    }
    PM_DEV WaveTimer() {
        t_enter = t_ready = t_eval = t_round = __builtin_amdgcn_s_memrealtime();
        for (int i = 0; i < kStampSections; ++i) t_mark[i] = 0;
        publish = collect = rounds = 0;
    }
    PM_DEV void ready() { t_ready = t_eval = __builtin_amdgcn_s_memrealtime(); }   // the block's dependencies are met: the update itself starts
    PM_DEV void first_eval() { t_eval = t_mark[kStampFirstEval] = __builtin_amdgcn_s_memrealtime(); }
    PM_DEV void stamp(int point) {   // `point` is a constant at every call
        if (point == kStampFirstEval) return first_eval();
        const unsigned long long t = now_drained();
        if (point < kStampSections) t_mark[point] = t;
        if (point == kStampRound) t_round = t, rounds += 1;
        if (point == kStampPublished) publish += (unsigned)(t - t_round);
        if (point == kStampEvaluated) t_round = t;
        if (point == kStampCollected) collect += (unsigned)(t - t_round);
    }
    PM_DEV void finish(unsigned long long* base, uint32_t launch, int b, int n_blocks) const {
        const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if ((threadIdx.x & 63) == 0 && b >= 0) {
            const unsigned waves = (unsigned)n_blocks * (blockDim.x >> 6);
            unsigned long long* rec = base + ((size_t)(launch & 15u) * waves + (unsigned)b * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kWaveRecWords;
            rec[0] = t_enter;
            rec[1] = t_end;
            unsigned long long prologue = t_eval - t_ready;   // ticks of 10 ns between "ready" and the first evaluation (0 for a wave without a pixel)
            prologue = prologue > 0xffffffull ? 0xffffffull : prologue;
            rec[2] = (prologue << 36) | ((unsigned long long)(xcc & 0xfu) << 32) | hw;
            unsigned long long waited = t_ready - t_enter;   // ticks of 10 ns between kernel entry and the start of the update (ticket, wait for the neighbours, barriers)
            waited = waited > 0xffffffull ? 0xffffffull : waited;
            rec[3] = ((unsigned long long)(unsigned)b << 32) | (waited << 8) | (threadIdx.x >> 6);
            // sections (all zero for a wave without a pixel: it never reached the first stamp)
            const auto span = [&](int from, int to) -> unsigned long long { return (unsigned)(t_mark[to] - t_mark[from]); };
            const bool ran = t_mark[kStampDealEnd] != 0;
            rec[4] = !ran ? 0ull : span(kStampFirstEval, kStampPhaseA) | (span(kStampPhaseA, kStampWeighted) << 32);
            rec[5] = !ran ? 0ull : span(kStampWeighted, kStampCurrent) | (span(kStampCurrent, kStampDealBegin) << 32);
            rec[6] = !ran ? 0ull : span(kStampDealBegin, kStampDealEnd) | ((unsigned long long)(unsigned)(t_end - t_mark[kStampDealEnd]) << 32);
            rec[7] = (unsigned long long)(publish & 0xffffffu) | ((unsigned long long)(collect & 0xffffffu) << 24) | ((unsigned long long)(rounds & 0xffffu) << 48);
        }
    }
};
#endif

// ---------------------------------------------------------------------------
// BlackPixelUpdate / RedPixelUpdate = CheckerboardPropagation +
// PlaneHypothesisRefinement, ref .cu:724-998 and :642-722
// ---------------------------------------------------------------------------
// One pixel update of one block: `b` is the block's raster position, `parity` the colour of this pass, `launch` its launch id (the
// key of the random streams), `thr` the view-selection threshold of its iteration (ref .cu:832).  The results leave through
// write-through stores (st_*_wt): what the chained launch below hands from one pass to the next.
// `use_own` (the same for the whole launch item): every pixel of this pass still holds the plane InitializeScore stored, and S.own
// holds that plane's photometric cost per view at this window scale -- phase B reads them instead of evaluating the plane again.
// (At window scales 1 and 2 the reference tile could be staged as a compact half tile of the pass's colour: built in round 6, bit-exact,
// 0-0.7 % on the scale-2 passes -- the prologue's 37 reads per pixel are not what scale 2 pays for, profiles/EXPERIMENTS.md 52.)
// `wait_for_neighbours` is called before the block's first load, `stamp` at the points of `Stamp` (the measurement builds' clock, empty otherwise).
template <bool GEOM, bool PRIOR, int MAXV, bool U8, int SCALE, class WAIT, class STAMP>
PM_DEV void update_body(const ProblemDev& P, const StateDev& S, const LaunchArgs& a, int b, int parity, uint32_t launch, float thr, bool use_own, WAIT wait_for_neighbours,
                        STAMP stamp) {
    constexpr int NT = kUpdThreads<U8, SCALE>, BW = kChkBlockW, BH = kChkBlockH<NT>;
    // gathers of two window columns ahead (ncc_core): always with the 8-byte texels; with the 16-byte ones where the variant
    // still has the 24 registers of a third column (8 views; more views spill 4 .. 81 registers around the evaluations)
    constexpr bool kDeep = U8 || MAXV == 8;
    constexpr bool kPriorCall = MAXV > 8;
    // Which variants park the refinement ingredients and the candidate costs in private memory: those that would otherwise spill
    // around the evaluations (fp32 texels with the planar prior, or with the geometric term above 16 views).  Measured per
    // variant: parking costs the non-spilling variants 1-4 %, and gains the spilling ones 3-6 %.
    constexpr bool kPark = !U8 && (PRIOR || (GEOM && MAXV > 16));
    // ... and the candidates' m vectors of phase A (see there)
    constexpr bool kParkM = !U8 && ((PRIOR && MAXV == 8) || (GEOM && MAXV == 32));
    // Where the loads of the candidates' planes are issued: right after the search, ahead of the weight records, or where the planes
    // are consumed.  In time the two are not told apart (2.280 against 2.269 ms per pass on cfg 1, 0.005 between runs of one build:
    // profiles/EXPERIMENTS.md 65), so registers decide, per variant: issued late, <photometric, 8 views, fp16 texels, scale 2> takes 239
    // registers instead of 215 and <geometric, 24 views, fp32 texels> spills 33 instead of 13; issued early, <geometric, 8 views, fp32
    // texels> spills 21 instead of 15.  Everywhere else the two orders allocate alike and the planes are loaded where they are used.
    constexpr bool kPlanesEarly = (U8 && SCALE == 2) || (GEOM && !U8 && MAXV > 8);
    // Which variants form the weighted candidate costs candidate by candidate, one private-memory load and one wait per (candidate,
    // weighted view), as all did until round 23: the planar prior with 9 .. 16 views.  Their 16 weights live in registers and are picked
    // by a chain of selects; view by view (below) the compiler forms the chain's 15 scalar conditions at once and spills 5 (fp32
    // texels) and 6 (fp16) scalar registers more than before.  And, in the build with 8-bit interpolation fractions only, the
    // photometric variant of 25 .. 32 views with fp16 texels at scale 0: 21 spilled scalar registers instead of 8.  Everywhere else
    // view by view allocates no worse (profiles/r23_kernel_resources.txt beside r23_kernel_resources_parent.txt).
#ifdef PM_TEX_Q8
    constexpr bool kQ8 = true;
#else
    constexpr bool kQ8 = false;
#endif
    constexpr bool kCostsByCandidate = (PRIOR && MAXV == 16) || (kQ8 && !GEOM && !PRIOR && MAXV == 32 && U8 && SCALE == 0);
    // Which variants keep the five refinement candidates' planes in registers instead of private memory (cpl, below).  In memory every
    // dealt round publishes with one scratch_load_dwordx4 and one s_waitcnt vmcnt(0) per candidate that has an item in it, on the same
    // in-order queue as the gathers, and the final acceptance reloads the survivors the same way.  In registers only what is distinct
    // stays alive (three normals, five offsets, most of them live anyway as plane_now and the draws): 3 .. 12 registers and 16 B of
    // scratch.  Two sieves, per variant (profiles/EXPERIMENTS.md 69).  Allocation: registers may cost, in both libraries, no spilled
    // register (vector or scalar) more than memory, at most 256 registers and at most 16 B of scratch
    // (profiles/r24_kernel_resources.txt, every variant in registers, beside r24_kernel_resources_parent.txt).  That leaves
    //   fp16 texels: photometric and geometric up to 24 views; photometric with 25 .. 32 views at scales 0 and 2 (scale 1 spills one
    //     scalar register more, the geometric variant too); the planar prior with 8 views (above 8: 48 B of scratch, 14 scalar spills);
    //   fp32 texels: the bucket of 9 .. 16 views without the prior.  The others sit at 248 .. 256 registers and spill 1 .. 53 more.
    // Time (profiles/r24_scales_modes.txt): of these, photometric with 9 .. 24 views and fp16 texels is 2.4 - 3.3 % SLOWER in registers
    // (218 -> 229 and 234 -> 245 registers) and stays in memory; the others gain 0.5 - 1.8 %, 25 .. 32 views 13 %.
    constexpr bool kPlanesInRegs = U8 ? (PRIOR ? MAXV == 8 : GEOM ? MAXV <= 24 : (MAXV == 8 || (MAXV == 32 && SCALE != 1)))
                                      : (!PRIOR && MAXV == 16);
    typedef Win<SCALE, BW, BH, kLdsXchgFloats<NT>> Wn;
    typedef CandTile<BW, BH> CT;
    static_assert(CT::floats <= kLdsWeightFloatsOf<NT>, "the candidate tile lives in the weight records' area until they are written");
    int x, y, x0, y0;
    const bool valid = checker_pixel<NT>(P, a, b, parity, x, y, x0, y0);
    const int W = P.W, Hh = P.H, V = P.V;

    // ---- the block's prologue.  Its round trips, in the order they are issued:
    //   wait for the neighbours, acquire  ->  reference tile (loads, into LDS)  ->  stored costs around the block (loads, into LDS)
    //   ->  search  ->  weight records  ->  the eight candidate planes (loads; ahead of the weight records where kPlanesEarly)  ->  phase A
    // Threads without a pixel take part in everything up to the last barrier of the prologue.
    wait_for_neighbours();
    __syncthreads();   // the acquire of the waiting wave stands before every load of the block that reads what a pass before wrote
    // the reference tile: all its loads first, then the stores (a loop of load-and-store pays one round trip per element), and into
    // LDS before the next loads go out (stored between them, its wait would split their batch)
    if constexpr (Wn::tile_in_lds) {
        float ref_v[(Wn::pitch * Wn::rows + NT - 1) / NT];
        load_ref_tile_values<NT, BW, BH, Wn::radius>(P, x0, y0, ref_v);
        store_ref_tile_values<NT, BW, BH, Wn::radius>(pm_lds + kLdsWeightFloatsOf<NT>, ref_v);
    }
    // -- the stored costs the block's searches can ask for, once per block (CandTile, pm_cand_tile.hpp).  Read UNCONDITIONALLY at
    // the position clamped into the image and replaced afterwards where the position lies outside: the loads sit in
    // straight-line code and go out back to back.
    // (loaded_here: left to itself the compiler moves each load under the test of its position, one branch and one s_waitcnt
    // vmcnt(0) per load -- 18 serialised round trips in the one-wave block)
    constexpr int kCostN = (CT::items + NT - 1) / NT;
    static_assert(kCostN <= 32, "one bit of `outside` per cell of a thread");
    const int tid = (int)threadIdx.x;
    __builtin_assume(tid >= 0 && tid < NT);
    const float* const costs = S.costs;
    float cost_v[kCostN];
    uint32_t outside = 0;   // bit k: the position of this thread's k-th cell lies outside the image
#pragma unroll
    for (int k = 0; k < kCostN; ++k) {
        int r, c, nx, ny;
        cand_tile_cell<BW, BH>(min(tid + k * NT, CT::items - 1), r, c);
        cand_tile_position<BW, BH>(r, c, x0, y0, parity, nx, ny);
        const int cx = nx < 0 ? 0 : (nx > W - 1 ? W - 1 : nx), cy = ny < 0 ? 0 : (ny > Hh - 1 ? Hh - 1 : ny);
        cost_v[k] = costs[__umul24((unsigned)cy, (unsigned)W) + (unsigned)cx];   // (one v_mad_u32_u24; rows and widths are far below 2^24)
        outside |= (((cx ^ nx) | (cy ^ ny)) != 0 ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < kCostN; ++k) cost_v[k] = loaded_here(cost_v[k]);
#pragma unroll
    for (int k = 0; k < kCostN; ++k) {
        if (tid + k * NT < CT::items) {
            int r, c;
            cand_tile_cell<BW, BH>(tid + k * NT, r, c);
            pm_lds[r * CT::pitch + c] = ((outside >> k) & 1u) ? kCandNone : cost_v[k];
        }
    }
    __syncthreads();

    // -- 8 sampling regions: position of the lowest stored cost (ref .cu:798-816).  A position outside the image holds kCandNone
    // in the tile and the comparison is strict, so it is never chosen and never sets its region's flag.
    int pos[8];
    uint32_t flags = 0;
    {
        int te, to;
        cand_tile_bases<BW, BH>(x, y, x0, y0, te, to);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float nc[12];
#pragma unroll
            for (int d = 0; d < kNumDirs[k]; ++d) nc[d] = pm_lds[cand_tile_index<BW, BH>(te, to, kDirs[k][d].x, kDirs[k][d].y)];
            float best = kCandNone;
            int bpos = 0;
#pragma unroll
            for (int d = 0; d < kNumDirs[k]; ++d) {
                if (best > nc[d]) {
                    best = nc[d];
                    bpos = (y + kDirs[k][d].y) * W + (x + kDirs[k][d].x);
                }
            }
            pos[k] = bpos;
            if (best < kCandNone) flags |= (1u << k);
        }
    }
    // (pos is 0 where a region has no candidate, and a position in the image otherwise, also for a thread without a pixel: the eight
    // loads are unconditional and in flight together)
    float4 cand_pl[8];
    if constexpr (kPlanesEarly) {
#pragma unroll
        for (int slot = 0; slot < 8; ++slot) cand_pl[slot] = S.planes[pos[slot]];
    }
    __syncthreads();   // the candidate tile is dead: its area takes the weight records

    RefWin rw;
    if (valid) ref_window_at_pixel<SCALE, BW, BH, NT, kLdsXchgFloats<NT>>(P, x, y, x0, y0, a.spatial, a.two_sc, rw);
    // the tile region becomes the exchange area of the refinement: every wave must be done reading the tile first
    if constexpr (Wn::tile_in_lds) __syncthreads();
    if (!valid) return;
    const int idx = y * W + x;
    Rng g = rng_make(a.seed, (uint32_t)idx, launch);

    // [view][candidate]: the eight costs of a view lie side by side, so that the weighted sums below fetch them as one batch
    alignas(16) float cost_arr[MAXV * 8];
    int cnt[MAXV];       // good count | bad count << 8   (ref .cu:834-845)
    float tmpw[MAXV];
    float probs[MAXV];
    float view_w[MAXV];
    for (int v = 0; v < V; ++v) {
        cnt[v] = 0;
        tmpw[v] = 0.0f;
    }
    // every entry is zeroed as in ref .cu:821: the refinement's geometric term
    // reads view_w[candidate 0..4], beyond V when V < 5 (ref .cu:689)
    for (int v = 0; v < MAXV; ++v) view_w[v] = 0.0f;

    // the pixel's current plane is read where it is needed (phase B) instead of being carried through phase A
    const float depth_sigma = (a.depth_max - a.depth_min) / 64.0f;
    const float two_ds2 = (2.0f * depth_sigma) * depth_sigma;
    const float angle_sigma = 0.08726646f;
    const float two_as2 = (2.0f * angle_sigma) * angle_sigma;
    const float beta = 0.18f;

    float4 plane_now = make_float4(0.f, 0.f, 0.f, 0.f), pp = make_float4(0.f, 0.f, 0.f, 0.f);
    float depth_now = 0.0f, cost_now = 0.0f, geom_now = 0.0f, restricted_cost = 0.0f, weight_norm = 0.0f;
    float depth_prior = 0.0f;
    // The ingredients of the five refinement candidates are drawn together (the order of the random draws is the
    // reference's) but consumed one evaluation at a time: they wait in private memory, not in registers that the
    // evaluations in between would have to spill.  Normals: 0 = current plane, 1 = random, 2 = perturbed; depths:
    // 0 = current, 1 = random, 2 = perturbed.
    float park_n[9];
    float park_d[3];
    float final_costs[8];  // written after phase A, read again only after the evaluation of the current plane: parked as well
    if (kPark) {
        keep_in_memory(park_n);
        keep_in_memory(park_d);
        keep_in_memory(final_costs);
    }
    uint32_t temp_sel = 0;
    int min_idx = 0;
    bool masked = false;

    // ---- phase A: the 8 propagated candidates against every view (ref .cu:798-819), VIEW BY VIEW: the eight evaluations of
    // a view follow each other, so that a wave keeps sampling one source texture (the candidates are the planes of
    // neighbouring pixels and land close to each other in it: the later ones find their texels in the L1) instead of walking
    // through all textures once per candidate; the per-view statistics (good / bad counts, weight sum) become two scalars.
    // The candidates' m vectors wait in private memory (fetched one evaluation ahead).
    // Where the variant has the registers, the m vectors live there and are picked by register index (s_set_gpr_idx_on): a
    // scratch load per value sits on the same in-order vmcnt queue as the gathers and costs 2 % (fp16 texels) to 3.5 % (fp32)
    // of the launch.  Parked in private memory only in the two variants that would otherwise spill around the evaluations.
    float cand_m[8 * 3];
    if (kParkM) keep_in_memory(cand_m);
#pragma unroll
    for (int slot = 0; slot < 8; ++slot) {
        float m0, m1, m2;
        if constexpr (!kPlanesEarly) cand_pl[slot] = S.planes[pos[slot]];
        plane_to_m(P, cand_pl[slot], m0, m1, m2);
        cand_m[3 * slot] = m0, cand_m[3 * slot + 1] = m1, cand_m[3 * slot + 2] = m2;
    }
    stamp(kStampFirstEval);
    for (int v = 0; v < V; ++v) {
        int cn = 0;       // good count | bad count << 8   (ref .cu:834-845)
        float tw = 0.0f;
        float n0 = cand_m[0], n1 = cand_m[1], n2 = cand_m[2];
        for (int slot = 0; slot < 8; ++slot) {
            const float m0 = n0, m1 = n1, m2 = n2;
            const int nxt = 3 * (slot < 7 ? slot + 1 : slot);
            n0 = cand_m[nxt], n1 = cand_m[nxt + 1], n2 = cand_m[nxt + 2];
            float c;
            if ((flags >> slot) & 1u)
                c = ncc_cost<U8, SCALE, kDeep, NT>(P.views[v], rw, x, y, m0, m1, m2);
            else
                c = (slot == 0 && v == 0) ? 2.0f : 0.0f;  // `= {2.0f}` initialiser quirk, ref .cu:795
            cost_arr[v * 8 + slot] = c;
            if (c < thr) {
                tw += d_exp_inrange((c * c) / (-0.18f));  // c in [0, 2]: argument in [-22.3, 0]
                cn += 1;
            }
            if (c > 1.2f) cn += 256;
        }
        cnt[v] = cn;
        tmpw[v] = tw;
    }
    stamp(kStampPhaseA);
    {
    // ---- view weights (ref .cu:821-878)
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const int idx_w = pinned_here(idx);
    if (flags & 1u) s0 = S.sel[idx_w - W];
    if (flags & 2u) s1 = S.sel[idx_w + W];
    if (flags & 4u) s2 = S.sel[idx_w - 1];
    if (flags & 8u) s3 = S.sel[idx_w + 1];
    float psum = 0.0f;
    for (int v = 0; v < V; ++v) {
        float vp = 0.0f;
        if (flags & 1u) vp += ((s0 >> v) & 1u) ? 0.9f : 0.1f;
        if (flags & 2u) vp += ((s1 >> v) & 1u) ? 0.9f : 0.1f;
        if (flags & 4u) vp += ((s2 >> v) & 1u) ? 0.9f : 0.1f;
        if (flags & 8u) vp += ((s3 >> v) & 1u) ? 0.9f : 0.1f;
        const int good = cnt[v] & 0xff, bad = cnt[v] >> 8;
        float pr;
        if (good > 2 && bad < 3)
            pr = (vp * tmpw[v]) / (float)good;
        else if (bad < 3)
            pr = vp * d_exp((thr * thr) / (-0.32f));
        else
            pr = 0.0f;
        probs[v] = pr;
        psum += pr;
    }
    const float inv = 1.0f / psum;  // 0 * inf = NaN when everything vanished (ref .cu:42-56)
    float cum = 0.0f;
    for (int v = 0; v < V; ++v) {
        cum += probs[v] * inv;
        probs[v] = cum;
    }
    probs[V - 1] = 1.0f;
    for (int s = 0; s < 15; ++s) {
        const float rp = rng_uniform(g) - 1.1920928955078125e-7f;
        for (int v = 0; v < V; ++v)
            if (probs[v] > rp) {
                view_w[v] += 1.0f;
                break;
            }
    }
    for (int v = 0; v < V; ++v)
        if (view_w[v] > 0.0f) {
            temp_sel |= (1u << v);
            weight_norm += view_w[v];
        }
    // ---- weighted candidate costs (ref .cu:880-899)
    float fcv[8];
    if constexpr (GEOM) {
        // VIEW by view, the geometric checks of the eight candidates of a view together: their forward halves first (eight
        // depth gathers in flight), then their backward halves -- a check issued and finished on its own exposes the whole
        // latency of its gather, 8 x V times per pixel.  For a fixed candidate the views are still added in ascending order.
        float gz[8];  // depth of the candidate's plane at this pixel: shared by the checks of all views
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            fcv[i] = 0.0f;
            gz[i] = ((flags >> i) & 1u) ? depth_from_plane(P, S.planes[pos[i]], x, y) : 0.0f;
        }
        for (int v = 0; v < V; ++v) {
            const float w = view_w[v];
            if (!(w > 0.0f)) continue;
            GeomCheck gc[8];
            // the view's eight photometric costs leave private memory ahead of the depth gathers, as one batch (loaded_here: fetched
            // where they are used, each pays its own round trip between two checks)
            float c8[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c8[i] = cost_arr[v * 8 + i];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((flags >> i) & 1u) gc[i].issue(P.views[v], gz[i], x, y);
#pragma unroll
            for (int i = 0; i < 8; ++i) c8[i] = loaded_here(c8[i]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float c = c8[i];
                if ((flags >> i) & 1u)
                    fcv[i] += w * (c + 0.2f * gc[i].finish(P.views[v], x, y));
                else
                    fcv[i] += w * (c + 0.1f * 3.0f);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            fcv[i] = fcv[i] / weight_norm;
            final_costs[i] = fcv[i];
        }
    } else if constexpr (kCostsByCandidate) {
        for (int i = 0; i < 8; ++i) {
            float fc = 0.0f;
            for (int v = 0; v < V; ++v)
                if (view_w[v] > 0.0f) fc += view_w[v] * cost_arr[v * 8 + i];
            const float fci = fc / weight_norm;
            final_costs[i] = fci;
            fcv[i] = fci;
        }
    } else {
        // VIEW by view as well: the weight and the eight costs of a view are fetched from private memory together and waited for
        // once (loaded_here: fetched under the test of the weight, every cost pays a round trip of its own, one after the other),
        // then every candidate takes its term under the lane's test.  For a fixed candidate the views are still added in
        // ascending order, each as w * c and then +; a view without weight adds nothing, not a zero product.
#pragma unroll
        for (int i = 0; i < 8; ++i) fcv[i] = 0.0f;
        const auto add_view = [&](int v) {
            const float w = view_w[v];
            float c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = cost_arr[v * 8 + i];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = loaded_here(c[i]);
            const bool weighted = w > 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float sum = fcv[i] + w * c[i];
                fcv[i] = weighted ? sum : fcv[i];
            }
        };
        // (unrolled where the bucket has 8 views: the weights live in registers there and are named instead of picked through a
        // chain of selects; a loop that leaves early is unrolled by its upper bound only up to 8 trips)
        if constexpr (MAXV == 8) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                if (v >= V) break;
                add_view(v);
            }
        } else {
            for (int v = 0; v < V; ++v) add_view(v);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            fcv[i] = fcv[i] / weight_norm;
            final_costs[i] = fcv[i];
        }
    }
    {
        float mc = fcv[0];
        for (int i = 1; i < 8; ++i)
            if (fcv[i] <= mc) {
                mc = fcv[i];
                min_idx = i;
            }
    }
    }
    stamp(kStampWeighted);

    // ---- phase B: the current plane under the new weights (ref .cu:901-913), the acceptance of the best neighbour, then the
    // 5 refinement candidates (ref .cu:642-722).  From here on a view with weight 0 contributes exactly +0.0 to every sum (all
    // costs are finite), so its evaluation is dead work; the reference computes it regardless (ref .cu:681,903).
    {
        const float4 pl = S.planes[pinned_here(idx)];
        plane_now = pl;
        float gz = 0.0f;
        if (GEOM) gz = depth_from_plane(P, pl, x, y);
        float tc = 0.0f, tg = 0.0f;
        if (use_own) {
            // The first pass of this colour after InitializeScore: `pl` is the plane k_init stored and evaluated, and the photometric
            // cost is a function of (pixel, plane, view, window scale, images) alone, so S.own holds the bits ncc_cost would return.
            // Same views, same ascending order, same sums; the loads sit outside every per-lane branch and travel together.
            const int idx_c = pinned_here(idx);
            const size_t wh = (size_t)W * Hh;
            if constexpr (GEOM) {
                // one view ahead: the stored cost and the depth gather of view v + 1 travel while the check of view v is finished
                float w_n = view_w[0], c_n = S.own[idx_c];
                GeomCheck gc_n{};
                if (w_n > 0.0f) gc_n.issue(P.views[0], gz, x, y);
                for (int v = 0; v < V; ++v) {
                    const float w = w_n, c = c_n;
                    const GeomCheck gc = gc_n;
                    if (v + 1 < V) {
                        w_n = view_w[v + 1];
                        c_n = (S.own + (v + 1) * wh)[idx_c];
                        if (w_n > 0.0f) gc_n.issue(P.views[v + 1], gz, x, y);
                    }
                    if (!(w > 0.0f)) continue;
                    const float gt = 0.2f * gc.finish(P.views[v], x, y);
                    tc += w * (c + gt);
                    tg += w * gt;
                }
            } else {
                float oc[MAXV];  // (views beyond V repeat the last one: a load, no branch)
#pragma unroll
                for (int v = 0; v < MAXV; ++v) oc[v] = (S.own + (v < V ? v : V - 1) * wh)[idx_c];
#pragma unroll
                for (int v = 0; v < MAXV; ++v) {
                    if (v >= V) break;
                    const float w = view_w[v];
                    if (!(w > 0.0f)) continue;
                    tc += w * oc[v];
                }
            }
        } else {
            float m0, m1, m2;
            plane_to_m(P, pl, m0, m1, m2);
            float w_next = view_w[0];  // one view ahead: hides the latency of private memory
            for (int v = 0; v < V; ++v) {
                const float w = w_next;
                w_next = view_w[v + 1 < MAXV ? v + 1 : v];
                if (!(w > 0.0f)) continue;
                GeomCheck gc;
                if (GEOM) gc.issue(P.views[v], gz, x, y);  // the depth gather travels behind the NCC evaluation
                const float c = ncc_cost<U8, SCALE, kDeep, NT>(P.views[v], rw, x, y, m0, m1, m2);
                if (GEOM) {
                    const float gt = 0.2f * gc.finish(P.views[v], x, y);
                    tc += w * (c + gt);
                    tg += w * gt;
                } else {
                    tc += w * c;
                }
            }
        }
        cost_now = tc / weight_norm;
        if (GEOM) geom_now = tg / weight_norm;
    }
    stamp(kStampCurrent);
    {
    // ---- acceptance of the best propagated neighbour (ref .cu:921-991)
    const float4 cur = plane_now;  // still the plane the pixel came in with
    depth_now = depth_from_plane(P, cur, x, y);
    const int idx_a = pinned_here(idx);
    if (PRIOR) pp = S.prior[idx_a];
    masked = PRIOR && S.mask[idx_a] > 0;
    if (PRIOR && !GEOM) {
        depth_prior = depth_from_plane(P, pp, x, y);
        if (masked) {
            float rfc[8];
            for (int i = 0; i < 8; ++i) {
                rfc[i] = 0.0f;
                if ((flags >> i) & 1u) {
                    const float4 cpl = S.planes[pinned_here(pos[i])];
                    const float di = depth_from_plane(P, cpl, x, y);
                    const float ac = (pp.x * cpl.x + pp.y * cpl.y) + pp.z * cpl.z;
                    const float pr = prior_term<kPriorCall>(di - depth_prior, ac, two_ds2, two_as2);
                    const float fci = final_costs[i];
                    rfc[i] = d_exp(-fci * fci / beta) * pr;
                }
            }
            int max_idx = 0;
            float mc = rfc[0];
            for (int i = 1; i < 8; ++i)
                if (rfc[i] >= mc) {
                    mc = rfc[i];
                    max_idx = i;
                }
            const float ac = (pp.x * cur.x + pp.y * cur.y) + pp.z * cur.z;
            const float pr = prior_term<kPriorCall>(depth_now - depth_prior, ac, two_ds2, two_as2);
            const float rc_now = d_exp(-cost_now * cost_now / beta) * pr;
            if ((flags >> max_idx) & 1u) {
                const float4 cpl = S.planes[pinned_here(pos[max_idx])];
                const float db = depth_from_plane(P, cpl, x, y);
                if (db >= a.depth_min && db <= a.depth_max && rfc[max_idx] > rc_now) {
                    // ref .cu:950/961: the shadowed depth_now keeps the old plane's depth
                    plane_now = cpl;
                    restricted_cost = rfc[max_idx];
                    st_u32_wt(&S.sel[idx_a], temp_sel);
                }
            }
        } else if ((flags >> min_idx) & 1u) {
            const float4 cpl = S.planes[pinned_here(pos[min_idx])];
            const float db = depth_from_plane(P, cpl, x, y);
            if (db >= a.depth_min && db <= a.depth_max && final_costs[min_idx] < cost_now) {
                depth_now = db;
                plane_now = cpl;
            }
        }
    }
    if (!PRIOR && ((flags >> min_idx) & 1u)) {
        const float4 cpl = S.planes[pinned_here(pos[min_idx])];
        const float db = depth_from_plane(P, cpl, x, y);
        if (db >= a.depth_min && db <= a.depth_max && final_costs[min_idx] < cost_now) {
            depth_now = db;
            plane_now = cpl;
            cost_now = final_costs[min_idx];
            st_u32_wt(&S.sel[idx_a], temp_sel);
        }
    }
    // ---- refinement candidates (ref .cu:644-675)
    const float perturbation = 0.02f;
    float depth_rand;
    float4 n_rand;
    if (masked) {
        // ref .cu:651-660: the prior-guided draw is overwritten below (missing else), its random numbers are still consumed
        depth_prior = depth_from_plane(P, pp, x, y);
        depth_rand = (rng_uniform(g) * 6.0f) * depth_sigma + (depth_prior - 3.0f * depth_sigma);
        n_rand = perturbed_normal(P, x, y, pp, g, angle_sigma);
    }
    depth_rand = rng_uniform(g) * (a.depth_max - a.depth_min) + a.depth_min;
    n_rand = random_normal(P, x, y, g);
    const float dmin_p = (1.0f - perturbation) * depth_now;
    const float dmax_p = (1.0f + perturbation) * depth_now;
    const float depth_pert = rng_uniform(g) * (dmax_p - dmin_p) + dmin_p;
    const float4 n_pert = perturbed_normal(P, x, y, plane_now, g, 0.06283185f);
    park_n[0] = plane_now.x, park_n[1] = plane_now.y, park_n[2] = plane_now.z;
    park_n[3] = n_rand.x, park_n[4] = n_rand.y, park_n[5] = n_rand.z;
    park_n[6] = n_pert.x, park_n[7] = n_pert.y, park_n[8] = n_pert.z;
    park_d[0] = depth_now, park_d[1] = depth_rand, park_d[2] = depth_pert;
    }
    // candidates: (d_rand,n) (d,n_rand) (d_rand,n_rand) (d,n_pert) (d_pert,n)   ref .cu:674-675.
    //
    // Their evaluations do not depend on each other (only the acceptance below is sequential) and MOST OF THEM CANNOT WIN:
    //   * a candidate whose depth lies outside [depth_min, depth_max] is never accepted (ref .cu:700,713);
    //   * outside the masked-prior branch a candidate is accepted only if sum_v w_v (c_v [+ g_v]) / weight_norm < cost_now
    //     (ref .cu:696,713).  Every term is >= 0, fp32 addition of non-negative terms and the division by the positive norm
    //     are monotone, and cost_now only decreases from one candidate to the next: once a candidate's running sum has reached
    //     T >= cost_now * weight_norm (exact product, rounded UP) with the cost_now the refinement started with, its quotient
    //     is >= that cost_now whatever the remaining views add -- they are dead work the reference performs (:681) and nothing
    //     reads.  (Measured with the oracle's statistics hook, tests/analysis/prune_stats.py: 45 % of a lane's refinement evaluations.)
    // A lane cannot profit from its own dead evaluations while other lanes of the wave are still live, so the live (pixel,
    // candidate) pairs of a view are DEALT TO THE LANES OF THE WAVE through LDS: every lane publishes the planes of its live
    // candidates at consecutive slots (ballot + mbcnt), lane j evaluates item j of the round for whoever owns it -- with the
    // owner's pixel, weight records and window statistics -- and the owner collects the costs in ascending view order, exactly
    // the sums of the uncompacted loop.  38 -> 25 evaluation rounds per wave and update on the cfg-1 scene.
    //   * a masked prior pixel accepts a candidate when exp(-tc^2 / beta) * prior_term > restricted_cost (ref .cu:707), and
    //     restricted_cost is 0 unless a neighbour was accepted above (a reference quirk, SURVEY a-10 iv).  With 0 on the right the
    //     test does not depend on the cost at all: tc lies in [0, 2], so the exponential is a positive normal number, and the
    //     prior term is either >= 0.5 or NaN (acos of a dot product beyond 1).  Every in-range candidate with a valid prior
    //     term is therefore accepted in turn, each overwriting the one before: only the LAST of them leaves a trace, the
    //     evaluations of all the others are dead.
    float cpl[5 * 4], tcs[5], tgs[5], pr5[5];
    // the candidate planes: in registers where the variant has them (kPlanesInRegs, above; every index below is a compile-time
    // constant of an unrolled loop), parked in private memory where registers would push other state out (profiles/EXPERIMENTS.md 69)
    if constexpr (!kPlanesInRegs) keep_in_memory(cpl);
    uint32_t dead = 0;
#pragma unroll
    for (int ci = 0; ci < 5; ++ci) {
        const int ni = 3 * ((ci == 1 || ci == 2) ? 1 : (ci == 3 ? 2 : 0));
        const float cd = park_d[(ci == 0 || ci == 2) ? 1 : (ci == 4 ? 2 : 0)];
        float4 pl;
        pl.x = park_n[ni], pl.y = park_n[ni + 1], pl.z = park_n[ni + 2];
        pl.w = plane_offset(P, x, y, cd, pl);
        cpl[4 * ci] = pl.x, cpl[4 * ci + 1] = pl.y, cpl[4 * ci + 2] = pl.z, cpl[4 * ci + 3] = pl.w;
        const float db = depth_from_plane(P, pl, x, y);
        if (!(db >= a.depth_min && db <= a.depth_max)) dead |= 1u << ci;
        tcs[ci] = 0.0f;
        tgs[ci] = 0.0f;
        pr5[ci] = 0.0f;
        if (PRIOR && masked) {
            const float ac = (pp.x * pl.x + pp.y * pl.y) + pp.z * pl.z;
            pr5[ci] = prior_term<kPriorCall>(cd - depth_prior, ac, two_ds2, two_as2);
        }
    }
    if (PRIOR && masked) {
        if (restricted_cost == 0.0f) {
            int last = -1;
#pragma unroll
            for (int ci = 0; ci < 5; ++ci)
                if (!((dead >> ci) & 1u) && pr5[ci] > 0.0f) last = ci;  // NaN > 0 is false
            dead = last >= 0 ? (31u & ~(1u << last)) : 31u;
        } else {
            //   * ... and where a neighbour's acceptance has raised restricted_cost, a candidate whose prior term alone is not
            //     above it cannot pass either: exp(-tc^2 / beta) <= 1 up to the 2 ulp of d_exp, so the product stays below
            //     prior_term * (1 + 3e-7) < fl(prior_term * 1.000001) <= restricted_cost whatever tc turns out to be (a NaN
            //     prior term fails the reference's test as it fails this one).  71-76 % of the candidates of a masked pixel
            //     (tests/analysis/prune_stats.py --prior): random depths and normals sit far from the prior plane.
#pragma unroll
            for (int ci = 0; ci < 5; ++ci)
                if (!(pr5[ci] * 1.000001f > restricted_cost)) dead |= 1u << ci;
        }
    }
    // T: the exact product cost_now * weight_norm rounded up (the fp32 product is within half an ulp of it; one ulp more is
    // above it; both factors are finite and >= 0).  Masked prior pixels accept on another criterion (ref .cu:707): no threshold.
    const float T = masked ? __uint_as_float(0x7f800000u) : __uint_as_float(__float_as_uint(cost_now * weight_norm) + 1u);
    {
        constexpr int kLanesPerRow = 64 / kWaveRows;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        char* const xw = reinterpret_cast<char*>(pm_lds + kLdsWeightFloatsOf<NT>) + wv * kXchgBytesPerWave;
        float4* const x_rec = reinterpret_cast<float4*>(xw);                           // [64] plane of the item
        float2* const x_res = reinterpret_cast<float2*>(xw + 1024);                    // [64] (photometric cost, geometric term)
        unsigned short* const x_id = reinterpret_cast<unsigned short*>(xw + 1536);     // [64] owner lane
        const int wave_y = y0 + wv * kWaveRows;
        const int wave_x = x0;
        // lanes without a pixel (image border) have left the kernel: the items of a round go to the lanes that are still here,
        // the r-th of them taking slot r
        const unsigned long long here = __ballot(1);
        const int n_here = __builtin_popcountll(here);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(here >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)here, 0u));
        float w_next = view_w[0];
        stamp(kStampDealBegin);
        for (int v = 0; v < V; ++v) {
            const float w = w_next;
            w_next = view_w[v + 1 < MAXV ? v + 1 : v];
            const uint32_t live = (w > 0.0f) ? (~dead & 31u) : 0u;
            int pos[5], total = 0;
#pragma unroll
            for (int ci = 0; ci < 5; ++ci) {
                const unsigned long long b = __ballot((live >> ci) & 1u);
                pos[ci] = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                total += __builtin_popcountll(b);
            }
            for (int base = 0; base < total; base += n_here) {
                // owners publish the items of this round
                stamp(kStampRound);
#pragma unroll
                for (int ci = 0; ci < 5; ++ci)
                    if (((live >> ci) & 1u) && (unsigned)(pos[ci] - base) < (unsigned)n_here) {
                        const int slot = pos[ci] - base;
                        x_rec[slot] = make_float4(cpl[4 * ci], cpl[4 * ci + 1], cpl[4 * ci + 2], cpl[4 * ci + 3]);
                        x_id[slot] = (unsigned short)lane;
                    }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                stamp(kStampPublished);
                // the lane of rank r evaluates item base + r with its owner's pixel, weight records and window statistics
                const bool have = base + rank < total;
                const int owner = have ? (int)x_id[rank] : lane;
                const float4 ipl = x_rec[rank];
                RefWin orw;
                orw.lw = reinterpret_cast<const float4*>(pm_lds) + ((threadIdx.x & ~63u) + owner);
                orw.inv_w = __int_as_float(__builtin_amdgcn_ds_bpermute(owner << 2, __float_as_int(rw.inv_w)));
                orw.mean_r = __int_as_float(__builtin_amdgcn_ds_bpermute(owner << 2, __float_as_int(rw.mean_r)));
                orw.var_r = __int_as_float(__builtin_amdgcn_ds_bpermute(owner << 2, __float_as_int(rw.var_r)));
                if (have) {
                    const int oy = wave_y + owner / kLanesPerRow;
                    const int ox = wave_x + 2 * (owner % kLanesPerRow) + ((oy + parity) & 1);
                    float m0, m1, m2;
                    plane_to_m(P, ipl, m0, m1, m2);
                    GeomCheck gc;
                    if (GEOM) gc.issue(P.views[v], depth_from_plane(P, ipl, ox, oy), ox, oy);
                    const float c = ncc_cost<U8, SCALE, kDeep, NT>(P.views[v], orw, ox, oy, m0, m1, m2);
                    float gt = 0.0f;
                    if (GEOM) gt = 0.2f * gc.finish(P.views[v], ox, oy);
                    x_res[rank] = make_float2(c, gt);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                stamp(kStampEvaluated);
                // owners collect: for a fixed candidate the views are still added in ascending order
#pragma unroll
                for (int ci = 0; ci < 5; ++ci)
                    if (((live >> ci) & 1u) && (unsigned)(pos[ci] - base) < (unsigned)n_here) {
                        const float2 r = x_res[pos[ci] - base];
                        if (GEOM) {
                            tcs[ci] += w * (r.x + r.y);
                            tgs[ci] += view_w[ci] * r.y;  // the candidate index used as view index, ref .cu:689
                        } else {
                            tcs[ci] += w * r.x;
                        }
                        if (tcs[ci] >= T) dead |= 1u << ci;
                    }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                stamp(kStampCollected);
            }
        }
        stamp(kStampDealEnd);
    }
#pragma unroll
    for (int ci = 0; ci < 5; ++ci) {
        if ((dead >> ci) & 1u) continue;  // out of range, or provably not below cost_now: the reference's tests below are false
        float4 pl;
        pl.x = cpl[4 * ci], pl.y = cpl[4 * ci + 1], pl.z = cpl[4 * ci + 2], pl.w = cpl[4 * ci + 3];
        const float tc = tcs[ci] / weight_norm;
        const float tg = GEOM ? tgs[ci] / weight_norm : 0.0f;
        if (masked) {
            const float rtc = d_exp(-tc * tc / beta) * pr5[ci];
            if (rtc > restricted_cost) {
                plane_now = pl;
                cost_now = tc;
            }
        } else if (tc < cost_now) {
            plane_now = pl;
            cost_now = tc;
            geom_now = tg;
        }
    }
    const int idx_o = pinned_here(idx);
    st_f32_wt(&S.costs[idx_o], cost_now);
    st_f32x4_wt(&S.planes[idx_o], plane_now);
    if (GEOM) st_f32_wt(&S.geom[idx_o], geom_now);
}

// ---------------------------------------------------------------------------
// The update LAUNCH: several passes (black, red, black, ...) of one window scale in ONE launch (round 5).
//
// Launched one pass at a time, every pass ends in a tail: once its last block has started, wave slots run empty while the
// slowest blocks finish -- 7.5-9 % of the slot-time of a 1600x1200 launch (profiles/r05_wave_timeline.txt; a wave lives ~300 us,
// 1/8 of the launch).  But a block of pass p + 1 needs only the blocks of pass p within the reach of the candidate search (23 px,
// kDirs).  Here the grid holds one block per work item (pass, position) of ALL passes; a block takes a ticket -- items are numbered
// pass-major, positions in raster order --, waits until the positions around its own have completed the pass before, runs the
// update and signals.  The tail of pass p fills with the head of pass p + 1; only the last pass of the launch has one.
// Correctness does not depend on placement or dispatch order:
//   * tickets: a block that holds ticket t knows that every ticket < t is held by a block that has STARTED, so whatever it waits
//     for is running or done -- no deadlock however the hardware orders the blocks, also not between two such launches sharing
//     the GPU (each waits only for its own started blocks).  Every wait is bounded all the same: after kSpinLimit polls a block
//     raises the launch's error word, which ends all waits, and the host reports -101;
//   * hand-over (MI355X_MICROARCH.md, "inter-workgroup visibility"): results leave through write-through stores (sc0 sc1); each
//     wave waits for its stores (s_waitcnt vmcnt(0)) and then adds 1 to its position's completion counter (agent-scope atomic);
//     the consumer polls the counters of the positions in reach with relaxed sc1 loads, then ONE agent-scope acquire
//     (invalidates the CU's L1), waits for it, and a workgroup barrier stands between that and every load of the block;
//   * read-after-write and write-after-read are the same condition: the item (p + 1, B) overwrites pixels of its colour that the
//     items (p, around B) read (as candidates) until they END -- it waits for exactly those.
// Order: plain raster order, every pass alike, so what a block waits for was handed out a whole pass earlier: blocks wait 1.5 us
// on average.  (The XCD bands of the single-pass launches -- xcd_remap -- cost 2 % here, 2.47 against 2.42 ms per pass: with a
// band bound to an XCD the slowest band paces the round-robin dispatch, and the L2 locality the bands bought in round 1 no longer
// shows since the view-major order of round 2.  Persistent blocks that loop over tickets fill 99 % of the wave slots instead of
// 96 % and are no faster, 2.46 ms with the registers the loop costs: the last slots add contention, not throughput.)
// The sync words live in global memory: [0] ticket, [1] waves that have left the kernel, [2] error, [16 + b] waves that have
// completed position b (monotonic over the passes).  The last wave to leave zeroes them for the next launch.
//
// Band counters (the banded end of Run(), mpmvs_api.hip enqueue_band_tail): in the LAST pass of the last update launch of a
// Run() every wave also adds 1 to the counter of the row band that holds its 8 rows, right after its completion signal.  The
// rows of band k are final once its counter has reached band_run x (waves of the last pass in band k): the host's finishing
// stream waits for that (hipStreamWaitValue32) and then runs GetDepthandNormal, the median filter and the copies of the band
// while the pass still works further down the image.  The counters live in their own buffer and are never reset while a wait may
// be armed: band_run counts the banded Run()s of the context, so the targets only grow.  A block that gives up waiting (kSpinLimit,
// the error word) first lifts every counter to its target, so that no wait of the finishing stream outlives the launch.
// ---------------------------------------------------------------------------
struct ChainArgs {
    int n_pass;    // passes in this launch; pass k has colour (a.parity + k) & 1, launch id a.launch + k, iteration a.iter + (a.parity + k) / 2
    int nb;        // block positions per pass, nbx per row, nby rows
    int nbx, nby;
    float thr[8];  // view-selection threshold (ref .cu:832) of the iterations a.iter, a.iter + 1, ...
    int* sync;
    int spin_limit;  // polls after which a waiting block gives up (kSpinLimit unless a test shortens it)
    int stall_pos;   // fault injection (mpmvs_dbg_chain_stall): the block at this position never signals its first pass; -1 = off
    unsigned* band;       // band counters, or nullptr: no band signals from this launch
    int band_groups;      // 8-row groups (kWaveRows) per band
    int n_groups;         // 8-row groups of the rows the launch updates: group g counts toward band g / band_groups
    unsigned band_run;    // the banded Run() this launch ends (1, 2, ...): band k's target is band_run x nbx x (groups of band k)
    // bit c: the FIRST pass of colour c in this launch (pass 0 or 1) reads its current planes' per-view costs from S.own (update_body);
    // set by the host for the passes that follow InitializeScore at its window scale with no writer of the planes in between
    int own_mask;
};
constexpr int kChainMaxIters = 8;
constexpr int kSyncHeader = 16;
constexpr int kSpinLimit = 1 << 20;   // polls of ~1-2 us each: seconds, three orders of magnitude above any legitimate wait

// The hand-over above is written for the memory system of gfx942 / gfx950 (write-through stores reach memory, an agent-scope acquire
// invalidates what the CU may hold of it): refuse to build it for anything else.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "the chained update launch (k_update) relies on gfx942 / gfx950 cache behaviour: see the comment above"
#endif
// memory order of the completion signal: RELAXED.  The write-through stores and the wave's own s_waitcnt vmcnt(0) have put the
// results in memory before the counter moves.  The memory model's own release adds an L2 write-back before every signal, which also
// flushes the wave's dirty scratch lines: +5.9 % per pass, same bits (round 6, profiles/EXPERIMENTS.md 47).
template <bool GEOM, bool PRIOR, int MAXV, bool U8, int SCALE>
__global__ __launch_bounds__((kUpdThreads<U8, SCALE>), kWavesPerSimd) void k_update(const ProblemDev* __restrict__ Pp, StateDev S, LaunchArgs a, ChainArgs ch) {
    const ProblemDev& P = *Pp;
    constexpr int NT = kUpdThreads<U8, SCALE>, BW = kChkBlockW, BH = kChkBlockH<NT>, kWaves = NT / 64;
    static_assert(NT % 64 == 0 && NT >= 64 && NT <= 256, "update blocks are 1 .. 4 waves");
    constexpr int RX = (23 + BW - 1) / BW, RY = (23 + BH - 1) / BH, NN = (2 * RX + 1) * (2 * RY + 1);  // positions within the 23 px of kDirs
    static_assert(NN <= 64, "one lane polls one neighbour");
#ifdef PM_DBG_WAVETIME
    WaveTimer wave_timer;
#endif
    // The ticket.  A four-wave block passes it on through two spare words of wave 0's exchange area (the tile / exchange region is not
    // in use yet: this barrier and the one behind the wait fence the hand-over); a one-wave block has it in its own registers.
    int pass, b;
    {
        int t = 0;
        if (threadIdx.x == 0) t = __hip_atomic_fetch_add(&ch.sync[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (kWaves > 1) {
            int* const bcast = reinterpret_cast<int*>(reinterpret_cast<char*>(pm_lds + kLdsWeightFloatsOf<NT>) + 1664);
            if (threadIdx.x == 0) bcast[0] = t;
            __syncthreads();
            t = bcast[0];
        }
        t = __builtin_amdgcn_readfirstlane(t);
        pass = t / ch.nb;
        b = t - pass * ch.nb;
    }
    // What the block waits for, called by update_body ahead of its loads: the positions around its own have completed the pass before.  Wave 0 polls, acquires and waits for the acquire; update_body's barrier comes next.
    const auto wait_for_neighbours = [&]() {
        if (threadIdx.x < 64 && pass > 0) {
            const int by = b / ch.nbx, bx = b - by * ch.nbx;
            int nbid = -1;
            if ((int)threadIdx.x < NN) {
                const int x = bx + (int)threadIdx.x % (2 * RX + 1) - RX, y = by + (int)threadIdx.x / (2 * RX + 1) - RY;
                if (x >= 0 && x < ch.nbx && y >= 0 && y < ch.nby) nbid = y * ch.nbx + x;
            }
            const int need = pass * kWaves;
            for (int spins = 0;; ++spins) {
                int d = need;
                if (nbid >= 0) d = __hip_atomic_load(&ch.sync[kSyncHeader + nbid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all(d >= need)) break;
                __builtin_amdgcn_s_sleep(8);
                if ((spins & 255) == 255) {
                    const bool give_up = spins >= ch.spin_limit || __hip_atomic_load(&ch.sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                    if (__builtin_amdgcn_readfirstlane((int)give_up)) {
                        if (threadIdx.x == 0) __hip_atomic_store(&ch.sync[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (ch.band) {   // release every wait of the finishing stream: this Run() is lost (-101) anyway
                            const int n_bands = (ch.n_groups + ch.band_groups - 1) / ch.band_groups;
                            for (int k = threadIdx.x; k < n_bands; k += 64) {
                                const int groups = min(ch.n_groups, (k + 1) * ch.band_groups) - k * ch.band_groups;
                                __hip_atomic_fetch_max(&ch.band[k], ch.band_run * (unsigned)(ch.nbx * groups), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                        break;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
#ifdef PM_DBG_WAVETIME
        wave_timer.ready();
#endif
    };
    const auto stamp = [&](int point) {
#ifdef PM_DBG_WAVETIME
        wave_timer.stamp(point);
#endif
    };
    {
        const int k = a.parity + pass;
        const bool use_own = pass < 2 && ((ch.own_mask >> (k & 1)) & 1) != 0;
        update_body<GEOM, PRIOR, MAXV, U8, SCALE>(P, S, a, b, k & 1, a.launch + (uint32_t)pass, ch.thr[(k >> 1) < kChainMaxIters ? (k >> 1) : 0], use_own, wait_for_neighbours, stamp);
    }
    // completion: this wave's stores have left (write-through) before it counts itself done
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef PM_DBG_WAVETIME
    wave_timer.finish(S.wavetime, a.launch + (uint32_t)pass, b, ch.nb);
#endif
    int fin = 0;
    if ((threadIdx.x & 63) == 0) {
        if (!(b == ch.stall_pos && pass == 0))   // (fault injection: a position that never completes its first pass)
            __hip_atomic_fetch_add(&ch.sync[kSyncHeader + b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ch.band && pass == ch.n_pass - 1) {   // the last pass: this wave's 8 rows of the image are final
            const int g = (b / ch.nbx) * kWaves + (int)(threadIdx.x >> 6);
            if (g < ch.n_groups) __hip_atomic_fetch_add(&ch.band[g / ch.band_groups], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        fin = __hip_atomic_fetch_add(&ch.sync[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    fin = __builtin_amdgcn_readfirstlane(fin);
    if (fin == (int)gridDim.x * kWaves - 1) {
        // the last wave of the launch: nobody polls any more; leave the words zeroed for the next launch (the error word stays)
        for (int i = threadIdx.x & 63; i < ch.nb; i += 64) ch.sync[kSyncHeader + i] = 0;
        if ((threadIdx.x & 63) == 0) {
            ch.sync[0] = 0;
            ch.sync[1] = 0;
        }
    }
}

// ---------------------------------------------------------------------------
// GetDepthandNormal, ref .cu:1021-1034
// ---------------------------------------------------------------------------
// by0: first block row (16 rows) of the launch -- the banded end of Run() launches it per band of rows, same arithmetic
__global__ __launch_bounds__(256) void k_depth_normal(const ProblemDev* __restrict__ Pp, StateDev S, int by0) {
    const ProblemDev& P = *Pp;
    int x, y, x0, y0;
    if (!dense_pixel(P, x, y, x0, y0, by0)) return;
    const int idx = y * P.W + x;
    float4 pl = S.planes[idx];
    pl.w = depth_from_plane(P, pl, x, y);
    float4 o;
    o.x = (P.cam.R[0] * pl.x + P.cam.R[3] * pl.y) + P.cam.R[6] * pl.z;
    o.y = (P.cam.R[1] * pl.x + P.cam.R[4] * pl.y) + P.cam.R[7] * pl.z;
    o.z = (P.cam.R[2] * pl.x + P.cam.R[5] * pl.y) + P.cam.R[8] * pl.z;
    o.w = pl.w;
    S.planes[idx] = o;
    S.depth[idx] = pl.w;  // the filter's dense depth plane
}

// ---------------------------------------------------------------------------
// Black/RedPixelFilter = CheckerboardFilter, ref .cu:1036-1174
// ---------------------------------------------------------------------------
// Median of 21 by min / max elimination in registers: of 12 values the smallest and the largest cannot be the median of all
// 21, they go and the next value comes in; after nine such rounds three values are left and their middle one is the median.
// All indices are compile-time constants (the array lives in registers); every step is a compare-exchange that keeps the
// multiset intact.  Valid for values that are totally ordered by `<` (finite, one sign of zero): the caller checks.
template <int K>
PM_DEV void min_to_front_max_to_back(float (&v)[21]) {
    constexpr int half = K / 2;
#pragma unroll
    for (int i = 0; i < half; ++i) {  // lows into the front half, highs into the back half
        const float a = v[i], b = v[K - 1 - i];
        v[i] = __builtin_fminf(a, b);
        v[K - 1 - i] = __builtin_fmaxf(a, b);
    }
    constexpr int front_end = (K + 1) / 2;  // the middle value of an odd K may be the minimum as well as the maximum
#pragma unroll
    for (int i = 1; i < front_end; ++i) {
        const float a = v[0], b = v[i];
        v[0] = __builtin_fminf(a, b);
        v[i] = __builtin_fmaxf(a, b);
    }
#pragma unroll
    for (int i = half; i < K - 1; ++i) {
        const float a = v[i], b = v[K - 1];
        v[i] = __builtin_fminf(a, b);
        v[K - 1] = __builtin_fmaxf(a, b);
    }
}
template <int K>
PM_DEV float median21_rounds(float (&v)[21], float& lowest) {
    min_to_front_max_to_back<K>(v);
    lowest = __builtin_fminf(lowest, v[0]);
    if constexpr (K == 3) {
        return v[1];
    } else {
        // drop v[0] and v[K-1]: the next unseen value (index 12 + (12 - K)) replaces v[0], the value before the maximum closes the gap
        v[0] = v[12 + (12 - K)];
        return median21_rounds<K - 1>(v, lowest);
    }
}

// The depths are gathered from the dense plane S.depth (written by k_depth_normal, kept in step with planes[].w here): 4 bytes
// per tap instead of the .w of a 16-byte float4 (4 x over-fetch; 84 -> 40 us per launch).  Every tap has the other colour, so
// the in-place update of one colour is race free in both arrays.
// b0: block position of the launch's first block (a band of block rows in the banded end of Run(); 0 for the whole image).
// At most 64 VGPRs (8 waves per SIMD; 72 unbounded): the banded end of Run() launches the filter while the last update pass holds
// two waves of 224 VGPRs on every SIMD, and only 64 of a SIMD's 512 are left beside them -- at 72 a band's filter waited for the
// update's last block (1.5 ms).
__global__ __launch_bounds__(256, 8) void k_filter(const ProblemDev* __restrict__ Pp, StateDev S, LaunchArgs a, int b0) {
    const ProblemDev& P = *Pp;
    int x, y, x0, y0;
    if (!checker_pixel(P, a, b0 + xcd_remap(blockIdx.x, gridDim.x), a.parity, x, y, x0, y0)) return;
    const int W = P.W, Hh = P.H;
    const int ctr = y * W + x;
    if (S.costs[ctr] < 0.001f) return;
    if (x > 4 && x < W - 5 && y > 4 && y < Hh - 5) {
        // interior pixel: all 21 values exist (the order of the taps below is the reference's, it does not matter for a median)
        float v[21];
        constexpr int dx[21] = {0, 0, 0, 0, 0, 0, 0, -1, -3, -5, 1, 3, 5, 2, 2, -2, -2, -1, 1, -1, 1};
        constexpr int dy[21] = {0, -1, -3, -5, 1, 3, 5, 0, 0, 0, 0, 0, 0, -1, 1, -1, 1, -2, -2, 2, 2};
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 21; ++i) {
            v[i] = S.depth[ctr + dy[i] * W + dx[i]];
            sum += v[i];
        }
        float lowest = v[0];
        const float med = median21_rounds<12>(v, lowest);
        // `<` orders finite positive depths totally, so the selection above found what the insertion sort below finds; anything
        // else (a NaN or infinite depth shows in the sum, a zero or negative one in the minimum) takes the general path
        if (lowest > 0.0f && sum < 3.0e38f) {
            S.planes[ctr].w = med;
            S.depth[ctr] = med;
            return;
        }
    }
    // Border pixels (a tap is missing): the reference's 20 bounds tests, but every depth is loaded UNCONDITIONALLY at the position
    // clamped into the image -- loaded under its test, each tap was its own branch with its own memory round trip, and the
    // image-border waves (the last blocks of the launch) set the duration of the whole launch.  Missing taps count as +inf; an
    // odd-even transposition sort in registers puts the n valid depths first; the median is picked by n.  Valid for finite positive
    // depths (totally ordered by `<`); anything else falls through to the reference's insertion sort below.
    {
        constexpr int dx[21] = {0, 0, 0, 0, 0, 0, 0, -1, -3, -5, 1, 3, 5, 2, 2, -2, -2, -1, 1, -1, 1};
        constexpr int dy[21] = {0, -1, -3, -5, 1, 3, 5, 0, 0, 0, 0, 0, 0, -1, 1, -1, 1, -2, -2, 2, 2};
        const bool ok[21] = {true,        y > 0,      y > 2,       y > 4,       y < Hh - 1,  y < Hh - 3,  y < Hh - 5,
                             x > 0,       x > 2,      x > 4,       x < W - 1,   x < W - 3,   x < W - 5,
                             y > 0 && x < W - 2,      y < Hh - 1 && x < W - 2,  y > 0 && x > 1,           y < Hh - 1 && x > 1,
                             x > 0 && y > 2,          x < W - 1 && y > 2,       x > 0 && y < Hh - 2,      x < W - 1 && y < Hh - 2};
        float v[21];
        float lowest = 3.0e38f, sum = 0.0f;
        int n = 0;
#pragma unroll
        for (int i = 0; i < 21; ++i) {
            const int cx = x + dx[i] < 0 ? 0 : (x + dx[i] > W - 1 ? W - 1 : x + dx[i]);
            const int cy = y + dy[i] < 0 ? 0 : (y + dy[i] > Hh - 1 ? Hh - 1 : y + dy[i]);
            const float d = S.depth[cy * W + cx];
            v[i] = ok[i] ? d : __uint_as_float(0x7f800000u);
            if (ok[i]) {
                lowest = __builtin_fminf(lowest, d);
                sum += d;
                n++;
            }
        }
        if (lowest > 0.0f && sum < 3.0e38f) {
#pragma unroll
            for (int pass = 0; pass < 21; ++pass)
#pragma unroll
                for (int i = pass & 1; i + 1 < 21; i += 2) {
                    const float a = v[i], b = v[i + 1];
                    v[i] = __builtin_fminf(a, b);
                    v[i + 1] = __builtin_fmaxf(a, b);
                }
            const int mid = n / 2;
            float lo = 0.0f, hi = 0.0f;
#pragma unroll
            for (int i = 0; i < 21; ++i) {
                lo = (i == mid - 1) ? v[i] : lo;
                hi = (i == mid) ? v[i] : hi;
            }
            const float med = (n % 2 == 0) ? (lo + hi) / 2.0f : hi;
            S.planes[ctr].w = med;
            S.depth[ctr] = med;
            return;
        }
    }
    float f[21];
    int n = 0;
#define PM_TAP(cond, off) \
    if (cond) f[n++] = S.depth[ctr + (off)];
    f[n++] = S.depth[ctr];
    PM_TAP(y > 0, -W)
    PM_TAP(y > 2, -3 * W)
    PM_TAP(y > 4, -5 * W)
    PM_TAP(y < Hh - 1, W)
    PM_TAP(y < Hh - 3, 3 * W)
    PM_TAP(y < Hh - 5, 5 * W)
    PM_TAP(x > 0, -1)
    PM_TAP(x > 2, -3)
    PM_TAP(x > 4, -5)
    PM_TAP(x < W - 1, 1)
    PM_TAP(x < W - 3, 3)
    PM_TAP(x < W - 5, 5)
    PM_TAP(y > 0 && x < W - 2, -W + 2)
    PM_TAP(y < Hh - 1 && x < W - 2, W + 2)
    PM_TAP(y > 0 && x > 1, -W - 2)
    PM_TAP(y < Hh - 1 && x > 1, W - 2)
    PM_TAP(x > 0 && y > 2, -1 - 2 * W)
    PM_TAP(x < W - 1 && y > 2, 1 - 2 * W)
    PM_TAP(x > 0 && y < Hh - 2, -1 + 2 * W)
    PM_TAP(x < W - 1 && y < Hh - 2, 1 + 2 * W)
#undef PM_TAP
    for (int i = 1; i < n; ++i) {
        const float tmp = f[i];
        int j = i;
        for (; j >= 1 && tmp < f[j - 1]; --j) f[j] = f[j - 1];
        f[j] = tmp;
    }
    const int mid = n / 2;
    const float med = (n % 2 == 0) ? (f[mid - 1] + f[mid]) / 2.0f : f[mid];
    S.planes[ctr].w = med;
    S.depth[ctr] = med;
}

// ---------------------------------------------------------------------------
// data-movement helpers and probes
// ---------------------------------------------------------------------------
// replicate-pad a dense W x H image into a (W+2A) x (H+2A) one
__global__ void k_pad(const float* __restrict__ src, int w, int h, float* __restrict__ dst, int apron) {
    const int pw = w + 2 * apron, ph = h + 2 * apron;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pw || y >= ph) return;
    int sx = x - apron, sy = y - apron;
    sx = sx < 0 ? 0 : (sx > w - 1 ? w - 1 : sx);
    sy = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
    dst[(long)y * pw + x] = src[(long)sy * w + sx];
}

// the same from an 8-bit image (an 8-bit exact reference image travels as bytes)
__global__ void k_pad_u8(const unsigned char* __restrict__ src, int w, int h, float* __restrict__ dst, int apron) {
    const int pw = w + 2 * apron, ph = h + 2 * apron;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pw || y >= ph) return;
    int sx = x - apron, sy = y - apron;
    sx = sx < 0 ? 0 : (sx > w - 1 ? w - 1 : sx);
    sy = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
    dst[(long)y * pw + x] = (float)src[(long)sy * w + sx];
}

// dense 8-bit w x h image -> fp16 quad-difference texture (SrcTex8), w x h texels of 8 bytes; the host converts the fp32 input
// to 8 bit while it checks that every pixel is an integer in [0, 255] (4x less PCIe traffic than staging fp32)
__global__ void k_pack_quads_u8(const unsigned char* __restrict__ src, int w, int h, uint2* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int x1 = x + 1 > w - 1 ? w - 1 : x + 1, y1 = y + 1 > h - 1 ? h - 1 : y + 1;
    const int t00 = src[(long)y * w + x], t10 = src[(long)y * w + x1];
    const int t01 = src[(long)y1 * w + x], t11 = src[(long)y1 * w + x1];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 lo = {(_Float16)(float)t00, (_Float16)(float)(t01 - t00)};                           // exact: integers, |.| <= 255
    const h2 hi = {(_Float16)(float)(t10 - t00), (_Float16)(float)((t11 - t01) - (t10 - t00))};  // exact: integers, |.| <= 510
    dst[(long)y * w + x] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}

// dense w x h image -> fp32 quad-difference texture (SrcTex), w x h float4 texels
__global__ void k_pack_quads_f32(const float* __restrict__ src, int w, int h, float4* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const int x1 = x + 1 > w - 1 ? w - 1 : x + 1, y1 = y + 1 > h - 1 ? h - 1 : y + 1;
    const float t00 = src[(long)y * w + x], t10 = src[(long)y * w + x1], t01 = src[(long)y1 * w + x], t11 = src[(long)y1 * w + x1];
    dst[(long)y * w + x] = make_float4(t00, t10 - t00, t01 - t00, (t11 - t01) - (t10 - t00));
}

__global__ void k_export_depth(const float4* __restrict__ planes, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = planes[i].w;
}

// probe: nh planes per pixel ([nh][H][W]) against every view; out [nh][V][H][W]
template <int MAXV, bool U8, int SCALE>
__global__ __launch_bounds__(256, kWavesPerSimd) void k_eval_ncc(const ProblemDev* __restrict__ Pp, const float4* __restrict__ planes, int nh, float* __restrict__ out, LaunchArgs a) {
    const ProblemDev& P = *Pp;
    int x, y, x0, y0;
    const bool valid = dense_pixel(P, x, y, x0, y0);
    RefWin rw;
    ref_window_of_pixel<SCALE, 16, 16>(P, x, y, x0, y0, valid, a.spatial, a.two_sc, rw);
    if (!valid) return;
    const int idx = y * P.W + x;
    const long wh = (long)P.W * P.H;
    for (int h = 0; h < nh; ++h) {
        float m0, m1, m2;
        plane_to_m(P, planes[h * wh + idx], m0, m1, m2);
        for (int v = 0; v < P.V; ++v) out[((long)h * P.V + v) * wh + idx] = ncc_cost<U8, SCALE, true>(P.views[v], rw, x, y, m0, m1, m2);
    }
}

__global__ __launch_bounds__(256) void k_eval_geom(const ProblemDev* __restrict__ Pp, const float4* __restrict__ planes, float* __restrict__ out) {
    const ProblemDev& P = *Pp;
    int x, y;
    if (!dense_pixel(P, x, y)) return;
    const int idx = y * P.W + x;
    const long wh = (long)P.W * P.H;
    const float4 pl = planes[idx];
    for (int v = 0; v < P.V; ++v) out[v * wh + idx] = geom_cost(P, P.views[v], pl, x, y);
}

__global__ void k_homography(const ProblemDev* __restrict__ Pp, float4 pl, int v, float* __restrict__ H9) {
    const ProblemDev& P = *Pp;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float m[3];
    plane_to_m(P, pl, m[0], m[1], m[2]);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) H9[r * 3 + k] = __builtin_fmaf(-P.views[v].b[r], m[k], P.views[v].A[r * 3 + k]);
}

__global__ void k_math(int fn, const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    float y;
    switch (fn) {
        case 0: y = d_rcp(x); break;
        case 1: y = d_exp(x); break;
        case 2: y = d_sin(x); break;
        case 3: y = d_cos(x); break;
        case 4: y = d_acos(x); break;
        case 6: y = d_exp_select(x); break;  // the branch-free form of the window prologue: the same value as fn 1
        default: y = __builtin_amdgcn_fractf(x); break;
    }
    out[i] = y;
}

// d_rcp against the rule the oracle implements (oracle/pm_oracle.cpp det_rcp), for the 2^24 bit patterns base .. base + 2^24 - 1:
// counts[0] inputs with z and 1 / z normal, [1] of those that differ from the device's correctly rounded quotient 1.0f / z,
// [2] other inputs, [3] of those that break the rule (signed zero where 1 / z is denormal, otherwise not finite)
__global__ void k_verify_rcp(uint32_t base, unsigned long long* __restrict__ counts) {
    const uint32_t bits = base + blockIdx.x * blockDim.x + threadIdx.x;
    const float z = __uint_as_float(bits);
    const float got = d_rcp(z);
    const float az = __builtin_fabsf(z);
    const bool z_normal = az >= 1.17549435e-38f && az <= 3.40282347e+38f;
    if (z_normal && az <= 0x1p+126f) {
        const float want = 1.0f / z;  // -fhip-fp32-correctly-rounded-divide-sqrt: IEEE
        atomicAdd(&counts[0], 1ULL);
        if (__float_as_uint(got) != __float_as_uint(want)) atomicAdd(&counts[1], 1ULL);
    } else {
        atomicAdd(&counts[2], 1ULL);
        const bool finite = __builtin_fabsf(got) <= 3.40282347e+38f;
        const bool ok = z_normal ? __float_as_uint(got) == (bits & 0x80000000u) : !finite;
        if (!ok) atomicAdd(&counts[3], 1ULL);
    }
}

__global__ void k_rng(uint64_t seed, uint32_t pix, uint32_t launch, int n, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Rng g = rng_make(seed, pix, launch);
    for (int i = 0; i < n; ++i) out[i] = rng_uniform(g);
}

}  // namespace pm
