// ggc_ccl.h — the lock-free, run-based connected-component labelling shared by ggc_post.hip (mask clean-up, 8 neighbours),
// ggc_slic.hip (SLIC connectivity, 4) and ggc_matte_eval.hip (connectivity error, 4 per level).  DESIGN.md §5.27.
//
// parent[] is a forest over the pixels of one image; a root points at itself.  A labelling is init, merge, compress.
// Roots are smallest indices.  Every write to parent[] stores an index no larger than the pixel's own: init the first pixel
// of the pixel's run, ccl_union the smaller of two roots at the larger (atomicMin), compress the root.  So chains descend
// and end, and a finished component's root is its smallest raster index: the pixel at which a raster scan discovers it,
// which is what the CPU paths number by.
// Runs need no atomics.  A wave of the init kernel covers 64 consecutive flat indices.  A lane starts a run if its pixel is
// set and its left neighbour does not belong with it, or if it is lane 0 (the neighbour is in another wave); a ballot of
// the starts gives every lane its run's first lane (ccl_run_start_lane), hence pixel, with one plain store each.  Merge
// then only joins runs: a run cut at lane 0 to its left part (the wave-boundary join: flat index % 64 == 0), and a run to
// the runs of the row above.  Compress adds a run's length at its root with one atomic per run (ccl_run_length; the runs
// are those of init as long as both kernels use the same flat index).
// Plain reads beside atomicMin.  During merge parent[] changes only at roots, by atomicMin, only downwards.  ccl_find loads
// with relaxed agent-scope atomics: it sees each word whole, an old link or a new one, and both lead towards the current
// root.  ccl_union rechecks through atomicMin's return value: if the root it meant to link was linked elsewhere meanwhile
// (old != a), it goes on from that link.  What a merge kernel reads plainly is only "is q set": the sign of parent[q] (or
// the caller's own maps), which nothing after init changes.  Launch boundaries order init, merge and compress.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ggc {

__device__ __forceinline__ int ccl_find(const int32_t* parent, int i) {
    int p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != i) { i = p; p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return i;
}
__device__ __forceinline__ void ccl_union(int32_t* parent, int a, int b) {
    for (;;) {
        a = ccl_find(parent, a); b = ccl_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }      // link the larger root under the smaller
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// The same two on a forest kept in LDS: the parent map of one tile, whose indices are tile-local (row * tile width + column,
// so their order inside the tile is the raster order of the image).  The rule is the one above, an index no larger than the
// pixel's own at every store, so the loops end for the same reason; the loads are workgroup-scope, the atomicMin an LDS one.
__device__ __forceinline__ int ccl_find_lds(const int* par, int i) {
    int p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != i) { i = p; p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    return i;
}
__device__ __forceinline__ void ccl_union_lds(int* par, int a, int b) {
    for (;;) {
        a = ccl_find_lds(par, a); b = ccl_find_lds(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// Raster rank from per-segment flag words: a segment is 64 consecutive pixels of a row, its word has a bit per flagged
// pixel, and prefix is the exclusive sum of the words' popcounts in raster order of the segments.
__host__ __device__ inline int ccl_rank_in_word(unsigned long long word, int lane) {
    const unsigned long long below = word & ((1ull << lane) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(below);
#else
    return __builtin_popcountll(below);
#endif
}

// The lane at which `lane`'s run starts: the highest start at or below it.  starts must have one (a set lane always has).
__host__ __device__ inline int ccl_run_start_lane(unsigned long long starts, int lane) {
    const unsigned long long below = starts & ((2ull << lane) - 1ull);          // lane 63: 2 << 63 wraps to 0, all ones
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)below);
#else
    return 63 - __builtin_clzll(below);
#endif
}
// The length of the run that starts at `lane`: up to the next start or hole above it, or the end of the wave.
__host__ __device__ inline int ccl_run_length(unsigned long long starts, unsigned long long vmask, int lane) {
    const unsigned long long stop = (starts | ~vmask) >> lane >> 1;             // two shifts: lane + 1 may be 64
#if defined(__HIP_DEVICE_COMPILE__)
    return stop ? __ffsll((long long)stop) : 64 - lane;
#else
    return stop ? __builtin_ffsll((long long)stop) : 64 - lane;
#endif
}

// Init, by every lane of the wave: the first pixel of p's run.  same_left: p's left neighbour is in its row and belongs with it.
__device__ __forceinline__ int ccl_run_first(bool on, bool same_left, int p) {
    const int lane = threadIdx.x & 63;
    const unsigned long long starts = __ballot(on && (!same_left || lane == 0));
    return p - (lane - ccl_run_start_lane(starts, lane));
}

// Merge, for one set pixel p of the image whose map is par; flat is its index in the init kernel, joined(q) says that q is
// set and belongs with p.  Pixels of one row that touch are one run already, so a pixel whose left neighbour is joined
// only adds what that neighbour could not see.  4 neighbours: the pixel above, unless the left neighbour sits under the
// same upper run.  8: with a left neighbour, up-right when the pixel above is clear (else both are in one upper run, which
// a pixel further left in this run joins); without, the pixel above, or, when it is clear, up-left and up-right.
template <int CONN, class Joined>
__device__ __forceinline__ void ccl_merge_pixel(int32_t* par, int p, int x, bool has_up, int W, size_t flat, Joined joined) {
    static_assert(CONN == 4 || CONN == 8, "4 or 8 neighbours");
    const bool left = x > 0 && joined(p - 1);
    if (left && (flat & 63) == 0) ccl_union(par, p, p - 1);                     // the run continues across the init kernel's wave boundary
    if (!has_up) return;
    if constexpr (CONN == 4) {
        if (joined(p - W) && !(left && joined(p - W - 1))) ccl_union(par, p, p - W);
    } else {
        const bool up = joined(p - W);
        const bool ul = x > 0 && joined(p - W - 1), ur = x + 1 < W && joined(p - W + 1);
        if (left) {
            if (ur && !up) ccl_union(par, p, p - W + 1);
        } else if (up) {
            ccl_union(par, p, p - W);
        } else {
            if (ul) ccl_union(par, p, p - W - 1);
            if (ur) ccl_union(par, p, p - W + 1);
        }
    }
}

// Compress, in two halves so that a caller may hold counts between them.  A set lane finds its root and writes it back
// (roots keep pointing at themselves); then, by every lane of the wave, one atomicAdd of each run's length to counts[cell],
// the cell of the start lane's root.  vmask = __ballot(valid).
__device__ __forceinline__ int ccl_compress(int32_t* par, int p) { const int r = ccl_find(par, p); par[p] = r; return r; }
__device__ __forceinline__ void ccl_count_runs(bool valid, bool same_left, unsigned long long vmask, int32_t* counts, size_t cell) {
    const int lane = threadIdx.x & 63;
    const unsigned long long starts = __ballot(valid && (!same_left || lane == 0));
    if (valid && ((starts >> lane) & 1ull)) atomicAdd(&counts[cell], ccl_run_length(starts, vmask, lane));
}

// The largest component by atomicMax: larger area first, ties to the smaller root, the first in raster order.  Key 0: none.
__host__ __device__ inline unsigned long long ccl_best_key(int area, int root) {
    return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)root);
}
__host__ __device__ inline int ccl_best_root(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

} // namespace ggc
