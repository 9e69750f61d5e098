// ggc_maxflow.hip — max-flow / min-cut for GrabCut (C5: GCGraph::maxFlow + the
// source/sink labelling of estimateSegmentation) on the
// implicit 8-neighbour pixel grid with int32 capacities, all images of a batch at once.
//
// Algorithm: lock-free push-relabel (Hong 2008) in rounds of
//     global relabel  (exact BFS distances to the sink, as a min-plus relaxation)
//     -> push-relabel sweeps
// until no pixel holds excess that can still reach the sink.  Only phase 1
// (maximum preflow) is needed: a pixel is foreground iff it cannot reach the sink
// in the residual graph, which the last relabel has just computed.
//
// Mapping to the hardware:
//  * both phases work on LDS-resident tiles.  Relabel: a 32x32 tile + halo of labels
//    is relaxed to a local fixpoint per visit.  Push: a 32x8 tile of excess / residual
//    capacities / labels runs `inner` sweeps with LDS atomics, a wave per tile; pushes across the tile
//    edge use global atomics, and the write-back applies DELTAS atomically because a
//    neighbouring tile may have added to this tile's excess or reverse arcs meanwhile.
//    Every stale value is a lower bound of the true one, which is the asynchrony the
//    lock-free algorithm tolerates.
//  * activity is sparse (about 1 % of the pixels after the first round, a handful of
//    images in the last rounds), so every launch walks a WORK LIST of tiles instead of
//    the whole grid: a tile that changes (relabel) or keeps / hands over excess (push)
//    appends itself or its neighbour to the next list (flag + atomic counter), and a
//    launch costs a few microseconds when there is little to do.  Three rotating
//    counters let the launch that consumes list L also clear the counter of list L+2.
//  * images without active pixels leave the open-image list; converged tiles cost nothing.
#include "ggc_gc.h"
#include "ggc_mf_sweep.h"
#include "ggc_mf_push.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>

namespace ggc {

constexpr int RT = MF_RT;              // relabel tile side
constexpr int PT_W = MF_PT_W, PT_H = MF_PT_H;   // push tile (32x16 measured 6 % slower end to end)
constexpr int PT_N = PT_W * PT_H;      // threads of a push block, one pixel each
// blocks per work-list launch and 64 open images: a block walks several tiles of the list (measured best, tools/mf_knobs.sh)
constexpr int PUSH_GRID = 1024, RELAX_GRID = 1024, ASYNC_GRID = 128;

// up to three int32 regions zeroed by ONE launch (a round used to issue seven hipMemsetAsync calls: each is a launch of its own)
__global__ void __launch_bounds__(256) k_mf_zero3(int32_t* __restrict__ a, size_t na, int32_t* __restrict__ b, size_t nb, int32_t* __restrict__ c, size_t nc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = 0;
    else if (i < na + nb) b[i - na] = 0;
    else if (i < na + nb + nc) c[i - na - nb] = 0;
}
void mf_zero3(hipStream_t st, int32_t* a, size_t na, int32_t* b, size_t nb, int32_t* c, size_t nc) {
    const size_t n = na + nb + nc;
    if (n) hipLaunchKernelGGL(k_mf_zero3, dim3(cdiv(n, 256)), dim3(256), 0, st, a, na, b, nb, c, nc);
}

// Ring and control words of an asynchronous launch's queue, zeroed on the way by a kernel that runs before it anyway (2-D grid,
// every thread calls it): the launch itself then needs no set-up launch.  Zeroed EVERY time: a launch that ended on its visit
// budget or on the time-out leaves entries behind.
__device__ __forceinline__ void aq_zero(unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap) {
    const size_t n_thr = (size_t)gridDim.x * gridDim.y * blockDim.x;
    const size_t i0 = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < (size_t)cap; i += n_thr) ring[i] = 0ull;
    if (i0 < (size_t)AQ_WORDS) q[i0] = 0;
}

// The same through a per-block list.  Every append used to be a returning atomicAdd on the ONE counter of the next list, and
// same-address atomics retire at ~90 per microsecond chip-wide: a dense launch appends ~15 000 tiles, i.e. >= 150 us of
// counter traffic — which is what those launches took (139-165 us), whatever the grid or the occupancy.  A block now
// collects its tiles in LDS and reserves their slots with one atomicAdd when it is done.
constexpr int OUT_CAP = 1024;
struct OutList { int n, base; int buf[OUT_CAP]; };
__device__ __forceinline__ void push_tile_l(int tile, int32_t* __restrict__ flag, OutList& L, int32_t* __restrict__ list,
                                            int32_t* __restrict__ count) {
    if (ldg(&flag[tile]) == 0 && atomicExch(&flag[tile], 1) == 0) {
        const int i = atomicAdd(&L.n, 1);
        if (i < OUT_CAP) L.buf[i] = tile;
        else list[atomicAdd(count, 1)] = tile;                             // (a block that overflows its list appends directly)
    }
}
// all threads of the block, once, after their last push_tile_l
__device__ __forceinline__ void flush_tiles(OutList& L, int32_t* __restrict__ list, int32_t* __restrict__ count) {
    __syncthreads();
    const int n = min(L.n, OUT_CAP);
    if (threadIdx.x == 0 && n > 0) L.base = atomicAdd(count, n);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) list[L.base + i] = L.buf[i];
}

// Start of a global relabel by TILES (the wave-per-tile relabel kernels): a wave writes the starting labels of one 32x32
// tile (1 next to the sink, infinity elsewhere) and puts the tile on the first work list only if it holds a pixel WITHOUT a
// sink link — a tile whose pixels all touch the sink (59 % of the bench's pixels are definite background) is final at
// label 1 and never needs a visit.  (Folding this pass into the first relabel launch was measured in round 3: the heavy kernel then visits every tile, 99 us against 18 + 70.)
// It is the first kernel of a round, so it also leaves the round's bookkeeping clean (each used to be a zero-fill launch of
// its own): BOTH membership flags of every relabel tile it looks at (tiles of closed images are never listed again), the
// image's active-pixel count, and the words the active scan and k_done_update accumulate into (scan[0]: open images,
// scan[4..6]: push-list counters, scan[7]: active total).  The relabel counters themselves are zeroed by k_done_update / k_open_init.
// And the queue of the asynchronous relabel launch that follows the work-list launches: ring[0 .. cap) and q (aq_zero).
// lmax: the image's label-ceiling word of THIS round (k_mf_active fills it), zeroed with active[].
// PROF (GGC_MF_TRACE): before a label is overwritten, parked[pixel] = the pixel holds excess and a label in [lim, DINF),
// lim from lmax_prev, the ceiling word of the round before (null in a solve's first round: nothing is marked); k_mf_active
// counts how many of the marked pixels the relabel found a way to the sink for.
template <bool PROF>
__global__ void __launch_bounds__(256) k_mf_rinit(GcDims d, MfTiles tl, const int32_t* __restrict__ open_list,
                                                  const int32_t* __restrict__ snk, int32_t* __restrict__ dist,
                                                  int32_t* __restrict__ list, int32_t* __restrict__ flag, int32_t* __restrict__ flag2,
                                                  int32_t* __restrict__ count, int32_t* __restrict__ active, int32_t* __restrict__ lmax,
                                                  int32_t* __restrict__ scan,
                                                  unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap,
                                                  const int32_t* __restrict__ lmax_prev, int slack, const int32_t* __restrict__ ex,
                                                  uint8_t* __restrict__ parked) {
    constexpr int T = MF_RT;
    __shared__ OutList outl;
    if (threadIdx.x == 0) outl.n = 0;
    aq_zero(ring, q, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) { active[open_list[blockIdx.y]] = 0; lmax[(size_t)open_list[blockIdx.y] * MF_LMAX_STRIDE] = 0; }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 8 && (threadIdx.x == 0 || threadIdx.x >= 4)) scan[threadIdx.x] = 0;   // not [1..3]: the relabel counters this launch appends to
    __syncthreads();
    const int tiles_per_image = tl.rt_x * tl.rt_y;
    const int tr = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tr < tiles_per_image) {
        const int b = open_list[blockIdx.y];
        const int ty0 = (tr / tl.rt_x) * T, tx0 = (tr % tl.rt_x) * T;
        const int lx = lane & 31, h = lane >> 5;
        const size_t base = (size_t)b * d.P;
        int sv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[r] = snk[base + (size_t)min(ty0 + 16 * h + r, d.H - 1) * d.W + min(tx0 + lx, d.W - 1)];
        bool open_px = false;
        if (PROF) {
            const int lim = (lmax_prev && slack >= 0) ? min(d.P, lmax_prev[(size_t)b * MF_LMAX_STRIDE] + 1 + slack) : d.P;
            for (int r = 0; r < 16; ++r) {
                const int y = ty0 + 16 * h + r, x = tx0 + lx;
                if (x < d.W && y < d.H) {
                    const size_t i = base + (size_t)y * d.W + x;
                    parked[i] = (lmax_prev && ex[i] > 0 && dist[i] >= lim && dist[i] < DINF) ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int y = ty0 + 16 * h + r, x = tx0 + lx;
            if (x < d.W && y < d.H) {
                dist[base + (size_t)y * d.W + x] = sv[r] > 0 ? 1 : DINF;
                open_px |= sv[r] <= 0;
            }
        }
        const bool listed = __any(open_px);
        if (lane == 0) {
            const int tile = b * tiles_per_image + tr;
            flag[tile] = listed ? 1 : 0;                                   // one writer per tile
            flag2[tile] = 0;
            if (listed) {
                const int i = atomicAdd(&outl.n, 1);
                if (i < OUT_CAP) outl.buf[i] = tile; else list[atomicAdd(count, 1)] = tile;
            }
        }
    }
    flush_tiles(outl, list, count);
}

// Global relabel over a work list of 32x32 tiles, a WAVE per tile (4 tiles per block, no block barrier): the labels are relaxed
// by alternating vertical and horizontal in-register sweeps (mf_relax_visit, ggc_mf_sweep.h), which carry a front across the
// tile in a handful of sweeps where a neighbour-at-a-time iteration needs one per pixel of the way.
template <bool PROF>
__global__ void __launch_bounds__(256) k_mf_relax_wave(GcDims d, MfTiles tl, int phase, long long* __restrict__ prof, uint8_t* __restrict__ rmask,
                                                       int32_t* __restrict__ dirty, const int32_t* __restrict__ rc, int32_t* __restrict__ dist, int32_t* __restrict__ counters,
                                                       const int32_t* __restrict__ list_in, int32_t* __restrict__ list_out,
                                                       int32_t* __restrict__ flag_in, int32_t* __restrict__ flag_out) {
    __shared__ RelaxWaveLds lds[4];
    __shared__ OutList outl;
    if (threadIdx.x == 0) outl.n = 0;
    __syncthreads();
    const int wv = threadIdx.x >> 6;
    const int n_in = counters[phase % 3];
    int32_t* n_out = counters + (phase + 1) % 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[(phase + 2) % 3] = 0;       // the list after next starts empty
    const int tiles_per_image = tl.rt_x * tl.rt_y;
    const int G = gridDim.x * 4;
    MfRelaxClocks<PROF> ck;
    // the list entry of the NEXT visit is requested one visit ahead: read at the top of its own visit it is a memory round
    // trip in front of the tile's 50 loads (measured: load + fill 12 us of a 22 us visit)
    int tile_nx = blockIdx.x * 4 + wv < n_in ? list_in[blockIdx.x * 4 + wv] : 0;
    for (int t = blockIdx.x * 4 + wv; t < n_in; t += G) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));                                     // keeps the lane arithmetic inside the loop (no hoist + spill)
        ck.begin();
        const int tile = __builtin_amdgcn_readfirstlane(tile_nx);
        tile_nx = t + G < n_in ? list_in[t + G] : 0;
        const int nbm = mf_relax_visit<false, PROF, GGC_MF_RELAX_BFS != 0>(d, tl, tile, lane, lds[wv], rmask, dirty, rc, dist, flag_in, ck);
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / tl.rt_x, txi = tr % tl.rt_x;
        if (lane < 9 && (nbm >> lane) & 1) {
            const int ty = tyi + lane / 3 - 1, tx = txi + lane % 3 - 1;
            if (ty >= 0 && ty < tl.rt_y && tx >= 0 && tx < tl.rt_x)
                push_tile_l(b * tiles_per_image + ty * tl.rt_x + tx, flag_out, outl, list_out, n_out);
        }
        mf_wave_sync();
        ck.end();
    }
    if (PROF && (threadIdx.x & 63) == 0 && ck.sum[3]) {                     // GGC_MF_TRACE: one set of atomics per wave
        unsigned long long* q = reinterpret_cast<unsigned long long*>(prof) + (64 + (blockIdx.x & 63)) * 8;
        for (int k = 0; k < 7; ++k) atomicAdd(&q[k], (unsigned long long)ck.sum[k]);
    }
    flush_tiles(outl, list_out, n_out);
}

// Push-relabel sweeps over a work list of 32x8 tiles, a WAVE per tile (4 tiles per block per step of the list, no block
// barrier inside a visit): push_tile_visit<8, false> of ggc_mf_push.h, the visit of the asynchronous launch with the memory
// rules of a launch over a work list.  A sweep costs what the tile's active pixels cost (11 to 56 of 256 in the bench) instead
// of four waves running the whole active path behind a block barrier.  A tile is on a list at most once per launch, so no
// second wave can hold it and it needs no state word.  The next tile's list entry is fetched one visit ahead; its loads are
// hidden by the other resident waves (12 tiles in flight per CU), not by a register prefetch.
// PROF (GGC_MF_TRACE): the visits' clocks into table 3 of the trace clocks.
#ifndef GGC_MF_PUSH_WAVE
#define GGC_MF_PUSH_WAVE 1          // dense push launches: 1 = k_mf_pr_wave, 0 = k_mf_pr_list (a block per tile, one pixel per thread)
#endif
constexpr int PUSH_WAVE_GRID_DIV = 2;   // blocks of k_mf_pr_wave = blocks k_mf_pr_list would get / this (a block visits four tiles at a time; measured: 1, 2, 4)
template <bool PROF>
__global__ void __launch_bounds__(256) k_mf_pr_wave(GcDims d, MfTiles tl, int phase, int inner, const int32_t* __restrict__ lmax, int slack,
                                                    long long* __restrict__ prof,
                                                    int32_t* __restrict__ rc, int32_t* __restrict__ ex,
                                                    int32_t* __restrict__ snk, int32_t* __restrict__ dist, uint8_t* __restrict__ rmask,
                                                    int32_t* __restrict__ dirty, int32_t* __restrict__ counters, const int32_t* __restrict__ list_in,
                                                    int32_t* __restrict__ list_out, int32_t* __restrict__ flag_in,
                                                    int32_t* __restrict__ flag_out) {
    __shared__ PushTileLds<PT_H> lds[4];
    __shared__ OutList outl;
    if (threadIdx.x == 0) outl.n = 0;
    __syncthreads();
    const int wv = threadIdx.x >> 6;
    const int n_in = counters[phase % 3];
    int32_t* n_out = counters + (phase + 1) % 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[(phase + 2) % 3] = 0;       // the list after next starts empty
    const int tiles_per_image = tl.pt_x * tl.pt_y;
    const size_t BP = (size_t)d.B * d.P;
    const int G = gridDim.x * 4;
    long long pv[4] = {0, 0, 0, 0}, p_all = 0, p_n = 0;                    // GGC_MF_TRACE: kept in registers, one set of atomics per wave
    int tile_nx = blockIdx.x * 4 + wv < n_in ? list_in[blockIdx.x * 4 + wv] : 0;   // the list entry of the NEXT visit, one visit ahead
    for (int t = blockIdx.x * 4 + wv; t < n_in; t += G) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));                                     // keeps the lane arithmetic inside the loop (no hoist + spill)
        const long long t_0 = PROF ? wall_clock64() : 0;
        const int tile = __builtin_amdgcn_readfirstlane(tile_nx);
        tile_nx = t + G < n_in ? list_in[t + G] : 0;
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / tl.pt_x, txi = tr % tl.pt_x;
        if (lane == 0) flag_in[tile] = 0;                                  // consumed
        const int nbm = push_tile_visit<PT_H, false>(d, lmax + (size_t)b * MF_LMAX_STRIDE, slack, tyi, txi, inner, (size_t)b * d.P, BP, rc, ex, snk, dist, rmask, lds[wv], lane, PROF, pv);
        if (lane < 9 && (nbm >> lane) & 1) {
            const int ty = tyi + lane / 3 - 1, tx = txi + lane % 3 - 1;
            if (ty >= 0 && ty < tl.pt_y && tx >= 0 && tx < tl.pt_x) {
                const int nbt = b * tiles_per_image + ty * tl.pt_x + tx;
                if (lane != 4) dirty[nbt] = 1;                             // its border arcs may have been re-opened (ggc_mf_sweep.h)
                push_tile_l(nbt, flag_out, outl, list_out, n_out);
            }
        }
        mf_wave_sync();
        if (PROF) { p_all += wall_clock64() - t_0; ++p_n; }
    }
    if (PROF && (threadIdx.x & 63) == 0 && p_n) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(prof) + (192 + (blockIdx.x & 63)) * 8;
        atomicAdd(&o[0], (unsigned long long)pv[0]); atomicAdd(&o[1], (unsigned long long)pv[1]);
        atomicAdd(&o[2], (unsigned long long)(p_all - pv[0] - pv[1]));     // write-back + hand-over
        atomicAdd(&o[3], (unsigned long long)p_n); atomicAdd(&o[4], (unsigned long long)pv[2]); atomicAdd(&o[5], (unsigned long long)pv[3]);
    }
    flush_tiles(outl, list_out, n_out);
}

// The same with a 256-thread block per tile, one pixel per thread and a block barrier per sweep: the dense push until
// k_mf_pr_wave, kept for comparison (-DGGC_MF_PUSH_WAVE=0, tools/build_variant.sh).
#if !GGC_MF_PUSH_WAVE
__global__ void __launch_bounds__(PT_N) k_mf_pr_list(GcDims d, MfTiles tl, int phase, int inner, const int32_t* __restrict__ lmax, int slack,
                                                    int32_t* __restrict__ rc, int32_t* __restrict__ ex,
                                                    int32_t* __restrict__ snk, int32_t* __restrict__ dist, uint8_t* __restrict__ rmask,
                                                    int32_t* __restrict__ dirty, int32_t* __restrict__ counters, const int32_t* __restrict__ list_in,
                                                    int32_t* __restrict__ list_out, int32_t* __restrict__ flag_in,
                                                    int32_t* __restrict__ flag_out) {
    __shared__ int s_ex[PT_N];
    __shared__ int s_d[PT_H + 2][PT_W + 2];
    __shared__ int s_rc[8][PT_N];
    __shared__ OutList outl;
    __shared__ int s_nbm;                                                  // bit (dy + 1) * 3 + (dx + 1): tiles to put on the next list
    const int tid = threadIdx.x, lx = tid & 31;
    if (tid == 0) outl.n = 0;                                              // (the first barrier of the tile loop orders it)
    const int n_in = counters[phase % 3];
    int32_t* n_out = counters + (phase + 1) % 3;
    if (blockIdx.x == 0 && tid == 0) counters[(phase + 2) % 3] = 0;
    const int tiles_per_image = tl.pt_x * tl.pt_y;
    const size_t BP = (size_t)d.B * d.P;
    // The visit latency bounds the dense launches, so the next tile of this block is loaded into registers while the
    // current one is swept (its list entry one step earlier still).  Safe for the same reason concurrent tiles are:
    // ring pixels are written back as atomic deltas, interior pixels have no other writer during a launch.
    constexpr int N_HALO = (PT_H + 2) * (PT_W + 2), HALO_IT = (N_HALO + PT_N - 1) / PT_N;
    struct TileRegs { int e, sk, r[8], hv[HALO_IT]; };
    auto load_tile = [&](int tile, TileRegs& R) {
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / tl.pt_x, txi = tr % tl.pt_x;
        const int x = txi * PT_W + lx;
        const size_t base = (size_t)b * d.P;
        const int y = tyi * PT_H + (tid >> 5);
        const bool in = x < d.W && y < d.H;
        const int p = y * d.W + x;
        R.e = in ? ex[base + p] : 0;
        R.sk = in ? snk[base + p] : 0;
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) R.r[dir] = in ? rc[rc_idx(dir, base + p)] : 0;
#pragma unroll
        for (int k = 0; k < HALO_IT; ++k) {
            const int i = tid + k * PT_N;
            const int gy = tyi * PT_H + i / (PT_W + 2) - 1, gx = txi * PT_W + i % (PT_W + 2) - 1;
            R.hv[k] = (i < N_HALO && gx >= 0 && gx < d.W && gy >= 0 && gy < d.H) ? dist[base + (size_t)gy * d.W + gx] : DINF;
        }
    };
    const int G = gridDim.x;
    int t = blockIdx.x;
    if (t >= n_in) return;
    int tile_next = list_in[t];
    int tile_next2 = t + G < n_in ? list_in[t + G] : 0;
    TileRegs N;
    load_tile(tile_next, N);
    for (; t < n_in; t += G) {
        const int tile = tile_next;
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / tl.pt_x, txi = tr % tl.pt_x;
        const int x = txi * PT_W + lx;
        const size_t base = (size_t)b * d.P;
        __syncthreads();
        const int y = tyi * PT_H + (tid >> 5);
        const bool inb = x < d.W && y < d.H;
        const int pp = y * d.W + x;
        const int e0 = N.e, sk0 = N.sk;
        int sk = sk0, r0[8];
        s_ex[tid] = e0;
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) { r0[dir] = N.r[dir]; s_rc[dir][tid] = r0[dir]; }
#pragma unroll
        for (int k = 0; k < HALO_IT; ++k) {
            const int i = tid + k * PT_N;
            if (i < N_HALO) s_d[i / (PT_W + 2)][i % (PT_W + 2)] = N.hv[k];
        }
        if (t + G < n_in) {                                                // block-uniform
            tile_next = tile_next2;
            tile_next2 = t + 2 * G < n_in ? list_in[t + 2 * G] : 0;
            load_tile(tile_next, N);
        }
        __syncthreads();
        if (tid == 0) { flag_in[tile] = 0; s_nbm = 0; }                                   // consumed
        const int d0 = s_d[(tid >> 5) + 1][lx + 1];
        const int lim = slack < 0 ? d.P : min(d.P, lmax[(size_t)b * MF_LMAX_STRIDE] + 1 + slack);   // the image's label ceiling (ggc_mf_push.h)
        int nbm = 0;
        for (int it = 0; it < inner; ++it) {
            int act = 0;
            if (inb) {
                const int slot = tid, ly = slot >> 5;
                const int e = __hip_atomic_load(&s_ex[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int dp = s_d[ly + 1][lx + 1];
                if (e > 0 && dp < lim) {
                    act = 1;
                    // the 8 residual capacities and 8 neighbour labels are read in one batch and the arg-min is branch-free:
                    // one LDS round trip per sweep instead of a chain of up to 16
                    int r[8], hq[8];
#pragma unroll
                    for (int dir = 0; dir < 8; ++dir) {
                        r[dir] = __hip_atomic_load(&s_rc[dir][slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        hq[dir] = s_d[ly + 1 + dir_dy(dir)][lx + 1 + dir_dx(dir)];
                    }
                    int hmin = sk > 0 ? 0 : DINF, best = sk > 0 ? 8 : -1, rb = 0;
#pragma unroll
                    for (int dir = 0; dir < 8; ++dir) {
                        const bool ok = r[dir] > 0 && hq[dir] < hmin;
                        hmin = ok ? hq[dir] : hmin; best = ok ? dir : best; rb = ok ? r[dir] : rb;
                    }
                    if (best >= 0 && dp > hmin) {
                        if (best == 8) {
                            const int dl = min(e, sk);
                            sk -= dl;
                            atomicSub(&s_ex[slot], dl);
                        } else {
                            const int dl = min(e, rb);
                            atomicSub(&s_rc[best][slot], dl);
                            atomicSub(&s_ex[slot], dl);
                            const int bx = dir_dx(best), by = dir_dy(best);
                            const int qlx = lx + bx, qly = ly + by;
                            if (qlx >= 0 && qlx < PT_W && qly >= 0 && qly < PT_H) {
                                const int qt = qly * PT_W + qlx;
                                atomicAdd(&s_rc[best ^ 1][qt], dl);
                                atomicAdd(&s_ex[qt], dl);
                            } else {                                        // across the tile edge: straight to global memory
                                const int q = pp + by * d.W + bx;
                                atomicAdd(&rc[rc_idx((best ^ 1), base + q)], dl);
                                atomicAdd(&ex[base + q], dl);
                                // (the neighbour tile is told after the sweeps)
                                const int tdy = qly < 0 ? -1 : (qly >= PT_H ? 1 : 0), tdx = qlx < 0 ? -1 : (qlx >= PT_W ? 1 : 0);
                                nbm |= 1 << ((tdy + 1) * 3 + tdx + 1);
                            }
                        }
                    } else {
                        s_d[ly + 1][lx + 1] = (best >= 0 && hmin < DINF) ? hmin + 1 : DINF;
                    }
                }
            }
            if (!__syncthreads_or(act)) break;
        }
        int left = 0;
        if (inb) {
            // only the tile's border ring can receive pushes from other tiles during this launch: the interior is
            // owned exclusively, so its write-back is a plain store (L2 atomics are the scarce resource in the
            // early rounds, when nearly every pixel changes)
            const int slot = tid, ly = slot >> 5, p = pp;
            const bool ring = lx == 0 || lx == PT_W - 1 || ly == 0 || ly == PT_H - 1;
            const int e1 = s_ex[slot];
            if (e1 != e0) { if (ring) atomicAdd(&ex[base + p], e1 - e0); else ex[base + p] = e1; }
            int m1 = 0, chg = 0;
#pragma unroll
            for (int dir = 0; dir < 8; ++dir) {
                const int r1 = s_rc[dir][slot];
                m1 |= (r1 > 0) ? (1 << dir) : 0;
                if (r1 != r0[dir]) {
                    chg = 1;
                    // another tile's push can only add to an arc that points OUT of this tile (the reverse of its own arc):
                    // those go back as atomic deltas, every other capacity is this block's alone (L2 atomics, ~30 G/s chip-wide,
                    // are what bounds the dense rounds)
                    const bool out = (ly == 0 && dir_dy(dir) < 0) || (ly == PT_H - 1 && dir_dy(dir) > 0) ||
                                     (lx == 0 && dir_dx(dir) < 0) || (lx == PT_W - 1 && dir_dx(dir) > 0);
                    if (out) atomicAdd(&rc[rc_idx(dir, base + p)], r1 - r0[dir]);
                    else rc[rc_idx(dir, base + p)] = r1;
                }
            }
            if (chg) rmask[base + p] = (uint8_t)m1;     // (arcs that leave the tile: the relabel reads the capacities, see mf_tile_dirty)
            if (sk != sk0) snk[base + p] = sk;
            const int d1 = s_d[ly + 1][lx + 1];
            if (d1 != d0) dist[base + p] = d1;
            left |= (e1 > 0 && d1 < lim) ? 1 : 0;
        }
        if (nbm) atomicOr(&s_nbm, nbm);
        if (__syncthreads_or(left) && tid == 0) s_nbm |= 1 << 4;           // still has work
        __syncthreads();
        if (tid < 9 && (s_nbm >> tid) & 1) {
            const int ty = tyi + tid / 3 - 1, tx = txi + tid % 3 - 1;
            if (ty >= 0 && ty < tl.pt_y && tx >= 0 && tx < tl.pt_x) {
                const int nbt = b * tiles_per_image + ty * tl.pt_x + tx;
                if (tid != 4) dirty[nbt] = 1;                              // its border arcs may have been re-opened (ggc_mf_sweep.h)
                push_tile_l(nbt, flag_out, outl, list_out, n_out);
            }
        }
    }
    flush_tiles(outl, list_out, n_out);
}
#endif

// per image: number of pixels whose excess can still reach the sink; their push tiles form the round's first work list.
// A wave scans one 32x8 push tile (4 pixels per lane, rows of 128 bytes) and appends it once when it holds an active pixel:
// no per-pixel membership test.  (The pixel-strided scan this replaces sent every active pixel through the tile's flag —
// 920 k flag reads and LDS appends in the first round of a 64-image solve: 203 us, against ~25 us for the 61 MB it reads.)
// aq_st != null (asynchronous push on 32x8 tiles, whose tiles are these tiles): the scan also leaves the queue of that launch
// ready — ring[0 .. cap) and q zero, and the state word of every push tile of an open image "queued" (1) when it is listed
// and 0 otherwise (a closed image's words are never read: its tiles are neither listed nor anybody's neighbours).
// The scan holds every label of the image, so it also leaves lmax[b], the image's largest FINITE label: the push phase that
// follows parks excess above it (the label ceiling, ggc_mf_push.h).  A running maximum per lane, one reduction per wave and
// one atomicMax per block; k_mf_rinit zeroed the word.
// PROF (GGC_MF_TRACE): of the pixels k_mf_rinit<true> marked as parked above the previous ceiling, how many still hold excess
// (slot 7 of the rows of trace table 2) and how many of those the relabel gave a finite label (slot 7 of table 1).
template <bool PROF>
__global__ void __launch_bounds__(256) k_mf_active(GcDims d, MfTiles tl, const int32_t* __restrict__ open_list,
                                                   const int32_t* __restrict__ ex, const int32_t* __restrict__ dist,
                                                   int32_t* __restrict__ active, int32_t* __restrict__ lmax, int32_t* __restrict__ flag, int32_t* __restrict__ flag2,
                                                   int32_t* __restrict__ list, int32_t* __restrict__ count,
                                                   int32_t* __restrict__ aq_st, unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap,
                                                   const uint8_t* __restrict__ parked, long long* __restrict__ prof) {
    __shared__ OutList outl;
    __shared__ int s_n, s_l;
    if (threadIdx.x == 0) { outl.n = 0; s_n = 0; s_l = 0; }
    if (aq_st) aq_zero(ring, q, cap);
    __syncthreads();
    const int tiles_per_image = tl.pt_x * tl.pt_y;
    const int b = open_list[blockIdx.y];
    const int lane = threadIdx.x & 63, lx = lane & 31, r0 = lane >> 5;
    const size_t base = (size_t)b * d.P;
    int n_block = 0, l_lane = 0, n_parked = 0, n_wrong = 0;
    for (int tr = blockIdx.x * 4 + (threadIdx.x >> 6); tr < tiles_per_image; tr += gridDim.x * 4) {
        const int tyi = tr / tl.pt_x, txi = tr - tyi * tl.pt_x;
        const int x = txi * PT_W + lx;
        int ev[PT_H / 2], dv[PT_H / 2];
#pragma unroll
        for (int j = 0; j < PT_H / 2; ++j) {                               // every load issued from a clamped address, then masked
            const int y = tyi * PT_H + r0 + 2 * j;
            const size_t i = base + (size_t)min(y, d.H - 1) * d.W + min(x, d.W - 1);
            ev[j] = ex[i]; dv[j] = dist[i];
        }
        int n = 0;
#pragma unroll
        for (int j = 0; j < PT_H / 2; ++j) {
            const int y = tyi * PT_H + r0 + 2 * j;
            n += (x < d.W && y < d.H && ev[j] > 0 && dv[j] < DINF) ? 1 : 0;
            l_lane = max(l_lane, dv[j] < DINF ? dv[j] : 0);                // (a clamped address repeats a pixel of the image)
            if (PROF && x < d.W && y < d.H && ev[j] > 0 && parked[base + (size_t)y * d.W + x]) { ++n_parked; n_wrong += dv[j] < DINF ? 1 : 0; }
        }
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) {
            const int tile = b * tiles_per_image + tr;
            flag[tile] = n > 0 ? 1 : 0;                                    // both membership flags of every push tile of an open image: one writer
            flag2[tile] = 0;                                               // per tile, no zero-fill launch before the scan
            if (aq_st) aq_st[tile] = n > 0 ? 1 : 0;
            if (n > 0) {
                const int i = atomicAdd(&outl.n, 1);
                if (i < OUT_CAP) outl.buf[i] = tile; else list[atomicAdd(count, 1)] = tile;
                n_block += n;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) l_lane = max(l_lane, __shfl_xor(l_lane, o, 64));
    if (lane == 0 && n_block) atomicAdd(&s_n, n_block);
    if (lane == 0 && l_lane) atomicMax(&s_l, l_lane);
    if (PROF) {
        for (int o = 32; o > 0; o >>= 1) { n_parked += __shfl_xor(n_parked, o, 64); n_wrong += __shfl_xor(n_wrong, o, 64); }
        unsigned long long* o = reinterpret_cast<unsigned long long*>(prof) + (64 + (blockIdx.x & 63)) * 8;
        if (lane == 0 && n_parked) { atomicAdd(&o[64 * 8 + 7], (unsigned long long)n_parked); atomicAdd(&o[7], (unsigned long long)n_wrong); }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(&active[b], s_n);
    if (threadIdx.x == 0 && s_l) atomicMax(&lmax[(size_t)b * MF_LMAX_STRIDE], s_l);
    flush_tiles(outl, list, count);
}

// closes images without active pixels and compacts the still-open ones into the next launch list
__global__ void k_done_update(int n_cur, const int32_t* __restrict__ list_cur, const int32_t* __restrict__ active,
                              int32_t* __restrict__ list_nxt, int32_t* __restrict__ n_open, int keep_all, int32_t* __restrict__ rl_cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3) rl_cnt[i] = 0;                              // this round's relabel is over: its work-list counters start the next one at zero
    if (i >= n_cur) return;
    const int b = list_cur[i];
    if (active[b] != 0 || keep_all) { list_nxt[atomicAdd(n_open, 1)] = b; atomicAdd(n_open + 7, active[b]); }   // [7]: active pixels in total
}
__global__ void k_open_init(int B, const int32_t* __restrict__ state, int32_t* __restrict__ list, int32_t* __restrict__ n_open,
                            int32_t* __restrict__ rl_cnt) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < 3) rl_cnt[b] = 0;
    if (b < B && !state[b]) list[atomicAdd(n_open, 1)] = b;
}

namespace {

constexpr int MF_PROF_TABLES = 4;

// The max-flow's scratch, one slot.  `dirty` must outlive a solve: the warm start of the next GrabCut iteration relies on
// the marks it left.  The slot keeps its size through the solves of a call, so it is not reallocated in between.
struct MfWork {
    int32_t *rl_list[2], *rl_flag[2];    // relabel tiles: ping-pong work lists and membership flags
    int32_t *pt_list[2], *pt_flag[2];    // push tiles: the same
    unsigned long long* ring;            // ticket ring of the asynchronous launches, one slot per tile of the larger kind
    int32_t* aq;                         // its control words
    int32_t* busy;                       // state word per tile of an asynchronous push
    long long* prof;                     // GGC_MF_TRACE clocks [MF_PROF_TABLES][64][8]: asynchronous push waves | tile visits (asynchronous push, dense relabel) | asynchronous relabel visits | dense push visits
    int32_t* dirty;                      // one word per push tile: a neighbour pushed into it since its arc masks were last exact
    int32_t* lmax;                       // [2][B * MF_LMAX_STRIDE] largest finite label per image, one word per 128-byte line, the word of an even round | of an odd round (label ceiling)
    uint8_t* parked;                     // GGC_MF_TRACE only, [B * P]: pixels whose excess the ceiling parked (k_mf_rinit<true>)
    void layout(Carve& c, size_t n_rt, size_t n_pt, size_t B, size_t n_parked) {
        for (auto& p : rl_list) p = c.take<int32_t>(n_rt);
        for (auto& p : rl_flag) p = c.take<int32_t>(n_rt);
        for (auto& p : pt_list) p = c.take<int32_t>(n_pt);
        for (auto& p : pt_flag) p = c.take<int32_t>(n_pt);
        ring = c.take<unsigned long long>(std::max(n_rt, n_pt));
        aq = c.take<int32_t>(AQ_WORDS);
        busy = c.take<int32_t>(n_pt);
        prof = c.take<long long>(MF_PROF_TABLES * 64 * 8);
        dirty = c.take<int32_t>(n_pt);
        lmax = c.take<int32_t>(2 * B * MF_LMAX_STRIDE);
        parked = c.take<uint8_t>(n_parked);
    }
};

// One solve: its buffers, its tiling, its workspace, and the two phases of a round.
struct MfSolve {
    ggc_ctx* ctx; hipStream_t st; GcDims d; MfTiles tl; size_t n_rt, n_pt;
    int32_t *rc, *ex, *snk, *dist; uint8_t* rmask;
    MfControl ctl;
    int32_t *n_open, *rl_cnt, *pr_cnt;   // ctl.cnt [0], [1..3], [4..6]
    MfWork w;
    long long* prof;                     // w.prof under GGC_MF_TRACE, null otherwise

    // Global relabel of the n_cur images on `open`.  k_mf_rinit starts the labels from the sink links and lists the tiles that
    // have a pixel away from the sink; the first launches relax every listed tile (bandwidth work, plain stores), and the long
    // sparse rest of the front runs inside ONE asynchronous launch that ends at the exact fixpoint (nothing to read back).
    // A PARTIAL relabel stops after the work-list launches.  `launches`: how many relabel launches ran.
    // The image's label-ceiling words alternate between two rows by the round's parity: the row k_mf_rinit zeroes and
    // k_mf_active fills is not the one the trace still reads the previous ceiling from.
    int32_t* lmax_row(int round) const { return w.lmax + (size_t)(round & 1) * d.B * MF_LMAX_STRIDE; }

    int relabel(const int32_t* open, int round, int n_cur, size_t scale, bool partial, int& launches) {
        const Knobs& kn = knobs();
        const int per_image = tl.rt_x * tl.rt_y;
        const int grid = (int)std::min<size_t>(RELAX_GRID * scale, std::max<size_t>(16, cdiv((size_t)n_cur * per_image, 4)));
        ProfScope ps(ctx, st, "maxflow_relabel");
        const int32_t* no_prev = nullptr;
        if (prof) hipLaunchKernelGGL(k_mf_rinit<true>, dim3(cdiv(per_image, 4), n_cur), dim3(256), 0, st, d, tl, open, snk, dist, w.rl_list[0], w.rl_flag[0],
                                     w.rl_flag[1], rl_cnt, ctl.active, lmax_row(round), n_open, w.ring, w.aq, partial ? 0 : (int)n_rt,
                                     round > 0 ? lmax_row(round - 1) : no_prev, kn.mf_label_slack, ex, w.parked);
        else hipLaunchKernelGGL(k_mf_rinit<false>, dim3(cdiv(per_image, 4), n_cur), dim3(256), 0, st, d, tl, open, snk, dist, w.rl_list[0], w.rl_flag[0],
                                w.rl_flag[1], rl_cnt, ctl.active, lmax_row(round), n_open, w.ring, w.aq, partial ? 0 : (int)n_rt,
                                no_prev, -1, ex, w.parked);
        int phase = 0;
        for (; phase < kn.mf_relax_dense; ++phase) {
            int32_t *li = w.rl_list[phase & 1], *lo = w.rl_list[(phase + 1) & 1], *fi = w.rl_flag[phase & 1], *fo = w.rl_flag[(phase + 1) & 1];
            if (prof) hipLaunchKernelGGL(k_mf_relax_wave<true>, dim3(grid), dim3(256), 0, st, d, tl, phase, prof, rmask, w.dirty, rc, dist, rl_cnt, li, lo, fi, fo);
            else hipLaunchKernelGGL(k_mf_relax_wave<false>, dim3(grid), dim3(256), 0, st, d, tl, phase, prof, rmask, w.dirty, rc, dist, rl_cnt, li, lo, fi, fo);
        }
        launches = phase;
        if (partial) return GGC_OK;
        // (pool size: 512 waves per 64 open images; a lane alone runs the same with 128 or 2048 — the launch is a latency
        // chain, not throughput — and four lanes with larger pools lose to each other's waiting waves: 56.6 -> 58.9 -> 62.8 ms)
        const int pool = (int)std::min<size_t>(ASYNC_GRID * scale, std::max<size_t>(16, cdiv((size_t)n_cur * per_image, 16)));
        launches = phase + 1;
        return maxflow_relax_async(ctx, st, d, tl, rmask, w.dirty, rc, dist, rl_cnt + phase % 3, w.rl_list[phase & 1], w.rl_flag[phase & 1],
                                   w.ring, w.aq, (int)n_rt, pool, ctl.err, prof);
    }

    // Push phase over the push tiles the active scan listed.  n_cur: the images open when the round began (the grids follow
    // them).  A sparse round is one asynchronous launch that chases the excess from tile to tile (chains of at most
    // GGC_MF_ASYNC_HOPS hops); `waves` is its pool, 0 for a dense round of launches over work lists.
    int push(int round, int n_cur, size_t scale, int total_active, int& waves) {
        const Knobs& kn = knobs();
        ProfScope ps(ctx, st, "maxflow_push");
        if (round > 0 && total_active <= kn.mf_async_push_active) {
            waves = (int)std::min<long long>(4ll * ASYNC_GRID * (long long)scale, std::max<long long>(64, total_active / 4));
            return maxflow_push_async(ctx, st, d, tl, kn.mf_async_tile, kn.mf_async_sweeps, kn.mf_async_hops, lmax_row(round), kn.mf_label_slack, rc, ex, snk, dist, rmask, w.dirty,
                                      pr_cnt, w.pt_list[0], (int)n_pt, w.busy, w.ring, w.aq, waves, ctl.err, prof);
        }
        waves = 0;
        // dense round.  First round: labels go stale fastest while most excess is still moving, an early relabel pays
        // (8 launches vs 12: +3 %); sweeps per visit: 12 under the label ceiling (8 before it; profiles/r24_label_ceiling.txt).
        const int launches = round == 0 ? kn.mf_dense_launches0 : kn.mf_dense_launches;
        const int pr_grid = (int)std::min<size_t>(PUSH_GRID * scale, std::max<size_t>(64, (size_t)n_cur * tl.pt_x * tl.pt_y / 2));
        // an active pixel opens at most its own tile: empty blocks only add dispatch time to launches that are pure latency
        const int grid = (int)std::min<long long>(pr_grid, std::max<long long>(128, 2ll * total_active));
        for (int phase = 0; phase < launches; ++phase) {
            int32_t *li = w.pt_list[phase & 1], *lo = w.pt_list[(phase + 1) & 1], *fi = w.pt_flag[phase & 1], *fo = w.pt_flag[(phase + 1) & 1];
#if GGC_MF_PUSH_WAVE
            // a block visits four tiles at a time
            const int grid_w = std::max(32, cdiv(grid, PUSH_WAVE_GRID_DIV));
            if (prof) hipLaunchKernelGGL(k_mf_pr_wave<true>, dim3(grid_w), dim3(256), 0, st, d, tl, phase, kn.mf_dense_sweeps, lmax_row(round), kn.mf_label_slack, prof, rc, ex, snk, dist, rmask, w.dirty, pr_cnt, li, lo, fi, fo);
            else hipLaunchKernelGGL(k_mf_pr_wave<false>, dim3(grid_w), dim3(256), 0, st, d, tl, phase, kn.mf_dense_sweeps, lmax_row(round), kn.mf_label_slack, prof, rc, ex, snk, dist, rmask, w.dirty, pr_cnt, li, lo, fi, fo);
#else
            hipLaunchKernelGGL(k_mf_pr_list, dim3(grid), dim3(PT_N), 0, st, d, tl, phase, kn.mf_dense_sweeps, lmax_row(round), kn.mf_label_slack, rc, ex, snk, dist, rmask, w.dirty, pr_cnt, li, lo, fi, fo);
#endif
        }
        GGC_LAUNCH_CHECK(ctx);
        return GGC_OK;
    }
};

// GGC_MF_TRACE=1: per-round diagnostics on stderr, blocking (tools/mf_trace.py reads them).  The clocks of the relabel
// visits are table 1 of the trace clocks (dense launches) and table 2 (asynchronous launch), those of an asynchronous push
// tables 0 (per wave) and 1 (inside the visit), those of a dense push round's visits table 3.
struct MfTrace {
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    double push_ms = 0.0;

    // after the active scan: the relabel visits' clocks, active pixels and open images, the stragglers by image
    int round(const MfSolve& s, int round, int n_next, int total_active, int relax_launches) {
        ggc_ctx* ctx = s.ctx;
        long long hh[128 * 8];
        GGC_HIP(ctx, hipStreamSynchronize(s.st));
        GGC_HIP(ctx, hipMemcpy(hh, s.prof + 64 * 8, sizeof hh, hipMemcpyDeviceToHost));
        GGC_HIP(ctx, hipMemsetAsync(s.prof + 64 * 8, 0, sizeof hh, s.st));
        long long n_wrong = 0, n_parked = 0;               // slot 7 of the two tables' rows: the active scan's count of parked excess
        for (int i = 0; i < 64; ++i) { n_wrong += hh[i * 8 + 7]; n_parked += hh[(64 + i) * 8 + 7]; }
        for (int t = 0; t < 2; ++t) {                      // dense launches | the asynchronous launch (write-back includes its hand-over)
            long long h[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 64; ++i) for (int k = 0; k < 7; ++k) h[k] += hh[(t * 64 + i) * 8 + k];
            if (h[3] > 0)
                std::fprintf(stderr, "    [%s] %lld %s visits: per visit load+fill %.2f us, sweeps %.2f us (%.1f sweeps, %.1f BFS levels, %lld visits fell back), write-back %.2f us\n",
                             t ? "async relabel visits" : "relabel visits", h[3], t ? "asynchronous" : "dense", 0.01 * h[0] / h[3], 0.01 * h[1] / h[3],
                             (double)h[4] / h[3], (double)h[5] / h[3], h[6], 0.01 * h[2] / h[3]);
        }
        std::vector<int32_t> act;
        if (int rcode = read_i32(ctx, s.st, s.ctl.active, s.d.B, act)) return rcode;
        const auto t_now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t_now - t_prev).count();
        std::fprintf(stderr, "[ggc maxflow] round %d: open images %d, active pixels %d, relabel launches %d, relabel+scan %.3f ms, previous push %.3f ms\n",
                     round, n_next, total_active, relax_launches, ms - push_ms, push_ms);
        t_prev = t_now;
        if (n_next > 0 && n_next <= 12) {
            std::fprintf(stderr, "    [open]");
            for (int b = 0; b < s.d.B; ++b) if (act[b]) std::fprintf(stderr, " %d:%d", b, act[b]);
            std::fprintf(stderr, "\n");
        }
        // the label ceiling: the largest finite label of the images still open (k_mf_active), and what the relabel made of the
        // excess the previous push phase parked at or above its ceiling
        std::vector<int32_t> lm;
        if (int rcode = read_i32(ctx, s.st, s.lmax_row(round), s.d.B * MF_LMAX_STRIDE, lm)) return rcode;
        int lo = 0, hi = 0, n_l = 0; long long sum = 0;
        for (int b = 0; b < s.d.B; ++b) if (act[b]) { const int l = lm[(size_t)b * MF_LMAX_STRIDE]; lo = n_l ? std::min(lo, l) : l; hi = std::max(hi, l); sum += l; ++n_l; }
        std::fprintf(stderr, "    [ceiling] slack %d, lmax of %d open images: min %d, mean %.1f, max %d; parked pixels with excess %lld, of them finite after the relabel %lld\n",
                     knobs().mf_label_slack, n_l, lo, n_l ? (double)sum / n_l : 0.0, hi, n_parked, n_wrong);
        if (n_next > 0 && n_next <= 12) {
            std::fprintf(stderr, "    [lmax]");
            for (int b = 0; b < s.d.B; ++b) if (act[b]) std::fprintf(stderr, " %d:%d", b, lm[(size_t)b * MF_LMAX_STRIDE]);
            std::fprintf(stderr, "\n");
        }
        return GGC_OK;
    }

    // after a push phase: its time, and where the waves of an asynchronous one (waves > 0) spent it
    int push(const MfSolve& s, int waves) {
        ggc_ctx* ctx = s.ctx;
        GGC_HIP(ctx, hipStreamSynchronize(s.st));
        push_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_prev).count();
        if (waves == 0) {                                  // a dense round: the visits of k_mf_pr_wave, table 3 (nothing with k_mf_pr_list)
            long long hd[64 * 8], v[6] = {0, 0, 0, 0, 0, 0};
            GGC_HIP(ctx, hipMemcpy(hd, s.prof + 192 * 8, sizeof hd, hipMemcpyDeviceToHost));
            GGC_HIP(ctx, hipMemsetAsync(s.prof + 192 * 8, 0, sizeof hd, s.st));
            for (int i = 0; i < 64; ++i) for (int k = 0; k < 6; ++k) v[k] += hd[i * 8 + k];
            if (v[3] > 0)
                std::fprintf(stderr, "    [dense push visits] %lld visits: per visit load+fill %.2f us, sweeps %.2f us (%.2f sweeps, %.2f with a deal), write-back+hand-over %.2f us\n",
                             v[3], 0.01 * v[0] / v[3], 0.01 * v[1] / v[3], (double)v[4] / v[3], (double)v[5] / v[3], 0.01 * v[2] / v[3]);
            return GGC_OK;
        }
        long long hh[128 * 8], h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, n_idle = 0, l_high = 0;
        GGC_HIP(ctx, hipMemcpy(hh, s.prof, sizeof hh, hipMemcpyDeviceToHost));
        GGC_HIP(ctx, hipMemsetAsync(s.prof, 0, sizeof hh, s.st));
        for (int i = 0; i < 64; ++i) for (int k = 0; k < 8; ++k) h[k] += hh[i * 8 + k];
        for (int i = 0; i < 64; ++i) for (int k = 0; k < 3; ++k) g[k] += hh[(64 + i) * 8 + k];
        for (int i = 0; i < 64; ++i) { n_idle += hh[(64 + i) * 8 + 3]; l_high = std::max(l_high, hh[(64 + i) * 8 + 4]); }
        if (h[3] > 0)
            std::fprintf(stderr, "    [async visit] load+fill %.2f us, sweeps %.2f us (%.1f sweeps), write-back+drain %.2f us\n", 0.01 * g[0] / h[3],
                         0.01 * g[1] / h[3], (double)g[2] / h[3], 0.01 * (h[1] - g[0] - g[1]) / h[3]);
        if (h[6] > 0)
            std::fprintf(stderr, "    [async push] %d waves alive %.1f us on average; %lld visits (%lld followed): per visit wait+lock %.2f us, "
                         "visit %.2f us, hand-over %.2f us; chains cut by the hop limit %lld, ended with nothing to hand on %lld, highest label written %lld\n",
                         waves, 0.01 * h[5] / h[6], h[3], h[4], h[3] ? 0.01 * h[0] / h[3] : 0.0,
                         h[3] ? 0.01 * h[1] / h[3] : 0.0, h[3] ? 0.01 * h[2] / h[3] : 0.0, h[7], n_idle, l_high);
        return GGC_OK;
    }
};

} // namespace

int maxflow(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const int32_t* state, int32_t* rc, int32_t* ex,
            int32_t* snk, int32_t* dist, uint8_t* rmask, const MfControl& ctl, bool masks_exact, int& n_open) {
    const Knobs& kn = knobs();
    const MfTiles tl{cdiv(d.W, RT), cdiv(d.H, RT), cdiv(d.W, PT_W), cdiv(d.H, PT_H)};
    MfSolve s{ctx, st, d, tl, (size_t)tl.rt_x * tl.rt_y * d.B, (size_t)tl.pt_x * tl.pt_y * d.B, rc, ex, snk, dist, rmask,
              ctl, ctl.cnt, ctl.cnt + 1, ctl.cnt + 4, {}, nullptr};
    GGC_REQUIRE(ctx, std::max(s.n_rt, s.n_pt) < (1u << 24), GGC_E_UNSUPPORTED, "batch has more max-flow tiles than a queue entry addresses");
    if (!carve_scratch(ctx, S_GC_M, [&](Carve& c) { s.w.layout(c, s.n_rt, s.n_pt, (size_t)d.B, kn.mf_trace ? (size_t)d.B * d.P : 0); })) return GGC_E_OOM;
    // k_build_graph writes exact masks for every pixel on a cold start; a warm start leaves capacities and masks alone, so
    // the tiles keep their dirty marks
    if (masks_exact) GGC_HIP(ctx, hipMemsetAsync(s.w.dirty, 0, sizeof(int32_t) * s.n_pt, st));
    if (kn.mf_trace) {
        s.prof = s.w.prof;
        GGC_HIP(ctx, hipMemsetAsync(s.prof, 0, MF_PROF_TABLES * 64 * 8 * sizeof(long long), st));
    }
    GGC_HIP(ctx, hipMemsetAsync(s.n_open, 0, sizeof(int32_t), st));
    int32_t *list_cur = ctl.lists, *list_nxt = ctl.lists + d.B;
    hipLaunchKernelGGL(k_open_init, dim3(cdiv(d.B, 256)), dim3(256), 0, st, d.B, state, list_cur, s.n_open, s.rl_cnt);
    GGC_LAUNCH_CHECK(ctx);
    std::vector<int32_t> host;
    int rcode = GGC_OK;
    if (n_open < 0) {                   // the first solve of a call: the later ones know the count and do not wait here
        if ((rcode = read_i32(ctx, st, s.n_open, 1, host))) return rcode;
        n_open = host[0];
    }
    int n_cur = n_open;
    if (n_cur == 0) return GGC_OK;
    MfTrace trace;
    const int max_rounds = 4096;
    for (int round = 0; round < max_rounds; ++round) {
        // Blocks walk their share of a list and load the next tile while they work on the current one, so a block should own
        // several tiles: the grid caps are per 64 open images (one GrabCut lane) and grow with the batch a call is given.
        // Late rounds (a handful of open images) are pure launch latency, and empty blocks add to it: never more blocks than tiles.
        const size_t scale = std::max<size_t>(1, ((size_t)n_cur + 32) / 64);
        // The first rounds relabel PARTIALLY: only the work-list launches, without the asynchronous launch that follows the
        // front to its fixpoint.  Labels steer the pushes, they do not have to be exact for the result to be: whatever labels
        // a push phase sees, it turns a valid preflow into a valid preflow, and the cut is read off the EXACT relabel that
        // ends the solve.  A pixel the front has not reached keeps "infinity" for this round — its excess waits (deep inside
        // an object most of it is trapped anyway) — so an image is never closed on a partial relabel, and the round that
        // decides "no active pixel left" is always a full one.  Measured: 57.7 -> 52.9 ms per GrabCut stage (batch 256).
        const bool partial = round < kn.mf_partial_rounds;
        int relax_launches = 0;
        if ((rcode = s.relabel(list_cur, round, n_cur, scale, partial, relax_launches))) return rcode;
        // ---- who still has work?  (active pixel = excess that can still reach the sink)
        // (active[], the open-image count, the push-list counters and the active total were zeroed by this round's k_mf_rinit)
        int32_t* aq_st = maxflow_push_async_tile(kn.mf_async_tile) == PT_H ? s.w.busy : nullptr;
        const dim3 scan_grid(std::min(cdiv(tl.pt_x * tl.pt_y, 4), 128), n_cur);
        if (s.prof) hipLaunchKernelGGL(k_mf_active<true>, scan_grid, dim3(256), 0, st, d, tl, list_cur, ex, dist, ctl.active, s.lmax_row(round), s.w.pt_flag[0],
                                       s.w.pt_flag[1], s.w.pt_list[0], s.pr_cnt, aq_st, s.w.ring, s.w.aq, (int)s.n_pt, s.w.parked, s.prof);
        else hipLaunchKernelGGL(k_mf_active<false>, scan_grid, dim3(256), 0, st, d, tl, list_cur, ex, dist, ctl.active, s.lmax_row(round), s.w.pt_flag[0],
                                s.w.pt_flag[1], s.w.pt_list[0], s.pr_cnt, aq_st, s.w.ring, s.w.aq, (int)s.n_pt, s.w.parked, s.prof);
        hipLaunchKernelGGL(k_done_update, dim3(cdiv(n_cur, 256)), dim3(256), 0, st, n_cur, list_cur, ctl.active, list_nxt, s.n_open, partial ? 1 : 0, s.rl_cnt);
        GGC_LAUNCH_CHECK(ctx);
        if ((rcode = read_i32(ctx, st, s.n_open, 8, host))) return rcode;
        const int n_next = host[0], total_active = host[7];
        if (kn.mf_trace && (rcode = trace.round(s, round, n_next, total_active, relax_launches))) return rcode;
        if (n_next == 0) return GGC_OK;
        std::swap(list_cur, list_nxt);
        int waves = 0;
        if ((rcode = s.push(round, n_cur, scale, total_active, waves))) return rcode;
        if (kn.mf_trace && (rcode = trace.push(s, waves))) return rcode;
        n_cur = n_next;
    }
    return set_err(ctx, GGC_E_DEVICE, "max-flow did not converge in %d rounds", max_rounds);
}

} // namespace ggc
