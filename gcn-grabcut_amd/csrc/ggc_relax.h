// ggc_relax.h — the tile relaxation shared by ggc_geodesic.hip and ggc_scissors.hip.
//
// Both entries want the unique fixed point of d(p) = min(d(p), min_q d(q) + c(p,q)) in int32 on the 8-connected pixel grid.
// It does not depend on the order in which tiles or pixels are relaxed, so the work goes by 32x32 tiles in rounds: one
// launch per round, one 256-lane workgroup per listed tile (grid-stride).  A visit has the PLANES distance planes of tile +
// one-pixel halo in LDS (staged by the caller, who knows where they live and what the halo holds outside its domain), the
// four arc-cost tables of the tile (relax_arcs: E, S, SE, SW; the other four arcs are the same tables read from the
// neighbour; an arc with an end outside the domain costs RX_BLOCKED), and relaxes to the tile's fixed point against the
// fixed halo (relax_visit): alternating column and row sweeps in which a lane walks a run of pixels forwards and backwards
// in place, so a front crosses the tile in a few sweeps.  Lowered pixels go back with plain stores; a lowered border pixel
// puts the tiles that see it in their halo on the next round's list (relax_list_neighbours; a stamp per tile keeps a tile
// from being listed twice, integer atomics only).  A tile read by a neighbour in the same launch may show the old or the
// new value: either is a valid upper bound, and the lowering lists that neighbour for the next round, where the kernel
// boundary makes it visible.  A visit reports only the pixels it lowers itself, so whoever writes a source into a plane
// lists the source's tile and every tile that holds it in its halo (relax_tiles_holding).
//
// Lanes.  256 / PLANES lanes per plane, plane = tid / (256 / PLANES); within a plane 8 / PLANES runs of RUN = 4 * PLANES
// pixels on each of 32 lines, run = (tid / 32) % (8 / PLANES), line = tid % 32.  Each 32-lane half of a wave holds one run
// index and 32 lines: conflict-free at the odd stride RX_S in both directions, every pixel has one writer per sweep, and no
// lane idles (PLANES = 2: 2 x 4 runs of 8; PLANES = 1: 8 runs of 4, where runs of 8 would leave half the lanes without work).
//
// Round bound (relax_rounds).  Round j makes every pixel final whose shortest path crosses a tile edge at most j times: the
// path's last crossing leaves a pixel that became final in a round before j, and the lowering that made it final listed the
// tile entered for the following round, whose visit runs to the tile's fixed point and so covers the rest of the path.  If
// no shortest path crosses more than J edges, round J + 1 can still be listed (by the lowerings of round J) but lowers
// nothing: the list of round J + 2 is empty, and J + 2 rounds bound the call.  A simple path has fewer arcs than its
// domain has pixels, at most 1024 per tile, so J <= 1024 * tiles - 1; each caller states its own J.
#pragma once
#include "ggc_internal.h"
#include <algorithm>

namespace ggc {

constexpr int RX_T = 32, RX_H = RX_T + 2;            // tile edge, with halo
constexpr int RX_S = RX_H + 1;                       // LDS row stride: odd, so that a row sweep's 32 rows fall into 32 banks
constexpr int RX_N = RX_H * RX_S;
constexpr int RX_THREADS = 256;
constexpr int RX_AXIAL = 80, RX_DIAG = 113;          // step lengths, 80 * sqrt(2) = 113.14
// An arc with an end outside the domain.  It never lowers anything: the caller stages a value h for the halo outside its
// domain such that h + RX_BLOCKED is no smaller than any stored distance, and keeps stored distances at or below 2^30, so
// that a sum with RX_BLOCKED fits int32.
constexpr int RX_BLOCKED = 1 << 29;
// A sweep relaxes every pixel against all 8 neighbours, so a sweep that changes something makes at least one more pixel of
// the tile final (the unsettled pixel of smallest final value): 1024 sweeps settle a plane, one more sees no change.
constexpr int RX_MAX_SWEEPS = RX_T * RX_T + 1;

template <int PLANES>
struct RelaxLds {
    int c[4][RX_N];              // arc (y,x) -> (y,x+1), (y+1,x), (y+1,x+1), (y+1,x-1)
    int d[PLANES][RX_N];
    int nbm;
};

// The work lists of a call.  cnt has three words; the callers' fourth counters are their own.
struct RelaxLists {
    int32_t* stamp;              // per tile: 1 + the round it is listed for, 0 = never listed by relax_enqueue
    int32_t* list[2];            // ping-pong: round r reads list[r & 1]
    int32_t* cnt;                // list lengths of rounds r, r+1, r+2 at [r % 3], [(r+1) % 3], [(r+2) % 3]
    int32_t* touched;            // null, or every tile that was ever listed, once,
    int32_t* n_touched;          //          and the length of that list: both null or both set
};

// One round's view of the lists: the list it reads and where a visit lists tiles for the next round.
struct RelaxRound { const int32_t* cur; int n; int32_t* nxt; int32_t* cnt_next; int stamp_next; };

// The round's prologue, called by every lane of the launch.  The length is read before the store: a load after a store
// that may alias it cannot be a scalar load, and most workgroups of a launch only read the length and leave.
__device__ __forceinline__ RelaxRound relax_round_begin(const RelaxLists& w, int round) {
    const RelaxRound rr{w.list[round & 1], w.cnt[round % 3], w.list[(round + 1) & 1], &w.cnt[(round + 1) % 3], round + 2};
    if (blockIdx.x == 0 && threadIdx.x == 0) w.cnt[(round + 2) % 3] = 0;   // read by the previous launch, appended to by the next
    return rr;
}

// lists `tile` on `list` (of length *cnt) for the round whose stamp is `stamp`, once; round 0's stamp is 1
__device__ __forceinline__ void relax_enqueue(const RelaxLists& w, int tile, int stamp, int32_t* list, int32_t* cnt) {
    const int old = atomicExch(&w.stamp[tile], stamp);
    if (old == stamp) return;
    list[atomicAdd(cnt, 1)] = tile;
    if (w.touched && old == 0) w.touched[atomicAdd(w.n_touched, 1)] = tile;
}

// Calls f(ny, nx) for the tile (tyi, txi) of the pixel at (ly, lx) inside it and for each neighbour tile of the
// tiles_y x tiles_x grid that holds the pixel in its halo.
template <class F>
__host__ __device__ inline void relax_tiles_holding(int tyi, int txi, int ly, int lx, int tiles_y, int tiles_x, F f) {
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const bool sees = (dy == 0 || (dy < 0 ? ly == 0 : ly == RX_T - 1)) && (dx == 0 || (dx < 0 ? lx == 0 : lx == RX_T - 1));
            const int ny = tyi + dy, nx = txi + dx;
            if (sees && ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) f(ny, nx);
        }
}

// The caller's domain inside the 34x34 halo window of a tile, as inclusive halo coordinates clipped to [0, RX_H - 1]:
// computed once per tile, so that "this halo position lies in the domain" is four compares against block-uniform values.
struct RelaxBox {
    int y_lo, y_hi, x_lo, x_hi;
    __device__ __forceinline__ bool has(int hy, int hx) const { return hy >= y_lo && hy <= y_hi && hx >= x_lo && hx <= x_hi; }
};
// The box of the tile whose first pixel is (ty0, tx0) in a domain of h x w pixels (halo position 0 is pixel ty0 - 1).
__device__ __forceinline__ RelaxBox relax_box(int ty0, int tx0, int h, int w) {
    return RelaxBox{max(1 - ty0, 0), min(h - ty0, RX_H - 1), max(1 - tx0, 0), min(w - tx0, RX_H - 1)};
}

// The four arc tables of tile + halo.  cost(j, q, len): the arc between the LDS indices j and q, both inside the box, of
// step length len.  An arc's far end lies below or beside its near end (oy >= 0), so with the near end inside only the
// far end's upper row bound and its column bounds are left to test.  The caller's guide arrays are visible (a barrier
// since they were staged); a barrier must follow before relax_visit.
template <int PLANES, class Cost>
__device__ __forceinline__ void relax_arcs(RelaxLds<PLANES>& L, const RelaxBox& box, Cost cost) {
    for (int i = threadIdx.x; i < RX_H * RX_H; i += RX_THREADS) {
        const int hy = i / RX_H, hx = i - hy * RX_H, j = hy * RX_S + hx;
        const bool in = box.has(hy, hx);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int oy = a == 0 ? 0 : 1, ox = a == 0 ? 1 : (a == 1 ? 0 : (a == 2 ? 1 : -1));
            const bool ok = in && hy + oy <= box.y_hi && hx + ox >= box.x_lo && hx + ox <= box.x_hi;
            L.c[a][j] = ok ? cost(j, j + oy * RX_S + ox, a < 2 ? RX_AXIAL : RX_DIAG) : RX_BLOCKED;
        }
    }
}

// relaxes the pixel at LDS index i against its 8 neighbours; returns the new value
__device__ __forceinline__ int relax_pixel(const int* dd, const int (&c)[4][RX_N], int i) {
    const int a = min(min(dd[i - 1] + c[0][i - 1], dd[i + 1] + c[0][i]),
                      min(dd[i - RX_S] + c[1][i - RX_S], dd[i + RX_S] + c[1][i]));
    const int e = min(min(dd[i - RX_S - 1] + c[2][i - RX_S - 1], dd[i + RX_S + 1] + c[2][i]),
                      min(dd[i - RX_S + 1] + c[3][i - RX_S + 1], dd[i + RX_S - 1] + c[3][i]));
    return min(dd[i], min(a, e));
}

// A lane owns RUN consecutive pixels of one column (step = RX_S) or one row (step = 1) of one plane and walks them there
// and back, in place.  Pixels of other lanes are read while their owners may lower them: any value seen is the cost of a
// real path, values only fall, and the sweep that ends the visit changed nothing, so all its reads saw final values.
template <int RUN>
__device__ __forceinline__ bool relax_sweep(int* dd, const int (&c)[4][RX_N], int first, int step) {
    bool changed = false;
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
        const int i = first + k * step, v = relax_pixel(dd, c, i);
        if (v != dd[i]) { dd[i] = v; changed = true; }
    }
#pragma unroll
    for (int k = RUN - 2; k >= 0; --k) {
        const int i = first + k * step, v = relax_pixel(dd, c, i);
        if (v != dd[i]) { dd[i] = v; changed = true; }
    }
    return changed;
}

// The visit, called by every lane of the workgroup with L.c and L.d visible: relaxes the tile to its fixed point and
// calls store(plane, ly, lx, v) for every lowered pixel of the tile (a pixel outside the domain never changes: its arcs
// are blocked).  Returns which of the tile's edges and corners had a lowered pixel, bit (dy + 1) * 3 + (dx + 1), the same
// in every lane; L is free to be staged again on return.
template <int PLANES, class Store>
__device__ __forceinline__ int relax_visit(RelaxLds<PLANES>& L, Store store) {
    static_assert(PLANES >= 1 && 8 % PLANES == 0, "8 / PLANES runs of 4 * PLANES pixels make a line of 32");
    constexpr int RUN = 4 * PLANES;
    const int tid = threadIdx.x;
    if (tid == 0) L.nbm = 0;
    // write-back ownership: rows tid / 32 + 8k of column tid % 32 (coalesced)
    const int wx = tid & 31, wy = tid >> 5;
    int old[PLANES][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < PLANES; ++q) old[q][k] = L.d[q][(wy + 8 * k + 1) * RX_S + wx + 1];
    __syncthreads();                                                       // the sweeps write what other lanes just read
    int* dd = L.d[tid / (RX_THREADS / PLANES)];
    const int run = (tid >> 5) % (8 / PLANES), line = tid & 31;
    const int first_v = (RUN * run + 1) * RX_S + line + 1, first_h = (line + 1) * RX_S + RUN * run + 1;
    for (int it = 0; it < RX_MAX_SWEEPS; ++it) {
        const bool ch = (it & 1) ? relax_sweep<RUN>(dd, L.c, first_h, 1) : relax_sweep<RUN>(dd, L.c, first_v, RX_S);
        if (!__syncthreads_or(ch)) break;
    }
    int nbm = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = wy + 8 * k, j = (ly + 1) * RX_S + wx + 1;
#pragma unroll
        for (int q = 0; q < PLANES; ++q) {
            const int v = L.d[q][j];
            if (v != old[q][k]) {
                store(q, ly, wx, v);
                const int Lf = wx == 0, Rt = wx == RX_T - 1, U = ly == 0, D = ly == RX_T - 1;
                nbm |= (U & Lf) | U << 1 | (U & Rt) << 2 | Lf << 3 | Rt << 5 | (D & Lf) << 6 | D << 7 | (D & Rt) << 8;
            }
        }
    }
    if (nbm) atomicOr(&L.nbm, nbm);
    __syncthreads();
    nbm = L.nbm;
    __syncthreads();                                                       // the next visit clears L.nbm
    return nbm;
}

// After a visit: lanes 0..8 list the neighbour tiles named by nbm for the next round.  The tile is (tyi, txi) of a
// tiles_y x tiles_x grid whose tiles are numbered row-major from tile0.
__device__ __forceinline__ void relax_list_neighbours(const RelaxLists& w, const RelaxRound& rr, int nbm, int tyi, int txi,
                                                      int tiles_y, int tiles_x, int tile0) {
    const int tid = threadIdx.x;
    if (tid < 9 && tid != 4 && ((nbm >> tid) & 1)) {
        const int ny = tyi + tid / 3 - 1, nx = txi + tid % 3 - 1;
        if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) relax_enqueue(w, tile0 + ny * tiles_x + nx, rr.stamp_next, rr.nxt, rr.cnt_next);
    }
}

// The host's round loop: launch_round(r) for r = 0, 1, ... on st; the length of the next list (cnt, the lists' three
// counters) is read back after first_look rounds and then every `stride`, and an empty one ends the call.  max_rounds is
// the caller's J + 2 of the header comment; past it the call fails as "<what> did not converge".
template <class Launch>
inline int relax_rounds(ggc_ctx* ctx, hipStream_t st, Launch launch_round, const int32_t* cnt, int first_look, int stride,
                        int64_t max_rounds, const char* what) {
    int64_t round = 0;
    int step = first_look;
    std::vector<int32_t> host;
    for (;;) {
        const int64_t stop = std::min(round + step, max_rounds);
        for (; round < stop; ++round) launch_round(round);
        GGC_LAUNCH_CHECK(ctx);
        if (int rc = read_i32(ctx, st, cnt + round % 3, 1, host)) return rc;
        if (host[0] == 0) return GGC_OK;
        GGC_REQUIRE(ctx, round < max_rounds, GGC_E_DEVICE, "%s did not converge in %lld rounds", what, (long long)max_rounds);
        step = stride;
    }
}

} // namespace ggc
