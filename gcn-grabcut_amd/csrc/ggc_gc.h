// ggc_gc.h — shared between ggc_grabcut.hip (GMMs, graph construction) and
// ggc_maxflow.hip (integer push-relabel on the implicit 8-neighbour grid).
#pragma once
#include "ggc_internal.h"

namespace ggc {

constexpr int DINF = 1 << 29;      // "cannot reach the sink"

struct GcDims { int B, H, W, P, n_chunks; };

// directions: 0 left, 1 right, 2 up, 3 down, 4 up-left, 5 down-right, 6 up-right, 7 down-left; rev(dir) = dir ^ 1
__device__ __forceinline__ int dir_dx(int dir) { return (dir == 0 || dir == 4 || dir == 7) ? -1 : ((dir == 1 || dir == 5 || dir == 6) ? 1 : 0); }
__device__ __forceinline__ int dir_dy(int dir) { return (dir == 2 || dir == 4 || dir == 6) ? -1 : ((dir == 3 || dir == 5 || dir == 7) ? 1 : 0); }
__device__ __forceinline__ int dir_nb(const GcDims& d, int y, int x, int dir) {
    const int yy = y + dir_dy(dir), xx = x + dir_dx(dir);
    if (xx < 0 || xx >= d.W || yy < 0 || yy >= d.H) return -1;
    return yy * d.W + xx;
}

// Residual capacities: [B * P][8] — the 8 arcs of a pixel are contiguous (one 32-byte sector).  Every consumer reads all 8
// of a pixel (push visits, arc masks), and the relabel's column reads (arcs that leave a push tile sideways, one pixel per
// image row) then touch one line per row instead of three; as 8 planes [8][B * P] those column reads were 6 us of a 22 us
// relabel visit.
__host__ __device__ __forceinline__ size_t rc_idx(int dir, size_t i) { return i * 8 + (size_t)dir; }

// One pixel of the network, the per-pixel part of graph construction (ggc_grabcut's k_build_graph, ggc_grid_maxflow's
// k_gf_build).  Cold: the 8 residual arcs from their capacities cap[dir] (0 for an arc that leaves the image), the arc
// mask, and the terminal balance of the t-link difference tw (source minus sink).
__device__ __forceinline__ void mf_cold_pixel(size_t i, int32_t tw, const int32_t (&cap)[8], int32_t* __restrict__ rc,
                                              int32_t* __restrict__ ex, int32_t* __restrict__ snk, uint8_t* __restrict__ rmask) {
    int arcs = 0;                                        // bit dir = residual arc towards dir (the push visits of ggc_maxflow*.hip keep it current)
    int4* r = reinterpret_cast<int4*>(rc + rc_idx(0, i));   // the 8 arcs of a pixel: one aligned 32-byte sector
    r[0] = make_int4(cap[0], cap[1], cap[2], cap[3]);
    r[1] = make_int4(cap[4], cap[5], cap[6], cap[7]);
#pragma unroll
    for (int dir = 0; dir < 8; ++dir) arcs |= cap[dir] > 0 ? 1 << dir : 0;
    rmask[i] = (uint8_t)arcs;
    ex[i] = tw > 0 ? tw : 0;
    snk[i] = tw < 0 ? -tw : 0;
}

// Capacities of a pixel's 8 arcs from the n-link planes nw [4][B][P] (0 left, 1 up-left, 2 up, 3 up-right; a link that
// points outside the image is ignored): own planes give the arcs towards left / up-left / up / up-right, the mirrored arcs
// read the neighbour's plane.
__device__ __forceinline__ void mf_plane_caps(const GcDims& d, int b, int p, const int32_t* __restrict__ nw, int32_t (&cap)[8]) {
    const size_t BP = (size_t)d.B * d.P;
    const int y = p / d.W, x = p % d.W;
    const int32_t* nwb = nw + (size_t)b * d.P;
    const int dirs[4] = {0, 4, 2, 6};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dir = dirs[k];
        cap[dir] = dir_nb(d, y, x, dir) >= 0 ? nwb[(size_t)k * BP + p] : 0;
        const int q = dir_nb(d, y, x, dir ^ 1);
        cap[dir ^ 1] = q >= 0 ? nwb[(size_t)k * BP + q] : 0;
    }
}

// Warm start (dynamic graph cuts): only the t-links change between solves, and adding a constant to both t-links of a
// pixel never changes the cut, so the old n-link flow stays a valid preflow: the pixel's new terminal balance is its
// t-link difference plus what its neighbours sent it, tw + sum (residual - capacity).  That sum is already in memory:
// every push moves one amount in ex and in the two arcs of its link, a push to the sink lowers ex and snk together, so at
// any kernel boundary ex - snk = tw_old + sum (residual - capacity), and the new balance is (ex - snk) + (tw - tw_old),
// the same integers.  Capacities and arc masks stay: the push visits keep rmask current for the arcs inside their tile and
// the tiles' dirty words cover arcs re-opened from a neighbouring tile (ggc_mf_sweep.h).
// Bounds: |tw| <= 2^27 and 8 capacities <= 2^24 each give |ex - snk| <= 2^27 + 8 * 2^24 = 2^28 (< 3 * 2^27), and
// |tw - tw_old| <= 2^28, so the new balance stays within 2^29 in int32.
// ex_old, snk_old: the pixel's words as loaded by the caller (k_build_graph issues them with its other loads)
__device__ __forceinline__ void mf_warm_pixel(size_t i, int32_t tw, int32_t tw_old, int32_t ex_old, int32_t snk_old,
                                              int32_t* __restrict__ ex, int32_t* __restrict__ snk) {
    const int32_t bal = (ex_old - snk_old) + (tw - tw_old);
    ex[i] = bal > 0 ? bal : 0;
    snk[i] = bal < 0 ? -bal : 0;
}
__device__ __forceinline__ void mf_warm_pixel(size_t i, int32_t tw, int32_t tw_old, int32_t* __restrict__ ex,
                                              int32_t* __restrict__ snk) {
    mf_warm_pixel(i, tw, tw_old, ex[i], snk[i], ex, snk);
}

// The max-flow's words in ggc_grabcut's control block, which the start of every call zeroes.
struct MfControl {
    int32_t* active;   // [B] active pixels per image (excess that can still reach the sink)
    int32_t* cnt;      // [8] open images | relabel list counters [3] | push list counters [3] | active pixels in total
    int32_t* lists;    // [2B] open-image lists, current and next round
    int32_t* err;      // receives a non-zero code if an asynchronous launch gives up
};

// Maximum preflow + canonical labels for every image with state[b] == 0.
//   rc   [B][P][8] residual capacities (in/out), rc_idx(dir, pixel)     ex, snk [B][P] excess / residual sink capacity (in/out)
//   dist [B][P] out: distance to the sink in the final residual graph, >= DINF when unreachable (=> foreground)
//   rmask [B][P] arc masks of rc (bit dir = residual arc towards dir); masks_exact: every byte is current (cold start) —
//   otherwise the tiles marked dirty by the previous solve of this call keep their mark.
//   n_open: in/out, the number of images with state[b] == 0.  Negative: counted on the device and read back (blocking);
//   state[] does not change between the solves of one call, so the caller hands the first solve's count to the later ones.
int maxflow(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const int32_t* state, int32_t* rc, int32_t* ex,
            int32_t* snk, int32_t* dist, uint8_t* rmask, const MfControl& ctl, bool masks_exact, int& n_open);

// Tile geometry of the max-flow kernels (ggc_maxflow.hip: launches over work lists; ggc_maxflow_async.hip: one launch per sparse phase)
constexpr int MF_RT = 32;                          // relabel tile side
constexpr int MF_PT_W = 32, MF_PT_H = 8;           // push tile
struct MfTiles { int rt_x, rt_y, pt_x, pt_y; };    // tiles per image
// Words between the label-ceiling words of two images (lmax[b * MF_LMAX_STRIDE]): a 128-byte line each.  k_mf_active raises
// an image's word with one atomic per block, about 8 000 per launch at 64 open images; packed into two lines they queue
// behind each other in one L2 channel (measured: the scan 29 -> 47 us).
constexpr int MF_LMAX_STRIDE = 32;

// up to three int32 regions zeroed by one launch on `st` (ggc_maxflow.hip)
void mf_zero3(hipStream_t st, int32_t* a, size_t na, int32_t* b, size_t nb, int32_t* c, size_t nc);

// Sparse phases as one asynchronous launch each (ggc_maxflow_async.hip): a pool of waves over a ticket queue of tiles.
// Queue control words (int32, every hot counter on its own 128-byte line):
constexpr int AQ_HEAD = 0, AQ_TAIL = 32, AQ_PENDING = 64, AQ_DONE = 96, AQ_BUDGET = 97, AQ_VISITS = 128, AQ_WORDS = 160;
// The queue starts with list[0 .. *count) (device-side count; the tiles' membership flags in `flag` are set): ONE launch that
// ends at the relabel's fixpoint.  ring: cap 64-bit slots, cap = number of relabel tiles of the batch; ring and q are zero
// (k_mf_rinit).  prof: the trace clocks under GGC_MF_TRACE (table 2), null otherwise.
int maxflow_relax_async(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const MfTiles& tl, uint8_t* rmask, int32_t* dirty, const int32_t* rc, int32_t* dist,
                        const int32_t* count, const int32_t* list, int32_t* flag, unsigned long long* ring, int32_t* q, int cap,
                        int grid, int32_t* err_flag, long long* prof = nullptr);
// the same for one push phase on 32 x th tiles (th = 8 | 16 | 32): chains of at most gen_max tile hops, at most `inner` sweeps
// per visit.  list: the active scan's 32x8 push tiles (n_list_max = their number in the batch); state: one word per tile.
// th = 8: the list is the queue's start, and the active scan has left ring and q zero and state "queued" (1) for the listed
// tiles, 0 for the others of every open image; th = 16 | 32: a zero-fill and a fill launch go first.
// lmax [B], slack: the images' label ceilings (push_tile_visit, ggc_mf_push.h); slack < 0: none.
int maxflow_push_async_tile(int th);               // the tile height a requested one runs as
int maxflow_push_async(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const MfTiles& tl, int th, int inner, int gen_max, const int32_t* lmax, int slack, int32_t* rc,
                       int32_t* ex, int32_t* snk, int32_t* dist, uint8_t* rmask, int32_t* dirty, const int32_t* count, const int32_t* list, int n_list_max, int32_t* state,
                       unsigned long long* ring, int32_t* q, int waves, int32_t* err_flag, long long* prof = nullptr);

} // namespace ggc
