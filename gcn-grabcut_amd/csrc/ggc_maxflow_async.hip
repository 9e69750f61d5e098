// ggc_maxflow_async.hip — the SPARSE phases of the max-flow of ggc_maxflow.hip as one launch each.
//
// Driven by the host, a sparse phase is a chain of dependent launches: the front of a global relabel crosses one
// tile per launch (12-56 launches per relabel), a unit of excess crosses one tile per push launch (24-64 launches per
// round), and every launch costs a tile visit plus a kernel boundary (~18 us) however little there is to do.  The dense
// phases (the first relabel launches, the first push round) are bandwidth work and stay launches over work lists.
//
// Here the chain runs inside ONE launch, asynchronously: a pool of waves takes tiles from a queue, and a visit that
// changes a neighbour's halo (relabel) or hands excess to a neighbour (push) appends that neighbour to the SAME queue.
// There are no passes, no barriers and no per-image phases: a front advances at the latency of a tile visit by one wave
// (a few microseconds).  A wave never waits for anything but a queue entry or a tile lock held by a RUNNING wave, so
// the launch finishes with any number of resident workgroups.
//
//  * queue: a ticket ring.  A consumer takes ticket t = head++ and waits for ring[t % cap] to carry tag t + 1; a producer
//    takes t = tail++ and publishes {t + 1, payload} into the same slot once it is empty.  `pending` counts entries
//    queued or in flight; the visit that brings it to zero raises `done` and every waiting wave leaves.  A tile is in
//    the queue at most once (membership flag, test-and-set), so `cap` = number of tiles never overflows.
//    The FIRST entries are not in the ring at all: the kernel before the launch left a work list with a device-side count n,
//    and a consumer whose ticket is below n reads list[ticket] (no wait, no ring traffic); ring tickets start after them,
//    and `pending` counts from n.  So a launch needs no set-up launch: ring and control words are zeroed by kernels that run
//    anyway (k_mf_rinit for the relabel, k_mf_active for the push), never assumed empty from the launch before — one that
//    ends on its visit budget or on the time-out leaves entries behind.
//  * memory: the per-XCD L2s are not coherent with each other inside a launch.  Every word another wave may change —
//    labels, excess, residual capacities, sink links, flags, locks, the ring — is therefore WRITTEN with a device-scope
//    atomic read-modify-write (performed at memory) and READ with an sc1 load; tools/micro/xcd_atomics.hip measured 0
//    stale reads of 1.6e8 for that pairing on MI355X, same XCD and across XCDs.  Kernel boundaries on either side make
//    the plain stores of the dense launches visible.
//  * relabel: labels only fall (atomicMin), stale halos only delay — the neighbour that lowers a halo pixel afterwards
//    re-queues the tile.  The launch ends at the exact fixpoint, so the host reads nothing back.
//  * push: a tile has ONE state word {queued, busy}.  A wave that takes a tile marks it busy and sweeps its private LDS
//    copy (two waves on one tile would push the same excess twice); a neighbour that hands excess over meanwhile only sets
//    `queued`, and the holder re-queues the tile when it lets go.  Everything goes back as atomic deltas, exactly like the
//    border ring of the launch-driven kernel.  A queue entry carries its hop count: chains stop after `gen_max` hops (the
//    equivalent of the launch count of a host-driven round); what is left is picked up by the next global relabel + active
//    scan, as before.
//  * a hop costs memory round trips (~2 us each for device-scope atomics and sc1 loads), so both kernels FOLLOW: the wave
//    that finishes a visit continues with one of the tiles it would have queued (no ring traffic on the critical path), and
//    a push sweep works one active pixel per lane, carried in a register from sweep to sweep (32x8 tiles by default, 32x16
//    and 32x32 on request), so it costs what the active pixels cost and one visit carries excess across the tile.
#include "ggc_gc.h"
#include "ggc_mf_sweep.h"
#include "ggc_mf_push.h"
#include <algorithm>
#include <cstdlib>

namespace ggc {
namespace {

constexpr int PT_H = MF_PT_H;
constexpr long long AQ_TIMEOUT = 200000000ll;        // 2 s of wall_clock64 (100 MHz): a wave that waits longer reports and ends the launch

__device__ __forceinline__ unsigned long long ldg64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }   // this wave's loads, stores and atomics are done

// The entries a launch starts with: list[0 .. n) of the kernel before it (n = 0: everything comes through the ring).
struct AqInit { const int32_t* list; int n; };

// consumer side, lane 0 of a wave; returns the payload (>= 0) to every lane, or -1 when the launch is over
__device__ __forceinline__ int aq_pop(unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap, const AqInit& in, int lane,
                                      int32_t* __restrict__ err_flag) {
    int payload = -1;
    if (lane == 0) {
        const unsigned t = (unsigned)atomicAdd(&q[AQ_HEAD], 1);
        if (t < (unsigned)in.n) {
            payload = in.list[t];                                          // written before the launch: a plain load, nothing to wait for
        } else {
            const unsigned tr = t - (unsigned)in.n;                        // ring ticket
            unsigned long long* slot = ring + tr % (unsigned)cap;
            const long long t0 = wall_clock64();
            for (int n = 0;; ++n) {
                const unsigned long long v = ldg64(slot);
                if ((unsigned)(v >> 32) == tr + 1u) { atomicExch(slot, 0ull); payload = (int)(unsigned)v; break; }
                if ((n & 3) == 3) {
                    if (ldg(&q[AQ_DONE]) || ldg(&q[AQ_PENDING]) + in.n == 0) break;   // nothing queued, nothing in flight
                    if (wall_clock64() - t0 > AQ_TIMEOUT) { if (err_flag) atomicOr(err_flag, 4); atomicExch(&q[AQ_DONE], 1); break; }
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
    }
    return __builtin_amdgcn_readfirstlane(payload);
}
// producer side, any single lane.  The caller has won the tile's membership flag.
__device__ __forceinline__ void aq_push(unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap, int payload,
                                        int32_t* __restrict__ err_flag) {
    atomicAdd(&q[AQ_PENDING], 1);
    const unsigned t = (unsigned)atomicAdd(&q[AQ_TAIL], 1);
    unsigned long long* slot = ring + t % (unsigned)cap;
    const unsigned long long e = ((unsigned long long)(t + 1u) << 32) | (unsigned)payload;
    const long long t0 = wall_clock64();
    while (atomicCAS(slot, 0ull, e) != 0ull) {           // the previous user of the slot (ticket t - cap) has not read it yet
        if (wall_clock64() - t0 > AQ_TIMEOUT) { if (err_flag) atomicOr(err_flag, 4); atomicExch(&q[AQ_DONE], 1); break; }
        __builtin_amdgcn_s_sleep(2);
    }
}
// AQ_PENDING holds the entries queued or in flight MINUS the in.n the launch started with (it starts at zero)
__device__ __forceinline__ void aq_finish(int32_t* __restrict__ q, const AqInit& in) {
    if (atomicSub(&q[AQ_PENDING], 1) + in.n == 1) atomicExch(&q[AQ_DONE], 1);
}

// ---- global relabel, asynchronous ---------------------------------------------------------------------------------
// The visit is the bit-row BFS of the dense launches with the sweeps as its fallback (ggc_mf_sweep.h).  It is safe against
// the other waves of the launch: the BFS takes only label-1 pixels and the halo as sources, tests `start < its label`
// afterwards (a label another wave lowered before the load: fallback to the sweeps, which carry any start label on), and
// labels go back by atomicMin where they fell (a label lowered behind the visit's back: a harmless write).
#ifndef GGC_MF_RELAX_ASYNC_BFS
#define GGC_MF_RELAX_ASYNC_BFS 1    // 1 = BFS visit with the sweeps as fallback, 0 = sweeps only
#endif
// count / list: the work list of the last launch-driven relabel kernel, the queue's first entries; ring and q zeroed by k_mf_rinit.
// PROF (GGC_MF_TRACE): the visits' clocks into table 2 of the trace clocks.
template <bool PROF>
__global__ void __launch_bounds__(256) k_mf_relax_async(GcDims d, MfTiles tl, uint8_t* __restrict__ rmask, int32_t* __restrict__ dirty,
                                                        const int32_t* __restrict__ rc, int32_t* __restrict__ dist, int32_t* __restrict__ flag,
                                                        const int32_t* __restrict__ count, const int32_t* __restrict__ list,
                                                        unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int cap,
                                                        int32_t* __restrict__ err_flag, long long* __restrict__ prof) {
    __shared__ RelaxWaveLds lds[4];
    RelaxWaveLds& S = lds[threadIdx.x >> 6];
    const int tiles_per_image = tl.rt_x * tl.rt_y;
    const AqInit in{list, min(*count, cap)};
    MfRelaxClocks<PROF> ck;
    int tile = -1;                                                         // >= 0: the neighbour this wave follows into
    for (;;) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));                                     // keeps the lane arithmetic inside the loop (no hoist + spill)
        if (tile < 0) {
            tile = aq_pop(ring, q, cap, in, lane, err_flag);
            if (tile < 0) break;
            if (lane == 0) atomicExch(&flag[tile], 0);                     // consumed: a halo change from now on re-queues the tile
            drain();                                                       // ... and the loads below come after it
        }
        ck.begin();
        const int nbm = mf_relax_visit<true, PROF, GGC_MF_RELAX_ASYNC_BFS != 0>(d, tl, tile, lane, S, rmask, dirty, rc, dist, flag, ck);
        drain();                                                           // the new labels are at memory before a neighbour is told
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / tl.rt_x, txi = tr % tl.rt_x;
        // Neighbours whose halo changed and that are not queued: the first one this wave visits next itself (its flag stays 0,
        // as if popped; a second wave relaxing the same tile meanwhile is harmless — labels only fall, atomically), the
        // others go through the queue.
        int nb = -1;
        if (lane < 9 && (nbm >> lane) & 1) {
            const int ty = tyi + lane / 3 - 1, tx = txi + lane % 3 - 1;
            if (ty >= 0 && ty < tl.rt_y && tx >= 0 && tx < tl.rt_x) nb = b * tiles_per_image + ty * tl.rt_x + tx;
        }
        const bool cand = nb >= 0 && ldg(&flag[nb]) == 0;
        const unsigned long long cm = __ballot(cand);
        int next = -1;
        if (cm) {
            const int fl = __ffsll((long long)cm) - 1;
            next = __shfl(nb, fl, 64);
            if (cand && lane != fl && atomicExch(&flag[nb], 1) == 0) aq_push(ring, q, cap, nb, err_flag);
            drain();                                                       // the entries count as pending before this visit ends
        }
        if (next < 0 && lane == 0) aq_finish(q, in);                       // (following keeps this visit's pending unit)
        tile = next;
        mf_wave_sync();
        ck.end();
    }
    if (PROF && (threadIdx.x & 63) == 0 && ck.sum[3]) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(prof) + (128 + (blockIdx.x & 63)) * 8;
        for (int k = 0; k < 7; ++k) atomicAdd(&o[k], (unsigned long long)ck.sum[k]);
    }
}

// ---- push-relabel sweeps, asynchronous --------------------------------------------------------------------------------
constexpr int ST_Q = 1, ST_BUSY = 2;                  // tile state word: queued (or owed a visit) | a wave holds it

// The tile visit is push_tile_visit<TH, true> of ggc_mf_push.h (sc1 loads, every write-back a device-scope atomic).

// PROF (GGC_MF_TRACE): the wave's clocks and chain counters; the untraced instance carries none of that state.
template <int TH, bool PROF>
__global__ void __launch_bounds__(64) k_mf_push_async(GcDims d, int bt_x, int bt_y, int pt_y, int inner, int gen_max, const int32_t* __restrict__ lmax, int slack,
                                                      int32_t* __restrict__ dirty, int32_t* __restrict__ rc,
                                                      int32_t* __restrict__ ex, int32_t* __restrict__ snk, int32_t* __restrict__ dist,
                                                      uint8_t* __restrict__ rmask, int32_t* __restrict__ st, unsigned long long* __restrict__ ring,
                                                      int32_t* __restrict__ q, int cap, const int32_t* __restrict__ count,
                                                      const int32_t* __restrict__ list, int32_t* __restrict__ err_flag,
                                                      long long* __restrict__ prof_p) {
    long long* const prof = PROF ? prof_p : nullptr;
    __shared__ PushTileLds<TH> S;
    const int tiles_per_image = bt_x * bt_y;
    const size_t BP = (size_t)d.B * d.P;
    // count != null (32x8 tiles): the queue starts with the active scan's list, which left every listed tile's state word
    // "queued" and zeroed ring and q; the visit budget follows from the same count.  null: k_aq_fill_big filled the ring.
    const AqInit in{list, count ? min(*count, cap) : 0};
    const int budget = count ? (int)min((long long)in.n * gen_max + 4096, (long long)0x3fffffff) : ldg(&q[AQ_BUDGET]);
    int tile = -1, gen = 0;
    // GGC_MF_TRACE (prof != null): where a wave's time goes — waiting for a queue entry, the visit, the hand-over — in
    // wall_clock64 ticks, kept in registers and added up once when the wave leaves
    long long p_wait = 0, p_visit = 0, p_hand = 0, p_n = 0, p_follow = 0, p_cut = 0, p_idle = 0, pv[4] = {0, 0, 0, 0};
    const long long t_start = prof ? wall_clock64() : 0;
    for (;;) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const long long t_0 = prof ? wall_clock64() : 0;
        if (tile < 0) {
            const int payload = aq_pop(ring, q, cap, in, lane, err_flag);
            if (payload < 0) { if (prof) p_wait += wall_clock64() - t_0; break; }
            tile = payload & 0xffffff; gen = payload >> 24;
        } else if (prof) ++p_follow;
        // A tile that is queued (or followed into) is never busy: it is only queued from the idle state, and its holder
        // re-queues it after letting go.  Busy from here on; excess that arrives meanwhile sets `queued` again.
        int over = 0;
        if (lane == 0) {
            atomicExch(&st[tile], ST_BUSY);
            over = atomicAdd(&q[AQ_VISITS], 1) >= budget;                  // runaway guard: the rest waits for the next relabel
            if (over) atomicExch(&q[AQ_DONE], 1);
        }
        drain();                                                           // ... before the tile is loaded
        const long long t_1 = prof ? wall_clock64() : 0;
        const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
        const int tyi = tr / bt_x, txi = tr % bt_x;
        const int nbm = push_tile_visit<TH, true>(d, lmax + (size_t)b * MF_LMAX_STRIDE, slack, tyi, txi, inner, (size_t)b * d.P, BP, rc, ex, snk, dist, rmask, S, lane, PROF, pv);
        drain();                                                           // the write-back is at memory
        const long long t_2 = prof ? wall_clock64() : 0;
        const bool left = (nbm >> 4) & 1;
        int nb = -1;
        bool cand = false;
        if (lane == 4) {
            nb = tile;
            const int old = atomicExch(&st[tile], left ? ST_Q : 0);        // let go; still active: owed a visit, ours to arrange
            if (left) cand = true;
            else if (old & ST_Q) cand = (atomicOr(&st[tile], ST_Q) & (ST_Q | ST_BUSY)) == 0;   // excess arrived while we held it
        } else if (lane < 9 && (nbm >> lane) & 1) {
            const int ty = tyi + lane / 3 - 1, tx = txi + lane % 3 - 1;
            if (ty >= 0 && ty < bt_y && tx >= 0 && tx < bt_x) {
                nb = b * tiles_per_image + ty * bt_x + tx;
                // its border arcs may have been re-opened: the 32x8 push tiles it consists of are dirty for the next relabel
                for (int k = 0; k < TH / PT_H; ++k)
                    if (ty * (TH / PT_H) + k < pt_y) atomicOr(&dirty[(size_t)b * bt_x * pt_y + (size_t)(ty * (TH / PT_H) + k) * bt_x + tx], 1);
                cand = (atomicOr(&st[nb], ST_Q) & (ST_Q | ST_BUSY)) == 0;  // idle: ours to arrange; busy: its holder re-queues it
            }
        }
        if (prof) {                                                        // how the chain ends here, if it does: on the hop limit, or with nothing to hand on
            const bool any = __ballot(cand) != 0ull;
            if (!any) ++p_idle; else if (gen + 1 >= gen_max) ++p_cut;
        }
        if (gen + 1 >= gen_max) cand = false;                              // chain length reached: left for the next relabel
        const unsigned long long cm = __ballot(cand);
        int next = -1;
        if (cm) {
            const int fl = __ffsll((long long)cm) - 1;
            next = __shfl(nb, fl, 64);                                     // follow the first, queue the others
            if (cand && lane != fl) aq_push(ring, q, cap, ((gen + 1) << 24) | nb, err_flag);
            drain();
        }
        if (next < 0 && lane == 0) aq_finish(q, in);
        tile = next; gen = gen + 1;
        mf_wave_sync();
        if (prof) { p_wait += t_1 - t_0; p_visit += t_2 - t_1; p_hand += wall_clock64() - t_2; ++p_n; }
    }
    if (prof) for (int o = 32; o > 0; o >>= 1) pv[3] = max(pv[3], __shfl_xor(pv[3], o, 64));   // the highest label any lane wrote back
    if (prof && (threadIdx.x & 63) == 0) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(prof) + (blockIdx.x & 63) * 8;
        atomicAdd(&o[7], (unsigned long long)p_cut);
        atomicAdd(&o[0], (unsigned long long)p_wait); atomicAdd(&o[1], (unsigned long long)p_visit); atomicAdd(&o[2], (unsigned long long)p_hand);
        atomicAdd(&o[3], (unsigned long long)p_n); atomicAdd(&o[4], (unsigned long long)p_follow);
        atomicAdd(&o[5], (unsigned long long)(wall_clock64() - t_start)); atomicAdd(&o[6], 1ull);
        unsigned long long* o2 = o + 64 * 8;                               // second table: inside the visit
        atomicAdd(&o2[0], (unsigned long long)pv[0]); atomicAdd(&o2[1], (unsigned long long)pv[1]); atomicAdd(&o2[2], (unsigned long long)pv[2]);
        atomicAdd(&o2[3], (unsigned long long)p_idle); atomicMax(&o2[4], (unsigned long long)pv[3]);
    }
}

// queue <- the big tiles that hold the 32x8 push tiles of list[0 .. *count) (the active scan's list); ring, q and st zeroed before
__global__ void __launch_bounds__(256) k_aq_fill_big(const int32_t* __restrict__ count, const int32_t* __restrict__ list, int pt_x, int pt_y,
                                                     int th, int bt_x, int bt_y, int32_t* __restrict__ st,
                                                     unsigned long long* __restrict__ ring, int32_t* __restrict__ q, int budget_per_item) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *count;
    if (i == 0) q[AQ_BUDGET] = (int)min((long long)n * budget_per_item + 4096, (long long)0x3fffffff);
    if (i >= n) return;
    const int t = list[i], b = t / (pt_x * pt_y), tr = t % (pt_x * pt_y);
    const int big = b * bt_x * bt_y + ((tr / pt_x) * PT_H / th) * bt_x + tr % pt_x;
    if (atomicOr(&st[big], ST_Q) == 0) {
        const int slot = atomicAdd(&q[AQ_TAIL], 1);
        atomicAdd(&q[AQ_PENDING], 1);
        ring[slot] = (((unsigned long long)(unsigned)(slot + 1)) << 32) | (unsigned)big;
    }
}

} // namespace

int maxflow_relax_async(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const MfTiles& tl, uint8_t* rmask, int32_t* dirty, const int32_t* rc, int32_t* dist,
                        const int32_t* count, const int32_t* list, int32_t* flag, unsigned long long* ring, int32_t* q, int cap,
                        int grid, int32_t* err_flag, long long* prof) {
    if (prof)
        hipLaunchKernelGGL(k_mf_relax_async<true>, dim3(grid), dim3(256), 0, st, d, tl, rmask, dirty, rc, dist, flag, count, list, ring, q, cap, err_flag, prof);
    else
        hipLaunchKernelGGL(k_mf_relax_async<false>, dim3(grid), dim3(256), 0, st, d, tl, rmask, dirty, rc, dist, flag, count, list, ring, q, cap, err_flag, prof);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int maxflow_push_async_tile(int th) { return th >= 32 ? 32 : (th >= 16 ? 16 : 8); }

int maxflow_push_async(ggc_ctx* ctx, hipStream_t st, const GcDims& d, const MfTiles& tl, int th, int inner, int gen_max, const int32_t* lmax, int slack, int32_t* rc,
                       int32_t* ex, int32_t* snk, int32_t* dist, uint8_t* rmask, int32_t* dirty, const int32_t* count, const int32_t* list, int n_list_max, int32_t* state,
                       unsigned long long* ring, int32_t* q, int waves, int32_t* err_flag, long long* prof) {
    th = maxflow_push_async_tile(th);
    const int bt_x = tl.pt_x, bt_y = cdiv(d.H, th), cap = bt_x * bt_y * d.B;
    gen_max = std::min(gen_max, 127);
    if (th == 8) {                      // the active scan's tiles ARE the queue's tiles: it left ring, q and the state words ready
        if (prof) hipLaunchKernelGGL((k_mf_push_async<8, true>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           count, list, err_flag, prof);
        else hipLaunchKernelGGL((k_mf_push_async<8, false>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           count, list, err_flag, prof);
        GGC_LAUNCH_CHECK(ctx);
        return GGC_OK;
    }
    const int32_t* no_list = nullptr;
    mf_zero3(st, reinterpret_cast<int32_t*>(ring), (size_t)cap * 2, q, AQ_WORDS, state, (size_t)cap);
    hipLaunchKernelGGL(k_aq_fill_big, dim3(cdiv(n_list_max, 256)), dim3(256), 0, st, count, list, tl.pt_x, tl.pt_y, th, bt_x, bt_y, state, ring, q,
                       gen_max);
    if (th == 32)
        if (prof) hipLaunchKernelGGL((k_mf_push_async<32, true>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           no_list, no_list, err_flag, prof);
        else hipLaunchKernelGGL((k_mf_push_async<32, false>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           no_list, no_list, err_flag, prof);
    else
        if (prof) hipLaunchKernelGGL((k_mf_push_async<16, true>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           no_list, no_list, err_flag, prof);
        else hipLaunchKernelGGL((k_mf_push_async<16, false>), dim3(waves), dim3(64), 0, st, d, bt_x, bt_y, tl.pt_y, inner, gen_max, lmax, slack, dirty, rc, ex, snk, dist, rmask, state, ring, q, cap,
                           no_list, no_list, err_flag, prof);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

} // namespace ggc
