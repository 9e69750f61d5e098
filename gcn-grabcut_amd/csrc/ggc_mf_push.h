// ggc_mf_push.h — the push visit of a 32 x TH tile by ONE wave (excess, sink links, labels + halo and residual capacities in
// LDS, one carried pixel per lane), shared by the asynchronous launch of ggc_maxflow_async.hip and the dense launches over
// work lists of ggc_maxflow.hip.  The sweep loop is one code; the two clients differ in how the tile is read and written back.
#pragma once
#include "ggc_gc.h"
#include "ggc_mf_sweep.h"

namespace ggc {

// One wave, one 32 x TH tile (TH/2 pixels per lane for loading and write-back).  A sweep works one active pixel (excess that
// can still reach the sink) per lane, so it costs what the active pixels cost and a visit can afford enough sweeps to carry
// excess across the tile.  A lane CARRIES its next pixel in a register from sweep to sweep: the receiver when it pushed inside
// the tile, its own pixel when that kept excess and nothing went to a receiver inside the tile.  Only what a lane cannot
// carry — its own pixel's remainder when it goes on with the receiver — is handed to a lane that carries nothing, or, when
// every lane is taken, spilled into a bitmask in LDS, one word per row; the mask's words are read in the round trip of the
// pixel's own reads, and only a sweep that finds it non-empty compacts mask and carried pixels into a list and deals the
// lanes new pixels (the first 64 in row-major order; bits beyond stay).  The mask also holds the visit's first pixels.
// Two lanes may carry the same pixel: the exchange on its excess hands it to one of them, the other sees 0.
template <int TH>
struct PushTileLds {
    int ex[32 * TH]; int sk[32 * TH]; int d[TH + 2][34]; int rc[8][32 * TH];
    uint32_t mask[32]; unsigned short list[64];
};

template <bool ASYNC>
__device__ __forceinline__ int mf_push_ld(const int32_t* p) { return ASYNC ? ldg(p) : *p; }

// Returns the 9-bit mask of tiles owed a visit: bit (dy + 1) * 3 + (dx + 1) for a neighbour that received excess, bit 4
// when this tile still holds active pixels.
//   ASYNC = true (k_mf_push_async, one launch that follows the excess from tile to tile): a tile can be visited from several
//           XCDs within the launch, so loads are sc1 loads and everything returns as a device-scope atomic read-modify-write.
//   ASYNC = false (k_mf_pr_wave, a launch over a work list: a tile is visited at most once per launch and the kernel
//           boundaries order the rest): plain loads; a pixel of the tile's interior has no other writer during the launch and
//           goes back with plain stores where it changed; only what a neighbouring tile's visit may add to meanwhile — the
//           excess of the border ring, the arcs that leave the tile — goes back as an atomic delta.
// lim_p, slack: the image's LABEL CEILING for this push phase.  *lim_p is the largest finite label the relabel before this
// phase gave the image (k_mf_active), and a pixel whose label reaches lim = min(d.P, *lim_p + 1 + slack) is treated exactly
// like one at d.P: it keeps its excess, is not active and waits for the next global relabel (slack < 0: lim = d.P).  Right
// after a relabel no pixel holds label *lim_p + 1, so everything above it is cut off from the sink (the gap theorem); where
// local relabels have filled that level since, the ceiling parks excess that could still have moved, which costs a round and
// never the result.  The word was written by an earlier kernel: a plain load, issued with the tile's loads.
// prof: pv[0..2] += ticks of load + fill, ticks of the sweeps, sweeps; ASYNC = false also pv[3] += sweeps that ended in a deal,
// ASYNC = true pv[3] = max(pv[3], the highest finite label this lane wrote back).
template <int TH, bool ASYNC>
__device__ int push_tile_visit(const GcDims& d, const int32_t* __restrict__ lim_p, int slack, int tyi, int txi, int inner, size_t base, size_t BP,
                               int32_t* __restrict__ rc, int32_t* __restrict__ ex, int32_t* __restrict__ snk,
                               int32_t* __restrict__ dist, uint8_t* __restrict__ rmask, PushTileLds<TH>& S, int lane,
                               bool prof, long long (&pv)[4]) {
    constexpr int NPX = TH / 2, HALO = (TH + 2) * 34, HALO_IT = (HALO + 63) / 64;
    const long long tv0 = prof ? wall_clock64() : 0;
    const int lx = lane & 31, r0 = lane >> 5;
    const int x = txi * 32 + lx;
    const int lmax = *lim_p;
    int e0[NPX], sk0[NPX], r0v[NPX][8];
    // every load of the visit is issued unconditionally from a clamped address, then masked
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
        const int y = tyi * TH + r0 + 2 * j;
        const int pc = min(y, d.H - 1) * d.W + min(x, d.W - 1);
        e0[j] = mf_push_ld<ASYNC>(ex + base + pc);
        sk0[j] = mf_push_ld<ASYNC>(snk + base + pc);
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) r0v[j][dir] = mf_push_ld<ASYNC>(rc + rc_idx(dir, base + pc));
    }
    int* sd = &S.d[0][0];
    int hv[HALO_IT];
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {
        const int i = min(lane + k * 64, HALO - 1);
        const int gy = tyi * TH + i / 34 - 1, gx = txi * 32 + i % 34 - 1;
        hv[k] = mf_push_ld<ASYNC>(dist + base + (size_t)min(max(gy, 0), d.H - 1) * d.W + min(max(gx, 0), d.W - 1));
    }
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {
        const int i = lane + k * 64;
        const int gy = tyi * TH + i / 34 - 1, gx = txi * 32 + i % 34 - 1;
        if (i < HALO) sd[i] = (gx >= 0 && gx < d.W && gy >= 0 && gy < d.H) ? hv[k] : DINF;
    }
    if (lane < 32) S.mask[lane] = 0u;
    const int lim = slack < 0 ? d.P : min(d.P, lmax + 1 + slack);
    mf_wave_sync();
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
        const int slot = lane + 64 * j, ly = r0 + 2 * j;
        const bool inb = x < d.W && tyi * TH + ly < d.H;
        if (!inb) { e0[j] = 0; sk0[j] = 0; }
        S.ex[slot] = e0[j];
        S.sk[slot] = sk0[j];
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) {
            if (!inb) r0v[j][dir] = 0;
            S.rc[dir][slot] = r0v[j][dir];
        }
        const bool a = e0[j] > 0 && S.d[ly + 1][lx + 1] < lim;
        const unsigned long long m = __ballot(a);                          // lanes 0-31: row 2j, lanes 32-63: row 2j + 1
        if (lane == 0) { S.mask[2 * j] = (uint32_t)m; S.mask[2 * j + 1] = (uint32_t)(m >> 32); }
    }
    mf_wave_sync();
    int nbm = 0;
    const long long tv1 = prof ? wall_clock64() : 0;
    int n_sw = 0, n_deal = 0;
    int cur = -1;                                                          // the pixel this lane carries into the next sweep
    // ---- bitmask -> list (row-major) -> one pixel per lane; the rows' bits that 64 lanes do not take stay in the mask
    // every lane reads all TH row words (broadcast reads) and forms the row offsets itself: no cross-lane step (a prefix
    // scan by __shfl_up is five dependent LDS-crossbar round trips)
    auto deal = [&]() {
        uint32_t w = 0u;
        int off = 0, n_act = 0;
#pragma unroll
        for (int r = 0; r < TH; ++r) {
            const uint32_t wr = S.mask[r];
            const int cr = __popc(wr);
            w = r == lane ? wr : w;
            off += r < lane ? cr : 0;
            n_act += cr;
        }
        mf_wave_sync();                                                    // every lane has read the words before they are rewritten
        while (w && off < 64) { const int bit = __ffs(w) - 1; S.list[off++] = (unsigned short)(lane * 32 + bit); w &= w - 1; }
        if (lane < TH) S.mask[lane] = w;
        mf_wave_sync();
        cur = lane < n_act ? (int)S.list[lane] : -1;
    };
    deal();                                                                // the fill's mask
    for (int it = 0; it < inner; ++it) {
        // ---- one round trip: the spill words and the carried pixel.  A lane TAKES the pixel's excess with an exchange and
        // gives back what it could not push, so what a neighbouring lane pushes into the pixel meanwhile is kept.  (Chasing a
        // unit of excess from pixel to pixel within a sweep, and parking pixels that only climb, were measured and removed:
        // DESIGN.md 5.5.)
        uint32_t sp = 0u;
#pragma unroll
        for (int r = 0; r < TH; ++r) sp |= S.mask[r];
        int carry = -1, spill = -1;
        if (cur >= 0) {
            const int slot = cur, ly = slot >> 5, plx = slot & 31;
            const int e = atomicExch(&S.ex[slot], 0);
            const int dp = S.d[ly + 1][plx + 1];
            const int sk = S.sk[slot];
            int r[8], hq[8];
#pragma unroll
            for (int dir = 0; dir < 8; ++dir) {
                r[dir] = __hip_atomic_load(&S.rc[dir][slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                hq[dir] = S.d[ly + 1 + dir_dy(dir)][plx + 1 + dir_dx(dir)];
            }
            if (e <= 0) {
                // nothing left (or another lane carried the same pixel and took it)
            } else if (dp >= lim) {
                atomicAdd(&S.ex[slot], e);                                 // cannot reach the sink: the excess stays where it is
            } else {
                int hmin = sk > 0 ? 0 : DINF, best = sk > 0 ? 8 : -1, rb = 0;
#pragma unroll
                for (int dir = 0; dir < 8; ++dir) {
                    const bool ok = r[dir] > 0 && hq[dir] < hmin;
                    hmin = ok ? hq[dir] : hmin; best = ok ? dir : best; rb = ok ? r[dir] : rb;
                }
                if (best >= 0 && dp > hmin) {
                    if (best == 8) {
                        const int dl = min(e, sk);
                        S.sk[slot] = sk - dl;                              // only the holder of the pixel's excess touches its sink link
                        if (e - dl > 0) { atomicAdd(&S.ex[slot], e - dl); carry = slot; }   // sink link full: on to the neighbours
                    } else {
                        const int dl = min(e, rb), rem = e - dl;
                        atomicSub(&S.rc[best][slot], dl);
                        if (rem > 0) atomicAdd(&S.ex[slot], rem);
                        // (dir_dx / dir_dy of a direction known only at run time, from bit tables: no branches)
                        const int qlx = plx + ((0x62 >> best) & 1) - ((0x91 >> best) & 1), qly = ly + ((0xa8 >> best) & 1) - ((0x54 >> best) & 1);
                        if (qlx >= 0 && qlx < 32 && qly >= 0 && qly < TH) {
                            const int qt = qly * 32 + qlx;
                            atomicAdd(&S.rc[best ^ 1][qt], dl);
                            atomicAdd(&S.ex[qt], dl);
                            carry = qt;                                    // on with the receiver ...
                            spill = rem > 0 ? slot : -1;                   // ... and the rest, which this lane cannot carry too, to the mask
                        } else {                                           // across the tile edge: straight to memory
                            const int gy = tyi * TH + qly, gx = txi * 32 + qlx;
                            const size_t qg = base + (size_t)gy * d.W + gx;
                            atomicAdd(&rc[rc_idx((best ^ 1), qg)], dl);
                            atomicAdd(&ex[qg], dl);
                            const int tdy = qly < 0 ? -1 : (qly >= TH ? 1 : 0), tdx = qlx < 0 ? -1 : (qlx >= 32 ? 1 : 0);
                            nbm |= 1 << ((tdy + 1) * 3 + tdx + 1);
                            carry = rem > 0 ? slot : -1;
                        }
                    }
                } else {
                    const int nd = (best >= 0 && hmin < DINF) ? hmin + 1 : DINF;
                    S.d[ly + 1][plx + 1] = nd;
                    atomicAdd(&S.ex[slot], e);                             // give it back; with the new label the next sweep can push
                    carry = nd >= lim ? -1 : slot;
                }
            }
        }
        sp = __builtin_amdgcn_readfirstlane(sp);                           // (every lane read the same words)
        if (sp == 0u && !__any(cur >= 0)) break;                           // no lane carries a pixel, nothing spilled
        ++n_sw;
        if (sp == 0u) {
            // A remainder goes to an IDLE lane where there is one: the k-th lane with a remainder leaves it in list[k], the
            // k-th lane that carries nothing picks it up (ranks from two ballots; one LDS write and read, only in a sweep that
            // has a remainder).  Only remainders beyond the idle lanes reach the mask, and with it the next sweep's deal.
            const unsigned long long rem_m = __ballot(spill >= 0);
            if (rem_m) {
                const unsigned long long idle_m = __ballot(carry < 0);
                const int n_rem = __popcll(rem_m), n_idle = __popcll(idle_m);
                const int k_rem = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(rem_m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rem_m, 0u));
                const int k_idle = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle_m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_m, 0u));
                if (spill >= 0) {
                    if (k_rem < n_idle) S.list[k_rem] = (unsigned short)spill;
                    else atomicOr(&S.mask[spill >> 5], 1u << (spill & 31));
                }
                mf_wave_sync();
                if (carry < 0 && k_idle < n_rem) carry = (int)S.list[k_idle];
            }
            cur = carry;
            mf_wave_sync();
        } else {                                                           // the mask is not empty: carried pixels into it, and a new deal
            if (carry >= 0) atomicOr(&S.mask[carry >> 5], 1u << (carry & 31));
            if (spill >= 0) atomicOr(&S.mask[spill >> 5], 1u << (spill & 31));
            mf_wave_sync();
            deal();
            if (!ASYNC) ++n_deal;
        }
    }
    const long long tv2 = prof ? wall_clock64() : 0;
    if (prof) { pv[0] += tv1 - tv0; pv[1] += tv2 - tv1; pv[2] += n_sw; }
    if (!ASYNC && prof) pv[3] += n_deal;
    int left = 0;
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
        const int slot = lane + 64 * j, ly = r0 + 2 * j;
        const int y = tyi * TH + ly;
        const bool inb = x < d.W && y < d.H;
        const size_t p = base + (size_t)min(y, d.H - 1) * d.W + min(x, d.W - 1);
        const int e1 = S.ex[slot], sk1 = S.sk[slot], d1 = S.d[ly + 1][lx + 1];
        int r1[8];
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) r1[dir] = S.rc[dir][slot];
        if (!inb) continue;
        if (ASYNC) {
            // everything returns as an atomic read-modify-write: deltas where a neighbouring tile's wave may have added meanwhile
            // (excess, reverse arcs), exchanges for what only the tile's holder writes (sink link, label)
            if (e1 != e0[j]) atomicAdd(&ex[p], e1 - e0[j]);
            int m1 = 0, chg = 0;
#pragma unroll
            for (int dir = 0; dir < 8; ++dir) {
                m1 |= (r1[dir] > 0) ? (1 << dir) : 0;
                if (r1[dir] != r0v[j][dir]) { chg = 1; atomicAdd(&rc[rc_idx(dir, p)], r1[dir] - r0v[j][dir]); }
            }
            if (chg) {
                // read by the next relabel only, but a tile can be visited from several XCDs within this launch: two plain stores to
                // one byte would sit in two L2s and reach memory in either order.  Atomics on the byte's word (clear, then set).
                uint32_t* w = reinterpret_cast<uint32_t*>(rmask + (p & ~(size_t)3));
                const int sh = 8 * (int)(p & 3);
                atomicAnd(w, ~(0xffu << sh));
                atomicOr(w, (uint32_t)m1 << sh);
            }
            if (sk1 != sk0[j]) atomicExch(&snk[p], sk1);
        } else {
            // only the tile's border ring can receive pushes from other tiles during this launch: the interior is owned
            // exclusively, so its write-back is a plain store (L2 atomics are the scarce resource in the early rounds, when
            // nearly every pixel changes)
            const bool ring = lx == 0 || lx == 31 || ly == 0 || ly == TH - 1;
            if (e1 != e0[j]) { if (ring) atomicAdd(&ex[p], e1 - e0[j]); else ex[p] = e1; }
            int m1 = 0, chg = 0;
#pragma unroll
            for (int dir = 0; dir < 8; ++dir) {
                m1 |= (r1[dir] > 0) ? (1 << dir) : 0;
                if (r1[dir] != r0v[j][dir]) {
                    chg = 1;
                    // another tile's push can only add to an arc that points OUT of this tile (the reverse of its own arc): those
                    // go back as atomic deltas, every other capacity is this wave's alone
                    const bool out = (ly == 0 && dir_dy(dir) < 0) || (ly == TH - 1 && dir_dy(dir) > 0) ||
                                     (lx == 0 && dir_dx(dir) < 0) || (lx == 31 && dir_dx(dir) > 0);
                    if (out) atomicAdd(&rc[rc_idx(dir, p)], r1[dir] - r0v[j][dir]);
                    else rc[rc_idx(dir, p)] = r1[dir];
                }
            }
            if (chg) rmask[p] = (uint8_t)m1;     // (arcs that leave the tile: the relabel reads the capacities, see mf_tile_dirty)
            if (sk1 != sk0[j]) snk[p] = sk1;
        }
        // the label: compare with the halo copy's origin is not kept, so write when the pixel was relabelled (d only rises here)
        left |= (e1 > 0 && d1 < lim) ? 1 : 0;
    }
    // labels: a pixel's label is written when it differs from what memory held at load time
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {
        const int i = lane + k * 64;
        const int hy = i / 34, hx = i % 34;
        if (i < HALO && hy >= 1 && hy <= TH && hx >= 1 && hx <= 32) {
            const int gy = tyi * TH + hy - 1, gx = txi * 32 + hx - 1;
            if (gx < d.W && gy < d.H && sd[i] != hv[k]) {
                if (ASYNC && prof && sd[i] < DINF) pv[3] = max(pv[3], (long long)sd[i]);
                if (ASYNC) atomicExch(&dist[base + (size_t)gy * d.W + gx], sd[i]);
                else dist[base + (size_t)gy * d.W + gx] = sd[i];
            }
        }
    }
    if (__any(left)) nbm |= 1 << 4;
    return mf_wave_or(nbm);
}

} // namespace ggc
