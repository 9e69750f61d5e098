// ggc_mf_sweep.h — the relabel visit of a 32x32 tile (labels + halo in LDS, in-register sweeps), shared by the work-list
// launches of ggc_maxflow.hip and the asynchronous launch of ggc_maxflow_async.hip.
#pragma once
#include "ggc_gc.h"

namespace ggc {

__device__ __forceinline__ void mf_wave_sync() {     // LDS traffic of one wave is in order: only the compiler needs telling
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int ldg(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // sc1 load
__device__ __forceinline__ int mf_wave_or(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

struct RelaxWaveLds { int d[MF_RT + 2][MF_RT + 2]; uint32_t m[MF_RT][MF_RT / 4]; };   // one per wave

// ---- relabel tile visit -----------------------------------------------------------------------------------------
// d(p) = 1 + min over residual arcs p -> q of d(q), relaxed to the tile's fixpoint against a fixed halo.  A sweep where
// every pixel looks at its 8 neighbours once moves the BFS front one pixel (32+ sweeps per tile, each a chain of LDS round
// trips).  Here a lane owns 16 consecutive pixels of one column (V sweep) or of one row (H sweep): it reads its 18x3
// window in one batch, runs a forward and a backward pass over its pixels IN REGISTERS (a front travels the whole
// segment in one pass), and stores what changed.  Alternating V and H sweeps carry a front across the tile in a
// handful of sweeps; the arithmetic is branch-free (a missing arc ORs the "infinite" bit into the neighbour's label).
__device__ __forceinline__ int gated(int v, uint32_t inv, int bit) {        // v if the arc exists, >= DINF otherwise
    return (__builtin_amdgcn_sbfe((int)inv, bit, 1) & DINF) | v;
}
__device__ __forceinline__ int min3i(int a, int b, int c) { return min(a, min(b, c)); }
// Five neighbours instead of eight: a pass that walks in one direction looks at the three neighbours it comes from and the two
// beside it; the opposite pass of the same sweep looks at the other three and the same two.  Together they cover all eight arcs,
// so a sweep that changes nothing is still a fixpoint test, and the fixpoint (the exact distances) is the same — at 10 gated
// minima per pixel and sweep instead of 16 (the sweeps are bound by instruction issue: ~1 100 instructions each before).
// bA..bE: bit offsets of the five arcs inside the pixel's mask byte.
template <int bA, int bB, int bC, int bD, int bE>
__device__ __forceinline__ int relax_px5(int c, uint32_t inv, int pos, int vA, int vB, int vC, int vD, int vE) {
    const int nd = min3i(min3i(gated(vA, inv, pos + bA), gated(vB, inv, pos + bB), gated(vC, inv, pos + bC)),
                         gated(vD, inv, pos + bD), gated(vE, inv, pos + bE));
    return min(c, nd + 1);
}


// Arc masks of a 32x32 relabel tile come from rmask (1 byte per pixel, kept current by the push visits for the arcs inside
// their 32x8 tile).  An arc that LEAVES its pixel's push tile may have been re-opened by a push from the neighbouring tile
// after the owner wrote the mask, so those bits are taken from the capacities themselves: rows with y % 8 == 0 / 7 (arcs
// up / down: rows 0, 8 / 7, 15 of the lane's V-sweep segment) and columns 0 / 31 (arcs left / right: the lane's H-sweep
// pixel of that column).  15 loads per lane.  Masks are INVERTED (bit set = no arc).
struct MfBorderArcs {
    int fr[4][3], fc[3];
    __device__ __forceinline__ void load(const GcDims& d, const int32_t* __restrict__ rc, size_t BP, size_t base, int ty0, int tx0,
                                         int lx, int h) {
        const size_t cx = min(tx0 + lx, d.W - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                      // q: rows 0, 7, 8, 15 of the lane's segment
            const int r = (q >> 1) * 8 + ((q & 1) ? 7 : 0);
            const size_t i = base + (size_t)min(ty0 + 16 * h + r, d.H - 1) * d.W + cx;
#pragma unroll
            for (int t = 0; t < 3; ++t) fr[q][t] = rc[rc_idx(((q & 1) ? 3 + 2 * t : 2 + 2 * t), i)];   // 3,5,7 | 2,4,6
        }
        const size_t i = base + (size_t)min(ty0 + lx, d.H - 1) * d.W + min(tx0 + (h ? 31 : 0), d.W - 1);   // H-sweep row lx
        fc[0] = rc[rc_idx((h ? 1 : 0), i)];
        fc[1] = rc[rc_idx((h ? 5 : 4), i)];
        fc[2] = rc[rc_idx((h ? 6 : 7), i)];
    }
    // inverted mask of row r (0..15) of the lane's segment
    __device__ __forceinline__ uint32_t row(uint32_t m, int r) const {
        if ((r & 7) == 0 || (r & 7) == 7) {
            const int q = (r >> 3) * 2 + ((r & 7) ? 1 : 0);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const uint32_t bit = 1u << (((r & 7) ? 3 : 2) + 2 * t);
                m = (fr[q][t] > 0) ? (m & ~bit) : (m | bit);
            }
        }
        return m;
    }
    // inverted mask of the pixel (row lx, column h ? 31 : 0)
    __device__ __forceinline__ uint32_t col(uint32_t m, int h) const {
        const uint32_t b0 = 1u << (h ? 1 : 0), b1 = 1u << (h ? 5 : 4), b2 = 1u << (h ? 6 : 7);
        m = (fc[0] > 0) ? (m & ~b0) : (m | b0);
        m = (fc[1] > 0) ? (m & ~b1) : (m | b1);
        m = (fc[2] > 0) ? (m & ~b2) : (m | b2);
        return m;
    }
};

// A push tile is DIRTY when a neighbouring tile pushed into it since its masks were last exact (k_build_graph, or a relabel
// visit that re-read its border arcs): only then can a border bit of rmask be stale, and only then does a relabel visit pay
// for the 15 border loads — 4 us of its 10 us load phase, the three column loads being 64 scattered lines each.  The visit
// that re-reads them writes the corrected bytes back and clears the flags (relabel and push phases alternate, nothing moves
// capacities during a relabel), so later relabels of the solve take the short path until the next push across that edge.
// dirty: one word per 32x8 push tile.  Returns whether any of the relabel tile's (up to) 4 push tiles is dirty (wave-uniform).
__device__ __forceinline__ bool mf_tile_dirty(const int32_t* __restrict__ dirty, const MfTiles& tl, int b, int tyi, int txi, int lane) {
    const int py = tyi * (MF_RT / MF_PT_H) + (lane & 3);
    const int v = (lane < 4 && py < tl.pt_y) ? dirty[(size_t)b * tl.pt_x * tl.pt_y + (size_t)py * tl.pt_x + txi] : 0;
    return __any(v != 0);
}
// after the row and column patches: the corrected mask bytes of the border pixels go back to rmask, the flags are cleared
__device__ __forceinline__ void mf_tile_repair(const GcDims& d, const MfTiles& tl, uint8_t* __restrict__ rmask, int32_t* __restrict__ dirty,
                                               const RelaxWaveLds& S, size_t base, int b, int tyi, int txi, int ty0, int tx0, int lx, int h, int lane) {
    const uint8_t* sm = reinterpret_cast<const uint8_t*>(&S.m[0][0]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (q >> 1) * 8 + ((q & 1) ? 7 : 0);
        const int y = ty0 + 16 * h + r, x = tx0 + lx;
        if (x < d.W && y < d.H) rmask[base + (size_t)y * d.W + x] = (uint8_t)(~sm[(16 * h + r) * MF_RT + lx] & 0xffu);
    }
    {
        const int y = ty0 + lx, x = tx0 + (h ? 31 : 0);
        if (x < d.W && y < d.H) rmask[base + (size_t)y * d.W + x] = (uint8_t)(~sm[lx * MF_RT + (h ? 31 : 0)] & 0xffu);
    }
    const int py = tyi * (MF_RT / MF_PT_H) + (lane & 3);
    if (lane < 4 && py < tl.pt_y) dirty[(size_t)b * tl.pt_x * tl.pt_y + (size_t)py * tl.pt_x + txi] = 0;
}

// lane = (column lx, half h): pixels (rows 16h .. 16h+15, column lx).  Returns 1 when a label changed.
__device__ __forceinline__ int relax_sweep_v(RelaxWaveLds& S, const uint32_t (&inv_in)[4], int lx, int h) {
    // the per-arc gate words are loop invariants of the caller's sweep loop: hide the masks from the optimiser, or it hoists
    // 128 of them out of the loop and spills
    uint32_t inv[4] = {inv_in[0], inv_in[1], inv_in[2], inv_in[3]};
    asm volatile("" : "+v"(inv[0]), "+v"(inv[1]), "+v"(inv[2]), "+v"(inv[3]));
    int w[18][3];
#pragma unroll
    for (int a = 0; a < 18; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[a][c] = S.d[16 * h + a][lx + c];
    uint32_t chg = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                          // downwards: left, right, up, up-left, up-right (bits 0, 1, 2, 4, 6)
        const int a = r + 1;
        const int nv = relax_px5<0, 1, 2, 4, 6>(w[a][1], inv[r >> 2], 8 * (r & 3), w[a][0], w[a][2], w[a - 1][1], w[a - 1][0], w[a - 1][2]);
        chg |= (nv != w[a][1]) ? 1u << r : 0u;
        w[a][1] = nv;
    }
#pragma unroll
    for (int r = 15; r >= 0; --r) {                         // upwards: left, right, down, down-right, down-left (bits 0, 1, 3, 5, 7)
        const int a = r + 1;
        const int nv = relax_px5<0, 1, 3, 5, 7>(w[a][1], inv[r >> 2], 8 * (r & 3), w[a][0], w[a][2], w[a + 1][1], w[a + 1][2], w[a + 1][0]);
        chg |= (nv != w[a][1]) ? 1u << r : 0u;
        w[a][1] = nv;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((chg >> r) & 1u) S.d[16 * h + r + 1][lx + 1] = w[r + 1][1];
    return chg != 0u;
}
// lane = (row ly, half h): pixels (row ly, columns 16h .. 16h+15)
__device__ __forceinline__ int relax_sweep_h(RelaxWaveLds& S, const uint32_t (&inv_in)[4], int ly, int h) {
    uint32_t inv[4] = {inv_in[0], inv_in[1], inv_in[2], inv_in[3]};
    asm volatile("" : "+v"(inv[0]), "+v"(inv[1]), "+v"(inv[2]), "+v"(inv[3]));
    int w[3][18];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 18; ++c) w[a][c] = S.d[ly + a][16 * h + c];
    uint32_t chg = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {                          // rightwards: up, down, left, up-left, down-left (bits 2, 3, 0, 4, 7)
        const int c = k + 1;
        const int nv = relax_px5<2, 3, 0, 4, 7>(w[1][c], inv[k >> 2], 8 * (k & 3), w[0][c], w[2][c], w[1][c - 1], w[0][c - 1], w[2][c - 1]);
        chg |= (nv != w[1][c]) ? 1u << k : 0u;
        w[1][c] = nv;
    }
#pragma unroll
    for (int k = 15; k >= 0; --k) {                         // leftwards: up, down, right, up-right, down-right (bits 2, 3, 1, 6, 5)
        const int c = k + 1;
        const int nv = relax_px5<2, 3, 1, 6, 5>(w[1][c], inv[k >> 2], 8 * (k & 3), w[0][c], w[2][c], w[1][c + 1], w[0][c + 1], w[2][c + 1]);
        chg |= (nv != w[1][c]) ? 1u << k : 0u;
        w[1][c] = nv;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if ((chg >> k) & 1u) S.d[ly + 1][16 * h + k + 1] = w[1][k + 1];
    return chg != 0u;
}

// GGC_MF_TRACE: the phases of a wave's relabel visits in wall_clock64 ticks, kept in registers (PROF = false: nothing).
// The kernel stamps the start of a visit (begin) and adds the visit up after its hand-over (end); mf_relax_visit stamps the sweeps.
template <bool PROF>
struct MfRelaxClocks {
    long long t0 = 0, t1 = 0, t2 = 0;      // this visit: start, first sweep, end of the sweeps
    int n_sw = 0, n_lv = 0, n_fb = 0;      // this visit's sweeps, BFS levels, 1 when the BFS handed it to the sweeps
    long long sum[7] = {0, 0, 0, 0, 0, 0, 0};   // load + fill, sweeps | levels, write-back + hand-over, visits, sweeps, BFS levels, fallbacks
    __device__ __forceinline__ long long now() const { return PROF ? wall_clock64() : 0; }
    __device__ __forceinline__ void begin() { t0 = now(); n_sw = n_lv = n_fb = 0; }
    __device__ __forceinline__ void end() {
        if (PROF) {
            sum[0] += t1 - t0; sum[1] += t2 - t1; sum[2] += wall_clock64() - t2; sum[3] += 1; sum[4] += n_sw; sum[5] += n_lv; sum[6] += n_fb;
        }
    }
};

// ---- relabel tile visit as a level-synchronous BFS on bit rows ------------------------------------------------------
// Every arc has length 1, so the fixpoint of a visit whose labelled pixels are all sink pixels (label 1) is a multi-source
// BFS: from the label-1 pixels at level 1 and from the halo, a border pixel entering at 1 + the lowest halo label behind
// its arcs that leave the tile.  Lane r (both halves of the wave carry the same rows) holds row r as 32-bit words: A[dir]
// (bit x: pixel (r, x) has a residual arc towards dir), `done`, `front`.  A level is eight shifted ANDs against the front
// rows r - 1, r, r + 1 — 75 instructions for the whole tile, where a min-plus sweep is ~640.  A pixel's level INDEX
// (< MF_BFS_CAP <= 128) is kept in seven bit planes, the level's label in a table (levels skip when the front runs dry and
// the next source enters), so nothing is stored per pixel inside the loop; one decode pass writes the labels that fell.
// The sweeps remain the general visit: a start label below the BFS label (or a labelled pixel the BFS does not reach)
// would have to be carried on, and a tile with more than MF_BFS_CAP levels (corridors: the serpentine nets have in-tile
// paths of 1 024) is theirs too.  Both tests are wave-uniform; a visit that fails the first puts the start labels back.
#ifndef GGC_MF_RELAX_BFS
#define GGC_MF_RELAX_BFS 1          // k_mf_relax_wave: 1 = BFS visit with the sweeps as fallback, 0 = sweeps only
#endif
constexpr int MF_BFS_CAP = 96;      // levels per visit; an unobstructed front crosses the tile in 32

__device__ __forceinline__ uint64_t bit_transpose8(uint64_t x) {            // 8x8 bits: bit 8 i + j <-> bit 8 j + i
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}
__device__ __forceinline__ int mf_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
// entry level of a border pixel: 1 + the lowest halo label behind an open arc (b*: the INVERTED arc bit), DINF if none
__device__ __forceinline__ int mf_entry3(int v0, uint32_t b0, int v1, uint32_t b1, int v2, uint32_t b2) {
    const int m = min3i((b0 & 1u) ? DINF : v0, (b1 & 1u) ? DINF : v1, (b2 & 1u) ? DINF : v2);
    return min(m, DINF - 1) + 1;
}

// S.d / S.m as the load phase left them, old[]: the lane's 16 start labels (rows 16h .., column lx).  Returns true with the
// visit's labels in S.d, or false with S.d as it was (the caller sweeps).  S.m is dead once the arc rows are in registers
// (the caller holds its gate words already): its first MF_BFS_CAP words become the level table.
template <bool PROF>
__device__ __forceinline__ bool mf_relax_visit_bfs(RelaxWaveLds& S, const int (&old)[16], int lane, MfRelaxClocks<PROF>& ck) {
    constexpr int T = MF_RT;
    static_assert(MF_BFS_CAP <= 4 * T && MF_BFS_CAP <= 128 && MF_BFS_CAP * 4 <= (int)sizeof(S.m), "level index: 7 bits; table inside S.m");
    const int r = lane & 31, h = lane >> 5;
    const uint8_t* sm = reinterpret_cast<const uint8_t*>(&S.m[0][0]);
    int* lv = reinterpret_cast<int*>(&S.m[0][0]);
    uint32_t A[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                          // 8 pixels x 8 arcs at a time
        const uint64_t x = bit_transpose8((uint64_t)S.m[r][2 * g] | (uint64_t)S.m[r][2 * g + 1] << 32);
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) A[dir] |= (uint32_t)((x >> (8 * dir)) & 0xffu) << (8 * g);
    }
#pragma unroll
    for (int dir = 0; dir < 8; ++dir) A[dir] = ~A[dir];                    // the bytes are inverted
    // entry levels: left / right border pixel of row r; lanes 0..31 the top row's pixel x = r, lanes 32..63 the bottom row's
    const int eL = mf_entry3(S.d[r][0], ~A[4], S.d[r + 1][0], ~A[0], S.d[r + 2][0], ~A[7]);
    const int eR = mf_entry3(S.d[r][T + 1], ~A[6] >> 31, S.d[r + 1][T + 1], ~A[1] >> 31, S.d[r + 2][T + 1], ~A[5] >> 31);
    const uint32_t ib = sm[(h ? T - 1 : 0) * T + r];
    const int hr = h ? T + 1 : 0;
    const int eTB = mf_entry3(S.d[hr][r], ib >> (h ? 7 : 4), S.d[hr][r + 1], ib >> (h ? 3 : 2), S.d[hr][r + 2], ib >> (h ? 5 : 6));
    uint32_t one = 0u;                                                      // row r: pixels that start at label 1
#pragma unroll
    for (int q = 0; q < 16; ++q) {                                         // a ballot over the column layout IS two bit rows
        const unsigned long long bal = __ballot(old[q] == 1);
        one = (r == q) ? (uint32_t)bal : one;
        one = (r == 16 + q) ? (uint32_t)(bal >> 32) : one;
    }
    mf_wave_sync();                                                        // S.m is read: the level table may overwrite it
    uint32_t done = 0u, front = 0u, pl[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const int up_lane = (r == 0 ? lane : lane - 1) * 4, dn_lane = (r == T - 1 ? lane : lane + 1) * 4;   // ds_bpermute byte addresses
    const uint32_t up_ok = r == 0 ? 0u : ~0u, dn_ok = r == T - 1 ? 0u : ~0u;    // row 0 has no row above in the tile, row 31 none below
    // the lowest entry level still pending (DINF: none) — at the start and whenever the front runs dry
    auto next_level = [&]() {
        int c = (one & ~done) ? 1 : DINF;
        c = min(c, (done & 1u) ? DINF : eL);
        c = min(c, (done >> 31) ? DINF : eR);
        const uint32_t d0 = __builtin_amdgcn_readlane(done, 0), d31 = __builtin_amdgcn_readlane(done, 31);
        c = min(c, (((h ? d31 : d0) >> r) & 1u) ? DINF : eTB);
        return __builtin_amdgcn_readfirstlane(mf_wave_min(c));
    };
    int L = next_level();                                                  // wave-uniform, kept scalar
    bool finished = L >= DINF;
    for (int k = 0; k < MF_BFS_CAP && !finished; ++k) {
        if (lane == 0) lv[k] = L;
        const unsigned long long tb = __ballot(eTB == L);                  // top row's entries | bottom row's entries
        uint32_t own = (eL == L ? 1u : 0u) | (eR == L ? 0x80000000u : 0u);
        own |= ((uint32_t)tb & ~up_ok) | ((uint32_t)(tb >> 32) & ~dn_ok);
        if (L == 1) own |= one;
        const uint32_t fu = (uint32_t)__builtin_amdgcn_ds_bpermute(up_lane, (int)front) & up_ok;   // rows r - 1, r + 1
        const uint32_t fd = (uint32_t)__builtin_amdgcn_ds_bpermute(dn_lane, (int)front) & dn_ok;
        const uint32_t reach = (A[0] & (front << 1)) | (A[1] & (front >> 1)) | (A[2] & fu) | (A[3] & fd) |
                               (A[4] & (fu << 1)) | (A[5] & (fd >> 1)) | (A[6] & (fu >> 1)) | (A[7] & (fd << 1));
        const uint32_t nw = (reach | own) & ~done;
        done |= nw;
#pragma unroll
        for (int j = 0; j < 7; ++j) pl[j] |= ((k >> j) & 1) ? nw : 0u;
        front = nw;
        if (PROF) ++ck.n_lv;
        if (__any(nw != 0u)) ++L;
        else { L = next_level(); finished = L >= DINF; }
    }
    if (!finished) return false;
    mf_wave_sync();
    // decode: lane (r, h) has columns 16h .. 16h + 15 of row r
    uint32_t viol = 0u;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        uint64_t x = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) x |= (uint64_t)((pl[j] >> (16 * h + 8 * g)) & 0xffu) << (8 * j);
        x = bit_transpose8(x);                                             // byte i: level index of pixel 8g + i
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = 16 * h + 8 * g + i;
            const bool reached = (done >> c) & 1u;
            const int start = S.d[r + 1][c + 1];
            const int b = reached ? lv[(int)((x >> (8 * i)) & 0x7fu)] : DINF;
            viol |= reached ? (uint32_t)(start < b) : (uint32_t)(start != DINF);
            if (b < start) S.d[r + 1][c + 1] = b;
        }
    }
    mf_wave_sync();
    if (__any(viol != 0u)) {                                               // back to the start labels (column layout)
#pragma unroll
        for (int q = 0; q < 16; ++q) S.d[16 * h + q + 1][r + 1] = old[q];
        mf_wave_sync();
        return false;
    }
    return true;
}

// One wave relabels the 32x32 tile `tile`: labels of tile + halo and arc masks to LDS (border arcs of a dirty tile re-read
// and repaired), V and H sweeps to the tile's fixpoint, changed labels back to dist.  Returns, in every lane, the 9-bit mask
// of the tiles whose halo changed, bit (dy + 1) * 3 + (dx + 1), with bit 4 when the sweeps stopped short of the fixpoint.
//   ASYNC = false (k_mf_relax_wave, launches over work lists): plain loads and stores of dist, which the kernel boundaries
//           order; the visit consumes the tile's membership flag itself once its loads are issued.
//   ASYNC = true (k_mf_relax_async, one launch for the whole front): labels are read with sc1 loads and lowered with a
//           device-scope atomicMin (ggc_maxflow_async.hip); the caller consumes the flag when it pops the tile.
//   BFS (k_mf_relax_wave only): mf_relax_visit_bfs first, the sweeps where it declines.
template <bool ASYNC, bool PROF, bool BFS = false>
__device__ __forceinline__ int mf_relax_visit(const GcDims& d, const MfTiles& tl, int tile, int lane, RelaxWaveLds& S,
                                              uint8_t* rmask, int32_t* dirty, const int32_t* rc,
                                              int32_t* dist, int32_t* flag, MfRelaxClocks<PROF>& ck) {
    constexpr int T = MF_RT, N_HALO = (T + 2) * (T + 2), HALO_IT = (N_HALO + 63) / 64;
    int* sd = &S.d[0][0];
    uint8_t* sm = reinterpret_cast<uint8_t*>(&S.m[0][0]);
    const int tiles_per_image = tl.rt_x * tl.rt_y;
    const int b = tile / tiles_per_image, tr = tile % tiles_per_image;
    const int tyi = tr / tl.rt_x, txi = tr % tl.rt_x;
    const int tx0 = txi * T, ty0 = tyi * T;
    const size_t base = (size_t)b * d.P, BP = (size_t)d.B * d.P;
    const int lx = lane & 31, h = lane >> 5;
    int hv[HALO_IT];
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {                                    // unconditional loads from clamped addresses
        const int i = min(lane + k * 64, N_HALO - 1);
        const int gy = ty0 + i / (T + 2) - 1, gx = tx0 + i % (T + 2) - 1;
        const int32_t* p = &dist[base + (size_t)min(max(gy, 0), d.H - 1) * d.W + min(max(gx, 0), d.W - 1)];
        hv[k] = ASYNC ? ldg(p) : *p;
    }
    uint32_t mv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)                                           // arc masks do not change during a relabel: plain loads
        mv[r] = rmask[base + (size_t)min(ty0 + 16 * h + r, d.H - 1) * d.W + min(tx0 + lx, d.W - 1)];
    const bool dirty_t = mf_tile_dirty(dirty, tl, b, tyi, txi, lane);      // wave-uniform: a neighbour pushed into one of its push tiles
    MfBorderArcs ba;                                                       // (capacities do not change during a relabel either)
    if (dirty_t) ba.load(d, rc, BP, base, ty0, tx0, lx, h);
    if (!ASYNC && lane == 0) flag[tile] = 0;                               // consumed
    uint32_t inv_v[4] = {0u, 0u, 0u, 0u}, inv_h[4];                        // bit set = no arc; outside the image: all blocked
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        uint32_t m = ~mv[r] & 0xffu;
        if (dirty_t) m = ba.row(m, r);
        sm[(16 * h + r) * T + lx] = (uint8_t)((tx0 + lx < d.W && ty0 + 16 * h + r < d.H) ? m : 0xffu);
    }
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {
        const int i = lane + k * 64;
        const int gy = ty0 + i / (T + 2) - 1, gx = tx0 + i % (T + 2) - 1;
        if (i < N_HALO) sd[i] = (gx >= 0 && gx < d.W && gy >= 0 && gy < d.H) ? hv[k] : DINF;
    }
    mf_wave_sync();
    if (dirty_t) {      // (a second wave relaxing the same tile meanwhile writes the same bytes)
        if (ty0 + lx < d.H && tx0 + (h ? 31 : 0) < d.W) sm[lx * T + (h ? 31 : 0)] = (uint8_t)ba.col(sm[lx * T + (h ? 31 : 0)], h);
        mf_wave_sync();
        mf_tile_repair(d, tl, rmask, dirty, S, base, b, tyi, txi, ty0, tx0, lx, h, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) inv_v[r >> 2] |= (uint32_t)sm[(16 * h + r) * T + lx] << (8 * (r & 3));
#pragma unroll
    for (int k = 0; k < 4; ++k) inv_h[k] = S.m[lx][4 * h + k];             // H sweep: row lx, columns 16h .. 16h+15
    int old[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) old[r] = S.d[16 * h + r + 1][lx + 1];
    bool settled = false;
    ck.t1 = ck.now();
    if (BFS) {
        settled = mf_relax_visit_bfs<PROF>(S, old, lane, ck);
        if (PROF && !settled) ck.n_fb = 1;
    }
    for (int it = 0; it < 4 * T && !(BFS && settled); ++it) {   // a sweep pair that changes nothing: fixpoint (a visit capped at 2-6 sweeps and re-queued
                                           // publishes its border earlier, but costs more visits: 56.4 -> 60.3 / 58.1 / 56.6 ms)
        const int ch = (it & 1) ? relax_sweep_h(S, inv_h, lx, h) : relax_sweep_v(S, inv_v, lx, h);
        mf_wave_sync();
        if (PROF) ++ck.n_sw;
        if (!__any(ch)) { settled = true; break; }
    }
    ck.t2 = ck.now();
    int nbm = settled ? 0 : 1 << 4;                                        // bit (dy + 1) * 3 + (dx + 1)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ly = 16 * h + r;
        const int v = S.d[ly + 1][lx + 1];
        if (v != old[r]) {                                                 // (pixels outside the image never change: all arcs blocked)
            int32_t* p = &dist[base + (size_t)(ty0 + ly) * d.W + tx0 + lx];
            if (ASYNC) atomicMin(p, v); else *p = v;                       // (asynchronous: labels only fall)
            const int Lf = lx == 0, Rt = lx == T - 1, U = ly == 0, D = ly == T - 1;
            nbm |= (U & Lf) | U << 1 | (U & Rt) << 2 | Lf << 3 | Rt << 5 | (D & Lf) << 6 | D << 7 | (D & Rt) << 8;
        }
    }
    return mf_wave_or(nbm);
}

} // namespace ggc
