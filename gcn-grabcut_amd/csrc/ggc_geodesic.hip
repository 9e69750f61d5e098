// ggc_geodesic.hip — H1: geodesic click hints.  A click labels the pixels whose shortest-path cost to it, on the 8-connected
// grid with arcs that pay for colour change, is within a cap and smaller than the cost to any click of the other label
// (include/ggc.h has the exact integer definition).  Everything is int32; the result is the unique fixed point of
// d(p) = min(d(p), min_q d(q) + c(p,q)), so it does not depend on the order in which tiles or pixels are relaxed.
//
//   k_geo_guide   streaming, one lane per pixel: the 3x3 box sums S (three u16 per pixel) and both distance planes filled
//                 with the cap limit + 1, which doubles as "infinity": a relaxed value above the limit never replaces it,
//                 and a shortest path of cost <= limit has only prefixes of cost <= limit, so nothing below the cap is lost.
//   k_geo_seed    one lane per click: a click that a later click of its image repeats is dropped (last click wins), the
//                 others write distance 0 into their label's plane and put their 32x32 tile, and the tiles that hold the
//                 pixel in their halo, on the first work list.
//   k_geo_round   one launch per round, one workgroup per listed tile (grid-stride).  The visit stages S and both planes of
//                 tile + halo in LDS, turns S into the four arc-cost tables of the tile (E, S, SE, SW; the other four arcs
//                 are the same tables read from the neighbour; an arc with an end outside the image costs GEO_BLOCKED), and
//                 relaxes to the tile's fixed point against the fixed halo: alternating column and row sweeps in which a
//                 lane walks 8 pixels forwards and backwards in place, so a front crosses the tile in a few sweeps.  Lowered
//                 pixels go back with plain stores; a lowered border pixel puts the tiles that see it in their halo on the
//                 next round's list (a stamp per tile keeps a tile from being listed twice, integer atomics only).  A tile
//                 read by a neighbour in the same launch may show the old or the new value: either is a valid upper bound,
//                 and the lowering lists that neighbour for the next round, where the kernel boundary makes it visible.
//   k_geo_label   over the tiles that were ever listed: the label rule on the mask and the per-superpixel minima by atomicMin.
// Since every arc costs at least 80, a tile farther than `radius` pixels from every click is never listed: beyond the two
// streaming launches the work is O(clicks x radius^2).
#include "ggc_internal.h"
#include <algorithm>

namespace ggc {
namespace {

constexpr int GEO_T = 32, GEO_H = GEO_T + 2;          // tile edge, with halo
constexpr int GEO_S = GEO_H + 1;                       // LDS row stride: odd, so that a row sweep's 32 rows fall into 32 banks
constexpr int GEO_N = GEO_H * GEO_S;
constexpr int GEO_THREADS = 256;
constexpr int GEO_AXIAL = 80, GEO_DIAG = 113;          // 80 * sqrt(2) = 113.14
constexpr int GEO_BLOCKED = 1 << 29;                   // cap (<= 1 310 721) + GEO_BLOCKED fits int32 and never lowers anything
// A sweep relaxes every pixel against all 8 neighbours, so a sweep that changes something makes at least one more pixel of
// the tile final (the unsettled pixel of smallest final value): 1024 sweeps settle a plane, one more sees no change.
constexpr int GEO_MAX_SWEEPS = GEO_T * GEO_T + 1;

struct GeoDims { int B, H, W, tiles_x, tiles_y, cap, gamma; };   // cap = limit + 1

struct GeoWork {
    uint16_t* S;                 // [B,H,W,3] box sums
    int32_t* plane[2];           // [B,H,W] foreground / background distances (the caller's buffers when given)
    int32_t* stamp;              // per tile: 1 + the round it is listed for, 0 = never listed
    int32_t* list[2];            // ping-pong work lists
    int32_t* touched;            // every tile that was ever listed, once
    int32_t* cnt;                // [0..2] list lengths of rounds r, r+1, r+2 (mod 3), [3] length of touched
};

struct GeoLds {
    uint16_t s[3][GEO_N];
    int c[4][GEO_N];             // arc (y,x) -> (y,x+1), (y+1,x), (y+1,x+1), (y+1,x-1)
    int d[2][GEO_N];
    int nbm;
};

// image of click k: the last b with hint_ptr[b] <= k (hint_ptr is non-decreasing, checked on the host)
__device__ __forceinline__ int geo_click_image(const int32_t* __restrict__ hint_ptr, int B, int k) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hint_ptr[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// lists `tile` for the round whose stamp is `s`, once
__device__ __forceinline__ void geo_enqueue(const GeoWork& w, int tile, int s, int32_t* __restrict__ list, int32_t* cnt) {
    const int old = atomicExch(&w.stamp[tile], s);
    if (old == s) return;
    list[atomicAdd(cnt, 1)] = tile;
    if (old == 0) w.touched[atomicAdd(&w.cnt[3], 1)] = tile;
}

__global__ void __launch_bounds__(256) k_geo_guide(GeoDims d, size_t total, const uint8_t* __restrict__ bgr, GeoWork w) {
    const size_t P = (size_t)d.H * d.W;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const size_t b = p / P, q = p - b * P;
        const int y = (int)(q / d.W), x = (int)(q - (size_t)y * d.W);
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const size_t row = b * P + (size_t)min(max(y + dy, 0), d.H - 1) * d.W;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const uint8_t* px = bgr + 3 * (row + min(max(x + dx, 0), d.W - 1));
                s0 += px[0]; s1 += px[1]; s2 += px[2];
            }
        }
        w.S[3 * p] = (uint16_t)s0; w.S[3 * p + 1] = (uint16_t)s1; w.S[3 * p + 2] = (uint16_t)s2;
        w.plane[0][p] = d.cap;
        w.plane[1][p] = d.cap;
    }
}

__global__ void __launch_bounds__(256) k_geo_fill(size_t n, int v, int32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

__global__ void __launch_bounds__(256) k_geo_seed(GeoDims d, int K, const int32_t* __restrict__ hints,
                                                  const int32_t* __restrict__ hint_ptr, GeoWork w) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int r = hints[3 * k], c = hints[3 * k + 1], fg = hints[3 * k + 2] != 0;
    if (r < 0 || r >= d.H || c < 0 || c >= d.W) return;                    // outside its image: ignored
    const int b = geo_click_image(hint_ptr, d.B, k);
    for (int j = k + 1; j < hint_ptr[b + 1]; ++j)                          // a later click on the same pixel wins
        if (hints[3 * j] == r && hints[3 * j + 1] == c) return;
    w.plane[fg ? 0 : 1][(size_t)b * d.H * d.W + (size_t)r * d.W + c] = 0;   // one surviving click per pixel: no two writers
    // its own tile and every tile that holds the pixel in its halo: a visit reports only the pixels it lowers itself
    const int tyi = r / GEO_T, txi = c / GEO_T, ly = r % GEO_T, lx = c % GEO_T;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const bool sees = (dy == 0 || (dy < 0 ? ly == 0 : ly == GEO_T - 1)) && (dx == 0 || (dx < 0 ? lx == 0 : lx == GEO_T - 1));
            const int ny = tyi + dy, nx = txi + dx;
            if (sees && ny >= 0 && ny < d.tiles_y && nx >= 0 && nx < d.tiles_x)
                geo_enqueue(w, (b * d.tiles_y + ny) * d.tiles_x + nx, 1, w.list[0], &w.cnt[0]);
        }
}

// relaxes the pixel at LDS index i against its 8 neighbours; returns the new value
__device__ __forceinline__ int geo_relax(const int* dd, const GeoLds& L, int i) {
    const int a = min(min(dd[i - 1] + L.c[0][i - 1], dd[i + 1] + L.c[0][i]),
                      min(dd[i - GEO_S] + L.c[1][i - GEO_S], dd[i + GEO_S] + L.c[1][i]));
    const int e = min(min(dd[i - GEO_S - 1] + L.c[2][i - GEO_S - 1], dd[i + GEO_S + 1] + L.c[2][i]),
                      min(dd[i - GEO_S + 1] + L.c[3][i - GEO_S + 1], dd[i + GEO_S - 1] + L.c[3][i]));
    return min(dd[i], min(a, e));
}

// A lane owns 8 consecutive pixels of one column (step = GEO_S) or one row (step = 1) of one plane and walks them there
// and back, in place.  Pixels of other lanes are read while their owners may lower them: any value seen is the cost of a
// real path, values only fall, and the sweep that ends the visit changed nothing, so all its reads saw final values.
__device__ __forceinline__ bool geo_sweep(GeoLds& L, int pl, int first, int step) {
    int* dd = L.d[pl];
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = first + k * step, v = geo_relax(dd, L, i);
        if (v != dd[i]) { dd[i] = v; changed = true; }
    }
#pragma unroll
    for (int k = 6; k >= 0; --k) {
        const int i = first + k * step, v = geo_relax(dd, L, i);
        if (v != dd[i]) { dd[i] = v; changed = true; }
    }
    return changed;
}

__global__ void __launch_bounds__(GEO_THREADS) k_geo_round(GeoDims d, int round, GeoWork w) {
    __shared__ GeoLds L;
    const int tid = threadIdx.x;
    int32_t* cur = w.list[round & 1];
    int32_t* nxt = w.list[(round + 1) & 1];
    const int n = w.cnt[round % 3];
    int32_t* cnt_next = &w.cnt[(round + 1) % 3];
    if (blockIdx.x == 0 && tid == 0) w.cnt[(round + 2) % 3] = 0;           // read by the previous launch, appended to by the next
    const int tpi = d.tiles_x * d.tiles_y;
    const size_t P = (size_t)d.H * d.W;
    for (int li = blockIdx.x; li < n; li += gridDim.x) {                   // block-uniform
        const int tile = cur[li];
        const int b = tile / tpi, tr = tile - b * tpi, tyi = tr / d.tiles_x, txi = tr - tyi * d.tiles_x;
        const int ty0 = tyi * GEO_T, tx0 = txi * GEO_T;
        const size_t base = (size_t)b * P;
        if (tid == 0) L.nbm = 0;
        for (int i = tid; i < GEO_H * GEO_H; i += GEO_THREADS) {
            const int hy = i / GEO_H, hx = i - hy * GEO_H, gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            const bool in = gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
            const size_t p = base + (size_t)min(max(gy, 0), d.H - 1) * d.W + min(max(gx, 0), d.W - 1);
            const int j = hy * GEO_S + hx;
            L.s[0][j] = w.S[3 * p]; L.s[1][j] = w.S[3 * p + 1]; L.s[2][j] = w.S[3 * p + 2];
            L.d[0][j] = in ? w.plane[0][p] : d.cap;
            L.d[1][j] = in ? w.plane[1][p] : d.cap;
        }
        __syncthreads();
        for (int i = tid; i < GEO_H * GEO_H; i += GEO_THREADS) {
            const int hy = i / GEO_H, hx = i - hy * GEO_H, gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            const bool in = gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
            const int j = hy * GEO_S + hx;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int oy = a == 0 ? 0 : 1, ox = a == 0 ? 1 : (a == 1 ? 0 : (a == 2 ? 1 : -1));
                const bool ok = in && hy + oy < GEO_H && hx + ox >= 0 && hx + ox < GEO_H && gy + oy < d.H &&
                                gx + ox >= 0 && gx + ox < d.W;
                int c = GEO_BLOCKED;
                if (ok) {
                    const int q = j + oy * GEO_S + ox;
                    c = (a < 2 ? GEO_AXIAL : GEO_DIAG) +
                        d.gamma * (abs((int)L.s[0][j] - (int)L.s[0][q]) + abs((int)L.s[1][j] - (int)L.s[1][q]) +
                                   abs((int)L.s[2][j] - (int)L.s[2][q]));
                }
                L.c[a][j] = c;
            }
        }
        __syncthreads();
        // write-back ownership: rows tid / 32 + 8k of column tid % 32 (coalesced)
        const int wx = tid & 31, wy = tid >> 5;
        int old[2][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = (wy + 8 * k + 1) * GEO_S + wx + 1;
            old[0][k] = L.d[0][j]; old[1][k] = L.d[1][j];
        }
        __syncthreads();                                                   // the sweeps write what other lanes just read
        // sweep ownership: plane tid / 128, segment (tid / 32) % 4 of line tid % 32
        const int pl = tid >> 7, seg = (tid >> 5) & 3, line = tid & 31;
        const int first_v = (8 * seg + 1) * GEO_S + line + 1, first_h = (line + 1) * GEO_S + 8 * seg + 1;
        for (int it = 0; it < GEO_MAX_SWEEPS; ++it) {
            const bool ch = (it & 1) ? geo_sweep(L, pl, first_h, 1) : geo_sweep(L, pl, first_v, GEO_S);
            if (!__syncthreads_or(ch)) break;
        }
        int nbm = 0;                                                       // bit (dy + 1) * 3 + (dx + 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ly = wy + 8 * k, j = (ly + 1) * GEO_S + wx + 1;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int v = L.d[q][j];
                if (v != old[q][k]) {                                      // (a pixel outside the image never changes: its arcs are blocked)
                    w.plane[q][base + (size_t)(ty0 + ly) * d.W + tx0 + wx] = v;
                    const int Lf = wx == 0, Rt = wx == GEO_T - 1, U = ly == 0, D = ly == GEO_T - 1;
                    nbm |= (U & Lf) | U << 1 | (U & Rt) << 2 | Lf << 3 | Rt << 5 | (D & Lf) << 6 | D << 7 | (D & Rt) << 8;
                }
            }
        }
        if (nbm) atomicOr(&L.nbm, nbm);
        __syncthreads();
        if (tid < 9 && tid != 4 && ((L.nbm >> tid) & 1)) {
            const int ny = tyi + tid / 3 - 1, nx = txi + tid % 3 - 1;
            if (ny >= 0 && ny < d.tiles_y && nx >= 0 && nx < d.tiles_x)
                geo_enqueue(w, (b * d.tiles_y + ny) * d.tiles_x + nx, round + 2, nxt, cnt_next);
        }
        __syncthreads();                                                   // L is reused by the block's next tile
    }
}

__global__ void __launch_bounds__(GEO_THREADS) k_geo_label(GeoDims d, GeoWork w, const int32_t* __restrict__ segments,
                                                           const int32_t* __restrict__ node_ptr, uint8_t* __restrict__ mask,
                                                           int32_t* __restrict__ node_dist) {
    const int tid = threadIdx.x, n = w.cnt[3], tpi = d.tiles_x * d.tiles_y, limit = d.cap - 1;
    const size_t P = (size_t)d.H * d.W;
    for (int li = blockIdx.x; li < n; li += gridDim.x) {
        const int tile = w.touched[li];
        const int b = tile / tpi, tr = tile - b * tpi, tyi = tr / d.tiles_x, txi = tr - tyi * d.tiles_x;
        const int x = txi * GEO_T + (tid & 31);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = tyi * GEO_T + (tid >> 5) + 8 * k;
            if (x >= d.W || y >= d.H) continue;
            const size_t p = (size_t)b * P + (size_t)y * d.W + x;
            const int df = w.plane[0][p], db = w.plane[1][p];
            if (mask) {
                if (df <= limit && df < db) mask[p] = GGC_FGD;
                else if (db <= limit && db < df) mask[p] = GGC_BGD;
            }
            if (node_dist && (df <= limit || db <= limit)) {
                const int n0 = node_ptr[b], s = segments[p];
                if (s >= 0 && s < node_ptr[b + 1] - n0) {
                    if (df <= limit) atomicMin(&node_dist[2 * (size_t)(n0 + s)], df);
                    if (db <= limit) atomicMin(&node_dist[2 * (size_t)(n0 + s) + 1], db);
                }
            }
        }
    }
}

} // namespace
} // namespace ggc

extern "C" int ggc_geodesic_hints(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* hints,
                                  const int32_t* hint_ptr, int radius, int gamma, const int32_t* segments,
                                  const int32_t* node_ptr, uint8_t* mask, int32_t* dist_fg, int32_t* dist_bg,
                                  int32_t* node_dist) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, radius >= 0 && radius <= 16384, GGC_E_INVALID_ARG, "geodesic radius %d outside [0, 16384]", radius);
    GGC_REQUIRE(ctx, gamma >= 0 && gamma <= 64, GGC_E_INVALID_ARG, "geodesic gamma %d outside [0, 64]", gamma);
    GGC_REQUIRE(ctx, mask || dist_fg || dist_bg || node_dist, GGC_E_INVALID_ARG, "no output requested");
    GGC_REQUIRE(ctx, bgr && hint_ptr, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, !node_dist || (segments && node_ptr), GGC_E_INVALID_ARG, "node_dist needs segments and node_ptr");
    const int tiles_x = cdiv(W, GEO_T), tiles_y = cdiv(H, GEO_T);
    const int64_t n_tiles64 = (int64_t)B * tiles_x * tiles_y;
    GGC_REQUIRE(ctx, n_tiles64 <= (int64_t)1 << 30, GGC_E_SHAPE, "too many tiles (%lld)", (long long)n_tiles64);
    const int n_tiles = (int)n_tiles64;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> hp;
    int rc = read_offsets(ctx, st, hint_ptr, B, "hint_ptr", "image", 0, hp);
    if (rc) return rc;
    const int K = hp[B];
    if (K == 0) return GGC_OK;
    GGC_REQUIRE(ctx, hints, GGC_E_INVALID_ARG, "null hints with %d clicks", K);
    int64_t N = 0;
    if (node_dist) {
        std::vector<int32_t> np_;
        rc = read_offsets(ctx, st, node_ptr, B, "node_ptr", "image", 0, np_);
        if (rc) return rc;
        N = np_[B];
    }

    const size_t total = (size_t)B * H * W;
    GeoWork w{};
    int32_t* ctl = nullptr;
    if (!carve_scratch(ctx, S_GEODESIC, [&](Carve& c) {
            w.S = c.take<uint16_t>(3 * total);
            w.plane[0] = dist_fg ? dist_fg : c.take<int32_t>(total);
            w.plane[1] = dist_bg ? dist_bg : c.take<int32_t>(total);
            w.list[0] = c.take<int32_t>(n_tiles);
            w.list[1] = c.take<int32_t>(n_tiles);
            w.touched = c.take<int32_t>(n_tiles);
            ctl = c.take<int32_t>((size_t)n_tiles + 4);                  // stamps, then the four counters: one memset
        }))
        return GGC_E_OOM;
    w.stamp = ctl;
    w.cnt = ctl + n_tiles;
    GGC_HIP(ctx, hipMemsetAsync(ctl, 0, sizeof(int32_t) * ((size_t)n_tiles + 4), st));
    const int limit = GEO_AXIAL * radius;
    const GeoDims d{B, H, W, tiles_x, tiles_y, limit + 1, gamma};
    const int wide = 16 * std::max(ctx->n_cu, 1);                          // blocks of a grid-stride launch
    hipLaunchKernelGGL(k_geo_guide, dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)wide * 4)), dim3(256), 0, st, d, total, bgr, w);
    if (N > 0)
        hipLaunchKernelGGL(k_geo_fill, dim3(cdiv(2 * N, 256)), dim3(256), 0, st, (size_t)(2 * N), limit + 1, node_dist);
    hipLaunchKernelGGL(k_geo_seed, dim3(cdiv(K, 256)), dim3(256), 0, st, d, K, hints, hint_ptr, w);
    GGC_LAUNCH_CHECK(ctx);
    // Round bound.  Round j makes every pixel final whose shortest path crosses a tile edge at most j times: the path's
    // last crossing leaves a pixel that became final in a round before j, and the lowering that made it final listed the
    // tile entered for the following round, whose visit runs to the tile's fixed point and so covers the rest of the path.
    // A path within the cap has at most `radius` arcs (each costs >= 80), and a simple path through the image fewer arcs
    // than the image has pixels (at most 1024 per tile), so it crosses at most J = min(radius, 1024 * tiles - 1) edges.
    // Round J + 1 can still be listed (by the lowerings of round J) but lowers nothing: the list of round J + 2 is empty.
    const int max_rounds = (int)std::min<int64_t>(radius, (int64_t)GEO_T * GEO_T * tiles_x * tiles_y - 1) + 2;
    const int grid = std::min(n_tiles, wide);
    int round = 0, step = 4;                                               // a click's reach is a few tiles: look after 4 rounds, then every 8
    std::vector<int32_t> host;
    for (;;) {
        const int stop = std::min(round + step, max_rounds);
        for (; round < stop; ++round)
            hipLaunchKernelGGL(k_geo_round, dim3(grid), dim3(GEO_THREADS), 0, st, d, round, w);
        GGC_LAUNCH_CHECK(ctx);
        if ((rc = read_i32(ctx, st, w.cnt + round % 3, 1, host))) return rc;
        if (host[0] == 0) break;
        GGC_REQUIRE(ctx, round < max_rounds, GGC_E_DEVICE, "geodesic hints did not converge in %d rounds", max_rounds);
        step = 8;
    }
    if (mask || node_dist) {
        hipLaunchKernelGGL(k_geo_label, dim3(grid), dim3(GEO_THREADS), 0, st, d, w, segments, node_ptr, mask, N > 0 ? node_dist : nullptr);
        GGC_LAUNCH_CHECK(ctx);
    }
    return GGC_OK;
}
