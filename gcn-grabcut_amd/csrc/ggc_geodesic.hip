// ggc_geodesic.hip — H1: geodesic click hints.  A click labels the pixels whose shortest-path cost to it, on the 8-connected
// grid with arcs that pay for colour change, is within a cap and smaller than the cost to any click of the other label
// (include/ggc.h has the exact integer definition).  Everything is int32, and the two distance planes are fixed points that
// ggc_relax.h computes by tile relaxation, both planes in the same visits (PLANES = 2).
//
//   k_geo_guide   streaming, one lane per pixel: the 3x3 box sums S (three u16 per pixel) and both distance planes filled
//                 with the cap limit + 1, which doubles as "infinity": a relaxed value above the limit never replaces it,
//                 and a shortest path of cost <= limit has only prefixes of cost <= limit, so nothing below the cap is lost.
//   k_geo_seed    one lane per click: a click that a later click of its image repeats is dropped (last click wins), the
//                 others write distance 0 into their label's plane and put the tiles that hold the pixel on the first list.
//   k_geo_round   one round of ggc_relax.h: S and both planes of tile + halo staged in LDS (the halo outside the image holds
//                 the cap: cap (<= 1 310 721) + RX_BLOCKED fits int32 and lowers nothing), the arc tables from S, the visit.
//   k_geo_label   over the tiles that were ever listed: the label rule on the mask and the per-superpixel minima by atomicMin.
// Since every arc costs at least 80, a tile farther than `radius` pixels from every click is never listed: beyond the two
// streaming launches the work is O(clicks x radius^2).
#include "ggc_relax.h"

namespace ggc {
namespace {

struct GeoDims { int B, H, W, tiles_x, tiles_y, cap, gamma; };   // cap = limit + 1

struct GeoWork {
    uint16_t* S;                 // [B,H,W,3] box sums
    int32_t* plane[2];           // [B,H,W] foreground / background distances (the caller's buffers when given)
    RelaxLists q;                // with `touched`: k_geo_label runs over it
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
    const int tile0 = b * d.tiles_y * d.tiles_x;
    relax_tiles_holding(r / RX_T, c / RX_T, r % RX_T, c % RX_T, d.tiles_y, d.tiles_x,
                        [&](int ny, int nx) { relax_enqueue(w.q, tile0 + ny * d.tiles_x + nx, 1, w.q.list[0], &w.q.cnt[0]); });
}

__global__ void __launch_bounds__(RX_THREADS) k_geo_round(GeoDims d, int round, GeoWork w) {
    __shared__ struct { uint16_t S[3][RX_N]; RelaxLds<2> rx; } lds;   // the guide beside the relaxation's arrays
    auto& s_S = lds.S;
    RelaxLds<2>& L = lds.rx;
    const int tid = threadIdx.x;
    const RelaxRound rr = relax_round_begin(w.q, round);
    const int tpi = d.tiles_x * d.tiles_y;
    const size_t P = (size_t)d.H * d.W;
    for (int li = blockIdx.x; li < rr.n; li += gridDim.x) {                // block-uniform
        const int tile = rr.cur[li];
        const int b = tile / tpi, tr = tile - b * tpi, tyi = tr / d.tiles_x, txi = tr - tyi * d.tiles_x;
        const int ty0 = tyi * RX_T, tx0 = txi * RX_T;
        const size_t base = (size_t)b * P;
        const RelaxBox box = relax_box(ty0, tx0, d.H, d.W);
        for (int i = tid; i < RX_H * RX_H; i += RX_THREADS) {
            const int hy = i / RX_H, hx = i - hy * RX_H, gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            const bool in = box.has(hy, hx);
            const size_t p = base + (size_t)min(max(gy, 0), d.H - 1) * d.W + min(max(gx, 0), d.W - 1);
            const int j = hy * RX_S + hx;
            s_S[0][j] = w.S[3 * p]; s_S[1][j] = w.S[3 * p + 1]; s_S[2][j] = w.S[3 * p + 2];
            L.d[0][j] = in ? w.plane[0][p] : d.cap;
            L.d[1][j] = in ? w.plane[1][p] : d.cap;
        }
        __syncthreads();
        relax_arcs(L, box, [&](int j, int q, int len) {
            return len + d.gamma * (abs((int)s_S[0][j] - (int)s_S[0][q]) + abs((int)s_S[1][j] - (int)s_S[1][q]) +
                                    abs((int)s_S[2][j] - (int)s_S[2][q]));
        });
        __syncthreads();
        const int nbm = relax_visit(L, [&](int q, int ly, int lx, int v) {
            w.plane[q][base + (size_t)(ty0 + ly) * d.W + tx0 + lx] = v;
        });
        relax_list_neighbours(w.q, rr, nbm, tyi, txi, d.tiles_y, d.tiles_x, b * tpi);
    }
}

__global__ void __launch_bounds__(RX_THREADS) k_geo_label(GeoDims d, GeoWork w, const int32_t* __restrict__ segments,
                                                           const int32_t* __restrict__ node_ptr, uint8_t* __restrict__ mask,
                                                           int32_t* __restrict__ node_dist) {
    const int tid = threadIdx.x, n = *w.q.n_touched, tpi = d.tiles_x * d.tiles_y, limit = d.cap - 1;
    const size_t P = (size_t)d.H * d.W;
    for (int li = blockIdx.x; li < n; li += gridDim.x) {
        const int tile = w.q.touched[li];
        const int b = tile / tpi, tr = tile - b * tpi, tyi = tr / d.tiles_x, txi = tr - tyi * d.tiles_x;
        const int x = txi * RX_T + (tid & 31);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = tyi * RX_T + (tid >> 5) + 8 * k;
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
    const int tiles_x = cdiv(W, RX_T), tiles_y = cdiv(H, RX_T);
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
            w.q.list[0] = c.take<int32_t>(n_tiles);
            w.q.list[1] = c.take<int32_t>(n_tiles);
            w.q.touched = c.take<int32_t>(n_tiles);
            ctl = c.take<int32_t>((size_t)n_tiles + 4);                  // stamps, the lists' three counters, the length of touched: one memset
        }))
        return GGC_E_OOM;
    w.q.stamp = ctl;
    w.q.cnt = ctl + n_tiles;
    w.q.n_touched = ctl + n_tiles + 3;
    GGC_HIP(ctx, hipMemsetAsync(ctl, 0, sizeof(int32_t) * ((size_t)n_tiles + 4), st));
    const int limit = RX_AXIAL * radius;
    const GeoDims d{B, H, W, tiles_x, tiles_y, limit + 1, gamma};
    const int wide = 16 * std::max(ctx->n_cu, 1);                          // blocks of a grid-stride launch
    hipLaunchKernelGGL(k_geo_guide, dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)wide * 4)), dim3(256), 0, st, d, total, bgr, w);
    if (N > 0)
        hipLaunchKernelGGL(k_geo_fill, dim3(cdiv(2 * N, 256)), dim3(256), 0, st, (size_t)(2 * N), limit + 1, node_dist);
    hipLaunchKernelGGL(k_geo_seed, dim3(cdiv(K, 256)), dim3(256), 0, st, d, K, hints, hint_ptr, w);
    GGC_LAUNCH_CHECK(ctx);
    // Round bound (ggc_relax.h).  A path within the cap has at most `radius` arcs (each costs >= 80), and a simple path through
    // the image fewer arcs than the image has pixels, so it crosses at most J = min(radius, 1024 * tiles - 1) tile edges.
    const int64_t max_rounds = std::min<int64_t>(radius, (int64_t)RX_T * RX_T * tiles_x * tiles_y - 1) + 2;
    const int grid = std::min(n_tiles, wide);
    const auto launch_round = [&](int64_t round) {
        hipLaunchKernelGGL(k_geo_round, dim3(grid), dim3(RX_THREADS), 0, st, d, (int)round, w);
    };
    // a click's reach is a few tiles: look after 4 rounds, then every 8
    if ((rc = relax_rounds(ctx, st, launch_round, w.q.cnt, 4, 8, max_rounds, "geodesic hints"))) return rc;
    if (mask || node_dist) {
        hipLaunchKernelGGL(k_geo_label, dim3(grid), dim3(RX_THREADS), 0, st, d, w, segments, node_ptr, mask, N > 0 ? node_dist : nullptr);
        GGC_LAUNCH_CHECK(ctx);
    }
    return GGC_OK;
}
