// ggc_scissors.hip — H4: intelligent scissors (live-wire).  Consecutive anchors of a path are joined by the cheapest
// 8-connected path along image edges inside a bounded window (include/ggc.h has the exact integer definition).  Everything
// is int32; D is the fixed point with d(b) = 0 that ggc_relax.h computes by tile relaxation, whatever the order of the
// visits, and the walk over D is a pure function of D.
//
//   k_sc_guide   one workgroup per 32x32 window tile: the 36x36 pixels around the tile staged in LDS, the 3x3 box sums S
//                of the 34x34 positions the gradient reads, then G and the flatness F, one byte per window pixel.  The
//                same launch fills the segment's distance plane: 0 at b, 2^30 ("unreached") elsewhere.
//   k_sc_round   one round of ggc_relax.h with one plane (PLANES = 1, so all 256 lanes belong to it): F and D of tile + halo
//                staged in LDS, the four arc-cost tables built from F, the visit.  A pixel outside the window holds
//                RX_BLOCKED = 2^29 in LDS: min(2^29, D(q) + 2^29) leaves it alone, and 2^29 + 2^29 = 2^30 lowers no pixel of
//                the window; the largest sum formed is 2^30 + 2^29.
//   k_sc_walk    one wave per segment, from a towards b: lanes 0..7 load the eight candidates, a ballot picks the first
//                in the order N, NE, E, SE, S, SW, W, NW with D(q) + c(p,q) == D(p); D and F of the chosen neighbour
//                travel by shuffle, so a step is one dependent pair of loads.  Run twice: counting, then filling.
//   k_sc_scan    one workgroup: segment counts -> segment offsets and vert_ptr_out.
// The first work list, the segment table and the tile -> segment table are built on the host from the anchors, which it
// has read back for the checks anyway.
#include "ggc_relax.h"
#include <climits>

namespace ggc {
namespace {

constexpr int SC_UNREACHED = 1 << 30;
constexpr int SC_MAX_MARGIN = 256, SC_MAX_EDGE_CAP = 13770, SC_MAX_SMOOTH = 64, SC_MAX_SPAN = 1024;
constexpr int64_t SC_MAX_AREA = (int64_t)1 << 26;      // window pixels of one call: 256 MiB of distance planes
constexpr int64_t SC_MAX_TILES = (int64_t)1 << 21;
constexpr int SC_PX = RX_T + 4;                        // staged pixels per tile side: the tile, the gradient's and the box's reach

struct ScSeg {                                         // one segment a -> b; 16 words
    int b, ar, ac, br, bc;                             // image, anchors (image coordinates)
    int y0, x0, wh, ww;                                // window
    int tiles_x, tiles_y, tile_base, plane_off;        // its tiles in the call's tile numbering, its plane in the planes
    int path, flags, pad;                              // flags: 1 = last segment of an open path (b is appended)
};
static_assert(sizeof(ScSeg) == 64, "uploaded as 16 words");

struct ScWork {
    const ScSeg* seg;
    const int32_t* tile_seg;     // tile -> segment
    int32_t* plane;              // the segments' distance planes, one after the other, each its window row-major
    uint8_t* F;                  // flatness, same layout
    RelaxLists q;                // no `touched`; list[0] starts as the host's first list
    int32_t* lost;               // set when a walk found no successor
};

__global__ void __launch_bounds__(RX_THREADS) k_sc_guide(int H, int W, int edge_cap, int n_tiles, const uint8_t* __restrict__ bgr,
                                                         ScWork w) {
    __shared__ uint8_t s_px[SC_PX * SC_PX * 3];
    __shared__ uint16_t s_S[3][RX_H * RX_H];
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {       // block-uniform
        const ScSeg g = w.seg[w.tile_seg[tile]];
        const int tr = tile - g.tile_base, tyi = tr / g.tiles_x, txi = tr - tyi * g.tiles_x;
        const int ty0 = g.y0 + tyi * RX_T, tx0 = g.x0 + txi * RX_T;
        const uint8_t* img = bgr + (size_t)g.b * H * W * 3;
        for (int i = tid; i < SC_PX * SC_PX; i += RX_THREADS) {           // pixel (ty0 - 2 + hy, tx0 - 2 + hx), clamped
            const int hy = i / SC_PX, hx = i - hy * SC_PX;
            const uint8_t* px = img + 3 * ((size_t)min(max(ty0 - 2 + hy, 0), H - 1) * W + min(max(tx0 - 2 + hx, 0), W - 1));
            s_px[3 * i] = px[0]; s_px[3 * i + 1] = px[1]; s_px[3 * i + 2] = px[2];
        }
        __syncthreads();
        // S at (ty0 - 1 + sy, tx0 - 1 + sx).  Right for positions inside the image, where clamping the nine pixels is the
        // definition; the gradient clamps its own coordinates first, so it reads no other position.
        for (int i = tid; i < RX_H * RX_H; i += RX_THREADS) {
            const int sy = i / RX_H, sx = i - sy * RX_H;
            int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int k = 3 * ((sy + dy) * SC_PX + sx + dx);
                    s0 += s_px[k]; s1 += s_px[k + 1]; s2 += s_px[k + 2];
                }
            s_S[0][i] = (uint16_t)s0; s_S[1][i] = (uint16_t)s1; s_S[2][i] = (uint16_t)s2;
        }
        __syncthreads();
        const int lx = tid & 31, x = tx0 + lx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ly = (tid >> 5) + 8 * k, y = ty0 + ly;
            if (y >= g.y0 + g.wh || x >= g.x0 + g.ww) continue;           // the window lies inside the image
            const int iy = ly + 1, ix = lx + 1;
            const int iyp = min(y + 1, H - 1) - ty0 + 1, iym = max(y - 1, 0) - ty0 + 1;
            const int ixp = min(x + 1, W - 1) - tx0 + 1, ixm = max(x - 1, 0) - tx0 + 1;
            int G = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                G += abs((int)s_S[c][iy * RX_H + ixp] - (int)s_S[c][iy * RX_H + ixm]) +
                     abs((int)s_S[c][iyp * RX_H + ix] - (int)s_S[c][iym * RX_H + ix]);
            const size_t q = (size_t)g.plane_off + (size_t)(y - g.y0) * g.ww + (x - g.x0);
            w.F[q] = (uint8_t)(((edge_cap - min(G, edge_cap)) * 255) / edge_cap);
            w.plane[q] = (y == g.br && x == g.bc) ? 0 : SC_UNREACHED;
        }
        __syncthreads();                                                   // LDS is reused by the block's next tile
    }
}

__global__ void __launch_bounds__(RX_THREADS) k_sc_round(int smooth, int round, ScWork w) {
    __shared__ struct { RelaxLds<1> rx; uint8_t F[RX_N]; } lds;        // the guide beside the relaxation's arrays
    auto& s_F = lds.F;
    RelaxLds<1>& L = lds.rx;
    const int tid = threadIdx.x;
    const RelaxRound rr = relax_round_begin(w.q, round);
    for (int li = blockIdx.x; li < rr.n; li += gridDim.x) {                // block-uniform
        const int tile = rr.cur[li];
        const ScSeg g = w.seg[w.tile_seg[tile]];
        const int tr = tile - g.tile_base, tyi = tr / g.tiles_x, txi = tr - tyi * g.tiles_x;
        const int wy0 = tyi * RX_T, wx0 = txi * RX_T;                      // window-relative
        int32_t* plane = w.plane + g.plane_off;
        const uint8_t* F = w.F + g.plane_off;
        const RelaxBox box = relax_box(wy0, wx0, g.wh, g.ww);
        for (int i = tid; i < RX_H * RX_H; i += RX_THREADS) {
            const int hy = i / RX_H, hx = i - hy * RX_H, y = wy0 + hy - 1, x = wx0 + hx - 1;
            const bool in = box.has(hy, hx);
            const int j = hy * RX_S + hx;
            L.d[0][j] = in ? plane[(size_t)y * g.ww + x] : RX_BLOCKED;
            s_F[j] = in ? F[(size_t)y * g.ww + x] : (uint8_t)0;
        }
        __syncthreads();
        relax_arcs(L, box, [&](int j, int q, int len) { return len * (smooth + (int)s_F[j] + (int)s_F[q]); });
        __syncthreads();
        const int nbm = relax_visit(L, [&](int, int ly, int lx, int v) {
            if (wy0 + ly < g.wh && wx0 + lx < g.ww) plane[(size_t)(wy0 + ly) * g.ww + wx0 + lx] = v;
        });
        relax_list_neighbours(w.q, rr, nbm, tyi, txi, g.tiles_y, g.tiles_x, g.tile_base);
    }
}

// One wave per segment.  Counting (FILL false): seg_cnt[s] = pixels from a inclusive to b exclusive.  Filling: the same walk,
// at most seg_cnt[s] steps, written from seg_off[s] on; the last segment of an open path appends b.
template <bool FILL>
__global__ void __launch_bounds__(256) k_sc_walk(int n_seg, int smooth, ScWork w, int32_t* __restrict__ seg_cnt,
                                                 const int32_t* __restrict__ seg_off, int32_t* __restrict__ verts_out) {
    const int s = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_seg) return;                                                // wave-uniform
    const ScSeg g = w.seg[s];
    const int32_t* D = w.plane + g.plane_off;
    const uint8_t* F = w.F + g.plane_off;
    // N, NE, E, SE, S, SW, W, NW
    const int dy = (lane == 0 || lane == 1 || lane == 7) ? -1 : ((lane >= 3 && lane <= 5) ? 1 : 0);
    const int dx = (lane >= 1 && lane <= 3) ? 1 : ((lane >= 5 && lane <= 7) ? -1 : 0);
    const int len = (lane & 1) ? RX_DIAG : RX_AXIAL;
    int r = g.ar - g.y0, c = g.ac - g.x0;                                  // window-relative
    const int tr = g.br - g.y0, tc = g.bc - g.x0;
    int Dp = D[(size_t)r * g.ww + c], Fp = F[(size_t)r * g.ww + c];
    const int limit = FILL ? seg_cnt[s] : g.wh * g.ww;                     // D falls at every step: a walk repeats no pixel
    int32_t* out = FILL ? verts_out + 2 * (size_t)seg_off[s] : nullptr;
    int n = 0;
    bool lost = false;
    while ((r != tr || c != tc) && n < limit) {
        if (FILL && lane == 0) { out[2 * (size_t)n] = r + g.y0; out[2 * (size_t)n + 1] = c + g.x0; }
        ++n;
        const int qr = r + dy, qc = c + dx;
        const bool ok = lane < 8 && qr >= 0 && qr < g.wh && qc >= 0 && qc < g.ww;
        int Dq = 0, Fq = 0;
        if (ok) { Dq = D[(size_t)qr * g.ww + qc]; Fq = F[(size_t)qr * g.ww + qc]; }
        const unsigned long long m = __ballot(ok && Dq + len * (smooth + Fp + Fq) == Dp);
        if (m == 0) { lost = true; break; }                                // cannot happen on a converged plane
        const int k = __ffsll(m) - 1;
        r += __shfl(dy, k, WAVE); c += __shfl(dx, k, WAVE);
        Dp = __shfl(Dq, k, WAVE); Fp = __shfl(Fq, k, WAVE);
    }
    if (!FILL) {
        if (lost || r != tr || c != tc) { n = 0; if (lane == 0) atomicOr(w.lost, 1); }
        if (lane == 0) seg_cnt[s] = n;
    } else if ((g.flags & 1) && lane == 0) {
        out[2 * (size_t)n] = g.br; out[2 * (size_t)n + 1] = g.bc;
    }
}

// one workgroup: segment counts (+1 where an open path ends) -> their exclusive offsets, and vert_ptr_out [Q+1].  Every
// path has at least one segment, and a path's segments are consecutive.
__global__ void __launch_bounds__(256) k_sc_scan(int n_seg, int Q, const ScSeg* __restrict__ seg, const int32_t* __restrict__ seg_cnt,
                                                 int32_t* __restrict__ seg_off, int32_t* __restrict__ vert_ptr_out,
                                                 int32_t* __restrict__ total_out) {
    __shared__ int part[256];
    const int tid = threadIdx.x, chunk = (n_seg + 255) / 256, s0 = min(n_seg, tid * chunk), s1 = min(n_seg, s0 + chunk);
    int sum = 0;
    for (int s = s0; s < s1; ++s) sum += seg_cnt[s] + (seg[s].flags & 1);
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        vert_ptr_out[Q] = run;
        *total_out = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int s = s0; s < s1; ++s) {
        seg_off[s] = run;
        if (s == 0 || seg[s - 1].path != seg[s].path) vert_ptr_out[seg[s].path] = run;
        run += seg_cnt[s] + (seg[s].flags & 1);
    }
}

} // namespace
} // namespace ggc

extern "C" int ggc_trace_paths(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr, const int32_t* anchors,
                               const int32_t* path_ptr, const int32_t* path_closed, const int32_t* image_ptr, int Q, int margin,
                               int edge_cap, int smooth, int32_t* vert_ptr_out, int32_t* verts_out, int64_t capacity) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0 || Q == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (each at most 65535)", B, H, W);
    GGC_REQUIRE(ctx, Q > 0, GGC_E_INVALID_ARG, "negative path count %d", Q);
    GGC_REQUIRE(ctx, margin >= 0 && margin <= SC_MAX_MARGIN, GGC_E_INVALID_ARG, "scissors margin %d outside 0..%d", margin, SC_MAX_MARGIN);
    GGC_REQUIRE(ctx, edge_cap >= 1 && edge_cap <= SC_MAX_EDGE_CAP, GGC_E_INVALID_ARG, "scissors edge_cap %d outside 1..%d", edge_cap,
                SC_MAX_EDGE_CAP);
    GGC_REQUIRE(ctx, smooth >= 1 && smooth <= SC_MAX_SMOOTH, GGC_E_INVALID_ARG, "scissors smooth %d outside 1..%d", smooth, SC_MAX_SMOOTH);
    GGC_REQUIRE(ctx, bgr && anchors && path_ptr && path_closed && image_ptr && vert_ptr_out, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, !verts_out || capacity >= 0, GGC_E_INVALID_ARG, "negative capacity %lld", (long long)capacity);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    std::vector<int32_t> ip, pp, closed, an;
    int rc = read_offsets(ctx, st, image_ptr, B, "image_ptr", "image", 0, ip);
    if (rc) return rc;
    GGC_REQUIRE(ctx, ip[B] == Q, GGC_E_INVALID_ARG, "image_ptr[B] = %d, expected Q = %d", ip[B], Q);
    if ((rc = read_offsets(ctx, st, path_ptr, Q, "path_ptr", "path", 2, pp))) return rc;
    if ((rc = read_i32(ctx, st, path_closed, Q, closed))) return rc;
    const int A = pp[Q];
    GGC_REQUIRE(ctx, A <= INT_MAX / 2, GGC_E_INVALID_ARG, "%d anchors are too many", A);
    if ((rc = read_i32(ctx, st, anchors, 2 * A, an))) return rc;

    // the segments, their windows and tiles, and the first work list
    std::vector<ScSeg> segs;
    std::vector<int32_t> first;
    int64_t area = 0, n_tiles64 = 0;
    int max_window_tiles = 0;
    for (int b = 0; b < B; ++b)
        for (int q = ip[b]; q < ip[b + 1]; ++q) {
            const int a0 = pp[q], n = pp[q + 1] - a0;
            GGC_REQUIRE(ctx, closed[q] == 0 || closed[q] == 1, GGC_E_INVALID_ARG, "path_closed[%d] = %d, expected 0 or 1", q, closed[q]);
            GGC_REQUIRE(ctx, !closed[q] || n >= 3, GGC_E_INVALID_ARG, "closed path %d has %d anchors: it needs at least 3", q, n);
            for (int i = 0; i < n; ++i) {
                const int r = an[2 * (size_t)(a0 + i)], c = an[2 * (size_t)(a0 + i) + 1];
                GGC_REQUIRE(ctx, r >= 0 && r < H && c >= 0 && c < W, GGC_E_INVALID_ARG, "anchor %d of path %d, (%d, %d), lies outside its %dx%d image",
                            i, q, r, c, H, W);
            }
            const int n_seg = closed[q] ? n : n - 1;
            for (int i = 0; i < n_seg; ++i) {
                const int j = i + 1 < n ? i + 1 : 0;
                ScSeg g{};
                g.b = b; g.path = q;
                g.ar = an[2 * (size_t)(a0 + i)]; g.ac = an[2 * (size_t)(a0 + i) + 1];
                g.br = an[2 * (size_t)(a0 + j)]; g.bc = an[2 * (size_t)(a0 + j) + 1];
                GGC_REQUIRE(ctx, std::abs(g.ar - g.br) <= SC_MAX_SPAN && std::abs(g.ac - g.bc) <= SC_MAX_SPAN, GGC_E_INVALID_ARG,
                            "anchors %d and %d of path %d are more than %d pixels apart", i, j, q, SC_MAX_SPAN);
                g.y0 = std::max(std::min(g.ar, g.br) - margin, 0);
                g.x0 = std::max(std::min(g.ac, g.bc) - margin, 0);
                g.wh = std::min(std::max(g.ar, g.br) + margin, H - 1) - g.y0 + 1;
                g.ww = std::min(std::max(g.ac, g.bc) + margin, W - 1) - g.x0 + 1;
                g.tiles_x = cdiv(g.ww, RX_T); g.tiles_y = cdiv(g.wh, RX_T);
                g.flags = (!closed[q] && i == n_seg - 1) ? 1 : 0;
                area += (int64_t)g.wh * g.ww;
                n_tiles64 += (int64_t)g.tiles_x * g.tiles_y;
                GGC_REQUIRE(ctx, area <= SC_MAX_AREA && n_tiles64 <= SC_MAX_TILES, GGC_E_INVALID_ARG,
                            "the windows hold more than 2^26 pixels or 2^21 tiles (at path %d): fewer paths or a smaller margin per call", q);
                g.plane_off = (int)(area - (int64_t)g.wh * g.ww);
                g.tile_base = (int)(n_tiles64 - (int64_t)g.tiles_x * g.tiles_y);
                max_window_tiles = std::max(max_window_tiles, g.tiles_x * g.tiles_y);
                // b's tile and every tile that holds b in its halo: a visit reports only the pixels it lowers itself
                const int tr = g.br - g.y0, tc = g.bc - g.x0;
                relax_tiles_holding(tr / RX_T, tc / RX_T, tr % RX_T, tc % RX_T, g.tiles_y, g.tiles_x,
                                    [&](int ny, int nx) { first.push_back(g.tile_base + ny * g.tiles_x + nx); });
                segs.push_back(g);
            }
        }
    const int n_seg = (int)segs.size(), n_tiles = (int)n_tiles64, n_first = (int)first.size();

    // uploaded in one copy: the four counters, the segments, tile -> segment, and the head of the first work list
    std::vector<int32_t> up(4 + 16 * (size_t)n_seg + (size_t)n_tiles + (size_t)n_first);
    up[0] = n_first; up[1] = up[2] = up[3] = 0;
    std::memcpy(up.data() + 4, segs.data(), sizeof(ScSeg) * (size_t)n_seg);
    {
        int32_t* ts = up.data() + 4 + 16 * (size_t)n_seg;
        for (int s = 0; s < n_seg; ++s) std::fill(ts + segs[s].tile_base, ts + segs[s].tile_base + segs[s].tiles_x * segs[s].tiles_y, s);
        std::copy(first.begin(), first.end(), ts + n_tiles);
    }
    ScWork w{};
    int32_t *dev_up = nullptr, *seg_cnt = nullptr, *seg_off = nullptr, *total = nullptr;
    if (!carve_scratch(ctx, S_SCISSORS, [&](Carve& c) {
            w.plane = c.take<int32_t>((size_t)area);                       // first: ggc_debug_read_scratch("scissors_planes")
            w.F = c.take<uint8_t>((size_t)area);
            dev_up = c.take<int32_t>(4 + 16 * (size_t)n_seg + 2 * (size_t)n_tiles);
            w.q.list[1] = c.take<int32_t>((size_t)n_tiles);
            w.q.stamp = c.take<int32_t>((size_t)n_tiles);
            seg_cnt = c.take<int32_t>((size_t)n_seg);
            seg_off = c.take<int32_t>((size_t)n_seg);
            total = c.take<int32_t>(2);
        }))
        return GGC_E_OOM;
    w.q.cnt = dev_up;
    w.lost = dev_up + 3;
    w.seg = reinterpret_cast<const ScSeg*>(dev_up + 4);
    w.tile_seg = dev_up + 4 + 16 * (size_t)n_seg;
    w.q.list[0] = dev_up + 4 + 16 * (size_t)n_seg + (size_t)n_tiles;
    GGC_HIP(ctx, hipMemcpyAsync(dev_up, up.data(), sizeof(int32_t) * up.size(), hipMemcpyHostToDevice, st));
    GGC_HIP(ctx, hipMemsetAsync(w.q.stamp, 0, sizeof(int32_t) * (size_t)n_tiles, st));
    GGC_HIP(ctx, hipStreamSynchronize(st));                                // `up` is pageable: the copy has left it

    const int wide = 16 * std::max(ctx->n_cu, 1), grid = std::min(n_tiles, wide);
    {
        ProfScope prof(ctx, st, "scissors_guide");
        hipLaunchKernelGGL(k_sc_guide, dim3(grid), dim3(RX_THREADS), 0, st, H, W, edge_cap, n_tiles, bgr, w);
    }
    GGC_LAUNCH_CHECK(ctx);
    // Round bound (ggc_relax.h).  A cheapest path is simple and stays in its window, so it has fewer arcs than the window has
    // pixels: it crosses at most J = 1024 * tiles - 1 tile edges.
    const int64_t max_rounds = (int64_t)RX_T * RX_T * max_window_tiles + 2;
    const auto launch_round = [&](int64_t round) {
        ProfScope prof(ctx, st, "scissors_round");
        hipLaunchKernelGGL(k_sc_round, dim3(grid), dim3(RX_THREADS), 0, st, smooth, (int)round, w);
    };
    // a window is a few tiles across: look after 6 rounds, then every 4
    if ((rc = relax_rounds(ctx, st, launch_round, w.q.cnt, 6, 4, max_rounds, "scissors"))) return rc;
    std::vector<int32_t> host;
    const int walk_blocks = cdiv(n_seg, 256 / WAVE);
    {
        ProfScope prof(ctx, st, "scissors_walk");
        hipLaunchKernelGGL(k_sc_walk<false>, dim3(walk_blocks), dim3(256), 0, st, n_seg, smooth, w, seg_cnt, seg_off, verts_out);
    }
    hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(256), 0, st, n_seg, Q, w.seg, seg_cnt, seg_off, vert_ptr_out, total);
    GGC_LAUNCH_CHECK(ctx);
    if ((rc = read_i32(ctx, st, w.lost, 1, host))) return rc;
    GGC_REQUIRE(ctx, host[0] == 0, GGC_E_DEVICE, "a scissors walk found no successor on its distance plane");
    if (!verts_out) return GGC_OK;
    if ((rc = read_i32(ctx, st, total, 1, host))) return rc;
    GGC_REQUIRE(ctx, capacity >= host[0], GGC_E_INVALID_ARG, "capacity %lld is below the %d traced vertices", (long long)capacity, host[0]);
    if (host[0] == 0) return GGC_OK;
    {
        ProfScope prof(ctx, st, "scissors_walk");
        hipLaunchKernelGGL(k_sc_walk<true>, dim3(walk_blocks), dim3(256), 0, st, n_seg, smooth, w, seg_cnt, seg_off, verts_out);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
