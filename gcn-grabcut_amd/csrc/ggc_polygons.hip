// ggc_polygons.hip — H3: filled polygons and lassos as hard constraints on the GrabCut mask (additive; the sibling of
// ggc_strokes.hip).
//
// A polygon is n >= 3 integer vertices (row, col), closed from the last to the first.  Pixel p = (r, c) is COVERED iff it
// lies on an edge or its crossing number is odd (include/ggc.h H3): for edge a -> b with d = b - a and
//   cr = d.r (c - a.c) - d.c (r - a.r),
// p is ON the edge iff cr == 0 inside the edge's box, and the edge is CROSSED to the right of p iff (a.r <= r) != (b.r <= r)
// and (a.r < b.r ? cr < 0 : cr > 0): H3's test with lo / hi the ends ordered by row is -cr for a.r < b.r and +cr otherwise.
// |coordinate| <= 2^20 keeps each product below 2^44, so cr is one signed 64-bit value (two v_mad_i64_i32).
//
//   k_polygon_boxes   one wave per polygon: its bounding box (rmin, rmax, cmin, cmax) into context scratch.
//   k_paint_polygons  one workgroup per 32x8 pixel tile of one image, as k_paint_strokes.  The image's edges (one per vertex:
//                     the vertex and its successor inside its polygon, the polygon found by bisection in poly_ptr) are
//                     culled 256 at a time into an LDS list that keeps their order (per-wave ballot + prefix over the four
//                     waves), each with its polygon's index and label.  An edge stays when its polygon's box meets the
//                     tile, its row span meets the tile's rows and it is not wholly left of the tile: every dropped edge
//                     is neither on nor crossed to the right of any pixel of the tile, and a polygon whose box misses the
//                     tile covers none of it, so culling cannot change a result.  Edges right of the tile stay: they
//                     flip the parity of whole rows.  Each lane walks the list for its pixel with one parity bit and one
//                     on-edge bit, and closes a polygon when the index changes (the state lives across the 256-edge
//                     passes, so a polygon may span them): a lasso sets "inside a lasso", a fill sets the new label, the
//                     later fill overwriting the earlier.  After the last edge: the fill's label if a fill covered the
//                     pixel, else GGC_BGD if the image has a lasso and none covers the pixel, else nothing is written.
//                     Work is O(pixels + tiles x edges); no atomics.
#include "ggc_internal.h"
#include <climits>

namespace ggc {
namespace {

constexpr int PG_W = 32, PG_H = 8, PG_THREADS = PG_W * PG_H;   // 4 waves, each two 32-pixel rows of the tile
constexpr int PG_MAX_COORD = 1 << 20;
constexpr int PG_LASSO = 2;

__global__ void __launch_bounds__(256) k_polygon_boxes(int P, const int32_t* __restrict__ verts, const int32_t* __restrict__ poly_ptr,
                                                       int32_t* __restrict__ boxes) {
    const int q = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= P) return;                                                    // wave-uniform
    int rmin = INT_MAX, rmax = INT_MIN, cmin = INT_MAX, cmax = INT_MIN;
    for (int k = poly_ptr[q] + lane, k1 = poly_ptr[q + 1]; k < k1; k += WAVE) {
        const int r = verts[2 * (size_t)k], c = verts[2 * (size_t)k + 1];
        rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, o, WAVE)); rmax = max(rmax, __shfl_xor(rmax, o, WAVE));
        cmin = min(cmin, __shfl_xor(cmin, o, WAVE)); cmax = max(cmax, __shfl_xor(cmax, o, WAVE));
    }
    if (lane == 0) { boxes[4 * q] = rmin; boxes[4 * q + 1] = rmax; boxes[4 * q + 2] = cmin; boxes[4 * q + 3] = cmax; }
}

__global__ void __launch_bounds__(PG_THREADS) k_paint_polygons(int H, int W, int tiles_x, const int32_t* __restrict__ verts,
                                                               const int32_t* __restrict__ poly_ptr, const int32_t* __restrict__ poly_label,
                                                               const int32_t* __restrict__ image_ptr, const int32_t* __restrict__ boxes,
                                                               uint8_t* __restrict__ mask) {
    __shared__ int s_ar[PG_THREADS], s_ac[PG_THREADS], s_dr[PG_THREADS], s_dc[PG_THREADS], s_pk[PG_THREADS];
    __shared__ int s_wave[PG_THREADS / WAVE], s_lasso[PG_THREADS / WAVE];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = image_ptr[b], p1 = image_ptr[b + 1];
    if (p0 == p1) return;                                                  // block-uniform: an image without polygons
    const int tx0 = (blockIdx.x % tiles_x) * PG_W, ty0 = (blockIdx.x / tiles_x) * PG_H;
    const int tx1 = tx0 + PG_W - 1, ty1 = ty0 + PG_H - 1;
    const int x = tx0 + (tid & (PG_W - 1)), y = ty0 + tid / PG_W;
    const bool inside = x < W && y < H;
    int v = -1, cur = -1;                                                  // new label, -1 = no fill; the open polygon's key
    bool par = false, on = false, in_lasso = false, has_lasso = false;
    auto close = [&]() {
        if (cur >= 0 && (par || on)) {
            const int l = cur & 3;
            if (l == PG_LASSO) in_lasso = true;
            else v = l != 0 ? GGC_FGD : GGC_BGD;
        }
    };
    const int k0 = poly_ptr[p0], k1 = poly_ptr[p1];
    for (int base = k0; base < k1; base += PG_THREADS) {                   // block-uniform loop
        const int k = base + tid;
        int ar = 0, ac = 0, dr = 0, dc = 0, pk = 0;
        bool keep = false, lasso = false;
        if (k < k1) {
            int lo = p0, hi = p1;                                          // the polygon q with poly_ptr[q] <= k < poly_ptr[q+1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (poly_ptr[mid] <= k) lo = mid; else hi = mid;
            }
            const int q = lo, l = poly_label[q];
            lasso = l == PG_LASSO;
            const int32_t* bx = boxes + 4 * (size_t)q;
            if (bx[0] <= ty1 && bx[1] >= ty0 && bx[2] <= tx1 && bx[3] >= tx0) {
                const int kn = k + 1 == poly_ptr[q + 1] ? poly_ptr[q] : k + 1;
                ar = verts[2 * (size_t)k]; ac = verts[2 * (size_t)k + 1];
                const int br = verts[2 * (size_t)kn], bc = verts[2 * (size_t)kn + 1];
                dr = br - ar; dc = bc - ac;
                pk = ((q - p0) << 2) | l;
                keep = min(ar, br) <= ty1 && max(ar, br) >= ty0 && max(ac, bc) >= tx0;
            }
        }
        const unsigned long long m = __ballot(keep);
        const unsigned long long ml = __ballot(lasso);
        if (lane == 0) { s_wave[wave] = __popcll(m); s_lasso[wave] = ml != 0; }
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
        for (int w = 0; w < PG_THREADS / WAVE; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            n += s_wave[w];
            has_lasso |= s_lasso[w] != 0;
        }
        if (keep) { s_ar[pos] = ar; s_ac[pos] = ac; s_dr[pos] = dr; s_dc[pos] = dc; s_pk[pos] = pk; }
        __syncthreads();
        if (inside) {
            for (int i = 0; i < n; ++i) {                                  // same address in every lane: LDS broadcast
                const int key = s_pk[i];
                if (key != cur) { close(); cur = key; par = on = false; }  // uniform: every lane sees the same list
                const int er = s_ar[i], ec = s_ac[i], edr = s_dr[i], edc = s_dc[i];
                const int wr = y - er, wc = x - ec;
                const int64_t cr = (int64_t)edr * wc - (int64_t)edc * wr;
                // inside the edge's box: 0 <= w <= d or d <= w <= 0, per axis
                if (cr == 0 && (edr >= 0 ? (wr >= 0 && wr <= edr) : (wr <= 0 && wr >= edr)) &&
                    (edc >= 0 ? (wc >= 0 && wc <= edc) : (wc <= 0 && wc >= edc)))
                    on = true;
                if ((wr >= 0) != (wr >= edr) && (edr > 0 ? cr < 0 : cr > 0)) par = !par;   // (a.r <= r) != (b.r <= r)
            }
        }
        __syncthreads();                                                   // the list is rewritten by the next 256 edges
    }
    if (!inside) return;
    close();
    if (v < 0 && has_lasso && !in_lasso) v = GGC_BGD;
    if (v >= 0) mask[(size_t)b * H * W + (size_t)y * W + x] = (uint8_t)v;
}

} // namespace
} // namespace ggc

extern "C" int ggc_apply_polygons(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* verts,
                                  const int32_t* poly_ptr, const int32_t* poly_label, const int32_t* image_ptr, int P,
                                  uint8_t* mask) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (each at most 65535)", B, H, W);
    GGC_REQUIRE(ctx, P >= 0, GGC_E_INVALID_ARG, "negative polygon count %d", P);
    if (P == 0) return GGC_OK;
    GGC_REQUIRE(ctx, mask && image_ptr && poly_ptr && poly_label && verts, GGC_E_INVALID_ARG, "null pointer");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> ip, pp, pl, vv;
    int rc = read_i32(ctx, st, image_ptr, B + 1, ip);
    if (rc) return rc;
    GGC_REQUIRE(ctx, ip[0] == 0, GGC_E_INVALID_ARG, "image_ptr[0] = %d, expected 0", ip[0]);
    for (int b = 0; b < B; ++b)
        GGC_REQUIRE(ctx, ip[b + 1] >= ip[b], GGC_E_INVALID_ARG, "image_ptr decreases at image %d (%d -> %d)", b, ip[b], ip[b + 1]);
    GGC_REQUIRE(ctx, ip[B] == P, GGC_E_INVALID_ARG, "image_ptr ends at %d, expected P = %d", ip[B], P);
    rc = read_i32(ctx, st, poly_ptr, P + 1, pp);
    if (rc) return rc;
    GGC_REQUIRE(ctx, pp[0] == 0, GGC_E_INVALID_ARG, "poly_ptr[0] = %d, expected 0", pp[0]);
    for (int q = 0; q < P; ++q) {
        GGC_REQUIRE(ctx, pp[q + 1] >= pp[q], GGC_E_INVALID_ARG, "poly_ptr decreases at polygon %d (%d -> %d)", q, pp[q], pp[q + 1]);
        GGC_REQUIRE(ctx, pp[q + 1] - pp[q] >= 3, GGC_E_INVALID_ARG, "polygon %d has %d vertices, at least 3 are needed", q,
                    pp[q + 1] - pp[q]);
    }
    const int V = pp[P];
    GGC_REQUIRE(ctx, V <= INT_MAX / 2, GGC_E_INVALID_ARG, "%d vertices are too many", V);
    rc = read_i32(ctx, st, poly_label, P, pl);
    if (rc) return rc;
    for (int q = 0; q < P; ++q)
        GGC_REQUIRE(ctx, pl[q] >= 0 && pl[q] <= 2, GGC_E_INVALID_ARG, "polygon %d has label %d, expected 0, 1 or 2", q, pl[q]);
    rc = read_i32(ctx, st, verts, 2 * V, vv);
    if (rc) return rc;
    for (int k = 0; k < 2 * V; ++k)
        GGC_REQUIRE(ctx, vv[k] >= -PG_MAX_COORD && vv[k] <= PG_MAX_COORD, GGC_E_INVALID_ARG,
                    "vertex %d has a coordinate %d beyond +-2^20", k / 2, vv[k]);
    int32_t* boxes = nullptr;
    if (!carve_scratch(ctx, S_POLYGONS, [&](Carve& c) { boxes = c.take<int32_t>(4 * (size_t)P); })) return GGC_E_OOM;
    const int tiles_x = cdiv(W, PG_W), tiles = tiles_x * cdiv(H, PG_H);
    hipLaunchKernelGGL(k_polygon_boxes, dim3(cdiv(P, 256 / WAVE)), dim3(256), 0, st, P, verts, poly_ptr, boxes);
    hipLaunchKernelGGL(k_paint_polygons, dim3(tiles, B), dim3(PG_THREADS), 0, st, H, W, tiles_x, verts, poly_ptr, poly_label,
                       image_ptr, boxes, mask);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
