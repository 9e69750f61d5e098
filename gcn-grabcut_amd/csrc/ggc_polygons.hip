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
//   k_paint_polygons  the tile painter (ggc_paint.h) over the image's edges, one per vertex: the vertex and its successor
//                     inside its polygon, the polygon found by bisection in poly_ptr; a record carries its polygon's
//                     index and label.  An edge is kept when its polygon's box meets the tile, its row span meets the
//                     tile's rows and it is not wholly left of the tile: every dropped edge is neither on nor crossed to
//                     the right of any pixel of the tile, and a polygon whose box misses the tile covers none of it, so
//                     culling cannot change a result.  Edges right of the tile stay: they flip the parity of whole rows.
//                     Each lane walks the list for its pixel with one parity bit and one on-edge bit, and closes a
//                     polygon when the index changes (the state lives across the 256-edge passes, so a polygon may span
//                     them): a lasso sets "inside a lasso", a fill sets the new label, the later fill overwriting the
//                     earlier.  After the last edge: the fill's label if a fill covered the pixel, else GGC_BGD if the
//                     image has a lasso and none covers the pixel, else nothing is written.
//                     Work is O(pixels + tiles x edges); no atomics.
#include "ggc_paint.h"
#include <climits>

namespace ggc {
namespace {

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

__global__ void __launch_bounds__(PT_THREADS) k_paint_polygons(int H, int W, int tiles_x, const int32_t* __restrict__ verts,
                                                               const int32_t* __restrict__ poly_ptr, const int32_t* __restrict__ poly_label,
                                                               const int32_t* __restrict__ image_ptr, const int32_t* __restrict__ boxes,
                                                               uint8_t* __restrict__ mask) {
    __shared__ int s_ar[PT_THREADS], s_ac[PT_THREADS], s_dr[PT_THREADS], s_dc[PT_THREADS], s_pk[PT_THREADS];
    __shared__ int s_wave[PT_THREADS / WAVE];
    const PaintTile t = paint_tile(H, W, tiles_x);
    const int p0 = image_ptr[t.b], p1 = image_ptr[t.b + 1];
    if (p0 == p1) return;                                                  // block-uniform: an image without polygons
    const int tx0 = t.tx0, ty0 = t.ty0, tx1 = tx0 + PT_W - 1, ty1 = ty0 + PT_H - 1;   // the whole tile, not clipped
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
    for (int base = k0; base < k1; base += PT_THREADS) {                   // block-uniform loop
        const int k = base + threadIdx.x;
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
        const PaintSlot slot = paint_slot<true>(keep, lasso, s_wave);
        has_lasso |= slot.extra;
        if (keep) { s_ar[slot.pos] = ar; s_ac[slot.pos] = ac; s_dr[slot.pos] = dr; s_dc[slot.pos] = dc; s_pk[slot.pos] = pk; }
        __syncthreads();
        if (t.inside) {
            for (int i = 0; i < slot.n; ++i) {                                  // same address in every lane: LDS broadcast
                const int key = s_pk[i];
                if (key != cur) { close(); cur = key; par = on = false; }  // uniform: every lane sees the same list
                const int er = s_ar[i], ec = s_ac[i], edr = s_dr[i], edc = s_dc[i];
                const int wr = t.y - er, wc = t.x - ec;
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
    if (!t.inside) return;
    close();
    if (v < 0 && has_lasso && !in_lasso) v = GGC_BGD;
    if (v >= 0) mask[t.p] = (uint8_t)v;
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
    int rc = read_offsets(ctx, st, image_ptr, B, "image_ptr", "image", 0, ip);
    if (rc) return rc;
    GGC_REQUIRE(ctx, ip[B] == P, GGC_E_INVALID_ARG, "image_ptr ends at %d, expected P = %d", ip[B], P);
    rc = read_offsets(ctx, st, poly_ptr, P, "poly_ptr", "polygon", 3, pp);                // a polygon has at least 3 vertices
    if (rc) return rc;
    const int V = pp[P];
    GGC_REQUIRE(ctx, V <= INT_MAX / 2, GGC_E_INVALID_ARG, "%d vertices are too many", V);
    rc = read_i32(ctx, st, poly_label, P, pl);
    if (rc) return rc;
    for (int q = 0; q < P; ++q)
        GGC_REQUIRE(ctx, pl[q] >= 0 && pl[q] <= 2, GGC_E_INVALID_ARG, "polygon %d has label %d outside 0..2", q, pl[q]);
    rc = read_i32(ctx, st, verts, 2 * V, vv);
    if (rc) return rc;
    for (int k = 0; k < 2 * V; ++k)
        GGC_REQUIRE(ctx, vv[k] >= -PG_MAX_COORD && vv[k] <= PG_MAX_COORD, GGC_E_INVALID_ARG,
                    "vertex %d has a coordinate %d beyond +-2^20", k / 2, vv[k]);
    int32_t* boxes = nullptr;
    if (!carve_scratch(ctx, S_POLYGONS, [&](Carve& c) { boxes = c.take<int32_t>(4 * (size_t)P); })) return GGC_E_OOM;
    const int tiles_x = cdiv(W, PT_W), tiles = tiles_x * cdiv(H, PT_H);
    hipLaunchKernelGGL(k_polygon_boxes, dim3(cdiv(P, 256 / WAVE)), dim3(256), 0, st, P, verts, poly_ptr, boxes);
    hipLaunchKernelGGL(k_paint_polygons, dim3(tiles, B), dim3(PT_THREADS), 0, st, H, W, tiles_x, verts, poly_ptr, poly_label,
                       image_ptr, boxes, mask);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
