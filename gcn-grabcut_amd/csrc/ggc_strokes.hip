// ggc_strokes.hip — H2: brush strokes as hard constraints on the GrabCut mask (additive; the sibling of ggc_hints.hip).
//
// A stroke travels as straight segments (r0, c0, r1, c1, label).  One exact integer rule decides whether pixel p is within
// rho of segment a->b (include/ggc.h H2): with w = p - a, d = b - a, L2 = d.d, t = w.d,
//   t <= 0:   4 |w|^2     <= rho4          t >= L2:  4 |p - b|^2 <= rho4          else:  4 (w x d)^2 <= rho4 L2,
// rho4 = max(4 radius^2, 1).  |coordinate| <= 2^20 keeps t and w x d inside int64; (w x d)^2 and rho4 L2 need up to 90 bits
// and are compared as unsigned __int128 (v_mad_u64_u32 chains, no scratch).
//
//   k_paint_strokes   the tile painter (ggc_paint.h).  A segment is kept when the tile's centre is within radius + the
//                     tile's half-diagonal of it, the same rule in doubled coordinates so that the centre is an integer.
//                     That is conservative and never by bounding box, so a long diagonal stroke is walked only by the
//                     tiles along it.  Work is O(pixels + tiles x segments), independent of stroke length.
//                     PAINT writes the label into the mask (a pixel no stroke touches is neither read nor written);
//                     STAMP writes 0 | 1 + label for every pixel into context scratch.
//   ggc_stroke_pixels stamps the centre lines (radius 0), then: k_stroke_row_count (one wave per row), k_stroke_image_scan
//                     (one workgroup per image: row offsets and the image's count), k_stroke_ptr_scan (one workgroup:
//                     hint_ptr_out), k_stroke_fill (one wave per row, raster order by ballot + prefix).  Integer sums
//                     only and no atomics: the list does not depend on launch order.
#include "ggc_paint.h"
#include <climits>

namespace ggc {
namespace {

constexpr int ST_MAX_COORD = 1 << 20, ST_MAX_RADIUS = 16384;

struct SDims { int B, H, W; unsigned long long rho4, cull; };   // cull = (max(2 radius, 1) + 32)^2, doubled coordinates

// M dist^2((wy, wx), segment 0 -> (dy, dx)) <= thr, exactly.  |w|, |d| < 2^23.
template <int M>
__device__ __forceinline__ bool seg_within(int64_t wy, int64_t wx, int64_t dy, int64_t dx, unsigned long long thr) {
    const int64_t L2 = dy * dy + dx * dx, t = wy * dy + wx * dx;
    if (t <= 0) return (unsigned long long)(M * (wy * wy + wx * wx)) <= thr;
    if (t >= L2) {
        const int64_t ey = wy - dy, ex = wx - dx;
        return (unsigned long long)(M * (ey * ey + ex * ex)) <= thr;
    }
    const int64_t cr = wy * dx - wx * dy;
    const unsigned long long a = (unsigned long long)(cr < 0 ? -cr : cr);
    return (unsigned __int128)a * a * (unsigned)M <= (unsigned __int128)thr * (unsigned long long)L2;
}

template <bool STAMP>
__global__ void __launch_bounds__(PT_THREADS) k_paint_strokes(SDims d, int tiles_x, const int32_t* __restrict__ strokes,
                                                              const int32_t* __restrict__ stroke_ptr, uint8_t* __restrict__ out) {
    __shared__ int s_r0[PT_THREADS], s_c0[PT_THREADS], s_dr[PT_THREADS], s_dc[PT_THREADS], s_l[PT_THREADS];
    __shared__ int s_wave[PT_THREADS / WAVE];
    const PaintTile t = paint_tile(d.H, d.W, tiles_x);
    const int64_t cy2 = 2 * t.ty0 + (PT_H - 1), cx2 = 2 * t.tx0 + (PT_W - 1);   // the tile's centre, doubled
    int v = -1;                                                            // new label, -1 = untouched
    const int k0 = stroke_ptr[t.b], k1 = stroke_ptr[t.b + 1];
    for (int base = k0; base < k1; base += PT_THREADS) {                  // block-uniform loop
        const int k = base + threadIdx.x;
        int r0 = 0, c0 = 0, dr = 0, dc = 0, l = 0;
        bool keep = false;
        if (k < k1) {
            r0 = strokes[5 * k]; c0 = strokes[5 * k + 1];
            dr = strokes[5 * k + 2] - r0; dc = strokes[5 * k + 3] - c0;
            l = strokes[5 * k + 4] != 0 ? GGC_FGD : GGC_BGD;
            keep = seg_within<1>(cy2 - 2 * (int64_t)r0, cx2 - 2 * (int64_t)c0, 2 * (int64_t)dr, 2 * (int64_t)dc, d.cull);
        }
        const PaintSlot slot = paint_slot<false>(keep, false, s_wave);
        if (keep) { s_r0[slot.pos] = r0; s_c0[slot.pos] = c0; s_dr[slot.pos] = dr; s_dc[slot.pos] = dc; s_l[slot.pos] = l; }
        __syncthreads();
        if (t.inside) {
            for (int i = 0; i < slot.n; ++i)                               // same address in every lane: LDS broadcast
                if (seg_within<4>(t.y - s_r0[i], t.x - s_c0[i], s_dr[i], s_dc[i], d.rho4)) v = s_l[i];
        }
        __syncthreads();                                                   // the list is rewritten by the next 256 segments
    }
    if (!t.inside) return;
    if (STAMP) out[t.p] = (uint8_t)(v + 1);
    else if (v >= 0) out[t.p] = (uint8_t)v;
}

// exclusive prefix of v over the 256 threads of a workgroup; total = the sum.  s_wave: 4 words of LDS.
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += t;
    }
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
    for (int w = 0; w < 256 / WAVE; ++w) {
        off += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    __syncthreads();
    return off + incl - v;
}

// one wave per row of the batch: the number of stamped pixels of the row
__global__ void __launch_bounds__(256) k_stroke_row_count(int rows, int W, const uint8_t* __restrict__ stamp,
                                                          int32_t* __restrict__ row_cnt) {
    const int row = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                                               // wave-uniform
    const uint8_t* s = stamp + (size_t)row * W;
    int n = 0;
    for (int x0 = 0; x0 < W; x0 += WAVE)
        n += __popcll(__ballot(x0 + lane < W && s[x0 + lane] != 0));
    if (lane == 0) row_cnt[row] = n;
}

// one workgroup per image: its rows' counts -> their exclusive offsets inside the image (in place), and the image's count
__global__ void __launch_bounds__(256) k_stroke_image_scan(int H, int32_t* __restrict__ row_cnt, int32_t* __restrict__ img_cnt) {
    __shared__ int s_wave[256 / WAVE];
    int32_t* rc = row_cnt + (size_t)blockIdx.x * H;
    const int chunk = (H + 255) / 256, r0 = min(H, (int)threadIdx.x * chunk), r1 = min(H, r0 + chunk);
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += rc[r];
    int total;
    int run = block_exclusive_scan(sum, s_wave, total);
    for (int r = r0; r < r1; ++r) {
        const int c = rc[r];
        rc[r] = run;
        run += c;
    }
    if (threadIdx.x == 0) img_cnt[blockIdx.x] = total;
}

// one workgroup: the images' counts -> hint_ptr_out [B+1]
__global__ void __launch_bounds__(256) k_stroke_ptr_scan(int B, const int32_t* __restrict__ img_cnt, int32_t* __restrict__ hint_ptr_out) {
    __shared__ int s_wave[256 / WAVE];
    const int chunk = (B + 255) / 256, b0 = min(B, (int)threadIdx.x * chunk), b1 = min(B, b0 + chunk);
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += img_cnt[b];
    int total;
    int run = block_exclusive_scan(sum, s_wave, total);
    for (int b = b0; b < b1; ++b) {
        hint_ptr_out[b] = run;
        run += img_cnt[b];
    }
    if (threadIdx.x == 0) hint_ptr_out[B] = total;
}

// one wave per row: the row's stamped pixels as (row, col, label) from its offset on, left to right
__global__ void __launch_bounds__(256) k_stroke_fill(int rows, int H, int W, const uint8_t* __restrict__ stamp,
                                                     const int32_t* __restrict__ row_off, const int32_t* __restrict__ hint_ptr_out,
                                                     int32_t* __restrict__ hints_out) {
    const int row = blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                                               // wave-uniform
    const uint8_t* s = stamp + (size_t)row * W;
    const int b = row / H, y = row - b * H;
    int base = hint_ptr_out[b] + row_off[row];
    for (int x0 = 0; x0 < W; x0 += WAVE) {
        const int x = x0 + lane;
        const int v = x < W ? s[x] : 0;
        const unsigned long long m = __ballot(v != 0);
        if (v != 0) {
            int32_t* o = hints_out + 3 * (size_t)(base + __popcll(m & ((1ull << lane) - 1ull)));
            o[0] = y; o[1] = x; o[2] = v - 1 == GGC_FGD ? 1 : 0;
        }
        base += __popcll(m);
    }
}

// The checks both entries share, before any launch.  n_seg = stroke_ptr[B].
int read_strokes(ggc_ctx* ctx, hipStream_t st, int B, int H, int W, const int32_t* strokes, const int32_t* stroke_ptr,
                 int radius, int& n_seg) {
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (each at most 65535)", B, H, W);
    GGC_REQUIRE(ctx, radius >= 0 && radius <= ST_MAX_RADIUS, GGC_E_INVALID_ARG, "stroke radius %d outside 0..%d", radius, ST_MAX_RADIUS);
    std::vector<int32_t> sp;
    int rc = read_offsets(ctx, st, stroke_ptr, B, "stroke_ptr", "image", 0, sp);
    if (rc) return rc;
    n_seg = sp[B];
    if (n_seg == 0) return GGC_OK;
    GGC_REQUIRE(ctx, strokes, GGC_E_INVALID_ARG, "null strokes with %d segments", n_seg);
    GGC_REQUIRE(ctx, n_seg <= INT_MAX / 5, GGC_E_INVALID_ARG, "%d segments are too many", n_seg);
    std::vector<int32_t> seg;
    rc = read_i32(ctx, st, strokes, 5 * n_seg, seg);
    if (rc) return rc;
    for (int k = 0; k < n_seg; ++k)
        for (int j = 0; j < 4; ++j) {
            const int32_t v = seg[5 * (size_t)k + j];
            GGC_REQUIRE(ctx, v >= -ST_MAX_COORD && v <= ST_MAX_COORD, GGC_E_INVALID_ARG,
                        "segment %d has an endpoint coordinate %d beyond +-2^20", k, v);
        }
    return GGC_OK;
}

SDims stroke_dims(int B, int H, int W, int radius) {
    const unsigned long long r2 = 2ull * (unsigned long long)radius;
    static_assert((PT_W - 1) * (PT_W - 1) + (PT_H - 1) * (PT_H - 1) < 32 * 32, "the cull's + 32 covers the tile's doubled half-diagonal");
    const unsigned long long reach = (r2 > 1 ? r2 : 1) + 32;              // doubled: brush + the 32x8 tile's half-diagonal, sqrt(1010) < 32
    return SDims{B, H, W, r2 * r2 > 1 ? r2 * r2 : 1, reach * reach};
}

} // namespace
} // namespace ggc

extern "C" int ggc_apply_strokes(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* strokes,
                                 const int32_t* stroke_ptr, int radius, uint8_t* mask) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, stroke_ptr && mask, GGC_E_INVALID_ARG, "null pointer");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int n_seg = 0;
    int rc = read_strokes(ctx, st, B, H, W, strokes, stroke_ptr, radius, n_seg);
    if (rc) return rc;
    if (n_seg == 0) return GGC_OK;
    const int tiles_x = cdiv(W, PT_W), tiles = tiles_x * cdiv(H, PT_H);
    hipLaunchKernelGGL(k_paint_strokes<false>, dim3(tiles, B), dim3(PT_THREADS), 0, st, stroke_dims(B, H, W, radius), tiles_x,
                       strokes, stroke_ptr, mask);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

extern "C" int ggc_stroke_pixels(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* strokes,
                                 const int32_t* stroke_ptr, int32_t* hint_ptr_out, int32_t* hints_out, int64_t capacity) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, stroke_ptr && hint_ptr_out, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, !hints_out || capacity >= 0, GGC_E_INVALID_ARG, "negative capacity %lld", (long long)capacity);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int n_seg = 0;
    int rc = read_strokes(ctx, st, B, H, W, strokes, stroke_ptr, 0, n_seg);
    if (rc) return rc;
    GGC_REQUIRE(ctx, (int64_t)B * H * W <= INT_MAX, GGC_E_SHAPE, "B*H*W = %lld does not fit the int32 hint_ptr",
                (long long)((int64_t)B * H * W));
    if (n_seg == 0) {
        GGC_HIP(ctx, hipMemsetAsync(hint_ptr_out, 0, sizeof(int32_t) * (size_t)(B + 1), st));
        return GGC_OK;
    }
    const int rows = B * H;
    uint8_t* stamp = nullptr;
    int32_t *row_off = nullptr, *img_cnt = nullptr;
    if (!carve_scratch(ctx, S_STROKES, [&](Carve& c) {
            stamp = c.take<uint8_t>((size_t)rows * W);
            row_off = c.take<int32_t>((size_t)rows);
            img_cnt = c.take<int32_t>((size_t)B);
        }))
        return GGC_E_OOM;
    const int tiles_x = cdiv(W, PT_W), tiles = tiles_x * cdiv(H, PT_H), row_blocks = cdiv(rows, 256 / WAVE);
    hipLaunchKernelGGL(k_paint_strokes<true>, dim3(tiles, B), dim3(PT_THREADS), 0, st, stroke_dims(B, H, W, 0), tiles_x,
                       strokes, stroke_ptr, stamp);
    hipLaunchKernelGGL(k_stroke_row_count, dim3(row_blocks), dim3(256), 0, st, rows, W, stamp, row_off);
    hipLaunchKernelGGL(k_stroke_image_scan, dim3(B), dim3(256), 0, st, H, row_off, img_cnt);
    hipLaunchKernelGGL(k_stroke_ptr_scan, dim3(1), dim3(256), 0, st, B, img_cnt, hint_ptr_out);
    GGC_LAUNCH_CHECK(ctx);
    if (!hints_out) return GGC_OK;
    std::vector<int32_t> total;
    rc = read_i32(ctx, st, hint_ptr_out + B, 1, total);
    if (rc) return rc;
    GGC_REQUIRE(ctx, capacity >= total[0], GGC_E_INVALID_ARG, "capacity %lld is below the %d stroke pixels", (long long)capacity, total[0]);
    if (total[0] == 0) return GGC_OK;
    hipLaunchKernelGGL(k_stroke_fill, dim3(row_blocks), dim3(256), 0, st, rows, H, W, stamp, row_off, hint_ptr_out, hints_out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
