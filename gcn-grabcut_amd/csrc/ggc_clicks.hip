// ggc_clicks.hip — C0: the next simulated click of the standard NoC protocol, per image.
//
// The click goes to the pixel of the false-negative (fn = gt & !pred) or false-positive (fp = !gt & pred) region that is
// farthest from the region's outside, in exact squared Euclidean distance (the image is padded by one pixel that belongs
// to no region).  Three launches, integer arithmetic only:
//   k_click_cols  one lane per (image, column): the vertical distance g to the nearest non-region pixel, for fn and fp at
//                 once (two u16 in one u32 per pixel), by a downward and an upward scan of the column.
//   k_click_rows  one workgroup per (image, row), the row's g in LDS: d2(x) = min over x' of (x-x')^2 + g(x')^2, which is
//                 the exact 2-D distance (separability of the squared Euclidean distance).  Each lane searches |x-x'| while
//                 (x-x')^2 < the best so far, starting from min(g(x)^2, (x+1)^2, (W-x)^2), so the work per pixel is at most
//                 its own distance.  A pixel lies in at most one region, so one search serves it.  The row's best key
//                 (d2 << 32) | ~(y*W+x) per region goes to the image's slot with an integer atomicMax: larger d2 wins,
//                 then the smaller raster index, whatever the order of arrival.
//   k_click_pick  one lane per image: fn wins only with a strictly larger maximum; (-1,-1,-1,0) when neither has a pixel.
#include "ggc_internal.h"

namespace ggc {
namespace {

constexpr int CK_THREADS = 256;
constexpr int CK_UNROLL = 8;          // column loads in flight per lane
constexpr int CK_MAX_W = 8192;        // u32 per column of the row in LDS: 32 KiB
constexpr int CK_MAX_H = 65535;       // g fits in u16

__global__ void __launch_bounds__(CK_THREADS) k_click_cols(int H, int W, const uint8_t* __restrict__ pred,
                                                          const uint8_t* __restrict__ gt, uint32_t* __restrict__ g) {
    const int x = blockIdx.x * CK_THREADS + threadIdx.x, b = blockIdx.y;
    if (x >= W) return;
    const size_t base = (size_t)b * H * W + x;
    const uint8_t* pp = pred + base;
    const uint8_t* gp = gt + base;
    uint32_t* out = g + base;
    uint32_t a_fn = 0, a_fp = 0;                     // run length of the region above, the padding row included
    int y = 0;
    for (; y + CK_UNROLL <= H; y += CK_UNROLL) {
        uint8_t p[CK_UNROLL], t[CK_UNROLL];
#pragma unroll
        for (int i = 0; i < CK_UNROLL; ++i) {
            p[i] = pp[(size_t)(y + i) * W];
            t[i] = gp[(size_t)(y + i) * W];
        }
#pragma unroll
        for (int i = 0; i < CK_UNROLL; ++i) {
            a_fn = (t[i] && !p[i]) ? a_fn + 1 : 0;
            a_fp = (!t[i] && p[i]) ? a_fp + 1 : 0;
            out[(size_t)(y + i) * W] = a_fn | (a_fp << 16);
        }
    }
    for (; y < H; ++y) {
        const uint8_t p = pp[(size_t)y * W], t = gp[(size_t)y * W];
        a_fn = (t && !p) ? a_fn + 1 : 0;
        a_fp = (!t && p) ? a_fp + 1 : 0;
        out[(size_t)y * W] = a_fn | (a_fp << 16);
    }
    // upward: g = min(down, up); a pixel outside the region has down == 0 and keeps it
    a_fn = a_fp = 0;
    y = H;
    for (; y - CK_UNROLL >= 0; y -= CK_UNROLL) {
        uint32_t v[CK_UNROLL];
#pragma unroll
        for (int i = 1; i <= CK_UNROLL; ++i) v[i - 1] = out[(size_t)(y - i) * W];
#pragma unroll
        for (int i = 1; i <= CK_UNROLL; ++i) {
            const uint32_t d_fn = v[i - 1] & 0xFFFFu, d_fp = v[i - 1] >> 16;
            a_fn = d_fn ? min(d_fn, a_fn + 1) : 0;
            a_fp = d_fp ? min(d_fp, a_fp + 1) : 0;
            const uint32_t nv = a_fn | (a_fp << 16);
            if (nv != v[i - 1]) out[(size_t)(y - i) * W] = nv;
        }
    }
    for (--y; y >= 0; --y) {
        const uint32_t v = out[(size_t)y * W];
        const uint32_t d_fn = v & 0xFFFFu, d_fp = v >> 16;
        a_fn = d_fn ? min(d_fn, a_fn + 1) : 0;
        a_fp = d_fp ? min(d_fp, a_fp + 1) : 0;
        const uint32_t nv = a_fn | (a_fp << 16);
        if (nv != v) out[(size_t)y * W] = nv;
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__global__ void __launch_bounds__(CK_THREADS) k_click_rows(int H, int W, const uint32_t* __restrict__ g,
                                                          unsigned long long* __restrict__ keys /*[B,2] fn, fp*/) {
    extern __shared__ uint32_t s_g[];                // [W]
    __shared__ unsigned long long s_key[2][CK_THREADS / WAVE];
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* row = g + ((size_t)b * H + y) * W;
    for (int x = tid; x < W; x += CK_THREADS) s_g[x] = row[x];
    __syncthreads();
    unsigned long long k_fn = 0, k_fp = 0;
    for (int x = tid; x < W; x += CK_THREADS) {
        const uint32_t v = s_g[x];
        if (!v) continue;                            // in no region
        const int shift = (v & 0xFFFFu) ? 0 : 16;    // fn and fp are disjoint: search the pixel's own region
        const uint32_t gx = (v >> shift) & 0xFFFFu;
        uint32_t best = gx * gx;
        const uint32_t bl = (uint32_t)(x + 1) * (uint32_t)(x + 1), br = (uint32_t)(W - x) * (uint32_t)(W - x);
        best = min(best, min(bl, br));               // the padding column on either side
        for (uint32_t dx = 1; dx * dx < best; ++dx) {    // x -+ dx stay inside the image: dx^2 < (x+1)^2 and < (W-x)^2
            const uint32_t gl = (s_g[x - dx] >> shift) & 0xFFFFu, gr = (s_g[x + dx] >> shift) & 0xFFFFu;
            const uint32_t gm = min(gl, gr);
            best = min(best, dx * dx + gm * gm);
        }
        const unsigned long long key = ((unsigned long long)best << 32) | (uint32_t)~(uint32_t)(y * W + x);
        if (shift == 0) k_fn = key > k_fn ? key : k_fn;
        else k_fp = key > k_fp ? key : k_fp;
    }
    k_fn = wave_max_u64(k_fn);
    k_fp = wave_max_u64(k_fp);
    if (lane == 0) { s_key[0][wave] = k_fn; s_key[1][wave] = k_fp; }
    __syncthreads();
    if (tid < 2) {
        unsigned long long k = 0;
        for (int w = 0; w < CK_THREADS / WAVE; ++w) k = s_key[tid][w] > k ? s_key[tid][w] : k;
        if (k) atomicMax(&keys[2 * b + tid], k);
    }
}

__global__ void k_click_pick(int B, int W, const unsigned long long* __restrict__ keys, int32_t* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long k_fn = keys[2 * b], k_fp = keys[2 * b + 1];
    const uint32_t m_fn = (uint32_t)(k_fn >> 32), m_fp = (uint32_t)(k_fp >> 32);
    int32_t* o = out + 4 * b;
    if (m_fn == 0 && m_fp == 0) { o[0] = -1; o[1] = -1; o[2] = -1; o[3] = 0; return; }
    const bool fg = m_fn > m_fp;                     // a tie goes to the background click
    const unsigned long long k = fg ? k_fn : k_fp;
    const uint32_t idx = ~(uint32_t)k;
    o[0] = (int32_t)(idx / (uint32_t)W);
    o[1] = (int32_t)(idx % (uint32_t)W);
    o[2] = fg ? 1 : 0;
    o[3] = (int32_t)(fg ? m_fn : m_fp);
}

} // namespace
} // namespace ggc

extern "C" int ggc_next_click(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* pred, const uint8_t* gt,
                              int32_t* out) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535, GGC_E_INVALID_ARG, "bad batch size B=%d", B);
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, H >= 1 && W >= 1 && H <= CK_MAX_H && W <= CK_MAX_W, GGC_E_INVALID_ARG,
                "bad image size H=%d W=%d (1..%d x 1..%d)", H, W, CK_MAX_H, CK_MAX_W);
    GGC_REQUIRE(ctx, pred && gt && out, GGC_E_INVALID_ARG, "null pointer");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint32_t* g = nullptr;
    unsigned long long* keys = nullptr;
    if (!carve_scratch(ctx, S_CLICK, [&](Carve& c) {
            g = c.take<uint32_t>((size_t)B * H * W);
            keys = c.take<unsigned long long>((size_t)B * 2);
        }))
        return GGC_E_OOM;
    GGC_HIP(ctx, hipMemsetAsync(keys, 0, sizeof(unsigned long long) * 2 * (size_t)B, st));
    hipLaunchKernelGGL(k_click_cols, dim3(cdiv(W, CK_THREADS), B), dim3(CK_THREADS), 0, st, H, W, pred, gt, g);
    hipLaunchKernelGGL(k_click_rows, dim3(H, B), dim3(CK_THREADS), sizeof(uint32_t) * (size_t)W, st, H, W, g, keys);
    hipLaunchKernelGGL(k_click_pick, dim3(cdiv(B, 64)), dim3(64), 0, st, B, W, keys, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
