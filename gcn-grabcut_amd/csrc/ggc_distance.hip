// ggc_distance.hip — the exact squared Euclidean distance transform of a mask and the modifiers that are thresholds of it
// (include/ggc.h K2 / K3): ggc_mask_distance, ggc_modify_mask.  Integer only.
//
// Separable, two launches per step; what a lane does in each is a function of ggc_edt.h, shared with the host:
//   k_dt_cols   one lane per column (loads and stores coalesced across x), edt_column: two sweeps, down leaves the distance
//               to the nearest opposite pixel above, up takes the minimum with the one below.  Both classes in one pass: a
//               pixel's g is the distance to the class it does not have.  Stored as 16 bits: g in the low 15 (EDT_NONE =
//               none, and also every g beyond the step's reach, which could not win), the pixel's class in bit 15, so that
//               the row pass never reads the mask and `out` may alias it.
//   k_dt_rows   one block per row, the row's 16-bit words staged in LDS (at most 32 KiB), every pixel runs edt_pixel over
//               them.  The result is written as the signed int32 plane, or thresholded into the u8 plane of a modifier.
// OPEN and CLOSE are two such steps through a u8 plane of scratch.  No host synchronisation, no atomics.
#include "ggc_internal.h"
#include "ggc_edt.h"
#include <algorithm>

namespace ggc {
namespace {

__global__ void __launch_bounds__(64) k_dt_cols(int B, int H, int W, EdtReach reach, int border,
                                                const uint8_t* __restrict__ mask, uint16_t* __restrict__ g) {
    const int per_image = (W + 63) >> 6;                                // blocks of 64 columns per image
    for (int64_t blk = blockIdx.x; blk < (int64_t)B * per_image; blk += gridDim.x) {
        const int x = (int)(blk % per_image) * 64 + (int)threadIdx.x;
        const size_t image = (size_t)(blk / per_image) * H * W;
        if (x < W) edt_column(H, W, reach, border, x, mask + image, g + image);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) k_dt_rows(int rows, int W, EdtReach reach, int border, const uint16_t* __restrict__ g,
                                                 int32_t* __restrict__ d2_out, uint8_t* __restrict__ u8_out) {
    extern __shared__ uint16_t s_row[];
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {           // uniform per block: the barriers below are safe
        const size_t base = (size_t)row * W;
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += blockDim.x) s_row[x] = g[base + x];
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += blockDim.x) {
            uint32_t mag;
            const int fg = edt_pixel(s_row, W, x, reach, border, &mag);
            if (MODE == EDT_D2) d2_out[base + x] = fg ? -(int32_t)mag : (int32_t)mag;
            else u8_out[base + x] = edt_threshold(MODE, fg, mag != EDT_FAR);
        }
    }
}

int dt_step(ggc_ctx* ctx, hipStream_t st, int B, int H, int W, const uint8_t* mask, const EdtReach& reach, int border, int mode,
            int32_t* d2_out, uint8_t* u8_out) {
    const size_t n = (size_t)B * H * W;
    uint16_t* g = scratch_t<uint16_t>(ctx, S_DIST, n);
    if (!g) return GGC_E_OOM;
    {
        ProfScope ps(ctx, st, "distance_cols");
        const int blocks = (int)std::min<int64_t>((int64_t)B * cdiv(W, 64), 1 << 20);
        hipLaunchKernelGGL(k_dt_cols, dim3(blocks), dim3(64), 0, st, B, H, W, reach, border, mask, g);
        GGC_LAUNCH_CHECK(ctx);
    }
    const int rows = B * H;                                             // B H W < 2^31
    const int threads = W <= 64 ? 64 : (W <= 128 ? 128 : 256);
    const int blocks = std::min(rows, 1 << 20);
    const size_t lds = (size_t)W * sizeof(uint16_t);
    ProfScope ps(ctx, st, "distance_rows");
#define GGC_DT_ROWS(M) hipLaunchKernelGGL(k_dt_rows<M>, dim3(blocks), dim3(threads), lds, st, rows, W, reach, border, g, d2_out, u8_out)
    switch (mode) {
        case EDT_D2: GGC_DT_ROWS(EDT_D2); break;
        case EDT_GROW: GGC_DT_ROWS(EDT_GROW); break;
        case EDT_SHRINK: GGC_DT_ROWS(EDT_SHRINK); break;
        case EDT_BORDER: GGC_DT_ROWS(EDT_BORDER); break;
        default: GGC_DT_ROWS(EDT_TRIMAP); break;
    }
#undef GGC_DT_ROWS
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

// The refusals the two entries share.
int dt_check(ggc_ctx* ctx, int B, int H, int W, const void* in, const void* out, int flags) {
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (H and W in 1..16384)", B, H, W);
    GGC_REQUIRE(ctx, (int64_t)B * H * W < (int64_t(1) << 31), GGC_E_SHAPE, "B*H*W = %lld, expected less than 2^31",
                (long long)((int64_t)B * H * W));
    GGC_REQUIRE(ctx, in && out, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, (flags & ~GGC_DIST_BORDER_BG) == 0, GGC_E_INVALID_ARG, "unknown flag bits 0x%x", flags);
    return GGC_OK;
}

} // namespace
} // namespace ggc

extern "C" int ggc_mask_distance(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask, int flags,
                                 int64_t max_dist2, int32_t* signed_d2_out) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    if (int rc = dt_check(ctx, B, H, W, mask, signed_d2_out, flags)) return rc;
    GGC_REQUIRE(ctx, max_dist2 >= 0, GGC_E_INVALID_ARG, "negative max_dist2 %lld", (long long)max_dist2);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    EdtReach reach;
    if (max_dist2 == 0) { reach.rcap[0] = -1; reach.cap2[0] = EDT_FAR; }
    else edt_reach(max_dist2, reach.rcap[0], reach.cap2[0]);
    reach.rcap[1] = reach.rcap[0]; reach.cap2[1] = reach.cap2[0];
    return dt_step(ctx, st, B, H, W, mask, reach, flags & GGC_DIST_BORDER_BG, EDT_D2, signed_d2_out, nullptr);
}

extern "C" int ggc_modify_mask(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask_in, int op,
                               int64_t r2_a, int64_t r2_b, int flags, uint8_t* out) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    if (int rc = dt_check(ctx, B, H, W, mask_in, out, flags)) return rc;
    GGC_REQUIRE(ctx, op >= GGC_MODIFY_GROW && op <= GGC_MODIFY_TRIMAP, GGC_E_INVALID_ARG, "unknown op %d", op);
    GGC_REQUIRE(ctx, r2_a >= 0 && r2_b >= 0, GGC_E_INVALID_ARG, "negative radius %lld / %lld", (long long)r2_a, (long long)r2_b);
    const bool two_radii = op == GGC_MODIFY_BORDER || op == GGC_MODIFY_TRIMAP;
    GGC_REQUIRE(ctx, two_radii || r2_b == 0, GGC_E_INVALID_ARG, "r2_b = %lld, expected 0 for op %d", (long long)r2_b, op);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int border = flags & GGC_DIST_BORDER_BG;
    EdtStep steps[2];
    if (edt_plan(op, r2_a, r2_b, steps) == 1)
        return dt_step(ctx, st, B, H, W, mask_in, steps[0].reach, border, steps[0].mode, nullptr, out);
    uint8_t* tmp = scratch_t<uint8_t>(ctx, S_DIST_TMP, (size_t)B * H * W);
    if (!tmp) return GGC_E_OOM;
    if (int rc = dt_step(ctx, st, B, H, W, mask_in, steps[0].reach, border, steps[0].mode, nullptr, tmp)) return rc;
    return dt_step(ctx, st, B, H, W, tmp, steps[1].reach, border, steps[1].mode, nullptr, out);
}
