// ggc_gridflow.hip — the max-flow of ggc_maxflow.hip on a caller's network (ggc_grid_maxflow, include/ggc.h).
//
// A test hook that shares the production path: k_gf_build runs the per-pixel graph set-up of ggc_grabcut
// (mf_cold_pixel / mf_warm_pixel, ggc_gc.h) on the given t-link differences, then maxflow() solves exactly as in a GrabCut iteration:
// step 0 cold, later steps warm under GGC_MF_WARM.  The networks a test builds (long corridors, walls crossed only at
// tile corners, cuts on tile borders, capacities at the stated bounds) are what GMM likelihoods of natural images
// never produce.
#include "ggc_gc.h"
#include <algorithm>
#include <vector>

namespace ggc {
namespace {

constexpr int32_t GF_TW_MAX = 1 << 27;   // |tw| bound: LAMBDA * CAP_SCALE = 117 964 800 fits under it
constexpr int32_t GF_NW_MAX = 1 << 24;   // nw bound: GAMMA * CAP_SCALE = 13 107 200 fits under it

// err bit 0: some |tw| > 2^27; bit 1: some in-image link < 0; bit 2: some in-image link > 2^24.  Links that point outside
// the image are never read by the solve, so they are not checked either.
__global__ void __launch_bounds__(256) k_gf_check(GcDims d, int n_steps, const int32_t* __restrict__ tw,
                                                  const int32_t* __restrict__ nw, int32_t* __restrict__ err) {
    const size_t BP = (size_t)d.B * d.P, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (i < BP) {
        const int p = (int)(i % d.P), y = p / d.W, x = p % d.W;
        for (int s = 0; s < n_steps; ++s) {
            const int32_t t = tw[(size_t)s * BP + i];
            bad |= (t < -GF_TW_MAX || t > GF_TW_MAX) ? 1 : 0;
        }
        const int dirs[4] = {0, 4, 2, 6};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (dir_nb(d, y, x, dirs[k]) < 0) continue;
            const int32_t w = nw[(size_t)k * BP + i];
            bad |= (w < 0 ? 2 : 0) | (w > GF_NW_MAX ? 4 : 0);
        }
    }
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(err, bad);
}

// tw_old: the previous step's t-link differences for a warm step (the caller's own plane), null for a cold one
__global__ void __launch_bounds__(256) k_gf_build(GcDims d, const int32_t* __restrict__ tw, const int32_t* __restrict__ tw_old,
                                                  const int32_t* __restrict__ nw, int32_t* __restrict__ rc, int32_t* __restrict__ ex,
                                                  int32_t* __restrict__ snk, uint8_t* __restrict__ rmask) {
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.P) return;
    const size_t i = (size_t)b * d.P + p;
    if (tw_old) { mf_warm_pixel(i, tw[i], tw_old[i], ex, snk); return; }
    int32_t cap[8];
    mf_plane_caps(d, b, p, nw, cap);
    mf_cold_pixel(i, tw[i], cap, rc, ex, snk, rmask);
}

__global__ void __launch_bounds__(256) k_gf_side(size_t n, const int32_t* __restrict__ dist, uint8_t* __restrict__ side) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) side[i] = dist[i] >= DINF ? 1 : 0;
}

// residual [B][P][10]: rc[8] in direction order, excess, residual sink capacity
__global__ void __launch_bounds__(256) k_gf_residual(size_t n, const int32_t* __restrict__ rc, const int32_t* __restrict__ ex,
                                                     const int32_t* __restrict__ snk, int32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int dir = 0; dir < 8; ++dir) out[i * 10 + dir] = rc[rc_idx(dir, i)];
    out[i * 10 + 8] = ex[i];
    out[i * 10 + 9] = snk[i];
}

} // namespace
} // namespace ggc

using namespace ggc;

extern "C" int ggc_grid_maxflow(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, int n_steps, const int32_t* tw,
                                const int32_t* nw, uint8_t* source_side, int32_t* residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_INVALID_ARG, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, (size_t)H * W < (1u << 28), GGC_E_SHAPE, "image too large");
    GGC_REQUIRE(ctx, n_steps >= 1, GGC_E_INVALID_ARG, "n_steps must be >= 1 (got %d)", n_steps);
    GGC_REQUIRE(ctx, tw && nw && source_side, GGC_E_INVALID_ARG, "null pointer");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GcDims d{B, H, W, H * W, 0};
    const size_t BP = (size_t)B * d.P;

    // the control block, zeroed once: state [B] (every image solved), err [2] (input check | max-flow), the max-flow's words
    int32_t *state, *err;
    MfControl mf;
    const size_t ctl_bytes = carve_scratch(ctx, S_GC_A, [&](Carve& c) {
        state = c.take<int32_t>(B); err = c.take<int32_t>(2);
        mf = {c.take<int32_t>(B), c.take<int32_t>(8), c.take<int32_t>(2 * (size_t)B), err ? err + 1 : nullptr};
    });
    int32_t* rc = scratch_t<int32_t>(ctx, S_GC_F, BP * 8);
    int32_t* ex = scratch_t<int32_t>(ctx, S_GC_G, BP * 3);
    uint8_t* rmask = scratch_t<uint8_t>(ctx, S_GC_L, BP);
    if (!ctl_bytes || !rc || !ex || !rmask) return GGC_E_OOM;
    int32_t* snk = ex + BP;
    int32_t* dist = ex + 2 * BP;
    GGC_HIP(ctx, hipMemsetAsync(state, 0, ctl_bytes, st));               // (state starts the control block)

    hipLaunchKernelGGL(k_gf_check, dim3(cdiv(BP, 256)), dim3(256), 0, st, d, n_steps, tw, nw, err);
    GGC_LAUNCH_CHECK(ctx);
    std::vector<int32_t> herr;
    int rcode = read_i32(ctx, st, err, 1, herr);
    if (rcode) return rcode;
    GGC_REQUIRE(ctx, !(herr[0] & 1), GGC_E_INVALID_ARG, "a t-link difference lies outside [-2^27, 2^27]");
    GGC_REQUIRE(ctx, !(herr[0] & 2), GGC_E_INVALID_ARG, "an in-image n-link is negative");
    GGC_REQUIRE(ctx, !(herr[0] & 4), GGC_E_INVALID_ARG, "an in-image n-link exceeds 2^24");

    int n_open = -1;                    // every image is open in every step: counted by the first solve only
    for (int s = 0; s < n_steps; ++s) {
        const bool warm = knobs().mf_warm && s > 0;
        const int32_t* tw_s = tw + (size_t)s * BP;
        hipLaunchKernelGGL(k_gf_build, dim3(cdiv(d.P, 256), B), dim3(256), 0, st, d, tw_s, warm ? tw_s - BP : nullptr, nw, rc, ex, snk, rmask);
        GGC_LAUNCH_CHECK(ctx);
        if ((rcode = maxflow(ctx, st, d, state, rc, ex, snk, dist, rmask, mf, !warm, n_open))) return rcode;
        hipLaunchKernelGGL(k_gf_side, dim3(cdiv(BP, 256)), dim3(256), 0, st, BP, dist, source_side + (size_t)s * BP);
        GGC_LAUNCH_CHECK(ctx);
        if ((rcode = read_i32(ctx, st, err + 1, 1, herr))) return rcode;
        GGC_REQUIRE(ctx, herr[0] == 0, GGC_E_DEVICE, "max-flow did not converge in step %d (code %d)", s, herr[0]);
    }
    if (residual) {
        hipLaunchKernelGGL(k_gf_residual, dim3(cdiv(BP, 256)), dim3(256), 0, st, BP, rc, ex, snk, residual);
        GGC_LAUNCH_CHECK(ctx);
    }
    GGC_HIP(ctx, hipStreamSynchronize(st));
    return GGC_OK;
}
