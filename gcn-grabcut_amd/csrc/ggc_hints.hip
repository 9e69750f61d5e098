// ggc_hints.hip — H0: user clicks as hard constraints on the GrabCut mask (reference graph_builder.py:457-494, batched).
//
// Three launches, the first two only when superpixels are involved:
//   k_hint_flags   one lane per click: atomicOr of bit 0 (foreground) / bit 1 (background) into a flag word per node.
//                  Integer OR is order independent, so the words do not depend on launch order.
//   k_node_hints   one lane per node: the three columns of encode_user_hints from its flag word.
//   k_apply_hints  the tile painter (ggc_paint.h).  The region pass reads the pixel's flag word; the disk pass keeps a
//                  click when its disk meets the tile, i.e. when the nearest pixel of the tile, clipped to the image, is
//                  within the radius.  Work is O(pixels + tiles x clicks); a pixel no hint touches is neither read nor
//                  written.
#include "ggc_paint.h"

namespace ggc {
namespace {

struct HDims { int B, H, W; int64_t r2; };

// image of click k: the last b with hint_ptr[b] <= k (hint_ptr is non-decreasing, checked on the host)
__device__ __forceinline__ int click_image(const int32_t* __restrict__ hint_ptr, int B, int k) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (hint_ptr[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_hint_flags(HDims d, int K, const int32_t* __restrict__ hints,
                                                    const int32_t* __restrict__ hint_ptr, const int32_t* __restrict__ segments,
                                                    const int32_t* __restrict__ node_ptr, int32_t* __restrict__ flags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int r = hints[3 * k], c = hints[3 * k + 1], fg = hints[3 * k + 2] != 0;
    if (r < 0 || r >= d.H || c < 0 || c >= d.W) return;                  // outside its image: ignored (reference :482, :489)
    const int b = click_image(hint_ptr, d.B, k);
    const int n0 = node_ptr[b], nb = node_ptr[b + 1] - n0;
    const int s = segments[(size_t)b * d.H * d.W + (size_t)r * d.W + c];
    if (s >= 0 && s < nb) atomicOr(&flags[n0 + s], fg ? 1 : 2);
}

__global__ void __launch_bounds__(256) k_node_hints(int N, const int32_t* __restrict__ flags, float* __restrict__ node_hints) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int f = flags[n];
    node_hints[3 * n] = (f & 1) ? 1.0f : 0.0f;
    node_hints[3 * n + 1] = (f & 2) ? 1.0f : 0.0f;
    node_hints[3 * n + 2] = f ? 0.0f : 1.0f;
}

__global__ void __launch_bounds__(PT_THREADS) k_apply_hints(HDims d, int tiles_x, const int32_t* __restrict__ hints,
                                                            const int32_t* __restrict__ hint_ptr,
                                                            const int32_t* __restrict__ segments,
                                                            const int32_t* __restrict__ node_ptr,
                                                            const int32_t* __restrict__ flags, uint8_t* __restrict__ mask) {
    __shared__ int s_r[PT_THREADS], s_c[PT_THREADS], s_l[PT_THREADS];
    __shared__ int s_wave[PT_THREADS / WAVE];
    const PaintTile t = paint_tile(d.H, d.W, tiles_x);
    int v = -1;                                                            // new label, -1 = untouched
    if (flags && t.inside) {
        const int s = segments[t.p], n0 = node_ptr[t.b];
        if (s >= 0 && s < node_ptr[t.b + 1] - n0) {
            const int f = flags[n0 + s];
            if (f == 1) v = GGC_FGD;                                       // every click on the region is foreground
            else if (f == 2) v = GGC_BGD;                                  // every click is background; mixed: the disks decide
        }
    }
    // the tile as a rectangle clipped to the image: a disk meets it when the nearest tile pixel is within the radius
    const int tx0 = t.tx0, ty0 = t.ty0, tx1 = min(tx0 + PT_W, d.W) - 1, ty1 = min(ty0 + PT_H, d.H) - 1;
    const int k0 = hint_ptr[t.b], k1 = hint_ptr[t.b + 1];
    for (int base = k0; base < k1; base += PT_THREADS) {                  // block-uniform loop
        const int k = base + threadIdx.x;
        int r = 0, c = 0, l = 0;
        bool keep = false;
        if (k < k1) {
            r = hints[3 * k]; c = hints[3 * k + 1]; l = hints[3 * k + 2] != 0 ? GGC_FGD : GGC_BGD;
            if (r >= 0 && r < d.H && c >= 0 && c < d.W) {
                const int64_t dy = r < ty0 ? ty0 - r : (r > ty1 ? r - ty1 : 0);
                const int64_t dx = c < tx0 ? tx0 - c : (c > tx1 ? c - tx1 : 0);
                keep = dy * dy + dx * dx <= d.r2;
            }
        }
        const PaintSlot slot = paint_slot<false>(keep, false, s_wave);
        if (keep) { s_r[slot.pos] = r; s_c[slot.pos] = c; s_l[slot.pos] = l; }
        __syncthreads();
        if (t.inside) {
            for (int i = 0; i < slot.n; ++i) {                             // same address in every lane: LDS broadcast
                const int64_t dy = t.y - s_r[i], dx = t.x - s_c[i];
                if (dy * dy + dx * dx <= d.r2) v = s_l[i];
            }
        }
        __syncthreads();                                                   // the list is rewritten by the next 256 clicks
    }
    if (t.inside && v >= 0) mask[t.p] = (uint8_t)v;
}

} // namespace
} // namespace ggc

extern "C" int ggc_apply_hints(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* hints,
                               const int32_t* hint_ptr, int radius, int region, const int32_t* segments,
                               const int32_t* node_ptr, float* node_hints, uint8_t* mask) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, radius >= 0, GGC_E_INVALID_ARG, "negative hint radius %d", radius);
    GGC_REQUIRE(ctx, region == 0 || region == 1, GGC_E_INVALID_ARG, "region must be 0 or 1, got %d", region);
    GGC_REQUIRE(ctx, hint_ptr && (mask || node_hints), GGC_E_INVALID_ARG, "null pointer");
    const bool need_nodes = region || node_hints;
    GGC_REQUIRE(ctx, !need_nodes || (segments && node_ptr), GGC_E_INVALID_ARG, "region pass and node_hints need segments and node_ptr");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    std::vector<int32_t> hp;
    int rc = read_offsets(ctx, st, hint_ptr, B, "hint_ptr", "image", 0, hp);
    if (rc) return rc;
    const int K = hp[B];
    if (K == 0) return GGC_OK;
    GGC_REQUIRE(ctx, hints, GGC_E_INVALID_ARG, "null hints with %d clicks", K);
    const HDims d{B, H, W, (int64_t)radius * radius};

    int32_t* flags = nullptr;
    if (need_nodes) {
        std::vector<int32_t> np_;
        rc = read_offsets(ctx, st, node_ptr, B, "node_ptr", "image", 0, np_);
        if (rc) return rc;
        const int N = np_[B];
        if (N > 0) {
            flags = scratch_t<int32_t>(ctx, S_MISC_A, (size_t)N);
            if (!flags) return GGC_E_OOM;
            GGC_HIP(ctx, hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)N, st));
            hipLaunchKernelGGL(k_hint_flags, dim3(cdiv(K, 256)), dim3(256), 0, st, d, K, hints, hint_ptr, segments, node_ptr, flags);
            if (node_hints)
                hipLaunchKernelGGL(k_node_hints, dim3(cdiv(N, 256)), dim3(256), 0, st, N, flags, node_hints);
        }
    }
    if (mask) {
        const int tiles_x = cdiv(W, PT_W), tiles = tiles_x * cdiv(H, PT_H);
        hipLaunchKernelGGL(k_apply_hints, dim3(tiles, B), dim3(PT_THREADS), 0, st, d, tiles_x, hints, hint_ptr, segments,
                           node_ptr, region ? flags : nullptr, mask);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
