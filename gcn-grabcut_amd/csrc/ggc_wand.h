// ggc_wand.h — the per-pixel rule of the magic wand (include/ggc.h H5), shared by the kernels of
// ggc_wand.hip and by a stand-alone host program (tests/wand_rule_main.cpp), as ggc_edt.h and ggc_outline.h are shared.
//
// A seed's reference colour is the sum of the n x n bytes around it, per channel, the border replicated; a pixel matches the
// seed iff, in every channel, n^2 times its byte is within n^2 * tolerance of that sum.  Integer only: no division, no
// float; the largest value is 25 * 255 = 6375.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GGC_WAND_HD __host__ __device__ inline
#else
#define GGC_WAND_HD inline
#endif

namespace ggc {

// One live seed (inside its image), in seed order: what the kernels read.
struct WandSeed {
    int32_t image;          // b
    int32_t pixel;          // row * W + col
    int32_t label;          // 0 = background / subtract, nonzero = foreground / add
    int32_t ref[3];         // the reference sums, filled on the device
};

// The reference sums of the seed at (r, c) of the image whose pixel (0, 0) is img[0..2]; n in {1, 3, 5}.
GGC_WAND_HD void wand_ref_sums(const uint8_t* img, int H, int W, int r, int c, int n, int32_t ref[3]) {
    const int h = n / 2;
    ref[0] = ref[1] = ref[2] = 0;
    for (int dy = -h; dy <= h; ++dy) {
        const int y = r + dy < 0 ? 0 : (r + dy > H - 1 ? H - 1 : r + dy);
        for (int dx = -h; dx <= h; ++dx) {
            const int x = c + dx < 0 ? 0 : (c + dx > W - 1 ? W - 1 : c + dx);
            const uint8_t* px = img + 3 * ((size_t)y * W + x);
            ref[0] += px[0]; ref[1] += px[1]; ref[2] += px[2];
        }
    }
}

// match(p, s): px = the pixel's three bytes, n2 = n * n, reach = n2 * tolerance.
GGC_WAND_HD bool wand_match(const uint8_t* px, const int32_t ref[3], int n2, int reach) {
    for (int c = 0; c < 3; ++c) {
        const int d = n2 * (int)px[c] - ref[c];
        if (d > reach || -d > reach) return false;
    }
    return true;
}

} // namespace ggc
