// ggc_image.h — the small pixel helpers that the trimap filter, the mattes, the foreground and the full-size cut share.
// The library is built without contraction, so each expression below rounds exactly as it is written.
#pragma once
#include "ggc_internal.h"

namespace ggc {

// BORDER_REFLECT_101: index i of a row of n reflected into [0, n)
__device__ __forceinline__ int refl101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) { if (i < 0) i = -i; if (i >= n) i = 2 * n - 2 - i; }
    return i;
}

// the half-pixel-centre source coordinate of output index o of n1, over a source of n (cv2.INTER_LINEAR, align_corners=False)
__device__ __forceinline__ void half_pixel_coord(int o, int n, int n1, int& i0, int& i1, double& w) {
    double s = (((double)o + 0.5) * (double)n) / (double)n1 - 0.5;
    if (s < 0.0) s = 0.0;
    const double f = floor(s);
    i0 = (int)f;
    if (i0 >= n - 1) { i0 = n - 1; w = 0.0; } else { w = s - f; }
    i1 = min(i0 + 1, n - 1);
}

__device__ __forceinline__ double lerp(double u, double v, double t) { return u + t * (v - u); }

// a clamped to [0, 1]; a NaN reads as 0
__device__ __forceinline__ double unit_clamp(float a) {
    const double v = (double)a;
    return !(v >= 0.0) ? 0.0 : (v > 1.0 ? 1.0 : v);
}

// floor(255 clamp(v, 0, 1) + 0.5); a NaN gives 0
__device__ __forceinline__ uint8_t unit_byte(double v) {
    const double c = v > 0.0 ? (v > 1.0 ? 1.0 : v) : 0.0;
    return (uint8_t)floor(255.0 * c + 0.5);
}

} // namespace ggc
