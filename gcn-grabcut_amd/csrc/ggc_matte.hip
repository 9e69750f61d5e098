// ggc_matte.hip — O1: soft alpha matte of a binary mask by guided-filter feathering (He, Sun and Tang, "Guided Image
// Filtering", ECCV 2010 / TPAMI 2013), with the colour image I = bgr / 255 as guide and the mask p in {0,1} as input:
//
//   stage 1, per window k:  a_k = (Sigma_k + eps U)^-1 cov_k(I, p),   b_k = mean_k(p) - a_k . mean_k(I)
//   stage 2, per pixel i:   alpha_i = clamp(mean_{k containing i}(a_k) . I_i + mean_{k containing i}(b_k), 0, 1)
//
// Windows are (2r+1)^2 with BORDER_REFLECT_101 (every window has n = (2r+1)^2 taps, also when it is larger than the
// image).
//
// Stage 1 is exact: the 13 window sums (B, G, R, the six products of two channels, p, and the three channel * p) are
// integers, kept in uint32 (the largest, 255^2 * n, is below 2^31 for r <= 64).  The centred moments n * S_jk - S_j * S_k
// are formed in int64 and only then scaled by 1 / (255^2 n^2), so the covariances carry no cancellation error and do
// not depend on the order of the sums: running sums (add the row entering the window, subtract the row leaving it) give
// exactly what direct sums give.  The 3x3 solve (adjugate) and the final combination run in float64.
//
// Stage 2 is exact as well: stage 1 rounds a and b to int64 fixed point, q = rint(v * 2^S), with S chosen per call so
// that no window sum of q can overflow: ||a|| <= sigma_p / (2 sqrt(eps)) <= 0.25 / sqrt(eps) (in the eigenbasis of
// Sigma, a_i = c_i / (lambda_i + eps) with sum c_i^2 / lambda_i <= var p) and |b| <= 1 + sqrt(3) ||a||, so
// n * 2 * (1 + 0.5 / sqrt(eps)) * 2^S < 2^62 holds with S = floor(62 - log2(that)), at most 52.  For 1e-12 <= eps this
// gives S >= 28, a rounding of at most 2^-29 per value.  The window sums of q are then exact integers, so a pixel whose
// windows all see one mask value gets exactly that value, and the running sums below equal direct sums.
//
// Both stages share one layout: a block is one wave that owns 64 output columns and 64 output rows of one image.  Each
// lane owns one output column and keeps its window sums in registers while the block walks down its rows; per row the
// wave stages the entering and the leaving input row (64 + 2r reflected columns) in LDS, and each lane sums its 2r+1
// horizontal taps of both.  Stage 1 writes q(a), q(b) as 4 int64 per pixel to the context's scratch; stage 2 reads them
// back with the same walk.  Every pixel's result depends only on its own image and its position, not on the batch: a
// batch equals its single-image calls bit for bit.  No atomics.
#include "ggc_image.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int MT_W = 64;                    // output columns of a block (one wave, one lane per column)
constexpr int MT_H = 64;                    // output rows of a block
constexpr int MT_RMAX = 64;
constexpr int MT_IW = MT_W + 2 * MT_RMAX;   // staged columns at the largest radius
constexpr int MT_CPL = MT_IW / MT_W;        // staged columns per lane (3)

struct alignas(32) MatteAB { int64_t a0, a1, a2, b; };   // fixed point, scale 2^S
struct alignas(32) MatteMean { double c0, c1, c2, c3; };  // mean coefficients of a pixel (stage 2')

// the reflected image column of each staged column a lane loads (-1: past the staged width).  Columns beyond W - 1 + r
// are only read by outputs outside the image, which are never written; clamping them first keeps refl101 short.
__device__ __forceinline__ void staged_columns(int lane, int x0, int r, int W, int (&gx)[MT_CPL]) {
    const int iw = MT_W + 2 * r;
#pragma unroll
    for (int j = 0; j < MT_CPL; ++j) {
        const int c = lane + MT_W * j;
        gx[j] = c < iw ? refl101(min(x0 - r + c, W - 1 + r), W) : -1;
    }
}

// one image row, packed b | g << 8 | r << 16 | (mask != 0) << 24 per staged column
__device__ __forceinline__ void stage_pixels(const uint8_t* __restrict__ im, const uint8_t* __restrict__ mk, int W, int gy,
                                             int lane, const int (&gx)[MT_CPL], uint32_t* __restrict__ dst) {
    const uint8_t* prow = im + (size_t)gy * W * 3;
    const uint8_t* mrow = mk + (size_t)gy * W;
#pragma unroll
    for (int j = 0; j < MT_CPL; ++j) {
        const int x = gx[j];
        if (x < 0) continue;
        dst[lane + MT_W * j] = (uint32_t)prow[3 * x] | ((uint32_t)prow[3 * x + 1] << 8) | ((uint32_t)prow[3 * x + 2] << 16) |
                               ((mrow[x] != 0 ? 1u : 0u) << 24);
    }
}

// the 13 integer moments of the 2r+1 staged pixels starting at column `lane`
__device__ __forceinline__ void row_moments(const uint32_t* __restrict__ row, int lane, int r, uint32_t (&s)[13]) {
#pragma unroll
    for (int k = 0; k < 13; ++k) s[k] = 0;
    for (int t = 0; t <= 2 * r; ++t) {
        const uint32_t v = row[lane + t];
        const uint32_t b = v & 255u, g = (v >> 8) & 255u, rr = (v >> 16) & 255u, m = v >> 24;
        s[0] += b; s[1] += g; s[2] += rr;
        s[3] += b * b; s[4] += b * g; s[5] += b * rr; s[6] += g * g; s[7] += g * rr; s[8] += rr * rr;
        s[9] += m; s[10] += b * m; s[11] += g * m; s[12] += rr * m;
    }
}

__device__ __forceinline__ double centred(int64_t n, uint32_t sjk, uint32_t sj, uint32_t sk) {
    return (double)(n * (int64_t)sjk - (int64_t)sj * (int64_t)sk);
}

// qmax = 2^62 / n: no window sum of n values can overflow.  Unreachable within the bound on a and b; keeps llrint defined.
__device__ __forceinline__ int64_t quantise(double v, double scale, double qmax) {
    v *= scale;
    v = v < -qmax ? -qmax : (v > qmax ? qmax : v);
    return llrint(v);
}

// a = (Sigma + eps U)^-1 c by the adjugate, b = mean p - a . mean I, in fixed point; s = the 13 window sums
__device__ __forceinline__ MatteAB solve_ab(const uint32_t (&s)[13], int64_t n, double eps, double scale) {
    const double qmax = 4611686018427387904.0 / (double)n;
    const double nn = (double)n * (double)n;
    const double dii = 65025.0 * nn, dip = 255.0 * nn;
    const double m00 = centred(n, s[3], s[0], s[0]) / dii + eps;
    const double m01 = centred(n, s[4], s[0], s[1]) / dii;
    const double m02 = centred(n, s[5], s[0], s[2]) / dii;
    const double m11 = centred(n, s[6], s[1], s[1]) / dii + eps;
    const double m12 = centred(n, s[7], s[1], s[2]) / dii;
    const double m22 = centred(n, s[8], s[2], s[2]) / dii + eps;
    const double v0 = centred(n, s[10], s[0], s[9]) / dip;
    const double v1 = centred(n, s[11], s[1], s[9]) / dip;
    const double v2 = centred(n, s[12], s[2], s[9]) / dip;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    const double a0 = (c00 * v0 + c01 * v1 + c02 * v2) / det;
    const double a1 = (c01 * v0 + c11 * v1 + c12 * v2) / det;
    const double a2 = (c02 * v0 + c12 * v1 + c22 * v2) / det;
    const double dn = 255.0 * (double)n;
    const double b = (double)s[9] / (double)n - (a0 * ((double)s[0] / dn) + a1 * ((double)s[1] / dn) + a2 * ((double)s[2] / dn));
    return MatteAB{quantise(a0, scale, qmax), quantise(a1, scale, qmax), quantise(a2, scale, qmax), quantise(b, scale, qmax)};
}

// stage 1: grid (cdiv(W, 64), cdiv(H, 64), B), 64 threads
__global__ void __launch_bounds__(MT_W) k_matte_ab(int H, int W, int r, double eps, double scale, const uint8_t* __restrict__ bgr,
                                                   const uint8_t* __restrict__ binary, MatteAB* __restrict__ ab) {
    __shared__ uint32_t s_in[MT_IW], s_out[MT_IW];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H, y1 = min(y0 + MT_H, H);
    const size_t P = (size_t)H * W;
    const uint8_t* im = bgr + (size_t)blockIdx.z * P * 3;
    const uint8_t* mk = binary + (size_t)blockIdx.z * P;
    MatteAB* dst = ab + (size_t)blockIdx.z * P;
    const int x = x0 + lane;
    const int64_t n = (int64_t)(2 * r + 1) * (2 * r + 1);
    int gx[MT_CPL];
    staged_columns(lane, x0, r, W, gx);
    uint32_t acc[13], tin[13], tout[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0;
    for (int dy = -r; dy <= r; ++dy) {          // the first row's window, row by row
        stage_pixels(im, mk, W, refl101(y0 + dy, H), lane, gx, s_in);
        __syncthreads();
        row_moments(s_in, lane, r, tin);
#pragma unroll
        for (int k = 0; k < 13; ++k) acc[k] += tin[k];
        __syncthreads();
    }
    for (int y = y0; y < y1; ++y) {
        if (y > y0) {                           // slide: row y + r enters, row y - 1 - r leaves (exact in uint32)
            stage_pixels(im, mk, W, refl101(y + r, H), lane, gx, s_in);
            stage_pixels(im, mk, W, refl101(y - 1 - r, H), lane, gx, s_out);
            __syncthreads();
            row_moments(s_in, lane, r, tin);
            row_moments(s_out, lane, r, tout);
#pragma unroll
            for (int k = 0; k < 13; ++k) acc[k] += tin[k] - tout[k];
            __syncthreads();
        }
        if (x < W) dst[(size_t)y * W + x] = solve_ab(acc, n, eps, scale);
    }
}

__device__ __forceinline__ void stage_ab(const MatteAB* __restrict__ ab, int W, int gy, int lane, const int (&gx)[MT_CPL],
                                         MatteAB* __restrict__ dst) {
    const MatteAB* row = ab + (size_t)gy * W;
#pragma unroll
    for (int j = 0; j < MT_CPL; ++j)
        if (gx[j] >= 0) dst[lane + MT_W * j] = row[gx[j]];
}

__device__ __forceinline__ void row_sum_ab(const MatteAB* __restrict__ row, int lane, int r, uint64_t (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = 0;
    for (int t = 0; t <= 2 * r; ++t) {
        const MatteAB v = row[lane + t];
        s[0] += (uint64_t)v.a0; s[1] += (uint64_t)v.a1; s[2] += (uint64_t)v.a2; s[3] += (uint64_t)v.b;
    }
}

// alpha = clamp(c0 B + c1 G + c2 R + c3, 0, 1), summed left to right: the one definition stages 2 and 3 share
__device__ __forceinline__ double matte_value(double c0, double c1, double c2, double c3, uint8_t pb, uint8_t pg, uint8_t pr) {
    const double a = c0 * (double)pb + c1 * (double)pg + c2 * (double)pr + c3;
    return a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
}

// stage 2: same grid.  MEAN = false: alpha [B,H,W] f32 and / or rgba [B,H,W,4] u8 (either may be NULL).  MEAN = true
// (stage 2' of ggc_upsample_matte): the per-pixel mean coefficients C = (acc0 / dn, acc1 / dn, acc2 / dn, acc3 / db)
// that the alpha of the other form is made of, to `mean` [B,H,W].
template <bool MEAN>
__global__ void __launch_bounds__(MT_W) k_matte_alpha(int H, int W, int r, double scale, const uint8_t* __restrict__ bgr,
                                                      const MatteAB* __restrict__ ab, float* __restrict__ alpha,
                                                      uint8_t* __restrict__ rgba, MatteMean* __restrict__ mean) {
    __shared__ MatteAB s_in[MT_IW], s_out[MT_IW];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H, y1 = min(y0 + MT_H, H);
    const size_t P = (size_t)H * W;
    const size_t base = (size_t)blockIdx.z * P;
    const MatteAB* src = ab + base;
    const int x = x0 + lane;
    const double n = (double)(2 * r + 1) * (double)(2 * r + 1);
    int gx[MT_CPL];
    staged_columns(lane, x0, r, W, gx);
    uint64_t acc[4] = {0, 0, 0, 0}, tin[4], tout[4];      // window sums of q, exact modulo 2^64 (the true sums fit int64)
    for (int dy = -r; dy <= r; ++dy) {
        stage_ab(src, W, refl101(y0 + dy, H), lane, gx, s_in);
        __syncthreads();
        row_sum_ab(s_in, lane, r, tin);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += tin[k];
        __syncthreads();
    }
    for (int y = y0; y < y1; ++y) {
        if (y > y0) {
            stage_ab(src, W, refl101(y + r, H), lane, gx, s_in);
            stage_ab(src, W, refl101(y - 1 - r, H), lane, gx, s_out);
            __syncthreads();
            row_sum_ab(s_in, lane, r, tin);
            row_sum_ab(s_out, lane, r, tout);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += tin[k] - tout[k];
            __syncthreads();
        }
        if (x < W) {
            const size_t i = base + (size_t)y * W + x;
            const double dn = 255.0 * n * scale, db = n * scale;
            const double c0 = (double)(int64_t)acc[0] / dn, c1 = (double)(int64_t)acc[1] / dn;
            const double c2 = (double)(int64_t)acc[2] / dn, c3 = (double)(int64_t)acc[3] / db;
            if constexpr (MEAN) {
                mean[i] = MatteMean{c0, c1, c2, c3};
            } else {
                const uint8_t pb = bgr[3 * i], pg = bgr[3 * i + 1], pr = bgr[3 * i + 2];
                const double a = matte_value(c0, c1, c2, c3, pb, pg, pr);
                if (alpha) alpha[i] = (float)a;
                if (rgba) {
                    rgba[4 * i] = pb; rgba[4 * i + 1] = pg; rgba[4 * i + 2] = pr;
                    rgba[4 * i + 3] = unit_byte(a);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- stage 3 of ggc_upsample_matte
// One pass over the full-resolution pixels.  A block is 256 lanes x 4 consecutive output columns (1024) and UP_H output
// rows of one image; it walks down its rows.  Each lane maps its 4 columns to (x0, x1, wx) once, and keeps the horizontal
// lerps of the two source rows its current output row reads (h0: row y0, h1: row y1, 4 coefficients x 4 pixels each) in
// registers: consecutive output rows mostly share them, and when y0 moves on by one row h1 becomes h0, so a source row's
// lerps are formed once per block.  The source coefficients are read through the cache (a block's window of the 32 B/px
// plane is small); the colour bytes and every output are streamed once, coalesced.  VEC (W1 % 4 == 0 and aligned
// pointers): 12 B of BGR in, 16 B of alpha, 4 B of mask and 16 B of BGRA out per lane and row, as single wide accesses.
constexpr int UP_PX = 4;                    // output columns per lane
constexpr int UP_THREADS = 256;
constexpr int UP_W = UP_PX * UP_THREADS;    // output columns of a block
constexpr int UP_H = 32;                    // output rows of a block

// the horizontal lerps of source row `row` at the lane's UP_PX columns
__device__ __forceinline__ void up_row(const MatteMean* __restrict__ row, const int (&x0)[UP_PX], const int (&x1)[UP_PX],
                                       const double (&wx)[UP_PX], double (&h)[UP_PX][4]) {
#pragma unroll
    for (int j = 0; j < UP_PX; ++j) {
        const MatteMean u = row[x0[j]], v = row[x1[j]];
        h[j][0] = lerp(u.c0, v.c0, wx[j]);
        h[j][1] = lerp(u.c1, v.c1, wx[j]);
        h[j][2] = lerp(u.c2, v.c2, wx[j]);
        h[j][3] = lerp(u.c3, v.c3, wx[j]);
    }
}

// grid (cdiv(W1, UP_W), cdiv(H1, UP_H), B), UP_THREADS threads; alpha [B,H1,W1] f32, binary [B,H1,W1] u8 and rgba
// [B,H1,W1,4] u8, each may be NULL
template <bool VEC>
__global__ void __launch_bounds__(UP_THREADS) k_upsample(int H, int W, int H1, int W1, const MatteMean* __restrict__ mean,
                                                         const uint8_t* __restrict__ bgr, float* __restrict__ alpha,
                                                         uint8_t* __restrict__ binary, uint8_t* __restrict__ rgba) {
    const int xb = (blockIdx.x * UP_THREADS + threadIdx.x) * UP_PX;
    if (xb >= W1) return;                       // no barrier below: idle lanes may leave
    const int yb = blockIdx.y * UP_H, ye = min(yb + UP_H, H1);
    const MatteMean* src = mean + (size_t)blockIdx.z * H * W;
    int x0[UP_PX], x1[UP_PX];
    double wx[UP_PX];
#pragma unroll
    for (int j = 0; j < UP_PX; ++j) half_pixel_coord(min(xb + j, W1 - 1), W, W1, x0[j], x1[j], wx[j]);
    double h0[UP_PX][4], h1[UP_PX][4];
    int ra = -1, rb = -1;                       // the source rows h0 and h1 hold
    for (int y = yb; y < ye; ++y) {
        int y0, y1;
        double wy;
        half_pixel_coord(y, H, H1, y0, y1, wy);
        if (y0 != ra) {
            if (y0 == rb) {
#pragma unroll
                for (int j = 0; j < UP_PX; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) h0[j][k] = h1[j][k];
            } else {
                up_row(src + (size_t)y0 * W, x0, x1, wx, h0);
            }
            ra = y0;
        }
        if (y1 != rb) {
            if (y1 == ra) {
#pragma unroll
                for (int j = 0; j < UP_PX; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) h1[j][k] = h0[j][k];
            } else {
                up_row(src + (size_t)y1 * W, x0, x1, wx, h1);
            }
            rb = y1;
        }
        const size_t p = ((size_t)blockIdx.z * H1 + y) * W1 + xb;
        uint8_t px[3 * UP_PX];
        if constexpr (VEC) {
            const uint32_t* s32 = reinterpret_cast<const uint32_t*>(bgr + 3 * p);
            const uint32_t w0 = s32[0], w1 = s32[1], w2 = s32[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                px[k] = (uint8_t)(w0 >> (8 * k));
                px[4 + k] = (uint8_t)(w1 >> (8 * k));
                px[8 + k] = (uint8_t)(w2 >> (8 * k));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * UP_PX; ++k) px[k] = xb + k / 3 < W1 ? bgr[3 * p + k] : 0;
        }
        double a[UP_PX];
#pragma unroll
        for (int j = 0; j < UP_PX; ++j)
            a[j] = matte_value(lerp(h0[j][0], h1[j][0], wy), lerp(h0[j][1], h1[j][1], wy), lerp(h0[j][2], h1[j][2], wy),
                               lerp(h0[j][3], h1[j][3], wy), px[3 * j], px[3 * j + 1], px[3 * j + 2]);
        if constexpr (VEC) {
            if (alpha)
                *reinterpret_cast<float4*>(alpha + p) = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
            if (binary) {
                uint32_t m = 0;
#pragma unroll
                for (int j = 0; j < UP_PX; ++j) m |= (a[j] >= 0.5 ? 1u : 0u) << (8 * j);
                *reinterpret_cast<uint32_t*>(binary + p) = m;
            }
            if (rgba) {
                uint32_t q[UP_PX];
#pragma unroll
                for (int j = 0; j < UP_PX; ++j)
                    q[j] = (uint32_t)px[3 * j] | ((uint32_t)px[3 * j + 1] << 8) | ((uint32_t)px[3 * j + 2] << 16) |
                           ((uint32_t)unit_byte(a[j]) << 24);
                *reinterpret_cast<uint4*>(rgba + 4 * p) = make_uint4(q[0], q[1], q[2], q[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < UP_PX; ++j) {
                if (xb + j >= W1) break;
                const size_t i = p + j;
                if (alpha) alpha[i] = (float)a[j];
                if (binary) binary[i] = a[j] >= 0.5 ? 1 : 0;
                if (rgba) {
                    rgba[4 * i] = px[3 * j]; rgba[4 * i + 1] = px[3 * j + 1]; rgba[4 * i + 2] = px[3 * j + 2];
                    rgba[4 * i + 3] = unit_byte(a[j]);
                }
            }
        }
    }
}

} // namespace
} // namespace ggc

using namespace ggc;

namespace {

// the argument checks ggc_alpha_matte and ggc_upsample_matte share, and the fixed-point scale 2^S of stage 1
int check_matte(ggc_ctx* ctx, int radius, float eps) {
    GGC_REQUIRE(ctx, radius >= 1 && radius <= MT_RMAX, GGC_E_INVALID_ARG, "matte radius %d outside 1..%d", radius, MT_RMAX);
    GGC_REQUIRE(ctx, eps >= 1e-12f && std::isfinite(eps), GGC_E_INVALID_ARG, "matte eps %g outside [1e-12, inf)", (double)eps);
    return GGC_OK;
}

double matte_scale(int radius, float eps) {
    const double n = (double)(2 * radius + 1) * (double)(2 * radius + 1);
    const int S = std::max(0, std::min(52, (int)std::floor(62.0 - std::log2(n * 2.0 * (1.0 + 0.5 / std::sqrt((double)eps))))));
    return std::ldexp(1.0, S);
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

} // namespace

extern "C" int ggc_alpha_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                               const uint8_t* binary, int radius, float eps, float* alpha, uint8_t* rgba) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, bgr && binary && (alpha || rgba), GGC_E_INVALID_ARG, "null pointer");
    if (int e = check_matte(ctx, radius, eps)) return e;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MatteAB* ab = scratch_t<MatteAB>(ctx, S_MATTE, (size_t)B * H * W);
    if (!ab) return GGC_E_OOM;
    ProfScope prof(ctx, st, "alpha_matte");
    const double scale = matte_scale(radius, eps);
    const dim3 grid(cdiv(W, MT_W), cdiv(H, MT_H), B);
    hipLaunchKernelGGL(k_matte_ab, grid, dim3(MT_W), 0, st, H, W, radius, (double)eps, scale, bgr, binary, ab);
    hipLaunchKernelGGL(k_matte_alpha<false>, grid, dim3(MT_W), 0, st, H, W, radius, scale, bgr, ab, alpha, rgba,
                       (MatteMean*)nullptr);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

extern "C" int ggc_upsample_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                                  const uint8_t* binary, int H1, int W1, const uint8_t* bgr_full, int radius, float eps,
                                  float* alpha_full, uint8_t* binary_full, uint8_t* rgba_full) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H1 >= H && W1 >= W && H1 <= 32768 && W1 <= 32768,
                GGC_E_SHAPE, "bad shape B=%d H=%d W=%d -> H1=%d W1=%d", B, H, W, H1, W1);
    GGC_REQUIRE(ctx, bgr && binary && bgr_full && (alpha_full || binary_full || rgba_full), GGC_E_INVALID_ARG, "null pointer");
    if (int e = check_matte(ctx, radius, eps)) return e;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MatteAB* ab = scratch_t<MatteAB>(ctx, S_MATTE, (size_t)B * H * W);
    if (!ab) return GGC_E_OOM;
    MatteMean* mean = scratch_t<MatteMean>(ctx, S_MATTE_MEAN, (size_t)B * H * W);
    if (!mean) return GGC_E_OOM;
    ProfScope prof(ctx, st, "upsample_matte");
    const double scale = matte_scale(radius, eps);
    const dim3 grid(cdiv(W, MT_W), cdiv(H, MT_H), B);
    hipLaunchKernelGGL(k_matte_ab, grid, dim3(MT_W), 0, st, H, W, radius, (double)eps, scale, bgr, binary, ab);
    hipLaunchKernelGGL(k_matte_alpha<true>, grid, dim3(MT_W), 0, st, H, W, radius, scale, bgr, ab, (float*)nullptr,
                       (uint8_t*)nullptr, mean);
    const bool vec = W1 % UP_PX == 0 && aligned(bgr_full, 4) && aligned(alpha_full, 16) && aligned(binary_full, 4) &&
                     aligned(rgba_full, 16);
    const dim3 up_grid(cdiv(W1, UP_W), cdiv(H1, UP_H), B);
    if (vec)
        hipLaunchKernelGGL(k_upsample<true>, up_grid, dim3(UP_THREADS), 0, st, H, W, H1, W1, mean, bgr_full, alpha_full,
                           binary_full, rgba_full);
    else
        hipLaunchKernelGGL(k_upsample<false>, up_grid, dim3(UP_THREADS), 0, st, H, W, H1, W1, mean, bgr_full, alpha_full,
                           binary_full, rgba_full);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
