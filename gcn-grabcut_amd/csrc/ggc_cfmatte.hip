// ggc_cfmatte.hip — O3, O3t: closed-form alpha matte (Levin, Lischinski and Weiss, TPAMI 2008) of a binary mask or of a
// caller's trimap, solved on the device by Jacobi-preconditioned conjugate gradients with the matting Laplacian applied
// without a matrix (He, Sun and Tang, CVPR 2010).  include/ggc.h states the systems; DESIGN.md §5.13 the tiling and the
// bytes, §5.16 the trimap entry.
//
// One solver, two front ends.  A front end says which pixels are unknown (U), what the known ones are and where the
// unknown ones start: it writes the flag plane (F_M = the known value, F_U = unknown), the start x on U, and the
// number of U pixels of every tile.  ggc_closed_form_matte's is the band around the mask's edge, started at the mask
// (k_cf_edge, k_cf_dilate_h, k_cf_dilate_v); ggc_trimap_matte's reads the trimap's bytes and the caller's start
// (k_cf_trimap).  Everything after that (cf_solve) is shared.  ggc_trimap_matte_warm is the trimap front end with a
// second stop reference: the residual of the 0.5 start, one more application of L in the set-up.
// ggc_lift_trimap and ggc_closed_form_band solve nothing: they write trimaps (a working-size trimap and alpha carried to
// a larger size; the band of the mask front end as a trimap) with the band front end's separable dilation.
//
// Layout.  The tile list, the fixed-order sums, the per-image scalars and the poll are ggc_cg.h's.  Listed here are the
// tiles that hold U or touch a tile that does (ring 1: every window centre within r <= 16 of U); an image whose U is
// empty or covers every pixel is not solved.  The vectors are full-frame float64 planes.  Per listed tile and iteration:
//   k_cf_window  a_k, b_k of the p of the product at every centre k in K of the tile (p staged with an r halo in LDS)
//   k_cf_pixel   (L p)_i = c_i p_i - sum_k (a_k . I_i + b_k) on U (a, b staged with an r halo in LDS); per-tile d . q
//   k_cg_scalar  per image: alpha = rz / (d . q)
//   k_cf_update  x += alpha d, r -= alpha q on U; per-tile r . z and r . r (z = r / diag L)
//   k_cg_scalar  per image: convergence (rel = sqrt(r.r / rr0) <= tol), the iteration count, beta
//   k_cf_direction  d = z + beta d on U
// The window statistics (mu_k and Delta_k^-1 from exact integer window sums, the 3x3 inverse by the adjugate in float64)
// and diag L are computed once per call.
#include "ggc_cg.h"
#include "ggc_image.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int CF_T = CG_T, CF_THREADS = CG_THREADS;
constexpr int CF_RMAX = 8;
constexpr int CF_SMAX = CF_T + 2 * CF_RMAX;       // staged side at the largest radius

constexpr uint8_t F_M = 1, F_U = 2;               // flags: known value (meaningful off U), unknown

struct alignas(8) CfStats { double mu[3]; double d00, d01, d02, d11, d12, d22; };   // Delta^-1, symmetric
struct alignas(32) CfAB { double a0, a1, a2, b; };

__device__ __forceinline__ double colour(const uint8_t* px, int c) { return (double)px[c] * (1.0 / 255.0); }

// ---------------------------------------------------------------- front end of the mask: the band, over the whole frame
// grid (cdiv(W, 16), cdiv(H, 16), B), 16 x 16 threads
__global__ void __launch_bounds__(CF_THREADS) k_cf_edge(int H, int W, const uint8_t* __restrict__ binary,
                                                        uint8_t* __restrict__ edge) {
    const int x = blockIdx.x * CF_T + threadIdx.x, y = blockIdx.y * CF_T + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint8_t* m = binary + (size_t)blockIdx.z * H * W;
    bool lo = true, hi = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const bool v = m[(size_t)yy * W + xx] != 0;
            lo = lo && v;
            hi = hi || v;
        }
    edge[(size_t)blockIdx.z * H * W + (size_t)y * W + x] = hi && !lo ? 1 : 0;
}

__global__ void __launch_bounds__(CF_THREADS) k_cf_dilate_h(int H, int W, int band, const uint8_t* __restrict__ edge,
                                                            uint8_t* __restrict__ out) {
    const int x = blockIdx.x * CF_T + threadIdx.x, y = blockIdx.y * CF_T + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint8_t* row = edge + (size_t)blockIdx.z * H * W + (size_t)y * W;
    uint8_t v = 0;
    for (int xx = max(0, x - band); xx <= min(W - 1, x + band); ++xx) v |= row[xx];
    out[(size_t)blockIdx.z * H * W + (size_t)y * W + x] = v;
}

// flags = m | U << 1; start = m on U; tile_u [B, tiles] = pixels of U in each tile (a block is a tile)
__global__ void __launch_bounds__(CF_THREADS) k_cf_dilate_v(int H, int W, int band, const uint8_t* __restrict__ hdil,
                                                            const uint8_t* __restrict__ binary, uint8_t* __restrict__ flags,
                                                            double* __restrict__ start, int32_t* __restrict__ tile_u) {
    __shared__ int s_cnt[CF_THREADS];
    const int tid = threadIdx.y * CF_T + threadIdx.x;
    const int x = blockIdx.x * CF_T + threadIdx.x, y = blockIdx.y * CF_T + threadIdx.y;
    const size_t base = (size_t)blockIdx.z * H * W;
    int u = 0;
    if (x < W && y < H) {
        uint8_t v = 0;
        for (int yy = max(0, y - band); yy <= min(H - 1, y + band); ++yy) v |= hdil[base + (size_t)yy * W + x];
        const size_t i = base + (size_t)y * W + x;
        const bool m = binary[i] != 0;
        flags[i] = (m ? F_M : 0) | (v ? F_U : 0);
        if (v) start[i] = m ? 1.0 : 0.0;
        u = v ? 1 : 0;
    }
    count_tile(u, s_cnt, tid, tile_u);
}

// ---------------------------------------------------------------- front end of the trimap, over the whole frame
// 255 is foreground, 0 background, every other byte unknown.  flags as above; the start x on U = alpha0 clamped to
// [0, 1] (a NaN reads as 0), or 0.5 without alpha0; tile_u as above
__global__ void __launch_bounds__(CF_THREADS) k_cf_trimap(int H, int W, const uint8_t* __restrict__ trimap,
                                                          const float* __restrict__ alpha0, uint8_t* __restrict__ flags,
                                                          double* __restrict__ x, int32_t* __restrict__ tile_u) {
    __shared__ int s_cnt[CF_THREADS];
    const int tid = threadIdx.y * CF_T + threadIdx.x;
    const int xp = blockIdx.x * CF_T + threadIdx.x, yp = blockIdx.y * CF_T + threadIdx.y;
    int u = 0;
    if (xp < W && yp < H) {
        const size_t i = (size_t)blockIdx.z * H * W + (size_t)yp * W + xp;
        const uint8_t t = trimap[i];
        u = t != 0 && t != 255 ? 1 : 0;
        flags[i] = (t == 255 ? F_M : 0) | (u ? F_U : 0);
        if (u) x[i] = alpha0 ? unit_clamp(alpha0[i]) : 0.5;
    }
    count_tile(u, s_cnt, tid, tile_u);
}

// ---------------------------------------------------------------- trimaps for a later solve, over the whole frame
// One output pixel per thread, grid (cdiv(W1, 16), cdiv(H1, 16), B).  trimap_full = 255 / 0 where the source pixels of
// nonzero weight all are, else 128 (unknown = that as a 0 / 1 plane, for the dilation); alpha0_full = the bilinear
// interpolation of the clamped alpha.  Each output may be NULL.
__global__ void __launch_bounds__(CF_THREADS) k_cf_lift(int H, int W, int H1, int W1, const uint8_t* __restrict__ trimap,
                                                        const float* __restrict__ alpha, uint8_t* __restrict__ trimap_full,
                                                        uint8_t* __restrict__ unknown, float* __restrict__ alpha0_full) {
    const int x = blockIdx.x * CF_T + threadIdx.x, y = blockIdx.y * CF_T + threadIdx.y;
    if (x >= W1 || y >= H1) return;
    int x0, x1, y0, y1;
    double wx, wy;
    half_pixel_coord(x, W, W1, x0, x1, wx);
    half_pixel_coord(y, H, H1, y0, y1, wy);
    const size_t src = (size_t)blockIdx.z * H * W, o = (size_t)blockIdx.z * H1 * W1 + (size_t)y * W1 + x;
    if (trimap_full) {
        const uint8_t* t = trimap + src;
        const int xb = wx > 0.0 ? x1 : x0, yb = wy > 0.0 ? y1 : y0;      // a source pixel of weight 0 does not count
        const uint8_t t00 = t[(size_t)y0 * W + x0], t01 = t[(size_t)y0 * W + xb];
        const uint8_t t10 = t[(size_t)yb * W + x0], t11 = t[(size_t)yb * W + xb];
        const uint8_t all_and = t00 & t01 & t10 & t11, all_or = t00 | t01 | t10 | t11;
        const uint8_t v = all_and == 255 ? 255 : (all_or == 0 ? 0 : 128);
        trimap_full[o] = v;
        if (unknown) unknown[o] = v == 128 ? 1 : 0;
    }
    if (alpha0_full) {
        const float* a = alpha + src;
        const double a00 = unit_clamp(a[(size_t)y0 * W + x0]), a01 = unit_clamp(a[(size_t)y0 * W + x1]);
        const double a10 = unit_clamp(a[(size_t)y1 * W + x0]), a11 = unit_clamp(a[(size_t)y1 * W + x1]);
        alpha0_full[o] = (float)lerp(lerp(a00, a01, wx), lerp(a10, a11, wx), wy);
    }
}

// the vertical half of the dilation, written as a trimap: 128 where the column of hdil within `band` holds a set byte,
// else the known value: base's own byte, with MASK 255 (base != 0).  out may be base: a thread reads its own pixel only
template <bool MASK>
__global__ void __launch_bounds__(CF_THREADS) k_cf_dilate_v_trimap(int H, int W, int band, const uint8_t* __restrict__ hdil,
                                                                   const uint8_t* base, uint8_t* out) {
    const int x = blockIdx.x * CF_T + threadIdx.x, y = blockIdx.y * CF_T + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)blockIdx.z * H * W;
    uint8_t v = 0;
    for (int yy = max(0, y - band); yy <= min(H - 1, y + band); ++yy) v |= hdil[plane + (size_t)yy * W + x];
    const size_t i = plane + (size_t)y * W + x;
    const uint8_t known = MASK ? (base[i] != 0 ? 255 : 0) : base[i];
    out[i] = v ? 128 : known;
}

// ---------------------------------------------------------------- per listed tile
// Delta_k^-1 and mu_k of every centre of the tile that lies in K, from exact integer window sums
__global__ void __launch_bounds__(CF_THREADS) k_cf_stats(int H, int W, int r, double eps, int ntx,
                                                         const int2* __restrict__ tiles, const uint8_t* __restrict__ bgr,
                                                         CfStats* __restrict__ stats) {
    const TileRef t = tile_of(tiles, ntx);
    const int x = t.tx * CF_T + threadIdx.x, y = t.ty * CF_T + threadIdx.y;
    if (x < r || x >= W - r || y < r || y >= H - r) return;       // not in K (outside the image included)
    const uint8_t* im = bgr + (size_t)t.b * H * W * 3;
    uint32_t s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int yy = y - r; yy <= y + r; ++yy)
        for (int xx = x - r; xx <= x + r; ++xx) {
            const uint8_t* px = im + ((size_t)yy * W + xx) * 3;
            const uint32_t c0 = px[0], c1 = px[1], c2 = px[2];
            s[0] += c0; s[1] += c1; s[2] += c2;
            s[3] += c0 * c0; s[4] += c0 * c1; s[5] += c0 * c2; s[6] += c1 * c1; s[7] += c1 * c2; s[8] += c2 * c2;
        }
    const int64_t n = (int64_t)(2 * r + 1) * (2 * r + 1);
    const double nn = (double)n * (double)n, dii = 65025.0 * nn, e = eps / (double)n;
    auto centred = [&](uint32_t sjk, uint32_t sj, uint32_t sk) {
        return (double)(n * (int64_t)sjk - (int64_t)sj * (int64_t)sk) / dii;
    };
    const double m00 = centred(s[3], s[0], s[0]) + e, m01 = centred(s[4], s[0], s[1]), m02 = centred(s[5], s[0], s[2]);
    const double m11 = centred(s[6], s[1], s[1]) + e, m12 = centred(s[7], s[1], s[2]), m22 = centred(s[8], s[2], s[2]) + e;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    const double dn = 255.0 * (double)n;
    CfStats st;
    st.mu[0] = (double)s[0] / dn; st.mu[1] = (double)s[1] / dn; st.mu[2] = (double)s[2] / dn;
    st.d00 = c00 / det; st.d01 = c01 / det; st.d02 = c02 / det; st.d11 = c11 / det; st.d12 = c12 / det; st.d22 = c22 / det;
    stats[(size_t)t.b * H * W + (size_t)y * W + x] = st;
}

// SETUP: p = the start image (d is x: the start on U, the known value elsewhere), with HALF the image of the stop
// reference instead (0.5 on U, d is not read); else p = d on U and 0 elsewhere
template <bool SETUP, bool HALF>
__device__ __forceinline__ double p_value(uint8_t f, const double* __restrict__ d, size_t i) {
    if constexpr (SETUP) return (f & F_U) ? (HALF ? 0.5 : d[i]) : ((f & F_M) ? 1.0 : 0.0);
    else return (f & F_U) ? d[i] : 0.0;
}

template <bool SETUP, bool HALF = false>
__global__ void __launch_bounds__(CF_THREADS) k_cf_window(int H, int W, int r, int ntx, const int2* __restrict__ tiles,
                                                          const CgImage* __restrict__ img, const uint8_t* __restrict__ bgr,
                                                          const uint8_t* __restrict__ flags, const CfStats* __restrict__ stats,
                                                          const double* __restrict__ d, CfAB* __restrict__ ab) {
    __shared__ double s_p[CF_SMAX * CF_SMAX];
    __shared__ double s_i[3][CF_SMAX * CF_SMAX];
    const TileRef t = tile_of(tiles, ntx);
    if (img[t.b].done) return;                                   // uniform over the block
    const int tid = threadIdx.y * CF_T + threadIdx.x;
    const int S = CF_T + 2 * r, x0 = t.tx * CF_T - r, y0 = t.ty * CF_T - r;
    const size_t base = (size_t)t.b * H * W;
    for (int e = tid; e < S * S; e += CF_THREADS) {
        const int yy = y0 + e / S, xx = x0 + e % S;
        double p = 0.0, i0 = 0.0, i1 = 0.0, i2 = 0.0;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const size_t i = base + (size_t)yy * W + xx;
            const double pv = p_value<SETUP, HALF>(flags[i], d, i);
            const uint8_t* px = bgr + 3 * i;
            p = pv; i0 = colour(px, 0) * pv; i1 = colour(px, 1) * pv; i2 = colour(px, 2) * pv;
        }
        s_p[e] = p; s_i[0][e] = i0; s_i[1][e] = i1; s_i[2][e] = i2;
    }
    __syncthreads();
    const int x = t.tx * CF_T + threadIdx.x, y = t.ty * CF_T + threadIdx.y;
    if (x < r || x >= W - r || y < r || y >= H - r) return;
    double sp = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int dy = 0; dy <= 2 * r; ++dy) {
        const int row = (threadIdx.y + dy) * S + threadIdx.x;
        for (int dx = 0; dx <= 2 * r; ++dx) {
            sp += s_p[row + dx]; s0 += s_i[0][row + dx]; s1 += s_i[1][row + dx]; s2 += s_i[2][row + dx];
        }
    }
    const double n = (double)(2 * r + 1) * (double)(2 * r + 1);
    const CfStats st = stats[base + (size_t)y * W + x];
    const double mp = sp / n;
    const double v0 = s0 / n - st.mu[0] * mp, v1 = s1 / n - st.mu[1] * mp, v2 = s2 / n - st.mu[2] * mp;
    const double a0 = st.d00 * v0 + st.d01 * v1 + st.d02 * v2;
    const double a1 = st.d01 * v0 + st.d11 * v1 + st.d12 * v2;
    const double a2 = st.d02 * v0 + st.d12 * v1 + st.d22 * v2;
    ab[base + (size_t)y * W + x] = CfAB{a0, a1, a2, mp - (a0 * st.mu[0] + a1 * st.mu[1] + a2 * st.mu[2])};
}

// q = (L p) on U.  SETUP: p = the start image (d is x); r = -q, diag L, and the per-tile r . z, r . r (into part_a,
// part_b); else the per-tile d . q (into part_a).  HALF (with SETUP): the same of the stop reference's image
template <bool SETUP, bool HALF = false>
__global__ void __launch_bounds__(CF_THREADS) k_cf_pixel(int H, int W, int r, int ntx, const int2* __restrict__ tiles,
                                                         const CgImage* __restrict__ img, const uint8_t* __restrict__ bgr,
                                                         const uint8_t* __restrict__ flags, const CfStats* __restrict__ stats,
                                                         const CfAB* __restrict__ ab, const double* __restrict__ d,
                                                         double* __restrict__ q, double* __restrict__ res,
                                                         double* __restrict__ diag, double* __restrict__ part_a,
                                                         double* __restrict__ part_b) {
    __shared__ CfAB s_ab[CF_SMAX * CF_SMAX];
    __shared__ double s_red[CF_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    if (img[t.b].done) return;
    const int tid = threadIdx.y * CF_T + threadIdx.x;
    const int S = CF_T + 2 * r, x0 = t.tx * CF_T - r, y0 = t.ty * CF_T - r;
    const size_t base = (size_t)t.b * H * W;
    for (int e = tid; e < S * S; e += CF_THREADS) {              // centres outside K are staged as 0 and skipped below
        const int yy = y0 + e / S, xx = x0 + e % S;
        const bool in_k = yy >= r && yy < H - r && xx >= r && xx < W - r;
        s_ab[e] = in_k ? ab[base + (size_t)yy * W + xx] : CfAB{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    const int xp = t.tx * CF_T + threadIdx.x, yp = t.ty * CF_T + threadIdx.y;
    double va = 0.0, vb = 0.0;
    if (xp < W && yp < H) {
        const size_t i = base + (size_t)yp * W + xp;
        const uint8_t f = flags[i];
        if (f & F_U) {
            const uint8_t* px = bgr + 3 * i;
            const double I0 = colour(px, 0), I1 = colour(px, 1), I2 = colour(px, 2);
            const int ky0 = max(yp - r, r), ky1 = min(yp + r, H - 1 - r), kx0 = max(xp - r, r), kx1 = min(xp + r, W - 1 - r);
            double acc = 0.0;
            for (int ky = ky0; ky <= ky1; ++ky)
                for (int kx = kx0; kx <= kx1; ++kx) {
                    const CfAB c = s_ab[(ky - y0) * S + (kx - x0)];
                    acc += c.a0 * I0 + c.a1 * I1 + c.a2 * I2 + c.b;
                }
            const double cnt = (double)((ky1 - ky0 + 1) * (kx1 - kx0 + 1));
            const double pi = p_value<SETUP, HALF>(f, d, i);
            const double qi = cnt * pi - acc;
            if constexpr (SETUP) {
                // diag L = sum_k [1 - (1 + (I_i - mu_k)^T Delta_k^-1 (I_i - mu_k)) / n]
                const double n = (double)(2 * r + 1) * (double)(2 * r + 1);
                double quad = 0.0;
                for (int ky = ky0; ky <= ky1; ++ky)
                    for (int kx = kx0; kx <= kx1; ++kx) {
                        const CfStats st = stats[base + (size_t)ky * W + kx];
                        const double e0 = I0 - st.mu[0], e1 = I1 - st.mu[1], e2 = I2 - st.mu[2];
                        quad += e0 * (st.d00 * e0 + st.d01 * e1 + st.d02 * e2) + e1 * (st.d01 * e0 + st.d11 * e1 + st.d12 * e2) +
                                e2 * (st.d02 * e0 + st.d12 * e1 + st.d22 * e2);
                    }
                const double dg = cnt * (1.0 - 1.0 / n) - quad / n;
                const double ri = -qi;
                diag[i] = dg;
                res[i] = ri;
                va = ri * (ri / dg);
                vb = ri * ri;
            } else {
                q[i] = qi;
                va = d[i] * qi;
            }
        }
    }
    if constexpr (SETUP) tile_partials(va, vb, s_red, tid, part_a, part_b);
    else tile_partial(va, s_red, tid, part_a);
}

// The closed form's side of k_cg_scalar (grid B, one wave).  Set-up MODEs: CF_START (after the set-up pass) rz, rr0, the
// trivial images.  The warm entry's: CF_REF (after the pass over the stop reference's image) rr0 = ||r_ref||^2 and the
// trivial images; CF_WARM (after the set-up pass, in CF_START's place) rz and the stop test on r_0 against that rr0.
constexpr int CF_START = 0, CF_REF = 3, CF_WARM = 4;
struct CfSolver {
    static __device__ __forceinline__ bool converged(CgImage& s, double rr, double tol) {
        s.rel = sqrt(rr / s.rr0);
        return s.rel <= tol;
    }
    template <int MODE>
    static __device__ __forceinline__ void setup(CgImage& s, double a, double b, double tol, int* __restrict__ n_done) {
        if (MODE == CF_WARM) {
            s.rz = a;
            if (converged(s, b, tol)) cg_finish(s, n_done);      // the start is already good enough
        } else {
            if (MODE == CF_START) s.rz = a;
            s.rr0 = b;
            s.rel = 0.0;
            s.iters = 0;
            if (!(b > 0.0)) cg_finish(s, n_done);                // r_0 (CF_REF: r_ref) = 0: solved, or nothing to measure against
        }
    }
};

// x += alpha d, r -= alpha q on U; per-tile r . z (part_a), r . r (part_b)
__global__ void __launch_bounds__(CF_THREADS) k_cf_update(int H, int W, int ntx, const int2* __restrict__ tiles,
                                                          const CgImage* __restrict__ img, const uint8_t* __restrict__ flags,
                                                          const double* __restrict__ d, const double* __restrict__ q,
                                                          const double* __restrict__ diag, double* __restrict__ x,
                                                          double* __restrict__ res, double* __restrict__ part_a,
                                                          double* __restrict__ part_b) {
    __shared__ double s_red[CF_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;
    const int tid = threadIdx.y * CF_T + threadIdx.x;
    const int xp = t.tx * CF_T + threadIdx.x, yp = t.ty * CF_T + threadIdx.y;
    double va = 0.0, vb = 0.0;
    if (xp < W && yp < H) {
        const size_t i = (size_t)t.b * H * W + (size_t)yp * W + xp;
        if (flags[i] & F_U) {
            const double al = s.alpha;
            x[i] += al * d[i];
            const double ri = res[i] - al * q[i];
            res[i] = ri;
            va = ri * (ri / diag[i]);
            vb = ri * ri;
        }
    }
    tile_partials(va, vb, s_red, tid, part_a, part_b);
}

// d = z + beta d on U (SETUP: d = z)
template <bool SETUP>
__global__ void __launch_bounds__(CF_THREADS) k_cf_direction(int H, int W, int ntx, const int2* __restrict__ tiles,
                                                             const CgImage* __restrict__ img, const uint8_t* __restrict__ flags,
                                                             const double* __restrict__ res, const double* __restrict__ diag,
                                                             double* __restrict__ d) {
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;
    const int xp = t.tx * CF_T + threadIdx.x, yp = t.ty * CF_T + threadIdx.y;
    if (xp >= W || yp >= H) return;
    const size_t i = (size_t)t.b * H * W + (size_t)yp * W + xp;
    if (!(flags[i] & F_U)) return;
    const double z = res[i] / diag[i];
    d[i] = SETUP ? z : z + s.beta * d[i];
}

// the outputs over the whole frame: alpha = x on U (the start where nothing was solved), the known value elsewhere.
// grid (cdiv(H*W, 256), B)
__global__ void __launch_bounds__(CF_THREADS) k_cf_output(int H, int W, const CgImage* __restrict__ img,
                                                          const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ flags,
                                                          const double* __restrict__ x, float* __restrict__ alpha,
                                                          uint8_t* __restrict__ rgba, double* __restrict__ raw,
                                                          int* __restrict__ iters, double* __restrict__ rel) {
    const size_t P = (size_t)H * W;
    const size_t j = (size_t)blockIdx.x * CF_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    const CgImage& s = img[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (iters) iters[b] = s.iters;
        if (rel) rel[b] = s.rel;
    }
    if (j >= P) return;
    const size_t i = (size_t)b * P + j;
    const uint8_t f = flags[i];
    const double a = (f & F_U) ? x[i] : ((f & F_M) ? 1.0 : 0.0);
    if (raw) raw[i] = a;
    if (alpha) alpha[i] = (float)(a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a));
    if (rgba) {
        rgba[4 * i] = bgr[3 * i]; rgba[4 * i + 1] = bgr[3 * i + 1]; rgba[4 * i + 2] = bgr[3 * i + 2];
        rgba[4 * i + 3] = unit_byte(a);
    }
}

} // namespace
} // namespace ggc

using namespace ggc;

namespace {

// the argument ranges the two entries share, in the order they are reported (the trimap entry has no band: it passes 0)
int cf_check(ggc_ctx* ctx, int B, int H, int W, const void* bgr, const void* guide, int radius, float eps, int band,
             int max_iter, float tol, bool any_output) {
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, any_output, GGC_E_INVALID_ARG, "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || (bgr && guide), GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, radius >= 1 && radius <= CF_RMAX, GGC_E_INVALID_ARG, "closed-form radius %d outside 1..%d", radius, CF_RMAX);
    GGC_REQUIRE(ctx, std::isfinite(eps) && eps >= 1e-12f && eps <= 1.0f, GGC_E_INVALID_ARG,
                "closed-form eps %g outside [1e-12, 1]", (double)eps);
    GGC_REQUIRE(ctx, band >= 0 && band <= 64, GGC_E_INVALID_ARG, "closed-form band %d outside 0..64", band);
    GGC_REQUIRE(ctx, max_iter >= 1 && max_iter <= 100000, GGC_E_INVALID_ARG, "closed-form max_iter %d outside 1..100000",
                max_iter);
    GGC_REQUIRE(ctx, std::isfinite(tol) && tol >= 1e-12f && tol < 1.0f, GGC_E_INVALID_ARG,
                "closed-form tol %g outside [1e-12, 1)", (double)tol);
    GGC_REQUIRE(ctx, H >= 2 * radius + 1 && W >= 2 * radius + 1, GGC_E_SHAPE,
                "closed-form matte needs H, W >= 2r+1 = %d, got %dx%d", 2 * radius + 1, H, W);
    return GGC_OK;
}

// what a front end fills in: the flag plane, the start on U, the U count of every tile (and two byte planes of its own)
struct CfFront { uint8_t *flags, *edge, *hdil; double* x; int32_t* tile_u; };

// The solver behind both entries.  front(f, fgrid, tblk) launches the front end's kernels on st; n_byte_planes is 1
// (flags) plus the byte planes the front end needs for itself.  warm: images stop against the residual of the 0.5 start
// (one more pass of the set-up kernels) instead of against their own start's.
template <class Front>
int cf_solve(ggc_ctx* ctx, hipStream_t st, const char* name, int B, int H, int W, const uint8_t* bgr, int n_byte_planes,
             int radius, float eps, int max_iter, float tol, float* alpha, uint8_t* rgba, double* raw, int32_t* iters,
             double* rel_residual, bool warm, Front&& front) {
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)B * H * W;
    const int ntx = cdiv(W, CF_T), nty = cdiv(H, CF_T), nt = ntx * nty;
    CfFront f{nullptr, nullptr, nullptr, nullptr, nullptr};
    CgImage* img = nullptr;
    int* n_done = nullptr;
    CfStats* stats = nullptr;
    CfAB* ab = nullptr;
    double *res = nullptr, *d = nullptr, *q = nullptr, *diag = nullptr;
    int2* tiles = nullptr;
    double *part_a = nullptr, *part_b = nullptr;
    // the per-pixel arrays (144 bytes per pixel and the byte planes) and the per-tile, per-image ones, sized for every
    // tile of the batch
    const size_t n_tiles_max = (size_t)B * nt;
    if (!carve_scratch(ctx, S_CFMATTE, [&](Carve& c) {
            f.flags = c.take<uint8_t>(P);
            f.edge = c.take<uint8_t>(n_byte_planes > 1 ? P : 0); f.hdil = c.take<uint8_t>(n_byte_planes > 2 ? P : 0);
            stats = c.take<CfStats>(P); ab = c.take<CfAB>(P);
            f.x = c.take<double>(P); res = c.take<double>(P); d = c.take<double>(P); q = c.take<double>(P);
            diag = c.take<double>(P);
            f.tile_u = c.take<int32_t>(n_tiles_max); tiles = c.take<int2>(n_tiles_max);
            part_a = c.take<double>(n_tiles_max); part_b = c.take<double>(n_tiles_max);
            img = c.take<CgImage>(B); n_done = c.take<int>(1);
        }))
        return GGC_E_OOM;
    ProfScope prof(ctx, st, name);
    const dim3 fgrid(ntx, nty, B), tblk(CF_T, CF_T);
    uint8_t* const flags = f.flags;
    double* const x = f.x;
    int32_t* const tile_u = f.tile_u;
    front(f, fgrid, tblk);
    GGC_LAUNCH_CHECK(ctx);

    // the tile list: tiles with U and their eight neighbours (r <= 16 = the tile side).  An image whose U is empty or
    // covers every pixel (nothing anchors it) gets no tiles: alpha = the start, 0 iterations.
    std::vector<int32_t> cnt;
    if (int e = cg_read_counts(ctx, st, tile_u, n_tiles_max, cnt)) return e;
    std::vector<int2> list;
    std::vector<CgImage> host_img;
    std::vector<int64_t> u_count;
    const int n_solve = cg_list_tiles(B, ntx, nty, cnt.data(), 1, (int64_t)H * W, list, host_img, u_count, nullptr);
    const int n_list = (int)list.size();
    if (int e = cg_upload(ctx, st, list, host_img, tiles, img, n_done)) return e;

    if (n_list > 0) {
        const double e = (double)eps;
        const CgScalars sc{st, B, max_iter, (double)tol, img, part_a, part_b, n_done};
        hipLaunchKernelGGL(k_cf_stats, dim3(n_list), tblk, 0, st, H, W, radius, e, ntx, tiles, bgr, stats);
        if (warm) {     // r_ref = -(L x^1/2)_U; ab, res, diag and the partial sums are written again by the set-up proper
            hipLaunchKernelGGL((k_cf_window<true, true>), dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr,
                               flags, stats, x, ab);
            hipLaunchKernelGGL((k_cf_pixel<true, true>), dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr,
                               flags, stats, ab, x, q, res, diag, part_a, part_b);
            sc.step<CfSolver, CF_REF>();
        }
        hipLaunchKernelGGL(k_cf_window<true>, dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr, flags, stats,
                           x, ab);
        hipLaunchKernelGGL(k_cf_pixel<true>, dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr, flags, stats, ab,
                           x, q, res, diag, part_a, part_b);
        if (warm) sc.step<CfSolver, CF_WARM>();
        else sc.step<CfSolver, CF_START>();
        hipLaunchKernelGGL(k_cf_direction<true>, dim3(n_list), tblk, 0, st, H, W, ntx, tiles, img, flags, res, diag, d);
        GGC_LAUNCH_CHECK(ctx);
        const int rc = cg_iterate(ctx, st, max_iter, n_done, n_solve, [&](int) {
            hipLaunchKernelGGL(k_cf_window<false>, dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr, flags,
                               stats, d, ab);
            hipLaunchKernelGGL(k_cf_pixel<false>, dim3(n_list), tblk, 0, st, H, W, radius, ntx, tiles, img, bgr, flags,
                               stats, ab, d, q, res, diag, part_a, part_b);
            sc.step<CfSolver, CG_ALPHA>();
            hipLaunchKernelGGL(k_cf_update, dim3(n_list), tblk, 0, st, H, W, ntx, tiles, img, flags, d, q, diag, x, res,
                               part_a, part_b);
            sc.step<CfSolver, CG_BETA>();
            hipLaunchKernelGGL(k_cf_direction<false>, dim3(n_list), tblk, 0, st, H, W, ntx, tiles, img, flags, res, diag, d);
        });
        if (rc) return rc;
    }
    const dim3 ogrid(cdiv((int64_t)H * W, CF_THREADS), B);
    hipLaunchKernelGGL(k_cf_output, ogrid, dim3(CF_THREADS), 0, st, H, W, img, bgr, flags, x, alpha, rgba, raw, iters,
                       rel_residual);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

} // namespace

extern "C" int ggc_closed_form_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                                     const uint8_t* binary, int radius, float eps, int band, int max_iter, float tol,
                                     float* alpha, uint8_t* rgba, double* raw, int32_t* iters, double* rel_residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    if (int e = cf_check(ctx, B, H, W, bgr, binary, radius, eps, band, max_iter, tol,
                         alpha || rgba || raw || iters || rel_residual))
        return e;
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return cf_solve(ctx, st, "closed_form_matte", B, H, W, bgr, 3, radius, eps, max_iter, tol, alpha, rgba, raw, iters,
                    rel_residual, false, [&](const CfFront& f, dim3 fgrid, dim3 tblk) {
                        hipLaunchKernelGGL(k_cf_edge, fgrid, tblk, 0, st, H, W, binary, f.edge);
                        hipLaunchKernelGGL(k_cf_dilate_h, fgrid, tblk, 0, st, H, W, band, f.edge, f.hdil);
                        hipLaunchKernelGGL(k_cf_dilate_v, fgrid, tblk, 0, st, H, W, band, f.hdil, binary, f.flags, f.x,
                                           f.tile_u);
                    });
}

extern "C" int ggc_trimap_matte(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                                const uint8_t* trimap, int radius, float eps, int max_iter, float tol, const float* alpha0,
                                float* alpha, uint8_t* rgba, double* raw, int32_t* iters, double* rel_residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    if (int e = cf_check(ctx, B, H, W, bgr, trimap, radius, eps, 0, max_iter, tol,
                         alpha || rgba || raw || iters || rel_residual))
        return e;
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return cf_solve(ctx, st, "trimap_matte", B, H, W, bgr, 1, radius, eps, max_iter, tol, alpha, rgba, raw, iters,
                    rel_residual, false, [&](const CfFront& f, dim3 fgrid, dim3 tblk) {
                        hipLaunchKernelGGL(k_cf_trimap, fgrid, tblk, 0, st, H, W, trimap, alpha0, f.flags, f.x, f.tile_u);
                    });
}

extern "C" int ggc_trimap_matte_warm(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                                     const uint8_t* trimap, int radius, float eps, int max_iter, float tol,
                                     const float* alpha0, float* alpha, uint8_t* rgba, double* raw, int32_t* iters,
                                     double* rel_residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    if (int e = cf_check(ctx, B, H, W, bgr, trimap, radius, eps, 0, max_iter, tol,
                         alpha || rgba || raw || iters || rel_residual))
        return e;
    GGC_REQUIRE(ctx, alpha0, GGC_E_INVALID_ARG, "null pointer: the warm solve needs alpha0");
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return cf_solve(ctx, st, "trimap_matte_warm", B, H, W, bgr, 1, radius, eps, max_iter, tol, alpha, rgba, raw, iters,
                    rel_residual, true, [&](const CfFront& f, dim3 fgrid, dim3 tblk) {
                        hipLaunchKernelGGL(k_cf_trimap, fgrid, tblk, 0, st, H, W, trimap, alpha0, f.flags, f.x, f.tile_u);
                    });
}

extern "C" int ggc_lift_trimap(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* trimap,
                               const float* alpha, int H1, int W1, int grow, uint8_t* trimap_full, float* alpha0_full) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H1 >= H && W1 >= W && H1 <= 32768 && W1 <= 32768,
                GGC_E_SHAPE, "bad shape B=%d H=%d W=%d H1=%d W1=%d", B, H, W, H1, W1);
    GGC_REQUIRE(ctx, trimap_full || alpha0_full, GGC_E_INVALID_ARG, "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || ((trimap || !trimap_full) && (alpha || !alpha0_full)), GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, grow >= 0 && grow <= 64, GGC_E_INVALID_ARG, "lift grow %d outside 0..64", grow);
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    const bool dilate = trimap_full && grow > 0;
    const size_t P1 = (size_t)B * H1 * W1;
    uint8_t *unknown = nullptr, *hdil = nullptr;
    if (dilate && !carve_scratch(ctx, S_CFMATTE, [&](Carve& c) { unknown = c.take<uint8_t>(P1); hdil = c.take<uint8_t>(P1); }))
        return GGC_E_OOM;
    ProfScope prof(ctx, st, "lift_trimap");
    const dim3 grid(cdiv(W1, CF_T), cdiv(H1, CF_T), B), tblk(CF_T, CF_T);
    hipLaunchKernelGGL(k_cf_lift, grid, tblk, 0, st, H, W, H1, W1, trimap, alpha, trimap_full, dilate ? unknown : nullptr,
                       alpha0_full);
    if (dilate) {
        hipLaunchKernelGGL(k_cf_dilate_h, grid, tblk, 0, st, H1, W1, grow, unknown, hdil);
        hipLaunchKernelGGL(k_cf_dilate_v_trimap<false>, grid, tblk, 0, st, H1, W1, grow, hdil, trimap_full, trimap_full);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

extern "C" int ggc_closed_form_band(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* binary, int band,
                                    uint8_t* trimap) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, trimap, GGC_E_INVALID_ARG, "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || binary, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, band >= 0 && band <= 64, GGC_E_INVALID_ARG, "closed-form band %d outside 0..64", band);
    if (B == 0) return GGC_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)B * H * W;
    uint8_t *edge = nullptr, *hdil = nullptr;
    if (!carve_scratch(ctx, S_CFMATTE, [&](Carve& c) { edge = c.take<uint8_t>(P); hdil = c.take<uint8_t>(P); }))
        return GGC_E_OOM;
    ProfScope prof(ctx, st, "closed_form_band");
    const dim3 grid(cdiv(W, CF_T), cdiv(H, CF_T), B), tblk(CF_T, CF_T);
    hipLaunchKernelGGL(k_cf_edge, grid, tblk, 0, st, H, W, binary, edge);
    hipLaunchKernelGGL(k_cf_dilate_h, grid, tblk, 0, st, H, W, band, edge, hdil);
    hipLaunchKernelGGL(k_cf_dilate_v_trimap<true>, grid, tblk, 0, st, H, W, band, hdil, binary, trimap);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
