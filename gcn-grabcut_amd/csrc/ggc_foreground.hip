// ggc_foreground.hip — O4: foreground colour estimation under a given alpha matte (the multi-level foreground
// estimation energy of Germer, Uelwer, Conrad and Harmeling, ICPR 2020, restricted to the pixels of fractional alpha with
// Dirichlet values), solved on the device by conjugate gradients preconditioned with the exact 2 x 2 block of every
// pixel.  include/ggc.h states the system; DESIGN.md §5.14 the tiling and the bytes.
//
// Layout.  The tile list, the fixed-order sums, the per-image scalars and the poll are ggc_cg.h's.  k_fg_snap writes alpha'
// over the whole frame and counts U per tile; listed are the tiles that hold U (ring 0: the stencil reaches one pixel, so
// no neighbour tile is needed).  The CG vectors live in a compact store of 256 entries per LISTED tile, six float64 per
// entry (F and B of the three channels); tile_slot maps a tile of the frame to its place in the list.  Per listed tile
// and iteration:
//   k_fg_apply   p = z + beta p (z = M^-1 r recomputed from r and alpha') on the tile and a one-pixel halo, staged in
//                LDS; q = A p on the tile; per-tile p . q.  p is double-buffered: a neighbour tile reads the old p of
//                this tile's edge while this tile writes the new one.
//   k_cg_scalar  per image: alpha = rz / (p . q)
//   k_fg_update  x += alpha p, r -= alpha q, z = M^-1 r; per-tile r . z and r . r
//   k_cg_scalar  per image: convergence (||r|| <= stop = max(tol ||r_0||, 1e-12 sqrt(6 |U|))), the iteration count, beta
// The link weights and the 2 x 2 inverse are recomputed from alpha' staged in LDS wherever they are needed.
#include "ggc_cg.h"
#include "ggc_image.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int FG_T = CG_T, FG_THREADS = CG_THREADS;
constexpr int FG_S1 = FG_T + 2;                   // tile with a one-pixel halo
constexpr int FG_S2 = FG_T + 4;                   // ... a two-pixel halo (alpha' under the halo's preconditioner)
constexpr double FG_DELTA = 1e-6;                 // the anchor of the definition
constexpr double FG_SNAP = 1.0 / 510.0;
constexpr double FG_OUTSIDE = -1.0;               // alpha' staged for a pixel outside the image: no link

struct alignas(16) V6 { double v[6]; };           // F (b, g, r) then B (b, g, r) of one pixel

__device__ __forceinline__ bool is_u(double a) { return a > 0.0 && a < 1.0; }

// alpha' and the per-tile count of U.  grid (cdiv(W, 16), cdiv(H, 16), B), 16 x 16 threads
__global__ void __launch_bounds__(FG_THREADS) k_fg_snap(int H, int W, const float* __restrict__ alpha,
                                                        float* __restrict__ ap, int32_t* __restrict__ tile_u) {
    __shared__ int s_cnt[FG_THREADS];
    const int tid = threadIdx.y * FG_T + threadIdx.x;
    const int x = blockIdx.x * FG_T + threadIdx.x, y = blockIdx.y * FG_T + threadIdx.y;
    int u = 0;
    if (x < W && y < H) {
        const size_t i = (size_t)blockIdx.z * H * W + (size_t)y * W + x;
        const float af = alpha[i];
        const double a = (double)af;
        float s = af;
        if (!(a >= FG_SNAP)) s = 0.0f;                           // a NaN lands here: it is snapped to 0
        else if (a > 1.0 - FG_SNAP) s = 1.0f;
        ap[i] = s;
        u = (s > 0.0f && s < 1.0f) ? 1 : 0;
    }
    count_tile(u, s_cnt, tid, tile_u);
}

// ---------------------------------------------------------------- per listed tile
// alpha' of the S x S pixels from (y0, x0) of image b, FG_OUTSIDE beyond the image
__device__ __forceinline__ void stage_alpha(double* s_a, int S, int y0, int x0, int H, int W, const float* __restrict__ ap,
                                            size_t base, int tid) {
    for (int e = tid; e < S * S; e += FG_THREADS) {
        const int yy = y0 + e / S, xx = x0 + e % S;
        s_a[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (double)ap[base + (size_t)yy * W + xx] : FG_OUTSIDE;
    }
}

// the link of a pixel of U (alpha' a) to a neighbour (alpha' an): its weight, and whether it carries F and B
struct Link { double wf, wb; };
__device__ __forceinline__ Link link_of(double a, double an, double eps_r, double omega) {
    if (an < 0.0) return Link{0.0, 0.0};                         // beyond the image
    const double w = eps_r + omega * fabs(a - an);
    return Link{an > 0.0 ? w : 0.0, an < 1.0 ? w : 0.0};         // F: the neighbour in U or O; B: in U or Z
}

// z = M^-1 r with M the 2 x 2 block [[a^2 + delta + sum wf, a (1 - a)], [a (1 - a), (1 - a)^2 + delta + sum wb]].
// s_a: alpha' staged with row stride S, c the pixel's index in it
__device__ __forceinline__ V6 precondition(const V6& r, const double* s_a, int c, int S, double eps_r, double omega) {
    const double a = s_a[c];
    const Link l0 = link_of(a, s_a[c - S], eps_r, omega), l1 = link_of(a, s_a[c - 1], eps_r, omega);
    const Link l2 = link_of(a, s_a[c + 1], eps_r, omega), l3 = link_of(a, s_a[c + S], eps_r, omega);
    const double dff = a * a + FG_DELTA + (((l0.wf + l1.wf) + l2.wf) + l3.wf);
    const double dbb = (1.0 - a) * (1.0 - a) + FG_DELTA + (((l0.wb + l1.wb) + l2.wb) + l3.wb);
    const double dfb = a * (1.0 - a);
    const double det = dff * dbb - dfb * dfb;
    V6 z;
    for (int ch = 0; ch < 3; ++ch) {
        z.v[ch] = (dbb * r.v[ch] - dfb * r.v[3 + ch]) / det;
        z.v[3 + ch] = (dff * r.v[3 + ch] - dfb * r.v[ch]) / det;
    }
    return z;
}

// where the CG vectors keep pixel (y, x) of image b: its tile's slot in the list, then the pixel within the tile
__device__ __forceinline__ size_t vec_index(const int32_t* __restrict__ tile_slot, int b, int nt, int ntx, int y, int x) {
    const int slot = tile_slot[(size_t)b * nt + (y / FG_T) * ntx + x / FG_T];
    return (size_t)slot * FG_THREADS + (y % FG_T) * FG_T + (x % FG_T);
}

// x = (I, I), r = b - A x on U, and the per-tile r . z (part_a), r . r (part_b)
__global__ void __launch_bounds__(FG_THREADS) k_fg_setup(int H, int W, int ntx, double eps_r, double omega,
                                                         const int2* __restrict__ tiles, const uint8_t* __restrict__ bgr,
                                                         const float* __restrict__ ap, V6* __restrict__ x,
                                                         V6* __restrict__ res, double* __restrict__ part_a,
                                                         double* __restrict__ part_b) {
    __shared__ double s_a[FG_S1 * FG_S1];
    __shared__ double s_i[FG_S1 * FG_S1][3];
    __shared__ double s_red[FG_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const int tid = threadIdx.y * FG_T + threadIdx.x;
    const int x0 = t.tx * FG_T - 1, y0 = t.ty * FG_T - 1;
    const size_t base = (size_t)t.b * H * W;
    stage_alpha(s_a, FG_S1, y0, x0, H, W, ap, base, tid);
    for (int e = tid; e < FG_S1 * FG_S1; e += FG_THREADS) {
        const int yy = y0 + e / FG_S1, xx = x0 + e % FG_S1;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        for (int ch = 0; ch < 3; ++ch)
            s_i[e][ch] = in ? (double)bgr[3 * (base + (size_t)yy * W + xx) + ch] / 255.0 : 0.0;
    }
    __syncthreads();
    const int c = (threadIdx.y + 1) * FG_S1 + threadIdx.x + 1;
    const double a = s_a[c];
    double va = 0.0, vb = 0.0;
    if (is_u(a)) {                                               // outside the image alpha' is FG_OUTSIDE
        const int nb[4] = {c - FG_S1, c - 1, c + 1, c + FG_S1};
        V6 r, xi;
        for (int ch = 0; ch < 3; ++ch) {
            const double I = s_i[c][ch];
            const double m = (a * I + (1.0 - a) * I) - I;        // the data term at F = B = I: rounding noise
            double gf = a * m, gb = (1.0 - a) * m;
            for (int k = 0; k < 4; ++k) {
                const Link l = link_of(a, s_a[nb[k]], eps_r, omega);
                const double d = I - s_i[nb[k]][ch];
                gf += l.wf * d;
                gb += l.wb * d;
            }
            r.v[ch] = -gf; r.v[3 + ch] = -gb;
            xi.v[ch] = I; xi.v[3 + ch] = I;
        }
        const size_t j = (size_t)blockIdx.x * FG_THREADS + tid;
        x[j] = xi;
        res[j] = r;
        const V6 z = precondition(r, s_a, c, FG_S1, eps_r, omega);
        for (int k = 0; k < 6; ++k) { va += r.v[k] * z.v[k]; vb += r.v[k] * r.v[k]; }
    }
    const double sa = block_sum(va, s_red, tid);
    if (tid == 0) part_a[blockIdx.x] = sa;
    __syncthreads();
    const double sb = block_sum(vb, s_red, tid);
    if (tid == 0) part_b[blockIdx.x] = sb;
}

// p = z + beta p_in (FIRST: p = z) on the tile and its halo, the tile's part written to p_out; q = A p; per-tile p . q
template <bool FIRST>
__global__ void __launch_bounds__(FG_THREADS) k_fg_apply(int H, int W, int ntx, int nt, double eps_r, double omega,
                                                         const int2* __restrict__ tiles, const int32_t* __restrict__ tile_slot,
                                                         const CgImage* __restrict__ img, const float* __restrict__ ap,
                                                         const V6* __restrict__ res, const V6* __restrict__ p_in,
                                                         V6* __restrict__ p_out, V6* __restrict__ q,
                                                         double* __restrict__ part_a) {
    __shared__ double s_a[FG_S2 * FG_S2];
    __shared__ V6 s_p[FG_S1 * FG_S1];
    __shared__ double s_red[FG_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;                                          // uniform over the block
    const int tid = threadIdx.y * FG_T + threadIdx.x;
    const int x0 = t.tx * FG_T, y0 = t.ty * FG_T;
    const size_t base = (size_t)t.b * H * W;
    stage_alpha(s_a, FG_S2, y0 - 2, x0 - 2, H, W, ap, base, tid);
    __syncthreads();
    const double beta = FIRST ? 0.0 : s.beta;
    for (int e = tid; e < FG_S1 * FG_S1; e += FG_THREADS) {
        const int ey = e / FG_S1, ex = e % FG_S1;
        const int c2 = (ey + 1) * FG_S2 + ex + 1;
        V6 p;
        for (int k = 0; k < 6; ++k) p.v[k] = 0.0;
        if (is_u(s_a[c2])) {                                     // in the image, in U: its tile is listed
            const int yy = y0 - 1 + ey, xx = x0 - 1 + ex;
            const bool own = ey >= 1 && ey <= FG_T && ex >= 1 && ex <= FG_T;
            const size_t j = own ? (size_t)blockIdx.x * FG_THREADS + (ey - 1) * FG_T + (ex - 1)
                                 : vec_index(tile_slot, t.b, nt, ntx, yy, xx);
            p = precondition(res[j], s_a, c2, FG_S2, eps_r, omega);
            if constexpr (!FIRST) {
                const V6 po = p_in[j];
                for (int k = 0; k < 6; ++k) p.v[k] = p.v[k] + beta * po.v[k];
            }
            if (own) p_out[j] = p;
        }
        s_p[e] = p;
    }
    __syncthreads();
    const int c = (threadIdx.y + 1) * FG_S1 + threadIdx.x + 1, c2 = (threadIdx.y + 2) * FG_S2 + threadIdx.x + 2;
    const double a = s_a[c2];
    double va = 0.0;
    if (is_u(a)) {
        const int nb[4] = {c - FG_S1, c - 1, c + 1, c + FG_S1}, nb2[4] = {c2 - FG_S2, c2 - 1, c2 + 1, c2 + FG_S2};
        Link l[4];
        for (int k = 0; k < 4; ++k) l[k] = link_of(a, s_a[nb2[k]], eps_r, omega);
        const V6 p = s_p[c];
        V6 qi;
        for (int ch = 0; ch < 3; ++ch) {
            const double pf = p.v[ch], pb = p.v[3 + ch];
            const double m = a * pf + (1.0 - a) * pb;
            double qf = a * m + FG_DELTA * pf, qb = (1.0 - a) * m + FG_DELTA * pb;
            for (int k = 0; k < 4; ++k) {                        // p is 0 off U: a neighbour in O or Z adds w p_i only
                qf += l[k].wf * (pf - s_p[nb[k]].v[ch]);
                qb += l[k].wb * (pb - s_p[nb[k]].v[3 + ch]);
            }
            qi.v[ch] = qf; qi.v[3 + ch] = qb;
        }
        q[(size_t)blockIdx.x * FG_THREADS + tid] = qi;
        for (int k = 0; k < 6; ++k) va += p.v[k] * qi.v[k];
    }
    const double sa = block_sum(va, s_red, tid);
    if (tid == 0) part_a[blockIdx.x] = sa;
}

// x += alpha p, r -= alpha q on U; per-tile r . z (part_a) with z = M^-1 r, and r . r (part_b)
__global__ void __launch_bounds__(FG_THREADS) k_fg_update(int H, int W, int ntx, double eps_r, double omega,
                                                          const int2* __restrict__ tiles, const CgImage* __restrict__ img,
                                                          const float* __restrict__ ap, const V6* __restrict__ p,
                                                          const V6* __restrict__ q, V6* __restrict__ x, V6* __restrict__ res,
                                                          double* __restrict__ part_a, double* __restrict__ part_b) {
    __shared__ double s_a[FG_S1 * FG_S1];
    __shared__ double s_red[FG_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;
    const int tid = threadIdx.y * FG_T + threadIdx.x;
    stage_alpha(s_a, FG_S1, t.ty * FG_T - 1, t.tx * FG_T - 1, H, W, ap, (size_t)t.b * H * W, tid);
    __syncthreads();
    const int c = (threadIdx.y + 1) * FG_S1 + threadIdx.x + 1;
    double va = 0.0, vb = 0.0;
    if (is_u(s_a[c])) {
        const size_t j = (size_t)blockIdx.x * FG_THREADS + tid;
        const double al = s.alpha;
        const V6 pj = p[j], qj = q[j];
        V6 xj = x[j], rj = res[j];
        for (int k = 0; k < 6; ++k) { xj.v[k] += al * pj.v[k]; rj.v[k] -= al * qj.v[k]; }
        x[j] = xj;
        res[j] = rj;
        const V6 z = precondition(rj, s_a, c, FG_S1, eps_r, omega);
        for (int k = 0; k < 6; ++k) { va += rj.v[k] * z.v[k]; vb += rj.v[k] * rj.v[k]; }
    }
    const double sa = block_sum(va, s_red, tid);
    if (tid == 0) part_a[blockIdx.x] = sa;
    __syncthreads();
    const double sb = block_sum(vb, s_red, tid);
    if (tid == 0) part_b[blockIdx.x] = sb;
}

// The foreground's side of k_cg_scalar (grid B, one wave).  s.stop is the absolute floor on entry and the threshold on
// ||r|| after the set-up MODE FG_START (after k_fg_setup): rz, rr0, the threshold, the images that start solved.
constexpr int FG_START = 0;
struct FgSolver {
    static __device__ __forceinline__ bool converged(CgImage& s, double rr, double) {
        const double rn = sqrt(rr);
        s.rel = rn / sqrt(s.rr0);
        return rn <= s.stop;
    }
    template <int MODE>
    static __device__ __forceinline__ void setup(CgImage& s, double a, double b, double tol, int* __restrict__ n_done) {
        const double r0 = sqrt(b), rel_stop = tol * r0;
        s.rz = a;
        s.rr0 = b;
        s.rel = 0.0;
        s.iters = 0;
        s.stop = rel_stop > s.stop ? rel_stop : s.stop;
        if (!(r0 > s.stop)) cg_finish(s, n_done);                // F = B = I already solves the system
    }
};

// the outputs over the whole frame.  grid (cdiv(H*W, 256), B)
__global__ void __launch_bounds__(FG_THREADS) k_fg_output(int H, int W, int ntx, int nt, const CgImage* __restrict__ img,
                                                          const int32_t* __restrict__ tile_slot, const uint8_t* __restrict__ bgr,
                                                          const float* __restrict__ alpha, const float* __restrict__ ap,
                                                          const V6* __restrict__ x, uint8_t* __restrict__ foreground,
                                                          uint8_t* __restrict__ rgba, double* __restrict__ raw_f,
                                                          double* __restrict__ raw_b, int* __restrict__ iters,
                                                          double* __restrict__ rel) {
    const size_t P = (size_t)H * W;
    const size_t j = (size_t)blockIdx.x * FG_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (iters) iters[b] = img[b].iters;
        if (rel) rel[b] = img[b].rel;
    }
    if (j >= P) return;
    const size_t i = (size_t)b * P + j;
    const uint8_t px[3] = {bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]};
    uint8_t col[3] = {px[0], px[1], px[2]};
    double f[3], bk[3];
    for (int ch = 0; ch < 3; ++ch) f[ch] = bk[ch] = (double)px[ch] / 255.0;
    if (is_u((double)ap[i])) {
        const V6 v = x[vec_index(tile_slot, b, nt, ntx, (int)(j / W), (int)(j % W))];
        for (int ch = 0; ch < 3; ++ch) { f[ch] = v.v[ch]; bk[ch] = v.v[3 + ch]; col[ch] = unit_byte(v.v[ch]); }
    }
    for (int ch = 0; ch < 3; ++ch) {
        if (foreground) foreground[3 * i + ch] = col[ch];
        if (rgba) rgba[4 * i + ch] = col[ch];
        if (raw_f) raw_f[3 * i + ch] = f[ch];
        if (raw_b) raw_b[3 * i + ch] = bk[ch];
    }
    if (rgba) rgba[4 * i + 3] = unit_byte((double)alpha[i]);
}

} // namespace
} // namespace ggc

using namespace ggc;

extern "C" int ggc_estimate_foreground(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* bgr,
                                       const float* alpha, float eps_r, float omega, int max_iter, float tol,
                                       uint8_t* foreground, uint8_t* rgba, double* raw_f, double* raw_b, int32_t* iters,
                                       double* rel_residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, foreground || rgba || raw_f || raw_b || iters || rel_residual, GGC_E_INVALID_ARG,
                "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || (bgr && alpha), GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, std::isfinite(eps_r) && eps_r >= 0.0f && eps_r <= 1.0f, GGC_E_INVALID_ARG,
                "foreground eps_r %g outside [0, 1]", (double)eps_r);
    GGC_REQUIRE(ctx, std::isfinite(omega) && omega >= 0.0f && omega <= 1e3f, GGC_E_INVALID_ARG,
                "foreground omega %g outside [0, 1000]", (double)omega);
    GGC_REQUIRE(ctx, eps_r + omega > 0.0f, GGC_E_INVALID_ARG, "foreground eps_r + omega must be positive");
    GGC_REQUIRE(ctx, max_iter >= 1 && max_iter <= 100000, GGC_E_INVALID_ARG, "foreground max_iter %d outside 1..100000",
                max_iter);
    GGC_REQUIRE(ctx, std::isfinite(tol) && tol >= 1e-12f && tol < 1.0f, GGC_E_INVALID_ARG,
                "foreground tol %g outside [1e-12, 1)", (double)tol);
    if (B == 0) return GGC_OK;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t P = (size_t)B * H * W;
    const int ntx = cdiv(W, FG_T), nty = cdiv(H, FG_T), nt = ntx * nty;
    const size_t n_tiles_max = (size_t)B * nt;
    float* ap = nullptr;
    int32_t *tile_u = nullptr, *tile_slot = nullptr;
    int2* tiles = nullptr;
    double *part_a = nullptr, *part_b = nullptr;
    CgImage* img = nullptr;
    int* n_done = nullptr;
    // over the whole frame: 4 bytes per pixel, 32 per tile, 64 per image
    if (!carve_scratch(ctx, S_FOREGROUND, [&](Carve& c) {
            ap = c.take<float>(P);
            tile_u = c.take<int32_t>(n_tiles_max); tile_slot = c.take<int32_t>(n_tiles_max);
            tiles = c.take<int2>(n_tiles_max);
            part_a = c.take<double>(n_tiles_max); part_b = c.take<double>(n_tiles_max);
            img = c.take<CgImage>(B); n_done = c.take<int>(1);
        }))
        return GGC_E_OOM;
    ProfScope prof(ctx, st, "estimate_foreground");
    hipLaunchKernelGGL(k_fg_snap, dim3(ntx, nty, B), dim3(FG_T, FG_T), 0, st, H, W, alpha, ap, tile_u);
    GGC_LAUNCH_CHECK(ctx);

    // the tile list: the tiles that hold a pixel of U
    std::vector<int32_t> cnt, slot;
    if (int e = cg_read_counts(ctx, st, tile_u, n_tiles_max, cnt)) return e;
    std::vector<int2> list;
    std::vector<CgImage> host_img;
    std::vector<int64_t> u_count;
    const int n_solve = cg_list_tiles(B, ntx, nty, cnt.data(), 0, 0, list, host_img, u_count, &slot);
    for (int b = 0; b < B; ++b) host_img[b].stop = 1e-12 * std::sqrt(6.0 * (double)u_count[b]);
    const int n_list = (int)list.size();
    // the CG vectors, 256 entries per listed tile: x, r, q and the two p, 240 bytes per entry
    V6 *x = nullptr, *res = nullptr, *q = nullptr, *p0 = nullptr, *p1 = nullptr;
    const size_t n_vec = (size_t)n_list * FG_THREADS;
    if (n_list > 0 && !carve_scratch(ctx, S_FOREGROUND_VEC, [&](Carve& c) {
            x = c.take<V6>(n_vec); res = c.take<V6>(n_vec); q = c.take<V6>(n_vec);
            p0 = c.take<V6>(n_vec); p1 = c.take<V6>(n_vec);
        }))
        return GGC_E_OOM;
    GGC_HIP(ctx, hipMemcpyAsync(tile_slot, slot.data(), n_tiles_max * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (int e = cg_upload(ctx, st, list, host_img, tiles, img, n_done)) return e;

    if (n_list > 0) {
        const double er = (double)eps_r, om = (double)omega;
        const CgScalars sc{st, B, max_iter, (double)tol, img, part_a, part_b, n_done};
        const dim3 tblk(FG_T, FG_T);
        hipLaunchKernelGGL(k_fg_setup, dim3(n_list), tblk, 0, st, H, W, ntx, er, om, tiles, bgr, ap, x, res, part_a, part_b);
        sc.step<FgSolver, FG_START>();
        GGC_LAUNCH_CHECK(ctx);
        const int rc = cg_iterate(ctx, st, max_iter, n_done, n_solve, [&](int it) {
            V6 *p_new = (it & 1) ? p1 : p0, *p_old = (it & 1) ? p0 : p1;
            if (it == 0)
                hipLaunchKernelGGL(k_fg_apply<true>, dim3(n_list), tblk, 0, st, H, W, ntx, nt, er, om, tiles, tile_slot, img,
                                   ap, res, p_old, p_new, q, part_a);
            else
                hipLaunchKernelGGL(k_fg_apply<false>, dim3(n_list), tblk, 0, st, H, W, ntx, nt, er, om, tiles, tile_slot, img,
                                   ap, res, p_old, p_new, q, part_a);
            sc.step<FgSolver, CG_ALPHA>();
            hipLaunchKernelGGL(k_fg_update, dim3(n_list), tblk, 0, st, H, W, ntx, er, om, tiles, img, ap, p_new, q, x, res,
                               part_a, part_b);
            sc.step<FgSolver, CG_BETA>();
        });
        if (rc) return rc;
    }
    const dim3 ogrid(cdiv((int64_t)H * W, FG_THREADS), B);
    hipLaunchKernelGGL(k_fg_output, ogrid, dim3(FG_THREADS), 0, st, H, W, ntx, nt, img, tile_slot, bgr, alpha, ap, x,
                       foreground, rgba, raw_f, raw_b, iters, rel_residual);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
