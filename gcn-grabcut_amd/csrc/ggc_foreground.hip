// ggc_foreground.hip — O4: foreground colour estimation under a given alpha matte (the multi-level foreground
// estimation energy of Germer, Uelwer, Conrad and Harmeling, ICPR 2020, restricted to the pixels of fractional alpha with
// Dirichlet values), solved on the device by conjugate gradients preconditioned with the exact 2 x 2 block of every
// pixel.  include/ggc.h states the system; DESIGN.md §5.14 the tiling and the bytes.
//
// Layout.  The tile list, the sums and the scalars are ggc_cg.h's; the compact vector store, the iteration's kernels, the
// stop rule (||r|| <= max(tol ||r_0||, 1e-12 sqrt(6 |U|))) and the host driver are ggc_cg_compact.h's.  Here are the front
// end (k_fg_snap: alpha' over the whole frame, U per tile), the set-up, the output and the policy FgProblem: six float64
// per entry (F and B of the three channels), alpha' as the field, the operator and the 2 x 2 block preconditioner.  The
// link weights and the 2 x 2 inverse are recomputed from alpha' staged in LDS wherever they are needed; the preconditioner
// reads a pixel's four neighbours, so the apply stages alpha' with a two-pixel halo and the update with one.
#include "ggc_cg_compact.h"
#include "ggc_image.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int FG_T = CG_T, FG_THREADS = CG_THREADS;
constexpr int FG_S1 = CGC_S1;                     // tile with a one-pixel halo
constexpr double FG_DELTA = 1e-6;                 // the anchor of the definition
constexpr double FG_SNAP = 1.0 / 510.0;

using V6 = CgVec<6>;                              // F (b, g, r) then B (b, g, r) of one pixel

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
// the link of a pixel of U (alpha' a) to a neighbour (alpha' an): its weight, and whether it carries F and B
struct Link { double wf, wb; };
__device__ __forceinline__ Link link_of(double a, double an, double eps_r, double omega) {
    if (an < 0.0) return Link{0.0, 0.0};                         // beyond the image
    const double w = eps_r + omega * fabs(a - an);
    return Link{an > 0.0 ? w : 0.0, an < 1.0 ? w : 0.0};         // F: the neighbour in U or O; B: in U or Z
}

// the foreground's policy for ggc_cg_compact.h.  s_a: alpha' staged with row stride S, c the pixel's index in it
struct FgProblem {
    static constexpr int N = 6, HALO = 2, UPDATE_HALO = 1;       // the halo's pixels are preconditioned: one more ring
    using Stored = float;
    using Field = double;
    static constexpr double OUTSIDE = -1.0;                      // alpha' staged for a pixel outside the image: no link
    static constexpr double FLOOR = 1e-12;
    struct Params { double eps_r, omega; };

    static __device__ __forceinline__ bool unknown(double a) { return a > 0.0 && a < 1.0; }

    // z = M^-1 r with M the 2 x 2 block [[a^2 + delta + sum wf, a (1 - a)], [a (1 - a), (1 - a)^2 + delta + sum wb]]
    static __device__ __forceinline__ V6 precondition(const V6& r, const double* s_a, int c, int S, Params prm) {
        const double eps_r = prm.eps_r, omega = prm.omega;
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

    // (A p) at the pixel staged at s_p[c] and s_a[c2]
    static __device__ __forceinline__ V6 apply(const V6* s_p, int c, const double* s_a, int c2, int S, Params prm) {
        const double a = s_a[c2];
        const int nb[4] = {c - FG_S1, c - 1, c + 1, c + FG_S1}, nb2[4] = {c2 - S, c2 - 1, c2 + 1, c2 + S};
        Link l[4];
        for (int k = 0; k < 4; ++k) l[k] = link_of(a, s_a[nb2[k]], prm.eps_r, prm.omega);
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
        return qi;
    }
};

// x = (I, I), r = b - A x on U, and the per-tile r . z (part_a), r . r (part_b)
__global__ void __launch_bounds__(FG_THREADS) k_fg_setup(int H, int W, int ntx, double eps_r, double omega,
                                                         const int2* __restrict__ tiles, const uint8_t* __restrict__ bgr,
                                                         const float* __restrict__ ap, V6* __restrict__ x,
                                                         V6* __restrict__ res, double* __restrict__ part_a,
                                                         double* __restrict__ part_b) {
    __shared__ double s_a[FG_S1 * FG_S1];
    __shared__ double s_i[FG_S1 * FG_S1][3];
    __shared__ double s_red[FG_THREADS];
    const FgProblem::Params prm{eps_r, omega};
    const TileRef t = tile_of(tiles, ntx);
    const int tid = threadIdx.y * FG_T + threadIdx.x;
    const int x0 = t.tx * FG_T - 1, y0 = t.ty * FG_T - 1;
    const size_t base = (size_t)t.b * H * W;
    cgc_stage<FgProblem>(s_a, FG_S1, y0, x0, H, W, ap, base, tid);
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
    if (FgProblem::unknown(a)) {                                 // outside the image alpha' is OUTSIDE
        const int nb[4] = {c - FG_S1, c - 1, c + 1, c + FG_S1};
        V6 r, xi;
        for (int ch = 0; ch < 3; ++ch) {
            const double I = s_i[c][ch];
            const double m = (a * I + (1.0 - a) * I) - I;        // the data term at F = B = I: rounding noise
            double gf = a * m, gb = (1.0 - a) * m;
            for (int k = 0; k < 4; ++k) {
                const Link l = link_of(a, s_a[nb[k]], prm.eps_r, prm.omega);
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
        const V6 z = FgProblem::precondition(r, s_a, c, FG_S1, prm);
        for (int k = 0; k < 6; ++k) { va += r.v[k] * z.v[k]; vb += r.v[k] * r.v[k]; }
    }
    tile_partials(va, vb, s_red, tid, part_a, part_b);
}

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
    if (FgProblem::unknown((double)ap[i])) {
        const V6 v = x[cg_vec_index(tile_slot, b, nt, ntx, (int)(j / W), (int)(j % W))];
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
    CgCompactFrame<FgProblem> f;                                 // the field is alpha': 4 bytes per pixel
    if (!cg_compact_frame(ctx, S_FOREGROUND, B, H, W, f)) return GGC_E_OOM;
    ProfScope prof(ctx, st, "estimate_foreground");
    hipLaunchKernelGGL(k_fg_snap, dim3(f.ntx, f.nty, B), dim3(FG_T, FG_T), 0, st, H, W, alpha, f.field, f.tile_u);
    GGC_LAUNCH_CHECK(ctx);

    // every image with a pixel of U is solved; the CG vectors take 240 bytes per entry
    const FgProblem::Params prm{(double)eps_r, (double)omega};
    V6* x = nullptr;
    const int rc = cg_compact_solve(
        ctx, st, f, S_FOREGROUND_VEC, B, H, W, 0, max_iter, (double)tol, prm,
        [](const std::vector<int64_t>&) { return (int)GGC_OK; },
        [&](int n_list, dim3 tblk, V6* x0, V6* res) {
            hipLaunchKernelGGL(k_fg_setup, dim3(n_list), tblk, 0, st, H, W, f.ntx, prm.eps_r, prm.omega, f.tiles, bgr, f.field, x0, res,
                               f.part_a, f.part_b);
        },
        x);
    if (rc) return rc;
    const dim3 ogrid(cdiv((int64_t)H * W, FG_THREADS), B);
    hipLaunchKernelGGL(k_fg_output, ogrid, dim3(FG_THREADS), 0, st, H, W, f.ntx, f.nt, f.img, f.tile_slot, bgr, alpha, f.field,
                       x, foreground, rgba, raw_f, raw_b, iters, rel_residual);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
