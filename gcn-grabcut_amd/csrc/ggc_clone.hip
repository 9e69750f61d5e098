// ggc_clone.hip — O5, O6: a cut-out placed on a new background.  ggc_composite_over is the integer alpha-over of a BGRA
// cut-out at an offset; ggc_poisson_clone is gradient-domain ("seamless") cloning after Perez, Gangnet and Blake, SIGGRAPH
// 2003, with source or mixed gradients, solved on the device by conjugate gradients with the Jacobi preconditioner.
// include/ggc.h states both rules; DESIGN.md §5.31 the tiling and the bytes.
//
// Layout of the clone.  The tile list, the sums and the scalars are ggc_cg.h's; the compact vector store, the iteration's
// kernels, the stop rule (||r|| <= max(tol ||r_0||, 2.55e-10 sqrt(3 |Omega|))) and the host driver are
// ggc_cg_compact.h's.  Here are the front end (k_clone_front: a byte per target pixel, CL_IN | |N_p| on Omega and 0
// elsewhere, and Omega per tile), the set-up, the output and the policy CloneProblem: three float64 per entry, the byte
// plane as the field, the 4-neighbour Laplacian and the Jacobi preconditioner r / |N_p|, which reads the pixel's own byte
// only: the apply stages the plane with a one-pixel halo, the update reads it directly.  The stencil's membership is never
// stored as a vector.
#include "ggc_cg_compact.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int CL_T = CG_T, CL_THREADS = CG_THREADS;
constexpr int CL_S = CGC_S1;                      // tile with a one-pixel halo
constexpr int CL_IN = 8;                          // the plane's byte: CL_IN | degree on Omega, 0 on the rest of the target
constexpr int CL_DEG = 7;
constexpr int CL_OUTSIDE = 0x80;                  // staged for a pixel outside the target: no link
constexpr int CL_OFFSET_MAX = 32768;

using V3 = CgVec<3>;                              // b, g, r of one pixel

// the clone's policy for ggc_cg_compact.h.  s_f: the plane's bytes staged with row stride S, c the pixel's index in it
struct CloneProblem {
    static constexpr int N = 3, HALO = 1, UPDATE_HALO = 0;
    using Stored = uint8_t;
    using Field = uint8_t;
    static constexpr uint8_t OUTSIDE = CL_OUTSIDE;
    static constexpr double FLOOR = 2.55e-10;                    // 1e-12 of the byte range
    struct Params {};

    static __device__ __forceinline__ bool unknown(int f) { return f & CL_IN; }

    static __device__ __forceinline__ V3 precondition(const V3& r, const uint8_t* s_f, int c, int, Params) {
        const double deg = (double)(s_f[c] & CL_DEG);
        V3 z;
        for (int k = 0; k < 3; ++k) z.v[k] = r.v[k] / deg;
        return z;
    }

    // (A p) at the pixel staged at s_p[c] and s_f[cf]
    static __device__ __forceinline__ V3 apply(const V3* s_p, int c, const uint8_t* s_f, int cf, int, Params) {
        const double deg = (double)(s_f[cf] & CL_DEG);
        const V3 p = s_p[c];
        V3 qi;
        for (int ch = 0; ch < 3; ++ch) {                         // p is 0 off Omega and beyond the target
            const double nsum = ((s_p[c - CL_S].v[ch] + s_p[c - 1].v[ch]) + s_p[c + 1].v[ch]) + s_p[c + CL_S].v[ch];
            qi.v[ch] = deg * p.v[ch] - nsum;
        }
        return qi;
    }
};

// the source pixel of target pixel (y, x) of image b, or -1 where it does not exist.  off = offsets + 2 b
__device__ __forceinline__ int64_t source_index(int y, int x, const int32_t* __restrict__ off, int b, int Hs, int Ws) {
    const int64_t sy = (int64_t)y - off[2 * b], sx = (int64_t)x - off[2 * b + 1];
    if (sy < 0 || sy >= Hs || sx < 0 || sx >= Ws) return -1;
    return ((int64_t)b * Hs + sy) * Ws + sx;
}

// ---------------------------------------------------------------- alpha-over
// grid (cdiv(H*W, 256), B).  out may alias bg: a thread reads and writes its own pixel only
__global__ void __launch_bounds__(CL_THREADS) k_composite_over(int Hs, int Ws, int H, int W, const uint8_t* __restrict__ rgba,
                                                               const uint8_t* bg, const int32_t* __restrict__ off,
                                                               uint8_t* out) {
    const size_t P = (size_t)H * W;
    const size_t j = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (j >= P) return;
    const int b = blockIdx.y;
    const size_t i = (size_t)b * P + j;
    const int64_t s = source_index((int)(j / W), (int)(j % W), off, b, Hs, Ws);
    int c[3] = {bg[3 * i], bg[3 * i + 1], bg[3 * i + 2]};
    if (s >= 0) {
        const int a = rgba[4 * s + 3];
        for (int ch = 0; ch < 3; ++ch) c[ch] = (a * (int)rgba[4 * s + ch] + (255 - a) * c[ch] + 127) / 255;
    }
    for (int ch = 0; ch < 3; ++ch) out[3 * i + ch] = (uint8_t)c[ch];
}

// ---------------------------------------------------------------- the clone's front end
// the byte plane and the per-tile count of Omega.  grid (cdiv(W, 16), cdiv(H, 16), B), 16 x 16 threads
__global__ void __launch_bounds__(CL_THREADS) k_clone_front(int Hs, int Ws, int H, int W, const uint8_t* __restrict__ mask,
                                                            const int32_t* __restrict__ off, uint8_t* __restrict__ plane,
                                                            int32_t* __restrict__ tile_u) {
    __shared__ int s_cnt[CL_THREADS];
    const int tid = threadIdx.y * CL_T + threadIdx.x;
    const int x = blockIdx.x * CL_T + threadIdx.x, y = blockIdx.y * CL_T + threadIdx.y;
    int u = 0;
    if (x < W && y < H) {
        const int b = blockIdx.z;
        const int64_t s = source_index(y, x, off, b, Hs, Ws);
        u = (s >= 0 && mask[s] != 0) ? 1 : 0;
        const int deg = (y > 0) + (x > 0) + (x < W - 1) + (y < H - 1);
        plane[(size_t)b * H * W + (size_t)y * W + x] = (uint8_t)(u ? (CL_IN | deg) : 0);
    }
    count_tile(u, s_cnt, tid, tile_u);
}

// ---------------------------------------------------------------- per listed tile
// x = g, r = b - A g on Omega (exact integers), and the per-tile r . z (part_a), r . r (part_b)
template <bool MIXED>
__global__ void __launch_bounds__(CL_THREADS) k_clone_setup(int Hs, int Ws, int H, int W, int ntx,
                                                            const int2* __restrict__ tiles, const uint8_t* __restrict__ src,
                                                            const uint8_t* __restrict__ tgt, const int32_t* __restrict__ off,
                                                            const uint8_t* __restrict__ plane, V3* __restrict__ x,
                                                            V3* __restrict__ res, double* __restrict__ part_a,
                                                            double* __restrict__ part_b) {
    __shared__ uint8_t s_f[CL_S * CL_S];
    __shared__ uint8_t s_has[CL_S * CL_S];                       // the pixel's source pixel exists
    __shared__ int16_t s_t[CL_S * CL_S][3], s_g[CL_S * CL_S][3];
    __shared__ double s_red[CL_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const int tid = threadIdx.y * CL_T + threadIdx.x;
    const int x0 = t.tx * CL_T - 1, y0 = t.ty * CL_T - 1;
    const size_t base = (size_t)t.b * H * W;
    cgc_stage<CloneProblem>(s_f, CL_S, y0, x0, H, W, plane, base, tid);
    for (int e = tid; e < CL_S * CL_S; e += CL_THREADS) {
        const int yy = y0 + e / CL_S, xx = x0 + e % CL_S;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t s = in ? source_index(yy, xx, off, t.b, Hs, Ws) : -1;
        s_has[e] = s >= 0;
        for (int ch = 0; ch < 3; ++ch) {
            s_t[e][ch] = in ? (int16_t)tgt[3 * (base + (size_t)yy * W + xx) + ch] : (int16_t)0;
            s_g[e][ch] = s >= 0 ? (int16_t)src[3 * s + ch] : (int16_t)0;
        }
    }
    __syncthreads();
    const int c = (threadIdx.y + 1) * CL_S + threadIdx.x + 1;
    const int f = s_f[c];
    double va = 0.0, vb = 0.0;
    if (f & CL_IN) {                                             // outside the target the staged byte is CL_OUTSIDE
        const int nb[4] = {c - CL_S, c - 1, c + 1, c + CL_S};
        const double deg = (double)(f & CL_DEG);
        V3 r, xi;
        for (int ch = 0; ch < 3; ++ch) {
            const int gp = s_g[c][ch], tp = s_t[c][ch];
            int rhs = 0, ag = (f & CL_DEG) * gp;
            for (int k = 0; k < 4; ++k) {
                const int fq = s_f[nb[k]];
                if (fq == CL_OUTSIDE) continue;                  // q is not in N_p
                const int tq = s_t[nb[k]][ch];
                const int ds = s_has[nb[k]] ? gp - s_g[nb[k]][ch] : 0;
                int v = ds;
                if constexpr (MIXED) {
                    const int dt = tp - tq;
                    if (abs(dt) > abs(ds)) v = dt;
                }
                rhs += v;
                if (fq & CL_IN) ag -= s_g[nb[k]][ch]; else rhs += tq;
            }
            r.v[ch] = (double)(rhs - ag);
            xi.v[ch] = (double)gp;
        }
        const size_t j = (size_t)blockIdx.x * CL_THREADS + tid;
        x[j] = xi;
        res[j] = r;
        for (int k = 0; k < 3; ++k) { va += r.v[k] * (r.v[k] / deg); vb += r.v[k] * r.v[k]; }
    }
    tile_partials(va, vb, s_red, tid, part_a, part_b);
}

// the outputs over the whole frame.  grid (cdiv(H*W, 256), B).  An Omega pixel of an image that was not solved (Omega the
// whole target: no listed tile) takes the source's colour, the plain paste.
__global__ void __launch_bounds__(CL_THREADS) k_clone_output(int Hs, int Ws, int H, int W, int ntx, int nt,
                                                             const CgImage* __restrict__ img,
                                                             const int32_t* __restrict__ tile_slot,
                                                             const uint8_t* __restrict__ src, const uint8_t* __restrict__ tgt,
                                                             const int32_t* __restrict__ off, const uint8_t* __restrict__ plane,
                                                             const V3* __restrict__ x, uint8_t* __restrict__ composite,
                                                             double* __restrict__ raw, int* __restrict__ iters,
                                                             double* __restrict__ rel) {
    const size_t P = (size_t)H * W;
    const size_t j = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (iters) iters[b] = img[b].iters;
        if (rel) rel[b] = img[b].rel;
    }
    if (j >= P) return;
    const size_t i = (size_t)b * P + j;
    uint8_t col[3] = {tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2]};
    double f[3] = {(double)col[0], (double)col[1], (double)col[2]};
    if (plane[i] & CL_IN) {
        const int y = (int)(j / W), xx = (int)(j % W);
        const int slot = tile_slot[(size_t)b * nt + (y / CL_T) * ntx + xx / CL_T];
        if (slot >= 0) {
            const V3 v = x[(size_t)slot * CL_THREADS + (y % CL_T) * CL_T + (xx % CL_T)];
            for (int ch = 0; ch < 3; ++ch) f[ch] = v.v[ch];
        } else {
            const int64_t s = source_index(y, xx, off, b, Hs, Ws);   // exists: the pixel is in Omega
            for (int ch = 0; ch < 3; ++ch) f[ch] = (double)src[3 * s + ch];
        }
        for (int ch = 0; ch < 3; ++ch) {
            const double c = f[ch] > 0.0 ? (f[ch] > 255.0 ? 255.0 : f[ch]) : 0.0;   // a NaN gives 0
            col[ch] = (uint8_t)floor(c + 0.5);
        }
    }
    for (int ch = 0; ch < 3; ++ch) {
        if (composite) composite[3 * i + ch] = col[ch];
        if (raw) raw[3 * i + ch] = f[ch];
    }
}

bool sides_ok(int B, int Hs, int Ws, int H, int W) {
    return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && Hs >= 1 && Ws >= 1 && Hs <= 32768 &&
           Ws <= 32768;
}

} // namespace
} // namespace ggc

using namespace ggc;

extern "C" int ggc_composite_over(ggc_ctx* ctx, ggc_stream stream, int B, int Hs, int Ws, const uint8_t* rgba, int H, int W,
                                  const uint8_t* background, const int32_t* offsets, uint8_t* out) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, sides_ok(B, Hs, Ws, H, W), GGC_E_SHAPE, "bad shape B=%d source %dx%d background %dx%d", B, Hs, Ws, H, W);
    GGC_REQUIRE(ctx, B == 0 || (rgba && background && offsets && out), GGC_E_INVALID_ARG, "null pointer");
    if (B == 0) return GGC_OK;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "composite_over");
    hipLaunchKernelGGL(k_composite_over, dim3(cdiv((int64_t)H * W, CL_THREADS), B), dim3(CL_THREADS), 0, st, Hs, Ws, H, W,
                       rgba, background, offsets, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

extern "C" int ggc_poisson_clone(ggc_ctx* ctx, ggc_stream stream, int B, int Hs, int Ws, const uint8_t* source,
                                 const uint8_t* mask, int H, int W, const uint8_t* target, const int32_t* offsets, int mixed,
                                 int max_iter, float tol, uint8_t* composite, double* raw, int32_t* n_omega, int32_t* iters,
                                 double* rel_residual) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, sides_ok(B, Hs, Ws, H, W), GGC_E_SHAPE, "bad shape B=%d source %dx%d target %dx%d", B, Hs, Ws, H, W);
    GGC_REQUIRE(ctx, composite || raw || n_omega || iters || rel_residual, GGC_E_INVALID_ARG,
                "null pointer: no output asked for");
    GGC_REQUIRE(ctx, B == 0 || (source && mask && target && offsets), GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, mixed == 0 || mixed == 1, GGC_E_INVALID_ARG, "clone mixed %d is neither 0 nor 1", mixed);
    GGC_REQUIRE(ctx, max_iter >= 1 && max_iter <= 100000, GGC_E_INVALID_ARG, "clone max_iter %d outside 1..100000", max_iter);
    GGC_REQUIRE(ctx, std::isfinite(tol) && tol >= 1e-12f && tol < 1.0f, GGC_E_INVALID_ARG,
                "clone tol %g outside [1e-12, 1)", (double)tol);
    if (B == 0) return GGC_OK;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    CgCompactFrame<CloneProblem> f;                              // the field is the byte plane: 1 byte per pixel
    if (!cg_compact_frame(ctx, S_CLONE, B, H, W, f)) return GGC_E_OOM;
    ProfScope prof(ctx, st, "poisson_clone");
    hipLaunchKernelGGL(k_clone_front, dim3(f.ntx, f.nty, B), dim3(CL_T, CL_T), 0, st, Hs, Ws, H, W, mask, offsets, f.field,
                       f.tile_u);
    GGC_LAUNCH_CHECK(ctx);

    // the offsets come to the host with the counts, under the one synchronisation of the tile list.  An image whose Omega
    // is the whole target is not solved; the CG vectors take 120 bytes per entry
    std::vector<int32_t> off(2 * (size_t)B), host_n(B);
    GGC_HIP(ctx, hipMemcpyAsync(off.data(), offsets, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    V3* x = nullptr;
    const int rc = cg_compact_solve(
        ctx, st, f, S_CLONE_VEC, B, H, W, (int64_t)H * W, max_iter, (double)tol, CloneProblem::Params{},
        [&](const std::vector<int64_t>& u_count) {
            for (size_t k = 0; k < off.size(); ++k)
                GGC_REQUIRE(ctx, off[k] >= -CL_OFFSET_MAX && off[k] <= CL_OFFSET_MAX, GGC_E_INVALID_ARG,
                            "clone offset %d of image %d outside +-%d", off[k], (int)(k / 2), CL_OFFSET_MAX);
            for (int b = 0; b < B; ++b) host_n[b] = (int32_t)u_count[b];
            if (n_omega)
                GGC_HIP(ctx, hipMemcpyAsync(n_omega, host_n.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
            return (int)GGC_OK;
        },
        [&](int n_list, dim3 tblk, V3* x0, V3* res) {
            if (mixed)
                hipLaunchKernelGGL(k_clone_setup<true>, dim3(n_list), tblk, 0, st, Hs, Ws, H, W, f.ntx, f.tiles, source, target,
                                   offsets, f.field, x0, res, f.part_a, f.part_b);
            else
                hipLaunchKernelGGL(k_clone_setup<false>, dim3(n_list), tblk, 0, st, Hs, Ws, H, W, f.ntx, f.tiles, source, target,
                                   offsets, f.field, x0, res, f.part_a, f.part_b);
        },
        x);
    if (rc) return rc;
    if (composite || raw || iters || rel_residual) {
        const dim3 ogrid(cdiv((int64_t)H * W, CL_THREADS), B);
        hipLaunchKernelGGL(k_clone_output, ogrid, dim3(CL_THREADS), 0, st, Hs, Ws, H, W, f.ntx, f.nt, f.img, f.tile_slot, source,
                           target, offsets, f.field, x, composite, raw, iters, rel_residual);
        GGC_LAUNCH_CHECK(ctx);
    }
    return GGC_OK;
}
