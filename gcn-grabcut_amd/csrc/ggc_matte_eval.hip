// ggc_matte_eval.hip — R2: the four matte errors of Rhemann et al. (CVPR 2009), SAD, MSE, gradient and connectivity, of
// an 8-bit matte against the true one.  include/ggc.h states the definition; DESIGN.md §5.15 the schedule and the bytes.
//
// Connectivity.  The ten threshold sets S_k are labelled by the union-find of ggc_ccl.h with 4 neighbours, L levels per
// pass (all ten while the maps fit 4 GiB, else one; GGC_MATTE_EVAL_LEVELS = 1, 2, 5 or 10 fixes it) into a parent map of
// L x 4 bytes per pixel: k_me_init, k_me_merge and k_me_area are its init, merge and compress, and
//   k_me_area    holds one count per stretch of up to 1024 pixels that lie in one component (the large one that every
//                low level has) instead of one atomic per run
//   k_me_best    best[b, k] = the largest component of S_k, ties to the smallest raster index
//   k_me_lev     lev = k - 1 at the first k with the pixel outside that component; 10 while there is none
// The whole of S_k is labelled at every level (a component of S_k may be larger than its part that is still alive).
// Sums.  k_me_sums adds n, SAD, SSE and CONN per block in LDS and issues four integer atomics per block.
// Gradient.  k_me_grad stages a 16 x 16 tile of both mattes with a halo of 4 in LDS (border replicated), applies the
// 9-tap Gaussian and its derivative separably in float64 and reduces (m(a) - m(g))^2 over the tile in a fixed LDS tree;
// k_me_grad_sum adds an image's tiles with one wave in a fixed order.  No float atomics: an image's GRAD does not depend
// on the batch.
#include "ggc_internal.h"
#include "ggc_ccl.h"
#include <algorithm>
#include <cmath>

namespace ggc {

namespace {

constexpr int ME_LEVELS = 10;
constexpr int ME_T = 16;                          // gradient tile side
constexpr int ME_R = 4;                           // half-width of the filter
constexpr int ME_TAPS = 2 * ME_R + 1;
constexpr int ME_S = ME_T + 2 * ME_R;             // tile with its halo
constexpr int ME_THREADS = 256;
constexpr int ME_AREA_CHUNKS = 16;                // chunks of 64 pixels that one wave of k_me_area walks
constexpr size_t ME_MAPS_MAX = size_t(4) << 30;   // bytes of parent and area maps up to which all ten levels share a pass
constexpr int ME_SUM_BLOCKS = 120;                // blocks per image of k_me_sums, at most

struct MDims { int B, H, W, P, L; };              // L: levels per labelling pass
struct MTaps { double g[ME_TAPS], d[ME_TAPS]; };  // G / ||G|| and G' / ||G'||: F_x[i][j] = g[i] d[j], F_y[i][j] = d[i] g[j]

__device__ __forceinline__ bool in_level(int a, int g, int k) { return 10 * a >= 255 * k && 10 * g >= 255 * k; }

// The labelling kernels run over the flat index i = ((b L + j) P + p): level k0 + j of image b, pixel p.
__global__ void __launch_bounds__(ME_THREADS) k_me_init(MDims d, int k0, const uint8_t* __restrict__ pred,
                                                        const uint8_t* __restrict__ gt, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ area) {
    const size_t n = (size_t)d.B * d.L * d.P;
    const size_t i = (size_t)blockIdx.x * ME_THREADS + threadIdx.x;
    bool on = false, same_left = false;
    int p = 0;
    if (i < n) {
        const size_t q = i / d.P;
        p = (int)(i - q * d.P);
        const int k = k0 + (int)(q % d.L);
        const size_t px = (q / d.L) * d.P + p;
        on = in_level(pred[px], gt[px], k);
        same_left = on && (p % d.W) > 0 && in_level(pred[px - 1], gt[px - 1], k);
    }
    const int first = ccl_run_first(on, same_left, p);
    if (i < n) {
        parent[i] = on ? first : -1;
        area[i] = 0;
    }
}

__global__ void __launch_bounds__(ME_THREADS) k_me_merge(MDims d, int32_t* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * ME_THREADS + threadIdx.x;
    if (i >= (size_t)d.B * d.L * d.P) return;
    const size_t base = (i / d.P) * d.P;
    int32_t* par = parent + base;
    const int p = (int)(i - base), x = p % d.W;
    if (par[p] < 0) return;
    ccl_merge_pixel<4>(par, p, x, p >= d.W, d.W, i, [par](int q) { return par[q] >= 0; });
}

// A wave walks ME_AREA_CHUNKS consecutive chunks of 64 pixels.  While chunk after chunk lies in one component, the count
// stays in a register and goes to area[root] in one atomic when the component changes or the walk ends: the large
// component that every low level has would otherwise take one atomic per 64 of its pixels, all on one address.
__global__ void __launch_bounds__(ME_THREADS) k_me_area(MDims d, int32_t* __restrict__ parent, int32_t* __restrict__ area) {
    const size_t n = (size_t)d.B * d.L * d.P;
    const int lane = threadIdx.x & 63;
    const size_t i0 = ((size_t)blockIdx.x * (ME_THREADS / 64) + (threadIdx.x >> 6)) * (64 * ME_AREA_CHUNKS);
    long long held = -1;                                    // area index of the component whose count is held; wave-uniform
    int held_cnt = 0;
    for (int c = 0; c < ME_AREA_CHUNKS && i0 + (size_t)c * 64 < n; ++c) {
        const size_t i = i0 + (size_t)c * 64 + lane;
        const bool valid = i < n && parent[i] >= 0;
        bool same_left = false;
        size_t base = 0;
        int r = -1, q = -1;
        if (valid) {
            q = (int)(i / d.P);
            base = (size_t)q * d.P;
            const int p = (int)(i - base);
            same_left = (p % d.W) > 0 && parent[i - 1] >= 0;
            r = ccl_compress(parent + base, p);
        }
        const unsigned long long vmask = __ballot(valid);
        if (!vmask) continue;
        const int lead = __ffsll((long long)vmask) - 1;
        const int r0 = __shfl(r, lead, 64), q0 = __shfl(q, lead, 64);
        if (!__ballot(valid && (r != r0 || q != q0))) {     // one component in this chunk
            const long long key = (long long)q0 * d.P + r0;
            if (key != held) {
                if (held_cnt && lane == 0) atomicAdd(&area[held], held_cnt);
                held = key;
                held_cnt = 0;
            }
            held_cnt += __popcll(vmask);
            continue;
        }
        ccl_count_runs(valid, same_left, vmask, area, base + r);
    }
    if (held_cnt && lane == 0) atomicAdd(&area[held], held_cnt);
}

// best[b, k - 1] = the ccl_best_key of the largest component of S_k; 0 when S_k is empty
__global__ void __launch_bounds__(ME_THREADS) k_me_best(MDims d, int k0, const int32_t* __restrict__ parent,
                                                        const int32_t* __restrict__ area,
                                                        unsigned long long* __restrict__ best) {
    const size_t i = (size_t)blockIdx.x * ME_THREADS + threadIdx.x;
    if (i >= (size_t)d.B * d.L * d.P) return;
    const size_t q = i / d.P;
    const int p = (int)(i - q * d.P);
    if (parent[i] != p) return;                              // roots only
    atomicMax(&best[(q / d.L) * ME_LEVELS + (k0 - 1) + (q % d.L)], ccl_best_key(area[i], p));
}

// one thread per pixel of the batch: the first level of this pass at which the pixel is outside the largest component
__global__ void __launch_bounds__(ME_THREADS) k_me_lev(MDims d, int k0, const int32_t* __restrict__ parent,
                                                       const unsigned long long* __restrict__ best,
                                                       uint8_t* __restrict__ lev) {
    const size_t i = (size_t)blockIdx.x * ME_THREADS + threadIdx.x;
    if (i >= (size_t)d.B * d.P) return;
    if (lev[i] != ME_LEVELS) return;                         // it failed at an earlier level
    const size_t b = i / d.P;
    const int p = (int)(i - b * d.P);
    for (int j = 0; j < d.L; ++j) {
        const unsigned long long bb = best[b * ME_LEVELS + (k0 - 1) + j];
        if (bb == 0 || parent[(b * d.L + j) * d.P + p] != ccl_best_root(bb)) { lev[i] = (uint8_t)(k0 + j - 1); return; }
    }
}

__device__ __forceinline__ int conn_d(int d) { return d >= 383 ? d : 0; }

// n, SAD, SSE, CONN.  grid (blocks, B); a block adds its pixels in LDS and issues four atomics
__global__ void __launch_bounds__(ME_THREADS) k_me_sums(MDims d, const uint8_t* __restrict__ pred,
                                                        const uint8_t* __restrict__ gt, const uint8_t* __restrict__ region,
                                                        const uint8_t* __restrict__ lev,
                                                        unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s[4][ME_THREADS];
    const size_t base = (size_t)blockIdx.y * d.P;
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * ME_THREADS + threadIdx.x; p < d.P; p += (int64_t)gridDim.x * ME_THREADS) {
        if (region && !region[base + p]) continue;
        const int a = pred[base + p], g = gt[base + p], l = lev[base + p];
        const int e = a > g ? a - g : g - a;
        const int c = conn_d(10 * a - 255 * l) - conn_d(10 * g - 255 * l);
        v[0] += 1; v[1] += e; v[2] += e * e; v[3] += c < 0 ? -c : c;
    }
    for (int k = 0; k < 4; ++k) s[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int h = ME_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int k = 0; k < 4; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 4 && s[threadIdx.x][0]) atomicAdd(&sums[(size_t)blockIdx.y * 4 + threadIdx.x], s[threadIdx.x][0]);
}

// (m(a) - m(g))^2 over one 16 x 16 tile.  grid (cdiv(W, 16), cdiv(H, 16), B), 16 x 16 threads
__global__ void __launch_bounds__(ME_THREADS) k_me_grad(MDims d, MTaps t, const uint8_t* __restrict__ pred,
                                                        const uint8_t* __restrict__ gt, const uint8_t* __restrict__ region,
                                                        double* __restrict__ part) {
    __shared__ double s_u[2][ME_S * ME_S];                   // alpha of a and g, tile and halo
    __shared__ double s_h[4][ME_S * ME_T];                   // rows filtered along x: a by g, a by d, g by g, g by d
    __shared__ double s_red[ME_THREADS];
    const int tid = threadIdx.y * ME_T + threadIdx.x;
    const int x0 = blockIdx.x * ME_T, y0 = blockIdx.y * ME_T;
    const size_t base = (size_t)blockIdx.z * d.P;
    for (int e = tid; e < ME_S * ME_S; e += ME_THREADS) {
        int yy = y0 - ME_R + e / ME_S, xx = x0 - ME_R + e % ME_S;
        yy = yy < 0 ? 0 : (yy >= d.H ? d.H - 1 : yy);
        xx = xx < 0 ? 0 : (xx >= d.W ? d.W - 1 : xx);
        const size_t i = base + (size_t)yy * d.W + xx;
        s_u[0][e] = (double)pred[i] / 255.0;
        s_u[1][e] = (double)gt[i] / 255.0;
    }
    __syncthreads();
    for (int e = tid; e < ME_S * ME_T; e += ME_THREADS) {
        const int row = e / ME_T, col = e % ME_T;
        for (int m = 0; m < 2; ++m) {
            const double* u = &s_u[m][row * ME_S + col];
            double hg = 0.0, hd = 0.0;
            for (int j = 0; j < ME_TAPS; ++j) { hg += t.g[j] * u[j]; hd += t.d[j] * u[j]; }
            s_h[2 * m][e] = hg;
            s_h[2 * m + 1][e] = hd;
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    double v = 0.0;
    if (x < d.W && y < d.H && (!region || region[base + (size_t)y * d.W + x])) {
        double mag[2];
        for (int m = 0; m < 2; ++m) {
            double fx = 0.0, fy = 0.0;
            for (int i = 0; i < ME_TAPS; ++i) {
                const int e = (threadIdx.y + i) * ME_T + threadIdx.x;
                fx += t.g[i] * s_h[2 * m + 1][e];
                fy += t.d[i] * s_h[2 * m][e];
            }
            mag[m] = sqrt(fx * fx + fy * fy);
        }
        v = (mag[0] - mag[1]) * (mag[0] - mag[1]);
    }
    s_red[tid] = v;
    __syncthreads();
    for (int k = ME_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) s_red[tid] += s_red[tid + k];
        __syncthreads();
    }
    if (tid == 0) part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s_red[0];
}

// one wave per image: its tiles in a fixed order
__global__ void __launch_bounds__(WAVE) k_me_grad_sum(int nt, const double* __restrict__ part, double* __restrict__ grad) {
    const double* p = part + (size_t)blockIdx.x * nt;
    double v = 0.0;
    for (int k = threadIdx.x; k < nt; k += WAVE) v += p[k];
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_down(v, o, WAVE);
    if (threadIdx.x == 0) grad[blockIdx.x] = v;
}

MTaps make_taps() {
    const double sigma = 1.4, pi = 3.14159265358979323846;
    MTaps t;
    double ng = 0.0, nd = 0.0;
    for (int j = 0; j < ME_TAPS; ++j) {
        const double x = (double)(j - ME_R);
        t.g[j] = std::exp(-x * x / (2.0 * sigma * sigma)) / (sigma * std::sqrt(2.0 * pi));
        t.d[j] = -x * t.g[j] / (sigma * sigma);
        ng += t.g[j] * t.g[j];
        nd += t.d[j] * t.d[j];
    }
    ng = std::sqrt(ng); nd = std::sqrt(nd);                  // ||G (x) G'||_2 = ||G||_2 ||G'||_2
    for (int j = 0; j < ME_TAPS; ++j) { t.g[j] /= ng; t.d[j] /= nd; }
    return t;
}

} // namespace
} // namespace ggc

using namespace ggc;

extern "C" int ggc_matte_errors(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* pred, const uint8_t* gt,
                                const uint8_t* region, uint64_t* sums, double* grad, uint8_t* levels) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (int64_t)H * W < (1ll << 31),
                GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, pred && gt && sums, GGC_E_INVALID_ARG, "null pointer");
    if (B == 0) return GGC_OK;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // all ten levels in one pass is the faster schedule and takes ten times the maps: level by level
    // once they would pass ME_MAPS_MAX.  The results do not depend on the schedule.
    int L = knobs().matte_eval_levels;
    if (L == 0) L = (size_t)B * H * W * 8 * ME_LEVELS <= ME_MAPS_MAX ? ME_LEVELS : 1;
    const MDims d{B, H, W, H * W, L};
    const size_t BP = (size_t)B * d.P, n_lab = BP * L;
    const int ntx = cdiv(W, ME_T), nty = cdiv(H, ME_T), nt = ntx * nty;
    int32_t *parent = nullptr, *area = nullptr;
    unsigned long long* best = nullptr;
    uint8_t* lev = nullptr;
    double* part = nullptr;
    // 8 L + 1 bytes per pixel (the level map only when the caller keeps none), 80 per image, 8 per 16 x 16 tile with grad
    if (!carve_scratch(ctx, S_MATTE_EVAL, [&](Carve& c) {
            parent = c.take<int32_t>(n_lab); area = c.take<int32_t>(n_lab);
            best = c.take<unsigned long long>((size_t)B * ME_LEVELS);
            lev = c.take<uint8_t>(levels ? 0 : BP);
            part = c.take<double>(grad ? (size_t)B * nt : 0);
        }))
        return GGC_E_OOM;
    if (levels) lev = levels;
    ProfScope prof(ctx, st, "matte_errors");
    GGC_HIP(ctx, hipMemsetAsync(best, 0, sizeof(unsigned long long) * B * ME_LEVELS, st));
    GGC_HIP(ctx, hipMemsetAsync(lev, ME_LEVELS, BP, st));
    GGC_HIP(ctx, hipMemsetAsync(sums, 0, sizeof(uint64_t) * 4 * B, st));
    const dim3 blk(ME_THREADS), g_lab(cdiv(n_lab, ME_THREADS)), g_px(cdiv(BP, ME_THREADS));
    const dim3 g_area(cdiv(n_lab, ME_THREADS * ME_AREA_CHUNKS));
    for (int k0 = 1; k0 <= ME_LEVELS; k0 += L) {
        hipLaunchKernelGGL(k_me_init, g_lab, blk, 0, st, d, k0, pred, gt, parent, area);
        hipLaunchKernelGGL(k_me_merge, g_lab, blk, 0, st, d, parent);
        hipLaunchKernelGGL(k_me_area, g_area, blk, 0, st, d, parent, area);
        hipLaunchKernelGGL(k_me_best, g_lab, blk, 0, st, d, k0, parent, area, best);
        hipLaunchKernelGGL(k_me_lev, g_px, blk, 0, st, d, k0, parent, best, lev);
        GGC_LAUNCH_CHECK(ctx);
    }
    const int sum_blocks = std::min(ME_SUM_BLOCKS, cdiv(d.P, ME_THREADS));
    hipLaunchKernelGGL(k_me_sums, dim3(sum_blocks, B), blk, 0, st, d, pred, gt, region, lev,
                       reinterpret_cast<unsigned long long*>(sums));
    if (grad) {
        static const MTaps taps = make_taps();
        hipLaunchKernelGGL(k_me_grad, dim3(ntx, nty, B), dim3(ME_T, ME_T), 0, st, d, taps, pred, gt, region, part);
        hipLaunchKernelGGL(k_me_grad_sum, dim3(B), dim3(WAVE), 0, st, nt, part, grad);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}
