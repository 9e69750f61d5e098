// ggc_grabcut.hip — C0-C6: GrabCut (reference grabcut.py:81-168, i.e. cv2.grabCut;
// semantics restated from SURVEY.md Appendix A.4, see DESIGN.md "GrabCut").
//
//   init        promotions + degenerate guard (grabcut.py:127-140) or rect mask
//   initGMMs    seeded k-means++ on the uint8 colours (exact integer D^2
//               sampling, 10 assignment steps), GMM fit from exact integer sums
//   calcBeta    exact integer sum of squared neighbour differences
//   n-links     gamma * exp(-beta d^2) quantised to int32 (scale 2^18), computed by the cold graph build
//   x n_iter    assign components | learn GMMs | t-links | max-flow | relabel
//
// Everything that feeds an integer decision is order independent (integer
// atomics) or a fixed IEEE sequence (det_exp / det_log), so the mask equals the
// CPU path bit for bit.
//
// The max-flow itself (lock-free push-relabel on LDS-resident tiles driven by work
// lists, warm-started across the GrabCut iterations) lives in ggc_maxflow.hip.
#include "ggc_gc.h"
#include "ggc_math.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace ggc {

constexpr int NCOMP = 5;
constexpr double CAP_SCALE = 262144.0;   // 2^18
constexpr double GAMMA = 50.0, LAMBDA = 9.0 * GAMMA;
constexpr int CHUNK = 1024;              // pixels per k-means++ sampling chunk


struct Gmm {
    double coef[NCOMP], mean[NCOMP][3], cov[NCOMP][9];
    double inv[NCOMP][3][3], det[NCOMP];
    double isd[NCOMP];                       // 1 / sqrt(det): the per-pixel likelihood multiplies by it (hoisted, same value)
};

// ------------------------------------------------------------------ GMM math
__host__ __device__ inline void gmm_prepare(Gmm& g, int ci, double fix) {   // calcInverseCovAndDeterm
    if (!(g.coef[ci] > 0.0)) return;
    double* c = g.cov[ci];
    double d = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    if (d <= 1e-6 && fix > 0.0) {
        c[0] += fix; c[4] += fix; c[8] += fix;
        d = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    }
    g.det[ci] = d;
    g.isd[ci] = 1.0 / sqrt(d);
    const double id = 1.0 / d;
    g.inv[ci][0][0] = (c[4] * c[8] - c[5] * c[7]) * id;
    g.inv[ci][1][0] = -(c[3] * c[8] - c[5] * c[6]) * id;
    g.inv[ci][2][0] = (c[3] * c[7] - c[4] * c[6]) * id;
    g.inv[ci][0][1] = -(c[1] * c[8] - c[2] * c[7]) * id;
    g.inv[ci][1][1] = (c[0] * c[8] - c[2] * c[6]) * id;
    g.inv[ci][2][1] = -(c[0] * c[7] - c[1] * c[6]) * id;
    g.inv[ci][0][2] = (c[1] * c[5] - c[2] * c[4]) * id;
    g.inv[ci][1][2] = -(c[0] * c[5] - c[2] * c[3]) * id;
    g.inv[ci][2][2] = (c[0] * c[4] - c[1] * c[3]) * id;
}

// What the per-pixel kernels read of a Gmm (no cov, no det), staged in LDS once per block: the 70 doubles of a class are
// then broadcast reads, and no pixel waits for a load of model parameters.
struct GmmEval {
    double coef[NCOMP], mean[NCOMP][3], inv[NCOMP][3][3], isd[NCOMP];
};
constexpr int GMM_EVAL_W = sizeof(GmmEval) / sizeof(double);      // 70
static_assert(sizeof(Gmm) == 120 * sizeof(double) && GMM_EVAL_W == 70, "gmm_stage copies by double index");
static_assert(offsetof(Gmm, coef) == 0 && offsetof(Gmm, mean) == 5 * sizeof(double) && offsetof(Gmm, inv) == 65 * sizeof(double) &&
              offsetof(Gmm, isd) == 115 * sizeof(double), "gmm_stage's source offsets: coef, mean | inv | isd");
static_assert(offsetof(GmmEval, inv) == 20 * sizeof(double) && offsetof(GmmEval, isd) == 65 * sizeof(double), "and its destinations");

// both classes of one image, g = gmm + 2 b; the caller's barrier follows
__device__ __forceinline__ void gmm_stage(GmmEval (&s)[2], const Gmm* __restrict__ g, int tid) {
    if (tid < 2 * GMM_EVAL_W) {
        const int c = tid / GMM_EVAL_W, k = tid % GMM_EVAL_W;
        const int src = k < 20 ? k : (k < 65 ? k + 45 : k + 50);            // coef, mean | inv | isd
        reinterpret_cast<double*>(&s[c])[k] = reinterpret_cast<const double*>(&g[c])[src];
    }
}

// c0 c1 c2: the pixel's colour, loaded once by the caller
__device__ __forceinline__ double gmm_comp(const GmmEval& g, int ci, double c0, double c1, double c2) {
    if (!(g.coef[ci] > 0.0)) return 0.0;
    const double d0 = c0 - g.mean[ci][0], d1 = c1 - g.mean[ci][1], d2 = c2 - g.mean[ci][2];
    const double mult = d0 * (d0 * g.inv[ci][0][0] + d1 * g.inv[ci][1][0] + d2 * g.inv[ci][2][0])
                      + d1 * (d0 * g.inv[ci][0][1] + d1 * g.inv[ci][1][1] + d2 * g.inv[ci][2][1])
                      + d2 * (d0 * g.inv[ci][0][2] + d1 * g.inv[ci][1][2] + d2 * g.inv[ci][2][2]);
    return g.isd[ci] * det_exp(-0.5 * mult);
}
// The mixture likelihood, and in `which` the component gmm_which would name (both from the same five scores).
__device__ __forceinline__ double gmm_total(const GmmEval& g, double c0, double c1, double c2, int& which) {
    double r = 0.0, mx = 0.0;
    which = 0;
    for (int ci = 0; ci < NCOMP; ++ci) {
        const double p = gmm_comp(g, ci, c0, c1, c2);
        r += g.coef[ci] * p;
        if (p > mx) { which = ci; mx = p; }
    }
    return r;
}
__device__ __forceinline__ int gmm_which(const GmmEval& g, double c0, double c1, double c2) {
    int k = 0; double mx = 0.0;
    for (int ci = 0; ci < NCOMP; ++ci) { const double p = gmm_comp(g, ci, c0, c1, c2); if (p > mx) { k = ci; mx = p; } }
    return k;
}

__device__ __forceinline__ bool is_bg(uint8_t m) { return m == GGC_BGD || m == GGC_PR_BGD; }

// ------------------------------------------------------------------ four pixels per thread
// A thread of the dense passes owns a quad: four consecutive pixels whose first flat index b P + p is a multiple of 4.
// The mask bytes of a whole quad are then one dword and its colours three, whatever P is (image b starts at byte b P of
// the mask and 3 b P of the colours, 4-aligned or not); the quad that holds an image's first pixels may begin in the
// previous image and its last may end in the next one, and those two take their own pixels byte by byte, as every quad does
// when the caller's buffer itself is not 4-aligned.  No load leaves [0, B P).
struct Quad {
    size_t g0;          // flat index of the quad's first pixel
    int p0;             // the same within the image: -3 .. P - 1
    unsigned ok;        // bit j: pixel p0 + j belongs to the image
};
__host__ __device__ inline int quads_per_image(int P) { return (P + 3 + 3) / 4; }       // at most 3 foreign pixels in front
__device__ __forceinline__ Quad quad_of(const GcDims& d, int b, int q) {
    const size_t base = (size_t)b * d.P;
    Quad r;
    r.g0 = (base & ~(size_t)3) + 4 * (size_t)q;
    r.p0 = (int)((long long)r.g0 - (long long)base);
    r.ok = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.ok |= (r.p0 + j >= 0 && r.p0 + j < d.P) ? 1u << j : 0u;
    return r;
}
__device__ __forceinline__ bool dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the n bytes per pixel (1: mask, comp; 3: colours) of a quad as n little-endian dwords; bytes of foreign pixels are 0
template <int N>
__device__ __forceinline__ void quad_load(const uint8_t* __restrict__ base, const Quad& q, uint32_t (&w)[N]) {
    const uint8_t* a = base + q.g0 * N;
    if (q.ok == 15u && dword_aligned(base)) {
        const uint32_t* a4 = reinterpret_cast<const uint32_t*>(a);
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = a4[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = 0;
#pragma unroll
        for (int k = 0; k < 4 * N; ++k)
            if ((q.ok >> (k / N)) & 1u) w[k >> 2] |= (uint32_t)a[k] << ((k & 3) * 8);
    }
}
// byte k of a quad's dwords (k = N j + channel, a constant once the loops over j are unrolled)
template <int N>
__device__ __forceinline__ unsigned quad_byte(const uint32_t (&w)[N], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

// one byte per pixel back (mask, comp): only the quad's own pixels are written
__device__ __forceinline__ void quad_store(uint8_t* __restrict__ base, const Quad& q, uint32_t w) {
    uint8_t* a = base + q.g0;
    if (q.ok == 15u && dword_aligned(base)) *reinterpret_cast<uint32_t*>(a) = w;
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if ((q.ok >> j) & 1u) a[j] = (uint8_t)(w >> (8 * j));
    }
}

// ------------------------------------------------------------------ mask init
// bit 0 FGD, 1 BGD, 2 a value outside {0..3}, 3 / 4 the background / foreground class has a pixel (a bad value is in
// neither class: bit 4 then says "FGD or PR_FGD present", which is what k_gc_state's promotion rule reads)
__device__ __forceinline__ int mask_flags(unsigned m) {
    if (m > 3u) return 4;
    return (m == GGC_FGD ? 1 : 0) | (m == GGC_BGD ? 2 : 0) | ((m == GGC_BGD || m == GGC_PR_BGD) ? 8 : 16);
}

__global__ void __launch_bounds__(256) k_gc_flags(GcDims d, const uint8_t* __restrict__ mask, int32_t* __restrict__ flags) {
    // a pixel per thread and pass: by quads the launch was no faster (101 against 95 us under four lanes; its time is not its loads)
    const int b = blockIdx.y;
    int f = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < d.P; p += gridDim.x * blockDim.x)
        f |= mask_flags(mask[(size_t)b * d.P + p]);
    for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o, 64);
    // one atomic per block and only for bits the cell does not hold yet: same-address atomics serialise in L2
    __shared__ int s_f[4];
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        f = s_f[0] | s_f[1] | s_f[2] | s_f[3];
        if (f & ~__hip_atomic_load(&flags[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&flags[b], f);
    }
}

// One quad of the flat [B P] mask per thread (a quad may span images, each pixel takes its own image's flags); a quad whose
// images hold both definite labels is left without reading the mask, and the mask is stored only where it changes.
__global__ void __launch_bounds__(256) k_gc_promote(GcDims d, const int32_t* __restrict__ flags, uint8_t* __restrict__ mask) {
    const size_t BP = (size_t)d.B * d.P, i0 = 4 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i0 >= BP) return;
    Quad q{i0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) q.ok |= i0 + j < BP ? 1u << j : 0u;
    int bj = (int)(i0 / d.P), f[4];
    size_t next = (size_t)(bj + 1) * d.P;           // first flat index of the next image
    int all = 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        while (i0 + j >= next && bj + 1 < d.B) { ++bj; next += d.P; }
        f[j] = flags[bj];
        if ((q.ok >> j) & 1u) all &= f[j];
    }
    if (all == 3) return;
    uint32_t w[1];
    quad_load<1>(mask, q, w);
    uint32_t out = w[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned m = quad_byte<1>(w, j);
        if (!(f[j] & 1) && m == GGC_PR_FGD) out = (out & ~(255u << (8 * j))) | ((uint32_t)GGC_FGD << (8 * j));
        if (!(f[j] & 2) && m == GGC_PR_BGD) out = (out & ~(255u << (8 * j))) | ((uint32_t)GGC_BGD << (8 * j));
    }
    if (out != w[0]) quad_store(mask, q, out);
}

__global__ void __launch_bounds__(256) k_gc_rect(GcDims d, const int32_t* __restrict__ rects, uint8_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)d.B * d.P) return;
    const int b = (int)(i / d.P), p = (int)(i % d.P);
    const int y = p / d.W, x = p % d.W;
    int x0 = rects[4 * b], y0 = rects[4 * b + 1], w = rects[4 * b + 2], h = rects[4 * b + 3];
    if (x0 < 0) { w += x0; x0 = 0; }
    if (y0 < 0) { h += y0; y0 = 0; }
    if (x0 + w > d.W) w = d.W - x0;
    if (y0 + h > d.H) h = d.H - y0;
    mask[i] = (x >= x0 && x < x0 + w && y >= y0 && y < y0 + h) ? GGC_PR_FGD : GGC_BGD;
}

// state[b]: 0 = run, 1 = degenerate / skip
// f1: the flags of the mask as given.  The flags after mode 0's promotion need no second pass over the mask: promotion
// turns an image's probable class into the definite one exactly when the definite one is absent, so afterwards the
// definite label is present iff its class is; every other bit stays.  Modes 1 and 2 do not promote.
__host__ __device__ inline int flags_after_promotion(int f1) { return f1 | ((f1 & 16) ? 1 : 0) | ((f1 & 8) ? 2 : 0); }

__global__ void k_gc_state(int B, int mode, const int32_t* __restrict__ f1, int32_t* __restrict__ state,
                           int32_t* __restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int f2 = mode == 0 ? flags_after_promotion(f1[b]) : f1[b];
    int s = 0;
    if (f2 & 4) { *err = 1; s = 1; }                                   // checkMask
    if (mode == 0 && (f2 & 3) != 3) s = 1;                             // degenerate trimap (grabcut.py:135-140)
    if (mode != 2 && (f2 & 24) != 24) s = 1;                           // a class has no sample
    state[b] = s;
}

// ----------------------------------------------------------- k-means++ (initGMMs)
__device__ __forceinline__ uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct KmState {               // per (image, class)
    uint64_t rng;
    int64_t n;                 // samples in the class
    int32_t K;                 // min(5, n)
    int32_t cen_px[NCOMP];     // pixel index of each k-means++ pick
    double cen[NCOMP][3];
};

// Update D^2 with the newest centre, then per-chunk class counts and D^2 sums.
__global__ void __launch_bounds__(256) k_km_chunks(GcDims d, int k, const uint8_t* __restrict__ img,
                                                   const uint8_t* __restrict__ mask, const int32_t* __restrict__ state,
                                                   const KmState* __restrict__ km, int32_t* __restrict__ d2,
                                                   int64_t* __restrict__ chunk_cnt, int64_t* __restrict__ chunk_d2) {
    // A thread takes a quad of the chunk: mask word, colours and D^2 words are loaded before any is used, and the newest
    // centre of either class (its pixel index and colour) is read once, not per pixel.  A chunk of an image that does not
    // start on a quad boundary overlaps 257 quads; thread 0 takes the last.  A block's sums fit 32 bits (1024 x 3 x 255^2).
    __shared__ int s_cnt[2][4], s_d2[2][4];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    if (state[b]) return;
    const uint8_t* im = img + (size_t)b * d.P * 3;
    const int lo = ch * CHUNK, hi = min(lo + CHUNK, d.P);
    const int first = (int)((((size_t)b * d.P + lo) >> 2) - (((size_t)b * d.P) >> 2));      // the image's quad that holds pixel lo
    const int n_quads = (int)((((size_t)b * d.P + hi - 1) >> 2) - (((size_t)b * d.P) >> 2)) - first + 1;
    bool upd[2] = {false, false};
    int cq[2][3] = {{0, 0, 0}, {0, 0, 0}};
    if (k > 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const KmState& s = km[b * 2 + c];
            upd[c] = k - 1 < s.K;
            if (upd[c]) { const int q = s.cen_px[k - 1]; for (int ch3 = 0; ch3 < 3; ++ch3) cq[c][ch3] = im[3 * q + ch3]; }
        }
    }
    int cnt[2] = {0, 0}, sd[2] = {0, 0};
    for (int t = tid; t < n_quads; t += 256) {
        Quad q = quad_of(d, b, first + t);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (q.p0 + j < lo || q.p0 + j >= hi) q.ok &= ~(1u << j);
        uint32_t mw[1], cw[3];
        quad_load<1>(mask, q, mw);
        if (k > 0) quad_load<3>(img, q, cw);
        int old[4] = {0, 0, 0, 0};
        if (k > 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) if ((q.ok >> j) & 1u) old[j] = d2[q.g0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!((q.ok >> j) & 1u)) continue;
            const int c = is_bg((uint8_t)quad_byte<1>(mw, j)) ? 0 : 1;
            int v = 0;
            if (k > 0) {
                if (upd[c]) {
                    int dd = 0;
#pragma unroll
                    for (int ch3 = 0; ch3 < 3; ++ch3) { const int t3 = (int)quad_byte<3>(cw, 3 * j + ch3) - cq[c][ch3]; dd += t3 * t3; }
                    v = (k == 1) ? dd : min(old[j], dd);
                    if (k == 1 || v != old[j]) d2[q.g0 + j] = v;
                } else v = (k > 1) ? old[j] : d2[q.g0 + j];
            }
            cnt[c] += 1; sd[c] += v;
        }
    }
    for (int c = 0; c < 2; ++c)
        for (int o = 32; o > 0; o >>= 1) { cnt[c] += __shfl_xor(cnt[c], o, 64); sd[c] += __shfl_xor(sd[c], o, 64); }
    if ((tid & 63) == 0) for (int c = 0; c < 2; ++c) { s_cnt[c][tid >> 6] = cnt[c]; s_d2[c][tid >> 6] = sd[c]; }
    __syncthreads();
    if (tid < 2) {
        const size_t o = ((size_t)b * 2 + tid) * d.n_chunks + ch;
        chunk_cnt[o] = s_cnt[tid][0] + s_cnt[tid][1] + s_cnt[tid][2] + s_cnt[tid][3];
        chunk_d2[o] = s_d2[tid][0] + s_d2[tid][1] + s_d2[tid][2] + s_d2[tid][3];
    }
}

__device__ __forceinline__ long long wave_sum64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ long long wave_scan64(long long v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// One wave per (image, class): draw the k-th centre exactly like the oracle's serial walk (first pixel of the class
// whose running count / D^2 sum exceeds the drawn threshold), as prefix scans over 64 chunks / 64 pixels at a time.
__global__ void __launch_bounds__(128) k_km_pick(GcDims d, int k, uint64_t seed, const uint8_t* __restrict__ img,
                                                 const uint8_t* __restrict__ mask, const int32_t* __restrict__ state,
                                                 const int32_t* __restrict__ d2, const int64_t* __restrict__ chunk_cnt,
                                                 const int64_t* __restrict__ chunk_d2, KmState* __restrict__ km) {
    const int b = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (state[b]) return;
    KmState& s = km[b * 2 + c];
    const int64_t* cc = chunk_cnt + ((size_t)b * 2 + c) * d.n_chunks;
    const int64_t* cd = chunk_d2 + ((size_t)b * 2 + c) * d.n_chunks;
    long long n; int K; uint64_t rng;
    if (k == 0) {
        long long part = 0;
        for (int i = lane; i < d.n_chunks; i += 64) part += cc[i];
        n = wave_sum64(part);
        K = n < NCOMP ? (int)n : NCOMP;
        rng = (seed + (uint64_t)b) * 2 + (uint64_t)c + 1;
        if (lane == 0) { s.n = n; s.K = K; s.rng = rng; }
    } else { n = s.n; K = s.K; rng = s.rng; }
    if (k >= K) return;
    long long total = 0;
    if (k > 0) {
        long long part = 0;
        for (int i = lane; i < d.n_chunks; i += 64) part += cd[i];
        total = wave_sum64(part);
    }
    const uint64_t r = splitmix(rng);
    const bool by_d2 = k > 0 && total > 0;
    const long long t = by_d2 ? (long long)(r % (uint64_t)total) : (long long)(r % (uint64_t)n);
    const int64_t* w = by_d2 ? cd : cc;
    // chunk holding the threshold (the last chunk when no prefix exceeds it)
    long long run = 0;
    int ch = d.n_chunks - 1;
    for (int base = 0; base < d.n_chunks; base += 64) {
        const int i = base + lane;
        const long long v = i < d.n_chunks ? (long long)w[i] : 0;
        const long long incl = wave_scan64(v, lane);
        const unsigned long long hit = __ballot(i < d.n_chunks && run + incl > t);
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            ch = base + l;
            run += __shfl(incl - v, l, 64);
            break;
        }
        run += __shfl(incl, 63, 64);
    }
    if (ch == d.n_chunks - 1) {                 // also the fallback: everything before the last chunk
        long long part = 0;
        for (int i = lane; i < d.n_chunks - 1; i += 64) part += w[i];
        run = wave_sum64(part);
    }
    int pick = -1, last = -1;
    const int p_end = min((ch + 1) * CHUNK, d.P);
    for (int base = ch * CHUNK; base < p_end; base += 64) {
        const int p = base + lane;
        const bool mine = p < p_end && (is_bg(mask[(size_t)b * d.P + p]) ? 0 : 1) == c;
        const long long v = mine ? (by_d2 ? (long long)d2[(size_t)b * d.P + p] : 1) : 0;
        const long long incl = wave_scan64(v, lane);
        const unsigned long long any = __ballot(mine);
        if (any) last = base + 63 - __clzll((long long)any);
        const unsigned long long hit = __ballot(mine && run + incl > t);
        if (hit) { pick = base + __ffsll((long long)hit) - 1; break; }
        run += __shfl(incl, 63, 64);
    }
    if (pick < 0) pick = last;                  // cannot happen for consistent sums; keeps the kernel total
    if (lane == 0) {
        s.rng = rng;
        s.cen_px[k] = pick;
        for (int ch3 = 0; ch3 < 3; ++ch3) s.cen[k][ch3] = (double)img[((size_t)b * d.P + pick) * 3 + ch3];
    }
}

// accumulators per (image, class, component): count, 3 sums, 9 products (int64, exact)
constexpr int ACC_W = 13;

// Block-local bins live in LDS as 32-bit counters.  A wave's 64 pixels fall into a handful of (class, component)
// bins, so plain LDS atomics would serialise ~13 deep on one address: every bin slot is kept in BIN_COPIES copies in
// adjacent banks (copy = lane % BIN_COPIES) and summed at the flush.  A block covers BIN_PX pixels per thread, which
// also divides the number of global 64-bit flush atomics.
constexpr int BIN_COPIES = 16, BIN_PX = 4;

__global__ void __launch_bounds__(256) k_km_assign(GcDims d, const uint8_t* __restrict__ img,
                                                   const uint8_t* __restrict__ mask, const int32_t* __restrict__ state,
                                                   const KmState* __restrict__ km, uint8_t* __restrict__ comp,
                                                   unsigned long long* __restrict__ acc, int store_comp) {
    __shared__ unsigned int s_acc[2 * NCOMP * 4 * BIN_COPIES];     // (256 * BIN_PX) x 255 fits 32 bits easily
    __shared__ double s_cen[2][NCOMP][3];                          // the centres of both classes, fetched once per block
    __shared__ int s_K[2];
    const int b = blockIdx.y, tid = threadIdx.x, cp = tid % BIN_COPIES;
    if (state[b]) return;
    // the thread's quad: mask word and colours are on their way before anything is used
    const Quad q = quad_of(d, b, blockIdx.x * 256 + tid);
    uint32_t mw[1], cw[3];
    quad_load<1>(mask, q, mw);
    quad_load<3>(img, q, cw);
    for (int i = tid; i < 2 * NCOMP * 4 * BIN_COPIES; i += 256) s_acc[i] = 0;
    if (tid < 2 * NCOMP * 3) s_cen[tid / (NCOMP * 3)][(tid / 3) % NCOMP][tid % 3] = km[b * 2 + tid / (NCOMP * 3)].cen[(tid / 3) % NCOMP][tid % 3];
    if (tid >= 64 && tid < 66) s_K[tid - 64] = km[b * 2 + tid - 64].K;
    __syncthreads();
    uint32_t cw_out = 0;
#pragma unroll
    for (int j = 0; j < BIN_PX; ++j) {
        if ((q.ok >> j) & 1u) {
            const int c = is_bg((uint8_t)quad_byte<1>(mw, j)) ? 0 : 1;
            const unsigned int v0 = quad_byte<3>(cw, 3 * j), v1 = quad_byte<3>(cw, 3 * j + 1), v2 = quad_byte<3>(cw, 3 * j + 2);
            const double x0 = (double)v0, x1 = (double)v1, x2 = (double)v2;
            int best = 0; double bd = 0.0;
            const int K = s_K[c];
#pragma unroll
            for (int k = 0; k < NCOMP; ++k) {
                const double a0 = x0 - s_cen[c][k][0], a1 = x1 - s_cen[c][k][1], a2 = x2 - s_cen[c][k][2];
                const double dist = (a0 * a0 + a1 * a1) + a2 * a2;
                if (k < K && (k == 0 || dist < bd)) { best = k; bd = dist; }
            }
            cw_out |= (uint32_t)best << (8 * j);
            unsigned int* a = s_acc + (c * NCOMP + best) * 4 * BIN_COPIES + cp;
            atomicAdd(&a[0], 1u); atomicAdd(&a[BIN_COPIES], v0);
            atomicAdd(&a[2 * BIN_COPIES], v1); atomicAdd(&a[3 * BIN_COPIES], v2);
        }
    }
    if (store_comp && q.ok) quad_store(comp, q, cw_out);          // read by k_gmm_accum<0> after the last step only
    __syncthreads();
    for (int i = tid; i < 2 * NCOMP * 4; i += 256) {
        unsigned int v = 0;
#pragma unroll
        for (int k = 0; k < BIN_COPIES; ++k) v += s_acc[i * BIN_COPIES + k];
        if (v) atomicAdd(&acc[((size_t)b * 2 * NCOMP + i / 4) * ACC_W + (i % 4)], (unsigned long long)v);
    }
}

__global__ void k_km_update(int B, const int32_t* __restrict__ state, KmState* __restrict__ km,
                            unsigned long long* __restrict__ acc, int update) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 2 * NCOMP) return;
    const int b = i / (2 * NCOMP), c = (i / NCOMP) % 2, k = i % NCOMP;
    unsigned long long* a = acc + (size_t)i * ACC_W;
    if (!state[b] && update && a[0] > 0)
        for (int ch = 0; ch < 3; ++ch) km[b * 2 + c].cen[k][ch] = (double)(long long)a[1 + ch] / (double)(long long)a[0];
    for (int j = 0; j < ACC_W; ++j) a[j] = 0;
}

// --------------------------------------------------------------- GMM learning
// MODE 0: components already in comp[] (after k-means). MODE 1: assignGMMsComponents first; with `dist` (the labels of
// the previous iteration's max-flow) the pixel first takes that iteration's estimateSegmentation, as k_gc_relabel would
// have: the pass over mask and the launch are this kernel's own, dist is read for probable pixels only and mask is
// stored only where it changes.
template <int MODE>
__global__ void __launch_bounds__(256) k_gmm_accum(GcDims d, const uint8_t* __restrict__ img,
                                                   uint8_t* __restrict__ mask, const int32_t* __restrict__ state,
                                                   const Gmm* __restrict__ gmm, const uint8_t* __restrict__ comp,
                                                   const int32_t* __restrict__ dist, unsigned long long* __restrict__ acc,
                                                   int use_comp) {
    // Block-local bins in LDS as 32-bit counters (256 * BIN_PX pixels x 255^2 < 2^32), products stored once per
    // symmetric pair: 10 LDS atomics per pixel into BIN_COPIES-fold privatised slots (see k_km_assign); the exact
    // 64-bit totals are formed by the global flush.
    constexpr int LW = 10;   // count | 3 sums | xx xy xz yy yz zz
    __shared__ unsigned int s_acc[2 * NCOMP * LW * BIN_COPIES];
    __shared__ GmmEval s_g[2];                                     // MODE 1: both classes' models, fetched once per block
    const int b = blockIdx.y, tid = threadIdx.x, cp = tid % BIN_COPIES;
    if (state[b]) return;
    // the thread's quad: mask word, colours and component bytes are on their way before anything is used
    const Quad q = quad_of(d, b, blockIdx.x * 256 + tid);
    uint32_t mw[1], cw[3], kw[1] = {0};
    quad_load<1>(mask, q, mw);
    quad_load<3>(img, q, cw);
    if (MODE == 0 || use_comp) quad_load<1>(comp, q, kw);
    for (int i = tid; i < 2 * NCOMP * LW * BIN_COPIES; i += 256) s_acc[i] = 0;
    if (MODE == 1) gmm_stage(s_g, gmm + b * 2, tid);
    __syncthreads();
    // the previous cut's labels, for probable pixels only (4 bytes a pixel that definite pixels do not need)
    int dw[4] = {0, 0, 0, 0};
    if (MODE == 1 && dist) {
#pragma unroll
        for (int j = 0; j < BIN_PX; ++j) {
            const unsigned m = quad_byte<1>(mw, j);
            if (((q.ok >> j) & 1u) && (m == GGC_PR_BGD || m == GGC_PR_FGD)) dw[j] = dist[q.g0 + j];
        }
    }
    uint32_t mw_out = mw[0];
#pragma unroll
    for (int j = 0; j < BIN_PX; ++j) {
        if ((q.ok >> j) & 1u) {
            uint8_t m = (uint8_t)quad_byte<1>(mw, j);
            const bool probable = m == GGC_PR_BGD || m == GGC_PR_FGD;
            if (MODE == 1 && dist && probable) {
                m = dw[j] >= DINF ? GGC_PR_FGD : GGC_PR_BGD;
                mw_out = (mw_out & ~(255u << (8 * j))) | ((uint32_t)m << (8 * j));
            }
            const int c = is_bg(m) ? 0 : 1;
            const unsigned int v0 = quad_byte<3>(cw, 3 * j), v1 = quad_byte<3>(cw, 3 * j + 1), v2 = quad_byte<3>(cw, 3 * j + 2);
            int ci;
            if (MODE == 0) ci = (int)quad_byte<1>(kw, j);
            else if (use_comp && probable) ci = (int)(quad_byte<1>(kw, j) >> (4 * c)) & 15;    // k_build_graph's arg-max of this class
            else ci = gmm_which(s_g[c], (double)v0, (double)v1, (double)v2);
            unsigned int* a = s_acc + (c * NCOMP + ci) * LW * BIN_COPIES + cp;
            atomicAdd(&a[0], 1u);
            atomicAdd(&a[1 * BIN_COPIES], v0); atomicAdd(&a[2 * BIN_COPIES], v1); atomicAdd(&a[3 * BIN_COPIES], v2);
            atomicAdd(&a[4 * BIN_COPIES], v0 * v0); atomicAdd(&a[5 * BIN_COPIES], v0 * v1); atomicAdd(&a[6 * BIN_COPIES], v0 * v2);
            atomicAdd(&a[7 * BIN_COPIES], v1 * v1); atomicAdd(&a[8 * BIN_COPIES], v1 * v2); atomicAdd(&a[9 * BIN_COPIES], v2 * v2);
        }
    }
    if (MODE == 1 && mw_out != mw[0]) quad_store(mask, q, mw_out);     // the relabel, stored only where it changes
    __syncthreads();
    for (int i = tid; i < 2 * NCOMP * ACC_W; i += 256) {
        const int bin = i / ACC_W, slot = i % ACC_W;
        int ls = slot;                                   // slots 0..3 map to themselves
        if (slot >= 4) {                                 // 4 + 3 r + c  ->  symmetric pair index
            const int r = (slot - 4) / 3, cc = (slot - 4) % 3;
            const int lo = r < cc ? r : cc, hi = r < cc ? cc : r;
            ls = 4 + (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5));
        }
        unsigned int v = 0;
#pragma unroll
        for (int k = 0; k < BIN_COPIES; ++k) v += s_acc[(bin * LW + ls) * BIN_COPIES + k];
        if (v) atomicAdd(&acc[(size_t)b * 2 * NCOMP * ACC_W + i], (unsigned long long)v);
    }
}

// endLearning: one thread per (image, class)
// fresh: the models hold nothing yet (the fit that follows k-means), so a component without a sample has no previous mean
// and covariance to keep: they are 0, as in the oracle, not what the workspace held.
__global__ void k_gmm_learn(int B, const int32_t* __restrict__ state, unsigned long long* __restrict__ acc,
                            Gmm* __restrict__ gmm, int fresh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 2) return;
    unsigned long long* a = acc + (size_t)i * NCOMP * ACC_W;
    if (!state[i / 2]) {
        Gmm& g = gmm[i];
        long long total = 0;
        for (int ci = 0; ci < NCOMP; ++ci) total += (long long)a[ci * ACC_W];
        for (int ci = 0; ci < NCOMP; ++ci) {
            const long long n = (long long)a[ci * ACC_W];
            if (n == 0) {
                g.coef[ci] = 0.0;
                if (fresh) { for (int r = 0; r < 3; ++r) g.mean[ci][r] = 0.0; for (int r = 0; r < 9; ++r) g.cov[ci][r] = 0.0; }
                continue;
            }
            const double inv_n = 1.0 / (double)n;
            g.coef[ci] = (double)n / (double)total;
            for (int r = 0; r < 3; ++r) g.mean[ci][r] = (double)(long long)a[ci * ACC_W + 1 + r] * inv_n;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c)
                    g.cov[ci][3 * r + c] = (double)(long long)a[ci * ACC_W + 4 + 3 * r + c] * inv_n - g.mean[ci][r] * g.mean[ci][c];
            gmm_prepare(g, ci, 0.01);
        }
    }
    for (int j = 0; j < NCOMP * ACC_W; ++j) a[j] = 0;
}

__global__ void k_gmm_from_model(int B, const double* __restrict__ bgd, const double* __restrict__ fgd, Gmm* __restrict__ gmm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 2) return;
    const double* m = (i & 1 ? fgd : bgd) + (size_t)(i / 2) * 65;
    Gmm& g = gmm[i];
    for (int k = 0; k < NCOMP; ++k) g.coef[k] = m[k];
    for (int k = 0; k < 15; ++k) g.mean[k / 3][k % 3] = m[NCOMP + k];
    for (int k = 0; k < 45; ++k) g.cov[k / 9][k % 9] = m[4 * NCOMP + k];
    for (int ci = 0; ci < NCOMP; ++ci) gmm_prepare(g, ci, 0.0);
}

__global__ void k_gmm_to_model(int B, const int32_t* __restrict__ state, const Gmm* __restrict__ gmm,
                               double* __restrict__ bgd, double* __restrict__ fgd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 2 || state[i / 2]) return;
    double* m = (i & 1 ? fgd : bgd) + (size_t)(i / 2) * 65;
    const Gmm& g = gmm[i];
    for (int k = 0; k < NCOMP; ++k) m[k] = g.coef[k];
    for (int k = 0; k < 15; ++k) m[NCOMP + k] = g.mean[k / 3][k % 3];
    for (int k = 0; k < 45; ++k) m[4 * NCOMP + k] = g.cov[k / 9][k % 9];
}

// ------------------------------------------------------------ beta, n-links, t-links
__device__ __forceinline__ int colour_d2(const uint8_t* a, const uint8_t* b) {
    const int t0 = (int)a[0] - (int)b[0], t1 = (int)a[1] - (int)b[1], t2 = (int)a[2] - (int)b[2];
    return t0 * t0 + t1 * t1 + t2 * t2;
}

__global__ void __launch_bounds__(256) k_beta(GcDims d, const uint8_t* __restrict__ img, unsigned long long* __restrict__ bsum) {
    // A thread takes a quad.  The left neighbour of a pixel is its predecessor in the quad (or the one pixel in front of the
    // quad), and the three upper neighbours of pixel j are pixels j, j + 1, j + 2 of the six that start at p0 - W - 1,
    // wherever the quad lies in its row: 3 dwords and 21 bytes for 16 pairs, all loaded before the first is used, and one
    // division per quad to place it (x and y then step along the row).
    const int b = blockIdx.y, nq = quads_per_image(d.P);
    const uint8_t* im = img + (size_t)b * d.P * 3;
    unsigned long long s = 0;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < nq; g += gridDim.x * blockDim.x) {
        const Quad q = quad_of(d, b, g);
        if (!q.ok) continue;
        uint32_t cw[3];
        quad_load<3>(img, q, cw);
        int nb[7][3];                               // 0: the pixel in front of the quad, 1..6: the row above from p0 - W - 1
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int pi = i == 0 ? q.p0 - 1 : q.p0 - d.W - 2 + i;
            const bool in = pi >= 0 && pi < d.P;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) nb[i][ch] = in ? (int)im[3 * (size_t)(in ? pi : 0) + ch] : 0;
        }
        const int pf = q.p0 < 0 ? 0 : q.p0;         // the quad's first pixel of this image
        int y = pf / d.W, x = pf - y * d.W;
        unsigned int sq = 0;                        // 16 pairs x 3 x 255^2
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!((q.ok >> j) & 1u) ) continue;
            int own[3], left[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                own[ch] = (int)quad_byte<3>(cw, 3 * j + ch);
                left[ch] = j == 0 ? nb[0][ch] : (int)quad_byte<3>(cw, 3 * (j > 0 ? j - 1 : 0) + ch);
            }
            const bool ok4[4] = {x > 0, y > 0 && x > 0, y > 0, y > 0 && x + 1 < d.W};     // left, up-left, up, up-right
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int dd = 0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { const int t = own[ch] - (k == 0 ? left[ch] : nb[j + k][ch]); dd += t * t; }
                sq += ok4[k] ? (unsigned int)dd : 0u;
            }
            if (++x == d.W) { x = 0; ++y; }
        }
        s += sq;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&bsum[b], s);
}

// n-link between two pixels: gamma (over sqrt 2 for a diagonal link) * exp(-beta d^2), quantised.  colour_d2 is symmetric
// in integers, so both ends of a link compute the same capacity.
__device__ __forceinline__ double gc_beta(const GcDims& d, unsigned long long bsum) {
    const long long bs = (long long)bsum;
    return bs > 0 ? 1.0 / (2.0 * (double)bs / (double)(4ll * d.W * d.H - 3ll * d.W - 3ll * d.H + 2)) : 0.0;
}
__device__ __forceinline__ int32_t nlink_cap(double beta, bool diagonal, const uint8_t* a, const uint8_t* b) {
    const double gdiv = GAMMA / sqrt(2.0);
    const double wt = (diagonal ? gdiv : GAMMA) * det_exp(-beta * (double)colour_d2(a, b));
    return (int32_t)rint(wt * CAP_SCALE);
}

// constructGCGraph: t-links cancelled against each other, clamped to +-lambda.  Cold: every pixel computes the capacities
// of its 8 arcs itself (a link that leaves the image is 0) and starts from them (mf_cold_pixel); warm: an open pixel moves
// its terminal balance by the change of its t-link difference (mf_warm_pixel), which is why tws [B][P] keeps the
// difference of the previous build.
__global__ void __launch_bounds__(256) k_build_graph(GcDims d, const uint8_t* __restrict__ img,
                                                     const uint8_t* __restrict__ mask, const int32_t* __restrict__ state,
                                                     const Gmm* __restrict__ gmm, const unsigned long long* __restrict__ bsum,
                                                     int32_t* __restrict__ rc, int32_t* __restrict__ ex,
                                                     int32_t* __restrict__ snk, uint8_t* __restrict__ rmask,
                                                     int32_t* __restrict__ tws, uint8_t* __restrict__ comp, int warm) {
    // One image per grid row and one pixel per thread: open pixels cluster, whole waves of definite pixels leave at once,
    // and the waves that stay are bound by their f64 sequences, which more waves hide better than more pixels per thread.
    // The two models are staged in LDS once per block while the mask byte is on its way; an open pixel then issues its
    // colour and (warm) its tws / ex / snk words together, before the first of them is used.
    __shared__ GmmEval s_g[2];
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (state[b]) return;
    const size_t i = (size_t)b * d.P + (p < d.P ? p : 0);
    const uint8_t m = mask[i];
    gmm_stage(s_g, gmm + b * 2, threadIdx.x);
    __syncthreads();
    if (p >= d.P) return;
    // Warm start, definite pixel: its t-link (+-lambda) is what it was, so its balance is too — and a finished solve leaves
    // no pixel with both excess and sink capacity, so excess and sink link are already what this kernel would write (59 %
    // of the bench's pixels are definite background).
    if (warm && (m == GGC_BGD || m == GGC_FGD)) return;
    const unsigned int v0 = img[i * 3], v1 = img[i * 3 + 1], v2 = img[i * 3 + 2];
    int32_t tw_old = 0, ex_old = 0, snk_old = 0;
    if (warm) { tw_old = tws[i]; ex_old = ex[i]; snk_old = snk[i]; }
    double dv;
    if (m == GGC_BGD) dv = -LAMBDA;
    else if (m == GGC_FGD) dv = LAMBDA;
    else {
        // both classes score all their components here, so the component each class would assign this pixel (gmm_which's
        // rule) is known: one byte, low nibble background, for the next iteration's k_gmm_accum<1>
        int k0, k1;
        const double c0 = (double)v0, c1 = (double)v1, c2 = (double)v2;
        const double from_src = -det_log(gmm_total(s_g[0], c0, c1, c2, k0));
        const double to_snk = -det_log(gmm_total(s_g[1], c0, c1, c2, k1));
        comp[i] = (uint8_t)(k0 | (k1 << 4));
        dv = from_src - to_snk;
        if (dv != dv) dv = 0.0;
        if (dv > LAMBDA) dv = LAMBDA;
        if (dv < -LAMBDA) dv = -LAMBDA;
    }
    const int32_t tw = (int32_t)rint(dv * CAP_SCALE);
    if (warm) mf_warm_pixel(i, tw, tw_old, ex_old, snk_old, ex, snk);
    else {
        const uint8_t* im = img + (size_t)b * d.P * 3;
        const double beta = gc_beta(d, bsum[b]);
        const int y = p / d.W, x = p % d.W;
        int32_t cap[8];
#pragma unroll
        for (int dir = 0; dir < 8; ++dir) {
            const int q = dir_nb(d, y, x, dir);
            cap[dir] = q >= 0 ? nlink_cap(beta, dir >= 4, im + 3 * p, im + 3 * q) : 0;
        }
        mf_cold_pixel(i, tw, cap, rc, ex, snk, rmask);
    }
    tws[i] = tw;
}

// estimateSegmentation: probable pixels take the side of the cut; foreground = cannot reach the sink
__global__ void __launch_bounds__(256) k_gc_relabel(GcDims d, const int32_t* __restrict__ state,
                                                    const int32_t* __restrict__ dist, uint8_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)d.B * d.P || state[i / d.P]) return;
    const uint8_t m = mask[i];
    if (m == GGC_PR_BGD || m == GGC_PR_FGD) mask[i] = dist[i] >= DINF ? GGC_PR_FGD : GGC_PR_BGD;
}

__global__ void __launch_bounds__(256) k_gc_binary(size_t n, const uint8_t* __restrict__ mask, uint8_t* __restrict__ binary) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) binary[i] = (mask[i] == GGC_FGD || mask[i] == GGC_PR_FGD) ? 1 : 0;
}

} // namespace ggc

using namespace ggc;

extern "C" int ggc_grabcut(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* image,
                           uint8_t* mask, const int32_t* rects, double* bgd_model, double* fgd_model,
                           int n_iter, int mode, uint64_t seed, uint8_t* binary) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, (size_t)H * W < (1u << 28), GGC_E_SHAPE, "image too large");
    GGC_REQUIRE(ctx, image && mask, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, mode >= 0 && mode <= 2, GGC_E_INVALID_ARG, "mode must be 0 (mask), 1 (rect) or 2 (eval)");
    GGC_REQUIRE(ctx, mode != 1 || rects, GGC_E_INVALID_ARG, "mode 1 needs rects");
    GGC_REQUIRE(ctx, mode != 2 || (bgd_model && fgd_model), GGC_E_INVALID_ARG, "mode 2 needs both models");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GcDims d{B, H, W, H * W, cdiv((size_t)H * W, CHUNK)};
    const size_t BP = (size_t)B * d.P;

    // the control block, zeroed at the start of every call
    int32_t *f1, *state, *err;          // [B] mask flags as given, [B] 1 = image skipped, [2] error words
    MfControl mf;                       // the max-flow's counters and lists; its error word is err[1]
    const size_t ctl_bytes = carve_scratch(ctx, S_GC_A, [&](Carve& c) {
        f1 = c.take<int32_t>(B); state = c.take<int32_t>(B); err = c.take<int32_t>(2);
        mf = {c.take<int32_t>(B), c.take<int32_t>(8), c.take<int32_t>(2 * (size_t)B), err ? err + 1 : nullptr};
    });
    Gmm* gmm = scratch_t<Gmm>(ctx, S_GC_B, (size_t)B * 2);
    unsigned long long* acc = scratch_t<unsigned long long>(ctx, S_GC_C, (size_t)B * 2 * NCOMP * ACC_W + B);
    uint8_t* comp = scratch_t<uint8_t>(ctx, S_GC_D, BP);
    int32_t* tws = scratch_t<int32_t>(ctx, S_GC_E, BP);          // t-link differences of the last graph build
    int32_t* rc = scratch_t<int32_t>(ctx, S_GC_F, BP * 8);
    int32_t* ex = scratch_t<int32_t>(ctx, S_GC_G, BP * 3);
    uint8_t* rmask = scratch_t<uint8_t>(ctx, S_GC_L, BP);
    if (!ctl_bytes || !gmm || !acc || !comp || !tws || !rc || !ex || !rmask) return GGC_E_OOM;
    int32_t* snk = ex + BP;
    int32_t* dist = ex + 2 * BP;
    unsigned long long* bsum = acc + (size_t)B * 2 * NCOMP * ACC_W;
    GGC_HIP(ctx, hipMemsetAsync(f1, 0, ctl_bytes, st));                  // (f1 starts the control block)
    GGC_HIP(ctx, hipMemsetAsync(acc, 0, sizeof(unsigned long long) * ((size_t)B * 2 * NCOMP * ACC_W + B), st));

    if (mode == 1) {
        int32_t* drects = scratch_t<int32_t>(ctx, S_GC_H, (size_t)B * 4);
        if (!drects) return GGC_E_OOM;
        GGC_HIP(ctx, hipMemcpyAsync(drects, rects, sizeof(int32_t) * B * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gc_rect, dim3(cdiv(BP, 256)), dim3(256), 0, st, d, drects, mask);
    }
    // dense passes: a thread per quad of four pixels (quad_of), one block of 256 per 1024 pixels
    const int quad_blocks = cdiv(quads_per_image(d.P), 256);
    const dim3 red(std::min(cdiv(d.P, 256 * 4), 128), B), dense(quad_blocks, B);
    hipLaunchKernelGGL(k_gc_flags, red, dim3(256), 0, st, d, mask, f1);
    if (mode == 0) hipLaunchKernelGGL(k_gc_promote, dim3(cdiv(cdiv(BP, 4), 256)), dim3(256), 0, st, d, f1, mask);
    hipLaunchKernelGGL(k_gc_state, dim3(cdiv(B, 256)), dim3(256), 0, st, B, mode, f1, state, err);   // derives the flags after promotion
    GGC_LAUNCH_CHECK(ctx);

    if (mode == 2) {
        hipLaunchKernelGGL(k_gmm_from_model, dim3(cdiv(B * 2, 64)), dim3(64), 0, st, B, bgd_model, fgd_model, gmm);
    } else {
        ProfScope prof(ctx, st, "grabcut_init_gmm");
        KmState* km = scratch_t<KmState>(ctx, S_GC_I, (size_t)B * 2);
        int32_t* d2 = scratch_t<int32_t>(ctx, S_GC_J, BP);
        int64_t* chunks = scratch_t<int64_t>(ctx, S_GC_K, (size_t)B * 2 * d.n_chunks * 2);
        if (!km || !d2 || !chunks) return GGC_E_OOM;
        int64_t* chunk_cnt = chunks;
        int64_t* chunk_d2 = chunks + (size_t)B * 2 * d.n_chunks;
        for (int k = 0; k < NCOMP; ++k) {
            hipLaunchKernelGGL(k_km_chunks, dim3(d.n_chunks, B), dim3(256), 0, st, d, k, image, mask, state, km, d2, chunk_cnt, chunk_d2);
            hipLaunchKernelGGL(k_km_pick, dim3(B), dim3(128), 0, st, d, k, (uint64_t)seed, image, mask, state, d2, chunk_cnt, chunk_d2, km);
        }
        for (int it = 0; it < 10; ++it) {
            hipLaunchKernelGGL(k_km_assign, dense, dim3(256), 0, st, d, image, mask, state, km, comp, acc, it == 9 ? 1 : 0);
            hipLaunchKernelGGL(k_km_update, dim3(cdiv(B * 2 * NCOMP, 256)), dim3(256), 0, st, B, state, km, acc, it < 9 ? 1 : 0);
        }
        hipLaunchKernelGGL((k_gmm_accum<0>), dense, dim3(256), 0, st, d, image, mask, state, gmm, comp, (const int32_t*)nullptr, acc, 0);
        hipLaunchKernelGGL(k_gmm_learn, dim3(cdiv(B * 2, 64)), dim3(64), 0, st, B, state, acc, gmm, 1);
    }
    GGC_LAUNCH_CHECK(ctx);

    if (n_iter > 0) {
        hipLaunchKernelGGL(k_beta, red, dim3(256), 0, st, d, image, bsum);
        GGC_LAUNCH_CHECK(ctx);
        int n_open = -1;                // counted by the first solve
        for (int it = 0; it < n_iter; ++it) {
            const bool warm = knobs().mf_warm && it > 0;
            {
                ProfScope prof(ctx, st, "grabcut_gmm");
                // it > 0: relabels from the previous cut first, and probable pixels take their component from the byte the
                // previous build left in comp[] (same models: k_gmm_learn runs after this read)
                hipLaunchKernelGGL((k_gmm_accum<1>), dense, dim3(256), 0, st, d, image, mask, state, gmm, comp,
                                   (const int32_t*)(it > 0 ? dist : nullptr), acc, it > 0 ? 1 : 0);
                hipLaunchKernelGGL(k_gmm_learn, dim3(cdiv(B * 2, 64)), dim3(64), 0, st, B, state, acc, gmm, 0);
                hipLaunchKernelGGL(k_build_graph, dim3(cdiv(d.P, 256), B), dim3(256), 0, st, d, image, mask, state, gmm, bsum, rc, ex, snk, rmask, tws, comp, warm ? 1 : 0);
            }
            GGC_LAUNCH_CHECK(ctx);
            // launches over work lists for the dense phases, one asynchronous launch for each sparse phase
            const int rcode = maxflow(ctx, st, d, state, rc, ex, snk, dist, rmask, mf, !warm, n_open);
            if (rcode) return rcode;
            // estimateSegmentation: the next iteration's k_gmm_accum<1> applies it; the last one has no successor
            if (it == n_iter - 1) hipLaunchKernelGGL(k_gc_relabel, dim3(cdiv(BP, 256)), dim3(256), 0, st, d, state, dist, mask);
            GGC_LAUNCH_CHECK(ctx);
        }
    }
    if (bgd_model && fgd_model)
        hipLaunchKernelGGL(k_gmm_to_model, dim3(cdiv(B * 2, 64)), dim3(64), 0, st, B, state, gmm, bgd_model, fgd_model);
    if (binary) hipLaunchKernelGGL(k_gc_binary, dim3(cdiv(BP, 256)), dim3(256), 0, st, BP, mask, binary);
    GGC_LAUNCH_CHECK(ctx);
    std::vector<int32_t> herr;
    int rcode = read_i32(ctx, st, err, 2, herr);
    if (rcode) return rcode;
    GGC_REQUIRE(ctx, herr[0] == 0, GGC_E_INVALID_ARG, "mask holds values outside {0,1,2,3}");
    GGC_REQUIRE(ctx, herr[1] == 0, GGC_E_DEVICE, "max-flow did not converge (code %d)", herr[1]);
    return GGC_OK;
}
