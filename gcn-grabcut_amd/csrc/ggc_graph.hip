// ggc_graph.hip — G2-G8: region statistics, node features, region-adjacency +
// non-local colour edges, automatic prior (reference graph_builder.py:190-454).
//
// Batched over B images with data-dependent node counts.  Design points:
//  * region sums follow np.bincount(weights=...) exactly — float64 running sums
//    in raster order, cast to float32 — by giving every region a group of 16
//    lanes, one per accumulator, that walks the region's bounding box in raster
//    order (SLIC regions are compact, so the box is a few hundred pixels).
//    Deterministic, no float atomics.
//  * np.unique(lo*N+hi, return_counts=True): an image's pairs and their counts
//    are collected in one CU's LDS (a hash table of integer atomics: exact,
//    order independent) and ranked through an N x N bitset, which yields them
//    sorted by code (k_region_scan, k_topology, k_emit).  Images that do not
//    fit the tables, small batches and GGC_GRAPH_ONCHIP=0 take the form this
//    replaced: a dense per-image N x N int32 matrix in HBM, read back row-major
//    with wave ballot/prefix compaction (256 images x 700^2 x 4 B = 0.5 GB).
//  * the non-local k-NN (argpartition): on chip a thread per node that keeps
//    its k best in registers, dense a wave per node over an LDS row of
//    distances with k rounds of wave arg-min; ties go to the lowest index.
//  * ggc_graph_count synchronises twice (node counts, pair counts) so that the
//    packed outputs can be sized exactly; ggc_graph_fill only copies.
#include "ggc_internal.h"
#include "ggc_math.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace ggc {

constexpr int NL_BIT = 1 << 30;

struct GDims { int B, H, W, Nmax, conn, k_nl; };

// Per-region record produced by k_stats (all float32, as the reference stores them).
struct RegionStats {
    float cnt, safe;
    float mlab[3], slab[3], mhsv[3];
    float cy, cx;         // _region_statistics centroids (f32 y/H accumulated in f64)
    float pcy, pcx;       // compute_auto_prior centroids (f64 y/H)
    float bpx, mgrad, mgn, area, border;
};

// ---- K1: bounding boxes, frame counts, per-image max gradient
constexpr int BBOX_ROWS = 32;
__global__ void __launch_bounds__(256) k_bbox(GDims d, const int32_t* __restrict__ seg, const float* __restrict__ grad,
                                              int4* __restrict__ bbox, int32_t* __restrict__ border,
                                              uint32_t* __restrict__ gmax) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int b = blockIdx.z;
    float gv = -INFINITY;
    const int lane = threadIdx.x & 63;
    // a block walks BBOX_ROWS rows: 4 rows per block made the launch itself (134 k tiny blocks) the cost
    for (int y = blockIdx.y * BBOX_ROWS + (threadIdx.x >> 6); y < min((int)(blockIdx.y + 1) * BBOX_ROWS, d.H); y += 4) {
    const bool valid = x < d.W;
    int s = -1;
    size_t p = 0;
    if (valid) {
        p = (size_t)b * d.H * d.W + (size_t)y * d.W + x;
        s = seg[p];
        const int mult = (y == 0) + (y == d.H - 1) + (x == 0) + (x == d.W - 1);
        if (mult) atomicAdd(&border[(size_t)b * d.Nmax + s], mult);
        gv = fmaxf(gv, grad[p]);
    }
    // A region's pixels inside this wave's 64-pixel row segment form runs; a run's x extremes are its two ends,
    // so its first lane issues the four min/max atomics for the whole run (4 per run instead of 4 per outline pixel).
    const int s_left = __shfl_up(s, 1, 64);
    const unsigned long long vmask = __ballot(valid);
    const unsigned long long starts = __ballot(valid && (lane == 0 || s_left != s));
    if (valid && ((starts >> lane) & 1ull)) {
        const unsigned long long stop = (starts | ~vmask) >> lane >> 1;
        const int len = stop ? __ffsll((long long)stop) : 64 - lane;
        int4* bb = bbox + (size_t)b * d.Nmax + s;
        // ... and a run whose neighbour row holds a same-region run reaching at least as far cannot set that extreme:
        // only "corner" runs reach the L2 atomic units (their throughput is what bounds this kernel)
        const int xe = x + len - 1;
        const bool up = y > 0, dn = y + 1 < d.H;
        const bool up_s = up && seg[p - d.W] == s, dn_s = dn && seg[p + d.W] == s;
        const bool up_e = up && seg[p - d.W + len - 1] == s, dn_e = dn && seg[p + d.W + len - 1] == s;
        if (!up_s && !up_e) atomicMin(&bb->x, y);
        if (!dn_s && !dn_e) atomicMax(&bb->y, y + 1);
        const bool left_cov = x > 0 && ((up_s && seg[p - d.W - 1] == s) || (dn_s && seg[p + d.W - 1] == s));
        const bool right_cov = xe + 1 < d.W && ((up_e && seg[p - d.W + len] == s) || (dn_e && seg[p + d.W + len] == s));
        if (!left_cov) atomicMin(&bb->z, x);
        if (!right_cov) atomicMax(&bb->w, xe + 1);
    }
    }
    for (int o = 32; o > 0; o >>= 1) gv = fmaxf(gv, __shfl_xor(gv, o, 64));
    if ((threadIdx.x & 63) == 0 && gv > -INFINITY) atomicMax(&gmax[b], f2ord(gv));
}

__global__ void k_bbox_init(size_t n, int4* bbox) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bbox[i] = make_int4(INT32_MAX, 0, INT32_MAX, 0);
}

// ---- K2: region statistics, a group of SG lanes per region, raster order, f64 sums
// The sums must be float64 running sums in raster order (= np.bincount(weights=...)).  Only the order of additions
// within ONE accumulator is fixed; the 15 rounded accumulators of a region are independent of each other, so each gets
// a lane of the region's group, and finding the members is separate from folding them.  The group walks the region's
// bounding box row by row in chunks of SG consecutive pixels (one coalesced label read for the four groups of a wave),
// a ballot gives the chunk's members in ascending x, the member lanes put their pixel's values into LDS, and then every
// lane of the group walks the set bits and adds its own accumulator's addend: the same additions in the same order.
// cnt and the boundary count are sums of 1.0 and are taken as popcounts.  (One lane per region with the rows of the
// wave's 64 boxes staged in LDS was a 1 ms latency chain per wave at 1.5 waves per SIMD.)
constexpr int SG = 16;                 // lanes per region
constexpr int SG_REGIONS = 64 / SG;    // regions per wave
constexpr int SG_COLS = 2 * SG;        // box columns whose (double)x/W is tabulated per group ...
constexpr int SG_TAB = SG_COLS + SG;   // ... plus one chunk of spill slots for boxes wider than that

// order the wave's own LDS writes before its reads (a block is one wave)
__device__ __forceinline__ void stats_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) k_stats(GDims d, const int32_t* __restrict__ seg,
                                              const int32_t* __restrict__ n_nodes,
                                              const float* __restrict__ lab, const float* __restrict__ hsv,
                                              const float* __restrict__ grad, const int4* __restrict__ bbox,
                                              const int32_t* __restrict__ border,
                                              const uint32_t* __restrict__ gmax, RegionStats* __restrict__ out) {
    // 3.8 KB of LDS and, by amdgpu_waves_per_eu, 64 VGPRs: the block is one wave, and what bounds the kernel is how many
    // waves have loads in flight (8 per SIMD this way; 0.94 ms per batch of 256 at 6, 0.85 at 8)
    __shared__ float s_f[9 * 64];                                   // chunk values: lab 0-2, hsv 3-5, grad 6, grad/max 7, (float)x/W 8
    __shared__ double s_d[SG_REGIONS * SG_TAB];                     // (double)x/W per group
    const int b = blockIdx.y, lane = threadIdx.x;
    const int N = n_nodes[b];
    const int r0 = blockIdx.x * SG_REGIONS;
    if (r0 >= N) return;
    const int g = lane / SG, li = lane % SG;
    const int r = r0 + g;
    const bool live = r < N;
    const int H = d.H, W = d.W;
    const size_t P = (size_t)H * W;
    const int32_t* sg = seg + (size_t)b * P;
    const float* lb = lab + (size_t)b * P * 3;
    const float* hv = hsv + (size_t)b * P * 3;
    const float* gr = grad + (size_t)b * P;
    const int4 bb = live ? bbox[(size_t)b * d.Nmax + r] : make_int4(INT32_MAX, 0, INT32_MAX, 0);
    const float gden = (float)((double)ord2f(gmax[b]) + 1e-6);
    const bool boxed = bb.y > bb.x && bb.w > bb.z;
    const int xa = boxed ? bb.z & ~(SG - 1) : 0;                    // chunks start at multiples of SG: aligned label reads
    const int ya = boxed ? bb.x : 0;

    // This lane's accumulator: 0-2 lab, 3-5 lab^2, 6-8 hsv, 9 (float)y/H, 10 (float)x/W, 11 (double)y/H, 12 (double)x/W,
    // 13 grad, 14 grad/max; lane 15 folds nothing that is kept.  The addend of a member at chunk position `bit` is
    // s_f[fbase + bit] (squared for 3-5), s_d[doff + bit], or the row's quotient, which the lane keeps in a register.
    const bool sq = li >= 3 && li < 6;
    const bool is_row = li == 9 || li == 11;
    const bool is_d = li == 12;
    const int frow = li < 3 ? li : li < 9 ? li - 3 : li == 10 ? 8 : li == 13 ? 6 : li == 14 ? 7 : 0;
    const int fbase = frow * 64 + g * SG;

    // (double)x/W of the first SG_COLS columns of the box, once per region instead of once per chunk
#pragma unroll
    for (int q = 0; q < SG_COLS / SG; ++q) s_d[g * SG_TAB + q * SG + li] = (double)(xa + q * SG + li) / (double)W;
    stats_lds_sync();

    // Everything a chunk needs from memory, for every lane inside the box whether it turns out to be a member or not:
    // one trip to memory per chunk, and the next chunk's trip is under way while this one is folded.
    struct Chunk { int lbl, up, dn, lf, rt; float l0, l1, l2, h0, h1, h2, gv; };
    auto fetch = [&](int y, int xc, bool active) {
        Chunk c{-1, -1, -1, -1, -1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int x = xc + li;
        if (active && x >= bb.z && x < bb.w) {                       // the box lies inside the image
            const size_t p = (size_t)y * W + x;
            c.lbl = sg[p];
            if (y > 0) c.up = sg[p - W];
            if (y < H - 1) c.dn = sg[p + W];
            if (x > 0) c.lf = sg[p - 1];
            if (x < W - 1) c.rt = sg[p + 1];
            c.l0 = lb[3 * p]; c.l1 = lb[3 * p + 1]; c.l2 = lb[3 * p + 2];
            c.h0 = hv[3 * p]; c.h1 = hv[3 * p + 1]; c.h2 = hv[3 * p + 2];
            c.gv = gr[p];
        }
        return c;
    };

    double acc = 0.0, rowq = 0.0;         // rowq: (float)y/H (lane 9) or (double)y/H of row y_q
    int cnt = 0, nb = 0, y_q = -1;        // cnt, nb: sums of 1.0, exact in any order
    int y_n = ya, xc_n = xa;              // the chunk being fetched
    bool act_n = boxed;
    Chunk nxt = fetch(y_n, xc_n, act_n);
    while (__any(act_n)) {
        const Chunk c = nxt;
        const int y = y_n, xc = xc_n, x = xc + li;
        const bool active = act_n;
        if (act_n) {
            xc_n += SG;
            if (xc_n >= bb.w) { xc_n = xa; ++y_n; act_n = y_n < bb.y; }
        }
        nxt = fetch(y_n, xc_n, act_n);
        const bool mem = active && c.lbl == r;                       // r >= 0, lanes outside the box hold -1
        const unsigned long long bal = __ballot(mem);
        if (bal) {
            const uint32_t gm = (uint32_t)(bal >> (g * SG)) & ((1u << SG) - 1u);
            const int kc = min((xc - xa) / SG, SG_COLS / SG);
            if (active && y != y_q) { y_q = y; rowq = li == 9 ? (double)((float)y / (float)H) : (double)y / (double)H; }
            bool bnd = false;
            if (mem) {
                // find_boundaries(mode="inner"): 4-neighbourhood max != min, and label != 0; no neighbour outside the image
                int mx = r, mn = r;
                if (y > 0) { mx = max(mx, c.up); mn = min(mn, c.up); }
                if (y < H - 1) { mx = max(mx, c.dn); mn = min(mn, c.dn); }
                if (x > 0) { mx = max(mx, c.lf); mn = min(mn, c.lf); }
                if (x < W - 1) { mx = max(mx, c.rt); mn = min(mn, c.rt); }
                bnd = mx != mn && r != 0;
                s_f[0 * 64 + lane] = c.l0; s_f[1 * 64 + lane] = c.l1; s_f[2 * 64 + lane] = c.l2;
                s_f[3 * 64 + lane] = c.h0; s_f[4 * 64 + lane] = c.h1; s_f[5 * 64 + lane] = c.h2;
                s_f[6 * 64 + lane] = c.gv;
                s_f[7 * 64 + lane] = c.gv / gden;
                s_f[8 * 64 + lane] = (float)x / (float)W;
                if (kc == SG_COLS / SG) s_d[g * SG_TAB + SG_COLS + li] = (double)x / (double)W;   // beyond the table: spill slot
            }
            cnt += __popc(gm);
            nb += __popc((uint32_t)(__ballot(bnd) >> (g * SG)) & ((1u << SG) - 1u));
            stats_lds_sync();
            const int doff = g * SG_TAB + kc * SG;
            // members of the chunk in ascending x: every lane of the group adds its own addend, so each accumulator sees
            // the region's pixels in raster order
            for (uint32_t m = gm; m; m &= m - 1) {
                const int bit = __ffs(m) - 1;
                const float v = s_f[fbase + bit];
                const double dv = s_d[doff + bit];
                acc += is_row ? rowq : is_d ? dv : (double)(sq ? v * v : v);
            }
            stats_lds_sync();             // the chunk's values are consumed before the next chunk overwrites them
        }
    }

    double a[SG];
#pragma unroll
    for (int j = 0; j < SG - 1; ++j) a[j] = __shfl(acc, g * SG + j, 64);
    if (!live || li != 0) return;
    RegionStats s;
    s.cnt = (float)(double)cnt;
    s.safe = s.cnt > 1.0f ? s.cnt : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = (float)a[c] / s.safe;
        const float sq2 = (float)a[3 + c] / s.safe;
        float v = sq2 - m * m;
        if (!(v > 0.0f)) v = (v != v) ? v : 0.0f;
        s.mlab[c] = m; s.slab[c] = sqrtf(v);
        s.mhsv[c] = (float)a[6 + c] / s.safe;
    }
    s.cy = (float)a[9] / s.safe; s.cx = (float)a[10] / s.safe;
    s.pcy = (float)(a[11] / (double)s.safe); s.pcx = (float)(a[12] / (double)s.safe);
    s.bpx = (float)(double)nb;
    s.mgrad = (float)a[13] / s.safe;
    s.mgn = (float)a[14] / s.safe;
    s.area = s.cnt / (float)((double)H * (double)W);
    s.border = (float)border[(size_t)b * d.Nmax + r];
    out[(size_t)b * d.Nmax + r] = s;
}

// ---- K3: adjacency counts into the dense matrix (integer atomics: exact)
__global__ void __launch_bounds__(256) k_adj(GDims d, const int32_t* __restrict__ seg, int32_t* __restrict__ dense) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= d.W || y >= d.H) return;
    const int b = blockIdx.z;
    const int32_t* sg = seg + (size_t)b * d.H * d.W;
    int32_t* m = dense + (size_t)b * d.Nmax * d.Nmax;
    const int a = sg[(size_t)y * d.W + x];
    auto link = [&](int u, int v) {
        if (u != v) atomicAdd(&m[(size_t)min(u, v) * d.Nmax + max(u, v)], 1);
    };
    if (x + 1 < d.W) link(a, sg[(size_t)y * d.W + x + 1]);
    if (y + 1 < d.H) link(a, sg[(size_t)(y + 1) * d.W + x]);
    if (d.conn == 8 && x + 1 < d.W && y + 1 < d.H) {
        link(a, sg[(size_t)(y + 1) * d.W + x + 1]);
        link(sg[(size_t)y * d.W + x + 1], sg[(size_t)(y + 1) * d.W + x]);
    }
}

// ---- K6: non-local k nearest neighbours in mean-Lab (one wave per node)
__global__ void __launch_bounds__(256) k_knn(GDims d, const int32_t* __restrict__ n_nodes,
                                             const RegionStats* __restrict__ st, int32_t* __restrict__ dense) {
    extern __shared__ float drow[];               // 4 waves x Nmax distances
    const int b = blockIdx.y;
    const int N = n_nodes[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    if (!(d.k_nl > 0 && N > d.k_nl + 1) || i >= N) return;   // graph_builder.py:291
    float* dr = drow + (size_t)wave * d.Nmax;
    const RegionStats* s = st + (size_t)b * d.Nmax;
    int32_t* m = dense + (size_t)b * d.Nmax * d.Nmax;
    const float l0 = s[i].mlab[0], l1 = s[i].mlab[1], l2 = s[i].mlab[2];
    for (int j = lane; j < N; j += 64) {
        const float dx = l0 - s[j].mlab[0], dy = l1 - s[j].mlab[1], dz = l2 - s[j].mlab[2];
        float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        const int lo = min(i, j), hi = max(i, j);
        if (j == i || (m[(size_t)lo * d.Nmax + hi] & ~NL_BIT) != 0) dist = INFINITY;
        dr[j] = dist;
    }
    // (same wave wrote and reads dr: no barrier needed beyond the implicit wave order)
    __builtin_amdgcn_wave_barrier();
    for (int t = 0; t < d.k_nl; ++t) {
        float best = NAN; int bj = INT32_MAX;       // arg-min over non-taken entries (NaN = taken)
        for (int j = lane; j < N; j += 64) {
            const float v = dr[j];
            if (v == v && (bj == INT32_MAX || v < best)) { best = v; bj = j; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            const bool take = (oj != INT32_MAX) && (bj == INT32_MAX || ov < best || (ov == best && oj < bj));
            if (take) { best = ov; bj = oj; }
        }
        if (bj == INT32_MAX) break;
        if (lane == 0) {
            dr[bj] = NAN;
            if (isfinite(best)) atomicOr(&m[(size_t)min(i, bj) * d.Nmax + max(i, bj)], NL_BIT);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- K4/K7: per-row counts of adjacency / non-local entries (wave per row)
__global__ void __launch_bounds__(256) k_rowcount(GDims d, const int32_t* __restrict__ n_nodes,
                                                  const int32_t* __restrict__ dense,
                                                  int32_t* __restrict__ cnt_adj, int32_t* __restrict__ cnt_nl) {
    const int b = blockIdx.y;
    const int N = n_nodes[b];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int32_t* row = dense + ((size_t)b * d.Nmax + i) * d.Nmax;
    int ca = 0, cn = 0;
    for (int j = i + 1 + lane; j < N; j += 64) {
        const int v = row[j];
        ca += (v & ~NL_BIT) != 0;
        cn += (v & NL_BIT) != 0;
    }
    for (int o = 32; o > 0; o >>= 1) { ca += __shfl_xor(ca, o, 64); cn += __shfl_xor(cn, o, 64); }
    if (lane == 0) { cnt_adj[(size_t)b * d.Nmax + i] = ca; cnt_nl[(size_t)b * d.Nmax + i] = cn; }
}

// per-image exclusive scans of the two row-count arrays; totals[b] = {n_adj, n_nl, max shared}
__global__ void __launch_bounds__(256) k_rowscan(GDims d, const int32_t* __restrict__ n_nodes,
                                                 int32_t* __restrict__ cnt_adj, int32_t* __restrict__ cnt_nl,
                                                 int32_t* __restrict__ totals) {
    __shared__ int pa[256], pn[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = n_nodes[b];
    int32_t* ca = cnt_adj + (size_t)b * d.Nmax;
    int32_t* cn = cnt_nl + (size_t)b * d.Nmax;
    const int chunk = (N + 255) / 256;
    const int beg = min(tid * chunk, N), end = min(beg + chunk, N);
    int sa = 0, sn = 0;
    for (int i = beg; i < end; ++i) { sa += ca[i]; sn += cn[i]; }
    pa[tid] = sa; pn[tid] = sn;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int va = tid >= off ? pa[tid - off] : 0, vn = tid >= off ? pn[tid - off] : 0;
        __syncthreads();
        pa[tid] += va; pn[tid] += vn;
        __syncthreads();
    }
    int ra = tid ? pa[tid - 1] : 0, rn = tid ? pn[tid - 1] : 0;
    for (int i = beg; i < end; ++i) { const int a = ca[i], n = cn[i]; ca[i] = ra; cn[i] = rn; ra += a; rn += n; }
    if (tid == 255) { totals[3 * b] = pa[255]; totals[3 * b + 1] = pn[255]; }
}

// ---- K5: ordered extraction of the pair lists (wave per row), raw pair features
struct PairOut {
    int32_t* lo; int32_t* hi; float* de; float* dxy; float* shared; float* gc;
};

__global__ void __launch_bounds__(256) k_extract(GDims d, const int32_t* __restrict__ n_nodes,
                                                 const int32_t* __restrict__ dense,
                                                 const RegionStats* __restrict__ st,
                                                 const int32_t* __restrict__ off_adj, const int32_t* __restrict__ off_nl,
                                                 const int64_t* __restrict__ pair_ptr /*[B+1] adj+nl pairs*/,
                                                 const int32_t* __restrict__ totals, PairOut out,
                                                 uint32_t* __restrict__ maxima /*[B,5]: de_adj,dxy_adj,de_nl,dxy_nl,shared*/) {
    const int b = blockIdx.y;
    const int N = n_nodes[b];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int32_t* row = dense + ((size_t)b * d.Nmax + i) * d.Nmax;
    const RegionStats* s = st + (size_t)b * d.Nmax;
    const int64_t base_adj = pair_ptr[b] + off_adj[(size_t)b * d.Nmax + i];
    const int64_t base_nl = pair_ptr[b] + totals[3 * b] + off_nl[(size_t)b * d.Nmax + i];
    int run_a = 0, run_n = 0;
    float mde_a = 0.f, mdx_a = 0.f, mde_n = 0.f, mdx_n = 0.f;
    int msh = 0;
    const RegionStats si = s[i];
    for (int j0 = i + 1; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const int v = j < N ? row[j] : 0;
        const bool isa = (v & ~NL_BIT) != 0, isn = (v & NL_BIT) != 0;
        const unsigned long long ba = __ballot(isa), bn = __ballot(isn);
        const unsigned long long lt = (1ull << lane) - 1ull;
        if (isa || isn) {
            const RegionStats sj = s[j];
            const float dx = si.mlab[0] - sj.mlab[0], dy = si.mlab[1] - sj.mlab[1], dz = si.mlab[2] - sj.mlab[2];
            const float de = sqrtf((dx * dx + dy * dy) + dz * dz);
            const float cy = si.cy - sj.cy, cx = si.cx - sj.cx;
            const float dxy = sqrtf(cy * cy + cx * cx);
            const float gc = fabsf(si.mgn - sj.mgn);
            if (isa) {
                const int64_t q = base_adj + run_a + __popcll(ba & lt);
                out.lo[q] = i; out.hi[q] = j; out.de[q] = de; out.dxy[q] = dxy; out.gc[q] = gc;
                out.shared[q] = (float)(v & ~NL_BIT);
                mde_a = fmaxf(mde_a, de); mdx_a = fmaxf(mdx_a, dxy); msh = max(msh, v & ~NL_BIT);
            }
            if (isn) {
                const int64_t q = base_nl + run_n + __popcll(bn & lt);
                out.lo[q] = i; out.hi[q] = j; out.de[q] = de; out.dxy[q] = dxy; out.gc[q] = gc;
                out.shared[q] = 0.0f;
                mde_n = fmaxf(mde_n, de); mdx_n = fmaxf(mdx_n, dxy);
            }
        }
        run_a += __popcll(ba); run_n += __popcll(bn);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mde_a = fmaxf(mde_a, __shfl_xor(mde_a, o, 64)); mdx_a = fmaxf(mdx_a, __shfl_xor(mdx_a, o, 64));
        mde_n = fmaxf(mde_n, __shfl_xor(mde_n, o, 64)); mdx_n = fmaxf(mdx_n, __shfl_xor(mdx_n, o, 64));
        msh = max(msh, __shfl_xor(msh, o, 64));
    }
    if (lane == 0) {
        uint32_t* mx = maxima + (size_t)b * 5;
        if (run_a) { atomicMax(&mx[0], f2ord(mde_a)); atomicMax(&mx[1], f2ord(mdx_a)); atomicMax(&mx[4], (uint32_t)msh); }
        if (run_n) { atomicMax(&mx[2], f2ord(mde_n)); atomicMax(&mx[3], f2ord(mdx_n)); }
    }
}

// ---- on-chip topology: the same pair lists without the dense matrix
// An image's region topology fits in one CU's LDS.  k_region_scan reads the label map and the gradient once and keeps the
// boxes, the frame counts and an open-addressing table of (lo*Nmax+hi, shared-boundary count) in LDS; all of it is integer
// min/max/add or a float max, so the order of the pixels does not matter.  k_topology then ranks the pairs through an
// N x N bitset, which is the dense matrix's row-major walk (the order np.unique gives) at one bit per entry, runs the k-NN
// on mean-Lab staged in LDS, and writes both sorted lists; k_emit computes the pair features from the lists.
// What does not fit (N, k, or the number of distinct pairs) goes through the dense kernels above.
constexpr int OC_NMAX = 704;                        // regions per image (a multiple of 64)
constexpr int OC_WPR = OC_NMAX / 32;                // bitset words per row
constexpr int OC_SLOT_BITS = 13;
constexpr int OC_SLOTS = 1 << OC_SLOT_BITS;         // pair table slots ...
constexpr int OC_PAIRS = OC_SLOTS / 4 * 3;          // ... of which at most this many are taken (distinct adjacent pairs per image)
constexpr int OC_KMAX = 8;                          // non-local neighbours per node
constexpr int OC_NL = OC_NMAX * OC_KMAX;            // non-local pairs per image
constexpr int OC_THREADS = 1024;
constexpr int OC_WAVES = OC_THREADS / 64;
constexpr int OC_BANDS_MAX = 8;                     // workgroups that share one image's rows when the batch is small
constexpr int OC_MIN_BATCH = 24;                    // smaller batches keep the dense kernels
constexpr uint32_t OC_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t OC_NONE = 0xFFFFu;
constexpr size_t OC_LDS_SCAN = (size_t)OC_SLOTS * 8 + (size_t)OC_NMAX * 20 + 64;
constexpr size_t OC_LDS_TOPO = (size_t)OC_NMAX * OC_WPR * 4 + (size_t)OC_NMAX * 12 + (size_t)(OC_NMAX + 1) * 4 +
                               (size_t)OC_PAIRS * 4 + (size_t)OC_NL * 2 + 256;
static_assert(OC_LDS_SCAN <= 160 * 1024 && OC_LDS_TOPO <= 160 * 1024, "the on-chip tables must fit one CU's LDS");
static_assert((size_t)OC_NMAX * OC_NMAX < OC_EMPTY && OC_NMAX < (int)OC_NONE && OC_NMAX <= OC_THREADS, "pair keys and node ids must stay below their empty marks");

struct OnchipLists {
    uint32_t* band_key; uint32_t* band_cnt;   // [B][bands][OC_PAIRS] unsorted (key, count) of each band of rows
    int32_t* band_n;                          // [B][bands]
    uint32_t* adj_key; uint32_t* adj_cnt;     // [B][OC_PAIRS] ascending by key, counts summed over the bands
    uint32_t* nl_key;                         // [B][OC_NL] ascending by key
};

__global__ void __launch_bounds__(OC_THREADS) k_region_scan(GDims d, int bands, const int32_t* __restrict__ seg,
                                                            const float* __restrict__ grad, int4* __restrict__ bbox,
                                                            int32_t* __restrict__ border, uint32_t* __restrict__ gmax,
                                                            uint32_t* __restrict__ maxima, int32_t* __restrict__ totals,
                                                            OnchipLists L) {
    __shared__ uint32_t s_key[OC_SLOTS], s_cnt[OC_SLOTS];
    __shared__ int s_y0[OC_NMAX], s_y1[OC_NMAX], s_x0[OC_NMAX], s_x1[OC_NMAX], s_border[OC_NMAX];
    __shared__ uint32_t s_gmax;
    __shared__ int s_new, s_out, s_over;
    const int band = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int H = d.H, W = d.W, Nmax = d.Nmax;
    for (int i = tid; i < OC_SLOTS; i += OC_THREADS) { s_key[i] = OC_EMPTY; s_cnt[i] = 0; }
    for (int i = tid; i < Nmax; i += OC_THREADS) { s_y0[i] = INT32_MAX; s_y1[i] = 0; s_x0[i] = INT32_MAX; s_x1[i] = 0; s_border[i] = 0; }
    if (tid == 0) { s_gmax = 0; s_new = 0; s_out = 0; s_over = 0; }
    __syncthreads();

    auto insert = [&](uint32_t key, int n) {
        if (__hip_atomic_load(&s_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;   // the batch takes the dense path anyway
        uint32_t h = (key * 2654435761u) >> (32 - OC_SLOT_BITS);
        for (int t = 0; t < OC_SLOTS; ++t) {
            const uint32_t prev = atomicCAS(&s_key[h], OC_EMPTY, key);
            if (prev == OC_EMPTY && atomicAdd(&s_new, 1) >= OC_PAIRS) atomicOr(&s_over, 1);
            if (prev == OC_EMPTY || prev == key) { atomicAdd(&s_cnt[h], (uint32_t)n); return; }
            h = (h + 1) & (OC_SLOTS - 1);
        }
        atomicOr(&s_over, 1);
    };
    // lanes next to each other that hold the same key form a run; its first lane adds the run's length once
    auto add_runs = [&](uint32_t key) {
        const uint32_t kl = __shfl_up(key, 1, 64);
        const bool has = key != OC_EMPTY;
        const unsigned long long hm = __ballot(has);
        if (!hm) return;
        const unsigned long long starts = __ballot(has && (lane == 0 || kl != key));
        if (has && ((starts >> lane) & 1ull)) {
            const unsigned long long stop = (starts | ~hm) >> lane >> 1;
            insert(key, stop ? __ffsll((long long)stop) : 64 - lane);
        }
    };
    auto key_of = [&](bool on, int u, int v) {
        return on && u != v ? (uint32_t)(min(u, v) * Nmax + max(u, v)) : OC_EMPTY;
    };

    const int rows_per = (H + bands - 1) / bands;
    const int y_beg = min(band * rows_per, H), y_end = min(y_beg + rows_per, H);
    const int nseg = (W + 63) / 64;
    const int items = (y_end - y_beg) * nseg;
    const int32_t* sg = seg + (size_t)b * H * W;
    const float* gr = grad + (size_t)b * H * W;
    // what one 64-pixel row segment needs from memory; three segments of loads are in flight per wave while one is folded.
    // A wave takes every OC_WAVES-th segment of the band; its place (row py, segment ps of the row) is kept in scalar
    // registers and stepped.  The kernel is bound by instruction issue (about 300 wave instructions per segment), not by
    // these loads: one segment in flight measured the same (profiles/r17_graph_onchip.txt).
    struct Seg { int y, x, s, rt, dn, dr; float g; };
    int py = y_beg, ps = __builtin_amdgcn_readfirstlane(wave);
    auto settle = [&]() { while (ps >= nseg && py < y_end) { ps -= nseg; ++py; } };
    auto fetch = [&]() {
        settle();
        Seg c{py, ps * 64 + lane, -1, -1, -1, -1, -INFINITY};
        if (py < y_end && c.x < W) {
            const size_t p = (size_t)c.y * W + c.x;
            c.s = sg[p];
            c.g = gr[p];
            if (c.x + 1 < W) c.rt = sg[p + 1];
            if (c.y + 1 < H) {
                c.dn = sg[p + W];
                if (d.conn == 8 && c.x + 1 < W) c.dr = sg[p + W + 1];
            }
        }
        ps += OC_WAVES;
        return c;
    };
    float gv = -INFINITY;
    Seg nxt = fetch(), nxt2 = fetch(), nxt3 = fetch();
    for (int it = wave; it < items; it += OC_WAVES) {
        const Seg c = nxt;
        nxt = nxt2; nxt2 = nxt3;
        nxt3 = fetch();
        const int y = c.y, x = c.x;
        bool valid = x < W;
        if (valid && (unsigned)c.s >= (unsigned)Nmax) { atomicOr(&s_over, 1); valid = false; }   // not a label of this batch
        const int s = valid ? c.s : -1;
        if (valid) {
            const int mult = (y == 0) + (y == H - 1) + (x == 0) + (x == W - 1);
            if (mult) atomicAdd(&s_border[s], mult);
            gv = fmaxf(gv, c.g);
        }
        // a region's pixels inside the segment form runs; a run's first lane folds the whole run into the region's box
        const int s_left = __shfl_up(s, 1, 64);
        const unsigned long long vmask = __ballot(valid);
        const unsigned long long starts = __ballot(valid && (lane == 0 || s_left != s));
        if (valid && ((starts >> lane) & 1ull)) {
            const unsigned long long stop = (starts | ~vmask) >> lane >> 1;
            const int len = stop ? __ffsll((long long)stop) : 64 - lane;
            atomicMin(&s_y0[s], y); atomicMax(&s_y1[s], y + 1);
            atomicMin(&s_x0[s], x); atomicMax(&s_x1[s], x + len);
        }
        // the links of k_adj
        const bool rt = valid && x + 1 < W, dn = valid && y + 1 < H;
        add_runs(key_of(rt, s, c.rt));
        add_runs(key_of(dn, s, c.dn));
        if (d.conn == 8) {
            add_runs(key_of(rt && dn, s, c.dr));
            add_runs(key_of(rt && dn, c.rt, c.dn));
        }
    }
    for (int o = 32; o > 0; o >>= 1) gv = fmaxf(gv, __shfl_xor(gv, o, 64));
    if (lane == 0 && gv > -INFINITY) atomicMax(&s_gmax, f2ord(gv));
    __syncthreads();

    // one band per image owns the image's words and stores them; several bands merge into words the host has initialised
    const bool over = s_over != 0;
    if (bands == 1) {
        for (int i = tid; i < Nmax; i += OC_THREADS) {
            bbox[(size_t)b * Nmax + i] = make_int4(s_y0[i], s_y1[i], s_x0[i], s_x1[i]);
            border[(size_t)b * Nmax + i] = s_border[i];
        }
        if (tid < 5) maxima[(size_t)b * 5 + tid] = 0;
        if (tid < 3) totals[3 * b + tid] = tid == 2 ? (int)over : 0;
        if (tid == 0) gmax[b] = s_gmax;
    } else {
        for (int i = tid; i < Nmax; i += OC_THREADS) {
            if (s_y1[i] > 0) {
                int4* bb = bbox + (size_t)b * Nmax + i;
                atomicMin(&bb->x, s_y0[i]); atomicMax(&bb->y, s_y1[i]);
                atomicMin(&bb->z, s_x0[i]); atomicMax(&bb->w, s_x1[i]);
            }
            if (s_border[i]) atomicAdd(&border[(size_t)b * Nmax + i], s_border[i]);
        }
        if (tid == 0) {
            atomicMax(&gmax[b], s_gmax);
            if (over) atomicOr(&totals[3 * b + 2], 1);
        }
    }
    const size_t base = ((size_t)b * bands + band) * OC_PAIRS;
    if (!over)
        for (int i = tid; i < OC_SLOTS; i += OC_THREADS)
            if (s_key[i] != OC_EMPTY) {
                const int q = atomicAdd(&s_out, 1);      // below OC_PAIRS: s_new never passed it
                L.band_key[base + q] = s_key[i];
                L.band_cnt[base + q] = s_cnt[i];
            }
    if (tid == 0) L.band_n[(size_t)b * bands + band] = over ? 0 : s_new;
}

// exclusive scan of one value per thread over the workgroup; `total` is the sum.  part: OC_WAVES + 1 words of LDS.
__device__ __forceinline__ int oc_block_scan(int v, int* part, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                  // part may still be read from the scan before
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int pre = 0, sum = 0;
    for (int w = 0; w < OC_WAVES; ++w) { const int p = part[w]; if (w < wave) pre += p; sum += p; }
    total = sum;
    return pre + inc - v;
}

// set bits of a bitset row in the columns [a, e)
__device__ __forceinline__ int oc_row_popc(const uint32_t* row, int a, int e) {
    int n = 0;
    if (e <= a) return 0;
    for (int w = a >> 5; w <= (e - 1) >> 5; ++w) {
        uint32_t m = row[w];
        if (w == a >> 5) m &= ~0u << (a & 31);
        if (w == (e - 1) >> 5) m &= ~0u >> (31 - ((e - 1) & 31));
        n += __popc(m);
    }
    return n;
}

// Row i's k nearest nodes in mean-Lab among those that are neither i nor adjacent to it: one thread walks j upwards with
// the K best so far sorted in registers.  A distance enters only where it is strictly smaller, so equal distances stay in
// ascending j: the first k_nl entries are k_knn's k rounds of lexicographic (distance, j) arg-min.  Every thread reads the
// same l[j] (an LDS broadcast), and no step crosses lanes; a wave per row spent most of its instructions on the arg-min
// butterflies.  NaN and infinite distances never enter, as k_knn never emits them.
template <int K>
__device__ __forceinline__ void oc_knn_row(int i, int N, int k_nl, const float* l0, const float* l1, const float* l2,
                                           const uint32_t* row, uint16_t* choice) {
    float bd[K]; int bj[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = INFINITY; bj[t] = (int)OC_NONE; }
    const float a0 = l0[i], a1 = l1[i], a2 = l2[i];
    uint32_t word = 0;
    for (int j = 0; j < N; ++j) {
        if ((j & 31) == 0) word = row[j >> 5];
        const float dx = a0 - l0[j], dy = a1 - l1[j], dz = a2 - l2[j];
        const float v = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (j != i && !((word >> (j & 31)) & 1u) && v < bd[K - 1]) {
#pragma unroll
            for (int t = K - 1; t > 0; --t) {
                const bool shift = v < bd[t - 1], here = v < bd[t];
                bj[t] = shift ? bj[t - 1] : here ? j : bj[t];
                bd[t] = shift ? bd[t - 1] : here ? v : bd[t];
            }
            if (v < bd[0]) { bd[0] = v; bj[0] = j; }
        }
    }
#pragma unroll
    for (int t = 0; t < K; ++t)
        if (t < k_nl && bj[t] != (int)OC_NONE) choice[t] = (uint16_t)bj[t];
}

// ---- sorted adjacent pairs, non-local k nearest neighbours in mean-Lab, sorted non-local pairs (workgroup per image)
__global__ void __launch_bounds__(OC_THREADS) k_topology(GDims d, int bands, const int32_t* __restrict__ n_nodes,
                                                         const RegionStats* __restrict__ st, OnchipLists L,
                                                         int32_t* __restrict__ totals) {
    __shared__ uint32_t s_bits[OC_NMAX * OC_WPR];
    __shared__ float s_l0[OC_NMAX], s_l1[OC_NMAX], s_l2[OC_NMAX];
    __shared__ int s_off[OC_NMAX + 1];
    __shared__ uint32_t s_sum[OC_PAIRS];
    __shared__ uint16_t s_choice[OC_NL];
    __shared__ int s_part[OC_WAVES + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (totals[3 * b + 2]) return;                    // the scan met what the tables do not hold
    const int N = n_nodes[b], Nmax = d.Nmax;
    const RegionStats* s = st + (size_t)b * Nmax;
    for (int i = tid; i < N * OC_WPR; i += OC_THREADS) s_bits[i] = 0;
    for (int i = tid; i < OC_PAIRS; i += OC_THREADS) s_sum[i] = 0;
    for (int i = tid; i < N; i += OC_THREADS) { s_l0[i] = s[i].mlab[0]; s_l1[i] = s[i].mlab[1]; s_l2[i] = s[i].mlab[2]; }
    __syncthreads();
    // adjacency as a symmetric bitset; labels from N on belong to no node (the dense rows stop at N too)
    for (int g = 0; g < bands; ++g) {
        const size_t base = ((size_t)b * bands + g) * OC_PAIRS;
        const int n = L.band_n[(size_t)b * bands + g];
        for (int e = tid; e < n; e += OC_THREADS) {
            const uint32_t key = L.band_key[base + e];
            const int lo = key / Nmax, hi = key % Nmax;
            if (hi >= N) continue;
            atomicOr(&s_bits[lo * OC_WPR + (hi >> 5)], 1u << (hi & 31));
            atomicOr(&s_bits[hi * OC_WPR + (lo >> 5)], 1u << (lo & 31));
        }
    }
    __syncthreads();
    // row i of the dense matrix holds its pairs (i, j > i) in ascending j: a pair's place is its row's offset plus the
    // row's bits below it
    int n_adj;
    {
        const int c = tid < N ? oc_row_popc(s_bits + tid * OC_WPR, tid + 1, N) : 0;
        const int off = oc_block_scan(c, s_part, n_adj);
        if (tid < N) s_off[tid] = off;
    }
    if (n_adj > OC_PAIRS) {                           // the bands' union is larger than any one band's table
        if (tid == 0) totals[3 * b + 2] = 1;
        return;
    }
    __syncthreads();
    for (int g = 0; g < bands; ++g) {
        const size_t base = ((size_t)b * bands + g) * OC_PAIRS;
        const int n = L.band_n[(size_t)b * bands + g];
        for (int e = tid; e < n; e += OC_THREADS) {
            const uint32_t key = L.band_key[base + e];
            const int lo = key / Nmax, hi = key % Nmax;
            if (hi >= N) continue;
            const int q = s_off[lo] + oc_row_popc(s_bits + lo * OC_WPR, lo + 1, hi);
            atomicAdd(&s_sum[q], L.band_cnt[base + e]);
            L.adj_key[(size_t)b * OC_PAIRS + q] = key;      // two bands that saw the pair store the same word
        }
    }
    __syncthreads();
    for (int q = tid; q < n_adj; q += OC_THREADS) L.adj_cnt[(size_t)b * OC_PAIRS + q] = s_sum[q];

    // k-NN: thread per row
    const bool knn = d.k_nl > 0 && N > d.k_nl + 1;    // graph_builder.py:291
    int n_nl = 0;
    if (knn) {
        for (int i = tid; i < N * OC_KMAX; i += OC_THREADS) s_choice[i] = (uint16_t)OC_NONE;
        __syncthreads();
        if (tid < N) {
            if (d.k_nl <= 4) oc_knn_row<4>(tid, N, d.k_nl, s_l0, s_l1, s_l2, s_bits + tid * OC_WPR, s_choice + tid * OC_KMAX);
            else oc_knn_row<OC_KMAX>(tid, N, d.k_nl, s_l0, s_l1, s_l2, s_bits + tid * OC_WPR, s_choice + tid * OC_KMAX);
        }
        __syncthreads();
        // both ends may have chosen each other: the pairs pass through a bitset of their own, which also sorts them
        for (int i = tid; i < N * OC_WPR; i += OC_THREADS) s_bits[i] = 0;
        __syncthreads();
        for (int e = tid; e < N * d.k_nl; e += OC_THREADS) {
            const int i = e / d.k_nl, j = s_choice[i * OC_KMAX + e % d.k_nl];
            if (j == (int)OC_NONE) continue;
            const int lo = min(i, j), hi = max(i, j);
            atomicOr(&s_bits[lo * OC_WPR + (hi >> 5)], 1u << (hi & 31));
        }
        __syncthreads();
        const int c = tid < N ? oc_row_popc(s_bits + tid * OC_WPR, 0, N) : 0;
        int q = oc_block_scan(c, s_part, n_nl);
        if (tid < N)
            for (int w = 0; w < OC_WPR; ++w)
                for (uint32_t m = s_bits[tid * OC_WPR + w]; m; m &= m - 1)
                    L.nl_key[(size_t)b * OC_NL + q++] = (uint32_t)(tid * Nmax + w * 32 + __ffs(m) - 1);
    }
    if (tid == 0) { totals[3 * b] = n_adj; totals[3 * b + 1] = n_nl; }
}

// ---- raw pair features from the sorted lists: entry q of image b goes to pair_ptr[b] + q, adjacent pairs first
__global__ void __launch_bounds__(256) k_emit(GDims d, const RegionStats* __restrict__ st, OnchipLists L,
                                              const int64_t* __restrict__ pair_ptr, const int32_t* __restrict__ totals,
                                              PairOut out, uint32_t* __restrict__ maxima) {
    const int b = blockIdx.y;
    const int n_adj = totals[3 * b], n_all = n_adj + totals[3 * b + 1];
    if ((int)(blockIdx.x * 256) >= n_all) return;
    const int e = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool isa = e < n_adj, isn = !isa && e < n_all;
    float mde_a = 0.f, mdx_a = 0.f, mde_n = 0.f, mdx_n = 0.f;
    int msh = 0;
    if (isa || isn) {
        const uint32_t key = isa ? L.adj_key[(size_t)b * OC_PAIRS + e] : L.nl_key[(size_t)b * OC_NL + (e - n_adj)];
        const int i = key / d.Nmax, j = key % d.Nmax;
        const RegionStats* s = st + (size_t)b * d.Nmax;
        const float dx = s[i].mlab[0] - s[j].mlab[0], dy = s[i].mlab[1] - s[j].mlab[1], dz = s[i].mlab[2] - s[j].mlab[2];
        const float de = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float cy = s[i].cy - s[j].cy, cx = s[i].cx - s[j].cx;
        const float dxy = sqrtf(cy * cy + cx * cx);
        const float gc = fabsf(s[i].mgn - s[j].mgn);
        const int64_t q = pair_ptr[b] + e;
        out.lo[q] = i; out.hi[q] = j; out.de[q] = de; out.dxy[q] = dxy; out.gc[q] = gc;
        if (isa) {
            const int v = (int)L.adj_cnt[(size_t)b * OC_PAIRS + e];
            out.shared[q] = (float)v;
            mde_a = fmaxf(mde_a, de); mdx_a = fmaxf(mdx_a, dxy); msh = v;
        } else {
            out.shared[q] = 0.0f;
            mde_n = fmaxf(mde_n, de); mdx_n = fmaxf(mdx_n, dxy);
        }
    }
    const bool any_a = __ballot(isa) != 0, any_n = __ballot(isn) != 0;
    for (int o = 32; o > 0; o >>= 1) {
        mde_a = fmaxf(mde_a, __shfl_xor(mde_a, o, 64)); mdx_a = fmaxf(mdx_a, __shfl_xor(mdx_a, o, 64));
        mde_n = fmaxf(mde_n, __shfl_xor(mde_n, o, 64)); mdx_n = fmaxf(mdx_n, __shfl_xor(mdx_n, o, 64));
        msh = max(msh, __shfl_xor(msh, o, 64));
    }
    if (lane == 0) {
        uint32_t* mx = maxima + (size_t)b * 5;
        if (any_a) { atomicMax(&mx[0], f2ord(mde_a)); atomicMax(&mx[1], f2ord(mdx_a)); atomicMax(&mx[4], (uint32_t)msh); }
        if (any_n) { atomicMax(&mx[2], f2ord(mde_n)); atomicMax(&mx[3], f2ord(mdx_n)); }
    }
}

// ---- K9: final edge attributes in place (de, dxy, shared normalised per image and per pair kind)
__global__ void __launch_bounds__(256) k_pair_final(int B, const int64_t* __restrict__ pair_ptr,
                                                    const int32_t* __restrict__ totals,
                                                    const uint32_t* __restrict__ maxima, PairOut io,
                                                    float* __restrict__ flag) {
    const int b = blockIdx.y;
    const int64_t beg = pair_ptr[b], end = pair_ptr[b + 1];
    const int64_t q = beg + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= end) return;
    const bool nl = (q - beg) >= totals[3 * b];
    const uint32_t* mx = maxima + (size_t)b * 5;
    const float de_den = (float)((double)ord2f(mx[nl ? 2 : 0]) + 1e-6);
    const float dx_den = (float)((double)ord2f(mx[nl ? 3 : 1]) + 1e-6);
    io.de[q] = io.de[q] / de_den;
    io.dxy[q] = io.dxy[q] / dx_den;
    if (!nl) io.shared[q] = io.shared[q] / (float)((double)mx[4] + 1e-6);
    flag[q] = nl ? 1.0f : 0.0f;
}

// ---- K10: node features incl. per-image min-max of the colour columns (block per image)
__device__ __forceinline__ float fix_nan(float v) {
    if (v != v) return 0.0f;
    if (isinf(v)) return v > 0 ? 1.0f : 0.0f;
    return v;
}

__global__ void __launch_bounds__(256) k_node_feats(GDims d, const int32_t* __restrict__ n_nodes,
                                                    const RegionStats* __restrict__ st,
                                                    float* __restrict__ feat /*[B,Nmax,16]*/) {
    __shared__ float rmin[6][256], rmax[6][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = n_nodes[b];
    const RegionStats* s = st + (size_t)b * d.Nmax;
    float* f = feat + (size_t)b * d.Nmax * 16;
    float lo[6], hi[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    for (int i = tid; i < N; i += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], s[i].mlab[c]); hi[c] = fmaxf(hi[c], s[i].mlab[c]);
            lo[3 + c] = fminf(lo[3 + c], s[i].slab[c]); hi[3 + c] = fmaxf(hi[3 + c], s[i].slab[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) { rmin[c][tid] = lo[c]; rmax[c][tid] = hi[c]; }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                rmin[c][tid] = fminf(rmin[c][tid], rmin[c][tid + o]);
                rmax[c][tid] = fmaxf(rmax[c][tid], rmax[c][tid + o]);
            }
        __syncthreads();
    }
    const float four_pi = (float)(4 * 3.141592653589793);
    for (int i = tid; i < N; i += 256) {
        const RegionStats r = s[i];
        float* o = f + (size_t)i * 16;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = fix_nan((r.mlab[c] - rmin[c][0]) / ((rmax[c][0] - rmin[c][0]) + (float)1e-6));
            o[3 + c] = fix_nan((r.slab[c] - rmin[3 + c][0]) / ((rmax[3 + c][0] - rmin[3 + c][0]) + (float)1e-6));
            o[6 + c] = fix_nan(r.mhsv[c]);
        }
        o[9] = fix_nan(r.cy); o[10] = fix_nan(r.cx); o[11] = fix_nan(r.area);
        const float per = r.bpx > 1.0f ? r.bpx : 1.0f;
        float comp = (four_pi * r.cnt) / (per * per);
        comp = comp < 0.0f ? 0.0f : (comp > 1.0f ? 1.0f : comp);
        o[12] = fix_nan(comp);
        o[13] = fix_nan(r.mgrad / (float)255.0);
        o[14] = fix_nan(r.bpx / r.safe);
        const float a = r.cy - 0.5f, c2 = r.cx - 0.5f;
        o[15] = fix_nan(sqrtf(a * a + c2 * c2) / (float)0.707);
    }
}

// ---- K11: prior cue 1, raw contrast (wave per node)
__global__ void __launch_bounds__(256) k_contrast(GDims d, const int32_t* __restrict__ n_nodes,
                                                  const RegionStats* __restrict__ st, float two_cs2, float* __restrict__ contrast) {
    const int b = blockIdx.y;
    const int N = n_nodes[b];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const RegionStats* s = st + (size_t)b * d.Nmax;
    const float csum = fmaxf((float)(d.H * d.W), 1.0f);   // counts.sum() == H*W exactly in float32 (< 2^24)
    const RegionStats si = s[i];
    float acc = 0.0f;
    for (int j = lane; j < N; j += 64) {
        const float dx = si.mlab[0] - s[j].mlab[0], dy = si.mlab[1] - s[j].mlab[1], dz = si.mlab[2] - s[j].mlab[2];
        const float cd = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float a = si.pcy - s[j].pcy, c = si.pcx - s[j].pcx;
        const float sd = sqrtf(a * a + c * c);
        acc += (cd * ggc_expf(-(sd * sd) / two_cs2)) * (s[j].cnt / csum);
    }
    acc = wave_sum(acc);
    if (lane == 0) contrast[(size_t)b * d.Nmax + i] = acc;
}

// block-wide min/max helper over values v(i), i < N
template <typename F>
__device__ void block_minmax(int N, F v, float& mn, float& mx, float* sa, float* sb) {
    const int tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < N; i += 256) { const float x = v(i); lo = fminf(lo, x); hi = fmaxf(hi, x); }
    sa[tid] = lo; sb[tid] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { sa[tid] = fminf(sa[tid], sa[tid + o]); sb[tid] = fmaxf(sb[tid], sb[tid + o]); }
        __syncthreads();
    }
    mn = sa[0]; mx = sb[0];
    __syncthreads();
}

__device__ __forceinline__ float unit_apply(float v, float mn, float mx) {  // _unit_norm (:447-454)
    if ((double)mx - (double)mn < 1e-8) return 0.0f;
    return (v - mn) / (float)((double)mx - (double)mn);
}

// ---- K12: the rest of compute_auto_prior (block per image)
__global__ void __launch_bounds__(256) k_prior(GDims d, const int32_t* __restrict__ n_nodes,
                                               const RegionStats* __restrict__ st, float* __restrict__ work /*[B,Nmax,2]*/,
                                               const float* __restrict__ contrast, float two_ce2, float* __restrict__ prior) {
    __shared__ float sa[256], sb[256];
    __shared__ double dsum[4][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = n_nodes[b];
    const RegionStats* s = st + (size_t)b * d.Nmax;
    const float* ct = contrast + (size_t)b * d.Nmax;
    float* fg = work + (size_t)b * d.Nmax * 2;
    float* bg = fg + d.Nmax;
    float* pr = prior + (size_t)b * d.Nmax * 3;
    float mn, mx;
    block_minmax(N, [&](int i) { return ct[i]; }, mn, mx, sa, sb);
    for (int i = tid; i < N; i += 256) {
        const float a = s[i].pcy - 0.5f, c = s[i].pcx - 0.5f;
        const float dd = sqrtf(a * a + c * c);
        fg[i] = unit_apply(ct[i], mn, mx) * ggc_expf(-(dd * dd) / two_ce2);
    }
    __syncthreads();
    block_minmax(N, [&](int i) { return fg[i]; }, mn, mx, sa, sb);
    for (int i = tid; i < N; i += 256) fg[i] = unit_apply(fg[i], mn, mx);
    // background colour model from the frame pixels; sums over N in double (order independent to ~1e-16)
    double bs = 0, m0 = 0, m1 = 0, m2 = 0;
    for (int i = tid; i < N; i += 256) {
        const double w = (double)s[i].border;
        bs += w; m0 += w * (double)s[i].mlab[0]; m1 += w * (double)s[i].mlab[1]; m2 += w * (double)s[i].mlab[2];
    }
    dsum[0][tid] = bs; dsum[1][tid] = m0; dsum[2][tid] = m1; dsum[3][tid] = m2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) for (int c = 0; c < 4; ++c) dsum[c][tid] += dsum[c][tid + o];
        __syncthreads();
    }
    const float bsum = (float)dsum[0][0];
    const float mu0 = (float)(dsum[1][0] / dsum[0][0]), mu1 = (float)(dsum[2][0] / dsum[0][0]),
                mu2 = (float)(dsum[3][0] / dsum[0][0]);
    __syncthreads();
    double var = 0;
    for (int i = tid; i < N; i += 256) {
        const float w = s[i].border / bsum;
        const float d0 = s[i].mlab[0] - mu0, d1 = s[i].mlab[1] - mu1, d2 = s[i].mlab[2] - mu2;
        var += (double)((d0 * d0) * w) + (double)((d1 * d1) * w) + (double)((d2 * d2) * w);
    }
    dsum[0][tid] = var;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) dsum[0][tid] += dsum[0][tid + o]; __syncthreads(); }
    const float var_bg = (float)dsum[0][0];
    const double sigma_bg = var_bg > 1e-6 ? (double)sqrtf(var_bg) : sqrt(1e-6);
    const float den = (float)(2.0 * (sigma_bg + 1e-6) * (sigma_bg + 1e-6));
    __syncthreads();
    for (int i = tid; i < N; i += 256) {
        float v = 0.0f;
        if (bsum > 0.0f) {
            const float d0 = s[i].mlab[0] - mu0, d1 = s[i].mlab[1] - mu1, d2 = s[i].mlab[2] - mu2;
            const float dd = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
            v = ggc_expf(-(dd * dd) / den);
        }
        float r = (s[i].border / s[i].safe) * 4.0f;
        r = r < 0.0f ? 0.0f : (r > 1.0f ? 1.0f : r);
        bg[i] = (v != v) ? v : fmaxf(v, r);
    }
    __syncthreads();
    block_minmax(N, [&](int i) { return bg[i]; }, mn, mx, sa, sb);
    for (int i = tid; i < N; i += 256) {
        const float bgv = unit_apply(bg[i], mn, mx), fgv = fg[i];
        pr[3 * i + 0] = fix_nan(fgv);
        pr[3 * i + 1] = fix_nan(bgv);
        pr[3 * i + 2] = fix_nan(1.0f - fabsf(fgv - bgv));
    }
}

// ---- fill: packed outputs
__global__ void __launch_bounds__(256) k_fill_nodes(GDims d, const int32_t* __restrict__ n_nodes,
                                                    const int64_t* __restrict__ node_ptr,
                                                    const float* __restrict__ feat, const float* __restrict__ prior,
                                                    const RegionStats* __restrict__ st, float* __restrict__ x,
                                                    float* __restrict__ cent, float* __restrict__ area) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes[b]) return;
    const int64_t o = node_ptr[b] + i;
    const size_t li = (size_t)b * d.Nmax + i;
    if (x) {
        for (int c = 0; c < 16; ++c) x[o * 19 + c] = feat[li * 16 + c];
        for (int c = 0; c < 3; ++c) x[o * 19 + 16 + c] = prior[li * 3 + c];
    }
    if (cent) { cent[o * 2] = st[li].cy; cent[o * 2 + 1] = st[li].cx; }
    if (area) area[o] = st[li].area;
}

__global__ void __launch_bounds__(256) k_fill_edges(int B, const int64_t* __restrict__ pair_ptr,
                                                    const int64_t* __restrict__ node_ptr, int global_ids, PairOut p,
                                                    const float* __restrict__ flag, int32_t* __restrict__ src,
                                                    int32_t* __restrict__ dst, float* __restrict__ attr) {
    const int b = blockIdx.y;
    const int off = global_ids ? (int)node_ptr[b] : 0;      // PyG Batch collation offsets
    const int64_t beg = pair_ptr[b], end = pair_ptr[b + 1];
    const int64_t q = beg + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= end) return;
    const int64_t np = end - beg;
    const int64_t e0 = 2 * beg + (q - beg), e1 = e0 + np;   // [lo.., hi..] then mirrored (:303-306)
    if (src) { src[e0] = p.lo[q] + off; src[e1] = p.hi[q] + off; }
    if (dst) { dst[e0] = p.hi[q] + off; dst[e1] = p.lo[q] + off; }
    if (attr) {
        const float a[5] = {p.de[q], p.dxy[q], p.shared[q], p.gc[q], flag[q]};
        for (int c = 0; c < 5; ++c) { attr[e0 * 5 + c] = a[c]; attr[e1 * 5 + c] = a[c]; }
    }
}

} // namespace ggc

using namespace ggc;

extern "C" int ggc_graph_count(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const int32_t* segments,
                               const int32_t* n_nodes, const float* lab, const float* hsv, const float* grad,
                               int connectivity, int n_nonlocal, int64_t* node_ptr, int64_t* edge_ptr) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1 && B <= 65535, GGC_E_SHAPE, "bad shape B=%d H=%d W=%d", B, H, W);
    GGC_REQUIRE(ctx, segments && n_nodes && lab && hsv && grad && node_ptr && edge_ptr, GGC_E_INVALID_ARG, "null pointer");
    GGC_REQUIRE(ctx, connectivity == 4 || connectivity == 8, GGC_E_INVALID_ARG, "connectivity must be 4 or 8");
    GGC_REQUIRE(ctx, n_nonlocal >= 0 && n_nonlocal <= 64, GGC_E_INVALID_ARG, "n_nonlocal out of range");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ctx->graph.valid = false;

    // sync 1: node counts
    std::vector<int32_t> nn;
    if (const int rc = read_i32(ctx, st, n_nodes, B, nn)) return rc;
    int Nmax = 1;
    GraphState& gs = ctx->graph;
    gs.node_ptr.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        GGC_REQUIRE(ctx, nn[b] >= 1 && (size_t)nn[b] <= (size_t)H * W, GGC_E_SHAPE, "n_nodes[%d]=%d is invalid", b, nn[b]);
        Nmax = std::max(Nmax, nn[b]);
        gs.node_ptr[b + 1] = gs.node_ptr[b] + nn[b];
    }
    GDims d{B, H, W, Nmax, connectivity, n_nonlocal};
    const size_t BN = (size_t)B * Nmax;

    int4* bbox = scratch_t<int4>(ctx, S_G_AUX, BN);
    int32_t* border = scratch_t<int32_t>(ctx, S_G_AUX2, BN);
    uint32_t* small = scratch_t<uint32_t>(ctx, S_G_AUX3, (size_t)B * 16);   // gmax[B] | maxima[B,5] | totals[B,3]
    RegionStats* stats = scratch_t<RegionStats>(ctx, S_G_STATS, BN);
    float* feat = scratch_t<float>(ctx, S_G_FEAT, BN * 16);
    float* prior = scratch_t<float>(ctx, S_G_PRIOR, BN * 3);
    float* work = scratch_t<float>(ctx, S_G_X, BN * 3);
    if (!bbox || !border || !small || !stats || !feat || !prior || !work) return GGC_E_OOM;
    uint32_t* gmax = small;
    uint32_t* maxima = small + B;
    int32_t* totals = reinterpret_cast<int32_t*>(small + (size_t)B * 6);   // {n_adj, n_nl, on-chip tables overflowed}
    float* contrast = work + BN * 2;
    const dim3 rows(cdiv(Nmax, 4), B);

    // The topology through the dense matrix: for what the on-chip tables do not hold, and with GGC_GRAPH_ONCHIP=0.
    int32_t *dense = nullptr, *cnt_adj = nullptr, *cnt_nl = nullptr;
    auto dense_topology = [&]() -> int {
        GGC_REQUIRE(ctx, (size_t)B * Nmax * Nmax * 4 < (size_t)64 << 30, GGC_E_OOM,
                    "dense adjacency of %d x %d^2 exceeds 64 GiB", B, Nmax);
        dense = scratch_t<int32_t>(ctx, S_G_PAIRCNT, BN * Nmax);
        cnt_adj = scratch_t<int32_t>(ctx, S_G_NL, BN * 2);
        if (!dense || !cnt_adj) return GGC_E_OOM;
        cnt_nl = cnt_adj + BN;
        GGC_HIP(ctx, hipMemsetAsync(dense, 0, sizeof(int32_t) * BN * Nmax, st));
        {
            ProfScope prof(ctx, st, "graph_dense");
            hipLaunchKernelGGL(k_adj, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(256), 0, st, d, segments, dense);
        }
        GGC_LAUNCH_CHECK(ctx);
        if (n_nonlocal > 0) {
            const size_t lds = (size_t)4 * Nmax * sizeof(float);
            GGC_REQUIRE(ctx, lds <= 64 * 1024, GGC_E_UNSUPPORTED, "k-NN row buffer for %d nodes exceeds LDS", Nmax);
            ProfScope prof(ctx, st, "graph_knn");
            hipLaunchKernelGGL(k_knn, rows, dim3(256), lds, st, d, n_nodes, stats, dense);
        }
        hipLaunchKernelGGL(k_rowcount, rows, dim3(256), 0, st, d, n_nodes, dense, cnt_adj, cnt_nl);
        hipLaunchKernelGGL(k_rowscan, dim3(B), dim3(256), 0, st, d, n_nodes, cnt_adj, cnt_nl, totals);
        GGC_LAUNCH_CHECK(ctx);
        return GGC_OK;
    };

    // k_topology is one workgroup per image: below OC_MIN_BATCH images the dense kernels, which spread an image's rows
    // over the chip, are the faster way (profiles/r17_graph_onchip.txt); GGC_GRAPH_ONCHIP=2 takes the tables at any size
    bool onchip = knobs().graph_onchip && (B >= OC_MIN_BATCH || knobs().graph_onchip >= 2) && Nmax <= OC_NMAX &&
                  n_nonlocal <= OC_KMAX;
    // one workgroup per image fills the chip at batch 256; a small batch splits each image's rows over several
    // (GGC_GRAPH_BANDS pins the number, for tests)
    const int bands = knobs().graph_bands ? std::min({OC_BANDS_MAX, knobs().graph_bands, H})
                                          : std::max(1, std::min({OC_BANDS_MAX, ctx->n_cu / B, H}));
    OnchipLists lists{};
    if (onchip) {
        const size_t got = carve_scratch(ctx, S_G_LISTS, [&](Carve& c) {
            lists.band_key = c.take<uint32_t>((size_t)B * bands * OC_PAIRS);
            lists.band_cnt = c.take<uint32_t>((size_t)B * bands * OC_PAIRS);
            lists.band_n = c.take<int32_t>((size_t)B * bands);
            lists.adj_key = c.take<uint32_t>((size_t)B * OC_PAIRS);
            lists.adj_cnt = c.take<uint32_t>((size_t)B * OC_PAIRS);
            lists.nl_key = c.take<uint32_t>((size_t)B * OC_NL);
        });
        if (!got) return GGC_E_OOM;
    }
    if (!onchip || bands > 1) {
        hipLaunchKernelGGL(k_bbox_init, dim3(cdiv(BN, 256)), dim3(256), 0, st, BN, bbox);
        GGC_HIP(ctx, hipMemsetAsync(border, 0, sizeof(int32_t) * BN, st));
        GGC_HIP(ctx, hipMemsetAsync(small, 0, sizeof(uint32_t) * (size_t)B * 16, st));
    }
    if (onchip) {
        ProfScope prof(ctx, st, "graph_scan");
        hipLaunchKernelGGL(k_region_scan, dim3(bands, B), dim3(OC_THREADS), 0, st, d, bands, segments, grad, bbox, border,
                           gmax, maxima, totals, lists);
    } else
        hipLaunchKernelGGL(k_bbox, dim3(cdiv(W, 64), cdiv(H, BBOX_ROWS), B), dim3(256), 0, st, d, segments, grad, bbox,
                           border, gmax);
    {
        ProfScope prof(ctx, st, "graph_stats");
        hipLaunchKernelGGL(k_stats, dim3(cdiv(Nmax, SG_REGIONS), B), dim3(64), 0, st, d, segments, n_nodes, lab, hsv, grad,
                           bbox, border, gmax, stats);
    }
    GGC_LAUNCH_CHECK(ctx);
    if (onchip) {
        ProfScope prof(ctx, st, "graph_knn");
        hipLaunchKernelGGL(k_topology, dim3(B), dim3(OC_THREADS), 0, st, d, bands, n_nodes, stats, lists, totals);
        GGC_LAUNCH_CHECK(ctx);
    } else if (const int rc = dense_topology()) {
        return rc;
    }

    // sync 2: pair counts, and whether any image overflowed the on-chip tables (then the batch goes the dense way)
    std::vector<int32_t> tot;
    if (const int rc = read_i32(ctx, st, totals, B * 3, tot)) return rc;
    if (onchip) {
        for (int b = 0; b < B && onchip; ++b) onchip = tot[3 * b + 2] == 0;
        if (!onchip) {
            if (const int rc = dense_topology()) return rc;
            if (const int rc = read_i32(ctx, st, totals, B * 3, tot)) return rc;
        }
    }
    std::vector<int64_t>& pair_ptr = gs.pair_ptr;
    pair_ptr.assign(B + 1, 0);
    gs.edge_ptr.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        pair_ptr[b + 1] = pair_ptr[b] + tot[3 * b] + tot[3 * b + 1];
        gs.edge_ptr[b + 1] = 2 * pair_ptr[b + 1];
    }
    const int64_t n_pairs = pair_ptr[B];
    int64_t* ptrs = scratch_t<int64_t>(ctx, S_G_PTR, (size_t)2 * (B + 1));
    int32_t* plo = scratch_t<int32_t>(ctx, S_G_PAIRS, (size_t)std::max<int64_t>(n_pairs, 1) * 2);
    float* pattr = scratch_t<float>(ctx, S_G_EDGE_ATTR, (size_t)std::max<int64_t>(n_pairs, 1) * 5);
    if (!ptrs || !plo || !pattr) return GGC_E_OOM;
    // both sources live in the context until the next count, which first waits for this stream
    GGC_HIP(ctx, hipMemcpyAsync(ptrs, gs.node_ptr.data(), sizeof(int64_t) * (B + 1), hipMemcpyHostToDevice, st));
    GGC_HIP(ctx, hipMemcpyAsync(ptrs + (B + 1), pair_ptr.data(), sizeof(int64_t) * (B + 1), hipMemcpyHostToDevice, st));
    const size_t np1 = (size_t)std::max<int64_t>(n_pairs, 1);
    PairOut po{plo, plo + np1, pattr, pattr + np1, pattr + 2 * np1, pattr + 3 * np1};
    float* flag = pattr + 4 * np1;
    int64_t max_pairs = 0;
    for (int b = 0; b < B; ++b) max_pairs = std::max(max_pairs, pair_ptr[b + 1] - pair_ptr[b]);
    if (!onchip)
        hipLaunchKernelGGL(k_extract, rows, dim3(256), 0, st, d, n_nodes, dense, stats, cnt_adj, cnt_nl, ptrs + (B + 1),
                           totals, po, maxima);
    else if (max_pairs > 0)
        hipLaunchKernelGGL(k_emit, dim3(cdiv(max_pairs, 256), B), dim3(256), 0, st, d, stats, lists, ptrs + (B + 1), totals,
                           po, maxima);
    if (max_pairs > 0)
        hipLaunchKernelGGL(k_pair_final, dim3(cdiv(max_pairs, 256), B), dim3(256), 0, st, B, ptrs + (B + 1), totals,
                           maxima, po, flag);
    hipLaunchKernelGGL(k_node_feats, dim3(B), dim3(256), 0, st, d, n_nodes, stats, feat);
    {
        ProfScope prof(ctx, st, "graph_prior");
        hipLaunchKernelGGL(k_contrast, rows, dim3(256), 0, st, d, n_nodes, stats, ctx->prior_two_cs2, contrast);
        hipLaunchKernelGGL(k_prior, dim3(B), dim3(256), 0, st, d, n_nodes, stats, work, contrast, ctx->prior_two_ce2, prior);
    }
    GGC_LAUNCH_CHECK(ctx);

    gs.B = B; gs.H = H; gs.W = W;
    gs.n_total = gs.node_ptr[B]; gs.e_total = gs.edge_ptr[B];
    gs.valid = true;
    gs.max_pairs = max_pairs; gs.n_max = Nmax; gs.n_nodes_dev = n_nodes;
    for (int b = 0; b <= B; ++b) { node_ptr[b] = gs.node_ptr[b]; edge_ptr[b] = gs.edge_ptr[b]; }
    return GGC_OK;
}

extern "C" int ggc_graph_fill(ggc_ctx* ctx, ggc_stream stream, float* x, float* centroids, float* area_ratio,
                              int32_t* edge_src, int32_t* edge_dst, float* edge_attr, int global_ids) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GraphState& gs = ctx->graph;
    GGC_REQUIRE(ctx, gs.valid, GGC_E_STATE, "ggc_graph_fill without a preceding successful ggc_graph_count");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int B = gs.B;
    const int64_t max_pairs = gs.max_pairs;
    const int Nmax = gs.n_max;
    const int32_t* n_nodes = gs.n_nodes_dev;
    GDims d{B, gs.H, gs.W, Nmax, 4, 0};
    const int64_t n_pairs = gs.e_total / 2;
    const size_t np1 = (size_t)std::max<int64_t>(n_pairs, 1);
    const int64_t* ptrs = reinterpret_cast<const int64_t*>(ctx->slots[S_G_PTR].p);
    int32_t* plo = reinterpret_cast<int32_t*>(ctx->slots[S_G_PAIRS].p);
    float* pattr = reinterpret_cast<float*>(ctx->slots[S_G_EDGE_ATTR].p);
    PairOut po{plo, plo + np1, pattr, pattr + np1, pattr + 2 * np1, pattr + 3 * np1};
    const float* flag = pattr + 4 * np1;
    hipLaunchKernelGGL(k_fill_nodes, dim3(cdiv(Nmax, 256), B), dim3(256), 0, st, d, n_nodes, ptrs,
                       reinterpret_cast<const float*>(ctx->slots[S_G_FEAT].p),
                       reinterpret_cast<const float*>(ctx->slots[S_G_PRIOR].p),
                       reinterpret_cast<const RegionStats*>(ctx->slots[S_G_STATS].p), x, centroids, area_ratio);
    if (max_pairs > 0 && (edge_src || edge_dst || edge_attr))
        hipLaunchKernelGGL(k_fill_edges, dim3(cdiv(max_pairs, 256), B), dim3(256), 0, st, B, ptrs + (B + 1), ptrs,
                           global_ids, po, flag, edge_src, edge_dst, edge_attr);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

extern "C" int ggc_graph_prior_sigmas(ggc_ctx* ctx, double centre_sigma, double contrast_sigma) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, centre_sigma > 0.0 && contrast_sigma > 0.0, GGC_E_INVALID_ARG, "prior sigmas must be positive");
    ctx->prior_two_ce2 = (float)(2 * centre_sigma * centre_sigma);     // python floats, then float32 operands (graph_builder.py:408,415)
    ctx->prior_two_cs2 = (float)(2 * contrast_sigma * contrast_sigma);
    return GGC_OK;
}
