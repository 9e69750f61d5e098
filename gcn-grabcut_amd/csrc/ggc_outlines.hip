// ggc_outlines.hip — K1 mask outlines: the exact vector contours of a binary mask, traced on the device.
// Definition: include/ggc.h K1.  Design and measurements: DESIGN.md §5.28.  Integer only.
//
// A group of G images is one flat lattice of G (H+1)(W+1) corners; a crack's flat key is 4 corner + direction, so flat key
// order is image order, then the image's own key order.
//   mark    one lane per corner: the leaving cracks from the 2x2 block (ggc_outline.h); a wave of 64 corners keeps one
//           ballot per direction (a bitmap over the keys, half a byte per corner) and its crack count.
//   scan    the wave counts.  rank(corner, d) = the wave's prefix + popcounts of its four words: the compact index of a
//           crack, in key order, without a dense table of successors.
//   fill    per crack: its key, its successor's compact index (the head corner's leaving cracks are in the bitmap), and
//           whether the successor turns.
//   jump    pointer doubling on the UNCUT cycles.  A crack carries, for the window of 2^j cracks that starts at it: where
//           the window ends, the smallest index in it, how far that is, and the turning cracks before it and in all.  After
//           ceil(log2(most cracks in one image)) rounds every window covers its loop: the smallest index is the loop's start,
//           the distance to it is "cracks to the end", the turning cracks before it are "vertices to the end".  No lane
//           walks a loop; a round is one gather per crack.
//   loops   start flags scanned into loop indices, vertex counts scanned into loop_ptr.
//   label   the foreground components by ggc_ccl.h at the call's connectivity (init, merge).  A component's root is its
//           smallest pixel, whose top-left corner is the smallest corner of the component's outer loop: the E crack there is
//           that loop's start, so a hole finds its outer loop by rank(root's corner, E) and nothing is published.
//   emit    vertices by plain stores at loop_ptr[loop] + (vertices - vertices to the end); twice the area by integer
//           atomics, one per loop and wave.
#include "ggc_internal.h"
#include "ggc_ccl.h"
#include "ggc_outline.h"
#include <algorithm>
#include <climits>

namespace ggc {
namespace {

typedef unsigned long long u64;

constexpr int64_t OL_GROUP_CORNERS = int64_t(1) << 26;     // corners of one image group (a single image may have more)
constexpr int OL_SCAN_BLOCK = 1024;                        // elements per block of the scan: 256 lanes x 4

struct OlDims { int G, H, W, L, P, n; };                   // L corners and P pixels per image, n = G L corners in the group

struct OlState {                                            // the window that starts at a crack
    int4* q;                                                // x: the crack after the window   y: the smallest index in it
                                                            // z: steps to that index           w: turning cracks before it
    int32_t* tt;                                            // turning cracks in the window
};

__device__ __forceinline__ int ol_block(const uint8_t* __restrict__ m, int H, int W, int r, int c) {
    const bool up = r > 0, dn = r < H, lf = c > 0, rt = c < W;
    const uint8_t* p = m + (size_t)r * W + c;               // pixel (r, c); only read where it exists
    int b = 0;
    if (up && lf && p[-W - 1]) b |= OL_NW;
    if (up && rt && p[-W]) b |= OL_NE;
    if (dn && lf && p[-1]) b |= OL_SW;
    if (dn && rt && p[0]) b |= OL_SE;
    return b;
}

// The compact index of the crack (corner i, direction d), or of the first crack at or after corner i with d = 0.
__device__ __forceinline__ int ol_rank(const u64* __restrict__ words, const int32_t* __restrict__ pref, int i, int d) {
    const int w = i >> 6, l = i & 63;
    const u64 below = (1ull << l) - 1ull;
    int r = pref[w];
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        const u64 x = words[4 * (size_t)w + dd];
        r += __popcll(x & below);
        if (dd < d) r += (int)((x >> l) & 1ull);
    }
    return r;
}
__device__ __forceinline__ int ol_leaving_at(const u64* __restrict__ words, int i) {
    const int w = i >> 6, l = i & 63;
    int leave = 0;
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) leave |= (int)((words[4 * (size_t)w + dd] >> l) & 1ull) << dd;
    return leave;
}

__global__ void __launch_bounds__(256) k_ol_mark(OlDims d, const uint8_t* __restrict__ mask, u64* __restrict__ words,
                                                 int32_t* __restrict__ wave_cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;           // the grid covers whole waves; words and wave_cnt do too
    int leave = 0;
    if (i < d.n) {
        const int g = i / d.L, v = i - g * d.L, r = v / (d.W + 1), c = v - r * (d.W + 1);
        leave = ol_leaving(ol_block(mask + (size_t)g * d.P, d.H, d.W, r, c));
    }
    const int lane = threadIdx.x & 63, w = i >> 6;
    int cnt = 0;
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        const u64 bal = __ballot((leave >> dd) & 1);
        if (lane == 0) words[4 * (size_t)w + dd] = bal;
        cnt += __popcll(bal);
    }
    if (lane == 0) wave_cnt[w] = cnt;
}

// ---- exclusive scan of int32, in place, with the total at a[n]: local (1024 per block), tops (one block), add ----
__device__ __forceinline__ int ol_block_scan(int v, int* total) {          // 256 lanes: the exclusive prefix of v
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                                        // ws may still be read from the call before
    if (lane == 63) ws[wid] = inc;
    __syncthreads();
    int off = 0;
    for (int k = 0; k < wid; ++k) off += ws[k];
    *total = ws[0] + ws[1] + ws[2] + ws[3];
    return off + inc - v;
}
__global__ void __launch_bounds__(256) k_ol_scan_local(int n, int32_t* __restrict__ a, int32_t* __restrict__ blk_tot) {
    const int64_t base = (int64_t)blockIdx.x * OL_SCAN_BLOCK + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? a[base + k] : 0; s += v[k]; }
    int total;
    int run = ol_block_scan(s, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (base + k < n) a[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) blk_tot[blockIdx.x] = total;
}
__global__ void __launch_bounds__(256) k_ol_scan_tops(int nb, int32_t* __restrict__ blk_tot, int32_t* __restrict__ total_out) {
    int carry = 0;
    for (int s0 = 0; s0 < nb; s0 += 256) {
        const int k = s0 + threadIdx.x;
        const int v = k < nb ? blk_tot[k] : 0;
        int total;
        const int ex = ol_block_scan(v, &total);
        if (k < nb) blk_tot[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}
__global__ void __launch_bounds__(256) k_ol_scan_add(int n, int32_t* __restrict__ a, const int32_t* __restrict__ blk_tot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] += blk_tot[i / OL_SCAN_BLOCK];
}

// base[g] = the compact index of image g's first crack, base[G] = the crack total (pref[n_waves], from the scan)
__global__ void k_ol_base(OlDims d, int n_waves, const u64* __restrict__ words, const int32_t* __restrict__ pref,
                          int32_t* __restrict__ base) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > d.G) return;
    base[g] = g < d.G ? ol_rank(words, pref, g * d.L, 0) : pref[n_waves];
}

__global__ void __launch_bounds__(256) k_ol_fill(OlDims d, int connectivity, const u64* __restrict__ words,
                                                 const int32_t* __restrict__ pref, int32_t* __restrict__ ckey,
                                                 int32_t* __restrict__ succ, uint8_t* __restrict__ turn) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int leave = ol_leaving_at(words, i);
    if (!leave) return;
    const int g = i / d.L, v = i - g * d.L;
    int k = ol_rank(words, pref, i, 0);
    for (int dd = 0; dd < 4; ++dd) {
        if (!((leave >> dd) & 1)) continue;
        ckey[k] = v * 4 + dd;
        const int hi = i + ol_step_r(dd) * (d.W + 1) + ol_step_c(dd);       // the head: a corner of the same image
        const int sd = ol_successor_of(ol_leaving_at(words, hi), dd, connectivity);
        int ks = k;                                                          // sd < 0 cannot happen at the head of a crack
        if (sd >= 0) ks = ol_rank(words, pref, hi, sd);
        succ[k] = ks;
        turn[ks] = sd != dd;                                                 // every crack has one predecessor: one writer
        ++k;
    }
}

// One doubling round: the window of 2 len cracks at k from the windows of len cracks at k and at the crack after the first.
template <bool FIRST>
__global__ void __launch_bounds__(256) k_ol_jump(int N, int len, const int32_t* __restrict__ succ, const uint8_t* __restrict__ turn,
                                                 OlState in, OlState out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    int4 a; int ta;
    if (FIRST) { a = make_int4(succ[k], k, 0, 0); ta = turn[k]; } else { a = in.q[k]; ta = in.tt[k]; }
    int4 b; int tb;
    if (FIRST) { b = make_int4(succ[a.x], a.x, 0, 0); tb = turn[a.x]; } else { b = in.q[a.x]; tb = in.tt[a.x]; }
    int4 o = a;
    o.x = b.x;
    if (b.y < a.y) { o.y = b.y; o.z = len + b.z; o.w = ta + b.w; }          // strictly: a window that wraps keeps the first visit
    out.q[k] = o;
    out.tt[k] = ta + tb;
}

__global__ void __launch_bounds__(256) k_ol_start_flags(int N, const int4* __restrict__ q, int32_t* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < N) flag[k] = q[k].y == k;
}
// per loop (at its start crack): the vertex count, which the scan then turns into the group's loop_ptr in place, and the start
__global__ void __launch_bounds__(256) k_ol_loops(int N, const int4* __restrict__ q, const int32_t* __restrict__ succ,
                                                  const int32_t* __restrict__ loop_idx, int32_t* __restrict__ n_verts,
                                                  int32_t* __restrict__ loop_start) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N || q[k].y != k) return;
    const int j = loop_idx[k];
    n_verts[j] = q[succ[k]].w + 1;                                           // the turning cracks after the start, and the start
    loop_start[j] = k;
}
// image g owns loops loop_idx[base[g]] .. loop_idx[base[g+1]) of the group; N == 0: no loops at all
__global__ void k_ol_image_ptr(int G, int N, const int32_t* __restrict__ base, const int32_t* __restrict__ loop_idx,
                               const int32_t* __restrict__ lptr, int loop_off, int vert_off, int32_t* __restrict__ image_ptr,
                               int32_t* __restrict__ image_vert_ptr) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    const int li = N ? loop_idx[base[g]] : 0;
    image_ptr[g] = loop_off + li;
    image_vert_ptr[g] = vert_off + (N ? lptr[li] : 0);
}

// The foreground labelling of ggc_ccl.h; "q is set" is parent[q] >= 0 (as in ggc_post.hip).
__global__ void __launch_bounds__(256) k_ol_lab_init(size_t n, int W, int P, const uint8_t* __restrict__ mask, int32_t* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int on = 0, p = 0;
    bool same_left = false;
    if (i < n) {
        on = mask[i] != 0;
        p = (int)(i % P);
        same_left = on && (p % W) > 0 && mask[i - 1] != 0;
    }
    const int first = ccl_run_first(on, same_left, p);
    if (i < n) parent[i] = on ? first : -1;
}
template <int CONN>
__global__ void __launch_bounds__(256) k_ol_lab_merge(int H, int W, int P, int32_t* __restrict__ parent) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t base = (size_t)blockIdx.z * P;
    int32_t* par = parent + base;
    const int p = y * W + x;
    if (par[p] < 0) return;
    ccl_merge_pixel<CONN>(par, p, x, y > 0, W, base + p, [par](int q) { return par[q] >= 0; });
}

__global__ void __launch_bounds__(256) k_ol_emit(int N, int W, const int32_t* __restrict__ ckey, const uint8_t* __restrict__ turn,
                                                 const int4* __restrict__ q, const int32_t* __restrict__ loop_idx,
                                                 const int32_t* __restrict__ lptr, int vert_off, int32_t* __restrict__ verts_out,
                                                 u64* __restrict__ area2) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    int j = -1, term = 0;
    if (k < N) {
        const int key = ckey[k], dd = key & 3, v = key >> 2, r = v / (W + 1), c = v - r * (W + 1);
        const int4 s = q[k];
        j = loop_idx[s.y];
        if (turn[k]) {
            const int idx = k == s.y ? 0 : lptr[j + 1] - lptr[j] - s.w;     // the start is vertex 0
            const size_t row = (size_t)vert_off + lptr[j] + idx;
            verts_out[2 * row] = r;
            verts_out[2 * row + 1] = c;
        }
        term = ol_shoelace(r, c, dd);
    }
    // one atomic per loop and wave: the lanes of the first unserved lane's loop add up, until all are served
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(j >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int jl = __shfl(j, lead, 64);
        const bool mine = j == jl;
        int s = mine ? term : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == lead) atomicAdd(&area2[jl], (u64)(long long)s);
        todo &= ~__ballot(mine);
    }
}

// per loop: loop_ptr, area, outer, perimeter
__global__ void __launch_bounds__(256) k_ol_info(OlDims d, int NL, const u64* __restrict__ words, const int32_t* __restrict__ pref,
                                                 const int32_t* __restrict__ base, const int32_t* __restrict__ ckey,
                                                 const int32_t* __restrict__ succ, const int4* __restrict__ q,
                                                 const int32_t* __restrict__ loop_idx, const int32_t* __restrict__ loop_start,
                                                 const int32_t* __restrict__ lptr, const u64* __restrict__ area2,
                                                 const int32_t* __restrict__ parent, int loop_off, int vert_off,
                                                 int32_t* __restrict__ loop_ptr_out, int32_t* __restrict__ loop_info_out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= NL) return;
    const int k = loop_start[j], key = ckey[k], dd = key & 3, v = key >> 2;
    int lo = 0, hi = d.G;                                                    // the image: the last g with base[g] <= k
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (base[mid] <= k) lo = mid; else hi = mid; }
    const int g = lo, first = loop_idx[base[g]];
    int outer = j - first;
    if (dd != 0) {                                                           // a hole: the component of the pixel on its right
        const int r = v / (d.W + 1), c = v - r * (d.W + 1);
        const int pix = (r + ol_right_r(dd)) * d.W + c + ol_right_c(dd);
        const int root = ccl_find(parent + (size_t)g * d.P, pix);
        const int ry = root / d.W, rx = root - ry * d.W;
        outer = loop_idx[ol_rank(words, pref, g * d.L + ry * (d.W + 1) + rx, 0)] - first;
    }
    const size_t row = (size_t)loop_off + j;
    loop_ptr_out[row + 1] = vert_off + lptr[j + 1];                          // [0] = 0 is the entry's
    loop_info_out[3 * row] = (int32_t)((long long)area2[j] / 2);
    loop_info_out[3 * row + 1] = outer;
    loop_info_out[3 * row + 2] = q[succ[k]].z + 1;
}

// Exclusive scan of a[0..n) in place, the total at a[n]; blk_tot: cdiv(n, 1024) words.
void ol_scan(hipStream_t st, int32_t* a, int n, int32_t* blk_tot) {
    const int nb = cdiv(n, OL_SCAN_BLOCK);
    hipLaunchKernelGGL(k_ol_scan_local, dim3(nb), dim3(256), 0, st, n, a, blk_tot);
    hipLaunchKernelGGL(k_ol_scan_tops, dim3(1), dim3(256), 0, st, nb, blk_tot, a + n);
    hipLaunchKernelGGL(k_ol_scan_add, dim3(cdiv(n, 256)), dim3(256), 0, st, n, a, blk_tot);
}

// What one image group's counting pass leaves in scratch for its filling pass.
struct OlGroup {
    OlDims d{};
    int n_waves = 0, N = 0, NL = 0, NV = 0;
    u64* words = nullptr; int32_t *pref = nullptr, *base = nullptr, *parent = nullptr;
    int32_t *ckey = nullptr, *succ = nullptr, *loop_idx = nullptr, *n_verts = nullptr, *loop_start = nullptr;
    uint8_t* turn = nullptr;
    u64* area2 = nullptr;
    OlState fin{};
};

// The counting pass of images g0 .. g0 + G: everything up to loop_ptr, and the group's part of the two image arrays.
int ol_count_group(ggc_ctx* ctx, hipStream_t st, int g0, int G, int H, int W, const uint8_t* mask, int connectivity, int loop_off,
                   int vert_off, int32_t* image_ptr_out, int32_t* image_vert_ptr_out, OlGroup& gr) {
    OlDims& d = gr.d;
    d.G = G; d.H = H; d.W = W; d.L = (H + 1) * (W + 1); d.P = H * W; d.n = G * d.L;
    const uint8_t* m = mask + (size_t)g0 * d.P;
    const int blocks = cdiv(d.n, 256);
    gr.n_waves = blocks * 4;
    int32_t* blk_tot = nullptr;
    if (!carve_scratch(ctx, S_OUTLINE, [&](Carve& c) {
            gr.words = c.take<u64>(4 * (size_t)gr.n_waves);
            gr.pref = c.take<int32_t>((size_t)gr.n_waves + 1);
            gr.base = c.take<int32_t>((size_t)G + 1);
            blk_tot = c.take<int32_t>((size_t)cdiv(gr.n_waves, OL_SCAN_BLOCK));
            gr.parent = c.take<int32_t>((size_t)G * d.P);
        }))
        return GGC_E_OOM;
    {
        ProfScope prof(ctx, st, "outline_mark");
        hipLaunchKernelGGL(k_ol_mark, dim3(blocks), dim3(256), 0, st, d, m, gr.words, gr.pref);
    }
    {
        ProfScope prof(ctx, st, "outline_scan");
        ol_scan(st, gr.pref, gr.n_waves, blk_tot);
        hipLaunchKernelGGL(k_ol_base, dim3(cdiv(G + 1, 256)), dim3(256), 0, st, d, gr.n_waves, gr.words, gr.pref, gr.base);
    }
    GGC_LAUNCH_CHECK(ctx);
    std::vector<int32_t> host;
    int rc = read_i32(ctx, st, gr.base, G + 1, host);
    if (rc) return rc;
    gr.N = host[G]; gr.NL = gr.NV = 0;
    const int N = gr.N;
    if (N == 0) {
        hipLaunchKernelGGL(k_ol_image_ptr, dim3(cdiv(G + 1, 256)), dim3(256), 0, st, G, 0, gr.base, nullptr, nullptr, loop_off, vert_off,
                           image_ptr_out + g0, image_vert_ptr_out + g0);
        GGC_LAUNCH_CHECK(ctx);
        return GGC_OK;
    }
    int most = 0;
    for (int g = 0; g < G; ++g) most = std::max(most, host[g + 1] - host[g]);
    int rounds = 1;                                                          // 2^rounds >= the longest loop, which is >= 4
    while ((int64_t(1) << rounds) < most) ++rounds;

    const size_t max_loops = (size_t)N / 4 + 1;                              // a loop has at least 4 cracks
    OlState st2[2];
    int32_t* blk2 = nullptr;
    if (!carve_scratch(ctx, S_OUTLINE_LIST, [&](Carve& c) {
            gr.ckey = c.take<int32_t>((size_t)N);
            gr.succ = c.take<int32_t>((size_t)N);
            gr.turn = c.take<uint8_t>((size_t)N);
            for (int s = 0; s < 2; ++s) { st2[s].q = c.take<int4>((size_t)N); st2[s].tt = c.take<int32_t>((size_t)N); }
            gr.loop_idx = c.take<int32_t>((size_t)N + 1);
            gr.n_verts = c.take<int32_t>(max_loops + 1);
            gr.loop_start = c.take<int32_t>(max_loops);
            gr.area2 = c.take<u64>(max_loops);
            blk2 = c.take<int32_t>((size_t)cdiv(N, OL_SCAN_BLOCK));
        }))
        return GGC_E_OOM;
    const int nb = cdiv(N, 256);
    {
        ProfScope prof(ctx, st, "outline_fill");
        hipLaunchKernelGGL(k_ol_fill, dim3(blocks), dim3(256), 0, st, d, connectivity, gr.words, gr.pref, gr.ckey, gr.succ, gr.turn);
    }
    {
        ProfScope prof(ctx, st, "outline_jump");
        hipLaunchKernelGGL(k_ol_jump<true>, dim3(nb), dim3(256), 0, st, N, 1, gr.succ, gr.turn, st2[1], st2[0]);
        for (int r = 1; r < rounds; ++r)
            hipLaunchKernelGGL(k_ol_jump<false>, dim3(nb), dim3(256), 0, st, N, 1 << r, gr.succ, gr.turn, st2[(r - 1) & 1], st2[r & 1]);
    }
    gr.fin = st2[(rounds - 1) & 1];
    {
        ProfScope prof(ctx, st, "outline_loops");
        hipLaunchKernelGGL(k_ol_start_flags, dim3(nb), dim3(256), 0, st, N, gr.fin.q, gr.loop_idx);
        ol_scan(st, gr.loop_idx, N, blk2);
    }
    GGC_LAUNCH_CHECK(ctx);
    if ((rc = read_i32(ctx, st, gr.loop_idx + N, 1, host))) return rc;
    gr.NL = host[0];
    {
        ProfScope prof(ctx, st, "outline_loops");
        hipLaunchKernelGGL(k_ol_loops, dim3(nb), dim3(256), 0, st, N, gr.fin.q, gr.succ, gr.loop_idx, gr.n_verts, gr.loop_start);
        ol_scan(st, gr.n_verts, gr.NL, blk2);
        hipLaunchKernelGGL(k_ol_image_ptr, dim3(cdiv(G + 1, 256)), dim3(256), 0, st, G, N, gr.base, gr.loop_idx, gr.n_verts, loop_off,
                           vert_off, image_ptr_out + g0, image_vert_ptr_out + g0);
    }
    GGC_LAUNCH_CHECK(ctx);
    if ((rc = read_i32(ctx, st, gr.n_verts + gr.NL, 1, host))) return rc;
    gr.NV = host[0];
    return GGC_OK;
}

// The filling pass of the group whose counting pass is still in scratch.
int ol_fill_group(ggc_ctx* ctx, hipStream_t st, int g0, const uint8_t* mask, int connectivity, int loop_off, int vert_off,
                  int32_t* loop_ptr_out, int32_t* loop_info_out, int32_t* verts_out, const OlGroup& gr) {
    if (gr.N == 0) return GGC_OK;
    const OlDims& d = gr.d;
    const uint8_t* m = mask + (size_t)g0 * d.P;
    const size_t GP = (size_t)d.G * d.P;
    {
        ProfScope prof(ctx, st, "outline_label");
        hipLaunchKernelGGL(k_ol_lab_init, dim3(cdiv(GP, 256)), dim3(256), 0, st, GP, d.W, d.P, m, gr.parent);
        const dim3 grid(cdiv(d.W, 64), cdiv(d.H, 4), d.G);
        if (connectivity == 8) hipLaunchKernelGGL(k_ol_lab_merge<8>, grid, dim3(256), 0, st, d.H, d.W, d.P, gr.parent);
        else hipLaunchKernelGGL(k_ol_lab_merge<4>, grid, dim3(256), 0, st, d.H, d.W, d.P, gr.parent);
    }
    GGC_HIP(ctx, hipMemsetAsync(gr.area2, 0, sizeof(u64) * (size_t)gr.NL, st));
    {
        ProfScope prof(ctx, st, "outline_emit");
        hipLaunchKernelGGL(k_ol_emit, dim3(cdiv(gr.N, 256)), dim3(256), 0, st, gr.N, d.W, gr.ckey, gr.turn, gr.fin.q, gr.loop_idx,
                           gr.n_verts, vert_off, verts_out, gr.area2);
        hipLaunchKernelGGL(k_ol_info, dim3(cdiv(gr.NL, 256)), dim3(256), 0, st, d, gr.NL, gr.words, gr.pref, gr.base, gr.ckey, gr.succ,
                           gr.fin.q, gr.loop_idx, gr.loop_start, gr.n_verts, gr.area2, gr.parent, loop_off, vert_off, loop_ptr_out,
                           loop_info_out);
    }
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

} // namespace
} // namespace ggc

extern "C" int ggc_mask_outlines(ggc_ctx* ctx, ggc_stream stream, int B, int H, int W, const uint8_t* mask, int connectivity,
                                 int32_t* image_ptr_out, int32_t* image_vert_ptr_out, int32_t* loop_ptr_out, int32_t* loop_info_out,
                                 int32_t* verts_out, int64_t loop_capacity, int64_t vert_capacity) {
    using namespace ggc;
    if (!ctx) return GGC_E_INVALID_ARG;
    if (B == 0) return GGC_OK;
    GGC_REQUIRE(ctx, B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, GGC_E_SHAPE,
                "bad shape B=%d H=%d W=%d (each at most 65535)", B, H, W);
    GGC_REQUIRE(ctx, (int64_t)(H + 1) * (W + 1) <= (int64_t(1) << 28), GGC_E_INVALID_ARG,
                "%dx%d has more than 2^28 corners: crack keys and areas would not fit int32", H, W);
    GGC_REQUIRE(ctx, connectivity == 4 || connectivity == 8, GGC_E_INVALID_ARG, "connectivity %d, expected 4 or 8", connectivity);
    GGC_REQUIRE(ctx, mask && image_ptr_out && image_vert_ptr_out, GGC_E_INVALID_ARG, "null pointer");
    const bool fill = loop_ptr_out && loop_info_out && verts_out;
    GGC_REQUIRE(ctx, fill || (!loop_ptr_out && !loop_info_out && !verts_out), GGC_E_INVALID_ARG,
                "loop_ptr_out, loop_info_out and verts_out are given together or not at all");
    GGC_REQUIRE(ctx, !fill || (loop_capacity >= 0 && vert_capacity >= 0), GGC_E_INVALID_ARG, "negative capacity %lld / %lld",
                (long long)loop_capacity, (long long)vert_capacity);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int64_t L = (int64_t)(H + 1) * (W + 1);
    const int per_group = (int)std::max<int64_t>(1, std::min<int64_t>(B, OL_GROUP_CORNERS / L));
    const bool one_group = per_group >= B;
    OlGroup gr;
    int64_t loops = 0, verts = 0;
    for (int g0 = 0; g0 < B; g0 += per_group) {                              // counting: the two image arrays and the totals
        const int G = std::min(per_group, B - g0);
        const int rc = ol_count_group(ctx, st, g0, G, H, W, mask, connectivity, (int)loops, (int)verts, image_ptr_out, image_vert_ptr_out, gr);
        if (rc) return rc;
        loops += gr.NL; verts += gr.NV;
        GGC_REQUIRE(ctx, loops <= INT_MAX && verts <= INT_MAX, GGC_E_SHAPE, "the batch has more than 2^31 - 1 loops or vertices");
    }
    if (!fill) return GGC_OK;
    GGC_REQUIRE(ctx, loop_capacity >= loops && vert_capacity >= verts, GGC_E_INVALID_ARG,
                "capacities %lld loops / %lld vertices are below the %lld loops / %lld vertices traced", (long long)loop_capacity,
                (long long)vert_capacity, (long long)loops, (long long)verts);
    GGC_HIP(ctx, hipMemsetAsync(loop_ptr_out, 0, sizeof(int32_t), st));
    if (one_group) return ol_fill_group(ctx, st, 0, mask, connectivity, 0, 0, loop_ptr_out, loop_info_out, verts_out, gr);
    loops = verts = 0;
    for (int g0 = 0; g0 < B; g0 += per_group) {                              // several groups: each is counted again, then filled
        const int G = std::min(per_group, B - g0);
        int rc = ol_count_group(ctx, st, g0, G, H, W, mask, connectivity, (int)loops, (int)verts, image_ptr_out, image_vert_ptr_out, gr);
        if (rc) return rc;
        if ((rc = ol_fill_group(ctx, st, g0, mask, connectivity, (int)loops, (int)verts, loop_ptr_out, loop_info_out, verts_out, gr))) return rc;
        loops += gr.NL; verts += gr.NV;
    }
    return GGC_OK;
}
