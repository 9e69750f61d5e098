// ggc_cg.h — the tile-list conjugate-gradient core shared by ggc_cfmatte.hip, ggc_foreground.hip and ggc_clone.hip
// (DESIGN.md §5.26).
//
// All three solve a sparse symmetric positive definite system on the unknown pixels U of every image of a batch by
// preconditioned conjugate gradients.  A tile is CG_T x CG_T pixels of one image and a block of CG_THREADS threads, one per
// pixel.  The solver's front end counts U per tile over the whole frame (count_tile); the host reads the counts and lists
// the tiles to work on, image by image (cg_list_tiles), so that an image owns the run [tile_lo, tile_hi) of the list.
// Every later kernel runs over the list only, one block per entry (tile_of).  What a solver adds is its operator, its
// preconditioner, its vector layout, the set-up of the first residual and its stop rule.  The closed form keeps full-frame
// vectors and its own kernels; the foreground and the clone share a compact vector store, its kernels, its stop rule and
// its host driver (ggc_cg_compact.h) and add a policy each.
//
// Sums.  A per-tile sum is a fixed LDS tree over the tile's 256 values (block_sum), written to the tile's place in the
// list (tile_partial, tile_partials); a per-image sum is one wave over the image's run of those, each lane a fixed stride
// and the lanes folded in a fixed order (image_sum).  Neither depends on what else is listed, so an image's iterates do not
// depend on the batch: a batch equals its single-image calls bit for bit.  No float atomics.
//
// Scalars.  CgImage holds an image's rz, alpha, beta, the stop reference, the iteration count and `done`; k_cg_scalar, one
// wave per image, steps it twice per iteration: CG_ALPHA after the operator (alpha = rz / p.q, or the end of the image on
// a breakdown), CG_BETA after the update (beta, the count, and the solver's stop rule Solver::converged).  Every other
// MODE is a set-up step of the solver's own (Solver::setup<MODE>).  Blocks of a finished image return at once.  The only
// atomic is the integer count of finished images (cg_finish), which the host reads every CG_POLL iterations to stop early
// (cg_iterate).
#pragma once
#include "ggc_internal.h"
#include <algorithm>
#include <cmath>

namespace ggc {

constexpr int CG_T = 16;                          // tile side
constexpr int CG_THREADS = CG_T * CG_T;
constexpr int CG_POLL = 8;                        // iterations between polls of the finished count
constexpr int CG_ALPHA = 1, CG_BETA = 2;          // the shared MODEs of k_cg_scalar

struct TileRef { int b, ty, tx; };

__device__ __forceinline__ TileRef tile_of(const int2* __restrict__ tiles, int ntx) {
    const int2 t = tiles[blockIdx.x];
    return TileRef{t.x, t.y / ntx, t.y % ntx};
}

struct CgImage {                                  // per-image solver state
    double rz, rr0, alpha, beta, rel, stop;       // stop: the solver's own (CgResidualStop's threshold on ||r||)
    int iters, done, tile_lo, tile_hi;
};

// the fixed-order sum of the block's 256 values, an LDS tree
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s, int tid) {
    s[tid] = v;
    __syncthreads();
    for (int k = CG_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) s[tid] += s[tid + k];
        __syncthreads();
    }
    return s[0];
}

// the block's sum of va to its tile's place in part_a; tile_partials: and that of vb to part_b
__device__ __forceinline__ void tile_partial(double va, double* s_red, int tid, double* __restrict__ part_a) {
    const double sa = block_sum(va, s_red, tid);
    if (tid == 0) part_a[blockIdx.x] = sa;
}
__device__ __forceinline__ void tile_partials(double va, double vb, double* s_red, int tid, double* __restrict__ part_a,
                                              double* __restrict__ part_b) {
    tile_partial(va, s_red, tid, part_a);
    __syncthreads();
    tile_partial(vb, s_red, tid, part_b);
}

// over the whole frame, grid (ntx, nty, B), a block is a tile: tile_u [B, tiles] of the block's tile = the sum of its u
__device__ __forceinline__ void count_tile(int u, int* s_cnt, int tid, int32_t* __restrict__ tile_u) {
    const int n = block_sum(u, s_cnt, tid);
    if (tid == 0) tile_u[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = n;
}

// one wave per image: the sum of part over the image's run of the tile list, lane 0's fixed order
__device__ __forceinline__ double image_sum(const double* __restrict__ part, int lo, int hi) {
    const int lane = threadIdx.x;
    double v = 0.0;
    for (int k = lo + lane; k < hi; k += WAVE) v += part[k];
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_down(v, o, WAVE);
    return __shfl(v, 0, WAVE);
}

// the image is finished: its blocks return from now on, and the host's poll counts it
__device__ __forceinline__ void cg_finish(CgImage& s, int* __restrict__ n_done) {
    s.done = 1;
    atomicAdd(n_done, 1);
}

// grid B, one wave.  a, b = the image's sums of part_a, part_b (CG_ALPHA: p . q, b unread; CG_BETA: r . z, r . r).
// Solver::converged(s, rr, tol) sets s.rel and says whether the residual is small enough; Solver::setup<MODE>(s, a, b,
// tol, n_done) is every other MODE.
template <class Solver, int MODE>
__global__ void __launch_bounds__(WAVE) k_cg_scalar(int max_iter, double tol, CgImage* __restrict__ img,
                                                    const double* __restrict__ part_a, const double* __restrict__ part_b,
                                                    int* __restrict__ n_done) {
    CgImage& s = img[blockIdx.x];
    if (s.done) return;
    const double a = image_sum(part_a, s.tile_lo, s.tile_hi);
    const double b = MODE == CG_ALPHA ? 0.0 : image_sum(part_b, s.tile_lo, s.tile_hi);
    if (threadIdx.x != 0) return;
    if constexpr (MODE == CG_ALPHA) {
        if (a > 0.0 && std::isfinite(a)) {
            s.alpha = s.rz / a;
        } else {                                                 // p = 0 or a breakdown: nothing left to do
            s.alpha = 0.0;
            cg_finish(s, n_done);
        }
    } else if constexpr (MODE == CG_BETA) {
        s.iters += 1;
        const bool small = Solver::converged(s, b, tol);
        s.beta = a / s.rz;
        s.rz = a;
        if (small || s.iters >= max_iter) cg_finish(s, n_done);
    } else {
        Solver::template setup<MODE>(s, a, b, tol, n_done);
    }
}

// what every launch of k_cg_scalar in a call shares
struct CgScalars {
    hipStream_t st; int B, max_iter; double tol; CgImage* img; const double *part_a, *part_b; int* n_done;
    template <class Solver, int MODE> void step() const {
        hipLaunchKernelGGL((k_cg_scalar<Solver, MODE>), dim3(B), dim3(WAVE), 0, st, max_iter, tol, img, part_a, part_b, n_done);
    }
};

// The tile list from the counts read back, cnt [B, nty * ntx].  An image with no U, or with U = skip_u pixels (the
// closed form passes H * W: nothing anchors such an image; 0 skips nothing more), is not solved: done = 1 and an empty
// run.  Every other image lists, in raster order, the tiles within `ring` tiles (0 or 1, Chebyshev) of a tile that holds
// U.  img [B] gets the runs and `done` (everything else 0), u [B] the U counts, slot [B, nty * ntx] (if asked for) each
// tile's place in the list or -1.  Returns the number of images to solve.
inline int cg_list_tiles(int B, int ntx, int nty, const int32_t* cnt, int ring, int64_t skip_u, std::vector<int2>& list,
                         std::vector<CgImage>& img, std::vector<int64_t>& u, std::vector<int32_t>* slot) {
    const int nt = ntx * nty;
    list.clear();
    img.assign(B, CgImage{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1, 0, 0});
    u.assign(B, 0);
    if (slot) slot->assign((size_t)B * nt, -1);
    std::vector<uint8_t> near(ring > 0 ? nt : 0), row(near.size());
    int n_solve = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* c = cnt + (size_t)b * nt;
        int32_t* sl = slot ? slot->data() + (size_t)b * nt : nullptr;
        CgImage& s = img[b];
        s.tile_lo = s.tile_hi = (int)list.size();
        if (ring > 0) {                               // near: the tile is within the ring of a tile with U
            for (int k = 0; k < nt; ++k) near[k] = c[k] > 0;
            for (int d = 0; d < ring; ++d) {          // one more ring: the OR over 3 tiles of a row, then over 3 rows
                for (int k = 0; k < nt; ++k)
                    row[k] = near[k] | (k % ntx > 0 ? near[k - 1] : 0) | (k % ntx < ntx - 1 ? near[k + 1] : 0);
                for (int k = 0; k < nt; ++k)
                    near[k] = row[k] | (k >= ntx ? row[k - ntx] : 0) | (k < nt - ntx ? row[k + ntx] : 0);
            }
        }
        int64_t total = 0;
        for (int k = 0; k < nt; ++k) {                // one pass over the counts: an image without U lists nothing
            total += c[k];
            if (!(ring > 0 ? near[k] : c[k] > 0)) continue;
            if (sl) sl[k] = (int32_t)list.size();
            list.push_back(make_int2(b, k));
        }
        u[b] = total;
        if (total != 0 && total == skip_u) {          // not solved after all: its tiles are taken back
            list.resize(s.tile_lo);
            if (sl) std::fill(sl, sl + nt, -1);
        }
        if ((int)list.size() == s.tile_lo) continue;
        s.tile_hi = (int)list.size();
        s.done = 0;
        ++n_solve;
    }
    return n_solve;
}

// the per-tile counts of the front end, read to the host
inline int cg_read_counts(ggc_ctx* ctx, hipStream_t st, const int32_t* tile_u, size_t n, std::vector<int32_t>& cnt) {
    cnt.resize(n);
    GGC_HIP(ctx, hipMemcpyAsync(cnt.data(), tile_u, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GGC_HIP(ctx, hipStreamSynchronize(st));
    return GGC_OK;
}

// the list, the images' states and a zero finished count to the device; synchronous, so the host vectors may go
inline int cg_upload(ggc_ctx* ctx, hipStream_t st, const std::vector<int2>& list, const std::vector<CgImage>& host_img,
                     int2* tiles, CgImage* img, int* n_done) {
    if (!list.empty()) GGC_HIP(ctx, hipMemcpyAsync(tiles, list.data(), list.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    GGC_HIP(ctx, hipMemcpyAsync(img, host_img.data(), host_img.size() * sizeof(CgImage), hipMemcpyHostToDevice, st));
    GGC_HIP(ctx, hipMemsetAsync(n_done, 0, sizeof(int), st));
    GGC_HIP(ctx, hipStreamSynchronize(st));
    return GGC_OK;
}

// The iteration: iteration(it) launches one iteration's kernels on st, up to max_iter times; every CG_POLL iterations,
// and not after the last, the finished count is read and the loop ends once all n_solve images are finished.
template <class Iteration>
inline int cg_iterate(ggc_ctx* ctx, hipStream_t st, int max_iter, const int* n_done, int n_solve, Iteration iteration) {
    std::vector<int32_t> h;
    for (int it = 0; it < max_iter; ++it) {
        iteration(it);
        GGC_LAUNCH_CHECK(ctx);
        if ((it + 1) % CG_POLL == 0 && it + 1 < max_iter) {
            if (int e = read_i32(ctx, st, n_done, 1, h)) return e;
            if (h[0] >= n_solve) break;
        }
    }
    return GGC_OK;
}

} // namespace ggc
