// ggc_cg_compact.h — the compact-store layer of the tile-list CG core (ggc_cg.h), shared by ggc_foreground.hip and
// ggc_clone.hip.  The closed form keeps full-frame planes and does not need it.
//
// Both clients solve a 4-neighbour system on the unknown pixels of a field plane (alpha', the clone's byte plane) that
// their front end writes over the whole frame.  Listed are the tiles that hold an unknown pixel (ring 0: the stencil
// reaches one pixel).  The CG vectors live in a compact store of 256 entries per LISTED tile, Problem::N float64 per entry;
// tile_slot maps a tile of the frame to its place in the list (cg_vec_index).  z = M^-1 r is never stored: it is
// recomputed from r and the field wherever it is needed.  Per listed tile and iteration:
//   k_cgc_apply   p = z + beta p on the tile and a one-pixel halo, staged in LDS; q = A p on the tile; per-tile p . q.
//                 p is double-buffered: a neighbour tile reads the old p of this tile's edge while this tile writes the
//                 new one.
//   k_cg_scalar   per image: alpha = rz / (p . q)
//   k_cgc_update  x += alpha p, r -= alpha q; per-tile r . z and r . r
//   k_cg_scalar   per image: convergence (CgResidualStop), the iteration count, beta
//
// A solver keeps its front end, its set-up kernel (x_0, r_0 and their per-tile r . z, r . r), its output kernel and a
// Problem policy:
//   N                        float64 per pixel of a CG vector
//   Stored, Field, OUTSIDE   the field plane's type in memory, its type staged in LDS, the value staged beyond the frame
//   HALO, UPDATE_HALO        the halo of the field that k_cgc_apply and k_cgc_update stage.  HALO is 1 plus what
//                            precondition reads around a pixel; UPDATE_HALO 0: no staging, a thread reads its own pixel
//   FLOOR                    the absolute floor on ||r||, per sqrt of an unknown
//   Params                   what the kernels take by value
//   unknown(f)               the pixel is solved for; false for OUTSIDE
//   precondition(r, s_f, c, S, prm)    M^-1 r at the pixel staged at s_f[c], row stride S
//   apply(s_p, c, s_f, cf, S, prm)     (A p) at the pixel staged at s_p[c] (row stride CGC_S1, p = 0 off the unknown
//                                      pixels) and s_f[cf] (row stride S)
#pragma once
#include "ggc_cg.h"

namespace ggc {

constexpr int CGC_S1 = CG_T + 2;                  // tile with a one-pixel halo

template <int N> struct alignas(N % 2 ? 8 : 16) CgVec { double v[N]; };

// where the CG vectors keep pixel (y, x) of image b: its tile's slot in the list, then the pixel within the tile
__device__ __forceinline__ size_t cg_vec_index(const int32_t* __restrict__ tile_slot, int b, int nt, int ntx, int y, int x) {
    const int slot = tile_slot[(size_t)b * nt + (y / CG_T) * ntx + x / CG_T];
    return (size_t)slot * CG_THREADS + (y % CG_T) * CG_T + (x % CG_T);
}

// The compact solvers' side of k_cg_scalar (grid B, one wave): the stop rule ||r|| <= stop.  s.stop is the absolute
// floor on entry and max(tol ||r_0||, floor) after the set-up MODE CG_START (after the solver's set-up kernel): rz, rr0,
// the threshold, the images that start solved.
constexpr int CG_START = 0;
struct CgResidualStop {
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
        if (!(r0 > s.stop)) cg_finish(s, n_done);                // the start already solves the system
    }
};

// the field of the S x S pixels from (y0, x0) of the image at `base`, Problem::OUTSIDE beyond the frame
template <class Problem>
__device__ __forceinline__ void cgc_stage(typename Problem::Field* s_f, int S, int y0, int x0, int H, int W,
                                          const typename Problem::Stored* __restrict__ field, size_t base, int tid) {
    for (int e = tid; e < S * S; e += CG_THREADS) {
        const int yy = y0 + e / S, xx = x0 + e % S;
        s_f[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (typename Problem::Field)field[base + (size_t)yy * W + xx]
                                                           : Problem::OUTSIDE;
    }
}

// p = z + beta p_in (FIRST: p = z) on the tile and its halo, the tile's part written to p_out; q = A p; per-tile p . q
template <class Problem, bool FIRST>
__global__ void __launch_bounds__(CG_THREADS) k_cgc_apply(int H, int W, int ntx, int nt, typename Problem::Params prm,
                                                          const int2* __restrict__ tiles, const int32_t* __restrict__ tile_slot,
                                                          const CgImage* __restrict__ img,
                                                          const typename Problem::Stored* __restrict__ field,
                                                          const CgVec<Problem::N>* __restrict__ res,
                                                          const CgVec<Problem::N>* __restrict__ p_in,
                                                          CgVec<Problem::N>* __restrict__ p_out,
                                                          CgVec<Problem::N>* __restrict__ q, double* __restrict__ part_a) {
    using Vec = CgVec<Problem::N>;
    constexpr int N = Problem::N, HALO = Problem::HALO, SF = CG_T + 2 * HALO;
    __shared__ typename Problem::Field s_f[SF * SF];
    __shared__ Vec s_p[CGC_S1 * CGC_S1];
    __shared__ double s_red[CG_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;                                          // uniform over the block
    const int tid = threadIdx.y * CG_T + threadIdx.x;
    const int x0 = t.tx * CG_T, y0 = t.ty * CG_T;
    cgc_stage<Problem>(s_f, SF, y0 - HALO, x0 - HALO, H, W, field, (size_t)t.b * H * W, tid);
    __syncthreads();
    const double beta = FIRST ? 0.0 : s.beta;
    for (int e = tid; e < CGC_S1 * CGC_S1; e += CG_THREADS) {
        const int ey = e / CGC_S1, ex = e % CGC_S1;
        const int cf = (ey + HALO - 1) * SF + ex + HALO - 1;
        Vec p;
        for (int k = 0; k < N; ++k) p.v[k] = 0.0;
        if (Problem::unknown(s_f[cf])) {                         // in the frame and unknown: its tile is listed
            const bool own = ey >= 1 && ey <= CG_T && ex >= 1 && ex <= CG_T;
            const size_t j = own ? (size_t)blockIdx.x * CG_THREADS + (ey - 1) * CG_T + (ex - 1)
                                 : cg_vec_index(tile_slot, t.b, nt, ntx, y0 - 1 + ey, x0 - 1 + ex);
            p = Problem::precondition(res[j], s_f, cf, SF, prm);
            if constexpr (!FIRST) {
                const Vec po = p_in[j];
                for (int k = 0; k < N; ++k) p.v[k] = p.v[k] + beta * po.v[k];
            }
            if (own) p_out[j] = p;
        }
        s_p[e] = p;
    }
    __syncthreads();
    const int c = (threadIdx.y + 1) * CGC_S1 + threadIdx.x + 1, cf = (threadIdx.y + HALO) * SF + threadIdx.x + HALO;
    double va = 0.0;
    if (Problem::unknown(s_f[cf])) {
        const Vec p = s_p[c];
        const Vec qi = Problem::apply(s_p, c, s_f, cf, SF, prm);
        q[(size_t)blockIdx.x * CG_THREADS + tid] = qi;
        for (int k = 0; k < N; ++k) va += p.v[k] * qi.v[k];
    }
    tile_partial(va, s_red, tid, part_a);
}

// x += alpha p, r -= alpha q on the unknown pixels; per-tile r . z (part_a) with z = M^-1 r, and r . r (part_b)
template <class Problem>
__global__ void __launch_bounds__(CG_THREADS) k_cgc_update(int H, int W, int ntx, typename Problem::Params prm,
                                                           const int2* __restrict__ tiles, const CgImage* __restrict__ img,
                                                           const typename Problem::Stored* __restrict__ field,
                                                           const CgVec<Problem::N>* __restrict__ p,
                                                           const CgVec<Problem::N>* __restrict__ q,
                                                           CgVec<Problem::N>* __restrict__ x,
                                                           CgVec<Problem::N>* __restrict__ res, double* __restrict__ part_a,
                                                           double* __restrict__ part_b) {
    using Vec = CgVec<Problem::N>;
    using Field = typename Problem::Field;
    constexpr int N = Problem::N, HALO = Problem::UPDATE_HALO, SF = CG_T + 2 * HALO;
    __shared__ double s_red[CG_THREADS];
    const TileRef t = tile_of(tiles, ntx);
    const CgImage& s = img[t.b];
    if (s.done) return;
    const int tid = threadIdx.y * CG_T + threadIdx.x;
    const size_t base = (size_t)t.b * H * W;
    Field own = Problem::OUTSIDE;
    const Field* s_f = &own;                                     // the field around the pixel at s_f[c], row stride SF
    int c = 0;
    if constexpr (HALO > 0) {
        __shared__ Field s_halo[SF * SF];
        cgc_stage<Problem>(s_halo, SF, t.ty * CG_T - HALO, t.tx * CG_T - HALO, H, W, field, base, tid);
        __syncthreads();
        s_f = s_halo;
        c = (threadIdx.y + HALO) * SF + threadIdx.x + HALO;
    } else {                                                     // the preconditioner reads the pixel's own field only
        const int xx = t.tx * CG_T + threadIdx.x, yy = t.ty * CG_T + threadIdx.y;
        if (xx < W && yy < H) own = (Field)field[base + (size_t)yy * W + xx];
    }
    double va = 0.0, vb = 0.0;
    if (Problem::unknown(s_f[c])) {
        const size_t j = (size_t)blockIdx.x * CG_THREADS + tid;
        const double al = s.alpha;
        const Vec pj = p[j], qj = q[j];
        Vec xj = x[j], rj = res[j];
        for (int k = 0; k < N; ++k) { xj.v[k] += al * pj.v[k]; rj.v[k] -= al * qj.v[k]; }
        x[j] = xj;
        res[j] = rj;
        const Vec z = Problem::precondition(rj, s_f, c, SF, prm);
        for (int k = 0; k < N; ++k) { va += rj.v[k] * z.v[k]; vb += rj.v[k] * rj.v[k]; }
    }
    tile_partials(va, vb, s_red, tid, part_a, part_b);
}

// ---------------------------------------------------------------- host
// what a compact solve keeps over the whole frame: the field plane (one Stored per pixel), 32 bytes per tile, 64 per image
template <class Problem>
struct CgCompactFrame {
    int ntx, nty, nt;
    typename Problem::Stored* field;
    int32_t *tile_u, *tile_slot;
    int2* tiles;
    double *part_a, *part_b;
    CgImage* img;
    int* n_done;
};

// carves the frame of a B x H x W batch from `slot`; false when the allocation failed
template <class Problem>
inline bool cg_compact_frame(ggc_ctx* ctx, int slot, int B, int H, int W, CgCompactFrame<Problem>& f) {
    f.ntx = cdiv(W, CG_T); f.nty = cdiv(H, CG_T); f.nt = f.ntx * f.nty;
    const size_t n_tiles_max = (size_t)B * f.nt;
    return carve_scratch(ctx, slot, [&](Carve& c) {
        f.field = c.take<typename Problem::Stored>((size_t)B * H * W);
        f.tile_u = c.take<int32_t>(n_tiles_max); f.tile_slot = c.take<int32_t>(n_tiles_max);
        f.tiles = c.take<int2>(n_tiles_max);
        f.part_a = c.take<double>(n_tiles_max); f.part_b = c.take<double>(n_tiles_max);
        f.img = c.take<CgImage>(B); f.n_done = c.take<int>(1);
    }) != 0;
}

// Everything between a solver's front end (f.field and f.tile_u written, on st) and its output kernel: the tile list
// (an image whose unknowns number 0 or skip_u is not solved), the CG vectors carved from vec_slot (x, r, q and the two p,
// 256 entries per listed tile), the set-up and the iteration.  listed(u_count) runs on the host once the counts are
// read, before anything else is launched or allocated, and may refuse the call; setup(n_list, tblk, x, res) launches the
// solver's set-up kernel.  x = the solution's store (NULL if no tile is listed); f.img and f.tile_slot are left on the
// device for the output kernel.
template <class Problem, class Listed, class Setup>
inline int cg_compact_solve(ggc_ctx* ctx, hipStream_t st, const CgCompactFrame<Problem>& f, int vec_slot, int B, int H, int W,
                            int64_t skip_u, int max_iter, double tol, typename Problem::Params prm, Listed&& listed,
                            Setup&& setup, CgVec<Problem::N>*& x) {
    using Vec = CgVec<Problem::N>;
    const size_t n_tiles_max = (size_t)B * f.nt;
    std::vector<int32_t> cnt, slot;
    if (int e = cg_read_counts(ctx, st, f.tile_u, n_tiles_max, cnt)) return e;
    std::vector<int2> list;
    std::vector<CgImage> host_img;
    std::vector<int64_t> u_count;
    const int n_solve = cg_list_tiles(B, f.ntx, f.nty, cnt.data(), 0, skip_u, list, host_img, u_count, &slot);
    for (int b = 0; b < B; ++b) host_img[b].stop = Problem::FLOOR * std::sqrt((double)Problem::N * (double)u_count[b]);
    if (int e = listed(u_count)) return e;
    const int n_list = (int)list.size();
    Vec *res = nullptr, *q = nullptr, *p0 = nullptr, *p1 = nullptr;
    x = nullptr;
    const size_t n_vec = (size_t)n_list * CG_THREADS;
    if (n_list > 0 && !carve_scratch(ctx, vec_slot, [&](Carve& c) {
            x = c.take<Vec>(n_vec); res = c.take<Vec>(n_vec); q = c.take<Vec>(n_vec);
            p0 = c.take<Vec>(n_vec); p1 = c.take<Vec>(n_vec);
        }))
        return GGC_E_OOM;
    GGC_HIP(ctx, hipMemcpyAsync(f.tile_slot, slot.data(), n_tiles_max * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (int e = cg_upload(ctx, st, list, host_img, f.tiles, f.img, f.n_done)) return e;
    if (n_list == 0) return GGC_OK;

    const CgScalars sc{st, B, max_iter, tol, f.img, f.part_a, f.part_b, f.n_done};
    const dim3 grid(n_list), tblk(CG_T, CG_T);
    setup(n_list, tblk, x, res);
    sc.step<CgResidualStop, CG_START>();
    GGC_LAUNCH_CHECK(ctx);
    return cg_iterate(ctx, st, max_iter, f.n_done, n_solve, [&](int it) {
        Vec *p_new = (it & 1) ? p1 : p0, *p_old = (it & 1) ? p0 : p1;
        if (it == 0)
            hipLaunchKernelGGL((k_cgc_apply<Problem, true>), grid, tblk, 0, st, H, W, f.ntx, f.nt, prm, f.tiles, f.tile_slot,
                               f.img, f.field, res, p_old, p_new, q, f.part_a);
        else
            hipLaunchKernelGGL((k_cgc_apply<Problem, false>), grid, tblk, 0, st, H, W, f.ntx, f.nt, prm, f.tiles, f.tile_slot,
                               f.img, f.field, res, p_old, p_new, q, f.part_a);
        sc.step<CgResidualStop, CG_ALPHA>();
        hipLaunchKernelGGL(k_cgc_update<Problem>, grid, tblk, 0, st, H, W, f.ntx, prm, f.tiles, f.img, f.field, p_new, q, x,
                           res, f.part_a, f.part_b);
        sc.step<CgResidualStop, CG_BETA>();
    });
}

} // namespace ggc
