// ggc_gnn_gather.hip — the CSR scatter-gather of GCNConv and SAGEConv, launched by
// ResGCNNet, GCNTrimapNet and the ggc_gcn_aggregate entry.
//
// Kernel map:
//   k_agg_pack           packed column words of the graph-resident gather, once per forward
//   k_aggregate_graph    graph-resident gather, a graph's column slice in LDS (forward pass)   <- graded kernel
//   k_aggregate          direct gather from L2 (no batch structure, graphs too large for the tile, GGC_AGG_DIRECT=1)
//
// MODE 0 is GCNConv with the fused epilogue h + gelu((agg + b) * gate), MODE 1 the SAGE mean.  The launchers are declared
// in ggc_gnn.h and every width the library uses is instantiated at the bottom of this file.
#include "ggc_gnn.h"
#include <cmath>

namespace ggc {

// Destination-major gather: LPR lanes x float4 cover one D-wide row, a wave
// handles 64/LPR rows, a block of 4 waves handles RPB consecutive rows.  Blocks
// are remapped so each XCD walks a contiguous range of rows (= whole images):
// the ~11 re-reads of every xw row then hit that XCD's L2.  Neighbours are
// summed in CSR (= edge) order with one rounding per multiply and per add, the
// self loop last, exactly like the oracle.
//   MODE 0 (GCNConv): out = sum dis[j] dis[i] xw[j] + dis[i]^2 xw[i] + bias,
//                     fused epilogue h + gelu(out * gate) when gate != null.
//   MODE 1 (SAGE mean): out = sum xw[j] / max(cnt, 1).
// (The lane layout AggCfg<D> is in ggc_gnn.h: k_jk shares it.)
__device__ __forceinline__ void fma4(float4& acc, float w, const float4& v) {
    acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
}
__device__ __forceinline__ void add4(float4& acc, const float4& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
// the two epilogues of the float4 routes: h + gelu(acc * gate) of GCNConv, the SAGE mean over cnt neighbours
__device__ __forceinline__ void gate4(float4& acc, const float4& gt, const float4& hv) {
    acc.x = hv.x + gelu_f(acc.x * gt.x); acc.y = hv.y + gelu_f(acc.y * gt.y);
    acc.z = hv.z + gelu_f(acc.z * gt.z); acc.w = hv.w + gelu_f(acc.w * gt.w);
}
__device__ __forceinline__ void mean4(float4& acc, int cnt) {
    const float c = (float)(cnt > 0 ? cnt : 1);
    acc.x /= c; acc.y /= c; acc.z /= c; acc.w /= c;
}

template <int D, int MODE>
__global__ void __launch_bounds__(1024) k_aggregate(int N, const float* __restrict__ xw,
                                                   const int32_t* __restrict__ row_ptr,
                                                   const int32_t* __restrict__ col,
                                                   const float* __restrict__ dis,
                                                   const float* __restrict__ bias,
                                                   const float* __restrict__ gate,
                                                   const float* __restrict__ h,
                                                   float* __restrict__ out) {
    constexpr int LPR = AggCfg<D>::LPR, RPW = AggCfg<D>::RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int row = blk * (RPW * (int)(blockDim.x >> 6)) + wave * RPW + sub;
    // The sub-group of LPR lanes that owns a row first loads up to LPR column indices (and their
    // dis weights) with ONE coalesced load each, then broadcasts them by shuffle: the dependent
    // chain per row is row_ptr -> col -> dis -> rows instead of one col/dis round trip per
    // neighbour, and up to 8 neighbour rows are in flight per lane.  Summation order is unchanged
    // (CSR = edge order, self loop last).
    const bool rvalid = row < N, cvalid = sl * 4 < D;
    const int rowc = rvalid ? row : 0, slc = cvalid ? sl : 0;
    const int beg = rvalid ? row_ptr[rowc] : 0, end = rvalid ? row_ptr[rowc + 1] : 0;
    const float di = (MODE == 0) ? dis[rowc] : 1.0f;
    constexpr int D4 = D / 4;
    const float4* xw4 = reinterpret_cast<const float4*>(xw) + slc;
    const size_t o4 = (size_t)rowc * D4 + slc;
    float4 self = make_float4(0.f, 0.f, 0.f, 0.f), gt = self, hv = self;
    if (MODE == 0) {                     // epilogue operands: issue their loads before the gather
        self = xw4[(size_t)rowc * D4];
        if (gate) { gt = reinterpret_cast<const float4*>(gate)[o4]; hv = reinterpret_cast<const float4*>(h)[o4]; }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = beg; base < end; base += LPR) {
        const int n = min(LPR, end - base);
        int c = 0;
        float w = 0.0f;
        if (sl < n) { c = col[base + sl]; if (MODE == 0) w = dis[c] * di; }
        for (int k = 0; k < n; k += 8) {
            float4 v[8];
            float wk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = min(k + u, n - 1);
                const int j = __shfl(c, kk, LPR);
                wk[u] = __shfl(w, kk, LPR);
                if (k + u < n) v[u] = xw4[(size_t)j * D4];     // predicated: no duplicate row fetches in the tail
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (k + u < n) {
                    if (MODE == 0) fma4(acc, wk[u], v[u]);
                    else add4(acc, v[u]);
                }
            }
        }
    }
    if (MODE == 0) {
        fma4(acc, di * di, self);
        if (bias) add4(acc, reinterpret_cast<const float4*>(bias)[slc]);
        if (gate) gate4(acc, gt, hv);
    } else {
        mean4(acc, end - beg);
    }
    if (rvalid && cvalid) reinterpret_cast<float4*>(out)[o4] = acc;
}

// Graph-resident form of the gather (the one the forward pass uses).  PMC profiling of the kernel
// above shows ideal HBM traffic (FETCH+WRITE == algorithmic bytes) but the per-CU L1/texture path
// ~76 % busy and two thirds of the L2 requests being re-reads: every neighbour row costs a 16-cycle
// slot of the 64 B/clk vector-memory pipe.  The graphs of a batch are independent and small (about
// 600 superpixels), so a block owns ONE graph and a SW-float column slice of the feature matrix:
// it copies its [n_g, SW] slice of xw (and the graph's dis) into LDS once by LDS-DMA (128-B segments,
// every byte of xw is read from memory exactly once) and then serves every neighbour row and the
// self loop by ds_read_b128 on the 256 B/clk LDS pipe.  Two blocks share a CU (80 KiB each), so one
// block's fill overlaps the other's gather.  The D/SW slices of one graph run on the same XCD and
// share the CSR through its L2.  A graph with more than CAP nodes, or an edge that leaves its graph,
// falls back to global loads per block / per row.  Arithmetic and summation order are those of
// k_aggregate.

// Block shape of the 32-float slices (round 3, bench batch, us per launch of the gated kernel on one box): 512 threads with 8
// neighbour rows per batch of LDS reads and the epilogue operands two rows ahead (116 VGPRs, 16 waves per CU) 60.3-62.0;
// 256 threads 72-75 whatever the prefetch depth (2 / 4 / 6 rows): the kernel is short of WAVES, not of bytes in flight;
// 768 threads, 2 rows per batch (76 VGPRs, 24 waves) 59.3-59.5; 1024 threads, 2 rows per batch, one row ahead (62 VGPRs, the
// full 32 waves per CU) 57.6-58.0.  Anything that spills (768 / 1024 threads with 4 or 8 rows per batch) loses 15 us.
// (16-float slices — 64-byte fill segments, three 52-KB blocks per CU, meant for graphs of 620-782 nodes — took 143-150 us on
// the same batch against 96 us for the direct gather k_aggregate: that route is gone, such batches gather directly.)
// Every byte of the kernel is touched once: the tile fill (LDS-DMA), the gate / h stream of the epilogue and the output are
// issued NON-TEMPORAL (NT bit 4 / 2 / 1).  Measured on configs[1] at batch 256, us per launch: 0: 56.6-57.1, 1: 55.9, 2: 57.6,
// 3: 55.3, 4: 55.8, 7: 55.2 (the forward as a whole is unchanged: the next kernel finds h' in HBM either way).
template <int SW> struct AggGraph {
    static_assert(SW == 32, "one slice width is built");
    static constexpr int T = 1024, NW = T / 64;                                // threads per block
    static constexpr int PF = 1;                                               // epilogue rows in flight ahead of the gather
    static constexpr int UB = 2;                                               // neighbour rows per batch of LDS reads
    static constexpr int NT = 7;                                               // non-temporal streams: all three
    static constexpr int LPR = SW / 4, RPW = 64 / LPR, RPP = NW * RPW;         // rows per pass of the block
    static constexpr int LDS = 80 * 1024;                                      // 2 blocks per CU
    static constexpr int OCC = 2 * T / 256 < 8 ? 2 * T / 256 : 8;              // waves per SIMD the blocks of a CU need
    static constexpr int CAP_LDS = (LDS - SW * 4 - 4) / (SW * 4 + 4);          // tile row + dis entry, one zero row
    static constexpr int CAP = CAP_LDS < 1023 ? CAP_LDS : 1023;                // 10-bit row offsets in the packed columns
    static constexpr int K = (CAP + RPP - 1) / RPP;                            // passes for a full tile
    static constexpr int FILL = (CAP * LPR + T - 1) / T;                       // LDS-DMA pieces per thread
};

// broadcast lane U of every group of W lanes (W = 4 or 8): ds_swizzle, no address VGPR and no VALU
template <int W, int U> __device__ __forceinline__ int group_bcast(int v) {
    return __builtin_amdgcn_ds_swizzle(v, (0x1f & ~(W - 1)) | (U << 5));
}
template <int W, int U> __device__ __forceinline__ float group_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (0x1f & ~(W - 1)) | (U << 5)));
}
template <int W, int U0, int NU, typename F> __device__ __forceinline__ void unroll_bcast(F&& f) {
    if constexpr (NU > 0) { f(std::integral_constant<int, U0>{}); unroll_bcast<W, U0 + 1, NU - 1>(f); }
}

// Per (row, lane) column words of the graph-resident gather, built once per forward pass and shared by
// every layer (7 aggregations read the same CSR): for lane sl of the LPR lanes that own a row,
//   bits 0-9 / 10-19: tile row (offset inside the graph) of neighbours sl and LPR + sl, ZROW when there is none
//   bits 20+        : n + 1, or 0 for an irregular row (more than 2 * LPR neighbours, or an edge that leaves
//                     the graph) which the kernel handles by the generic route
// One coalesced load per row replaces the dependent row_ptr -> col hops in the gather kernel.
template <int SW>
__global__ void __launch_bounds__(256) k_agg_pack(int N, const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ batch,
                                                  const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  int32_t* __restrict__ pack) {
    constexpr int LPR = AggGraph<SW>::LPR, ZROW = AggGraph<SW>::CAP;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // N * LPR is a multiple of LPR: whole groups stay together
    const int row = min(i / LPR, N - 1), sl = i % LPR;
    const int g = batch[row];
    const int g0 = node_ptr[g], n_g = node_ptr[g + 1] - g0;
    const int beg = row_ptr[row], n = row_ptr[row + 1] - beg;
    bool regular = n <= 2 * LPR;
    int pk = 0;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const bool have = nb * LPR + sl < n;
        const int off = have ? col[beg + nb * LPR + sl] - g0 : 0;
        regular = regular && (unsigned)off < (unsigned)n_g;
        pk |= (have ? off & 1023 : ZROW) << (10 * nb);
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
        const int other = __shfl_xor((int)regular, o, LPR);     // every lane takes part: no short-circuit around the shuffle
        regular = regular && other != 0;
    }
    if (i < N * LPR) pack[i] = regular ? pk | (n + 1) << 20 : (ZROW | ZROW << 10);
}

// One row of the column slice by the generic route (columns, weights and out-of-tile rows from global memory).
template <int D, int MODE, int SW>
__device__ __forceinline__ void agg_row_generic(int row, int g0, int n_g, const float4* tile, const float4* __restrict__ xw4g,
                                                const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                const float* __restrict__ dis, const float4& bias4,
                                                const float* __restrict__ gate, const float* __restrict__ h,
                                                float* __restrict__ out, int s, int sl) {
    constexpr int LPR = SW / 4, D4 = D / 4;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    const float di = (MODE == 0) ? dis[row] : 1.0f;
    const size_t o4 = (size_t)row * D4 + s * LPR + sl;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = beg; base < end; base += LPR) {
        const int m = min(LPR, end - base);
        int c = g0;
        float w = 0.0f;
        if (sl < m) { c = col[base + sl]; if (MODE == 0) w = dis[c] * di; }
        for (int u = 0; u < m; ++u) {
            const int j = __shfl(c, u, LPR);
            const float wu = __shfl(w, u, LPR);
            const int off = j - g0;
            const float4 v = (tile && (unsigned)off < (unsigned)n_g) ? tile[off * LPR + sl] : xw4g[(size_t)j * D4 + sl];
            if (MODE == 0) fma4(acc, wu, v);
            else add4(acc, v);
        }
    }
    if (MODE == 0) {
        fma4(acc, di * di, tile ? tile[(row - g0) * LPR + sl] : xw4g[(size_t)row * D4 + sl]);
        add4(acc, bias4);
        if (gate) {
            const float4 gt = reinterpret_cast<const float4*>(gate)[o4], hv = reinterpret_cast<const float4*>(h)[o4];
            gate4(acc, gt, hv);
        }
    } else {
        mean4(acc, end - beg);
    }
    reinterpret_cast<float4*>(out)[o4] = acc;
}

template <int D, int MODE, int SW, bool GATED>
__global__ void __launch_bounds__(AggGraph<SW>::T, AggGraph<SW>::OCC) k_aggregate_graph(int G, const int32_t* __restrict__ node_ptr,
                                                            const float* __restrict__ xw,
                                                            const int32_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ pack,
                                                            const float* __restrict__ dis,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ gate,
                                                            const float* __restrict__ h,
                                                            float* __restrict__ out) {
    using C = AggGraph<SW>;
    constexpr int LPR = C::LPR, RPW = C::RPW, RPP = C::RPP, CAP = C::CAP, K = C::K, FILL = C::FILL, NS = D / SW, D4 = D / 4, T = C::T;
    constexpr int NB = 2;                                  // column batches kept in registers (NB * LPR neighbours)
    constexpr int PF = C::PF;                              // epilogue rows kept in flight ahead of the gather
    constexpr int ZROW = CAP;                              // all-zero tile row (and dis entry) the padding lanes point at
    static_assert(D % SW == 0, "slice width must divide D");
    static_assert(!GATED || MODE == 0, "the gated epilogue belongs to GCNConv");
    static_assert(C::NT == 7, "the fill, the gate / h stream and the output are written non-temporal below");
    extern __shared__ float4 tile[];                       // [CAP + 1][LPR] float4, then dis_l[CAP + 1]
    float* dis_l = reinterpret_cast<float*>(tile + (CAP + 1) * LPR);
    const v4f* tile4 = reinterpret_cast<const v4f*>(tile);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);                    // tells the compiler it is wave-uniform
    const int sub = lane / LPR, sl = lane % LPR;
    const int s = ((int)blockIdx.x >> 3) % NS;                                  // blocks b, b+8, ... share an XCD
    const int g = ((int)blockIdx.x / (8 * NS)) * 8 + ((int)blockIdx.x & 7);
    if (g >= G) return;
    const int g0 = node_ptr[g], n_g = node_ptr[g + 1] - g0;
    if (n_g <= 0) return;
    const float4* xw4g = reinterpret_cast<const float4*>(xw) + s * LPR;         // column slice
    const v4f* gate4 = reinterpret_cast<const v4f*>(gate) + s * LPR + sl;
    const v4f* h4 = reinterpret_cast<const v4f*>(h) + s * LPR + sl;
    const int r0 = wave * RPW + sub;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == 0 && bias) bias4 = reinterpret_cast<const float4*>(bias)[s * LPR + sl];
    if (n_g > CAP) {                                       // graph larger than the tile: everything from global memory
        for (int r = r0; r < n_g; r += RPP)
            agg_row_generic<D, MODE, SW>(g0 + r, g0, n_g, nullptr, xw4g, row_ptr, col, dis, bias4, gate, h, out, s, sl);
        return;
    }
    // ---- preamble: the packed column words of this block's rows (k_agg_pack) and the tile fill are independent
    // loads, so the block waits for one memory round trip; the gather then touches LDS only.
    int cp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int r = r0 + k * RPP;
        cp[k] = (r < n_g) ? pack[(size_t)(g0 + r) * LPR + sl] : (ZROW | ZROW << 10 | 1 << 20);
    }
    // tile + dis fill: LDS-DMA, no registers; a wave instruction writes 64 consecutive elements (the tile non-temporal:
    // the last operand)
#pragma unroll
    for (int f = 0; f < FILL; ++f) {
        const int i = tid + f * T;
        if (i < n_g * LPR)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xw4g + (size_t)(g0 + i / LPR) * D4 + i % LPR),
                                             (__attribute__((address_space(3))) void*)(tile + f * T + wave * 64), 16, 0, 2);
    }
    if (MODE == 0) {
#pragma unroll
        for (int f = 0; f < (CAP + T - 1) / T; ++f) {
            const int i = tid + f * T;
            if (i < n_g)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dis + g0 + i),
                                                 (__attribute__((address_space(3))) void*)(dis_l + f * T + wave * 64), 4, 0, 0);
        }
    }
    if (tid < LPR) tile[ZROW * LPR + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == LPR) dis_l[ZROW] = 0.0f;
    // The gated epilogue streams gate and h from HBM: PF rows ahead are kept in flight, unconditionally (row
    // clamped into the graph) so that the main loop is straight-line code and its waits stay counted.
    v4f gtq[K], hvq[K];
    if (GATED) {
#pragma unroll
        for (int k = 0; k < PF && k < K; ++k) {
            const size_t p4 = (size_t)(g0 + min(r0 + k * RPP, n_g - 1)) * D4;
            gtq[k] = __builtin_nontemporal_load(&gate4[p4]); hvq[k] = __builtin_nontemporal_load(&h4[p4]);
        }
    }
    __syncthreads();
    // ---- gather: LDS only, no global load besides the epilogue prefetch; no predication either, a padding
    // lane adds 0 * 0 from the zero row (acc starts at +0 and x + (+-0) == x, so the sum is unchanged)
    bool irregular = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k * RPP + wave_s * RPW >= n_g) break;          // scalar: no exec-masked region around the body, waits stay counted
        {
            const int r = r0 + k * RPP;
            const bool valid = r < n_g;
            const int rc = valid ? r : n_g - 1;
            if (GATED && k + PF < K) {
                const size_t p4 = (size_t)(g0 + min(r + PF * RPP, n_g - 1)) * D4;
                gtq[k + PF] = __builtin_nontemporal_load(&gate4[p4]); hvq[k + PF] = __builtin_nontemporal_load(&h4[p4]);
            }
            const float di = (MODE == 0) ? dis_l[rc] : 1.0f;
            const int code = cp[k] >> 20;
            const int n = code > 0 ? code - 1 : 0;
            v4f acc = 0.0f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if (nb == 0 || nb * LPR < n) {
                    const int myoff = (cp[k] >> (10 * nb)) & 1023;
                    const float myw = (MODE == 0) ? dis_l[myoff] * di : 0.0f;
                    constexpr int UB = C::UB < LPR ? C::UB : LPR;
                    unroll_bcast<1, 0, LPR / UB>([&](auto ub) {
                        v4f v[UB];
                        float wk[UB];
                        unroll_bcast<LPR, 0, UB>([&](auto u) {
                            v[u] = tile4[group_bcast<LPR, ub * UB + u>(myoff) * LPR + sl];
                            if (MODE == 0) wk[u] = group_bcast<LPR, ub * UB + u>(myw);
                        });
#pragma unroll
                        for (int u = 0; u < UB; ++u) {
                            if (MODE == 0) acc += wk[u] * v[u];
                            else acc += v[u];
                        }
                    });
                }
            }
            if (MODE == 0) {
                acc += (di * di) * tile4[rc * LPR + sl];
                acc += (v4f){bias4.x, bias4.y, bias4.z, bias4.w};
                if (GATED) acc = hvq[k] + gelu4_f(acc * gtq[k]);
            } else {
                acc /= (float)(n > 0 ? n : 1);
            }
            if (valid && code > 0)
                __builtin_nontemporal_store(acc, reinterpret_cast<v4f*>(out) + (size_t)(g0 + r) * D4 + s * LPR + sl);
            irregular = irregular || (valid && code == 0);
        }
    }
    if (__any(irregular)) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int r = r0 + k * RPP;
            if (r < n_g && (cp[k] >> 20) == 0)
                agg_row_generic<D, MODE, SW>(g0 + r, g0, n_g, tile, xw4g, row_ptr, col, dis, bias4, GATED ? gate : nullptr, h, out, s, sl);
        }
    }
}

// ------------------------------------------------------------ launch helpers

template <int D, int MODE, int SW, bool GATED>
static int launch_aggregate_graph_t(ggc_ctx* ctx, hipStream_t st, int G, const int32_t* node_ptr, const int32_t* pack,
                                    const float* xw, const int32_t* row_ptr, const int32_t* col, const float* dis,
                                    const float* bias, const float* gate, const float* h, float* out) {
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        GGC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_aggregate_graph<D, MODE, SW, GATED>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, AggGraph<SW>::LDS));
        attr_set.done(ctx->device);
    }
    hipLaunchKernelGGL((k_aggregate_graph<D, MODE, SW, GATED>), dim3(cdiv(G, 8) * 8 * (D / SW)), dim3(AggGraph<SW>::T), AggGraph<SW>::LDS, st,
                       G, node_ptr, xw, row_ptr, col, pack, dis, bias, gate, h, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

// Column-slice width of the graph-resident gather for G graphs with N nodes in total: 32 when the [nodes-per-graph, 32]
// tile fits half a CU's LDS with a little head-room over the mean graph size (a larger graph falls back per block);
// 0 = use the direct gather.
static int agg_graph_slice(int N, int G) {
    if (G <= 0 || knobs().agg_direct) return 0;
    const double want = 1.02 * (double)N / G;
    return want <= AggGraph<32>::CAP ? 32 : 0;
}

int build_agg_pack(ggc_ctx* ctx, hipStream_t st, int N, int G, const int32_t* node_ptr, const int32_t* batch,
                   const int32_t* row_ptr, const int32_t* col, AggGraphs& ag) {
    ag = AggGraphs{};
    const int sw = agg_graph_slice(N, G);
    if (!sw || N <= 0) return GGC_OK;
    const int lpr = sw / 4;
    int32_t* pack = scratch_t<int32_t>(ctx, S_AGG_PACK, (size_t)N * lpr);
    if (!pack) return GGC_E_OOM;
    hipLaunchKernelGGL(k_agg_pack<32>, dim3(cdiv(N * lpr, 256)), dim3(256), 0, st, N, node_ptr, batch, row_ptr, col, pack);
    GGC_LAUNCH_CHECK(ctx);
    ag.G = G; ag.sw = sw; ag.node_ptr = node_ptr; ag.pack = pack;
    return GGC_OK;
}

template <int D, int MODE, int SW>
static int launch_aggregate_graph(ggc_ctx* ctx, hipStream_t st, const AggGraphs& ag, const float* xw,
                                  const int32_t* row_ptr, const int32_t* col, const float* dis, const float* bias,
                                  const float* gate, const float* h, float* out) {
    if constexpr (MODE == 0) {
        if (gate)
            return launch_aggregate_graph_t<D, MODE, SW, true>(ctx, st, ag.G, ag.node_ptr, ag.pack, xw, row_ptr, col, dis, bias, gate, h, out);
    }
    return launch_aggregate_graph_t<D, MODE, SW, false>(ctx, st, ag.G, ag.node_ptr, ag.pack, xw, row_ptr, col, dis, bias, nullptr, nullptr, out);
}

template <int D, int MODE>
int launch_aggregate(ggc_ctx* ctx, hipStream_t st, int N, const float* xw, const int32_t* row_ptr, const int32_t* col,
                     const float* dis, const float* bias, const float* gate, const float* h, float* out, const AggGraphs& ag) {
    ProfScope prof(ctx, st, MODE == 0 ? "gcn_aggregate" : "sage_aggregate");
    if (ag.sw == 32) return launch_aggregate_graph<D, MODE, 32>(ctx, st, ag, xw, row_ptr, col, dis, bias, gate, h, out);
    constexpr int threads = 256;
    const int rows_per_block = AggCfg<D>::RPW * (threads / 64);
    hipLaunchKernelGGL((k_aggregate<D, MODE>), dim3(cdiv(N, rows_per_block)), dim3(threads), 0, st,
                       N, xw, row_ptr, col, dis, bias, gate, h, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

#define GGC_AGG(D, MODE) template int launch_aggregate<D, MODE>(ggc_ctx*, hipStream_t, int, const float*, const int32_t*, const int32_t*, \
                                                               const float*, const float*, const float*, const float*, float*, const AggGraphs&);
// GCNConv: ResGCNNet and ggc_gcn_aggregate at all eight widths, GCNTrimapNet at 32 ... 128
GGC_AGG(32, 0) GGC_AGG(64, 0) GGC_AGG(96, 0) GGC_AGG(128, 0) GGC_AGG(160, 0) GGC_AGG(192, 0) GGC_AGG(224, 0) GGC_AGG(256, 0)
// SAGE mean: ResGCNNet
GGC_AGG(32, 1) GGC_AGG(64, 1) GGC_AGG(96, 1) GGC_AGG(128, 1) GGC_AGG(160, 1) GGC_AGG(192, 1) GGC_AGG(224, 1) GGC_AGG(256, 1)
#undef GGC_AGG

} // namespace ggc

using namespace ggc;

extern "C" int ggc_gcn_aggregate(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* xw,
                                 const int32_t* row_ptr, const int32_t* col, const float* dis, const float* bias,
                                 const float* gate, const float* h, float* h_out) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && xw && row_ptr && col && dis && h_out, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, (gate == nullptr) == (h == nullptr), GGC_E_INVALID_ARG, "gate and h must be given together");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if (with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto w) {
            return launch_aggregate<decltype(w)::value, 0>(ctx, st, N, xw, row_ptr, col, dis, bias, gate, h, h_out); }))
        return rc;
    return set_err(ctx, GGC_E_UNSUPPORTED, "D=%d unsupported (a multiple of 32 from 32 to 256)", D);
}
