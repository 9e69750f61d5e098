// ggc_train.hip — the graph operators of the ResGCNNet TRAINING forward (reference model.py:508-536 in train mode) and
// their backward passes, f32, for gfx950.
//
// The dense layers of the training forward (Linear, LayerNorm, GELU, BatchNorm, softmax over jk_logits) stay in torch
// and autograd; the operators below are the ones that move data along edges or across the nodes of a graph:
//   k_inv_cnt             graph preparation: inv_cnt = 1 / max(indeg, 1) (CSRs and dis come from build_csr)
//   k_gather<D, SYM>      GCNConv aggregation out = A_hat xw + b with the residual epilogue h + gelu(out * gate);
//                         its backward runs the same gather over the SOURCE CSR (A_hat is symmetric in its weights)
//   k_gcn_epi_bwd<D>      backward of the epilogue: g_out = g gelu'(out gate) gate, g_gate = g gelu'(out gate) out
//   k_gather<D, MEAN_*>   SAGEConv mean over incoming edges, and its transpose over the source CSR
//   k_edge_mean           EdgeContext scatter-mean of the encoded edge rows (through the CSR's edge ids)
//   k_edge_mean_bwd       its backward, a gather: g_enc_e = inv_cnt[dst e] g_ctx[dst e]
//   k_pool / k_pool_bwd   GlobalContextModule readout: per-graph softmax of the scores, sum a h, broadcast; one
//                         workgroup per graph
//
// No kernel here uses a float atomic.  Every sum has one fixed order (CSR order, or a fixed partition of a workgroup
// followed by a fixed-order combine), so two runs give identical bits; a scatter in a backward pass is a gather over
// the transposed CSR, which build_csr produces stable in edge order like the forward one.
#include "ggc_internal.h"
#include <cmath>

namespace ggc {

constexpr int TB = 256;

__global__ void __launch_bounds__(TB) k_inv_cnt(int N, const int32_t* __restrict__ row_ptr, float* __restrict__ inv_cnt) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < N) inv_cnt[i] = 1.0f / (float)max(row_ptr[i + 1] - row_ptr[i], 1);
}

// d/dx [x Phi(x)] = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

enum { G_SYM = 0, G_MEAN_ROW = 1, G_MEAN_COL = 2 };

// One thread per (row, channel); the threads of a row read the same col[] words and consecutive channels of each
// neighbour row.  Sum in CSR order.
//   G_SYM:      out_r = w_r (sum_k w_c x_c + w_r x_r) + bias          (w = dis)
//   G_MEAN_ROW: out_r = w_r sum_k x_c                                  (w = inv_cnt, destination CSR)
//   G_MEAN_COL: out_r = sum_k w_c x_c                                  (w = inv_cnt, source CSR)
// EPI (G_SYM only): also y_r = [h_r +] gelu(out_r gate_r).
template <int D, int MODE, bool EPI>
__global__ void __launch_bounds__(TB) k_gather(int N, const float* __restrict__ x, const int32_t* __restrict__ row_ptr,
                                               const int32_t* __restrict__ col, const float* __restrict__ w,
                                               const float* __restrict__ bias, const float* __restrict__ gate,
                                               const float* __restrict__ h, float* __restrict__ out, float* __restrict__ y) {
    const int64_t total = (int64_t)N * D;
    for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total; t += (int64_t)gridDim.x * TB) {
        const int r = (int)(t / D), c = (int)(t % D);
        const int beg = row_ptr[r], end = row_ptr[r + 1];
        float acc = 0.0f;
        for (int k = beg; k < end; ++k) {
            const int s = col[k];
            const float v = x[(int64_t)s * D + c];
            acc += (MODE == G_MEAN_ROW) ? v : w[s] * v;
        }
        float o;
        if (MODE == G_SYM) {
            const float wr = w[r];
            o = wr * (acc + wr * x[t]);
            if (bias) o += bias[c];
        } else if (MODE == G_MEAN_ROW) {
            o = w[r] * acc;
        } else {
            o = acc;
        }
        out[t] = o;
        if (EPI) {
            const float a = ggc_geluf(o * gate[t]);
            y[t] = h ? h[t] + a : a;
        }
    }
}

template <int D>
__global__ void __launch_bounds__(TB) k_gcn_epi_bwd(int N, const float* __restrict__ g, const float* __restrict__ out,
                                                    const float* __restrict__ gate, float* __restrict__ g_out,
                                                    float* __restrict__ g_gate) {
    const int64_t total = (int64_t)N * D;
    for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total; t += (int64_t)gridDim.x * TB) {
        const float o = out[t], q = gate[t];
        const float tg = g[t] * gelu_grad(o * q);
        g_out[t] = tg * q;
        g_gate[t] = tg * o;
    }
}

// ctx_r = inv_cnt_r sum_{k in row r} enc[eid_k]   (C: any width)
__global__ void __launch_bounds__(TB) k_edge_mean(int N, int C, const float* __restrict__ enc, const int32_t* __restrict__ row_ptr,
                                                  const int32_t* __restrict__ eid, const float* __restrict__ inv_cnt,
                                                  float* __restrict__ out) {
    const int64_t total = (int64_t)N * C;
    for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total; t += (int64_t)gridDim.x * TB) {
        const int r = (int)(t / C), c = (int)(t % C);
        float acc = 0.0f;
        for (int k = row_ptr[r]; k < row_ptr[r + 1]; ++k) acc += enc[(int64_t)eid[k] * C + c];
        out[t] = inv_cnt[r] * acc;
    }
}

__global__ void __launch_bounds__(TB) k_edge_mean_bwd(int E, int C, const int32_t* __restrict__ dst, const float* __restrict__ inv_cnt,
                                                      const float* __restrict__ g_ctx, float* __restrict__ g_enc) {
    const int64_t total = (int64_t)E * C;
    for (int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x; t < total; t += (int64_t)gridDim.x * TB) {
        const int e = (int)(t / C), c = (int)(t % C);
        const int d = dst[e];
        g_enc[t] = inv_cnt[d] * g_ctx[(int64_t)d * C + c];
    }
}

// Fixed-order reduction of one value per thread over the workgroup (TB threads): butterflies inside each wave, then the
// four wave totals in order.  Every thread gets the result.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = MAX ? fmaxf(v, u) : v + u;
    }
    __syncthreads();                               // sh may still be read by the previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int i = 1; i < TB / 64; ++i) r = MAX ? fmaxf(r, sh[i]) : r + sh[i];
    return r;
}

// One workgroup per graph.  a_i = exp(s_i - max) / (sum exp + 1e-12) (reference _graph_softmax), pooled = sum a_i h_i,
// hb_i = pooled for every node of the graph.  P = TB / D partial sums per channel (node stride P), combined in order.
template <int D>
__global__ void __launch_bounds__(TB) k_pool(const int32_t* __restrict__ node_ptr, const float* __restrict__ h,
                                             const float* __restrict__ score, float* __restrict__ attn,
                                             float* __restrict__ hb) {
    constexpr int P = TB / D;
    static_assert(P >= 1, "a workgroup covers the row");
    __shared__ float red[TB / 64];
    __shared__ float part[P][D];
    __shared__ float pooled[D];
    const int n0 = node_ptr[blockIdx.x], n1 = node_ptr[blockIdx.x + 1];
    if (n1 <= n0) return;                          // uniform over the workgroup
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int i = n0 + tid; i < n1; i += TB) m = fmaxf(m, score[i]);
    m = block_reduce<true>(m, red);
    float s = 0.0f;
    for (int i = n0 + tid; i < n1; i += TB) s += expf(score[i] - m);
    s = block_reduce<false>(s, red) + 1e-12f;
    for (int i = n0 + tid; i < n1; i += TB) attn[i] = expf(score[i] - m) / s;
    __syncthreads();                               // attn of the whole graph visible to the workgroup
    const int p = tid / D, c = tid % D;
    if (p < P) {
        float acc = 0.0f;
        for (int i = n0 + p; i < n1; i += P) acc += attn[i] * h[(int64_t)i * D + c];
        part[p][c] = acc;
    }
    __syncthreads();
    if (tid < D) {
        float acc = part[0][tid];
        for (int q = 1; q < P; ++q) acc += part[q][tid];
        pooled[tid] = acc;
    }
    __syncthreads();
    const int64_t beg = (int64_t)n0 * D, end = (int64_t)n1 * D;
    for (int64_t t = beg + tid; t < end; t += TB) hb[t] = pooled[(int)(t % D)];
}

// Backward of k_pool.  gp = sum_i g_hb_i (per graph); g_h_i = a_i gp; ga_i = <gp, h_i>;
// g_score_i = a_i (ga_i - sum_j a_j ga_j)  (exact for the eps-shifted softmax as well).
// ga_i is staged in g_score; one wave per node for the dot product.
template <int D>
__global__ void __launch_bounds__(TB) k_pool_bwd(const int32_t* __restrict__ node_ptr, const float* __restrict__ h,
                                                 const float* __restrict__ attn, const float* __restrict__ g_hb,
                                                 float* __restrict__ g_h, float* __restrict__ g_score) {
    constexpr int P = TB / D, W = TB / 64;
    static_assert(P >= 1, "a workgroup covers the row");
    __shared__ float red[W];
    __shared__ float part[P][D];
    __shared__ float gp[D];
    const int n0 = node_ptr[blockIdx.x], n1 = node_ptr[blockIdx.x + 1];
    if (n1 <= n0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = tid / D, c = tid % D;
    if (p < P) {
        float acc = 0.0f;
        for (int i = n0 + p; i < n1; i += P) acc += g_hb[(int64_t)i * D + c];
        part[p][c] = acc;
    }
    __syncthreads();
    if (tid < D) {
        float acc = part[0][tid];
        for (int q = 1; q < P; ++q) acc += part[q][tid];
        gp[tid] = acc;
    }
    __syncthreads();
    for (int i = n0 + wave; i < n1; i += W) {
        const float a = attn[i];
        float dot = 0.0f;
        for (int k = lane; k < D; k += 64) {
            const float v = gp[k];
            dot += v * h[(int64_t)i * D + k];
            g_h[(int64_t)i * D + k] = a * v;
        }
        dot = wave_sum(dot);
        if (lane == 0) g_score[i] = dot;
    }
    __syncthreads();                               // ga of the whole graph visible to the workgroup
    float s = 0.0f;
    for (int i = n0 + tid; i < n1; i += TB) s += attn[i] * g_score[i];
    s = block_reduce<false>(s, red);
    for (int i = n0 + tid; i < n1; i += TB) g_score[i] = attn[i] * (g_score[i] - s);
}

static inline dim3 grid_for(int64_t total) {
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + TB - 1) / TB, 65536)));
}

template <int D, int MODE, bool EPI>
static int launch_gather(ggc_ctx* ctx, hipStream_t st, int N, const float* x, const int32_t* row_ptr, const int32_t* col,
                         const float* w, const float* bias, const float* gate, const float* h, float* out, float* y) {
    hipLaunchKernelGGL((k_gather<D, MODE, EPI>), grid_for((int64_t)N * D), dim3(TB), 0, st, N, x, row_ptr, col, w, bias,
                       gate, h, out, y);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

template <int MODE, bool EPI>
static int gather_any(ggc_ctx* ctx, hipStream_t st, int N, int D, const float* x, const int32_t* row_ptr, const int32_t* col,
                      const float* w, const float* bias, const float* gate, const float* h, float* out, float* y) {
    int rc;
    if (with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto d) {
            return launch_gather<decltype(d)::value, MODE, EPI>(ctx, st, N, x, row_ptr, col, w, bias, gate, h, out, y); }))
        return rc;
    return set_err(ctx, GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
}

static bool train_width(int D) { return D >= 32 && D <= 256 && D % 32 == 0; }

} // namespace ggc

using namespace ggc;

extern "C" {

int ggc_train_prepare(ggc_ctx* ctx, ggc_stream stream, int N, int E, const int32_t* edge_src, const int32_t* edge_dst,
                      int32_t* row_ptr, int32_t* col, int32_t* eid, int32_t* srow_ptr, int32_t* scol, int32_t* seid,
                      float* dis, float* inv_cnt) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && E >= 0 && row_ptr && srow_ptr && dis && inv_cnt &&
                (E == 0 || (edge_src && edge_dst && col && eid && scol && seid)), GGC_E_INVALID_ARG, "bad arguments");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_prepare");
    int32_t* cursor = scratch_t<int32_t>(ctx, S_CSR_CURSOR, (size_t)N + 1);
    if (!cursor) return GGC_E_OOM;
    int rc = build_csr(ctx, st, N, E, edge_src, edge_dst, row_ptr, col, eid, cursor, dis);
    if (rc != GGC_OK) return rc;
    rc = build_csr(ctx, st, N, E, edge_dst, edge_src, srow_ptr, scol, seid, cursor, nullptr);
    if (rc != GGC_OK) return rc;
    hipLaunchKernelGGL(k_inv_cnt, dim3(cdiv(N, TB)), dim3(TB), 0, st, N, row_ptr, inv_cnt);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int ggc_train_gcn_forward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* xw, const int32_t* row_ptr,
                          const int32_t* col, const float* dis, const float* bias, const float* gate, const float* h,
                          float* out, float* y) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && xw && row_ptr && col && dis && bias && gate && out && y, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_gcn_forward");
    return gather_any<G_SYM, true>(ctx, st, N, D, xw, row_ptr, col, dis, bias, gate, h, out, y);
}

int ggc_train_gcn_backward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* g_y, const float* out,
                           const float* gate, const int32_t* srow_ptr, const int32_t* scol, const float* dis,
                           float* g_out, float* g_gate, float* g_xw) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && g_y && out && gate && srow_ptr && scol && dis && g_out && g_gate && g_xw, GGC_E_INVALID_ARG,
                "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_gcn_backward");
    const dim3 grid = grid_for((int64_t)N * D);
    int rc;
    with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto d) {       // train_width(D): one of them matches
        hipLaunchKernelGGL(k_gcn_epi_bwd<decltype(d)::value>, grid, dim3(TB), 0, st, N, g_y, out, gate, g_out, g_gate);
        return GGC_OK; });
    GGC_LAUNCH_CHECK(ctx);
    return gather_any<G_SYM, false>(ctx, st, N, D, g_out, srow_ptr, scol, dis, nullptr, nullptr, nullptr, g_xw, nullptr);
}

int ggc_train_sage_mean(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* x, const int32_t* row_ptr,
                        const int32_t* col, const float* inv_cnt, float* out) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && x && row_ptr && col && inv_cnt && out, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_sage_mean");
    return gather_any<G_MEAN_ROW, false>(ctx, st, N, D, x, row_ptr, col, inv_cnt, nullptr, nullptr, nullptr, out, nullptr);
}

int ggc_train_sage_mean_backward(ggc_ctx* ctx, ggc_stream stream, int N, int D, const float* g_m, const int32_t* srow_ptr,
                                 const int32_t* scol, const float* inv_cnt, float* g_x) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && g_m && srow_ptr && scol && inv_cnt && g_x, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_sage_mean");
    return gather_any<G_MEAN_COL, false>(ctx, st, N, D, g_m, srow_ptr, scol, inv_cnt, nullptr, nullptr, nullptr, g_x, nullptr);
}

int ggc_train_edge_mean(ggc_ctx* ctx, ggc_stream stream, int N, int C, const float* enc, const int32_t* row_ptr,
                        const int32_t* eid, const float* inv_cnt, float* out) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, N >= 1 && C >= 1 && row_ptr && inv_cnt && out, GGC_E_INVALID_ARG, "bad arguments");
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_edge_mean");
    hipLaunchKernelGGL(k_edge_mean, grid_for((int64_t)N * C), dim3(TB), 0, st, N, C, enc, row_ptr, eid, inv_cnt, out);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int ggc_train_edge_mean_backward(ggc_ctx* ctx, ggc_stream stream, int E, int C, const int32_t* edge_dst,
                                 const float* inv_cnt, const float* g_ctx, float* g_enc) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, E >= 0 && C >= 1 && (E == 0 || (edge_dst && inv_cnt && g_ctx && g_enc)), GGC_E_INVALID_ARG,
                "bad arguments");
    if (E == 0) return GGC_OK;
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_edge_mean");
    hipLaunchKernelGGL(k_edge_mean_bwd, grid_for((int64_t)E * C), dim3(TB), 0, st, E, C, edge_dst, inv_cnt, g_ctx, g_enc);
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int ggc_train_graph_pool(ggc_ctx* ctx, ggc_stream stream, int G, int N, int D, const int32_t* node_ptr, const float* h,
                         const float* score, float* attn, float* hb) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, G >= 1 && N >= 1 && node_ptr && h && score && attn && hb, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_graph_pool");
    int rc;
    with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto d) {
        hipLaunchKernelGGL(k_pool<decltype(d)::value>, dim3(G), dim3(TB), 0, st, node_ptr, h, score, attn, hb);
        return GGC_OK; });
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

int ggc_train_graph_pool_backward(ggc_ctx* ctx, ggc_stream stream, int G, int N, int D, const int32_t* node_ptr,
                                  const float* h, const float* attn, const float* g_hb, float* g_h, float* g_score) {
    if (!ctx) return GGC_E_INVALID_ARG;
    GGC_REQUIRE(ctx, G >= 1 && N >= 1 && node_ptr && h && attn && g_hb && g_h && g_score, GGC_E_INVALID_ARG, "bad arguments");
    GGC_REQUIRE(ctx, train_width(D), GGC_E_UNSUPPORTED, "D=%d unsupported in training (a multiple of 32 from 32 to 256)", D);
    GGC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ProfScope prof(ctx, st, "train_graph_pool");
    int rc;
    with_width<32, 64, 96, 128, 160, 192, 224, 256>(D, rc, [&](auto d) {
        hipLaunchKernelGGL(k_pool_bwd<decltype(d)::value>, dim3(G), dim3(TB), 0, st, node_ptr, h, attn, g_hb, g_h, g_score);
        return GGC_OK; });
    GGC_LAUNCH_CHECK(ctx);
    return GGC_OK;
}

} // extern "C"
